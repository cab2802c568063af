#!/usr/bin/env python
"""Times rm_autoint_layer_fwd / rm_autoint_layer_bwd (hipEvents, warm clocks, 50 timed launches, min / median / mean)
beside the comparator - the same arithmetic composed from torch ops in fp32 over the same X
(tests/autoint_ref.interacting_layer, forward + autograd backward: Q, K, V, the [B,H,F,F] scores and the weights go
through HBM) - alternating the contenders in one process.  Flops per layer: AutoIntEngine.autoint_flops (8 F Din HD
for the four projections + 4 F^2 HD for scores and weighted sums per example; the backward is priced at three
forwards), against the 157.3 TFLOP/s f32 matrix peak.  Also the three-layer default model's AutoIntEngine.fwd_bwd step.
    python tools/bench_autoint.py [--json out.json] [--kernels-only]
`--kernels-only` launches nothing but the fused kernels (the run to put under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import autoint_ref as R
from tools._bench import PEAK_MFMA as PEAK, alternate, criteo_like, hbm_fields, main


def kernels(B, F, Din, H, dk, comparator=True):
    HD = H * dk
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    X, dY = r(B, F, Din) * 0.3, r(B, F, HD)
    W = [r(Din, HD) * (2 / (Din + HD)) ** 0.5 for _ in range(4)]
    Y, st = torch.empty(B, F, HD, device="cuda"), torch.empty(B, H, F, 2, device="cuda")
    dX, dW = torch.empty(B, F, Din, device="cuda"), [torch.empty(Din, HD, device="cuda") for _ in range(4)]
    ws = torch.empty(ops.autoint_layer_bwd_workspace(B, F, Din, H, dk), device="cuda")
    fwd = lambda: ops.autoint_layer_fwd(X, *W, H, 1.0, Y, stats=st)  # noqa: E731
    bwd = lambda: ops.autoint_layer_bwd(X, *W, Y, st, dY, H, 1.0, dX, *dW, ws)  # noqa: E731
    fns = [fwd, bwd]
    if comparator:
        leaves = [t.clone().requires_grad_(True) for t in [X] + W]

        def composed():
            for t in leaves:
                t.grad = None
            R.interacting_layer(*leaves, H).backward(dY)

        fns.append(composed)
    ms = alternate(fns)
    f_fwd, f_bwd = eng.AutoIntEngine.autoint_flops(B, F, Din, HD)
    hbm_fwd = 4 * B * F * (Din + HD + 2 * H)            # X in, Y and the softmax record out
    hbm_bwd = 4 * B * F * (Din + 2 * HD + 2 * H + Din)  # X, Y, dY, the record in; dX out
    rec = {"shape": dict(B=B, F=F, Din=Din, H=H, dk=dk), "fwd_ms": ms[0], "bwd_ms": ms[1],
           "fwd_tflops": round(f_fwd / ms[0]["median"] / 1e9, 2), "bwd_tflops": round(f_bwd / ms[1]["median"] / 1e9, 2),
           "fwd_peak_share": round(f_fwd / (ms[0]["median"] * 1e-3) / PEAK, 4),
           "bwd_peak_share": round(f_bwd / (ms[1]["median"] * 1e-3) / PEAK, 4),
           **hbm_fields(hbm_fwd, hbm_bwd, ms[0], ms[1], peak_share=False)}
    if comparator:
        fused = ms[0]["median"] + ms[1]["median"]
        rec.update(composed_fwd_bwd_ms=ms[2], ratio_composed_over_fused=round(ms[2]["median"] / fused, 2))
    return rec


def step(B=65536, F=26, D=16, Dn=13, hidden=()):
    """AutoIntEngine.fwd_bwd, the default model (three layers, two heads of 8, residual), hashed ids over 26 x 40000
    rows; with `hidden` the AutoInt+ variant."""
    spec, idx, dense, y = criteo_like(B, F, Dn)
    e = eng.AutoIntEngine(spec, D, dict(deep_hidden_units=tuple(hidden)))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, y)])[0]


def all_kernels(comparator):
    out = [kernels(65536, 26, 16, 2, 8, comparator=comparator)]
    if comparator:
        out += [kernels(65536, 26, 16, 2, 16), kernels(8192, 40, 64, 8, 8, comparator=False)]
    return out


if __name__ == "__main__":
    main(all_kernels, lambda: {"autoint_fwd_bwd_ms": step(), "autoint_plus_32x32_fwd_bwd_ms": step(hidden=(32, 32))})
