#!/usr/bin/env python
"""Times rm_afm_fwd / rm_afm_bwd (hipEvents, warm-up, 20 timed launches) beside the comparator - the same arithmetic
composed from torch ops in fp32 over the same E (tests/afm_ref.afm_layer, forward + autograd backward; it materialises
the [B, P, D] pair tensor), whole-batch and in pieces of 4096 examples - alternating the contenders in one process.
Flops per kernel: AFMEngine.afm_flops (per pair D + 2 D T + 2 T + 2 D forward; the backward recomputes that and adds
2 (2 D T) + 4 D), priced against the 157.3 TFLOP/s fp32 peak.  Also an AFMEngine.fwd_bwd step beside a DeepFM step at
the same shape.  python tools/bench_afm.py [--json out.json]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import afm_ref as R
from tools._bench import PEAK_MFMA as PEAK, criteo_like, emit, medians


def kernels(B, F, D, T, comparator=True):
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    E, W, b, h, p, g = r(B, F, D) * 0.3, r(D, T) * (2 / (D + T)) ** 0.5, r(T) * 0.1, r(T) * 0.5, r(D) * 0.3, r(B)
    logit, st = torch.empty(B, device="cuda"), torch.empty(B, D + 2, device="cuda")
    d_rows = torch.empty(B, F, D, device="cuda")
    dW, db, dh, dp = (torch.empty(s, device="cuda") for s in ((D, T), (T,), (T,), (D,)))
    ws = torch.empty(ops.afm_bwd_workspace(B, F, D, T), device="cuda")
    fwd = lambda: ops.afm_fwd(E, W, b, h, p, logit, stats=st)  # noqa: E731
    inf = lambda: ops.afm_fwd(E, W, b, h, p, logit)  # noqa: E731
    bwd = lambda: ops.afm_bwd(E, W, b, h, p, g, logit, st, d_rows, dW, db, dh, dp, ws)  # noqa: E731
    fns = [fwd, inf, bwd]
    if comparator:
        leaves = [t.clone().requires_grad_(True) for t in (E, W, b, h, p)]

        def composed(rows=None):
            for t in leaves:
                t.grad = None
            if rows is None:
                y = R.afm_layer(*leaves)
            else:
                y = torch.cat([R.afm_layer(leaves[0][s:s + rows], *leaves[1:]) for s in range(0, B, rows)])
            y.backward(g)

        fns += [composed, lambda: composed(4096)]
    ms = medians(fns, 20, 3)
    f_fwd, f_bwd = eng.AFMEngine.afm_flops(B, F, D, T)
    rec = {"shape": dict(B=B, F=F, D=D, T=T), "afm_fwd_ms": round(ms[0], 4), "afm_fwd_inference_ms": round(ms[1], 4),
           "afm_bwd_ms": round(ms[2], 4), "fwd_tflops": round(f_fwd / ms[0] / 1e9, 2),
           "bwd_tflops": round(f_bwd / ms[2] / 1e9, 2), "fwd_peak_share": round(f_fwd / (ms[0] * 1e-3) / PEAK, 4),
           "bwd_peak_share": round(f_bwd / (ms[2] * 1e-3) / PEAK, 4)}
    if comparator:
        fused = ms[0] + ms[2]
        rec.update(composed_fwd_bwd_ms=round(ms[3], 3), composed_in_pieces_fwd_bwd_ms=round(ms[4], 3),
                   ratio_composed_over_fused=round(ms[3] / fused, 2),
                   ratio_composed_in_pieces_over_fused=round(ms[4] / fused, 2))
    return rec


def steps(B=65536, F=26, D=16, Dn=13):
    """An AFMEngine.fwd_bwd step beside a DeepFM step at the same shape (hashed ids over 26 x 40000 rows)."""
    out = {}
    spec, idx, dense, y = criteo_like(B, F, Dn)
    for name, hp in (("afm", dict(att_factor=8)), ("deepfm", dict(deep_hidden_units=(32, 32)))):
        e = eng.ENGINES[name](spec, D, hp)
        eng.init_reference(e)
        out[name + "_fwd_bwd_ms"] = round(medians([lambda: e.fwd_bwd(idx, dense, y)], 20, 3)[0], 4)
        del e
    return out


if __name__ == "__main__":
    emit({"kernels": [kernels(65536, 26, 16, 8), kernels(65536, 26, 16, 32),
                      kernels(8192, 40, 64, 64, comparator=False)], "steps": steps()})
