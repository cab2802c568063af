#!/usr/bin/env python
"""Times rm_fmfm_fwd / rm_fmfm_bwd (hipEvents, warm clocks, 50 timed launches, min / median / mean) for the three pair
weight types beside the comparator - the same arithmetic composed from torch ops in fp32 over the same E and weights:
the rows of every pair gathered ([P,B,D] twice), one batched matmul against the P matrices (an elementwise product for
"vector" / "scalar"), the product with the right rows summed to the logit, forward + autograd backward - alternating
the contenders in one process.  The matrix kernels are priced in flops (2 B P D^2 forward, three times that backward)
against the 157.3 TFLOP/s f32-MFMA peak, the vector and scalar kernels in algorithmic bytes (E in, logit out; E and g in,
d_rows out) against the 8 TB/s HBM spec.  Also FmFMEngine.fwd_bwd without a DNN and with deep_hidden_units=(400, 400).
    python tools/bench_fmfm.py [--json out.json] [--kernels-only | --step-only]
`--kernels-only` launches nothing but the fused kernels, `--step-only` nothing but the engine's step (the runs to put
under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import fmfm_ref as R
from tools._bench import PEAK_MFMA, alternate, criteo_like, hbm_gb_s_fields, main


def composed_logit(E, W, ftype, li, lj):
    """The contract as a user would compose it from torch ops: gather the pairs' rows, one batched matmul."""
    Et = E.transpose(0, 1)  # [F,B,D]
    Ei, Ej = Et[li], Et[lj]  # [P,B,D]
    if ftype == "matrix":
        return (torch.bmm(Ei, W) * Ej).sum(dim=(0, 2))
    if ftype == "vector":
        return (Ei * W.unsqueeze(1) * Ej).sum(dim=(0, 2))
    return ((Ei * Ej).sum(dim=2) * W.unsqueeze(1)).sum(dim=0)


def kernels(B, F, D, ftype, comparator=True):
    P = R.pairs(F)
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    E = r(B, F, D) * (P * D) ** -0.25
    W = r(*R.weight_shape(F, D, ftype))
    if ftype == "matrix":
        W = torch.eye(D, device="cuda") + 0.25 * W
    g = r(B)
    logit, d_rows, dW = torch.empty(B, device="cuda"), torch.empty(B, F, D, device="cuda"), torch.empty_like(W)
    ws = torch.empty(max(4, ops.fmfm_bwd_workspace(B, F, D, ftype)), device="cuda")
    fwd = lambda: ops.fmfm_fwd(E, W, ftype, logit)  # noqa: E731
    bwd = lambda: ops.fmfm_bwd(E, W, ftype, g, d_rows, dW, ws)  # noqa: E731
    fns = [fwd, bwd]
    if comparator:
        leaves = [t.clone().requires_grad_(True) for t in (E, W)]
        li, lj = (t.cuda() for t in R.pair_fields(F))

        def composed():
            for t in leaves:
                t.grad = None
            composed_logit(*leaves, ftype, li, lj).backward(g)

        fns.append(composed)
    ms = alternate(fns)
    rec = {"shape": dict(B=B, F=F, D=D, type=ftype, **{k: ops.fmfm_tile(F, D, ftype, k) for k in ops.FMFM_TILE}),
           "fwd_ms": ms[0], "bwd_ms": ms[1]}
    if ftype == "matrix":
        flops = 2.0 * B * P * D * D
        rec.update(fwd_gflop=round(flops / 1e9, 3), bwd_gflop=round(3 * flops / 1e9, 3),
                   fwd_tflop_s=round(flops / (ms[0]["median"] * 1e-3) / 1e12, 2),
                   bwd_tflop_s=round(3 * flops / (ms[1]["median"] * 1e-3) / 1e12, 2))
        rec.update(fwd_peak_share=round(rec["fwd_tflop_s"] * 1e12 / PEAK_MFMA, 4),
                   bwd_peak_share=round(rec["bwd_tflop_s"] * 1e12 / PEAK_MFMA, 4))
    else:
        hbm_fwd, hbm_bwd = 4.0 * (B * F * D + B + W.numel()), 4.0 * (2 * B * F * D + B + 2 * W.numel())
        rec.update(hbm_gb_s_fields(hbm_fwd, hbm_bwd, ms[0], ms[1], "peak_share"))
    if comparator:
        fused = ms[0]["median"] + ms[1]["median"]
        rec.update(composed_fwd_bwd_ms=ms[2], ratio_composed_over_fused=round(ms[2]["median"] / fused, 2))
        # the contenders compute the same thing (against float64: tests/test_gpu_fmfm.py)
        with torch.no_grad():
            want = composed_logit(E[:2048], W, ftype, li, lj)
        rec["max_abs_diff_vs_composed"] = float((logit[:2048] - want).abs().max())
        rec["max_abs_grad_diff_vs_composed"] = float((d_rows - leaves[0].grad).abs().max())
    return rec


def step(ftype, hidden, B=65536, F=26, D=16, Dn=13):
    """FmFMEngine.fwd_bwd, hashed ids over 26 x 40000 rows."""
    spec, idx, dense, y = criteo_like(B, F, Dn)
    e = eng.FmFMEngine(spec, D, dict(deep_hidden_units=tuple(hidden), field_interaction=ftype))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, y)], n=20, warm=3)[0]


if __name__ == "__main__":
    main(lambda comparator: [kernels(65536, 26, 16, t, comparator=comparator) for t in R.TYPES],
         lambda: {f"fmfm_{t}_{'x'.join(map(str, h)) or 'no_dnn'}_fwd_bwd_ms": step(t, h)
                  for t in R.TYPES for h in ((), (400, 400))})
