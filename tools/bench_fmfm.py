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
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import fmfm_ref as R

PEAK_HBM, PEAK_MFMA = 8.0e12, 157.3e12


def stats(ts):
    ts = sorted(ts)
    return dict(min=round(ts[0], 4), median=round(ts[len(ts) // 2], 4), mean=round(sum(ts) / len(ts), 4))


def alternate(fns, n=50, warm=5):
    """min / median / mean ms per contender, the contenders taking turns (warm-up rounds first: clocks and caches)."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(n):
        for fn, acc in zip(fns, ts):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            acc.append(a.elapsed_time(z))
    return [stats(t) for t in ts]


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
        rec.update(fwd_hbm_gb=round(hbm_fwd / 1e9, 4), bwd_hbm_gb=round(hbm_bwd / 1e9, 4),
                   fwd_gb_s=round(hbm_fwd / (ms[0]["median"] * 1e-3) / 1e9, 1),
                   bwd_gb_s=round(hbm_bwd / (ms[1]["median"] * 1e-3) / 1e9, 1))
        rec.update(fwd_peak_share=round(rec["fwd_gb_s"] * 1e9 / PEAK_HBM, 4),
                   bwd_peak_share=round(rec["bwd_gb_s"] * 1e9 / PEAK_HBM, 4))
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
    g = torch.Generator().manual_seed(0)
    sizes = [40000] * F
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in sizes], 1).cuda()
    dense, y = torch.randn(B, Dn, generator=g).cuda(), (torch.rand(B, generator=g) < 0.3).long().cuda()
    spec = eng.FeatureSpec([f"C{i}" for i in range(F)], sizes, [f"I{j}" for j in range(Dn)])
    e = eng.FmFMEngine(spec, D, dict(deep_hidden_units=tuple(hidden), field_interaction=ftype))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, y)], n=20, warm=3)[0]


if __name__ == "__main__":
    only, step_only = "--kernels-only" in sys.argv, "--step-only" in sys.argv
    res = {}
    if not step_only:
        res["kernels"] = [kernels(65536, 26, 16, t, comparator=not only) for t in R.TYPES]
    if not only:
        res["steps"] = {f"fmfm_{t}_{'x'.join(map(str, h)) or 'no_dnn'}_fwd_bwd_ms": step(t, h)
                        for t in R.TYPES for h in ((), (400, 400))}
    for k in res.get("kernels", ()):
        print(json.dumps(k), flush=True)
    if "steps" in res:
        print(json.dumps(res["steps"]), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)
