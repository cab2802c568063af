#!/usr/bin/env python
"""Times rm_cross_mix_fwd / rm_cross_mix_bwd (hipEvents, warm clocks, 50 timed launches, min / median / mean) beside
the comparator - the same arithmetic composed from torch ops in fp32 over the same t, s, C (tests/crossmix_ref.core_fwd:
tanh, a batched matmul, softmax, mul; forward + autograd backward: a, h, c, p and their gradients go through HBM) -
alternating the contenders in one process.  Algorithmic bytes per example: forward 4 (2 E r + E), backward
4 (2 E r + E) read + 4 (E r + E) written, against the 8 TB/s HBM spec.  Also DCNEngine.fwd_bwd for cross_type vector,
matrix and mix with deep_hidden_units (400, 400) in the same process.
    python tools/bench_crossmix.py [--json out.json] [--kernels-only | --step-only]
`--kernels-only` launches nothing but the fused kernels, `--step-only` nothing but the engine's steps (the runs to put
under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import crossmix_ref as R
from tools._bench import PEAK_HBM as PEAK, alternate, criteo_like, main


def kernels(B, E, r, comparator=True):
    """T | S and dT | dS as column ranges of one buffer each, as the engine lays them out."""
    W, N = E * r, E * r + E
    ld = (N + 3) // 4 * 4
    g0 = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    ts, dts = torch.zeros(B, ld, device="cuda"), torch.zeros(B, ld, device="cuda")
    ts[:, :W], ts[:, W:N] = rn(B, W), 2.0 * rn(B, E)
    T, S, dT, dS = ts[:, :W], ts[:, W:N], dts[:, :W], dts[:, W:N]
    C = rn(E, r, r) * (1.5 / r ** 0.5)
    M, dM, dC = torch.empty(B, W, device="cuda"), rn(B, W), torch.empty(E, r, r, device="cuda")
    ws = torch.empty(max(1, ops.cross_mix_bwd_workspace(B, E, r)), device="cuda")
    fns = [lambda: ops.cross_mix_fwd(T, S, C, M), lambda: ops.cross_mix_bwd(T, S, C, dM, dT, dS, dC, ws)]
    if comparator:
        leaves = [t.contiguous().requires_grad_(True) for t in (T, S, C)]

        def composed():
            for t in leaves:
                t.grad = None
            R.core_fwd(*leaves).backward(dM)

        fns.append(composed)
    ms = alternate(fns)
    hbm_fwd, hbm_bwd = 4 * B * (2 * W + E), 4 * B * (2 * W + E) + 4 * B * (W + E)
    rec = {"shape": dict(B=B, E=E, r=r, ld=ld), "fwd_ms": ms[0], "bwd_ms": ms[1],
           "fwd_hbm_gb": round(hbm_fwd / 1e9, 4), "bwd_hbm_gb": round(hbm_bwd / 1e9, 4),
           "fwd_gb_s": round(hbm_fwd / (ms[0]["median"] * 1e-3) / 1e9, 1),
           "bwd_gb_s": round(hbm_bwd / (ms[1]["median"] * 1e-3) / 1e9, 1),
           "fwd_peak_share": round(hbm_fwd / (ms[0]["median"] * 1e-3) / PEAK, 4),
           "bwd_peak_share": round(hbm_bwd / (ms[1]["median"] * 1e-3) / PEAK, 4)}
    if comparator:
        fused = ms[0]["median"] + ms[1]["median"]
        rec.update(composed_fwd_bwd_ms=ms[2], ratio_composed_over_fused=round(ms[2]["median"] / fused, 2))
        # the contenders compute the same thing (against float64: tests/test_gpu_cross_mix.py)
        with torch.no_grad():
            want = R.core_fwd(T[:4096].contiguous(), S[:4096].contiguous(), C)
        rec["max_abs_diff_vs_composed"] = float((M[:4096] - want).abs().max())
        rec["max_abs_grad_diff_vs_composed"] = float((dT - leaves[0].grad).abs().max())
        rec["max_abs_dC_diff_vs_composed"] = float((dC - leaves[2].grad).abs().max())
    return rec


def steps(B=65536, F=26, D=16, Dn=13, L=3, E=4, r=32, hidden=(400, 400)):
    """DCNEngine.fwd_bwd for the three cross types taking turns, hashed ids over 26 x 40000 rows."""
    spec, idx, dense, y = criteo_like(B, F, Dn)
    engines = {}
    for ct in ("vector", "matrix", "mix"):
        e = eng.DCNEngine(spec, D, dict(deep_hidden_units=tuple(hidden), cross_layer_num=L, cross_type=ct,
                                        cross_experts=E, cross_low_rank=r))
        eng.init_reference(e)
        engines[ct] = e
    ms = alternate([lambda e=e: e.fwd_bwd(idx, dense, y) for e in engines.values()], n=30, warm=3)
    return {f"dcn_{ct}_fwd_bwd_ms": m for ct, m in zip(engines, ms)}


def all_kernels(comparator):
    out = [kernels(65536, 4, 32, comparator=comparator)]
    if comparator:
        out += [kernels(65536, 8, 32, comparator=False), kernels(65536, 4, 64, comparator=False),
                kernels(65536, 3, 8, comparator=False)]
    return out


if __name__ == "__main__":
    main(all_kernels, steps)
