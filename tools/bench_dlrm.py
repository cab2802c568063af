#!/usr/bin/env python
"""Times rm_dot_interact_fwd / rm_dot_interact_bwd (hipEvents, warm clocks, 50 timed launches, min / median / mean)
beside the comparator - the same arithmetic composed from torch ops in fp32 over the same E and z
(tests/dlrm_ref.interact: cat + bmm + triangular gather, forward + autograd backward: the [B,T,T] Gram matrix and the
concatenated input go through HBM) - alternating the contenders in one process.  Algorithmic bytes per example:
forward 4 (F D + D + ldx), backward 4 (2 F D + 2 D + ldx), against the 8 TB/s HBM spec.  Also DLRMEngine.fwd_bwd with
bottom_hidden_units=(512, 256) and deep_hidden_units=(512, 256).
    python tools/bench_dlrm.py [--json out.json] [--kernels-only | --step-only]
`--kernels-only` launches nothing but the fused kernels, `--step-only` nothing but the engine's step (the runs to put
under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import dlrm_ref as R
from tools._bench import alternate, criteo_like, hbm_fields, main


def kernels(B, F, D, comparator=True):
    W, ldx = ops.dot_interact_width(F, D)
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    E, z = r(B, F, D) * 0.3, r(B, D)
    Xb, dXb = torch.empty(B, ldx, device="cuda"), torch.zeros(B, ldx, device="cuda")
    dXb[:, :W] = r(B, W)
    X, dX = Xb[:, :W], dXb[:, :W]
    d_rows, dz = torch.empty(B, F, D, device="cuda"), torch.empty(B, D, device="cuda")
    fwd = lambda: ops.dot_interact_fwd(E, z, X)  # noqa: E731
    bwd = lambda: ops.dot_interact_bwd(E, z, dX, d_rows, dz)  # noqa: E731
    fns = [fwd, bwd]
    if comparator:
        leaves = [t.clone().requires_grad_(True) for t in (E, z)]
        dXc = dX.contiguous()

        def composed():
            for t in leaves:
                t.grad = None
            R.interact(*leaves).backward(dXc)

        fns.append(composed)
    ms = alternate(fns)
    hbm_fwd, hbm_bwd = 4 * B * (F * D + D + ldx), 4 * B * (2 * F * D + 2 * D + ldx)
    rec = {"shape": dict(B=B, F=F, D=D, ldx=ldx), "fwd_ms": ms[0], "bwd_ms": ms[1],
           **hbm_fields(hbm_fwd, hbm_bwd, ms[0], ms[1])}
    if comparator:
        fused = ms[0]["median"] + ms[1]["median"]
        rec.update(composed_fwd_bwd_ms=ms[2], ratio_composed_over_fused=round(ms[2]["median"] / fused, 2))
        # the contenders compute the same thing (against float64: tests/test_gpu_dot_interact.py)
        with torch.no_grad():
            want = R.interact(E[:4096], z[:4096])
        rec["max_abs_diff_vs_composed"] = float((X[:4096] - want).abs().max())
        rec["max_abs_grad_diff_vs_composed"] = float((d_rows - leaves[0].grad).abs().max())
    return rec


def step(B=65536, F=26, D=16, Dn=13, bottom=(512, 256), hidden=(512, 256)):
    """DLRMEngine.fwd_bwd, hashed ids over 26 x 40000 rows."""
    spec, idx, dense, y = criteo_like(B, F, Dn)
    e = eng.DLRMEngine(spec, D, dict(bottom_hidden_units=tuple(bottom), deep_hidden_units=tuple(hidden)))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, y)])[0]


def all_kernels(comparator):
    out = [kernels(65536, 26, 16, comparator=comparator)]
    if comparator:
        out += [kernels(65536, 40, 64, comparator=False), kernels(65536, 7, 16, comparator=False)]
    return out


if __name__ == "__main__":
    main(all_kernels, lambda: {"dlrm_512x256_512x256_fwd_bwd_ms": step()})
