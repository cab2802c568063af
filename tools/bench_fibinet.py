#!/usr/bin/env python
"""Times rm_fibinet_fwd / rm_fibinet_bwd (hipEvents, warm clocks, 50 timed launches, min / median / mean) beside the
comparator - the same arithmetic composed from torch ops in fp32 over the same E and weights (the gate as two small
matmuls, per branch one batched left product, two gathers of [B,P,D] and their product, forward + autograd backward) -
alternating the contenders in one process, for bilinear_type "each" and "all".  Algorithmic bytes per example: forward
4 (F D + ldx), backward 4 (2 F D + ldx) (a is recomputed, not stored), against the 8 TB/s HBM spec.  Also
FiBiNETEngine.fwd_bwd with deep_hidden_units=(400, 400).
    python tools/bench_fibinet.py [--json out.json] [--kernels-only | --step-only]
`--kernels-only` launches nothing but the fused kernels, `--step-only` nothing but the engine's step (the runs to put
under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import fibinet_ref as R
from tools._bench import alternate, criteo_like, hbm_fields, main


def composed_interact(E, W1, W2, Wb, Wsb, btype, li, lj):
    """The contract as a user would compose it from torch ops (tests/fibinet_ref.interact forms one matrix per pair,
    which nobody would run at this size)."""
    B = E.shape[0]
    a = torch.relu(torch.relu(E.mean(dim=2) @ W1) @ W2)
    V = a.unsqueeze(2) * E

    def bilinear(Y, W):
        U = Y @ W[0] if btype == "all" else torch.einsum("bfk,fkd->bfd", Y[:, :-1], W)
        return (U[:, li] * Y[:, lj]).reshape(B, -1)

    return torch.cat([bilinear(E, Wb), bilinear(V, Wsb)], dim=1)


def kernels(B, F, D, Rr, btype, comparator=True):
    W, ldx = ops.fibinet_width(F, D)
    nW = R.n_matrices(F, btype)
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    E = r(B, F, D) * 0.3
    W1, W2 = r(F, Rr) * (2.0 / (F + Rr)) ** 0.5, r(Rr, F) * (2.0 / (F + Rr)) ** 0.5
    Wb, Wsb = r(nW, D, D) * D ** -0.5, r(nW, D, D) * D ** -0.5
    Xb, dXb = torch.empty(B, ldx, device="cuda"), torch.zeros(B, ldx, device="cuda")
    dXb[:, :W] = r(B, W)
    X, dX = Xb[:, :W], dXb[:, :W]
    dE = torch.empty(B, F, D, device="cuda")
    dws = [torch.empty_like(t) for t in (W1, W2, Wb, Wsb)]
    ws = torch.empty(max(4, ops.fibinet_bwd_workspace(B, F, D, Rr, btype)), device="cuda")
    fwd = lambda: ops.fibinet_fwd(E, W1, W2, Wb, Wsb, btype, X)  # noqa: E731
    bwd = lambda: ops.fibinet_bwd(E, W1, W2, Wb, Wsb, btype, dX, dE, *dws, ws)  # noqa: E731
    fns = [fwd, bwd]
    if comparator:
        leaves = [t.clone().requires_grad_(True) for t in (E, W1, W2, Wb, Wsb)]
        li, lj = (t.cuda() for t in R.pair_fields(F))
        dXc = dX.contiguous()

        def composed():
            for t in leaves:
                t.grad = None
            composed_interact(*leaves, btype, li, lj).backward(dXc)

        fns.append(composed)
    ms = alternate(fns)
    hbm_fwd, hbm_bwd = 4 * B * (F * D + ldx), 4 * B * (2 * F * D + ldx)
    rec = {"shape": dict(B=B, F=F, D=D, R=Rr, type=btype, ldx=ldx,
                         tile_fwd=ops.fibinet_tile(F, D, Rr, btype), tile_bwd=ops.fibinet_tile(F, D, Rr, btype, True)),
           "fwd_ms": ms[0], "bwd_ms": ms[1], **hbm_fields(hbm_fwd, hbm_bwd, ms[0], ms[1])}
    if comparator:
        fused = ms[0]["median"] + ms[1]["median"]
        rec.update(composed_fwd_bwd_ms=ms[2], ratio_composed_over_fused=round(ms[2]["median"] / fused, 2))
        # the contenders compute the same thing (against float64: tests/test_gpu_fibinet.py)
        with torch.no_grad():
            want = composed_interact(E[:2048], W1, W2, Wb, Wsb, btype, li, lj)
        rec["max_abs_diff_vs_composed"] = float((X[:2048] - want).abs().max())
        rec["max_abs_grad_diff_vs_composed"] = float((dE - leaves[0].grad).abs().max())
    return rec


def step(btype, B=65536, F=26, D=16, Dn=13, hidden=(400, 400)):
    """FiBiNETEngine.fwd_bwd, hashed ids over 26 x 40000 rows."""
    spec, idx, dense, y = criteo_like(B, F, Dn)
    e = eng.FiBiNETEngine(spec, D, dict(deep_hidden_units=tuple(hidden), bilinear_type=btype))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, y)], n=20, warm=3)[0]


if __name__ == "__main__":
    main(lambda comparator: [kernels(65536, 26, 16, 8, t, comparator=comparator) for t in ("each", "all")],
         lambda: {f"fibinet_{t}_400x400_fwd_bwd_ms": step(t) for t in ("each", "all")})
