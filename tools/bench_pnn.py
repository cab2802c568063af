#!/usr/bin/env python
"""Times rm_pnn_fwd / rm_pnn_bwd (hipEvents, warm clocks, 50 timed launches, min / median / mean) for inner only, outer
only for each kernel type and inner + mat, beside the comparator - the same arithmetic composed from torch ops in fp32
over the same E and kernels: the rows of every pair gathered ([P,B,D] twice), one batched matmul against the P matrices
(an elementwise product for "vec" / "num"), the product with the right rows summed over d, the blocks concatenated behind
the flattened rows, forward + autograd backward - and, for the "mat" kernels, beside rm_fmfm_fwd / rm_fmfm_bwd (matrix)
on the same E and matrices: the difference is the price of the P-wide output and of the per-pair gradient.  All
contenders alternate in one process.  The mat kernels are priced in flops (2 B P D^2 forward, three times that
backward) against the 157.3 TFLOP/s f32-MFMA peak (the forward runs on the f64 MFMA: its share of that figure is
there to compare with FmFM's, it is no roofline of its own), the others in algorithmic bytes (E in, X out; E and dX
in, d_rows out) against the 8 TB/s HBM spec.  Also PNNEngine.fwd_bwd with deep_hidden_units=(400, 400).
    python tools/bench_pnn.py [--json out.json] [--kernels-only | --step-only]
`--kernels-only` launches nothing but the fused kernels, `--step-only` nothing but the engine's step (the runs to put
under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import pnn_ref as R
from tools._bench import PEAK_MFMA, alternate, criteo_like, hbm_gb_s_fields, main


def composed_layer(E, K, products, kt, li, lj):
    """The contract as a user would compose it from torch ops: gather the pairs' rows, one batched matmul."""
    Et = E.transpose(0, 1)  # [F,B,D]
    Ei, Ej = Et[li], Et[lj]  # [P,B,D]
    blocks = [E.reshape(E.shape[0], -1)]
    if products & R.INNER:
        blocks.append((Ei * Ej).sum(dim=2).t())
    if products & R.OUTER:
        if kt == "mat":
            blocks.append((torch.bmm(Ei, K) * Ej).sum(dim=2).t())
        elif kt == "vec":
            blocks.append((Ei * K.unsqueeze(1) * Ej).sum(dim=2).t())
        else:
            blocks.append(((Ei * Ej).sum(dim=2) * K.unsqueeze(1)).t())
    return torch.cat(blocks, dim=1)


def kernels(B, F, D, products, kt, comparator=True):
    P = R.pairs(F)
    outer = bool(products & R.OUTER)
    mat = outer and kt == "mat"
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    E = r(B, F, D) * D ** -0.25
    K = None
    if outer:
        K = r(*R.weight_shape(F, D, kt))
        if mat:
            K = torch.eye(D, device="cuda") + 0.25 * K
    W, ldx = ops.pnn_width(F, D, products)
    Xb, dXb = torch.zeros(B, ldx, device="cuda"), torch.zeros(B, ldx, device="cuda")
    X, dX = Xb[:, :W], dXb[:, :W]
    dX.copy_(r(B, W))
    d_rows = torch.empty(B, F, D, device="cuda")
    dK = torch.empty_like(K) if outer else None
    ws = torch.empty(max(4, ops.pnn_bwd_workspace(B, F, D, products, kt)), device="cuda") if outer else None
    fns = [lambda: ops.pnn_fwd(E, K, products, kt, X), lambda: ops.pnn_bwd(E, K, products, kt, dX, d_rows, dK, ws)]
    names = ["fwd_ms", "bwd_ms"]
    if mat:  # rm_fmfm_fwd / rm_fmfm_bwd on the same E and matrices: one logit out, one scalar per example in
        logit, g = torch.empty(B, device="cuda"), r(B)
        fr, fdw = torch.empty(B, F, D, device="cuda"), torch.empty_like(K)
        fws = torch.empty(max(4, ops.fmfm_bwd_workspace(B, F, D, "matrix")), device="cuda")
        fns += [lambda: ops.fmfm_fwd(E, K, "matrix", logit), lambda: ops.fmfm_bwd(E, K, "matrix", g, fr, fdw, fws)]
        names += ["fmfm_fwd_ms", "fmfm_bwd_ms"]
    if comparator:
        leaves = [E.clone().requires_grad_(True)] + ([K.clone().requires_grad_(True)] if outer else [None])
        li, lj = (t.cuda() for t in R.pair_fields(F))
        dXc = dX.contiguous()

        def composed():
            for t in leaves:
                if t is not None:
                    t.grad = None
            composed_layer(*leaves, products, kt, li, lj).backward(dXc)

        fns.append(composed)
        names.append("composed_fwd_bwd_ms")
    ms = dict(zip(names, alternate(fns)))
    rec = {"shape": dict(B=B, F=F, D=D, products=products, kernel_type=kt, W=W, ldx=ldx,
                         **{k: ops.pnn_tile(F, D, products, kt, k) for k in ops.PNN_TILE})}
    rec.update(ms)
    f_ms, b_ms = ms["fwd_ms"]["median"] * 1e-3, ms["bwd_ms"]["median"] * 1e-3
    nk = K.numel() if outer else 0
    hbm_fwd, hbm_bwd = 4.0 * (B * F * D + B * ldx + nk), 4.0 * (2 * B * F * D + B * ldx + 2 * nk)
    rec.update(hbm_gb_s_fields(hbm_fwd, hbm_bwd, ms["fwd_ms"], ms["bwd_ms"], "hbm_share"))
    if mat:
        flops = 2.0 * B * P * D * D
        rec.update(fwd_gflop=round(flops / 1e9, 3), bwd_gflop=round(3 * flops / 1e9, 3),
                   fwd_tflop_s=round(flops / f_ms / 1e12, 2), bwd_tflop_s=round(3 * flops / b_ms / 1e12, 2))
        rec.update(fwd_mfma_share=round(rec["fwd_tflop_s"] * 1e12 / PEAK_MFMA, 4),
                   bwd_mfma_share=round(rec["bwd_tflop_s"] * 1e12 / PEAK_MFMA, 4),
                   ratio_fwd_over_fmfm=round(ms["fwd_ms"]["median"] / ms["fmfm_fwd_ms"]["median"], 2),
                   ratio_bwd_over_fmfm=round(ms["bwd_ms"]["median"] / ms["fmfm_bwd_ms"]["median"], 2))
    if comparator:
        fused = ms["fwd_ms"]["median"] + ms["bwd_ms"]["median"]
        rec["ratio_composed_over_fused"] = round(ms["composed_fwd_bwd_ms"]["median"] / fused, 2)
        # the contenders compute the same thing (against float64: tests/test_gpu_pnn.py)
        with torch.no_grad():
            want = composed_layer(E[:2048], K, products, kt, li, lj)
        rec["max_abs_diff_vs_composed"] = float((X[:2048] - want).abs().max())
        rec["max_abs_grad_diff_vs_composed"] = float((d_rows - leaves[0].grad).abs().max())
    return rec


def step(products, kt, hidden=(400, 400), B=65536, F=26, D=16, Dn=13):
    """PNNEngine.fwd_bwd, hashed ids over 26 x 40000 rows."""
    spec, idx, dense, y = criteo_like(B, F, Dn)
    e = eng.PNNEngine(spec, D, dict(deep_hidden_units=tuple(hidden), use_inner=bool(products & R.INNER),
                                    use_outer=bool(products & R.OUTER), kernel_type=kt))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, y)], n=20, warm=3)[0]


def tag(products, kt):
    return {1: "inner", 2: f"outer_{kt}", 3: f"inner_outer_{kt}"}[products]


if __name__ == "__main__":
    main(lambda comparator: [kernels(65536, 26, 16, pr, kt, comparator=comparator) for pr, kt in R.COMBOS],
         lambda: {f"pnn_{tag(pr, kt)}_400x400_fwd_bwd_ms": step(pr, kt) for pr, kt in R.COMBOS})
