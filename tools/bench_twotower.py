#!/usr/bin/env python
"""Times rm_inbatch_softmax_fwd / rm_inbatch_softmax_bwd (hipEvents, warm clocks, 50 timed launches, min / median /
mean) beside the comparator - the same arithmetic composed from torch ops in fp32 over the same U, V, ids, logq and w:
`U @ V.T`, a masked log_softmax, the weighted mean, forward alone and forward + autograd backward, at the sizes where
the [B, B] score matrix and its autograd copies fit - and TwoTowerEngine.fwd_bwd, the full model step.  All contenders of a
shape alternate in one process.  The kernels are priced in FLOP, 2 B^2 H forward and 8 B^2 H backward (two
recomputations of the scores and two products), against the 157.3 TFLOP/s f32-MFMA peak.
    python tools/bench_twotower.py [--json out.json] [--kernels-only | --step-only]
Shapes: H = 64 and 128 at B = 4096, 8192 and 32768; the step with the default towers (256, 128) at F = 26 (13 user and
13 item features), D = 16, 13 dense features, B = 8192.  `--kernels-only` launches nothing but the fused kernels,
`--step-only` nothing but the engine's step (the runs to put under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tools._bench import PEAK_MFMA as PEAK_F32_MFMA, alternate, hashed_batch, main

SHAPES = [(B, H) for H in (64, 128) for B in (4096, 8192, 32768)]
COMPOSED_MAX_B = 32768  # beyond it each of the composition's [B, B] matrices (4 B^2 bytes) passes 17 GB
STEP = dict(B=8192, F=26, D=16, Dn=13, towers=(256, 128))
SCALE = 20.0


def composed_loss(U, V, ids, logq, w):
    """The contract as a user would compose it from torch ops."""
    S = SCALE * (U @ V.t()) - logq.unsqueeze(0)
    hit = (ids.unsqueeze(0) == ids.unsqueeze(1)) & ~torch.eye(U.shape[0], dtype=torch.bool, device=U.device)
    lp = torch.log_softmax(S.masked_fill(hit, float("-inf")), dim=1)
    return -(w * lp.diagonal()).sum() / w.sum()


def kernels(B, H, comparator=True):
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    U, V = torch.nn.functional.normalize(r(B, H)), torch.nn.functional.normalize(r(B, H))
    ids = torch.randint(0, max(1, B // 3), (B,), device="cuda", generator=g0)
    logq = -6.0 * torch.rand(B, device="cuda", generator=g0)
    w = (torch.rand(B, device="cuda", generator=g0) >= 0.25).float()
    lse, row_loss, loss = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
    rank = torch.empty(B, dtype=torch.int32, device="cuda")
    dU, dV = torch.empty(B, H, device="cuda"), torch.empty(B, H, device="cuda")
    ws = torch.empty(ops.inbatch_softmax_workspace(B, H), device="cuda")
    kw = dict(item_id=ids, logq=logq, w=w)
    fns = [lambda: ops.inbatch_softmax_fwd(U, V, SCALE, lse, row_loss, loss, ws, rank=rank, **kw),
           lambda: ops.inbatch_softmax_bwd(U, V, SCALE, lse, dU, dV, ws, **kw)]
    names = ["fwd_ms", "bwd_ms"]
    comparator = comparator and B <= COMPOSED_MAX_B
    if comparator:
        Ul, Vl = U.clone().requires_grad_(True), V.clone().requires_grad_(True)

        def composed_fwd():
            with torch.no_grad():
                composed_loss(U, V, ids, logq, w)

        def composed():
            Ul.grad = Vl.grad = None
            composed_loss(Ul, Vl, ids, logq, w).backward()

        fns += [composed_fwd, composed]
        names += ["composed_fwd_ms", "composed_fwd_bwd_ms"]
    ms = dict(zip(names, alternate(fns)))
    rec = {"shape": dict(B=B, H=H, rows=ops.inbatch_softmax_tile(H), cols=ops.inbatch_softmax_tile(H, "cols")),
           "score_matrix_mb": round(4.0 * B * B / 1e6, 1)}
    rec.update(ms)
    f_s, b_s = ms["fwd_ms"]["median"] * 1e-3, ms["bwd_ms"]["median"] * 1e-3
    rec.update(fwd_tflops=round(2.0 * B * B * H / f_s / 1e12, 2), bwd_tflops=round(8.0 * B * B * H / b_s / 1e12, 2))
    rec.update(fwd_peak_share=round(rec["fwd_tflops"] * 1e12 / PEAK_F32_MFMA, 4),
               bwd_peak_share=round(rec["bwd_tflops"] * 1e12 / PEAK_F32_MFMA, 4),
               floor_ms_at_peak=round(10.0 * B * B * H / PEAK_F32_MFMA * 1e3, 4))
    if comparator:
        fused = ms["fwd_ms"]["median"] + ms["bwd_ms"]["median"]
        rec["ratio_composed_fwd_over_fused_fwd"] = round(ms["composed_fwd_ms"]["median"] / ms["fwd_ms"]["median"], 2)
        rec["ratio_composed_over_fused"] = round(ms["composed_fwd_bwd_ms"]["median"] / fused, 2)
        # the contenders compute the same thing (against float64: tests/test_gpu_twotower.py)
        with torch.no_grad():
            rec["loss_diff_vs_composed"] = abs(float(loss) - float(composed_loss(U, V, ids, logq, w)))
        rec["max_abs_grad_diff_vs_composed"] = max(float((dU - Ul.grad).abs().max()), float((dV - Vl.grad).abs().max()))
    else:
        rec["composed"] = "not measured: its [B, B] matrices do not fit the comparison" if B > COMPOSED_MAX_B else "off"
    return rec


def step(B, F, D, Dn, towers):
    """TwoTowerEngine.fwd_bwd: hashed ids over 26 x 40000 rows, the first half of the features the user's."""
    spec, idx, dense, _ = hashed_batch(B, F, Dn)
    names, dn = spec.sparse_names, spec.dense_names
    hp = dict(user_features=tuple(names[: F // 2] + dn[: Dn // 2]), item_features=tuple(names[F // 2:] + dn[Dn // 2:]),
              item_id_feature=names[F // 2], user_hidden_units=tuple(towers), item_hidden_units=tuple(towers),
              temperature=0.05)
    e = eng.TwoTowerEngine(spec, D, hp)
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, None)], n=20, warm=3)[0]


if __name__ == "__main__":
    main(lambda comparator: [kernels(B, H, comparator=comparator) for B, H in SHAPES],
         lambda: {f"twotower_B{STEP['B']}_2x256x128_fwd_bwd_ms": step(**STEP)})
