#!/usr/bin/env python
"""Times rm_cgc_mix_fwd / rm_cgc_mix_bwd (hipEvents, warm clocks, 50 timed launches, min / median / mean) beside
  - the comparator: the same arithmetic composed from torch ops in fp32 over the same Z, A and dM - a softmax per gate
    and one einsum per gate over the experts it sees, forward alone and forward + autograd backward;
  - the yardstick: rm_mmoe_mix_fwd / rm_mmoe_mix_bwd at E = N experts and T gates on the same Z - a kernel that moves
    almost the same bytes (no shared gate; every gate over all experts);
and rm_multitask_loss_es beside rm_multitask_loss, and PLEEngine.fwd_bwd, the full model step.  All contenders of a
setting alternate in one process.  The mixture kernels are priced in algorithmic bytes, 4 B (N H + AW + G H) forward
and twice that backward (dM in, dZ and dA out on top), against the 8 TB/s HBM spec.
    python tools/bench_ple.py [--json out.json] [--kernels-only | --step-only]
Settings: B = 65536, H = 128, (T, S, C) = (2, 2, 2) and (3, 2, 4), with and without the shared gate.  The step: F = 26,
D = 16, 13 dense features, experts of (256, 128), towers of (64,), two levels, the entire-space loss on (ctr, cvr).
`--kernels-only` launches nothing but the fused kernels, `--step-only` nothing but the engine's step (the runs to put
under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tools._bench import alternate, hashed_batch, hbm_gb_s_fields, main

B, H = 65536, 128
SETTINGS = [(2, 2, 2, 1), (2, 2, 2, 0), (3, 2, 4, 1), (3, 2, 4, 0)]  # (T, S, C, shared_gate)
STEP = dict(B=B, F=26, D=16, Dn=13, T=2, S=2, C=2, L=2, experts=(256, 128), towers=(64,))


def gates(T, S, C, sg):
    """Per gate: (its columns of A, the experts it sees)."""
    N, W = T * S + C, S + C
    out = [(g * W, (g + 1) * W, list(range(g * S, (g + 1) * S)) + list(range(T * S, N))) for g in range(T)]
    return out + ([(T * W, T * W + N, list(range(N)))] if sg else [])


def composed_mix(Z, A, T, S, C, sg):
    """The contract as a user would compose it from torch ops."""
    Zr = Z.reshape(Z.shape[0], T * S + C, -1)
    return torch.cat([torch.einsum("be,beh->bh", torch.softmax(A[:, a0:a1], dim=1), Zr[:, ex])
                      for a0, a1, ex in gates(T, S, C, sg)], dim=1)


def kernels(T, S, C, sg, comparator=True):
    N, AW, G = ops.cgc_widths(T, S, C, sg)
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    pad4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    Z, A, dM = r(B, N * H), r(B, pad4(AW))[:, :AW], r(B, G * H)
    M, dZ = torch.empty(B, G * H, device="cuda"), torch.empty(B, N * H, device="cuda")
    dA = torch.empty(B, pad4(AW), device="cuda")[:, :AW]
    fns = [lambda: ops.cgc_mix_fwd(Z, A, T, S, C, sg, M), lambda: ops.cgc_mix_bwd(Z, A, T, S, C, sg, dM, dZ, dA)]
    names = ["fwd_ms", "bwd_ms"]
    if comparator:
        Zl, Al = Z.clone().requires_grad_(True), A.clone().requires_grad_(True)
        # the MMoE sibling on the same Z: T gates over all N experts
        Am, dMm = r(B, pad4(T * N))[:, : T * N], r(B, T * H)
        Mm, dZm = torch.empty(B, T * H, device="cuda"), torch.empty(B, N * H, device="cuda")
        dAm = torch.empty(B, pad4(T * N), device="cuda")[:, : T * N]

        def composed_fwd():
            with torch.no_grad():
                composed_mix(Z, A, T, S, C, sg)

        def composed():
            Zl.grad = Al.grad = None
            composed_mix(Zl, Al, T, S, C, sg).backward(dM)

        fns += [composed_fwd, composed, lambda: ops.mmoe_mix_fwd(Z, Am, N, T, Mm),
                lambda: ops.mmoe_mix_bwd(Z, Am, N, T, dMm, dZm, dAm)]
        names += ["composed_fwd_ms", "composed_fwd_bwd_ms", "mmoe_fwd_ms", "mmoe_bwd_ms"]
    ms = dict(zip(names, alternate(fns)))
    rec = {"shape": dict(B=B, T=T, S=S, C=C, H=H, shared_gate=sg, N=N, gate_logits=AW, gates=G,
                         tile=ops.cgc_mix_tile(T, S, C, H, sg), cap=ops.cgc_mix_tile(T, S, C, H, sg, "cap"))}
    rec.update(ms)
    hbm_fwd = 4.0 * B * (N * H + AW + G * H)
    rec.update(hbm_gb_s_fields(hbm_fwd, 2 * hbm_fwd, ms["fwd_ms"], ms["bwd_ms"], "hbm_share"))
    if comparator:
        med = lambda n: ms[n]["median"]  # noqa: E731
        fused = med("fwd_ms") + med("bwd_ms")
        rec["ratio_composed_fwd_over_fused_fwd"] = round(med("composed_fwd_ms") / med("fwd_ms"), 2)
        rec["ratio_composed_over_fused"] = round(med("composed_fwd_bwd_ms") / fused, 2)
        mm_fwd = 4.0 * B * (N * H + T * N + T * H)
        rec["mmoe"] = hbm_gb_s_fields(mm_fwd, 2 * mm_fwd, ms["mmoe_fwd_ms"], ms["mmoe_bwd_ms"], "hbm_share")
        rec["ratio_cgc_fwd_over_mmoe_fwd"] = round(med("fwd_ms") / med("mmoe_fwd_ms"), 3)
        rec["ratio_cgc_bwd_over_mmoe_bwd"] = round(med("bwd_ms") / med("mmoe_bwd_ms"), 3)
        # the contenders compute the same thing (against float64: tests/test_gpu_ple.py)
        with torch.no_grad():
            rec["max_abs_diff_vs_composed"] = float(
                (M[:4096] - composed_mix(Z[:4096], A[:4096], T, S, C, sg)).abs().max())
        rec["max_abs_grad_diff_vs_composed"] = max(float((dZ - Zl.grad).abs().max()), float((dA - Al.grad).abs().max()))
    return rec


def _labels(g, T):
    """Clicks (30 %), conversions observed on clicks only, further tasks 0 / 1 with NaN on non-clicks."""
    Y = (torch.rand(B, T, generator=g) < 0.3).float()
    Y[Y[:, 0] == 0, 1:] = float("nan")
    return Y.cuda()


def loss_heads(T=3):
    """rm_multitask_loss_es with the pair (0, 1) beside rm_multitask_loss on the same logits and labels."""
    g = torch.Generator().manual_seed(0)
    logit = (torch.randn(T, B, generator=g) * 2).cuda()
    Y = _labels(g, T)
    types = ["classification"] * T
    out = [dict(pred=torch.empty(T, B, device="cuda"), dlogit=torch.empty(T, B, device="cuda"),
                n_t=torch.zeros(T, dtype=torch.int64, device="cuda"), loss_t=torch.zeros(T, device="cuda"),
                loss=torch.zeros(1, device="cuda")) for _ in range(2)]
    ws = torch.empty(ops.multitask_loss_es_workspace(B, T), device="cuda")

    def run(fn, o, **kw):
        fn(logit, types, o["pred"], Y=Y, dlogit=o["dlogit"], n_t=o["n_t"], loss_t=o["loss_t"], loss=o["loss"],
           workspace=ws, **kw)

    es, plain = alternate([lambda: run(ops.multitask_loss_es, out[0], es=(0, 1)),
                           lambda: run(ops.multitask_loss, out[1])])
    return {"loss_head": dict(B=B, T=T, es_ms=es, plain_ms=plain,
                              ratio_es_over_plain=round(es["median"] / plain["median"], 3))}


def step(B, F, D, Dn, T, S, C, L, experts, towers):
    """PLEEngine.fwd_bwd, hashed ids over 26 x 40000 rows, conversions observed on clicks only."""
    spec, idx, dense, g = hashed_batch(B, F, Dn)
    Y = _labels(g, T)
    names = ("ctr", "cvr", "like", "dwell", "t4", "t5", "t6", "t7")[:T]
    e = eng.PLEEngine(spec, D, dict(task_names=names, task_types=("classification",) * T, num_experts=C,
                                    task_experts=S, num_levels=L, expert_hidden_units=tuple(experts),
                                    tower_hidden_units=tuple(towers), entire_space=names[:2]))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, Y)], n=20, warm=3)[0]


def gate_gemm_paths(K=128, W=6):
    """A gate GEMM of a level above the first, [B, K] x [K, W]: a gate whose columns of A start 16-byte aligned runs on
    the split-operand kernels, one that starts at an odd column (W no multiple of 4) on the plain-f32 kernels - the
    same GEMM on both paths, forward, weight gradient and input gradient."""
    g0 = torch.Generator(device="cuda").manual_seed(1)
    X, Wg = torch.randn(B, K, device="cuda", generator=g0), torch.randn(K, W, device="cuda", generator=g0)
    A, dW, dX = torch.empty(B, 8, device="cuda")[:, :W], torch.empty(K, W, device="cuda"), torch.empty(B, K, device="cuda")
    fws = torch.empty(ops.dense_filter_workspace(K, K), device="cuda")
    wws = torch.empty(max(1, ops.dense_wgrad_workspace(K, W, B)), device="cuda")
    fws6 = torch.empty(ops.dense6_workspace(K, K, B), device="cuda")
    wws6 = torch.empty(ops.dense_wgrad6_workspace(K, W, B), device="cuda")

    def gate(ws6, w6):
        ops.dense_fwd(X, None, Wg, A, fws, act="identity", ws6=ws6)
        ops.dense_wgrad(X, None, A, dW, wws, ws6=w6)
        ops.dense_fwd(A, None, Wg, dX, fws, transposed=True, epilogue=ops.DENSE_ADD, ws6=ws6)

    split, plain = alternate([lambda: gate(fws6, wws6), lambda: gate(None, None)])
    return dict(B=B, K=K, W=W, split_operand_ms=split, plain_f32_ms=plain,
                plain_minus_split_ms=round(plain["median"] - split["median"], 4))


def steps():
    s = STEP
    rec = {"ple_2lv_2+2x256x128_2x64_fwd_bwd_ms": step(**s)}
    # gates of width 6 (T = 3, S = 2, C = 4): on the second level they start at odd columns of A and take the plain-f32
    # GEMMs; what that costs per gate, and the step that has three of them
    rec["ple_2lv_3x2+4x256x128_3x64_fwd_bwd_ms"] = step(**dict(s, T=3, C=4))
    rec["gate_gemm_paths"] = gate_gemm_paths()
    # the share of the step in the new kernels: the step's own mixture launches (level 0 with the shared gate, level 1
    # without) and its loss head, timed on their own at the step's shapes
    T, S, C = s["T"], s["S"], s["C"]
    new = sum(kernels(T, S, C, sg, comparator=False)[n]["median"] for sg in (1, 0) for n in ("fwd_ms", "bwd_ms"))
    new += loss_heads(T)["loss_head"]["es_ms"]["median"]
    rec["new_kernels_ms"] = round(new, 4)
    rec["new_kernels_share_of_step"] = round(new / rec["ple_2lv_2+2x256x128_2x64_fwd_bwd_ms"]["median"], 4)
    return rec


def all_kernels(comparator):
    recs = [kernels(*s, comparator=comparator) for s in SETTINGS]
    return recs + ([loss_heads()] if comparator else [])


if __name__ == "__main__":
    main(all_kernels, steps)
