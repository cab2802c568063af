#!/usr/bin/env python
"""Times rm_mmoe_mix_fwd / rm_mmoe_mix_bwd (hipEvents, warm clocks, 50 timed launches, min / median / mean) beside the
comparator - the same arithmetic composed from torch ops in fp32 over the same Z, A and dM: softmax over the gate
logits, one einsum for the mixture, forward alone and forward + autograd backward - and MMoEEngine.fwd_bwd, the full
model step.  All contenders alternate in one process.  The kernels are priced in algorithmic bytes, 4 B (E H + T E +
T H) forward and twice that backward (dM in, dZ and dA out on top), against the 8 TB/s HBM spec.
    python tools/bench_mmoe.py [--json out.json] [--kernels-only | --step-only]
The shape: B = 65536, F = 26, D = 16, 13 dense features, 8 experts of (256, 128), 2 tasks, towers of (64,).
`--kernels-only` launches nothing but the fused kernels, `--step-only` nothing but the engine's step (the runs to put
under rocprofv3 --kernel-trace --stats)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tools._bench import alternate, hashed_batch, hbm_gb_s_fields, main

SHAPE = dict(B=65536, F=26, D=16, Dn=13, E=8, experts=(256, 128), T=2, towers=(64,))


def composed_mix(Z, A, E, T):
    """The contract as a user would compose it from torch ops."""
    B = Z.shape[0]
    p = torch.softmax(A.reshape(B, T, E), dim=2)
    return torch.einsum("bte,beh->bth", p, Z.reshape(B, E, -1)).reshape(B, -1)


def kernels(B, E, T, H, comparator=True):
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    Z, A, dM = r(B, E * H), r(B, T * E), r(B, T * H)
    M, dZ, dA = torch.empty(B, T * H, device="cuda"), torch.empty(B, E * H, device="cuda"), torch.empty(
        B, T * E, device="cuda")
    fns = [lambda: ops.mmoe_mix_fwd(Z, A, E, T, M), lambda: ops.mmoe_mix_bwd(Z, A, E, T, dM, dZ, dA)]
    names = ["fwd_ms", "bwd_ms"]
    if comparator:
        Zl, Al = Z.clone().requires_grad_(True), A.clone().requires_grad_(True)

        def composed_fwd():
            with torch.no_grad():
                composed_mix(Z, A, E, T)

        def composed():
            Zl.grad = Al.grad = None
            composed_mix(Zl, Al, E, T).backward(dM)

        fns += [composed_fwd, composed]
        names += ["composed_fwd_ms", "composed_fwd_bwd_ms"]
    ms = dict(zip(names, alternate(fns)))
    rec = {"shape": dict(B=B, E=E, T=T, H=H, tile=ops.mmoe_mix_tile(E, T, H), cap=ops.mmoe_mix_tile(E, T, H, "cap"))}
    rec.update(ms)
    hbm_fwd = 4.0 * B * (E * H + T * E + T * H)
    hbm_bwd = 2 * hbm_fwd
    rec.update(hbm_gb_s_fields(hbm_fwd, hbm_bwd, ms["fwd_ms"], ms["bwd_ms"], "hbm_share"))
    if comparator:
        fused = ms["fwd_ms"]["median"] + ms["bwd_ms"]["median"]
        rec["ratio_composed_fwd_over_fused_fwd"] = round(ms["composed_fwd_ms"]["median"] / ms["fwd_ms"]["median"], 2)
        rec["ratio_composed_over_fused"] = round(ms["composed_fwd_bwd_ms"]["median"] / fused, 2)
        # the contenders compute the same thing (against float64: tests/test_gpu_mmoe.py)
        with torch.no_grad():
            rec["max_abs_diff_vs_composed"] = float((M[:4096] - composed_mix(Z[:4096], A[:4096], E, T)).abs().max())
        rec["max_abs_grad_diff_vs_composed"] = max(float((dZ - Zl.grad).abs().max()), float((dA - Al.grad).abs().max()))
    return rec


def step(B, F, D, Dn, E, experts, T, towers):
    """MMoEEngine.fwd_bwd, hashed ids over 26 x 40000 rows, about 30 % of the second task's labels observed."""
    spec, idx, dense, g = hashed_batch(B, F, Dn)
    Y = (torch.rand(B, T, generator=g) < 0.3).float()
    Y[Y[:, 0] == 0, 1:] = float("nan")
    Y = Y.cuda()
    names = ("ctr", "cvr", "like", "dwell", "t4", "t5", "t6", "t7")[:T]
    e = eng.MMoEEngine(spec, D, dict(task_names=names, task_types=("classification",) * T, num_experts=E,
                                     expert_hidden_units=tuple(experts), tower_hidden_units=tuple(towers)))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, Y)], n=20, warm=3)[0]


if __name__ == "__main__":
    s = SHAPE
    main(lambda comparator: [kernels(s["B"], s["E"], s["T"], s["experts"][-1], comparator=comparator)],
         lambda: {"mmoe_8x256x128_2x64_fwd_bwd_ms": step(**s)})
