#!/usr/bin/env python
"""Times rm_dien_fwd (save on, as in training) / rm_dien_bwd (hipEvents, warm-up, median of 20 timed launches) beside the
comparator - the same arithmetic composed from torch ops in fp32 on the GPU (tests/dien_ref.dien_layer over the gathered
rows: the padded-batch loop over time with masks, forward + autograd backward) - alternating the contenders in one
process.  Shape (that of tools/bench_bst.py, so the three pooling units compare): B = 65536, D = 16, history lengths
uniform 1..20, ids uniform over 1 M rows; plus one run with Zipf-distributed ids.  Flops: per history position two GRU
steps of two [D] x [D, 3D] products each (24 D D) and the score (2 D), per example att_w q (2 D D); the backward
recomputes the gates and adds the transposed products and the weight gradients (three times the forward); priced against
the 157.3 TFLOP/s fp32 peak.  Bytes: per position one D-float row read, h_t written and read back, g_t and a_t written
(forward); the rows, h_t, g_t, a_t read, two [4, D] sets of pre-activation gradients written and read, the key gradient
written (backward); priced against 8 TB/s.  Also a DIEN engine step with and without the sequence feature.
python tools/bench_dien.py [--json out.json]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import dien_ref as R
from tools._bench import emit, medians
from tools.bench_asp import history

PEAK = 157.3e12
HBM = 8.0e12


def dien_work(offsets, D, LD):
    """(forward flops, backward flops, forward bytes, backward bytes) of the fused kernels."""
    n = (offsets[1:] - offsets[:-1]).double().cpu()
    pos, B = float(n.sum()), n.numel()
    fwd = pos * (24 * D * D + 2 * D) + B * 2 * D * D
    row = 4 * D
    f_bytes = pos * (row + 2 * row + row + 4) + B * (row + 4 * LD)
    b_bytes = pos * (row + 3 * row + 4 + 2 * 2 * 4 * row + row) + B * 4 * row
    return fwd, 3 * fwd, f_bytes, b_bytes


def kernels(B=65536, D=16, max_len=20, rows=1_000_000, zipf=False):
    g = torch.Generator().manual_seed(0)
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    LD = 2 * D
    table = r(rows, LD) * 0.3
    offsets, ids, qrow = history(B, max_len, rows, zipf, g)
    nnz = int(ids.shape[0])
    p = {n: r(*s) * ((2 / (s[0] + s[1])) ** 0.5 if len(s) == 2 else 0.1) for n, s in ops.dien_param_shapes(D).items()}
    out = torch.empty(B, LD, device="cuda")
    ws = torch.empty(ops.dien_workspace(D, max_len, B, nnz, True), device="cuda")
    d_rows = r(B, 2, D)
    d_keys = torch.empty(nnz, D, device="cuda")
    grads = {n: torch.empty_like(v) for n, v in p.items()}
    fwd = lambda: ops.dien_fwd(table, 0, D, offsets, ids, qrow, p, max_len, True, out, ws)  # noqa: E731
    bwd = lambda: ops.dien_bwd(table, 0, D, offsets, ids, qrow, p, max_len, d_rows[:, 1, :], d_keys,  # noqa: E731
                               d_rows[:, 0, :], grads, ws)
    g_out = d_rows[:, 1, :].contiguous()
    leaves = {n: v.clone().requires_grad_(True) for n, v in p.items()}

    def composed():
        # the gathered rows are leaves: their gradients are the [nnz, D] key rows and the [B, D] query rows
        Q, K = table[qrow, :D].requires_grad_(True), table[ids, :D].requires_grad_(True)
        for t in leaves.values():
            t.grad = None
        R.dien_layer(Q, K, offsets, leaves).backward(g_out)

    ms = medians([fwd, bwd, composed], 20, 3)
    alone = medians([fwd, bwd], 20, 3)  # without the comparator's other traffic between the launches
    f_fwd, f_bwd, b_fwd, b_bwd = dien_work(offsets, D, LD)
    fused = ms[0] + ms[1]
    # the contenders compute the same thing (gradients: tests/test_gpu_dien.py, against float64)
    fwd()
    with torch.no_grad():
        err = float((out[:, :D] - R.dien_layer(table[qrow, :D], table[ids, :D], offsets, p)).abs().max())
    return {"shape": dict(B=B, D=D, max_len=max_len, nnz=nnz, rows=rows, ids="zipf" if zipf else "uniform"),
            "workspace_mb": round(4 * ws.numel() / 1e6, 1),
            "dien_fwd_ms": round(ms[0], 4), "dien_bwd_ms": round(ms[1], 4), "fused_fwd_bwd_ms": round(fused, 4),
            "fused_fwd_bwd_without_comparator_ms": round(alone[0] + alone[1], 4),
            "composed_fwd_bwd_ms": round(ms[2], 4), "ratio_composed_over_fused": round(ms[2] / fused, 2),
            "fwd_gflop": round(f_fwd / 1e9, 2), "bwd_gflop": round(f_bwd / 1e9, 2),
            "fwd_mb": round(b_fwd / 1e6, 1), "bwd_mb": round(b_bwd / 1e6, 1),
            "fwd_peak_share": round(f_fwd / (ms[0] * 1e-3) / PEAK, 4),
            "bwd_peak_share": round(f_bwd / (ms[1] * 1e-3) / PEAK, 4),
            "fwd_hbm_share": round(b_fwd / (ms[0] * 1e-3) / HBM, 4),
            "bwd_hbm_share": round(b_bwd / (ms[1] * 1e-3) / HBM, 4), "max_abs_diff_vs_composed": err}


def steps(B=65536, F=26, D=16, Dn=13, max_len=20, rows=1_000_000):
    """A DIEN engine fwd_bwd step with the sequence feature beside the same engine without it, the two taking turns."""
    g = torch.Generator().manual_seed(0)
    sizes = [rows] + [40000] * (F - 1)
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in sizes], 1)
    dense, y = torch.randn(B, Dn, generator=g).cuda(), (torch.rand(B, generator=g) < 0.3).long().cuda()
    offsets, ids, _ = history(B, max_len, rows, False, g)
    names = [f"C{i}" for i in range(F)]
    dn = [f"I{j}" for j in range(Dn)]
    hp = dict(deep_hidden_units=(32, 32))
    plain = eng.DIENEngine(eng.FeatureSpec(names, sizes, dn), D, hp)
    seq = eng.DIENEngine(eng.FeatureSpec(names + ["hist"], sizes + [0], dn, seq_query={"hist": "C0"},
                                         seq_max_len={"hist": max_len}), D, hp)
    eng.init_reference(plain)
    eng.init_reference(seq)
    ix = idx.cuda()
    ix_seq = torch.cat([idx, torch.zeros(B, 1, dtype=torch.int64)], 1).cuda()
    mv = {"hist": (offsets, ids)}
    ms = medians([lambda: plain.fwd_bwd(ix, dense, y), lambda: seq.fwd_bwd(ix_seq, dense, y, mv=mv)], 20, 3)
    return {"dien_fwd_bwd_without_sequence_ms": round(ms[0], 4), "dien_fwd_bwd_with_sequence_ms": round(ms[1], 4),
            "nnz": int(ids.shape[0])}


if __name__ == "__main__":
    emit({"kernels": [kernels(), kernels(zipf=True)], "steps": steps()})
