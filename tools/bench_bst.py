#!/usr/bin/env python
"""Times rm_bst_fwd / rm_bst_bwd (hipEvents, warm-up, median of 20 timed launches) beside the comparator - the same
arithmetic composed from torch ops in fp32 on the GPU (tests/bst_ref.bst_layer over the gathered rows: examples padded
to max_len + 1 tokens with a key mask, forward + autograd backward) - alternating the contenders in one process.
Shape: B = 65536, D = 16, 2 heads, Hf = 64, history lengths uniform 1..20, ids uniform over 1 M rows; plus one run with
Zipf-distributed ids.  Flops per token of an example with T tokens: 2 (4 D D + 2 D Hf) + 4 T D forward; the backward
recomputes that and adds two products per forward product (the input's and the weight's gradient); priced against the
157.3 TFLOP/s fp32 peak.  Bytes: one D-float row read per token and direction, the pooled rows, and in the backward the
key gradients, the pooled rows' gradient and the query gradient's read-modify-write; priced against 8 TB/s.  Also a
BST engine step with and without the sequence feature.  python tools/bench_bst.py [--json out.json]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import bst_ref as R
from tools._bench import emit, medians
from tools.bench_asp import history

PEAK = 157.3e12
HBM = 8.0e12


def bst_work(offsets, D, Hf, LD):
    """(forward flops, backward flops, forward bytes, backward bytes) of the fused kernels."""
    T = (offsets[1:] - offsets[:-1]).double().cpu() + 1
    tokens, B = float(T.sum()), T.numel()
    fwd = tokens * 2 * (4 * D * D + 2 * D * Hf) + float((T * T).sum()) * 4 * D
    row = 4 * D
    # backward: the rows again, the key gradients, and per example d_out read + d_query read and written
    return fwd, 3 * fwd, tokens * row + B * 4 * LD, tokens * row + (tokens - B) * row + B * 3 * row


def kernels(B=65536, D=16, heads=2, Hf=64, max_len=20, rows=1_000_000, zipf=False):
    g = torch.Generator().manual_seed(0)
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    LD = 2 * D
    table = r(rows, LD) * 0.3
    offsets, ids, qrow = history(B, max_len, rows, zipf, g)
    nnz = int(ids.shape[0])
    p = {}
    for n, s in ops.bst_param_shapes(D, Hf, max_len).items():
        if n.endswith("_gamma"):
            p[n] = 1 + 0.1 * r(*s)
        elif len(s) == 2 and n != "pos":
            p[n] = r(*s) * (2 / (s[0] + s[1])) ** 0.5
        else:
            p[n] = r(*s) * 0.1
    out = torch.empty(B, LD, device="cuda")
    ws = torch.empty(ops.bst_workspace(D, heads, Hf, max_len, B, True), device="cuda")
    d_rows = r(B, 2, D)
    d_keys = torch.empty(nnz, D, device="cuda")
    grads = {n: torch.empty_like(v) for n, v in p.items()}
    fwd = lambda: ops.bst_fwd(table, 0, D, offsets, ids, qrow, p, heads, max_len, out, ws)  # noqa: E731
    bwd = lambda: ops.bst_bwd(table, 0, D, offsets, ids, qrow, p, heads, max_len, d_rows[:, 1, :], d_keys,  # noqa: E731
                              d_rows[:, 0, :], grads, ws)
    g_out = d_rows[:, 1, :].contiguous()
    leaves = {n: v.clone().requires_grad_(True) for n, v in p.items()}

    def composed():
        # the gathered rows are leaves: their gradients are the [nnz, D] key rows and the [B, D] query rows
        Q, K = table[qrow, :D].requires_grad_(True), table[ids, :D].requires_grad_(True)
        for t in leaves.values():
            t.grad = None
        R.bst_layer(Q, K, offsets, leaves, heads).backward(g_out)

    ms = medians([fwd, bwd, composed], 20, 3)
    alone = medians([fwd, bwd], 20, 3)  # without the comparator's 50 ms of other traffic between the launches
    f_fwd, f_bwd, b_fwd, b_bwd = bst_work(offsets, D, Hf, LD)
    fused = ms[0] + ms[1]
    # the contenders compute the same thing (gradients: tests/test_gpu_bst.py, against float64)
    fwd()
    with torch.no_grad():
        err = float((out[:, :D] - R.bst_layer(table[qrow, :D], table[ids, :D], offsets, p, heads)).abs().max())
    return {"shape": dict(B=B, D=D, heads=heads, Hf=Hf, max_len=max_len, nnz=nnz, tokens=nnz + B, rows=rows,
                          ids="zipf" if zipf else "uniform"),
            "bst_fwd_ms": round(ms[0], 4), "bst_bwd_ms": round(ms[1], 4), "fused_fwd_bwd_ms": round(fused, 4),
            "fused_fwd_bwd_without_comparator_ms": round(alone[0] + alone[1], 4),
            "composed_fwd_bwd_ms": round(ms[2], 4), "ratio_composed_over_fused": round(ms[2] / fused, 2),
            "fwd_gflop": round(f_fwd / 1e9, 2), "bwd_gflop": round(f_bwd / 1e9, 2),
            "fwd_mb": round(b_fwd / 1e6, 1), "bwd_mb": round(b_bwd / 1e6, 1),
            "fwd_peak_share": round(f_fwd / (ms[0] * 1e-3) / PEAK, 4),
            "bwd_peak_share": round(f_bwd / (ms[1] * 1e-3) / PEAK, 4),
            "fwd_hbm_share": round(b_fwd / (ms[0] * 1e-3) / HBM, 4),
            "bwd_hbm_share": round(b_bwd / (ms[1] * 1e-3) / HBM, 4), "max_abs_diff_vs_composed": err}


def steps(B=65536, F=26, D=16, Dn=13, max_len=20, rows=1_000_000):
    """A BST engine fwd_bwd step with the sequence feature beside the same engine without it, the two taking turns."""
    g = torch.Generator().manual_seed(0)
    sizes = [rows] + [40000] * (F - 1)
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in sizes], 1)
    dense, y = torch.randn(B, Dn, generator=g).cuda(), (torch.rand(B, generator=g) < 0.3).long().cuda()
    offsets, ids, _ = history(B, max_len, rows, False, g)
    names = [f"C{i}" for i in range(F)]
    dn = [f"I{j}" for j in range(Dn)]
    hp = dict(deep_hidden_units=(32, 32), att_head_num=2, att_ffn_units=64)
    plain = eng.BSTEngine(eng.FeatureSpec(names, sizes, dn), D, hp)
    seq = eng.BSTEngine(eng.FeatureSpec(names + ["hist"], sizes + [0], dn, seq_query={"hist": "C0"},
                                        seq_max_len={"hist": max_len}), D, hp)
    eng.init_reference(plain)
    eng.init_reference(seq)
    ix = idx.cuda()
    ix_seq = torch.cat([idx, torch.zeros(B, 1, dtype=torch.int64)], 1).cuda()
    mv = {"hist": (offsets, ids)}
    ms = medians([lambda: plain.fwd_bwd(ix, dense, y), lambda: seq.fwd_bwd(ix_seq, dense, y, mv=mv)], 20, 3)
    return {"bst_fwd_bwd_without_sequence_ms": round(ms[0], 4), "bst_fwd_bwd_with_sequence_ms": round(ms[1], 4),
            "nnz": int(ids.shape[0])}


if __name__ == "__main__":
    emit({"kernels": [kernels(), kernels(zipf=True)], "steps": steps()})
