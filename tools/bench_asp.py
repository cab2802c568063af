#!/usr/bin/env python
"""Times rm_asp_fwd / rm_asp_bwd (hipEvents, warm-up, median of 20 timed launches) beside the comparator - the same
arithmetic composed from torch ops in fp32 on the GPU (tests/asp_ref.asp_layer over the gathered rows, forward +
autograd backward; it writes and re-reads x [nnz, 4D] and both hidden activations) - alternating the contenders in one
process.  Shape: B = 65536, D = 16, hidden (80, 40), history lengths uniform 1..50, ids uniform over 1 M rows; plus one
run with Zipf-distributed ids.  Flops per position: 2 (4D H1 + H1 H2) + 2 H_last forward; the backward recomputes that
and adds four products of the two GEMMs' sizes (dz1, dx, dW1, dW0); priced against the 157.3 TFLOP/s fp32 peak.  Also
a DIN engine step with and without the sequence feature.  python tools/bench_asp.py [--json out.json]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tests import asp_ref as R
from tools._bench import emit, medians

PEAK = 157.3e12


def asp_flops(nnz, D, hidden):
    """(forward, backward) flops of the tile kernels."""
    dims = [4 * D] + list(hidden)
    gemm = sum(2 * dims[i] * dims[i + 1] for i in range(len(hidden)))
    fwd = nnz * (gemm + 2 * dims[-1])
    return fwd, fwd + nnz * 2 * gemm


def history(B, max_len, rows, zipf, g):
    n = torch.randint(1, max_len + 1, (B,), generator=g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    nnz = int(offsets[-1])
    if zipf:
        u = torch.rand(nnz + B, generator=g, dtype=torch.float64)
        ids = (rows ** u).long().clamp(1, rows) - 1  # density ~ 1 / id: a few hot rows, a long tail
    else:
        ids = torch.randint(0, rows, (nnz + B,), generator=g)
    return offsets.cuda(), ids[:nnz].cuda(), ids[nnz:].cuda()


def kernels(B=65536, D=16, hidden=(80, 40), max_len=50, rows=1_000_000, act="sigmoid", norm=False, zipf=False):
    g = torch.Generator().manual_seed(0)
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    LD = 2 * D
    table = r(rows, LD) * 0.3
    offsets, ids, qrow = history(B, max_len, rows, zipf, g)
    nnz = int(ids.shape[0])
    dims = [4 * D] + list(hidden)
    Ws = [r(dims[i], dims[i + 1]) * (2 / (dims[i] + dims[i + 1])) ** 0.5 for i in range(len(hidden))]
    bs = [r(h) * 0.1 for h in hidden]
    w, w0 = r(hidden[-1]) * 0.3, r(1) * 0.1
    out, scores = torch.empty(B, LD, device="cuda"), torch.empty(nnz, device="cuda")
    ws = torch.empty(ops.asp_workspace(D, hidden, nnz, True), device="cuda")
    d_rows = r(B, 2, D)
    d_keys = torch.empty(nnz, D, device="cuda")
    dWs, dbs, dw, dw0 = [torch.empty_like(W) for W in Ws], [torch.empty_like(b) for b in bs], torch.empty_like(w), \
        torch.empty_like(w0)
    fwd = lambda: ops.asp_fwd(table, 0, D, offsets, ids, qrow, Ws, bs, w, w0, act, norm, out, scores, ws)  # noqa: E731
    bwd = lambda: ops.asp_bwd(table, 0, D, offsets, ids, qrow, Ws, bs, w, w0, act, norm, scores, d_rows[:, 1, :],  # noqa: E731
                              d_keys, d_rows[:, 0, :], dWs, dbs, dw, dw0, ws)
    g_out = d_rows[:, 1, :].contiguous()
    leaves = [t.clone().requires_grad_(True) for t in Ws + bs + [w, w0]]
    m = len(hidden)

    def composed():
        # the gathered rows are leaves: their gradients are the [nnz, D] key rows and the [B, D] query rows
        Q, K = table[qrow, :D].requires_grad_(True), table[ids, :D].requires_grad_(True)
        for t in leaves:
            t.grad = None
        R.asp_layer(Q, K, offsets, leaves[:m], leaves[m:2 * m], leaves[-2], leaves[-1], act, norm).backward(g_out)

    ms = medians([fwd, bwd, composed], 20, 3)
    f_fwd, f_bwd = asp_flops(nnz, D, hidden)
    fused = ms[0] + ms[1]
    # the contenders compute the same thing (gradients: tests/test_gpu_asp.py, against float64)
    Q, K = table[qrow, :D], table[ids, :D]
    fwd()
    err = float((out[:, :D] - R.asp_layer(Q, K, offsets, Ws, bs, w, w0, act, norm)).abs().max())
    return {"shape": dict(B=B, D=D, hidden=list(hidden), max_len=max_len, nnz=nnz, rows=rows, act=act, norm=norm,
                          ids="zipf" if zipf else "uniform"),
            "asp_fwd_ms": round(ms[0], 4), "asp_bwd_ms": round(ms[1], 4), "fused_fwd_bwd_ms": round(fused, 4),
            "composed_fwd_bwd_ms": round(ms[2], 4), "ratio_composed_over_fused": round(ms[2] / fused, 2),
            "fwd_tflops": round(f_fwd / ms[0] / 1e9, 2), "bwd_tflops": round(f_bwd / ms[1] / 1e9, 2),
            "fwd_peak_share": round(f_fwd / (ms[0] * 1e-3) / PEAK, 4),
            "bwd_peak_share": round(f_bwd / (ms[1] * 1e-3) / PEAK, 4), "max_abs_diff_vs_composed": err}


def steps(B=65536, F=26, D=16, Dn=13, max_len=50, rows=1_000_000):
    """A DIN engine fwd_bwd step with the sequence feature beside the same engine without it."""
    out = {}
    g = torch.Generator().manual_seed(0)
    sizes = [rows] + [40000] * (F - 1)
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in sizes], 1)
    dense, y = torch.randn(B, Dn, generator=g).cuda(), (torch.rand(B, generator=g) < 0.3).long().cuda()
    offsets, ids, _ = history(B, max_len, rows, False, g)
    names = [f"C{i}" for i in range(F)]
    hp = dict(deep_hidden_units=(32, 32))
    for tag, seq in (("without_sequence", False), ("with_sequence", True)):
        if seq:
            spec = eng.FeatureSpec(names + ["hist"], sizes + [0], [f"I{j}" for j in range(Dn)],
                                   seq_query={"hist": "C0"}, seq_max_len={"hist": max_len})
            ix = torch.cat([idx, torch.zeros(B, 1, dtype=torch.int64)], 1).cuda()
            mv = {"hist": (offsets, ids)}
        else:
            spec, ix, mv = eng.FeatureSpec(names, sizes, [f"I{j}" for j in range(Dn)]), idx.cuda(), None
        e = eng.DINEngine(spec, D, hp)
        eng.init_reference(e)
        out[f"din_fwd_bwd_{tag}_ms"] = round(medians([lambda: e.fwd_bwd(ix, dense, y, mv=mv)], 20, 3)[0], 4)
        del e
    return out


if __name__ == "__main__":
    emit({"kernels": [kernels(), kernels(zipf=True), kernels(norm=True, act="relu")], "steps": steps()})
