#!/usr/bin/env python
"""Times rm_topk_ip (csrc/topk.hip; hipEvent pairs, warm clocks, 50 timed launches, min / median / mean) beside the
comparator - the same result built from torch ops: torch.topk(scale * Q @ C_chunk.T, k) over catalogue chunks of at
most 2 GB of scores, then a second torch.topk over the chunks' candidates - and TwoTowerEngine.topk (the grouped
model-level call).  Both contenders of a shape alternate in one process.  The op is priced against its GEMM floor,
2 Nq N H / 157.3 TFLOP/s (the f32-MFMA peak): the scores alone, as if selecting them cost nothing.
    python tools/bench_topk.py [--json out.json] [--kernels-only | --step-only]
Shapes: N = 2^20 catalogue rows of L2-normalised N(0, 1) entries, H in {64, 128}, Nq in {256, 4096}, k in {10, 100,
1000}, scale 20; the step: TwoTowerEngine.topk at Nq = 4096, N = 2^20, H = 64, k = 100."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tools._bench import PEAK_MFMA, alternate, hashed_batch, main

N_ITEMS = 1 << 20
SHAPES = [(H, Nq, k) for H in (64, 128) for Nq in (256, 4096) for k in (10, 100, 1000)]
CHUNK_BYTES = 2 << 30  # the comparator's largest score block
SCALE = 20.0
STEP = dict(Nq=4096, H=64, k=100)


def _data(Nq, H):
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    return torch.nn.functional.normalize(r(Nq, H)), torch.nn.functional.normalize(r(N_ITEMS, H))


def composed(Q, C, k):
    """(scores, rows) of the top k by torch ops, chunked so that no score block passes CHUNK_BYTES."""
    rows_per = max(k, CHUNK_BYTES // (4 * Q.shape[0]))
    vals, idx = [], []
    for s in range(0, C.shape[0], rows_per):
        v, i = torch.topk(SCALE * (Q @ C[s:s + rows_per].t()), k, dim=1)
        vals.append(v)
        idx.append(i + s)
    if len(vals) == 1:
        return vals[0], idx[0]
    v, j = torch.topk(torch.cat(vals, 1), k, dim=1)
    return v, torch.gather(torch.cat(idx, 1), 1, j)


def kernels(H, Nq, k, comparator=True):
    Q, C = _data(Nq, H)
    rows = torch.empty(Nq, k, dtype=torch.int64, device="cuda")
    scores = torch.empty(Nq, k, device="cuda")
    ws = torch.empty(ops.topk_ip_workspace(Nq, N_ITEMS, H, k), device="cuda")
    fns = [lambda: ops.topk_ip(Q, C, k, SCALE, rows, scores, ws)]
    names = ["fused_ms"]
    if comparator:
        fns.append(lambda: composed(Q, C, k))
        names.append("composed_ms")
    ms = dict(zip(names, alternate(fns)))
    floor = 2.0 * Nq * N_ITEMS * H / PEAK_MFMA * 1e3
    rec = {"shape": dict(N=N_ITEMS, H=H, Nq=Nq, k=k, splits=0, cols=ops.topk_ip_tile(H, "cols")),
           "workspace_mb": round(4.0 * ws.numel() / 1e6, 1)}
    rec.update(ms)
    rec.update(gemm_floor_ms=round(floor, 4), fused_floor_share=round(floor / ms["fused_ms"]["median"], 4))
    if comparator:
        rec.update(composed_floor_share=round(floor / ms["composed_ms"]["median"], 4),
                   ratio_composed_over_fused=round(ms["composed_ms"]["median"] / ms["fused_ms"]["median"], 2))
        # the same result: the k-th score of every query agrees to float32 rounding (torch.topk breaks ties its own
        # way, so the rows are compared as sets only where the k-th and (k+1)-th scores differ)
        v, _ = composed(Q, C, k)
        rec["max_abs_score_diff_vs_composed"] = float((v - scores).abs().max())
    return rec


def step(Nq, H, k):
    """TwoTowerEngine.topk over the same catalogue: query groups bounded by TOPK_WS_FLOATS."""
    spec, _, _, _ = hashed_batch(8, 4, 2, rows=16)
    names, dn = spec.sparse_names, spec.dense_names
    hp = dict(user_features=tuple(names[:2] + dn[:1]), item_features=tuple(names[2:] + dn[1:]),
              item_id_feature=names[2], user_hidden_units=(H,), item_hidden_units=(H,), temperature=1.0 / SCALE)
    e = eng.TwoTowerEngine(spec, 8, hp)
    Q, C = _data(Nq, H)
    return alternate([lambda: e.topk(Q, C, k)], n=20, warm=3)[0]


if __name__ == "__main__":
    main(lambda comparator: [kernels(H, Nq, k, comparator=comparator) for H, Nq, k in SHAPES],
         lambda: {f"engine_topk_Nq{STEP['Nq']}_N{N_ITEMS}_H{STEP['H']}_k{STEP['k']}_ms": step(**STEP)})
