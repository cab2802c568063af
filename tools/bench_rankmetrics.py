"""Device NDCG@k per group (recman_amd.metrics.group_ndcg, csrc/rankmetrics.hip) beside group_auc on the same
tensors in the same process - the same sort, seven passes - and, once, the host alternative.  Prints one JSON object.

    python tools/bench_rankmetrics.py [--sizes 1000000,45840617] [--calls 20] [--groups 1000000] [--loop-rows 20000]
                                      [--no-loop]

Inputs: those of tools/bench_metrics.py --gauc (click rate 0.2, sigmoid scores, ids Zipf-like over --groups ranks).
Per size: the median of --calls hipEvent pairs per contender after two warm-up rounds, the contenders taking turns
(tools/_bench.py): group_auc, group_ndcg with k = 10 and with k = (5, 10, 100), from the Python call to the float
returned.  Beside the measured ratio to group_auc, the ratio the algorithmic bytes predict (counted here from n, the
passes that ran and the group sizes).  At --loop-rows examples: sklearn.metrics.ndcg_score(k=10) once per group with
both classes, on the host, against group_ndcg on the same inputs."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools._bench import times
from tools.bench_metrics import gauc_bytes, gauc_inputs, score_keys, varying_digits


def gain_bytes(n, passes, group_n, kmax):
    """Bytes the grouped gain moves: key pass 29 and 22 per radix pass as gauc_bytes; the count pass (id 4 + label
    byte read), the starts pass (id 4 + label byte read, label prefix 4 written; start 4 + id 4 written per group);
    the group pass (two starts, two prefixes and the id read per group: 20, key 4 + prefix 4 per walked rank, which
    are min(n_g, kmax))."""
    walked = int(torch.clamp(group_n, max=kmax).sum())
    return n * (29 + 22 * passes + 5 + 9) + int(group_n.numel()) * (8 + 20) + walked * 8


def host_loop(y, s, g, k):
    """sklearn.metrics.ndcg_score(k=k) once per group holding both classes; the plain mean."""
    from sklearn.metrics import ndcg_score

    order = np.argsort(g, kind="stable")
    y, s, g = y[order], s[order], g[order]
    cuts = np.flatnonzero(g[1:] != g[:-1]) + 1
    vals = [ndcg_score(yy[None], ss[None], k=k) for yy, ss in zip(np.split(y, cuts), np.split(s, cuts))
            if yy.min() != yy.max()]
    return float(np.mean(vals)), len(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,45840617")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--loop-rows", type=int, default=20_000)
    ap.add_argument("--no-loop", action="store_true", help="skip the host loop (a run under a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rankmetrics.py needs the MI355X")
    from recman_amd import metrics as M

    sizes = [int(v) for v in a.sizes.split(",")]
    out = {"metric": "device group_ndcg beside group_auc", "calls": a.calls, "groups_drawn_from": a.groups, "sizes": []}
    for n in sizes:
        y, s, g = gauc_inputs(n, a.groups)
        fns = [lambda: M.group_auc(y, s, g), lambda: M.group_ndcg(y, s, g, k=10),
               lambda: M.group_ndcg(y, s, g, k=(5, 10, 100))]
        ts = [sorted(t) for t in times(fns, a.calls, 2)]
        t_auc, t_10, t_3 = (t[len(t) // 2] for t in ts)
        v, per = M.group_ndcg(y, s, g, k=10, return_groups=True)
        G = int(per["ids"].numel())
        passes = varying_digits(score_keys(s)) + varying_digits(g)
        b_auc, b_10, b_3 = gauc_bytes(n, passes, G), gain_bytes(n, passes, per["n"], 10), gain_bytes(n, passes, per["n"], 100)
        row = {"n": n, "groups": G, "scored_groups": int(((per["pos"] > 0) & (per["pos"] < per["n"])).sum()),
               "passes": passes, "ndcg@10": v, "group_auc_ms": t_auc, "ndcg_k10_ms": t_10, "ndcg_k5_10_100_ms": t_3,
               "spread_ms": {name: [t[0], t[-1]] for name, t in zip(("group_auc", "ndcg_k10", "ndcg_k5_10_100"), ts)},
               "ratio_k10": t_10 / t_auc, "ratio_k5_10_100": t_3 / t_auc,
               "group_auc_bytes": b_auc, "ndcg_k10_bytes": b_10, "ndcg_k5_10_100_bytes": b_3,
               "ratio_expected_from_bytes_k10": b_10 / b_auc, "ratio_expected_from_bytes_k5_10_100": b_3 / b_auc}
        out["sizes"].append(row)
        print(json.dumps({"progress": row}), file=sys.stderr, flush=True)
        del per, y, s, g
        torch.cuda.empty_cache()
    if a.no_loop:
        print(json.dumps(out))
        return
    y, s, g = gauc_inputs(a.loop_rows, max(2, a.groups * a.loop_rows // max(sizes)))
    yh, sh, gh = y.cpu().numpy(), s.cpu().numpy().astype(np.float64), g.cpu().numpy()
    t0 = time.perf_counter()
    ref, scored = host_loop(yh, sh, gh, 10)
    t1 = time.perf_counter()
    t_dev = sorted(times([lambda: M.group_ndcg(y, s, g, k=10)], a.calls, 2)[0])[a.calls // 2]
    out["host_loop"] = {"n": a.loop_rows, "groups": int(np.unique(gh).size), "scored_groups": scored,
                        "sklearn_per_group_s": t1 - t0, "ndcg_k10_ms": t_dev,
                        "speedup": (t1 - t0) * 1e3 / t_dev, "ndcg_minus_host_loop": M.group_ndcg(y, s, g, k=10) - ref}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
