"""Device ROC AUC / log loss (recman_amd.metrics, csrc/metrics.hip) against sklearn on the host, and one fit() epoch
of a DeepFM scored either way.  Prints one JSON object.

    python tools/bench_metrics.py [--calls 20] [--sizes 1000000,10000000,45840617] [--e2e-rows 4000000] [--no-e2e]
    python tools/bench_metrics.py --gauc [--groups 1000000] [--loop-rows 200000] [--calls 20] [--sizes ...]

Per size: the median time of a call, from the Python call to the float returned (host clock; the call ends in
its one device-to-host read) and its device span (events around the call), the algorithmic bytes (counted here
from n and the sort's pass count), their share of the 8 TB/s HBM peak, sklearn's time on the same inputs (one
call), and at 10 M the device AUC against the exact integer count.

--gauc: the grouped AUC (recman_amd.metrics.group_auc, csrc/gauc.hip) beside roc_auc_score on the same scores, in
the same process: group ids drawn Zipf-like over --groups ranks and hashed into 24 bits.  Per size: both times,
their ratio, the radix passes that ran (digits that vary, found here from the data as the plan kernel finds them),
the ratio the byte counts predict, and the result against the exact host count at the smallest size.  Once, at
--loop-rows examples, the host alternative: sklearn's roc_auc_score per group.
"""
import argparse
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12  # B/s, MI355X spec


def auc_bytes(n, passes=4):
    """Bytes the AUC moves: key pass (score 4 + label 8 read, key 4 + label byte 1 written), per radix pass
    (key read by the histogram, key + label read and written by the scatter: 4 + 5 + 5), group pass (key +
    label read)."""
    return n * (17 + 14 * passes + 5)


def logloss_bytes(n):
    return n * (4 + 8)


def exact_two_u(y, s):
    _, inv = np.unique(s, return_inverse=True)
    k = int(inv.max()) + 1
    pos = np.bincount(inv[y == 1], minlength=k).astype(np.int64)
    neg = np.bincount(inv[y == 0], minlength=k).astype(np.int64)
    nb = np.cumsum(neg) - neg
    two_u = int((pos.astype(object) * (2 * nb + neg).astype(object)).sum())
    P, N = int(pos.sum()), int(neg.sum())
    return Fraction(two_u, 2 * P * N)


def time_calls(fn, calls):
    fn()
    fn()
    host, dev = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        t1 = time.perf_counter()
        b.synchronize()
        host.append(t1 - t0)
        dev.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(host)), float(np.median(dev))


def sizes_run(sizes, calls):
    from sklearn import metrics as skm

    from recman_amd import metrics as M

    out = []
    for n in sizes:
        g = torch.Generator(device="cuda").manual_seed(n)
        y = (torch.rand(n, device="cuda", generator=g) < 0.2).to(torch.int64)
        s = torch.sigmoid(torch.randn(n, device="cuda", generator=g) * 2 + y.float())
        t_auc, d_auc = time_calls(lambda: M.roc_auc_score(y, s), calls)
        t_ll, d_ll = time_calls(lambda: M.log_loss(y, s), calls)
        yh, sh = y.cpu().numpy(), s.cpu().numpy()
        t0 = time.perf_counter()
        sk_auc = skm.roc_auc_score(yh, sh)
        t1 = time.perf_counter()
        sk_ll = skm.log_loss(yh, sh)
        t2 = time.perf_counter()
        auc, ll = M.roc_auc_score(y, s), M.log_loss(y, s)
        row = {"n": n,
               "roc_auc_ms": t_auc * 1e3, "roc_auc_device_ms": d_auc * 1e3,
               "roc_auc_bytes": auc_bytes(n), "roc_auc_hbm_fraction": auc_bytes(n) / t_auc / HBM_PEAK,
               "log_loss_ms": t_ll * 1e3, "log_loss_device_ms": d_ll * 1e3,
               "log_loss_bytes": logloss_bytes(n), "log_loss_hbm_fraction": logloss_bytes(n) / t_ll / HBM_PEAK,
               "sklearn_roc_auc_s": t1 - t0, "sklearn_log_loss_s": t2 - t1,
               "speedup_roc_auc": (t1 - t0) / t_auc, "speedup_log_loss": (t2 - t1) / t_ll,
               "roc_auc_minus_sklearn": auc - sk_auc, "log_loss_rel_diff_sklearn": (ll - sk_ll) / sk_ll}
        if n == 10_000_000:
            exact = exact_two_u(yh, sh)
            row["roc_auc_minus_exact"] = float(Fraction(auc) - exact)
        out.append(row)
        print(json.dumps({"progress": row}), file=sys.stderr, flush=True)
    return out


def gauc_bytes(n, passes, groups):
    """Bytes the grouped AUC moves: key pass (score 4 + label 8 + id 8 read, key 4 + id 4 + label byte written),
    per radix pass (one digit source read by the histogram, key + id + label read and written by the scatter:
    4 + 9 + 9), the marks pass (key + id read), the segment pass (key + id + label read, id 4 + two sums of 8
    cleared and added per group) and the reduce pass (20 read per group)."""
    return n * (29 + 22 * passes + 8 + 9) + groups * (16 + 20 + 20)


def varying_digits(keys):
    """How many of the four bytes of a uint32-valued int64 tensor take more than one value."""
    return sum(int(((keys >> (8 * p)) & 255).unique().numel() > 1) for p in range(4))


def score_keys(s):
    """The order-preserving key of csrc/rm_metric_common.h, as int64."""
    b = s.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    return torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)


def host_loop(y, s, g):
    """sklearn.roc_auc_score once per group holding both classes, weighted by the group's examples."""
    from sklearn.metrics import roc_auc_score

    order = np.argsort(g, kind="stable")
    y, s, g = y[order], s[order], g[order]
    cuts = np.flatnonzero(g[1:] != g[:-1]) + 1
    num = den = 0.0
    for yy, ss in zip(np.split(y, cuts), np.split(s, cuts)):
        if yy.min() != yy.max():
            num += len(yy) * roc_auc_score(yy, ss)
            den += len(yy)
    return num / den


def gauc_inputs(n, G):
    """(labels, scores, group ids) on the GPU, seeded by n: a click rate of 0.2, sigmoid scores, ids drawn Zipf-like
    over the ranks 1 .. G and hashed into 24 bits."""
    gen = torch.Generator(device="cuda").manual_seed(n)
    y = (torch.rand(n, device="cuda", generator=gen) < 0.2).to(torch.int64)
    s = torch.sigmoid(torch.randn(n, device="cuda", generator=gen) * 2 + y.float())
    rank = torch.pow(float(G), torch.rand(n, device="cuda", generator=gen, dtype=torch.float64)).to(torch.int64)
    return y, s, (rank * 2654435761) % (1 << 24)


def gauc_run(sizes, calls, groups, loop_rows):
    from recman_amd import metrics as M

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import gauc_ref

    draw = gauc_inputs

    out = {"groups_drawn_from": groups, "sizes": []}
    for i, n in enumerate(sizes):
        y, s, g = draw(n, groups)
        t_auc, d_auc = time_calls(lambda: M.roc_auc_score(y, s), calls)
        t_g, d_g = time_calls(lambda: M.group_auc(y, s, g), calls)
        v, per = M.group_auc(y, s, g, return_groups=True)
        G = int(per["ids"].numel())
        kd, gd = varying_digits(score_keys(s)), varying_digits(g)
        row = {"n": n, "groups": G, "scored_groups": int(((per["pos"] > 0) & (per["pos"] < per["n"])).sum()),
               "score_passes": kd, "group_passes": gd, "gauc": v,
               "roc_auc_ms": t_auc * 1e3, "roc_auc_device_ms": d_auc * 1e3,
               "gauc_ms": t_g * 1e3, "gauc_device_ms": d_g * 1e3,
               "ratio_device": d_g / d_auc, "ratio_host_clock": t_g / t_auc,
               "gauc_bytes": gauc_bytes(n, kd + gd, G), "roc_auc_bytes": auc_bytes(n, kd),
               "ratio_expected_from_bytes": gauc_bytes(n, kd + gd, G) / auc_bytes(n, kd),
               "gauc_hbm_fraction": gauc_bytes(n, kd + gd, G) / d_g / HBM_PEAK}
        del per
        if i == 0:
            exact, scored, _, _ = gauc_ref.exact_gauc(y.cpu().numpy(), s.cpu().numpy(), g.cpu().numpy())
            row["gauc_minus_exact"] = float(Fraction(v) - exact)
        out["sizes"].append(row)
        print(json.dumps({"progress": row}), file=sys.stderr, flush=True)
        del y, s, g
        torch.cuda.empty_cache()
    y, s, g = draw(loop_rows, max(2, groups * loop_rows // max(sizes)))
    yh, sh, gh = y.cpu().numpy(), s.cpu().numpy(), g.cpu().numpy()
    t0 = time.perf_counter()
    ref = host_loop(yh, sh, gh)
    t1 = time.perf_counter()
    t_g, _ = time_calls(lambda: M.group_auc(y, s, g), calls)
    out["host_loop"] = {"n": loop_rows, "groups": int(np.unique(gh).size), "sklearn_per_group_s": t1 - t0,
                        "gauc_ms": t_g * 1e3, "gauc_minus_host_loop": M.group_auc(y, s, g) - ref}
    return out


def e2e_run(rows):
    """One fit() epoch of a DeepFM with configs[1]-shaped features (26 sparse fields, 13 dense, D = 16, batch
    65 536): wall time between the epoch callbacks of epochs 1 and 2, i.e. a training epoch plus its evaluation."""
    import pandas as pd
    from sklearn.metrics import log_loss, roc_auc_score
    from sklearn.preprocessing import MinMaxScaler

    import recman_amd.th as th
    from recman_amd.metrics import LogLoss, RocAucScore

    rng = np.random.default_rng(0)
    vocab = [int(v) for v in rng.integers(100, 200_000, 26)]
    cols = {f"C{i}": rng.integers(0, v, rows, dtype=np.int64) for i, v in enumerate(vocab)}
    cols.update({f"I{i}": rng.random(rows, dtype=np.float32) for i in range(13)})
    df = pd.DataFrame(cols)
    y = (rng.random(rows) < 0.25).astype(np.int64)
    fd = th.FeatureDictionary()
    for i in range(26):
        fd[f"C{i}"] = th.SparseFeat(name=f"C{i}", feat_size=int(np.unique(df[f"C{i}"].values).size))
    for i in range(13):
        fd[f"I{i}"] = th.DenseFeat(name=f"I{i}", scaler=MinMaxScaler())
    fd.initialize(df)
    res = {"rows": rows}
    for name, metrics in (("sklearn", (roc_auc_score, log_loss)), ("recman_amd", (RocAucScore(), LogLoss()))):
        m = th.DeepFM(fd, embedding_size=16, deep_dropout=(1, 1, 1), epoch=2, batch_size=65536, learning_rate=1e-3,
                      eval_metric=metrics)
        stamps = []
        m.fit(df, y, epoch_callback=lambda model, eval_results, df_all: (torch.cuda.synchronize(),
                                                                         stamps.append(time.perf_counter())))
        torch.cuda.synchronize()
        idx, dense, yt = m._encode(df, y)
        t0 = time.perf_counter()
        if name == "sklearn":
            m._eval_at_epoch((idx, dense, None), y)
        else:
            m._eval_at_epoch((idx, dense, None), yt)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res[f"epoch_s_{name}"] = stamps[1] - stamps[0]
        res[f"eval_s_{name}"] = t1 - t0
        del m
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="1000000,10000000,45840617")
    ap.add_argument("--e2e-rows", type=int, default=4_000_000)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--gauc", action="store_true")
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--loop-rows", type=int, default=200_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs the MI355X")
    if a.gauc:
        out = {"metric": "device group_auc beside roc_auc_score", "calls": a.calls}
        out.update(gauc_run([int(v) for v in a.sizes.split(",")], a.calls, a.groups, a.loop_rows))
        print(json.dumps(out))
        return
    out = {"metric": "device roc_auc / log_loss vs sklearn", "calls": a.calls,
           "sizes": sizes_run([int(v) for v in a.sizes.split(",")], a.calls)}
    if not a.no_e2e:
        out["e2e"] = e2e_run(a.e2e_rows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
