"""Device ROC AUC / log loss (recman_amd.metrics, csrc/metrics.hip) against sklearn on the host, and one fit() epoch
of a DeepFM scored either way.  Prints one JSON object.

    python tools/bench_metrics.py [--calls 20] [--sizes 1000000,10000000,45840617] [--e2e-rows 4000000] [--no-e2e]

Per size: the median time of a call, from the Python call to the float returned (host clock; the call ends in
its one device-to-host read) and its device span (events around the call), the algorithmic bytes (counted here
from n and the sort's pass count), their share of the 8 TB/s HBM peak, sklearn's time on the same inputs (one
call), and at 10 M the device AUC against the exact integer count.
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs the MI355X")
    out = {"metric": "device roc_auc / log_loss vs sklearn", "calls": a.calls,
           "sizes": sizes_run([int(v) for v in a.sizes.split(",")], a.calls)}
    if not a.no_e2e:
        out["e2e"] = e2e_run(a.e2e_rows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
