"""GPU: fit() / evaluate() with recman_amd.metrics keep predictions and labels on the device; the results equal
sklearn on predict()'s output.  Host metrics keep the host path."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from sklearn.metrics import log_loss as sk_log_loss
from sklearn.metrics import roc_auc_score as sk_roc_auc

from tests.test_gpu_metrics import exact_auc, logloss64
from tests.test_gpu_models import ml_features, ml_frame

pytestmark = pytest.mark.gpu


def make_model(cls_name, fd, metrics, epoch=2, **kw):
    import recman_amd.th as th

    common = dict(epoch=epoch, batch_size=128, random_seed=2019, **kw)
    if cls_name == "DeepFM":
        return th.DeepFM(fd, embedding_size=8, deep_dropout=(1, 1, 1), learning_rate=0.01, eval_metric=metrics,
                         **common)
    if cls_name == "DCN":
        return th.DCN(fd, embedding_size=8, deep_dropout=(1, 1, 1), learning_rate=0.01, cross_layer_num=2,
                      eval_metric=metrics, **common)
    hpx = {"embedding_size": 8, "deep_dropout": (1, 1, 1), "cin_cross_layer_units": [16, 16],
           "cin_dropout": [1, 1, 1], "learning_rate": 0.01}
    return th.xDeepFM(fd, hpx, metrics=metrics, **common)


def check_against_host(res, y, pred, tol):
    """res = [roc_auc, LogLoss(1e-7), log_loss] results on labels y / predictions pred (host)."""
    pred = np.asarray(pred, dtype=np.float32)
    assert abs(res[0] - float(exact_auc(y, pred))) <= tol[0]
    assert abs(res[0] - sk_roc_auc(y, pred)) <= max(tol[0], 1e-13)
    ref1, ref2 = logloss64(y, pred, 1e-7), sk_log_loss(y, pred)
    assert abs(res[1] - ref1) <= tol[1] * abs(ref1)
    assert abs(res[2] - ref2) <= tol[1] * abs(ref2)


@pytest.mark.parametrize("cls_name", ["DeepFM", "DCN", "xDeepFM"])
def test_fit_and_evaluate_with_device_metrics(hip_lib, cls_name):
    from recman_amd.metrics import LogLoss, RocAucScore, log_loss

    df = ml_frame()
    fd = ml_features(df)
    tr, va = df.iloc[:768], df.iloc[768:]  # (the slice has 1024 rows)
    m = make_model(cls_name, fd, (RocAucScore(), LogLoss(), log_loss))
    seen = []
    m.fit(tr, tr["label"].values, va, va["label"].values,
          epoch_callback=lambda model, eval_results, df_all: seen.append(eval_results))
    assert len(seen) == 2
    for r_tr, r_va in seen:
        assert len(r_tr) == 3 and len(r_va) == 3
        assert all(type(v) is float for v in r_tr + r_va)
    ytr, yva = tr["label"].values, va["label"].values
    # the last epoch scored the shuffled training set: other batches, so a loose bound
    check_against_host(seen[-1][0], ytr, m.predict(tr), (1e-6, 1e-6))
    # the validation set is scored in predict()'s batches: exact
    check_against_host(seen[-1][1], yva, m.predict(va), (1e-15, 1e-12))
    ev = m.evaluate(va, yva)
    assert all(type(v) is float for v in ev)
    check_against_host(ev, yva, m.predict(va), (1e-15, 1e-12))


def test_fit_with_the_pinned_feeder_and_device_metrics(hip_lib):
    from recman_amd.metrics import LogLoss, RocAucScore, log_loss

    df = ml_frame()
    fd = ml_features(df)
    m = make_model("DeepFM", fd, (RocAucScore(), LogLoss(), log_loss))
    m.hparams["feeder"] = "pinned"
    assert m._use_feeder(len(df))
    seen = []
    m.fit(df, df["label"].values, epoch_callback=lambda model, eval_results, df_all: seen.append(eval_results))
    # the pinned path scores the unshuffled rows in predict()'s batches
    check_against_host(seen[-1][0], df["label"].values, m.predict(df), (1e-15, 1e-12))


@pytest.mark.parametrize("strict", [False, True])
def test_device_prediction_buffer_equals_predict_bitwise(hip_lib, strict):
    import recman_amd.th as th
    from recman_amd.metrics import RocAucScore

    df = ml_frame()
    fd = ml_features(df)
    m = th.DeepFM(fd, embedding_size=8, deep_dropout=(0.7, 0.8, 0.9), fm_dropout=(1.0, 0.9), learning_rate=0.01,
                  epoch=1, batch_size=300, strict_reference=strict, eval_metric=(RocAucScore(),))
    m.fit(df, df["label"].values)
    idx, dense, _ = m._encode(df)
    mv = m._mv_host
    torch.manual_seed(11)
    host = m._predict_encoded(idx, dense, strict, mv)
    torch.manual_seed(11)
    dev = m._predict_device(idx, dense, strict, mv)
    assert dev.dtype == torch.float32 and dev.is_cuda
    assert np.array_equal(host.view(np.int32), dev.cpu().numpy().view(np.int32))
    if not strict:
        assert np.array_equal(host.view(np.int32), m.predict(df).view(np.int32))


def test_host_metrics_keep_the_host_path(hip_lib):
    df = ml_frame()
    fd = ml_features(df)
    m = make_model("DeepFM", fd, (sk_roc_auc, sk_log_loss), epoch=1)
    assert not m._metrics_on_device()
    calls = []

    def spy(y, p):
        calls.append((type(y), type(p)))
        return sk_roc_auc(y, p)

    m.metrics = (spy, sk_log_loss)
    seen = []
    m.fit(df, df["label"].values, epoch_callback=lambda model, eval_results, df_all: seen.append(eval_results))
    assert all(t == (np.ndarray, np.ndarray) for t in calls)
    y = df["label"].values
    pred = m.predict(df)
    ev = m.evaluate(df, y)
    assert ev[0] == sk_roc_auc(y, pred) and ev[1] == sk_log_loss(y, pred)
    assert abs(seen[-1][0][0] - sk_roc_auc(y, pred)) < 1e-6


def _sharded_worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.pop("RECMAN_FORCE_COLLECTIVES", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys

        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import recman_amd.th as th
        from recman_amd.metrics import LogLoss, RocAucScore
        from tests.test_gpu_models import ml_features, ml_frame

        df = ml_frame().iloc[:1000].copy()
        fd = ml_features(df)
        m = th.DeepFM(fd, embedding_size=16, embedding_l2_reg=0.0, linear_l2_reg=0.0, deep_dropout=(1, 1, 1),
                      learning_rate=0.01, epoch=2, batch_size=96, eval_metric=(RocAucScore(), LogLoss()))
        yv = df["label"].values
        seen = []
        m.fit(df, yv, epoch_callback=lambda model, eval_results, df_all: seen.append(eval_results))
        assert m._shard == (rank, world)
        pred = m.predict(df)
        torch.save({"results": [list(r[0]) for r in seen], "pred": torch.from_numpy(pred), "y": torch.from_numpy(yv)},
                   f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


def test_sharded_fit_with_device_metrics_on_two_ranks(hip_lib, tmp_path):
    world = 2
    out = str(tmp_path / "m")
    mp.spawn(_sharded_worker, args=(world, 29377, out), nprocs=world, join=True)
    res = [torch.load(f"{out}.{r}", weights_only=True) for r in range(world)]
    assert res[0]["results"] == res[1]["results"]
    assert all(type(v) is float for r in res[0]["results"] for v in r)
    for r in range(world):
        y, pred = res[r]["y"].numpy(), res[r]["pred"].numpy()
        last = res[r]["results"][-1]
        assert abs(last[0] - sk_roc_auc(y, pred)) < 1e-6
        ref = logloss64(y, pred, 1e-7)
        assert abs(last[1] - ref) < 1e-6 * abs(ref)
