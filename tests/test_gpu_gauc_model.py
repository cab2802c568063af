"""GPU: GroupAuc(by=...) in fit() / evaluate(): the models hand the metric the encoded id column of the feature,
on the device path, through the pinned feeder and on the host path.  The golden ml-100k slice: its first 768 rows
hold 7 users, its last 256 rows one, and every user has both classes."""
from fractions import Fraction

import numpy as np
import pytest
from sklearn.metrics import log_loss as sk_log_loss

from tests import gauc_ref as R
from tests.test_gpu_din_model import _features as din_features
from tests.test_gpu_din_model import _frame as din_frame
from tests.test_gpu_models import ml_features, ml_frame

pytestmark = pytest.mark.gpu

U = Fraction(1, 2 ** 53)


def deepfm(fd, metrics, epoch=2, **kw):
    import recman_amd.th as th

    return th.DeepFM(fd, embedding_size=8, deep_dropout=(1, 1, 1), learning_rate=0.01, eval_metric=metrics,
                     epoch=epoch, batch_size=128, random_seed=2019, **kw)


def reference(df, pred, by="user_id"):
    """(exact GAUC, scored groups) of the predictions, grouped by the RAW column."""
    ids = np.unique(df[by].values, return_inverse=True)[1].reshape(-1)
    exact, scored, _, counts = R.exact_gauc(df["label"].values, np.asarray(pred, dtype=np.float32), ids)
    assert scored >= 1
    return exact, scored, counts


def check_exact(got, df, pred, by="user_id"):
    exact, scored, _ = reference(df, pred, by)
    assert type(got) is float
    assert abs(Fraction(got) - exact) <= (scored + 8) * U * exact, (got, float(exact))


def split():
    df = ml_frame()
    tr, va = df.iloc[:768], df.iloc[768:]
    assert tr["user_id"].nunique() == 7 and va["user_id"].nunique() == 1
    return df, tr, va


def collect(m, tr, va=None):
    seen = []
    args = (va, va["label"].values) if va is not None else ()
    m.fit(tr, tr["label"].values, *args,
          epoch_callback=lambda model, eval_results, df_all: seen.append(eval_results))
    return seen


def test_fit_and_evaluate_with_gauc_on_the_device(hip_lib):
    from recman_amd.metrics import GroupAuc, RocAucScore

    df, tr, va = split()
    m = deepfm(ml_features(df), (GroupAuc("user_id"), RocAucScore()))
    assert m._metrics_on_device()
    seen = collect(m, tr, va)
    assert len(seen) == 2 and all(len(r) == 2 and type(v) is float for rs in seen for r in rs for v in r)
    for _, r_va in seen:  # one user in the validation part: the GAUC is its AUC, bit for bit
        assert np.float64(r_va[0]).tobytes() == np.float64(r_va[1]).tobytes()
    # the validation part and evaluate() are scored in predict()'s batches: the derived bound
    check_exact(seen[-1][1][0], va, m.predict(va))
    check_exact(m.evaluate(va, va["label"].values)[0], va, m.predict(va))
    check_exact(m.evaluate(tr, tr["label"].values)[0], tr, m.predict(tr))
    assert reference(tr, m.predict(tr))[1] == 7
    # the last epoch scored the shuffled training rows in other batches: a loose bound
    assert abs(seen[-1][0][0] - float(reference(tr, m.predict(tr))[0])) <= 1e-6
    # the clicks weighting goes through the same plumbing
    m.metrics = (GroupAuc("user_id", weight="clicks"),)
    got = m.evaluate(tr, tr["label"].values)[0]
    exact, scored, _ = R.gauc_of_counts(reference(tr, m.predict(tr))[2], "clicks")
    assert abs(Fraction(got) - exact) <= (scored + 8) * U * exact


def test_fit_with_the_pinned_feeder(hip_lib):
    from recman_amd.metrics import GroupAuc, RocAucScore

    df, tr, va = split()
    m = deepfm(ml_features(df), (GroupAuc("user_id"), RocAucScore()))
    m.hparams["feeder"] = "pinned"
    assert m._use_feeder(len(tr))
    seen = collect(m, tr, va)
    assert len(seen) == 2
    # the pinned path scores the unshuffled rows in predict()'s batches
    check_exact(seen[-1][0][0], tr, m.predict(tr))
    check_exact(seen[-1][1][0], va, m.predict(va))
    assert np.float64(seen[-1][1][0]).tobytes() == np.float64(seen[-1][1][1]).tobytes()


def test_a_host_metric_beside_it_takes_the_host_path(hip_lib):
    from recman_amd.metrics import GroupAuc

    df, tr, va = split()
    calls = []

    class Spy(GroupAuc):
        def __call__(self, y_true, y_pred, groups=None):
            calls.append((type(y_true), type(y_pred), type(groups)))
            return GroupAuc.__call__(self, y_true, y_pred, groups=groups)

    m = deepfm(ml_features(df), (Spy("user_id"), sk_log_loss), epoch=1)
    assert not m._metrics_on_device()
    seen = collect(m, tr, va)
    assert calls and all(c == (np.ndarray, np.ndarray, np.ndarray) for c in calls)
    check_exact(seen[-1][1][0], va, m.predict(va))
    assert abs(seen[-1][0][0] - float(reference(tr, m.predict(tr))[0])) <= 1e-6
    host = m.evaluate(tr, tr["label"].values)
    assert host[1] == sk_log_loss(tr["label"].values, m.predict(tr))
    m.metrics = (GroupAuc("user_id"),)  # the same model on the device path: the same GAUC
    assert m._metrics_on_device()
    dev = m.evaluate(tr, tr["label"].values)
    assert np.float64(host[0]).tobytes() == np.float64(dev[0]).tobytes()


def test_din_grouped_by_its_user_feature(hip_lib):
    from recman_amd import metrics as gm

    df = din_frame()
    th, fd = din_features(df)
    m = th.DIN(fd, embedding_size=8, epoch=1, batch_size=256, learning_rate=0.01,
               eval_metric=(gm.GroupAuc("user"), gm.roc_auc_score))
    assert m._metrics_on_device()
    tr, va = df.iloc[:400], df.iloc[400:]
    seen = []
    m.fit(tr, tr["label"].values, va, va["label"].values, random_seed_for_mini_batch=False,
          epoch_callback=lambda model, eval_results, df_all: seen.append(eval_results))
    check_exact(seen[-1][1][0], va, m.predict(va), by="user")
    check_exact(m.evaluate(df, df["label"].values)[0], df, m.predict(df), by="user")
    with pytest.raises(ValueError, match="group_by"):
        th.DIN(fd, eval_metric=(gm.GroupAuc("hist"),))
