"""GPU: GroupNdcg / GroupRecall / GroupPrecision(by=...) in fit() / evaluate(): the models hand the metric the
encoded id column of the feature, on the device path, through the pinned feeder and on the host path.  The golden
ml-100k slice: its first 768 rows hold 7 users, its last 256 rows one, and every user has both classes.  Values are
checked against the exact reference on predict() within (3 kmax + S + 16) 2^-53 (tests/test_gpu_rankmetrics.py)."""
from fractions import Fraction

import numpy as np
import pytest
from sklearn.metrics import log_loss as sk_log_loss

from tests import rankmetrics_ref as R
from tests.test_gpu_gauc_model import collect, deepfm, split
from tests.test_gpu_models import ml_features
from tests.test_gpu_rankmetrics import SETTINGS

pytestmark = pytest.mark.gpu

U = Fraction(1, 2 ** 53)
KMAX = 1024


def reference(df, pred, metric="ndcg", k=5, scored="both_classes", weight="groups", by="user_id"):
    """(the exact mean, scored groups) of the predictions, grouped by the RAW column (None: one list)."""
    ids = None if by is None else np.unique(df[by].values, return_inverse=True)[1].reshape(-1)
    disc_kind, norm = SETTINGS[metric]
    ex = R.exact(df["label"].values, np.asarray(pred, dtype=np.float32), ids, R.discounts(disc_kind, k), (k,), norm)
    exact, count, _ = ex.mean(scored, weight)
    assert count >= 1
    return exact[0], count


def check_exact(got, df, pred, **kw):
    exact, count = reference(df, pred, **kw)
    assert type(got) is float
    assert abs(Fraction(got) - exact) <= (3 * KMAX + count + 16) * U * exact, (got, float(exact))


def test_fit_and_evaluate_with_ndcg_on_the_device(hip_lib):
    from recman_amd.metrics import GroupNdcg, GroupPrecision, GroupRecall, RocAucScore

    df, tr, va = split()
    m = deepfm(ml_features(df), (GroupNdcg("user_id", k=5), RocAucScore()))
    assert m._metrics_on_device()
    seen = collect(m, tr, va)
    # epoch_callback sees floats
    assert len(seen) == 2 and all(len(r) == 2 and type(v) is float for rs in seen for r in rs for v in r)
    # the validation part and evaluate() are scored in predict()'s batches: the derived bound
    check_exact(seen[-1][1][0], va, m.predict(va))
    check_exact(m.evaluate(va, va["label"].values)[0], va, m.predict(va))
    check_exact(m.evaluate(tr, tr["label"].values)[0], tr, m.predict(tr))
    assert reference(tr, m.predict(tr))[1] == 7
    # (the last epoch scored the shuffled training rows in other batches: a last-bit change of a score may swap two
    # ranks, so that value has no bound against predict() and only its type and range are checked)
    assert 0.0 <= seen[-1][0][0] <= 1.0
    # recall, precision, the other rule and weights, and one list go through the same plumbing
    pred = m.predict(tr)
    for metric, kw in ((GroupRecall("user_id", k=20), dict(metric="recall", k=20)),
                       (GroupPrecision("user_id", k=3, weight="clicks"), dict(metric="precision", k=3, weight="clicks")),
                       (GroupNdcg("user_id", k=1024, scored="has_positive", weight="impressions"),
                        dict(k=1024, scored="has_positive", weight="impressions")),
                       (GroupNdcg(None, k=50), dict(k=50, by=None))):
        m.metrics = (metric,)
        assert m._metrics_on_device()
        check_exact(m.evaluate(tr, tr["label"].values)[0], tr, pred, **kw)


def test_fit_with_the_pinned_feeder(hip_lib):
    from recman_amd.metrics import GroupNdcg, RocAucScore

    df, tr, va = split()
    m = deepfm(ml_features(df), (GroupNdcg("user_id", k=5), RocAucScore()))
    m.hparams["feeder"] = "pinned"
    assert m._use_feeder(len(tr))
    seen = collect(m, tr, va)
    assert len(seen) == 2
    # the pinned path scores the unshuffled rows in predict()'s batches
    check_exact(seen[-1][0][0], tr, m.predict(tr))
    check_exact(seen[-1][1][0], va, m.predict(va))


def test_a_host_metric_beside_it_takes_the_host_path(hip_lib):
    from recman_amd.metrics import GroupNdcg

    df, tr, va = split()
    calls = []

    class Spy(GroupNdcg):
        def __call__(self, y_true, y_pred, groups=None):
            calls.append((type(y_true), type(y_pred), type(groups)))
            return GroupNdcg.__call__(self, y_true, y_pred, groups=groups)

    m = deepfm(ml_features(df), (Spy("user_id", k=5), sk_log_loss), epoch=1)
    assert not m._metrics_on_device()
    seen = collect(m, tr, va)
    assert calls and all(c == (np.ndarray, np.ndarray, np.ndarray) for c in calls)
    check_exact(seen[-1][1][0], va, m.predict(va))
    host = m.evaluate(tr, tr["label"].values)
    assert host[1] == sk_log_loss(tr["label"].values, m.predict(tr))
    m.metrics = (GroupNdcg("user_id", k=5),)  # the same model on the device path: the same NDCG
    assert m._metrics_on_device()
    dev = m.evaluate(tr, tr["label"].values)
    assert np.float64(host[0]).tobytes() == np.float64(dev[0]).tobytes()


def test_a_listwise_model_is_scored_with_ndcg(hip_lib):
    """rank_loss="listwise" grouped by user, evaluated with GroupNdcg: the value is the reference's (no claim that it
    is better than the pointwise model's)."""
    from recman_amd.metrics import GroupNdcg

    df, tr, va = split()
    m = deepfm(ml_features(df), (GroupNdcg("user_id", k=10),))
    m.hparams.update(dict(rank_loss="listwise", rank_group_by="user_id", rank_loss_weight=0.5))
    seen = collect(m, tr, va)
    assert len(seen) == 2 and m._build().rank["kind"] == "listwise"
    check_exact(seen[-1][1][0], va, m.predict(va), k=10)
    check_exact(m.evaluate(tr, tr["label"].values)[0], tr, m.predict(tr), k=10)
