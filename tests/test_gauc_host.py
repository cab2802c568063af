"""CPU: the grouped-AUC reference against a per-group sklearn loop, and the surface of the feature - the metric
objects, the C ABI symbols and the group_by check of the models - none of which needs a GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
from sklearn.metrics import roc_auc_score as sk_roc_auc

from tests import gauc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sklearn_loop(y, s, g, weight):
    num = den = 0.0
    scored = 0
    for gid in np.unique(g):
        m = g == gid
        if y[m].min() == y[m].max():
            continue
        w = m.sum() if weight == "impressions" else y[m].sum()
        num += w * sk_roc_auc(y[m], s[m])
        den += w
        scored += 1
    return num / den, scored, den


@pytest.mark.parametrize("weight", ["impressions", "clicks"])
@pytest.mark.parametrize("n,ids,ties", [(8193, 6000, False), (12289, 300, True), (12289, 5, False)])
def test_reference_equals_a_per_group_sklearn_loop(n, ids, ties, weight):
    rng = np.random.default_rng(2019)
    y = (rng.random(n) < 0.4).astype(np.int64)
    s = rng.random(n).astype(np.float32)
    if ties:
        s = np.floor(s * 8) / 8
    g = rng.integers(0, ids, n)
    exact, scored, wsum, counts = R.exact_gauc(y, s, g, weight)
    ref, ref_scored, ref_w = sklearn_loop(y, s.astype(np.float32), g, weight)
    assert scored == ref_scored and wsum == ref_w and scored >= 2
    assert abs(float(exact) - ref) <= 1e-13
    assert counts == R.group_counts_loop(y, s, g)
    assert [c[0] for c in counts] == sorted(set(g.tolist()))
    assert sum(c[1] for c in counts) == n and sum(c[2] for c in counts) == int(y.sum())


def test_reference_on_a_hand_computed_case():
    #         group 3: one positive above one negative, one tie  | group 9: one class | group 1: inverted
    y = np.array([1, 0, 1, 0, 1, 1, 0, 1])
    s = np.array([.9, .1, .5, .5, .3, .4, .8, .2], dtype=np.float32)
    g = np.array([3, 3, 3, 3, 9, 9, 1, 1])
    exact, scored, wsum, counts = R.exact_gauc(y, s, g)
    # group 3: pairs (0.9 > 0.1), (0.9 > 0.5), (0.5 > 0.1), (0.5 = 0.5): 2U = 2 + 2 + 2 + 1 = 7 of 8
    assert counts == [(1, 2, 1, 0), (3, 4, 2, 7), (9, 2, 2, 0)]
    assert (exact, scored, wsum) == (Fraction(4 * Fraction(7, 8) + 2 * 0, 6), 2, 6)
    assert R.exact_gauc(y, s, g, "clicks")[0] == Fraction(2 * Fraction(7, 8), 3)
    assert R.exact_gauc(y[4:6], s[4:6], g[4:6])[:3] == (None, 0, 0)
    assert R.scored_share(counts) == 0.75
    # the signed zeros are one level: two positives tie with one negative there, the other negative is on top
    z = np.array([-0.0, 0.0, 1.0, -1.0, 0.0], dtype=np.float32)
    yz = [1, 0, 0, 1, 1]
    assert R.group_counts(yz, z, [4] * 5) == R.group_counts_loop(yz, z, [4] * 5) == [(4, 5, 3, 2)]


def test_metric_objects():
    from recman_amd import metrics as M

    assert {"group_auc", "GroupAuc"} <= set(M.__all__)
    m = M.GroupAuc("user_id")
    assert str(m) == repr(m) == "gauc"
    assert m.on_device is True and m.higher_the_better is True and m.group_by == "user_id"
    assert m.weight == "impressions" and M.GroupAuc("u", weight="clicks").weight == "clicks"
    assert M.group_auc.on_device is True
    with pytest.raises(ValueError):
        M.GroupAuc("u", weight="views")
    with pytest.raises(TypeError, match="user_id"):
        m(np.array([0, 1]), np.array([0.1, 0.2], dtype=np.float32))
    # refused on the host, before anything touches a device
    with pytest.raises(ValueError):
        M.group_auc([0, 1], [0.1, 0.2], [0, 1], weight="views")
    with pytest.raises(TypeError):
        M.group_auc([0, 1], [0.1, 0.2], [0, 1], sample_weight=[1, 1])


def test_abi_symbols_and_binding():
    from recman_amd import _lib, ops

    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    assert re.search(r"#define\s+RM_METRIC_BAD_GROUP\s+16\b", text)
    assert "rm_group_auc_result" in text
    assert re.search(r"\bint64_t\s+rm_group_auc_workspace\s*\(\s*int64_t\s+n\s*\)", text)
    assert re.search(r"\bint\s+rm_group_auc\s*\(", text)
    assert len(_lib.SIGNATURES["rm_group_auc"]) == 12
    assert "rm_group_auc_workspace" in _lib.SIGNATURES_I64
    assert ops.METRIC_BAD_GROUP == 16
    assert all(callable(getattr(ops, f)) for f in ("group_auc_workspace", "group_auc", "read_group_auc"))


def test_workspace_query_without_a_gpu(hip_lib):
    from recman_amd import ops

    assert ops.group_auc_workspace(0) == 0 and ops.group_auc_workspace(2 ** 31) == 0
    small, big = ops.group_auc_workspace(1), ops.group_auc_workspace(4097)
    assert 0 < small < big and small % 16 == 0
    # keys, groups and labels twice over, plus the per-group id / counts / 2U: at least 38 bytes an element
    assert ops.group_auc_workspace(2 ** 31 - 1) >= 38 * (2 ** 31 - 1)


def _features():
    import recman_amd.th as th

    df = pd.DataFrame({"user_id": [1, 2, 3, 1], "tags": ["a|b", "a", "b", ""], "hist": [[1], [2, 3], [], [1]],
                       "age_dense_feature": [1.0, 2.0, 3.0, 4.0]})
    fd = th.FeatureDictionary()
    fd["user_id"] = th.SparseFeat("user_id", 3)
    fd["tags"] = th.MultiValCsvFeat("tags", tags=("a", "b"))
    fd["hist"] = th.SequenceFeat("hist", fd["user_id"], max_len=2)
    fd["age_dense_feature"] = th.DenseFeat("age_dense_feature")
    fd.initialize(df)
    return th, fd


@pytest.mark.parametrize("by", ["age_dense_feature", "tags", "hist", "nope"])
def test_group_by_must_name_a_sparse_feature(by):
    from recman_amd.metrics import GroupAuc, RocAucScore

    th, fd = _features()
    with pytest.raises(ValueError, match="group_by"):
        th.DeepFM(fd, eval_metric=(GroupAuc(by),))
    with pytest.raises(ValueError, match="group_by"):
        th.DIN(fd, eval_metric=(RocAucScore(), GroupAuc(by)))
    with pytest.raises(ValueError, match="group_by"):
        th.xDeepFM(fd, {"embedding_size": 8}, metrics=(GroupAuc(by),))


def test_group_by_a_sparse_feature_is_accepted_and_keeps_the_device_path():
    from sklearn.metrics import log_loss

    from recman_amd.metrics import GroupAuc, RocAucScore

    th, fd = _features()
    m = th.DeepFM(fd, eval_metric=(GroupAuc("user_id"), RocAucScore()))
    assert m._metrics_on_device() and m._group_columns() == {"user_id": 0}
    m = th.DeepFM(fd, eval_metric=(GroupAuc("user_id"), log_loss))
    assert not m._metrics_on_device() and m._group_columns() == {"user_id": 0}
    assert th.DeepFM(fd)._group_columns() == {}
