"""CPU: the reference of the grouped top-k ranking metrics (tests/rankmetrics_ref.py) against a per-group sklearn
loop and plain numpy, a hand-computed case, and the surface of the feature - the metric objects, the C ABI of
include/recman_hip_rankmetrics.h and the group_by check of the models - none of which needs a GPU."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
from sklearn.metrics import ndcg_score

from tests import rankmetrics_ref as R
from tests.test_gauc_host import _features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recman_hip_rankmetrics.h")
CUTS = (1, 5, 50)


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _case(n, ids, ties):
    rng = np.random.default_rng(2019)
    y = (rng.random(n) < 0.4).astype(np.int64)
    s = rng.random(n).astype(np.float32)
    if ties:
        s = np.floor(s * 8) / 8
    return y, s, rng.integers(0, ids, n)


@pytest.mark.parametrize("n,ids,ties", [(8193, 6000, False), (8193, 6000, True), (12289, 300, True),
                                        (12289, 300, False), (12289, 5, False), (12289, 5, True)])
def test_reference_equals_a_per_group_sklearn_loop(n, ids, ties):
    y, s, g = _case(n, ids, ties)
    ex = R.exact(y, s, g, R.discounts("log2", max(CUTS)), CUTS, "ideal")
    rows = ex.rows()
    assert [r[0] for r in rows] == sorted(set(g.tolist()))
    assert sum(r[1] for r in rows) == n and sum(r[2] for r in rows) == int(y.sum())
    checked = 0
    for i, (gid, ng, P, vals) in enumerate(rows):
        if i % 7 and ids > 300:  # (sklearn takes a millisecond a call)
            continue
        m = g == gid
        assert (ng, P) == (int(m.sum()), int(y[m].sum()))
        if ng < 2:  # sklearn refuses a single document
            assert vals == [Fraction(P)] * len(CUTS)
            continue
        for k, v in zip(CUTS, vals):
            assert abs(ndcg_score(y[m][None], s[m][None].astype(np.float64), k=k) - float(v)) <= 1e-12
            checked += 1
    assert checked >= 15
    mean, scored, wsum = ex.mean()
    assert scored >= 2 and wsum == scored == sum(0 < P < ng for _, ng, P, _ in rows)
    if ids <= 300:
        assert rows == R.group_values_loop(y, s, g, R.discounts("log2", max(CUTS)), CUTS, "ideal")
        for scoring in R.SCORED:
            for weight in R.WEIGHTS:
                assert ex.mean(scoring, weight) == R.mean_of_values(rows, scoring, weight)


@pytest.mark.parametrize("n,ids", [(8193, 6000), (12289, 300), (12289, 5)])
def test_recall_and_precision_equal_plain_numpy_on_untied_scores(n, ids):
    y, _, g = _case(n, ids, False)
    s = np.random.default_rng(5).permutation(n).astype(np.float32)
    ones = R.discounts("none", max(CUTS))
    rec = R.exact(y, s, g, ones, CUTS, "positives").rows()
    pre = R.exact(y, s, g, ones, CUTS, "k").rows()
    for (gid, ng, P, r), (_, _, _, p) in zip(rec, pre):
        m = g == gid
        top = y[m][np.argsort(-s[m])]
        for c, k in enumerate(CUTS):
            hits = int(top[:k].sum())
            assert p[c] == Fraction(hits, k)
            assert r[c] == (Fraction(hits, P) if P else 0)


def test_reference_on_a_hand_computed_case():
    d = [Fraction(float(v)) for v in R.discounts("log2", 4)]
    #   group 3: 0.9 (+) | tie {0.5, 0.5, 0.5} with one positive, across the cutoff 2 | 0.1 (+)
    #   group 9: all positive (one class)   group 1: shorter than k, the signed zeros tie: {0.0 (+), -0.0 (-)}
    y = np.array([1, 0, 1, 0, 1, 1, 1, 1, 0])
    s = np.array([.9, .5, .5, .5, .1, .3, .4, 0.0, -0.0], dtype=np.float32)
    g = np.array([3, 3, 3, 3, 3, 9, 9, 1, 1])
    rows = R.group_values(y, s, g, R.discounts("log2", 4), (2, 4), "ideal")
    assert rows == R.group_values_loop(y, s, g, R.discounts("log2", 4), (2, 4), "ideal")
    g3_2 = (d[0] + Fraction(1, 3) * d[1]) / (d[0] + d[1])
    g3_4 = (d[0] + Fraction(1, 3) * (d[1] + d[2] + d[3])) / (d[0] + d[1] + d[2])
    g1 = Fraction(1, 2) * (d[0] + d[1]) / d[0]
    assert rows == [(1, 2, 1, [g1, g1]), (3, 5, 3, [g3_2, g3_4]), (9, 2, 2, [Fraction(1), Fraction(1)])]
    assert R.mean_of_values(rows) == ([(g1 + g3_2) / 2, (g1 + g3_4) / 2], 2, 2)
    assert R.mean_of_values(rows, "has_positive", "impressions") == (
        [(2 * g1 + 5 * g3_2 + 2) / 9, (2 * g1 + 5 * g3_4 + 2) / 9], 3, 9)
    assert R.mean_of_values(rows, "both_classes", "clicks")[1:] == (2, 4)
    assert R.mean_of_values(rows[2:]) == (None, 0, 0)
    # recall and precision of the same lists: the tie group gives a third of its one positive per rank
    ones = R.discounts("none", 4)
    rec = R.group_values(y, s, g, ones, (2, 4), "positives")
    pre = R.group_values(y, s, g, ones, (2, 4), "k")
    assert [r[3] for r in rec] == [[1, 1], [Fraction(4, 9), Fraction(2, 3)], [1, 1]]
    assert [r[3] for r in pre] == [[Fraction(1, 2), Fraction(1, 4)], [Fraction(2, 3), Fraction(1, 2)],
                                   [1, Fraction(1, 2)]]
    assert rec == R.group_values_loop(y, s, g, ones, (2, 4), "positives")
    assert pre == R.group_values_loop(y, s, g, ones, (2, 4), "k")
    # no id column: one list with id 0
    assert R.group_values(y, s, None, ones, (4,), "k") == R.group_values(y, s, np.zeros(9, dtype=int), ones, (4,), "k")


def test_metric_objects():
    from recman_amd import metrics as M

    names = {"group_ndcg", "group_recall", "group_precision", "GroupNdcg", "GroupRecall", "GroupPrecision"}
    assert names <= set(M.__all__) and all(n in M.__doc__ for n in names)
    for cls, fn, name in ((M.GroupNdcg, M.group_ndcg, "ndcg"), (M.GroupRecall, M.group_recall, "recall"),
                          (M.GroupPrecision, M.group_precision, "precision")):
        m = cls("user_id")
        assert str(m) == repr(m) == f"{name}@10" and str(cls("u", k=3)) == f"{name}@3"
        assert m.on_device is True and m.higher_the_better is True and m.group_by == m.by == "user_id"
        assert (m.k, m.scored, m.weight) == (10, "both_classes", "groups")
        assert cls(None).group_by is None and fn.on_device is True
        c = cls("u", k=1024, scored="has_positive", weight="clicks")
        assert (c.k, c.scored, c.weight) == (1024, "has_positive", "clicks")
        for bad in (dict(k=0), dict(k=1025), dict(k=(5, 10)), dict(k=2.0), dict(k=True), dict(scored="all"),
                    dict(weight="views")):
            with pytest.raises(ValueError):
                cls("u", **bad)
        with pytest.raises(TypeError, match="user_id"):
            m(np.array([0, 1]), np.array([0.1, 0.2], dtype=np.float32))
        # refused on the host, before anything touches a device
        y, s, g = [0, 1], [0.1, 0.2], [0, 1]
        for bad in (dict(k=0), dict(k=1025), dict(k=(5, 5)), dict(k=tuple(range(1, 10))), dict(k=()), dict(k=1.5),
                    dict(scored="all"), dict(weight="views")):
            with pytest.raises(ValueError):
                fn(y, s, g, **bad)
        with pytest.raises(TypeError):
            fn(y, s, g, sample_weight=[1, 1])
        with pytest.raises(TypeError):
            fn(y, s, g, ignore_ties=True)


def test_the_header_is_bound_in_its_own_table(hip_lib):
    from recman_amd import _lib, ops

    text = _header_text()
    syms = sorted(set(re.findall(r"\b(rm_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["rm_group_gain", "rm_group_gain_workspace"]
    for name in syms:
        assert hasattr(hip_lib, name), f"{name} declared in recman_hip_rankmetrics.h but not exported"
    assert set(_lib.SIGNATURES_RANKMETRICS) == set(syms)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_I64) | set(_lib.SIGNATURES_TOPK)
              | set(_lib.SIGNATURES_MULTITASK) | set(_lib.SIGNATURES_RANK))
    assert not set(_lib.SIGNATURES_RANKMETRICS) & others
    assert hip_lib.rm_group_gain_workspace.restype is ctypes.c_int64 and hip_lib.rm_group_gain.restype is ctypes.c_int
    for name in syms:  # one argtype per declared parameter
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, text, flags=re.S)
        assert len(_lib.SIGNATURES_RANKMETRICS[name][1]) == len(m.group(1).split(",")), name
    # the entry points with a stream: one, an evaluation metric, which the ledger files under NOT_IN_A_STEP
    entries = {m.group(1) for m in re.finditer(r"\b(rm_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
               if re.search(r"\brm_stream_t\s+stream\b", m.group(2))}
    assert entries == {"rm_group_gain"}
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "recman_hip_rankmetrics.h":
            assert "rm_group_gain" not in open(os.path.join(ROOT, "include", h)).read(), h
    raw = open(HEADER).read()
    assert "NOT_IN_A_STEP" in raw and "tests/graph_replay.py" in raw
    assert "NOT_IN_A_STEP" in open(os.path.join(ROOT, "profiles", "rankmetrics.md")).read()
    # the constants and the record: eight doubles and five int64
    for name, value in (("RM_GAIN_MAX_K", 1024), ("RM_GAIN_MAX_CUTOFFS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text)
    assert (ops.GAIN_MAX_K, ops.GAIN_MAX_CUTOFFS) == (1024, 8)
    for table, prefix in ((ops.GAIN_NORMS, "RM_GAIN_NORM_"), (ops.GAIN_SCORED, "RM_GAIN_SCORED_"),
                          (ops.GAIN_WEIGHTS, "RM_GAIN_WEIGHT_")):
        for name, value in table.items():
            assert re.search(r"#define\s+%s%s\s+%d\b" % (prefix, name.upper(), value), text), name
    body = text[text.index("typedef struct rm_group_gain_result"):]
    assert re.search(r"double\s+value\[RM_GAIN_MAX_CUTOFFS\];", body)
    assert re.findall(r"^\s+int64_t\s+(\w+);", body, flags=re.M)[:5] == ["groups", "scored_groups", "weight", "pos",
                                                                       "flags"]
    assert all(callable(getattr(ops, f)) for f in ("group_gain_workspace", "group_gain", "read_group_gain"))


def test_workspace_query_without_a_gpu(hip_lib):
    from recman_amd import ops

    assert ops.group_gain_workspace(0) == 0 and ops.group_gain_workspace(2 ** 31) == 0
    assert ops.group_gain_workspace(-1) == 0
    small, big = ops.group_gain_workspace(1), ops.group_gain_workspace(4097)
    assert 0 < small < big and small % 16 == 0
    # keys, groups and labels twice over, group starts, ids and the label prefix: 30 bytes an element, and O(n)
    top = ops.group_gain_workspace(2 ** 31 - 1)
    assert 30 * (2 ** 31 - 1) <= top <= 32 * (2 ** 31 - 1)


@pytest.mark.parametrize("by", ["age_dense_feature", "tags", "hist", "nope"])
def test_group_by_must_name_a_sparse_feature(by):
    from recman_amd.metrics import GroupNdcg, GroupPrecision, GroupRecall, RocAucScore

    th, fd = _features()
    with pytest.raises(ValueError, match="group_by"):
        th.DeepFM(fd, eval_metric=(GroupNdcg(by),))
    with pytest.raises(ValueError, match="group_by"):
        th.DIN(fd, eval_metric=(RocAucScore(), GroupRecall(by, k=3)))
    with pytest.raises(ValueError, match="group_by"):
        th.xDeepFM(fd, {"embedding_size": 8}, metrics=(GroupPrecision(by),))


def test_group_by_a_sparse_feature_or_none_keeps_the_device_path():
    from sklearn.metrics import log_loss

    from recman_amd.metrics import GroupAuc, GroupNdcg, GroupRecall, RocAucScore

    th, fd = _features()
    m = th.DeepFM(fd, eval_metric=(GroupNdcg("user_id"), RocAucScore()))
    assert m._metrics_on_device() and m._group_columns() == {"user_id": 0}
    m = th.DeepFM(fd, eval_metric=(GroupNdcg("user_id", k=5), GroupAuc("user_id"), GroupRecall(None)))
    assert m._metrics_on_device() and m._group_columns() == {"user_id": 0}
    m = th.DeepFM(fd, eval_metric=(GroupNdcg(None), RocAucScore()))  # one list: no id column is needed
    assert m._metrics_on_device() and m._group_columns() == {}
    m = th.DeepFM(fd, eval_metric=(GroupNdcg("user_id"), log_loss))
    assert not m._metrics_on_device() and m._group_columns() == {"user_id": 0}
