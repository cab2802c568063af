"""GPU: recman_amd.metrics (csrc/metrics.hip) against host oracles - an exact rational AUC from np.unique group
counts, a float64 numpy log loss, and sklearn itself."""
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch
from sklearn import metrics as skm
from sklearn.exceptions import UndefinedMetricWarning

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max


def exact_auc(y, s):
    """(sum over groups of pos_g (2 neg_before_g + neg_g), 2 P N) as a Fraction: equal scores form one group
    (np.unique merges -0.0 and +0.0)."""
    s = np.asarray(s, dtype=np.float32)
    y = np.asarray(y).astype(np.int64)
    _, inv = np.unique(s, return_inverse=True)
    k = int(inv.max()) + 1
    pos = np.bincount(inv[y == 1], minlength=k).astype(object)
    neg = np.bincount(inv[y == 0], minlength=k).astype(object)
    neg_before = np.concatenate([[0], np.cumsum(neg)[:-1]]).astype(object)
    two_u = int(np.sum(pos * (2 * neg_before + neg)))
    P, N = int(pos.sum()), int(neg.sum())
    return Fraction(two_u, 2 * P * N)


def scores_of(kind, n, rng):
    """(labels int64, scores float32) of one case; both classes present."""
    rate = {"rate_1e-3": 1e-3, "rate_0.999": 0.999}.get(kind, 0.2)
    y = (rng.random(n) < rate).astype(np.int64)
    y[0], y[-1] = 1, 0
    if kind in ("sigmoid", "rate_1e-3", "rate_0.999"):
        s = 1.0 / (1.0 + np.exp(-(rng.standard_normal(n) * 2 + y)))
    elif kind == "q8":
        s = np.floor(rng.random(n) * 8 + y * 1.5).clip(0, 7) / 8
    elif kind == "q256":
        s = np.floor(rng.random(n) * 256 + y * 30).clip(0, 255) / 256
    elif kind == "equal":
        s = np.full(n, 0.5)
    elif kind == "perfect":
        s = y.astype(np.float64)
    elif kind == "inverted":
        s = 1.0 - y
    elif kind == "signed_zero":
        s = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), n)
    elif kind == "general":
        s = rng.standard_normal(n) * 30 - 10
        pick = rng.integers(0, 8, n)
        specials = np.array([1e-40, -1e-40, 1e-45, -1e-45, FLT_MAX, -FLT_MAX, 0.0, -0.0], dtype=np.float32)
        m = rng.random(n) < 0.3
        s = np.where(m, specials[pick], s)
    else:
        raise KeyError(kind)
    return y, np.asarray(s, dtype=np.float32)


KINDS = ["sigmoid", "q8", "q256", "equal", "perfect", "inverted", "signed_zero", "general", "rate_1e-3",
         "rate_0.999"]
SIZES = [2, 63, 64, 65, 1000, 4097, 2 ** 16 + 3, 1_000_003]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_auc_equals_the_exact_rational_and_sklearn(hip_lib, kind, n):
    from recman_amd.metrics import roc_auc_score

    rng = np.random.default_rng(n * 31 + KINDS.index(kind))
    y, s = scores_of(kind, n, rng)
    got = roc_auc_score(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())
    assert isinstance(got, float)
    exact = exact_auc(y, s)
    assert abs(Fraction(got) - exact) <= Fraction(1, 10 ** 15), (got, float(exact))
    assert abs(got - skm.roc_auc_score(y, s)) <= 1e-13
    if kind == "perfect":
        assert got == 1.0
    if kind == "inverted":
        assert got == 0.0
    if kind == "equal":
        assert got == 0.5


def test_auc_at_2p25_elements_is_exact_and_order_independent(hip_lib):
    """Five score levels with chosen counts (each past 2^24, where fp32 counting fails): the exact AUC in closed
    form; a random permutation of the same input gives a bitwise identical result."""
    from recman_amd.metrics import roc_auc_score

    pos = [3_000_001, 5_000_000, 1_234_567, 7_000_000, 800_000]
    neg = [6_000_000, 2_500_000, 4_000_000, 1_019_871, 3_000_000]
    n = sum(pos) + sum(neg)
    assert n == 2 ** 25 + 7
    levels = torch.tensor([-3.5, 0.0, 0.25, 0.2500001, 7.0], dtype=torch.float32)
    counts = torch.tensor([c for pn in zip(pos, neg) for c in pn])
    s = torch.repeat_interleave(levels.repeat_interleave(2), counts).cuda()
    y = torch.repeat_interleave(torch.tensor([1, 0] * 5, dtype=torch.int64), counts).cuda()
    two_u, nb = 0, 0
    for p, q in zip(pos, neg):
        two_u += p * (2 * nb + q)
        nb += q
    exact = Fraction(two_u, 2 * sum(pos) * sum(neg))
    got = roc_auc_score(y, s)
    assert abs(Fraction(got) - exact) <= Fraction(1, 10 ** 15), (got, float(exact))
    g = torch.Generator(device="cuda").manual_seed(5)
    perm = torch.randperm(n, device="cuda", generator=g)
    got2 = roc_auc_score(y[perm], s[perm])
    assert np.float64(got).tobytes() == np.float64(got2).tobytes()


def logloss64(y, p, eps):
    """float64 restatement: clip p and 1 - p in float32 at eps, log and mean in float64."""
    e = np.float32(eps)
    c = np.clip(np.asarray(p, dtype=np.float32), e, np.float32(1) - e)
    q = np.float32(1) - c
    v = np.where(np.asarray(y).astype(np.int64) == 1, c, q).astype(np.float64)
    return float(-np.mean(np.log(v)))


@pytest.mark.parametrize("n", [2, 65, 4097, 100_003, 1_000_000])
@pytest.mark.parametrize("ydtype", ["int64", "bool", "float32"])
def test_log_loss_against_sklearn(hip_lib, n, ydtype):
    from recman_amd.metrics import LogLoss, log_loss

    rng = np.random.default_rng(n + len(ydtype))
    y = (rng.random(n) < 0.3).astype(np.int64)
    y[0], y[1] = 1, 0
    p = (1.0 / (1.0 + np.exp(-rng.standard_normal(n) * 3))).astype(np.float32)
    p[rng.random(n) < 0.01] = 0.0
    p[rng.random(n) < 0.01] = 1.0
    p[0], p[1] = 0.0, 1.0  # the worst cases: clipped
    yt = torch.from_numpy(y.astype(ydtype)).cuda()
    pt = torch.from_numpy(p).cuda()
    got = log_loss(yt, pt)
    ref = skm.log_loss(y, p)
    assert isinstance(got, float)
    assert abs(got - ref) <= 1e-12 * abs(ref), (got, ref)
    assert abs(got - logloss64(y, p, np.finfo(np.float32).eps)) <= 1e-12 * abs(ref)
    again = log_loss(yt, pt)
    assert np.float64(got).tobytes() == np.float64(again).tobytes()
    ll = LogLoss(eps=1e-7)
    v = ll(yt, pt)
    ref7 = logloss64(y, p, 1e-7)
    assert abs(v - ref7) <= 1e-12 * abs(ref7), (v, ref7)


@pytest.mark.parametrize("fn", ["roc_auc_score", "log_loss"])
@pytest.mark.parametrize("bad", ["nan", "inf", "label2", "label-1", "label0.5", "empty"])
def test_invalid_inputs_raise_value_error(hip_lib, fn, bad):
    import recman_amd.metrics as M

    y = np.array([0, 1, 1, 0, 1], dtype=np.float64)
    s = np.array([0.1, 0.8, 0.4, 0.3, 0.9], dtype=np.float32)
    if bad == "nan":
        s[2] = np.nan
    elif bad == "inf":
        s[3] = np.inf
    elif bad == "label2":
        y[1] = 2
    elif bad == "label-1":
        y[0] = -1
    elif bad == "label0.5":
        y[4] = 0.5
    else:
        y, s = y[:0], s[:0]
    if bad.startswith("label") and bad != "label0.5":
        y = y.astype(np.int64)
    with pytest.raises(ValueError):
        getattr(M, fn)(y, s)
    if bad != "empty":
        with pytest.raises(ValueError):
            getattr(M, fn)(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())


def test_one_class_and_keyword_and_input_forms(hip_lib):
    import recman_amd.metrics as M

    y1 = np.ones(10, dtype=np.int64)
    s = np.linspace(0, 1, 10).astype(np.float32)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        v = M.roc_auc_score(y1, s)
    assert np.isnan(v) and any(issubclass(x.category, UndefinedMetricWarning) for x in w)
    with pytest.raises(ValueError, match="only one label"):
        M.log_loss(y1, s)
    with pytest.raises(ValueError, match="only one label"):
        M.log_loss(np.zeros(10, dtype=np.int64), s)
    with pytest.raises(TypeError):
        M.roc_auc_score(y1, s, max_fpr=0.5)
    with pytest.raises(TypeError):
        M.log_loss(y1, s, sample_weight=np.ones(10))
    rng = np.random.default_rng(3)
    y = (rng.random(5000) < 0.4).astype(np.int64)
    p = rng.random(5000).astype(np.float32)
    dev = M.roc_auc_score(torch.from_numpy(y).cuda(), torch.from_numpy(p).cuda())
    assert M.roc_auc_score(y, p) == dev
    assert M.roc_auc_score(y.tolist(), p.tolist()) == dev
    assert M.roc_auc_score(torch.from_numpy(y), torch.from_numpy(p)) == dev
    assert M.roc_auc_score(y.astype(np.int32), p) == dev
    assert M.log_loss(y, p) == M.log_loss(torch.from_numpy(y).cuda(), torch.from_numpy(p).cuda())


def test_metric_classes_mirror_the_reference():
    from recman_amd.metrics import LogLoss, RocAucScore, log_loss, roc_auc_score

    a, b = RocAucScore(), LogLoss()
    assert str(a) == repr(a) == "roc_auc" and a.higher_the_better is True
    assert str(b) == repr(b) == "logloss" and b.higher_the_better is False and b.eps == 1e-7
    assert all(getattr(x, "on_device", False) for x in (a, b, roc_auc_score, log_loss))
