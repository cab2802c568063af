"""GPU: the grouped AUC (csrc/gauc.hip) against the exact host reference of tests/gauc_ref.py.

The per-group integers (id, n_g, P_g, 2U_g), the number of groups and of scored groups, the weight sum and P must
be EQUAL to the reference's.  The value: with S scored groups the device rounds at most three times per AUC_g (two
integer -> double conversions, one division), once for w_g AUC_g, adds at most S non-negative terms and divides
once, so |got - exact| <= (S + 8) 2^-53 exact is required (derived, not measured).

Sizes: 4096 is the tile, 12 289 three tiles plus one, 300 007 past one grid stride of the key kernel (1024 x 256).
Layouts meant to score (skewed, zipf24, high, gap at n >= 4095) must, by the reference alone, hold at least two
scored groups and 40 % of the examples in scored groups: the labels of scores_of have a click rate of 0.2, at
which `pairs` (two examples a group) scores a third of its groups and is checked without that condition."""
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch
from sklearn.exceptions import UndefinedMetricWarning

from tests import gauc_ref as R
from tests.test_gpu_metrics import exact_auc, scores_of

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097, 12_289, 300_007]
KINDS = ["sigmoid", "q8", "equal", "signed_zero", "general"]
LAYOUTS = ["one", "each", "pairs", "skewed", "zipf24", "high", "gap"]
SCORING = ("skewed", "zipf24", "high", "gap")
U = Fraction(1, 2 ** 53)


def groups_of(layout, n, rng):
    if layout == "one":
        return np.full(n, 5, dtype=np.int64)
    if layout == "each":
        return rng.permutation(n).astype(np.int64) * 3 + 1
    if layout == "pairs":
        return rng.permutation(np.arange(n, dtype=np.int64) // 2)
    if layout == "skewed":  # 90 % in one id (at n = 12 289 it covers whole tiles), the rest over 300 ids
        return np.where(rng.random(n) < 0.9, 77, 1000 + rng.integers(0, 300, n)).astype(np.int64)
    if layout == "zipf24":  # three group digits vary
        return ((np.minimum(rng.zipf(1.3, n), 700) - 1).astype(np.int64) * 2654435761) % (1 << 24)
    if layout == "high":  # the top digit is constant and non-zero
        return rng.integers(0, 50, n).astype(np.int64) + 0xF0000000
    if layout == "gap":  # a middle digit (bits 8..15) is constant
        a = np.minimum(rng.zipf(1.3, n), 200) - 1
        b = np.minimum(rng.zipf(1.5, n), 200) - 1
        return a.astype(np.int64) + (b.astype(np.int64) << 16)
    raise KeyError(layout)


def run(y, s, g, weight=0, per_group=True, workspace=None):
    """The device record (value, groups, scored, weight sum, P, flags) and the per-group rows."""
    from recman_amd import ops

    n = len(y)
    yt, st, gt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (y, s, g))
    per = [torch.full((n,), -7, dtype=torch.int64, device="cuda") for _ in range(4)] if per_group else None
    rec = ops.read_group_auc(ops.group_auc(st, yt, gt, weight, workspace=workspace, per_group=per))
    rows = None
    if per_group:
        G = rec[1]
        assert all(bool((t[G:] == -7).all()) for t in per)  # only the first `groups` entries are written
        rows = list(zip(*(t[:G].cpu().tolist() for t in per)))
    return rec, rows


def check_value(got, exact, scored):
    assert exact is not None and not np.isnan(got)
    assert abs(Fraction(got) - exact) <= (scored + 8) * U * exact, (got, float(exact), scored)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_group_auc_equals_the_exact_reference(hip_lib, layout, n):
    from recman_amd import ops
    from recman_amd.metrics import roc_auc_score

    rng = np.random.default_rng(2019 + 97 * SIZES.index(n) + LAYOUTS.index(layout))
    g = groups_of(layout, n, rng)
    for kind in KINDS:
        y, s = scores_of(kind, n, rng)
        counts = R.group_counts(y, s, g)
        for wk, weight in enumerate(("impressions", "clicks")):
            exact, scored, wsum = R.gauc_of_counts(counts, weight)
            (v, G, S, W, P, flags), rows = run(y, s, g, wk)
            assert rows == counts
            assert (G, S, W, P) == (len(counts), scored, wsum, int(y.sum()))
            if layout in SCORING and n >= 4095:
                assert scored >= 2 and R.scored_share(counts) >= 0.4
            if scored == 0:
                assert np.isnan(v) and flags == ops.METRIC_ONE_CLASS
                continue
            assert flags == 0
            check_value(v, exact, scored)
            if kind == "equal":
                assert v == 0.5
            if layout == "one":  # the integers behind roc_auc_score, and its value bit for bit
                assert Fraction(counts[0][3], 2 * P * (n - P)) == exact_auc(y, s)
                auc = roc_auc_score(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())
                assert np.float64(v).tobytes() == np.float64(auc).tobytes()
            if n >= 12_289 and wk == 0:  # sorted by group: the same bits; and a second call
                o = np.argsort(g, kind="stable")
                again = run(y[o], s[o], g[o], wk, per_group=False)[0]
                assert np.float64(again[0]).tobytes() == np.float64(v).tobytes() and again[1:] == (G, S, W, P, flags)
        if layout == "each":
            assert G == n and S == 0


def test_equal_scores_in_different_groups_do_not_tie(hip_lib):
    """q8 scores, ids laid out so that the same score ends one group and begins the next in the sorted order."""
    y = np.array([1, 0, 0, 1, 1, 0], dtype=np.int64)
    s = np.array([.5, .25, .5, .5, .75, .5], dtype=np.float32)
    g = np.array([1, 1, 1, 2, 2, 2], dtype=np.int64)
    (v, G, S, W, P, flags), rows = run(y, s, g)
    # group 1: the positive beats 0.25 and ties 0.5: 2U = 3 of 4; group 2: 0.5 ties, 0.75 wins: 3 of 4
    assert rows == [(1, 3, 1, 3), (2, 3, 2, 3)] == R.group_counts(y, s, g)
    assert (v, G, S, W, P, flags) == (0.75, 2, 2, 6, 3, 0)


def test_python_surface_values_groups_warning_and_input_forms(hip_lib):
    import recman_amd.metrics as M

    rng = np.random.default_rng(7)
    n = 12_289
    g = groups_of("zipf24", n, rng)
    y, s = scores_of("q8", n, rng)
    counts = R.group_counts(y, s, g)
    yt, st, gt = (torch.from_numpy(a).cuda() for a in (y, s, g))
    for weight in ("impressions", "clicks"):
        exact, scored, _ = R.gauc_of_counts(counts, weight)
        v, d = M.group_auc(yt, st, gt, weight=weight, return_groups=True)
        assert type(v) is float and sorted(d) == ["ids", "n", "pos", "two_u"]
        assert all(t.is_cuda and t.dtype == torch.int64 and t.shape == (len(counts),) for t in d.values())
        assert list(zip(*(d[k].cpu().tolist() for k in ("ids", "n", "pos", "two_u")))) == counts
        check_value(v, exact, scored)
        assert M.group_auc(yt, st, gt, weight=weight) == v  # two calls: the same bits
        assert M.GroupAuc("user", weight=weight)(yt, st, groups=gt) == v
    v = M.group_auc(yt, st, gt)
    # numpy arrays, lists, CPU tensors and narrower integer types are copied once and give the same result
    assert M.group_auc(y, s, g) == v
    assert M.group_auc(y.tolist(), s.tolist(), g.tolist()) == v
    assert M.group_auc(torch.from_numpy(y), torch.from_numpy(s), torch.from_numpy(g)) == v
    assert M.group_auc(y.astype(bool), s, g.astype(np.uint32)) == v
    assert M.group_auc(y, s, gt.to(torch.int32)) == v
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        nan = M.group_auc(y, s, np.arange(n))
    assert np.isnan(nan) and any(issubclass(x.category, UndefinedMetricWarning) for x in w)


def test_stream_and_caller_workspace(hip_lib):
    from recman_amd import ops

    rng = np.random.default_rng(11)
    n = 12_289
    g = groups_of("skewed", n, rng)
    y, s = scores_of("sigmoid", n, rng)
    base, rows = run(y, s, g)
    need = ops.group_auc_workspace(n)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, rows2 = run(y, s, g, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    assert got == base and rows2 == rows
    assert np.float64(got[0]).tobytes() == np.float64(base[0]).tobytes()
    with pytest.raises(ValueError, match="workspace too small"):
        run(y, s, g, workspace=ws[: need - 1])


@pytest.mark.parametrize("bad", ["nan", "label2", "id-1", "id2^32", "float_ids", "bool_ids", "str_ids", "shape",
                                 "empty", "weight", "keyword"])
def test_invalid_inputs_raise(hip_lib, bad):
    import recman_amd.metrics as M

    y = np.array([0, 1, 1, 0, 1], dtype=np.int64)
    s = np.array([0.1, 0.8, 0.4, 0.3, 0.9], dtype=np.float32)
    g = np.array([3, 3, 4, 4, 4], dtype=np.int64)
    kw, err = {}, ValueError
    if bad == "nan":
        s[2] = np.nan
    elif bad == "label2":
        y[1] = 2
    elif bad == "id-1":
        g[0] = -1
    elif bad == "id2^32":
        g[4] = 2 ** 32
    elif bad == "float_ids":
        g = g.astype(np.float64)
    elif bad == "bool_ids":
        g = g > 3
    elif bad == "str_ids":
        g = g.astype(str)
    elif bad == "shape":
        g = g[:4]
    elif bad == "empty":
        y, s, g = y[:0], s[:0], g[:0]
    elif bad == "weight":
        kw = {"weight": "views"}
    else:
        kw, err = {"sample_weight": np.ones(5)}, TypeError
    with pytest.raises(err):
        M.group_auc(y, s, g, **kw)
    if bad not in ("empty", "str_ids"):
        with pytest.raises(err):
            M.group_auc(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), **kw)


def test_roc_auc_is_what_it_was(hip_lib):
    """rm_roc_auc on scores the grouped kernel has just sorted: the exact rational, as before."""
    from recman_amd.metrics import group_auc, roc_auc_score

    rng = np.random.default_rng(3)
    for kind, n in (("q8", 12_289), ("general", 300_007)):
        y, s = scores_of(kind, n, rng)
        yt, st = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
        before = roc_auc_score(yt, st)
        group_auc(yt, st, torch.from_numpy(groups_of("zipf24", n, rng)).cuda())
        after = roc_auc_score(yt, st)
        assert np.float64(before).tobytes() == np.float64(after).tobytes()
        assert abs(Fraction(after) - exact_auc(y, s)) <= Fraction(1, 10 ** 15)
