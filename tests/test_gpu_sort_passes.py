"""GPU: what the shared radix sort (csrc/rm_radix_sort.h) decides for its four users at once - which passes run, and
in which buffer the sorted records end up - through rm_roc_auc, rm_group_auc, rm_group_gain and rm_rank_loss.

The sort skips every 8-bit digit that is the same in all records; with m digits left, pass i reads buffer i & 1 and
the kernels after the sort read buffer m & 1.  Each entry point gets inputs whose m is known: the host computes it
here from a numpy restatement of the score key and the byte columns (a digit varies when it is not the same in every
example).  Per entry point the cases hold m = 0, m = 1, an even m >= 2, an odd m >= 3 and m = every digit (4, 8, 8
and 5 digits): asserted on import, before anything is launched - a condition on the inputs, not on the library.

Sizes: 4097 is two tiles, the second with one element; 12 289 three tiles plus one - the smallest shapes at which the
tile loop, the scan over the tiles and the padding past n can go wrong.

Compared against the host references of the four existing modules at their own exactness: the exact rational AUC and
sklearn (tests/test_gpu_metrics.py), the exact per-group integers and the (S + 8) 2^-53 bound
(tests/test_gpu_gauc.py), the exact rationals and the (3k + 8) 2^-53 bounds (tests/test_gpu_rankmetrics.py), and the
float64 twin with the bound of tests/test_gpu_rank.py.  The record of a random permutation of the same input is
bit-equal for the three metrics; two runs of the rank loss are bit-equal.

The rank loss with one group of both classes (m = 1) is pairwise only at 4097: its float64 twin forms the P x N matrix
of the group."""
from fractions import Fraction

import numpy as np
import pytest
import torch
from sklearn import metrics as skm

from tests import gauc_ref, rank_ref
from tests import test_gpu_gauc as G
from tests import test_gpu_rank as K
from tests import test_gpu_rankmetrics as T
from tests.test_gpu_metrics import exact_auc

SIZES = (4097, 12_289)
FIXED_ID = 0xA1B2C3D4  # the bytes of an id column that do not vary


# ------------------------------------------------------------------------------------------- the host's count of m
def score_key(s):
    """The order-preserving uint32 key of a float32 score; -0.0 is +0.0."""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def varying_bytes(col):
    """How many of the four bytes of a uint32 column are not the same in every example."""
    col = np.asarray(col, dtype=np.uint32)
    return sum(int(len(np.unique((col >> (8 * p)) & 255)) > 1) for p in range(4))


def passes_of(entry, y, s, g):
    """m of the entry point's sort.  The top-k metrics sort by the key's complement: the same bytes vary."""
    ids = 0 if g is None else varying_bytes(g)
    if entry == "rank_loss":
        return int(len(np.unique(np.asarray(y) == 1)) > 1) + ids
    return varying_bytes(score_key(s)) + (0 if entry == "roc_auc" else ids)


# -------------------------------------------------------------------------------------------------------- the inputs
def scores_with(digits, n, rng):
    """float32 scores whose key varies in its `digits` low bytes only (4: in every byte)."""
    if digits == 0:
        return np.full(n, 0.5, dtype=np.float32)
    if digits < 4:  # 1.0 + j 2^-23: the exponent byte is fixed
        j = rng.integers(0, (256, 65_536, 2 ** 23)[digits - 1], n)
        return (np.float32(1.0) + j.astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return (sign * (1.0 + rng.random(n)) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)


def ids_with(digits, n, rng, pool=48):
    """int64 ids from a pool of `pool` values that vary in their `digits` low bytes only."""
    mask = (1 << (8 * digits)) - 1
    values = (rng.integers(0, mask + 1, pool).astype(np.int64) & mask) | (FIXED_ID & ~mask)
    return values[rng.integers(0, pool, n)]


def labels_of(n, rng, rate=0.3):
    y = (rng.random(n) < rate).astype(np.int64)
    y[0], y[-1] = 1, 0
    return y


# (score digits, id digits) per case; the rank loss: (both classes, id digits or None for no id column)
PLANS = {
    "roc_auc": [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)],
    "group_auc": [(0, 0), (1, 0), (1, 1), (2, 1), (3, 3), (4, 3), (4, 4)],
    "group_gain": [(0, 0), (1, 0), (1, 1), (2, 1), (3, 3), (4, 3), (4, 4)],
    "rank_loss": [(False, 0), (True, None), (True, 0), (True, 1), (True, 2), (False, 4), (True, 4)],
}
DIGITS = {"roc_auc": 4, "group_auc": 8, "group_gain": 8, "rank_loss": 5}


def make(entry, plan, n):
    """(y, s, g) of a case, numpy; g None: no id column."""
    rng = np.random.default_rng(7001 + 131 * PLANS[entry].index(plan) + n + len(entry))
    if entry == "rank_loss":
        both, id_digits = plan
        y = labels_of(n, rng, 0.4) if both else np.ones(n, dtype=np.int64)
        return y, rng.standard_normal(n).astype(np.float32), None if id_digits is None else ids_with(id_digits, n, rng)
    return labels_of(n, rng), scores_with(plan[0], n, rng), ids_with(plan[1], n, rng)


CASES = {(entry, plan, n): make(entry, plan, n) for entry in PLANS for plan in PLANS[entry] for n in SIZES}
PASSES = {key: passes_of(key[0], *case) for key, case in CASES.items()}


def covered(ms, digits):
    return (0 in ms and 1 in ms and digits in ms and any(m >= 2 and m % 2 == 0 for m in ms)
            and any(m >= 3 and m % 2 == 1 for m in ms))


for _entry in PLANS:  # on import: no GPU is needed to know that the inputs are what the module says
    for _n in SIZES:
        _ms = [PASSES[_entry, plan, _n] for plan in PLANS[_entry]]
        assert covered(_ms, DIGITS[_entry]), (_entry, _n, _ms)
        assert max(_ms) <= DIGITS[_entry]


def params(entry):
    return [pytest.param(plan, n, id=f"m{PASSES[entry, plan, n]}-n{n}") for plan in PLANS[entry] for n in SIZES]


def bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


# --------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.gpu
@pytest.mark.parametrize("plan,n", params("roc_auc"))
def test_roc_auc(hip_lib, plan, n):
    from recman_amd import ops

    y, s, _ = CASES["roc_auc", plan, n]

    def record(o):
        return ops.read_metric(ops.roc_auc(torch.from_numpy(s[o]).cuda(), torch.from_numpy(y[o]).cuda()))

    v, P, N, flags = record(np.arange(n))
    assert (P, N, flags) == (int(y.sum()), n - int(y.sum()), 0)
    assert abs(Fraction(v) - exact_auc(y, s)) <= Fraction(1, 10 ** 15)
    assert abs(v - skm.roc_auc_score(y, s)) <= 1e-13
    if plan[0] == 0:
        assert v == 0.5
    again = record(np.random.default_rng(n).permutation(n))
    assert bits(again[0]) == bits(v) and again[1:] == (P, N, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("plan,n", params("group_auc"))
def test_group_auc(hip_lib, plan, n):
    y, s, g = CASES["group_auc", plan, n]
    counts = gauc_ref.group_counts(y, s, g)
    exact, scored, wsum = gauc_ref.gauc_of_counts(counts, "impressions")
    (v, groups, S, W, P, flags), rows = G.run(y, s, g)
    assert rows == counts
    assert (groups, S, W, P, flags) == (len(counts), scored, wsum, int(y.sum()), 0) and scored >= 1
    G.check_value(v, exact, scored)
    if plan[0] == 0:
        assert v == 0.5
    o = np.random.default_rng(n).permutation(n)
    again, rows2 = G.run(y[o], s[o], g[o])
    assert bits(again[0]) == bits(v) and again[1:] == (groups, S, W, P, flags) and rows2 == rows


@pytest.mark.gpu
@pytest.mark.parametrize("plan,n", params("group_gain"))
def test_group_gain(hip_lib, plan, n):
    y, s, g = CASES["group_gain", plan, n]
    ex = T.reference(y, s, g)
    _, scored, wsum = ex.mean()
    (values, groups, S, W, P, flags), rows, vals = T.run(y, s, g)
    assert rows == ex.counts()
    assert (groups, S, W, P, flags) == (len(ex.ids), scored, wsum, int(y.sum()), 0) and scored >= 1
    T.check_group_values(vals, ex, T.CUTS)
    T.check_mean(values, ex)
    o = np.random.default_rng(n).permutation(n)
    again = T.run(y[o], s[o], g[o])
    assert bits(again[0][0]) + bits(again[2]) == bits(values) + bits(vals)
    assert again[0][1:] == (groups, S, W, P, flags) and again[1] == rows


@pytest.mark.gpu
@pytest.mark.parametrize("plan,n", params("rank_loss"))
def test_rank_loss(hip_lib, plan, n):
    y, s, g = CASES["rank_loss", plan, n]
    rng = np.random.default_rng(n + 5)
    case = dict(s=torch.from_numpy(s).double(), y=torch.from_numpy(y), groups=None if g is None else torch.from_numpy(g),
                dlogit_in=torch.from_numpy(rng.standard_normal(n) / n),
                loss_in=torch.from_numpy(np.abs(rng.standard_normal(1)) + 0.3).float().double())
    one_scored_group = plan[0] and not plan[1]
    tot = rank_ref.counts(case["y"], case["groups"])
    assert tot["scored_groups"] == (0 if not plan[0] else 1 if one_scored_group else tot["groups"])
    for kind in rank_ref.KINDS:
        if kind == "pairwise" and one_scored_group and n > 4097:
            continue  # (the twin's P x N matrix: see the module's docstring)
        tag = f"m{PASSES['rank_loss', plan, n]} n{n} {kind}"
        K._check(case, kind, "pairs", False, tag + " alone")
        a = K._check(case, kind, "group", True, tag + " combined")
        b = K._run(case, kind, "group", True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
