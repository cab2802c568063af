"""Exact host reference of the grouped AUC (GAUC): numpy integers per group, the weighted mean as a Fraction.

Per group g (ascending id): n_g, P_g and 2U_g = sum over its score levels of pos (2 neg_before + neg), the
Mann-Whitney count with ties one half - exact_auc of tests/test_gpu_metrics.py inside the group (np.unique of the
float32 scores, so -0.0 and +0.0 tie).  Groups with one class are left out of the mean."""
from fractions import Fraction

import numpy as np


def group_counts(y, s, g):
    """[(id, n, P, 2U)] as Python ints, ascending id.  One pass over the examples sorted by (id, score); the
    sums are int64, exact while 2 P N < 2^63, that is for every n < 2^31."""
    y = np.asarray(y).astype(np.int64)
    s = np.asarray(s, dtype=np.float32)
    g = np.asarray(g).astype(np.int64)
    assert len(y) == len(s) == len(g) and 0 < len(y) < 2 ** 31
    order = np.lexsort((s, g))
    y, s, g = y[order], s[order], g[order]
    gstart = np.concatenate([[True], g[1:] != g[:-1]])
    tstart = gstart | np.concatenate([[True], s[1:] != s[:-1]])  # (-0.0 == +0.0: one level, as np.unique)
    tie = np.cumsum(tstart) - 1                                  # level of each example
    k = int(tie[-1]) + 1
    pos = np.bincount(tie[y == 1], minlength=k)
    neg = np.bincount(tie[y == 0], minlength=k)
    first_level = tie[gstart]                                    # first level of each group
    level_group = np.cumsum(gstart)[tstart] - 1                  # group of each level
    cneg = np.cumsum(neg) - neg                                  # negatives before the level, all groups
    neg_before = cneg - cneg[first_level][level_group]           # ... inside its group
    two_u = np.add.reduceat(pos * (2 * neg_before + neg), first_level)
    n_g = np.add.reduceat(pos + neg, first_level)
    p_g = np.add.reduceat(pos, first_level)
    return list(zip(g[gstart].tolist(), n_g.tolist(), p_g.tolist(), two_u.tolist()))


def group_counts_loop(y, s, g):
    """group_counts, one group at a time with exact_auc's arithmetic in Python integers (slow: the check of
    the vectorised version)."""
    y = np.asarray(y).astype(np.int64)
    s = np.asarray(s, dtype=np.float32)
    g = np.asarray(g).astype(np.int64)
    out = []
    for gid in np.unique(g).tolist():
        m = g == gid
        yy, ss = y[m], s[m]
        _, inv = np.unique(ss, return_inverse=True)
        inv = inv.reshape(-1)
        k = int(inv.max()) + 1
        pos = np.bincount(inv[yy == 1], minlength=k).astype(object)
        neg = np.bincount(inv[yy == 0], minlength=k).astype(object)
        neg_before = np.concatenate([[0], np.cumsum(neg)[:-1]]).astype(object)
        out.append((int(gid), int(m.sum()), int(pos.sum()), int(np.sum(pos * (2 * neg_before + neg)))))
    return out


def gauc_of_counts(counts, weight="impressions"):
    """(GAUC as a Fraction or None when no group is scored, scored groups, weight sum)."""
    num, den, scored = Fraction(0), 0, 0
    for _, n, P, two_u in counts:
        N = n - P
        if P == 0 or N == 0:
            continue
        w = n if weight == "impressions" else P
        num += w * Fraction(two_u, 2 * P * N)
        den += w
        scored += 1
    return (num / den if scored else None), scored, den


def exact_gauc(y, s, g, weight="impressions"):
    """(GAUC Fraction or None, scored groups, weight sum, [(id, n, P, 2U)])."""
    counts = group_counts(y, s, g)
    return gauc_of_counts(counts, weight) + (counts,)


def scored_share(counts):
    """The share of the examples that lie in scored groups."""
    return sum(n for _, n, P, _ in counts if 0 < P < n) / sum(n for _, n, _, _ in counts)
