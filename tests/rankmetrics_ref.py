"""Exact host reference of the grouped top-k ranking metrics (include/recman_hip_rankmetrics.h, csrc/rankmetrics.hip).

Inside a group the examples are ordered by float32 score, descending; equal scores (-0.0 == +0.0) form a tie group T
at the 0-based ranks [lo, hi) with pos_T positives.  The discounts are doubles and are taken as exact rationals:
    gain_g(k)  = sum over T with lo < k of (pos_T / (hi - lo)) (disc[lo] + ... + disc[min(hi, k) - 1])
    value_g(k) = gain_g(k) / norm_g(k),   norm "ideal" sum_{r < min(P_g, k)} disc[r], "positives" P_g, "k" k
and value_g = 0 where the norm is 0.  Every double is a multiple of a power of two, so the table is scaled to integers
once (scaled) and a range sum is a difference of two integers; only tie groups longer than one bring a denominator.

exact() is vectorised and returns an Exact record; group_values_loop walks one group and one rank at a time in
Fractions (slow: the check of the first).  group_values and group_values_loop return [(id, n, P, [Fraction per
cutoff])] in ascending id order; Exact.mean and mean_of_values give the weighted mean over the scored groups."""
from fractions import Fraction

import numpy as np

NORMS = ("ideal", "positives", "k")
SCORED = ("both_classes", "has_positive")
WEIGHTS = ("groups", "impressions", "clicks")


def discounts(kind, kmax):
    """The table the library builds: "log2" 1 / log2(r + 2), "none" ones; float64 [kmax]."""
    if kind == "log2":
        return 1 / np.log2(np.arange(2, kmax + 2, dtype=np.float64))
    assert kind == "none"
    return np.ones(kmax, dtype=np.float64)


def scaled(disc):
    """(C, scale): C[r] = scale * (disc[0] + ... + disc[r - 1]) as Python ints in an object array, scale a power of 2."""
    fr = [Fraction(float(d)) for d in disc]
    assert all(f >= 0 for f in fr)
    scale = max(f.denominator for f in fr)  # powers of two: the largest is the common one
    c, run = [0], 0
    for f in fr:
        q = f * scale
        assert q.denominator == 1
        run += q.numerator
        c.append(run)
    return np.array(c, dtype=object), scale


def _sorted(y, s, g):
    y = np.asarray(y).astype(np.int64)
    s = np.asarray(s, dtype=np.float32)
    g = np.zeros(len(y), dtype=np.int64) if g is None else np.asarray(g).astype(np.int64)
    assert len(y) == len(s) == len(g) and 0 < len(y) < 2 ** 31
    order = np.lexsort((-s, g))  # (-0.0 and +0.0 compare equal under the sort and below)
    return y[order], s[order], g[order]


class Exact:
    """The per-group integers (ids, n, P: lists, ascending id) and, per cutoff c and group i, value = numer[c][i] /
    den[c][i] with the denominators NOT reduced: den takes few distinct values (one per min(P_g, k), P_g or k), which
    keeps the exact mean cheap.  numer entries are ints or Fractions whose denominators are tie-group lengths."""

    def __init__(self, ids, n, P, numer, den):
        self.ids, self.n, self.P, self.numer, self.den = ids, n, P, numer, den

    def value(self, c, i):
        return Fraction(self.numer[c][i]) / self.den[c][i] if self.den[c][i] else Fraction(0)

    def rows(self):
        """[(id, n, P, [value_g(k) as a Fraction per cutoff])]"""
        C = range(len(self.numer))
        return [(self.ids[i], self.n[i], self.P[i], [self.value(c, i) for c in C]) for i in range(len(self.ids))]

    def counts(self):
        return list(zip(self.ids, self.n, self.P))

    def mean(self, scored="both_classes", weight="groups"):
        """([weighted mean per cutoff as a Fraction] or None when no group is scored, scored groups, weight sum)."""
        assert weight in WEIGHTS
        w = [(1 if weight == "groups" else n if weight == "impressions" else P) if is_scored(n, P, scored) else 0
             for n, P in zip(self.n, self.P)]
        count = sum(is_scored(n, P, scored) for n, P in zip(self.n, self.P))
        if not count:
            return None, 0, 0
        out = []
        for numer, den in zip(self.numer, self.den):
            by_den = {}
            for wi, a, d in zip(w, numer, den):
                if wi and d:
                    by_den[d] = by_den.get(d, 0) + wi * a
            out.append(sum((Fraction(a) / d for d, a in by_den.items()), Fraction(0)) / sum(w))
        return out, count, sum(w)

    def scored_share(self):
        """The share of the examples that lie in groups with both classes."""
        return sum(n for n, P in zip(self.n, self.P) if 0 < P < n) / sum(self.n)


def exact(y, s, g, disc, cutoffs, norm="ideal"):
    """The Exact record of the inputs (vectorised).  g None: one group with id 0."""
    assert norm in NORMS and max(cutoffs) <= len(disc)
    y, s, g = _sorted(y, s, g)
    n = len(y)
    C, scale = scaled(disc)
    gstart = np.concatenate([[True], g[1:] != g[:-1]])
    tstart = gstart | np.concatenate([[True], s[1:] != s[:-1]])
    gpos = np.flatnonzero(gstart)                           # first position of each group
    tpos = np.flatnonzero(tstart)                           # first position of each tie group
    tgroup = np.cumsum(gstart)[tstart] - 1                  # group of each tie group
    lo = tpos - gpos[tgroup]
    length = np.diff(np.concatenate([tpos, [n]]))
    hi = lo + length
    pos = np.add.reduceat(y, tpos)
    n_g = np.diff(np.concatenate([gpos, [n]]))
    p_g = np.add.reduceat(y, gpos)
    G = len(gpos)
    numers, dens = [], []
    for k in cutoffs:
        m = (lo < k) & (pos > 0)
        span = C[np.minimum(hi, k)] - C[np.minimum(lo, k)]  # scale * the range sum, Python ints (0 where lo >= k)
        numer = np.zeros(G, dtype=object)
        one = m & (length == 1)
        np.add.at(numer, tgroup[one], span[one])
        for t in np.flatnonzero(m & (length > 1)).tolist():
            numer[tgroup[t]] += Fraction(int(pos[t]) * span[t], int(length[t]))
        if norm == "ideal":
            den = C[np.minimum(p_g, k)]
        elif norm == "positives":
            den = p_g.astype(object) * scale
        else:
            den = np.full(G, k * scale, dtype=object)
        numers.append(numer.tolist())
        dens.append(den.tolist())
    return Exact(g[gstart].tolist(), n_g.tolist(), p_g.tolist(), numers, dens)


def group_values(y, s, g, disc, cutoffs, norm="ideal"):
    """[(id, n, P, [value_g(k) as a Fraction for k in cutoffs])], ascending id."""
    return exact(y, s, g, disc, cutoffs, norm).rows()


def group_values_loop(y, s, g, disc, cutoffs, norm="ideal"):
    """group_values, one group and one rank at a time in Fractions."""
    y = np.asarray(y).astype(np.int64)
    s = np.asarray(s, dtype=np.float32)
    g = np.zeros(len(y), dtype=np.int64) if g is None else np.asarray(g).astype(np.int64)
    d = [Fraction(float(v)) for v in disc]
    out = []
    for gid in np.unique(g).tolist():
        m = g == gid
        yy, ss = y[m], s[m]
        levels = sorted(set(float(v) + 0.0 for v in ss), reverse=True)  # (+ 0.0: -0.0 becomes +0.0)
        P = int(yy.sum())
        vals = []
        for k in cutoffs:
            gain, lo = Fraction(0), 0
            for v in levels:
                tie = ss == np.float32(v)
                hi = lo + int(tie.sum())
                if lo < k:
                    gain += Fraction(int(yy[tie].sum()), hi - lo) * sum(d[lo:min(hi, k)], Fraction(0))
                lo = hi
            den = sum(d[:min(P, k)], Fraction(0)) if norm == "ideal" else Fraction(P if norm == "positives" else k)
            vals.append(gain / den if den else Fraction(0))
        out.append((int(gid), int(m.sum()), P, vals))
    return out


def is_scored(n, P, scored="both_classes"):
    assert scored in SCORED
    return 0 < P < n if scored == "both_classes" else P >= 1


def mean_of_values(rows, scored="both_classes", weight="groups"):
    """Exact.mean from rows (of either version), term by term: for small inputs."""
    assert weight in WEIGHTS
    kept = [(1 if weight == "groups" else n if weight == "impressions" else P, v) for _, n, P, v in rows
            if is_scored(n, P, scored)]
    if not kept:
        return None, 0, 0
    den = sum(w for w, _ in kept)
    return [sum((w * v[c] for w, v in kept), Fraction(0)) / den for c in range(len(kept[0][1]))], len(kept), den
