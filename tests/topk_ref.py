"""CPU float64 twin of exact top-k retrieval by inner product (include/recman_hip_topk.h, csrc/topk.hip) and the case
lists of its tests.

TEST INFRASTRUCTURE, a plain module on tests/ref_common.  Nothing in the reference implements retrieval, so the contract
is the project's own:

    s_ij   = scale <Q_i, C_j>
    order  = score descending, then catalogue row ascending; -0.0 == +0.0; NaN below every number, by row among itself
    result = the best min(k, available) rows not excluded (exclusions outside [0, N) ignored), then row -1 / -inf

`topk` is a lexsort by (NaN, -score, row); `loops` restates it as plain Python for tests/test_topk_host.py.

Cases.  EXACT: entries are multiples of 1/8 in [-1, 1] and the scale is 4, so every product is a multiple of 1/64,
every partial sum times 64 an integer below 2^24 (checked by exact_precondition) and every fp32 score exact in any
summation order: the kernel's ids AND scores must equal the twin's bit for bit.  The catalogue repeats rows and holds a
block of all-equal rows, so ties are frequent.  RISING: scores that rise with the row, so every row beats the running
threshold (the filter's worst case), exact too.  RANDOM: L2-normalised N(0, 1) rows (float32 values), scale 20, against
float64, where a boundary near tie (twotower_ref.TIE) lets ids swap within the tie.
"""
import math

import numpy as np
import torch

from tests import ref_common as C
from tests import twotower_ref as TT

EXACT_SCALE = 4.0
RANDOM_SCALE = 20.0
PAD = 12  # the GPU tests pass Q and C as column ranges of rows H + PAD floats long

# (Nq, N, H, k, item_splits)
EXACT_CASES = [(1, 1, 4, 1, 0), (1, 5, 4, 8, 0), (17, 100, 8, 10, 0), (65, 1000, 20, 100, 0), (64, 257, 64, 257, 3),
               (130, 3000, 36, 256, 7), (33, 2100, 256, 1024, 2)]
RISING_CASES = [(2, 5000, 4, 100, 1), (2, 5000, 4, 1024, 1)]
# (Nq, N, H, k)
RANDOM_CASES = [(65, 1000, 64, 100), (130, 3000, 36, 256), (200, 4000, 64, 100), (97, 2500, 128, 1000)]


# ------------------------------------------------------------------------------------------------------ the twin
def topk(S, k, exclude=None):
    """S [Nq, N] scores (float64 or float32) -> (rows int64 [Nq, k], scores [Nq, k] of S's dtype) in the contract's
    order; exclude: None or one iterable of catalogue rows per query.  Scores of zero are +0.0."""
    S = S.detach().cpu()
    Nq, N = S.shape
    rows = torch.full((Nq, k), -1, dtype=torch.int64)
    out = torch.full((Nq, k), -math.inf, dtype=S.dtype)
    ar = np.arange(N)
    for i in range(Nq):
        s = S[i].numpy()
        nan = np.isnan(s)
        order = np.lexsort((ar, np.where(nan, 0.0, -s), nan))  # the last key is the primary one
        if exclude is not None:
            ex = np.zeros(N, dtype=bool)
            r = np.asarray(list(exclude[i]), dtype=np.int64)
            ex[r[(r >= 0) & (r < N)]] = True
            order = order[~ex[order]]
        order = order[:k]
        rows[i, :len(order)] = torch.from_numpy(order)
        out[i, :len(order)] = torch.from_numpy(s[order] + 0.0)  # (+ 0.0: -0.0 becomes +0.0)
    return rows, out


def loops(S, k, exclude=None):
    """The same as plain Python: (rows, scores) as lists of lists, NaN as float('nan')."""
    res_r, res_s = [], []
    for i, row in enumerate(S.tolist()):
        ex = set() if exclude is None else set(int(r) for r in exclude[i])
        cand = [(math.isnan(s), 0.0 if math.isnan(s) else -s, j) for j, s in enumerate(row) if j not in ex]
        cand.sort()
        best = cand[:k]
        res_r.append([j for _, _, j in best] + [-1] * (k - len(best)))
        res_s.append([row[j] + 0.0 for _, _, j in best] + [-math.inf] * (k - len(best)))
    return res_r, res_s


def scores(Q, Cat, scale):
    return scale * (Q @ Cat.t())


# ------------------------------------------------------------------------------------------------------ the cases
def _eighths(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).double() / 8.0


@C.memo
def exact_case(Nq, N, H, k, seed=0):
    """Q [Nq, H], Cat [N, H] in multiples of 1/8, scale 4; every 7th row repeats its predecessor and the rows
    [N/3, N/3 + N/10) are all equal.  With the float64 twin's (rows, scores)."""
    g = torch.Generator().manual_seed(61000 + 101 * seed + 13 * N + 7 * H + Nq)
    Q, Cat = _eighths(g, Nq, H), _eighths(g, N, H)
    for j in range(1, N, 7):
        Cat[j] = Cat[j - 1]
    a, b = N // 3, N // 3 + N // 10
    if b > a:
        Cat[a:b] = Cat[a]
    S = scores(Q, Cat, EXACT_SCALE)
    rows, sc = topk(S, k)
    return dict(Q=Q, C=Cat, scale=EXACT_SCALE, k=k, S=S, rows=rows, scores=sc)


@C.memo
def rising_case(Nq, N, H, k):
    """Cat[j] = j / 8192 in every column, Q rows of positive dyadic entries: s_ij rises strictly with j, exactly."""
    assert N <= 8192
    base = torch.tensor([1.0, 0.5, 0.25, 0.125, 0.125, 1.0, 1.0, 0.5], dtype=torch.float64)
    Q = torch.stack([base.roll(i).repeat(H // 8 + 1)[:H] for i in range(Nq)])
    Cat = (torch.arange(N, dtype=torch.float64) / 8192.0).unsqueeze(1).repeat(1, H)
    S = scores(Q, Cat, EXACT_SCALE)
    rows, sc = topk(S, k)
    return dict(Q=Q, C=Cat, scale=EXACT_SCALE, k=k, S=S, rows=rows, scores=sc)


EXACT_QUANTUM = 1.0 / 64      # EXACT: every product Q_ih C_jh is a multiple of it
RISING_QUANTUM = 2.0 ** -16   # RISING: 1/8 times j / 8192


def exact_precondition(case, quantum=EXACT_QUANTUM):
    """The largest |partial sum| / quantum of any summation order of any score (bounded by sum_h |Q_ih C_jh|): below
    2^24, with every product a multiple of `quantum`, every fp32 partial sum is exact."""
    return float((case["Q"].abs() @ case["C"].abs().t()).max()) / quantum


def exclusion_lists(case, seed=0):
    """One list per query: query 0 drops rows of its top-k with a duplicate and out-of-range rows, query 1 none,
    query 2 all but 3 rows (unsorted), the others 0..5 random rows with duplicates, in random order."""
    g = torch.Generator().manual_seed(62000 + seed)
    rows, N = case["rows"], case["C"].shape[0]
    Nq = rows.shape[0]
    out = []
    for i in range(Nq):
        if i == 0:
            top = [int(r) for r in rows[0, :3]]
            out.append([top[1], -5, top[0], N, top[0], 10 ** 9] + top[2:])
        elif i == 1:
            out.append([])
        elif i == 2:
            keep = set(torch.randperm(N, generator=g)[:3].tolist())
            out.append([j for j in range(N - 1, -1, -1) if j not in keep] + [N + 3])
        else:
            n = int(torch.randint(0, 6, (1,), generator=g))
            r = torch.randint(0, N, (n,), generator=g).tolist()
            out.append(r + r[:1])
    return out


@C.memo
def random_case(Nq, N, H, k, seed=0):
    """L2-normalised N(0, 1) rows rounded to float32 values, scale 20: the float64 twin's top-k, the float64 scores
    S [Nq, N], the boundary near ties (|s_k - s_k+1| <= TIE max(1, |s_k|)) and the float32 restatement's scores."""
    rnd = C.rnd_stream(torch.Generator().manual_seed(63000 + 101 * seed + 13 * N + 7 * H + Nq))
    Q, Cat = TT.rownorm_fwd(rnd(Nq, H))[0].float().double(), TT.rownorm_fwd(rnd(N, H))[0].float().double()
    S = scores(Q, Cat, RANDOM_SCALE)
    rows, sc = topk(S, k + 1)
    kth, nxt = sc[:, k - 1], sc[:, k]
    tie = (kth - nxt).abs() <= TT.TIE * kth.abs().clamp(min=1.0)
    S32 = RANDOM_SCALE * (Q.float() @ Cat.float().t())
    return dict(Q=Q, C=Cat, scale=RANDOM_SCALE, k=k, S=S, S32=S32, rows=rows[:, :k], scores=sc[:, :k],
                boundary_tie=tie)


def tie_share(case):
    return float(case["boundary_tie"].double().mean())
