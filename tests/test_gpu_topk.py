"""GPU: rm_topk_ip (csrc/topk.hip) through recman_amd.ops against the float64 twin of tests/topk_ref.py.

EXACT and RISING cases (every fp32 score exact in any summation order): ids and scores bit for bit equal to the twin,
the same bits at every item_splits and on every run.  Exclusions and NaN scores on exact cases.  RANDOM cases
(L2-normalised rows, scale 20): ids equal to the twin's except within a near tie (twotower_ref.TIE), scores within
twotower_ref.bound() of the float32 restatement's own error.  Q and C are always column ranges of rows PAD floats
longer whose pad columns hold NaN (a kernel that reads them poisons its scores); the outputs are column ranges too, and
the columns past k must stay untouched.

COVERED is this module's part of the stale-LDS ledger (tests/test_gpu_stale_lds.py keeps the one of recman_hip.h):
every entry point of include/recman_hip_topk.h with an rm_stream_t stream, with the test here that runs it under
tests/stale_state.py's lds_pattern (checked without a GPU by tests/test_topk_host.py).
"""
import math

import pytest
import torch

from tests import topk_ref as R
from tests import twotower_ref as TT
from tests.stale_state import assert_guards_intact, guarded, lds_pattern, padded, run_patterns  # noqa: F401

gpu = pytest.mark.gpu
COVERED = {"rm_topk_ip": "test_stale_lds"}
ROW_SENTINEL = -777  # what out_rows holds before a call


def _exclusions(lists):
    offsets = [0]
    for r in lists:
        offsets.append(offsets[-1] + len(r))
    rows = [int(x) for r in lists for x in r]
    return (torch.tensor(offsets, dtype=torch.int64, device="cuda"),
            torch.tensor(rows, dtype=torch.int64, device="cuda"))


def _run(case, splits=0, exclude=None, workspace=None, C=None):
    """One call -> dict(rows, scores) [Nq, k] device views of outputs 4 columns wider than k (rows_buf, scores_buf)."""
    from recman_amd import ops

    Q, _ = padded(case["Q"].float(), R.PAD)
    Cv, _ = padded((case["C"] if C is None else C).float(), R.PAD)
    Nq, N, H, k = Q.shape[0], Cv.shape[0], Q.shape[1], case["k"]
    rows_buf = torch.full((Nq, k + 4), ROW_SENTINEL, dtype=torch.int64, device="cuda")
    scores_buf = torch.full((Nq, k + 4), float("nan"), dtype=torch.float32, device="cuda")
    ws = workspace if workspace is not None else \
        torch.empty(ops.topk_ip_workspace(Nq, N, H, k), dtype=torch.float32, device="cuda")
    ex = None if exclude is None else _exclusions(exclude)
    ops.topk_ip(Q, Cv, k, case["scale"], rows_buf[:, :k], scores_buf[:, :k], ws, exclude=ex, item_splits=splits)
    return dict(rows=rows_buf[:, :k], scores=scores_buf[:, :k], rows_buf=rows_buf, scores_buf=scores_buf)


def _pads_untouched(out, k, what):
    assert bool((out["rows_buf"][:, k:] == ROW_SENTINEL).all()), f"{what}: out_rows written past column k"
    assert bool(torch.isnan(out["scores_buf"][:, k:]).all()), f"{what}: out_scores written past column k"


def _bits(t):
    return t.detach().cpu().contiguous().float().view(torch.int32)


def _check_exact(out, rows, scores, what):
    """ids equal, scores bit-equal (NaN where the twin has NaN)."""
    got_r, got_s = out["rows"].cpu(), out["scores"].cpu()
    if not torch.equal(got_r, rows):
        bad = (got_r != rows).nonzero()[0].tolist()
        raise AssertionError(f"{what}: rows differ first at {bad}: {got_r[bad[0], bad[1]].item()} against "
                             f"{rows[bad[0], bad[1]].item()}")
    want = scores.float()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got_s), nan), f"{what}: NaN scores in other places"
    assert torch.equal(_bits(got_s)[~nan], _bits(want)[~nan]), f"{what}: scores differ in their bits"


def _max_splits(H):
    from recman_amd import ops

    return ops.topk_ip_tile(H, "max_splits")


# ------------------------------------------------------------------------------------------- 1. exact arithmetic
@gpu
@pytest.mark.parametrize("Nq,N,H,k,splits", R.EXACT_CASES)
def test_exact_bits_against_the_twin(hip_lib, Nq, N, H, k, splits):
    case = R.exact_case(Nq, N, H, k)
    out = _run(case, splits)
    torch.cuda.synchronize()
    what = f"exact Nq={Nq} N={N} H={H} k={k} splits={splits}"
    _check_exact(out, case["rows"], case["scores"], what)
    _pads_untouched(out, k, what)
    if N < k:
        assert bool((out["rows"][:, N:] == -1).all()) and bool((out["scores"][:, N:] == -math.inf).all())


# ------------------------------------------------------------------------------- 2. split invariance, determinism
@gpu
@pytest.mark.parametrize("Nq,N,H,k,splits", R.EXACT_CASES)
def test_every_split_count_gives_the_same_bits(hip_lib, Nq, N, H, k, splits):
    case = R.exact_case(Nq, N, H, k)
    first = None
    for s in (1, 2, 0, _max_splits(H)):
        for run in range(2):
            out = _run(case, s)
            torch.cuda.synchronize()
            snap = (out["rows"].cpu(), _bits(out["scores"]))
            if first is None:
                first = snap
                _check_exact(out, case["rows"], case["scores"], f"exact {Nq}x{N} splits={s}")
            assert torch.equal(snap[0], first[0]) and torch.equal(snap[1], first[1]), \
                f"Nq={Nq} N={N} H={H} k={k}: splits={s} run {run} differs from splits=1"


# ----------------------------------------------------------------------------------- 3. the filter's worst case
@gpu
@pytest.mark.parametrize("Nq,N,H,k,splits", R.RISING_CASES)
def test_rising_catalogue_cuts_the_list_most_often(hip_lib, Nq, N, H, k, splits):
    case = R.rising_case(Nq, N, H, k)
    out = _run(case, splits)
    torch.cuda.synchronize()
    assert int(case["rows"][0, 0]) == N - 1
    _check_exact(out, case["rows"], case["scores"], f"rising N={N} k={k}")


# ---------------------------------------------------------------------------------------------- 4. exclusions
@gpu
@pytest.mark.parametrize("Nq,N,H,k,splits", [(17, 100, 8, 10, 0), (65, 1000, 20, 100, 3)])
def test_exclusions(hip_lib, Nq, N, H, k, splits):
    case = R.exact_case(Nq, N, H, k)
    lists = R.exclusion_lists(case)
    rows, scores = R.topk(case["S"], k, lists)
    assert int((rows[2] >= 0).sum()) == 3 and not set(rows[0, :3].tolist()) & set(lists[0])
    for s in (splits, 1):
        out = _run(case, s, exclude=lists)
        torch.cuda.synchronize()
        what = f"exclusions Nq={Nq} N={N} splits={s}"
        _check_exact(out, rows, scores, what)
        _pads_untouched(out, k, what)
    assert bool((out["rows"][2, 3:] == -1).all()) and bool((out["scores"][2, 3:] == -math.inf).all())


# ------------------------------------------------------------------------------------------------------- 5. NaN
@gpu
@pytest.mark.parametrize("N,k", [(200, 10), (40, 64)])
def test_a_nan_row_ranks_last(hip_lib, N, k):
    case = dict(R.exact_case(9, N, 8, k))
    Cn = case["C"].clone()
    Cn[37, 2] = float("nan")
    S = R.scores(case["Q"], Cn, case["scale"])
    rows, scores = R.topk(S, k)
    for s in (0, 1, 3):
        out = _run(case, s, C=Cn)
        torch.cuda.synchronize()
        _check_exact(out, rows, scores, f"NaN row N={N} k={k} splits={s}")
        got = out["rows"].cpu()
        if k < N:
            assert not bool((got == 37).any())
        else:
            assert bool((got[:, N - 1] == 37).all()) and bool(torch.isnan(out["scores"][:, N - 1]).all())
            assert bool((got[:, N:] == -1).all())
            assert _bits(out["scores"][:, N - 1]).eq(0x7FC00000).all()


# ----------------------------------------------------------------------------------- 6. random rows, float64
def _check_random(out, case, what):
    """ids: equal to the twin's, except that a position may hold another row whose float64 score is within a near
    tie of the twin's there; on a query without a boundary near tie the sets are equal.  Scores: within
    twotower_ref.bound() of the float32 restatement's own error."""
    got_r, got_s = out["rows"].cpu(), out["scores"].cpu()
    want_r, S = case["rows"], case["S"]
    Nq, k = want_r.shape
    share = R.tie_share(case)
    print(f"{what}: boundary near-tie share {share:.3f}")
    assert share <= TT.TIE_SHARE
    s_got = torch.gather(S, 1, got_r.clamp(min=0))
    s_want = torch.gather(S, 1, want_r)
    assert bool((got_r >= 0).all()), f"{what}: padding where N > k"
    swap = got_r != want_r
    near = (s_got - s_want).abs() <= TT.TIE * s_want.abs().clamp(min=1.0)
    assert bool((~swap | near).all()), f"{what}: a row differs from the twin's beyond a near tie"
    for i in range(Nq):
        assert len(set(got_r[i].tolist())) == k, f"{what}: query {i} returns a row twice"
        if not bool(case["boundary_tie"][i]):
            assert set(got_r[i].tolist()) == set(want_r[i].tolist()), f"{what}: query {i} has other rows"
    m = TT.grad_measure(got_s, s_got)
    f32 = TT.grad_measure(torch.gather(case["S32"], 1, want_r), s_want)
    print(f"{what}: {int(swap.sum())} swapped places, score measure {m:.2e}, float32 CPU {f32:.2e}, "
          f"bound {TT.bound(f32):.2e}")
    assert m <= TT.bound(f32), f"{what}: scores {m:.3e} > {TT.bound(f32):.3e}"


@gpu
@pytest.mark.parametrize("Nq,N,H,k", R.RANDOM_CASES)
def test_random_rows_against_float64(hip_lib, Nq, N, H, k):
    case = R.random_case(Nq, N, H, k)
    out = _run(case)
    torch.cuda.synchronize()
    what = f"random Nq={Nq} N={N} H={H} k={k}"
    _check_random(out, case, what)
    _pads_untouched(out, k, what)


# ------------------------------------------------------------------------------------------------ 7. stale state
@gpu
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_stale_lds(lds_pattern, kind):
    from recman_amd import ops

    if kind == "exact":
        Nq, N, H, k, splits = R.EXACT_CASES[0]
        case = R.exact_case(Nq, N, H, k)
    else:
        (Nq, N, H, k), splits = R.RANDOM_CASES[0], 0
        case = R.random_case(Nq, N, H, k)
    ws, buf = guarded(ops.topk_ip_workspace(Nq, N, H, k))

    def run():
        return _run(case, splits, workspace=ws)

    def check(out):
        what = f"stale {kind}"
        if kind == "exact":
            _check_exact(out, case["rows"], case["scores"], what)
        else:
            _check_random(out, case, what)
        _pads_untouched(out, k, what)

    run_patterns(run, check, f"topk {kind}: ")
    assert_guards_intact(buf, f"topk {kind}")
    assert set(e for e, t in COVERED.items() if t == "test_stale_lds") <= lds_pattern["seen"]
    assert lds_pattern["fills"] > 0
