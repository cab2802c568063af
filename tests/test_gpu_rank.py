"""GPU: rm_rank_loss through the C ABI (recman_amd.ops) against the float64 twin (tests/rank_ref.py, pinned on the CPU
by tests/test_rank_host.py).

Tolerance, the convention of tests/test_gpu_asp.py: for dlogit and for the loss the gradient measure of
tests/test_gpu_parity.py against float64 must be <= max(2e-5, 4 x the float32 CPU restatement's own measure on the
case); both numbers are printed.  Every case runs twice: the ranking term alone (alpha 1, no dlogit_in / loss_in) and
combined (alpha 0.3, grad_scale 0.25, dlogit_in aliased with dlogit_out, loss_in with loss_out).

COVERED is the stale-state ledger of include/recman_hip_rank.h: per entry point with a stream, the test here that
runs it under tests/stale_state.py's lds_pattern (checked without a GPU by tests/test_rank_host.py)."""
import numpy as np
import pytest
import torch

from tests import rank_ref as R
from tests import stale_state as S
from tests.stale_state import lds_pattern  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64
COMBOS = [(k, n) for k in R.KINDS for n in R.NORMS]
COVERED = {"rm_rank_loss": "test_result_is_independent_of_stale_lds_and_workspace"}
BAD_LABEL, BAD_SCORE, BAD_GROUP = 1, 2, 16  # RM_METRIC_* of include/recman_hip.h


def _run(case, kind, norm, combined, workspace=None, record=True):
    """-> (dlogit [B], loss [1], record tuple or None) of one call; combined: alpha 0.3, grad_scale 0.25, the
    pointwise parts in the output buffers (aliased); else the ranking term alone."""
    from recman_amd import ops

    s, y = case["s"].to(F32).cuda(), case["y"].cuda()
    groups = None if case["groups"] is None else case["groups"].cuda()
    out = torch.full((8,), -1, dtype=I64, device="cuda")[:7] if record else None
    if combined:
        d, loss = case["dlogit_in"].to(F32).cuda(), case["loss_in"].to(F32).cuda()
        ops.rank_loss(s, y, groups, kind, norm, 0.3, d, grad_scale=0.25, dlogit_in=d, loss_in=loss, loss_out=loss,
                      out=out, workspace=workspace)
    else:
        d, loss = S.poisoned(s.shape[0]), S.poisoned(1)
        ops.rank_loss(s, y, groups, kind, norm, 1.0, d, loss_out=loss, out=out, workspace=workspace)
    torch.cuda.synchronize()
    return d, loss, (ops.read_rank_loss(out) if record else None)


def _twin(case, kind, norm, combined, dtype=torch.float64):
    s = case["s"].to(dtype)
    if combined:
        loss, d, _ = R.combine(s, case["y"], case["groups"], kind, norm, 0.3, 0.25, case["dlogit_in"].to(dtype),
                               case["loss_in"].to(dtype))
    else:
        loss, d, _ = R.combine(s, case["y"], case["groups"], kind, norm, 1.0)
    return d, loss.reshape(1)


def _check(case, kind, norm, combined, tag):
    d, loss, rec = _run(case, kind, norm, combined)
    (wd, wl), (cd, cl) = _twin(case, kind, norm, combined), _twin(case, kind, norm, combined, F32)
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(loss).all()), f"{tag}: not finite"
    for name, got, want, c32 in (("dlogit", d, wd, cd), ("loss", loss, wl, cl)):
        m, m32 = R.C.grad_measure(got, want), R.C.grad_measure(c32, want)
        bound = max(2e-5, 4 * m32)
        print(f"{tag}: {name} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        assert m <= bound, f"{tag}: {name} measure {m:.3e} > {bound:.3e} (float32 CPU {m32:.3e})"
    tot = R.counts(case["y"], case["groups"])
    assert rec[1:6] == (tot["groups"], tot["scored_groups"], tot["pairs"], tot["pos"], tot["weight"]), (rec, tot)
    assert rec[6] == 0
    L = float(R.rank_term(case["s"], case["y"], case["groups"], kind, norm))
    assert abs(rec[0] - L) <= max(2e-5, 4 * R.C.grad_measure(cl, wl)) * abs(L), (rec[0], L)
    return d, loss, rec


@pytest.mark.parametrize("kind,norm", COMBOS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_rank_loss_matches_float64(hip_lib, name, kind, norm):
    case = R.make_case(name)
    for combined in (False, True):
        _check(case, kind, norm, combined, f"{name} {kind}/{norm} {'combined' if combined else 'alone'}")


@pytest.mark.parametrize("kind,norm", COMBOS)
def test_unscored_groups_get_exactly_plus_zero(hip_lib, kind, norm):
    """Every group single-class (and B = 1): dL/ds is +0.0 in every bit, L is 0, and the combined loss is the pointwise
    part's share, rounded once."""
    for name in ("single_class_groups", "b1"):
        case = R.make_case(name)
        d, loss, rec = _run(case, kind, norm, False)
        assert torch.equal(d.view(torch.int32), torch.zeros_like(d, dtype=torch.int32)), name  # +0.0, not -0.0
        assert float(loss) == 0.0 and rec[0] == 0.0 and rec[2:6] == (0, 0, 0, 0)
        d, loss, _ = _run(case, kind, norm, True)
        a = np.float32(0.3)
        l_in, d_in = case["loss_in"].to(F32).numpy(), case["dlogit_in"].to(F32).numpy()
        want_loss = np.float32((1.0 - np.float64(a)) * np.float64(l_in[0]))
        assert loss.cpu().numpy().view(np.int32)[0] == want_loss.view(np.int32), name
        want_d = np.float32(0.25) * ((np.float32(1) - a) * d_in + a * np.float32(0))
        assert np.array_equal(d.cpu().numpy().view(np.int32), want_d.astype(np.float32).view(np.int32)), name


@pytest.mark.parametrize("norm", R.NORMS)
def test_tied_logits_in_closed_form(hip_lib, norm):
    """Gradient -/+ 0.5 c_g per pair, loss log 2 per pair - exact up to the rounding of c_g and of the sums."""
    case = R.make_case("tied_logits")
    d, loss, rec = _run(case, "pairwise", norm, False)
    tot = R.counts(case["y"], case["groups"])
    want = torch.zeros_like(case["s"])
    for pos, neg in R.split(case["y"], case["groups"]):
        P, N = len(pos), len(neg)
        if P and N:
            c = R.coef("pairwise", norm, P, N, tot)
            want[pos], want[neg] = -0.5 * c * N, 0.5 * c * P
    assert float((d.cpu().double() - want).abs().max()) <= 2e-7 * float(want.abs().max())
    total = sum(R.coef("pairwise", norm, len(p), len(n), tot) * len(p) * len(n) for p, n in
                R.split(case["y"], case["groups"]) if len(p) and len(n)) * R.LN2
    # (log1pf within an ulp, at most 8 float32 additions per tile, one final rounding: below 10 x 2^-24 = 6e-7)
    assert abs(float(loss) - total) <= 1e-6 * total and abs(rec[0] - total) <= 1e-6 * total


@pytest.mark.parametrize("kind,norm", COMBOS)
@pytest.mark.parametrize("name", ["sizes_1_to_5_b1000", "group_300_across_a_tile_edge", "group_700_among_singletons",
                                  "no_ids_b777"])
def test_two_runs_are_bit_equal(hip_lib, name, kind, norm):
    case = R.make_case(name)
    a, b = _run(case, kind, norm, True), _run(case, kind, norm, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("kind,norm", COMBOS)
@pytest.mark.parametrize("name", ["sizes_1_to_5_b1000", "group_700_among_singletons"])
def test_a_permuted_input_agrees(hip_lib, name, kind, norm):
    case = R.make_case(name)
    B = case["s"].shape[0]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(11))
    moved = {k: (v[perm] if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for k, v in case.items()}
    d, loss, rec = _run(case, kind, norm, True)
    dp, lossp, recp = _run(moved, kind, norm, True)
    want = _twin(case, kind, norm, True)[0]
    m = R.C.grad_measure(dp.cpu().double(), d.cpu().double()[perm])
    bound = max(2e-5, 4 * R.C.grad_measure(_twin(case, kind, norm, True, F32)[0], want))
    print(f"{name} {kind}/{norm}: permuted against plain {m:.2e}, bound {bound:.2e}")
    assert m <= bound and rec[1:] == recp[1:]
    assert abs(float(loss) - float(lossp)) <= 2e-5 * abs(float(loss))


def test_each_flag_is_raised_by_its_bad_input(hip_lib):
    base = R.make_case("sizes_1_to_5_b1000")
    B = base["s"].shape[0]

    def flags(**kw):
        case = dict(base, **{k: v.clone() for k, v in kw.items()})
        d, loss, rec = _run(case, "pairwise", "group", False)
        assert d.shape == (B,)
        return rec[6]

    assert flags() == 0
    y = base["y"].clone()
    y[17] = 2
    assert flags(y=y) == BAD_LABEL
    y[17] = -1
    assert flags(y=y) == BAD_LABEL
    for bad in (float("nan"), float("inf")):
        s = base["s"].clone()
        s[B - 1] = bad
        assert flags(s=s) == BAD_SCORE
    for bad in (-1, 2 ** 32):
        g = base["groups"].clone()
        g[0] = bad
        assert flags(groups=g) == BAD_GROUP
    g = base["groups"].clone()
    g[0], y[3] = -5, 7
    assert flags(groups=g, y=y) == BAD_GROUP | BAD_LABEL


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", ["group_300_across_a_tile_edge", "no_ids_b777", "b1"])
def test_workspace_contract(hip_lib, name, kind):
    """Nothing is written past rm_rank_loss_workspace(B) bytes, and what the workspace holds on entry (NaN bytes, all
    ones, zeros) does not matter."""
    from recman_amd import ops

    case = R.make_case(name)
    need = ops.rank_loss_workspace(case["s"].shape[0])
    assert need % 4 == 0
    results = []
    for fill in (float("nan"), 0.0, -1.0):
        view, buf = S.guarded(need // 4, fill)
        if fill == -1.0:
            view.view(torch.int32).fill_(-1)  # every bit set
        results.append(S.snapshot(_run(case, kind, "group", True, workspace=view)[:2]))
        S.assert_guards_intact(buf, f"{name} {kind}")
    for r in results[1:]:
        S.same_bits(results[0], r, f"{name} {kind}: stale workspace contents")


@pytest.mark.parametrize("kind", R.KINDS)
def test_result_is_independent_of_stale_lds_and_workspace(hip_lib, lds_pattern, kind):  # noqa: F811
    from recman_amd import ops

    case = R.make_case("group_300_across_a_tile_edge")
    need = ops.rank_loss_workspace(case["s"].shape[0])
    want = [_twin(case, kind, "group", True), _twin(case, kind, "group", True, F32)]

    def run():
        view, buf = S.guarded(need // 4)
        d, loss, rec = _run(case, kind, "group", True, workspace=view)
        S.assert_guards_intact(buf, kind)
        return dict(dlogit=d, loss=loss, record=list(rec))

    def check(res):
        for key, i in (("dlogit", 0), ("loss", 1)):
            m, m32 = R.C.grad_measure(res[key], want[0][i]), R.C.grad_measure(want[1][i], want[0][i])
            assert m <= max(2e-5, 4 * m32), (key, m, m32)

    S.run_patterns(run, check, f"rm_rank_loss {kind}: ")
    assert lds_pattern["seen"] == {"rm_rank_loss"} and lds_pattern["fills"] == 4
