"""CPU: pins tests/optim_ref.py, the float64 restatement of the optimizer steps and the case builder that
tests/test_gpu_optim_kernels.py runs the kernels of csrc/optim.hip on.

  * the float64 restatement equals recman_amd.optim.Optimizer (plain torch) on the densified gradient while every
    row is touched every step, and differs for Adam in exactly the row a step leaves out (lazy state);
  * the builder's cases hold every run length and placement the GPU file relies on;
  * the GPU file's bounds (optim_ref.compare) catch four deliberately wrong restatements on every case that has the
    runs or terms they touch, and pass the plain float32 restatement.
"""
from collections import Counter

import pytest
import torch

from recman_amd.optim import Optimizer
from tests import optim_ref as R

F32, F64 = torch.float32, torch.float64


def test_restated_constants_are_the_kernels():
    """K_LONG, K_SEG, K_POS, K_FLIGHT and the dense grid cap, read from the source text of csrc/optim.hip."""
    k = R.kernel_constants()
    assert (k["kLong"], k["kSeg"], k["kPos"], k["kLongFlight"]) == (R.K_LONG, R.K_SEG, R.K_POS, R.K_FLIGHT)
    assert k["dense_grid_cap"] == R.DENSE_GRID_CAP and k["kBlock"] == R.K_BLOCK


def _every_row_case(kind, leave_out=None):
    """Three steps over 9 rows in 3 fields; every row occurs in every step, except row `leave_out` in step 2."""
    sizes, B = [3, 4, 2], 40
    g = torch.Generator().manual_seed(5)
    steps = []
    for s in range(3):
        ids = torch.stack([torch.randint(0, v, (B,), generator=g) for v in sizes], 1)
        for f, v in enumerate(sizes):
            ids[:v, f] = torch.arange(v)
        if s == 1 and leave_out is not None:
            ids[:, 0] = ids[:, 0].clamp(min=1)
        steps.append(ids)
    return R.assemble(8, kind, "pairs", sizes, steps, seed=3, prepared_at=())


def _optimizer_on_dense_grads(case):
    """recman_amd.optim.Optimizer, in float64 on the CPU, on the densified gradient of every step."""
    D, kind = case["D"], case["kind"]
    P = {"t": case["rows0"][:, : D + 2].double().clone()}
    opt = Optimizer(kind, case["lr"])
    if kind == "adagrad":  # (the same starting accumulator as the case's state: the float32 number 0.1f)
        opt.state["t"] = torch.full_like(P["t"], R.f32(0.1))
    for s in range(len(case["steps"])):
        rows = R.occurrence_rows(case, s)
        G = torch.zeros_like(P["t"]).index_add_(0, rows, R.occurrence_grads(case, s).double())
        opt.step(P, {"t": G})
    return P["t"]


@pytest.mark.parametrize("kind", R.KINDS)
def test_float64_reference_equals_the_dense_optimizer_when_every_row_is_touched(kind):
    case = _every_row_case(kind)
    want = _optimizer_on_dense_grads(case)
    got = R.reference(case, F64, f32_hyper=False)[-1][0]
    assert float((got - want).abs().max()) <= 1e-12
    assert float((got - case["rows0"][:, : case["D"] + 2].double()).abs().max()) > 1e-3
    # the float32-rounded hyper-parameters are another computation: beta2 alone moves v by a relative 1.29e-5
    if kind == "adam":
        v64, v32h = R.reference(case, F64, f32_hyper=False)[0][2], R.reference(case, F64)[0][2]
        rel = float(((v64 - v32h).abs() / v64.abs()).max())
        assert 1.2e-5 < rel < 1.4e-5, rel


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_row_left_out_differs_for_adam_in_that_row_only(kind):
    case = _every_row_case(kind, leave_out=0)
    assert 0 not in R.occurrence_rows(case, 1).tolist() and 0 in R.occurrence_rows(case, 0).tolist()
    want = _optimizer_on_dense_grads(case)
    got = R.reference(case, F64, f32_hyper=False)[-1][0]
    assert float((got[1:] - want[1:]).abs().max()) <= 1e-12
    d0 = float((got[0] - want[0]).abs().max())
    if kind == "adam":   # Keras decays m, v of the row and moves it on its momentum; the lazy step leaves it alone
        assert d0 > 1e-5
    else:                # a zero gradient moves nothing under Adagrad / SGD
        assert d0 <= 1e-12


def test_moment_layout_round_trips():
    g = torch.Generator().manual_seed(0)
    for D in R.WIDTHS:
        m, v = torch.randn(5, D, generator=g), torch.randn(5, D, generator=g)
        mom = R.interleave(m, v)
        assert mom.shape == (5, 2 * D)
        assert torch.equal(mom[:, 0:4], m[:, 0:4]) and torch.equal(mom[:, 4:8], v[:, 0:4])
        assert torch.equal(mom[:, 2 * D - 4:], v[:, D - 4:]) and torch.equal(mom[:, 2 * D - 8: 2 * D - 4], m[:, D - 4:])
        m2, v2 = R.deinterleave(mom, D)
        assert torch.equal(m2, m) and torch.equal(v2, v)
        rows = torch.randn(5, 2 * D, generator=g)
        p, ms, vs = R.state_of(rows, mom, D, "adam")
        assert torch.equal(p, rows[:, : D + 2].double())
        assert torch.equal(ms, torch.cat([m, rows[:, D + 2: D + 4]], 1).double())
        assert torch.equal(vs, torch.cat([v, rows[:, D + 4: D + 6]], 1).double())


def test_lane_groups_of_every_width():
    assert {D: R.group_lanes(D) for D in R.WIDTHS} == {
        8: (4, 2, 16), 12: (8, 3, 8), 16: (8, 4, 8), 24: (8, 6, 8), 32: (16, 8, 4), 48: (16, 12, 4), 64: (32, 16, 2)}


# ------------------------------------------------------------------------------------------ the builder's conditions
def _layout_key(kw):
    return (kw["entry"], kw.get("tail", "long"), kw.get("skip_share", 0.06))


LAYOUTS = sorted({_layout_key(kw) for kw in R.ALL_CASES.values()})


def test_every_gpu_case_uses_a_checked_layout_and_the_ids_do_not_depend_on_the_width():
    assert len(LAYOUTS) == 9 and len(R.SPARSE_CASES) == 63
    assert {(kw["D"], kw["kind"], kw["entry"]) for kw in R.SPARSE_CASES.values()} == {
        (D, k, e) for D in R.WIDTHS for k in R.KINDS for e in R.ENTRIES}
    a, b = R.make_case(8, "sgd", "fields"), R.make_case(64, "adam", "fields", l2_emb=0.5, ld=72)
    for s in range(3):
        assert torch.equal(a["steps"][s]["idx"], b["steps"][s]["idx"])


@pytest.mark.parametrize("entry,tail,skip_share", LAYOUTS)
def test_builder_places_every_run_the_kernels_branch_on(entry, tail, skip_share):
    case = R.make_case(8, "adam", entry, tail=tail, skip_share=skip_share)
    Rn, n = case["R"], R.sorted_keys(case, 0).numel()
    keys = R.sorted_keys(case, 0)
    runs = R.runs_of(keys, Rn)
    hist = Counter(L for _, L, _ in runs)
    print(f"{entry} {tail} skip {skip_share}: n = {n}, R = {Rn}, {len(runs)} runs, lengths {sorted(hist.items())}")
    assert 8000 >= n >= 6000 and 100 <= Rn <= 400
    for L in R.RUN_LENGTHS:
        assert hist[L] >= 1, L
    for L in (1, 2, 17, 129):   # kPos = 2: a run starts at the first and at the second position of a lane group
        assert {i % 2 for i, ln, _ in runs if ln == L} == {0, 1}, L
    touched = {r for _, _, r in runs}
    assert 0 in touched and Rn - 1 in touched and len(touched) < Rn   # (and some rows no step-1 occurrence names)
    assert {R.cdiv(L, R.K_SEG) for L in hist if L > R.K_LONG} == {1, 2, 3, 4, 5, 6, 8, 9}
    skipped = float((keys == Rn).double().mean())
    last = runs[-1]
    if skip_share == 0.0:
        assert skipped == 0.0 and last[0] + last[1] == n   # the list ENDS with a run
        if tail == "long":
            assert last[1] > R.K_LONG                       # the gallop runs into t >= n
        else:
            assert 2 <= last[1] <= R.K_LONG                 # the inline count stops at i + len < n
    else:
        assert skipped >= 0.05
        # a run of several segments directly followed by skipped keys
        assert any(L >= 129 and i + L < n and int(keys[i + L]) == Rn for i, L, _ in runs)
        raw = case["steps"][0]["ids"] if entry == "rows" else case["steps"][0]["idx"]
        if entry == "rows":
            assert bool((raw == -1).any()) and bool((raw >= Rn).any())
        if entry == "fields":   # an id that is a row of the largest field, and not of its own
            sizes = torch.tensor(case["sizes"])
            assert bool(((raw >= sizes[None, :]) & (raw < int(sizes.max()))).any())
            for f in range(case["F"]):   # field f's block: its rows ascending, its skipped ids at the end
                blk = keys[f * R.B_FULL: (f + 1) * R.B_FULL]
                assert bool((blk[1:] >= blk[:-1]).all()) and int(blk[-1]) == Rn
                assert int(blk[0]) >= int(case["foff"][f])
    # step 2: other ids, no run the long-run kernels would take, rows of step 1 left out; step 3: step 1's ids
    k2 = R.sorted_keys(case, 1)
    runs2 = R.runs_of(k2, Rn)
    assert k2.numel() % 2 == 1                              # (and an odd n: the last lane group has one position)
    assert max(L for _, L, _ in runs2) == R.K_LONG
    t2 = {r for _, _, r in runs2}
    assert len(touched - t2) >= 10 and len(t2 & touched) >= 10
    assert torch.equal(R.occurrence_rows(case, 2), R.occurrence_rows(case, 0))
    assert not torch.equal(case["steps"][2]["d_rows"], case["steps"][0]["d_rows"])
    assert case["prepared_at"] == (2,)
    # occurrence order is not row order
    rows0 = R.occurrence_rows(case, 0)
    assert not bool((rows0[1:] >= rows0[:-1]).all())


def test_builder_takes_the_run_lengths_as_a_list():
    case = R.make_case(8, "sgd", "pairs", run_lengths=R.RUN_LENGTHS + (40, 300))
    hist = Counter(L for _, L, _ in R.runs_of(R.sorted_keys(case, 0), case["R"]))
    assert all(hist[L] >= 1 for L in R.RUN_LENGTHS + (40, 300))
    assert 300 not in Counter(L for _, L, _ in R.runs_of(R.sorted_keys(R.make_case(8, "sgd", "pairs"), 0), case["R"]))


def test_entries_hold_the_same_occurrences():
    for D in R.WIDTHS:   # (optim_ref shares the float32 sums of a width among its entries on the strength of this)
        cases = [R.make_case(D, "adam", e) for e in R.ENTRIES]
        for s in range(3):
            for c in cases[1:]:
                assert torch.equal(R.occurrence_rows(c, s), R.occurrence_rows(cases[0], s))
                assert torch.equal(R.occurrence_grads(c, s), R.occurrence_grads(cases[0], s))
    wide = R.make_case(12, "adam", "rows", gw=20)
    assert wide["steps"][0]["packed"].shape[1] == 20
    assert torch.equal(R.occurrence_grads(wide, 0), R.occurrence_grads(R.make_case(12, "adam", "rows"), 0))


@pytest.mark.parametrize("which", ["n1", "n2_same_row", "n_odd", "all_skipped", "empty"])
def test_smallest_cases(which):
    for entry in R.ENTRIES:
        case = R.small_case(which, 12, "adam", entry)
        rows = R.occurrence_rows(case, 0)
        want = {"n1": 1, "n2_same_row": 2, "n_odd": 15, "all_skipped": 18, "empty": 0}[which]
        assert rows.numel() == want
        if which == "n2_same_row":
            assert rows[0] == rows[1] >= 0
        if which == "all_skipped":
            assert bool((rows < 0).all())
        p0 = case["rows0"][:, :14].double()
        p = R.reference(case)[0][0]
        touched = torch.zeros(case["R"], dtype=torch.bool)
        touched[rows[rows >= 0]] = True
        assert torch.equal(p[~touched], p0[~touched])
        if touched.any():
            assert float((p[touched] - p0[touched]).abs().min()) > 0


# -------------------------------------------------------------------------------------------- the bounds have teeth
def _failures(case, want, ref32, got):
    bad = []
    for s in range(len(want)):
        bad += [(s,) + q for q in R.compare(got[s], want[s], ref32[s], case["D"], show=False)]
    return bad


def _applies(mutation, kw):
    if mutation == "no_l2":
        return bool(kw.get("l2_emb") or kw.get("l2_lin"))
    if mutation == "neighbour_v":
        return kw["kind"] != "sgd"
    return True   # every full case has runs beyond K_LONG and beyond K_SEG


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_bounds_catch_every_wrong_restatement(name):
    kw = R.ALL_CASES[name]
    case = R.make_case(**kw)
    want, ref32 = R.reference(case, F64), R.reference(case, F32)
    for s in range(3):
        R.compare(ref32[s], want[s], ref32[s], case["D"], tag=f"{name} step {s + 1} (float32 restatement)")
    assert _failures(case, want, ref32, ref32) == []
    for mutation in R.MUTATIONS:
        if not _applies(mutation, kw):
            continue
        bad = _failures(case, want, ref32, R.reference(case, F32, mutate=mutation))
        assert bad, f"{name}: {mutation} passes the bounds"
        if mutation == "drop_last" and kw["kind"] == "adam":
            # at t = 1 Adam's update is ~ lr sign(G), nearly blind to a lost member: the moments show it at once
            assert any(s == 0 and q.startswith("v") for s, q, *_ in bad)
