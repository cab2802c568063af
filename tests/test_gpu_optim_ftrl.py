"""GPU: FTRL-Proximal (kind 3) and the two-rule row-wise step of csrc/optim.hip against the float64 restatement of
tests/optim_ftrl_ref.py (pinned without a GPU by tests/test_optim_ftrl_host.py), through recman_amd.ops.

What each family of cases pins:

  * "ftrl" at every width D in {8, 12, 16, 24, 32, 48, 64}, through the three entries, over optim_ref.RUN_LENGTHS:
    inline runs, the hand-over at 17, one full segment and two to nine segments with the combine kernel all end in
    the FTRL branch of apply_row (ftrl_update), whose z and n travel in the m and v slots - of the moment array for
    lanes sub < GE, of the state columns (z_b z_l in lane GE's .z .w, n_b n_l handed over from lane GE + 1) for the
    side entries.  Three steps: other ids at step 2, step 1's ids through `prepared` at step 3.  The three entries
    agree bit for bit; two runs are bit-equal.
  * exact zeros: where the float64 reference has |z| <= l1 (1 - 1e-3) the kernel's parameter IS 0.0, where
    |z| >= l1 (1 + 1e-3) it is not; l1 is the median |z| of step 1, so both sides hold >= 10 % of the touched
    elements at every step (the host file asserts that on the reference).  No element is left out of the error
    bounds: the soft threshold is continuous.
  * two rules (D = 8, 24, 64: G = 4, 8, 32): adam + ftrl, adagrad + ftrl, sgd + ftrl, ftrl + adam, ftrl + sgd
    (embedding rule + side rule).  Columns < D follow the embedding rule's reference, columns D, D + 1 the side
    rule's.  What must not be written keeps its sentinel: no moment array exists under sgd + ftrl (and the state
    columns ARE written); the state columns D+2 .. D+5 under ftrl + sgd; the m halves under adagrad + ftrl; the padding
    from D+6 on; untouched rows.
  * options under FTRL: reset, l2_embedding / l2_linear, lin_field_mask, g_bias / g_lin absent, ld in {D + 8,
    D + 12, 2 D}, l1 = 0 (no touched element with a gradient becomes 0), l2 and beta > 0, side_lr != lr.
  * rm_dense_optimizer_step_rule with kind 3 at n = 77, 262144 + 77, 3 * 262144 + 77 (the grid-stride loop goes round
    once, twice and four times).
  * equal rules of kind 0 - 2 through the new entry points: bit-identical to rm_sparse_optimizer_step /
    rm_sparse_optimizer_step_rows / rm_dense_optimizer_step.
  * invalid rules return an error and leave rows and moments untouched.

Bounds (optim_ref.compare; the float32 restatement rounds after every operation, as ftrl_update does):
  parameters  max |got - want| <= max(5e-6 max(1, max |want|), 4 x the float32 restatement's error)
  state       grad_measure     <= max(2e-5, 4 x the float32 restatement's measure)

Largest values observed on the MI355X over all cases of this file (the float32 restatement's beside them):
  rule of the part     quantity   kernel     float32 restatement
  ftrl (one rule)      p          9.99e-06   7.99e-06    (max |want| 3.9: the 5e-6 max|want| term is 1.9e-05)
  ftrl (one rule)      z_emb      1.52e-05   3.03e-05
  ftrl (one rule)      z_side     3.84e-06   2.32e-05
  ftrl (one rule)      n_emb      8.80e-07   5.56e-06
  ftrl (one rule)      n_side     1.34e-06   5.87e-06
  ftrl (part of two)   p 9.99e-06 / 7.99e-06, z 9.28e-06 / 5.77e-05, n 1.40e-06 / 4.07e-06
  adam (part of two)   p 2.61e-06 / 2.61e-06, m 2.40e-06 / 5.38e-06, v 9.15e-07 / 4.09e-06
  adagrad (part)       p 3.59e-07 / 3.74e-07, v 8.91e-07 / 5.56e-06;  sgd (part) p 4.05e-07 / 1.10e-06
  dense ftrl           p 6.86e-07, z 6.22e-07 (9.31e-07), n 1.51e-07 (the restatement: the same where not given)
No case failed at any width or run length, and z stays within the 4 x figure everywhere (ftrl_update is compiled
without contraction, so an inline run rounds exactly where the restatement does; the long-run kernels' tree sums err
less than its sequential sum).  Exact zeros: 180 (case, step) checks, 389 elements in all within 1e-3 of l1 and so
left to either side; every other touched element was 0.0 or non-zero as the float64 z says.
"""
import ctypes

import pytest
import torch

from tests import optim_ftrl_ref as FR
from tests import optim_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _cuda(t):
    return None if t is None else t.cuda().contiguous()


def _rules(case):
    return dict(l1=case["l1"], l2=case["ftrl_l2"], ftrl_beta=case["ftrl_beta"], side_kind=case["side"],
                side_lr=case["side_lr"])


def _run(case, ops):
    """The case's steps through recman_amd.ops: [(rows, mom) after every step] (clones, on the GPU)."""
    D, kind, entry = case["D"], case["kind"], case["entry"]
    rows, mom = _cuda(case["rows0"].clone()), _cuda(None if case["mom0"] is None else case["mom0"].clone())
    assert (mom is None) == (kind == "sgd")
    n_max = max(st["B"] for st in case["steps"]) * case["F"]
    ws = torch.zeros(ops.sparse_optimizer_workspace(n_max), dtype=torch.uint8, device="cuda")
    foff = _cuda(case["foff"])
    mask = None if case["lin_mask"] is None else torch.tensor(case["lin_mask"], dtype=F32, device="cuda")
    hyper = dict(beta1=case["beta1"], beta2=case["beta2"], eps=case["eps"], l2_embedding=case["l2_emb"],
                 l2_linear=case["l2_lin"], **_rules(case))
    out = []
    for s, st in enumerate(case["steps"]):
        t, reset, prepared = case["step0"] + s, s in case["reset_at"], s in case["prepared_at"]
        if entry == "rows":
            ids, packed = _cuda(st["ids"]), _cuda(st["packed"])
            if prepared:
                ops.sparse_optimizer_prepare(ws, case["R"], row_ids=ids)
            ops.sparse_optimizer_step_rows(ids, packed, D, rows, mom, ws, t, kind, case["lr"], reset=reset,
                                           prepared=prepared, **hyper)
        else:
            idx = _cuda(st["idx"])
            if prepared:
                ops.sparse_optimizer_prepare(ws, case["R"], idx=idx, field_off=foff,
                                             max_field_rows=case["max_field_rows"])
            ops.sparse_optimizer_step(idx, foff, _cuda(st["d_rows"]), rows, mom, ws, t, kind, case["lr"],
                                      g_bias=None if case["no_bias"] else _cuda(st["g_bias"]),
                                      g_lin=None if case["no_lin"] else _cuda(st["g_lin"]), reset=reset,
                                      lin_field_mask=mask, prepared=prepared,
                                      max_field_rows=case["max_field_rows"], **hyper)
        out.append((rows.clone(), None if mom is None else mom.clone()))
    torch.cuda.synchronize()
    return out


_REFS = {}


def _references(case, name):
    """(float64, float32) restatement of a case: computed once, shared by the tests that need it, never changed."""
    if name not in _REFS:
        _REFS[name] = (FR.reference(case, F64), FR.reference(case, F32))
    return _REFS[name]


def _check_case(case, ops, name):
    """Runs the case twice; against float64 after every step; exact zeros; what must not change, bit for bit."""
    D, emb, side, Rn = case["D"], case["kind"], case["side"], case["R"]
    got, again = _run(case, ops), _run(case, ops)
    want, ref32 = _references(case, name)
    prev = (case["rows0"], case["mom0"])
    cols = FR.ftrl_columns(case)
    seen = torch.zeros(Rn, dtype=torch.bool)
    for s in range(len(case["steps"])):
        rows, mom = got[s][0].cpu(), None if got[s][1] is None else got[s][1].cpu()
        assert torch.equal(got[s][0], again[s][0]), (name, s)
        assert mom is None or torch.equal(got[s][1], again[s][1]), (name, s)
        occ = R.occurrence_rows(case, s)
        touched = torch.zeros(Rn, dtype=torch.bool)
        touched[occ[occ >= 0]] = True
        seen |= touched
        # untouched rows: all ld columns, and their moment rows; the padding of every row
        assert torch.equal(rows[~touched], prev[0][~touched]), (name, s)
        assert mom is None or torch.equal(mom[~touched], prev[1][~touched]), (name, s)
        assert bool((rows[:, D + 6:] == R.SENTINEL).all()), (name, s)
        # state a rule does not keep is never written
        assert (mom is None) == (emb == "sgd")
        if emb == "adagrad":
            assert bool((R.deinterleave(mom, D)[0] == R.SENTINEL).all()), (name, s)
        if side in ("adagrad", "sgd"):
            assert bool((rows[:, D + 2: D + 4] == R.SENTINEL).all()), (name, s)
        if side == "sgd":
            assert bool((rows[:, D + 4: D + 6] == R.SENTINEL).all()), (name, s)
        else:   # ... and the state it keeps is: v_b, v_l of the touched rows moved (no gradient at all: they stay)
            moved = rows[touched][:, D + 4: D + 6] != prev[0][touched][:, D + 4: D + 6]
            assert bool(moved.any()) or (case["no_bias"] and case["no_lin"]), (name, s)
        state = FR.state_of(rows, mom, D, emb, side)
        bad = FR.compare(state, want[s], ref32[s], case, tag=f"{name} step {s + 1}")
        assert not bad, (name, s, bad)
        if cols.any():
            # exact zeros: decided by the float64 z, clear of the threshold by 1e-3 of it
            z, p = want[s][1][seen][:, cols].abs(), state[0][seen][:, cols]
            l1 = case["l1"]
            below, above = z <= l1 * (1 - 1e-3), z >= l1 * (1 + 1e-3)
            assert bool((p[below] == 0.0).all()), (name, s, int((p[below] != 0).sum()))
            assert bool((p[above] != 0.0).all()), (name, s, int((p[above] == 0).sum()))
            print(f"{name} step {s + 1}: exact zeros {int(below.sum())}, non-zero {int(above.sum())}, "
                  f"within 1e-3 of l1 {int((~below & ~above).sum())}")
        prev = (rows, mom)
    return got


@pytest.mark.parametrize("name", list(FR.FTRL_CASES))
def test_ftrl_step_against_float64(hip_lib, name):
    from recman_amd import ops

    case = FR.make_case(**FR.FTRL_CASES[name])
    lengths = {L for _, L, _ in R.runs_of(R.sorted_keys(case, 0), case["R"])}
    assert set(R.RUN_LENGTHS) <= lengths
    _check_case(case, ops, name)


@pytest.mark.parametrize("D", R.WIDTHS)
def test_ftrl_entries_agree_bit_for_bit(hip_lib, D):
    from recman_amd import ops

    l1 = FR.make_case(D, "ftrl", "fields")["l1"]
    runs = {entry: _run(FR.make_case(D, "ftrl", entry, l1=l1), ops) for entry in R.ENTRIES}
    for entry in R.ENTRIES[1:]:
        for s in range(3):
            assert torch.equal(runs[entry][s][0], runs["fields"][s][0]), (entry, s)
            assert torch.equal(runs[entry][s][1], runs["fields"][s][1]), (entry, s)


@pytest.mark.parametrize("name", list(FR.SPLIT_CASES))
def test_two_rules_against_float64(hip_lib, name):
    from recman_amd import ops

    _check_case(FR.make_case(**FR.SPLIT_CASES[name]), ops, name)


@pytest.mark.parametrize("name", list(FR.OPTION_CASES))
def test_ftrl_options_against_float64(hip_lib, name):
    from recman_amd import ops

    kw = FR.OPTION_CASES[name]
    case = FR.make_case(**kw)
    _check_case(case, ops, name)
    plain_kw = {k: v for k, v in kw.items() if k not in ("reset_at", "l2_emb", "l2_lin", "ftrl_l2", "ftrl_beta",
                                                          "side_lr")}
    if plain_kw != kw:
        # the option is not a no-op: the float64 result without it lies far outside the bounds
        plain = FR.reference(FR.make_case(**dict(plain_kw, l1=case["l1"])), F64)
        assert float((plain[-1][0] - _references(case, name)[0][-1][0]).abs().max()) > 1e-4
    if kw.get("l1") == 0.0:
        # no exact zero among the touched elements (every one of them has a gradient)
        got = _run(case, ops)[-1][0].cpu()
        occ = torch.cat([R.occurrence_rows(case, s) for s in range(3)])
        touched = torch.zeros(case["R"], dtype=torch.bool)
        touched[occ[occ >= 0]] = True
        assert int((got[touched][:, : case["D"] + 2] == 0).sum()) == 0


@pytest.mark.parametrize("n", [77, 262144 + 77, 3 * 262144 + 77])
def test_dense_ftrl_against_float64(hip_lib, n):
    """rm_dense_optimizer_step_rule, kind 3: two persistent steps and one with reset (m = z, v = n)."""
    from recman_amd import ops

    k = R.kernel_constants()
    blocks = min(R.cdiv(n, k["kBlock"]), k["dense_grid_cap"])
    assert R.cdiv(n, blocks * k["kBlock"]) == {77: 1, 262144 + 77: 2, 3 * 262144 + 77: 4}[n]
    g = torch.Generator().manual_seed(n % 1000)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    hyper = dict(lr=0.02, l1=0.0, l2=0.1, beta=0.3)
    # l1 at the median |z| of step 1 (z does not depend on l1 there), from the float64 restatement
    hyper["l1"] = R.f32(float(FR.dense_reference(p0, grads[:1], F64, **hyper)[0][1].abs().median()))
    want = FR.dense_reference(p0, grads, F64, reset_at=(2,), **hyper)
    ref32 = FR.dense_reference(p0, grads, F32, reset_at=(2,), **hyper)
    p, z, acc = p0.cuda(), torch.zeros(n, device="cuda"), torch.full((n,), 0.1, device="cuda")
    for s in range(3):
        ops.dense_optimizer_step(p, grads[s].cuda(), z, acc, s + 1, "ftrl", hyper["lr"], reset=(s == 2),
                                 l1=hyper["l1"], l2=hyper["l2"], ftrl_beta=hyper["beta"])
        got = tuple(x.cpu().double()[None, :] for x in (p, z, acc))
        w, r = (tuple(x[None, :] for x in q[s]) for q in (want, ref32))
        bad = R.compare(got, w, r, None, tag=f"dense ftrl n={n} step {s + 1}")
        assert not bad, (n, s, bad)
        zabs = w[1].abs()
        assert bool((got[0][zabs <= hyper["l1"] * (1 - 1e-3)] == 0).all())
        assert bool((got[0][zabs >= hyper["l1"] * (1 + 1e-3)] != 0).all())
        share = float((zabs > hyper["l1"]).double().mean())
        assert 0.1 <= share <= 0.9, share


def _old_entry(case, lib_mod):
    """The case's steps through the entry points that take `kind` and the Adam / Adagrad constants as arguments."""
    from recman_amd import ops

    D, entry = case["D"], case["entry"]
    rows, mom = _cuda(case["rows0"].clone()), _cuda(None if case["mom0"] is None else case["mom0"].clone())
    ws = torch.zeros(ops.sparse_optimizer_workspace(max(st["B"] for st in case["steps"]) * case["F"]),
                     dtype=torch.uint8, device="cuda")
    foff = _cuda(case["foff"])
    kind = ops.OPT_KINDS[case["kind"]]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mp = None if mom is None else mom.data_ptr()
    out = []
    for s, st in enumerate(case["steps"]):
        if entry == "rows":
            ids, packed = _cuda(st["ids"]), _cuda(st["packed"])
            lib_mod.call("rm_sparse_optimizer_step_rows", ids.data_ptr(), packed.data_ptr(), packed.shape[1],
                         ids.numel(), D, case["R"], rows.data_ptr(), case["ld"], mp, s + 1, kind, case["lr"],
                         case["beta1"], case["beta2"], case["eps"], 0, 0.0, 0.0, 0, ws.data_ptr(), ws.numel(), stream)
        else:
            idx, d_rows, gb, gl = (_cuda(st[k]) for k in ("idx", "d_rows", "g_bias", "g_lin"))
            lib_mod.call("rm_sparse_optimizer_step", idx.data_ptr(), foff.data_ptr(), d_rows.data_ptr(),
                         gb.data_ptr(), gl.data_ptr(), st["B"], case["F"], D, case["R"], rows.data_ptr(), case["ld"],
                         mp, s + 1, kind, case["lr"], case["beta1"], case["beta2"], case["eps"], 0, 0.0, 0.0, None,
                         case["max_field_rows"], 0, ws.data_ptr(), ws.numel(), stream)
        out.append((rows.clone(), None if mom is None else mom.clone()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("entry", ["fields", "rows"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_equal_rules_are_the_old_entry_points_bit_for_bit(hip_lib, kind, entry):
    from recman_amd import _lib, ops

    case = FR.reseed(R.make_case(16, "adam", entry, prepared_at=()), kind)
    new, old = _run(case, ops), _old_entry(case, _lib)
    for s in range(3):
        assert torch.equal(new[s][0], old[s][0]), (kind, entry, s)
        assert kind == "sgd" or torch.equal(new[s][1], old[s][1]), (kind, entry, s)
    # the dense step
    g = torch.Generator().manual_seed(5)
    n = 1000
    p0, grad = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    res = []
    for which in ("new", "old"):
        p = p0.clone()
        m = torch.zeros(n, device="cuda") if kind == "adam" else None
        v = None if kind == "sgd" else torch.full((n,), 0.1 if kind == "adagrad" else 0.0, device="cuda")
        for t in (1, 2):
            if which == "new":
                ops.dense_optimizer_step(p, grad, m, v, t, kind, 0.01)
            else:
                _lib.call("rm_dense_optimizer_step", p.data_ptr(), grad.data_ptr(), None if m is None else m.data_ptr(),
                          None if v is None else v.data_ptr(), n, t, ops.OPT_KINDS[kind], 0.01, 0.9, 0.999, 1e-7, 0,
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        res.append((p, m, v))
    for a, b in zip(*res):
        assert a is None or torch.equal(a, b)


def test_invalid_rules_are_refused_and_leave_the_state_untouched(hip_lib):
    from recman_amd import _lib, ops

    case = FR.make_case(16, "ftrl", "fields", l1=1.0)
    st = case["steps"][1]
    rows, mom = _cuda(case["rows0"].clone()), _cuda(case["mom0"].clone())
    ws = torch.zeros(ops.sparse_optimizer_workspace(st["B"] * case["F"]), dtype=torch.uint8, device="cuda")
    idx, foff, d_rows = _cuda(st["idx"]), _cuda(case["foff"]), _cuda(st["d_rows"])
    gb, gl = _cuda(st["g_bias"]), _cuda(st["g_lin"])

    def step(kind="ftrl", lr=0.01, mom_=mom, **kw):
        ops.sparse_optimizer_step(idx, foff, d_rows, rows, mom_, ws, 1, kind, lr, g_bias=gb, g_lin=gl, **kw)

    def raw(emb, side):
        _lib.call("rm_sparse_optimizer_step_rules", idx.data_ptr(), foff.data_ptr(), d_rows.data_ptr(), gb.data_ptr(),
                  gl.data_ptr(), st["B"], case["F"], 16, case["R"], rows.data_ptr(), case["ld"], mom.data_ptr(), 1,
                  ctypes.byref(emb), ctypes.byref(side), 0, 0.0, 0.0, None, 0, 0, ws.data_ptr(), ws.numel(),
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    good = _lib.OptRule(3, 0.01, 0.9, 0.999, 1e-7, 1.0, 0.0, 0.0)
    bad_kind = _lib.OptRule(4, 0.01, 0.9, 0.999, 1e-7, 0.0, 0.0, 0.0)
    attempts = [
        lambda: raw(bad_kind, good), lambda: raw(good, bad_kind),                      # kind 4, in either role
        lambda: step(l1=-1.0), lambda: step(l2=-0.5), lambda: step(ftrl_beta=-0.5),    # negative constants
        lambda: step("adam", side_kind="ftrl", side_l1=-1.0),
        lambda: step(lr=0.0), lambda: step("adam", side_kind="ftrl", side_lr=0.0),     # FTRL divides by lr
        lambda: step(mom_=None), lambda: step("adagrad", mom_=None, side_kind="ftrl"),  # the embedding rule's state
    ]
    for i, attempt in enumerate(attempts):
        with pytest.raises(_lib.RecmanHipError):
            attempt()
        torch.cuda.synchronize()
        assert torch.equal(rows.cpu(), case["rows0"]) and torch.equal(mom.cpu(), case["mom0"]), i
    z, acc, p = torch.zeros(8, device="cuda"), torch.full((8,), 0.1, device="cuda"), torch.ones(8, device="cuda")
    for kw in (dict(lr=0.0), dict(lr=0.01, l1=-1.0)):
        with pytest.raises(_lib.RecmanHipError):
            ops.dense_optimizer_step(p, p.clone(), z, acc, 1, "ftrl", **kw)
    with pytest.raises(_lib.RecmanHipError):
        ops.dense_optimizer_step(p, p.clone(), None, acc, 1, "ftrl", 0.01)   # z is needed
    assert bool((p == 1).all()) and bool((z == 0).all())
    step("sgd", mom_=None, side_kind="ftrl", l1=1.0)   # an SGD embedding rule needs no moment array
    assert not torch.equal(rows.cpu(), case["rows0"])
