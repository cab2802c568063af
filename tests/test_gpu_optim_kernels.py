"""GPU: the optimizer kernels of csrc/optim.hip against a float64 restatement (tests/optim_ref.py, pinned without a
GPU by tests/test_optim_host.py), through recman_amd.ops, at every embedding width the row-wise step is compiled for
and at every run length at which it takes another path.

What each family of cases pins (lines of csrc/optim.hip):

  * D in {8, 12, 16, 24, 32, 48, 64}: the seven instantiations of sparse_step's dispatch on GE = D / 4 (:768-779),
    lane groups G = 4, 8, 8, 8, 16, 16, 32.  G = 8 with GE = 3 has three idle lanes, with GE = 6 none (the side
    lanes GE and GE + 1 are the last two of the group); G = 16 with GE = 12 has two idle lanes; G = 32 leaves the
    long-run kernel NG = 2 groups a wave.  apply_row's __shfl_down / __shfl_up hand-off of (v_b, v_l) between lanes
    GE and GE + 1 (:175, :191) runs in each of these layouts, for Adam, Adagrad and SGD (opt_update, :105-118).
  * run lengths of step 1 (sparse_apply_kernel :266-267, :283; sparse_apply_long_kernel :332; the combine kernel
    :379-389): 1, 2, 3 (no sum, the shortest sums); 16, 17, 18 (the last inline run, the first one handed over as
    len > kLong, the gallop's first step); 33, 127 (gallop + bisect inside one segment); 128 (a full segment, applied
    by the long-run kernel), 129, 130 (two segments, the second of 1 and of 2 members); 256, 257 (2, 3 segments: the
    combine kernel's tail loop only); 512, 513 (4: one unrolled round and no tail; 5: unrolled + 1); 641, 897, 1025
    (6, 8, 9 segments: unrolled + 2, two unrolled rounds, two + 1).  A segment of 128 takes 1, 2, 4 and 8 rounds of
    kLongFlight * NG = 128, 64, 32, 16 members at G = 4, 8, 16, 32.
  * kPos = 2 (:230): runs of 1, 2, 17 and 129 start once at an even and once at an odd sorted position.
  * the end of the list: a run of >= 129 directly followed by the skipped keys (every full case); no skipped id and
    the list ending with a handed-over run (the gallop's t >= n, :272) or an inline one (i + len < n, :266) (the
    "ends" cases); >= 5 % of ids skipped, spelled -1, -5, the entry's limit (the field's size - an id that IS a row
    of a larger field -, R - field_off[f], R) and beyond (:98-100, :447-452).
  * step 2 has other ids, no run beyond kLong and an odd n, on a workspace whose ticket counters step 1 used
    (:89, :438); rows step 1 touched and step 2 leaves out keep their state; step 3 repeats step 1's ids through
    rm_sparse_optimizer_prepare + prepared (opt_clear_word_kernel, :742).
  * the three entries - [B, F] ids sorted per field (max_field_rows > 0), the one sort over all pairs, and
    rm_sparse_optimizer_step_rows on packed [n, gw] rows (gw = D + 4, D + 8) - agree bit for bit at every D.
  * what must not change: untouched rows (all ld columns) and their moment rows, the padding D+6 .. ld-1 of touched
    rows, Adagrad's m halves (pm[0] is written for kind 0 only, :199) and m_b, m_l, SGD's state columns D+2 .. D+5.
  * options: reset (:107, :112, :649), l2_embedding / l2_linear (:178-180), lin_field_mask (:131), g_bias / g_lin
    absent (:130-131), ld in {D + 8, D + 12, 2 D}, other beta1 / beta2 / eps / lr, step = 1000 (:648-651).
  * rm_dense_optimizer_step (:835-845): n up to 3 * 262144 + 77 - the grid is min(ceil(n / 256), 1024) blocks of
    256 (:841), so the grid-stride loop (:400) goes round twice and four times.
  * SparseTableOptimizer inside an engine at D = 8 (the minimal row, LD = 16 = D + 8), 32 and 64.

Bounds (optim_ref.compare; the float32 restatement sums every run sequentially in occurrence order):
  parameters  max |got - want| <= max(5e-6 max(1, max |want|), 4 x the float32 restatement's error)
  moments     grad_measure     <= max(2e-5, 4 x the float32 restatement's measure)
(5e-6 is tests/test_gpu_optim.py's figure for these kernels; 4 x because the long-run kernels add in another tree
than the sequential restatement.)  tests/test_optim_host.py shows that these bounds catch a lost run member, a
segment added twice, a missing l2 term and a side entry reading the wrong lane's v.

Largest values observed on the MI355X over all cases of this file (the float32 restatement's beside them):
  row-wise step   quantity   kernel     float32 restatement
  adam            p          2.61e-06   2.61e-06
  adam            m_emb      2.40e-06   1.01e-05
  adam            m_side     1.77e-06   5.47e-06
  adam            v_emb      9.94e-07   5.57e-06
  adam            v_side     1.31e-06   5.91e-06
  adagrad         p          2.68e-06   1.61e-05
  adagrad         v_emb      8.91e-07   5.56e-06
  adagrad         v_side     1.40e-06   4.66e-06
  sgd             p          4.05e-07   1.19e-06
  dense step      adam p 6.75e-07, m 7.26e-07, v 2.84e-07; adagrad p 6.93e-07, v 1.46e-07; sgd p 6.59e-07 (the float32
                  restatement: the same to two digits - one element, one rounding chain)
  engine          table parameters 4.8e-07; dense parameters 6.6e-07 .. 2.15e-06 from run to run at D = 64 under Adam
                  (see test_engine_sparse_step_equals_dense_step_when_reset_every_batch), <= 1.2e-06 else
No kernel case failed at any width or run length; the kernels' sums (a tree over lane groups and segments) err less
than the sequential float32 sum wherever runs are long.
"""
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _cuda(t):
    return None if t is None else t.cuda().contiguous()


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
                 l2_linear=case["l2_lin"])
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


def _check_launch_arithmetic(case):
    """The paths the case is meant to take, from the limits csrc/optim.hip states today."""
    k = R.kernel_constants()
    assert (k["kLong"], k["kSeg"], k["kPos"], k["kLongFlight"]) == (R.K_LONG, R.K_SEG, R.K_POS, R.K_FLIGHT)
    D = case["D"]
    G, GE, NG = R.group_lanes(D)
    assert G == {8: 4, 12: 8, 16: 8, 24: 8, 32: 16, 48: 16, 64: 32}[D] and GE == D // 4 and NG == 64 // G
    assert G >= GE + 2 and G // 2 < GE + 2                              # lanes GE and GE + 1 exist; no smaller group
    assert k["kLongFlight"] * NG == {4: 128, 8: 64, 16: 32, 32: 16}[G]  # members per round of a wave
    keys = R.sorted_keys(case, 0)
    lengths = {L for _, L, _ in R.runs_of(keys, case["R"])}
    inline, handed = {L for L in lengths if L <= k["kLong"]}, {L for L in lengths if L > k["kLong"]}
    assert {1, 2, 3, 16} <= inline and {17, 18, 33, 127, 128} <= handed
    segs = {L: R.cdiv(L, k["kSeg"]) for L in handed}
    assert [segs[L] for L in (127, 128, 129, 130, 256, 257, 512, 513, 641, 897, 1025)] == [
        1, 1, 2, 2, 2, 3, 4, 5, 6, 8, 9]
    assert keys.numel() > (k["kBlock"] // G) * k["kPos"]                # more than one block of sparse_apply_kernel
    assert max(L for _, L, _ in R.runs_of(R.sorted_keys(case, 1), case["R"])) == k["kLong"]


def _check_case(case, ops, name, full=True):
    """Runs the case twice; against float64 after every step; what must not change, bit for bit."""
    D, kind, ld, Rn = case["D"], case["kind"], case["ld"], case["R"]
    if full:
        _check_launch_arithmetic(case)
    got, again = _run(case, ops), _run(case, ops)
    want, ref32 = R.reference(case, F64), R.reference(case, F32)
    prev = (case["rows0"], case["mom0"])
    for s in range(len(case["steps"])):
        rows, mom = got[s][0].cpu(), None if got[s][1] is None else got[s][1].cpu()
        # two runs from the same state agree on everything
        assert torch.equal(got[s][0], again[s][0]), (name, s)
        assert mom is None or torch.equal(got[s][1], again[s][1]), (name, s)
        occ = R.occurrence_rows(case, s)
        touched = torch.zeros(Rn, dtype=torch.bool)
        touched[occ[occ >= 0]] = True
        # untouched rows: all ld columns, and their moment rows
        assert torch.equal(rows[~touched], prev[0][~touched]), (name, s)
        assert mom is None or torch.equal(mom[~touched], prev[1][~touched]), (name, s)
        # the padding of every row
        assert bool((rows[:, D + 6:] == R.SENTINEL).all()), (name, s)
        if kind == "adagrad":   # no first moment: the m halves and m_b, m_l are never written
            assert bool((R.deinterleave(mom, D)[0] == R.SENTINEL).all()), (name, s)
            assert bool((rows[:, D + 2: D + 4] == R.SENTINEL).all()), (name, s)
        if kind == "sgd":       # no state at all
            assert bool((rows[:, D + 2: D + 6] == R.SENTINEL).all()), (name, s)
        if touched.any():
            assert not torch.equal(rows[touched][:, : D + 2], prev[0][touched][:, : D + 2]), (name, s)
        bad = R.compare(R.state_of(rows, mom, D, kind), want[s], ref32[s], D, tag=f"{name} step {s + 1}")
        assert not bad, (name, s, bad)
        prev = (rows, mom)
    return got


@pytest.mark.parametrize("name", list(R.SPARSE_CASES))
def test_sparse_step_against_float64(hip_lib, name):
    from recman_amd import ops

    _check_case(R.make_case(**R.SPARSE_CASES[name]), ops, name)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_entries_agree_bit_for_bit(hip_lib, D, kind):
    """[B, F] ids sorted per field, the one sort over all pairs and the packed-rows entry leave the same table and
    moments after every step: the runs hold the same occurrences in the same order."""
    from recman_amd import ops

    runs = {entry: _run(R.make_case(D, kind, entry), ops) for entry in R.ENTRIES}
    for entry in R.ENTRIES[1:]:
        for s in range(3):
            assert torch.equal(runs[entry][s][0], runs["fields"][s][0]), (entry, s)
            if kind != "sgd":
                assert torch.equal(runs[entry][s][1], runs["fields"][s][1]), (entry, s)


@pytest.mark.parametrize("name", list(R.END_CASES))
def test_sorted_list_ends_with_a_run(hip_lib, name):
    from recman_amd import ops

    case = R.make_case(**R.END_CASES[name])
    keys = R.sorted_keys(case, 0)
    last = R.runs_of(keys, case["R"])[-1]
    assert int((keys == case["R"]).sum()) == 0 and last[0] + last[1] == keys.numel()
    assert (last[1] > R.K_LONG) == (R.END_CASES[name]["tail"] == "long")
    _check_case(case, ops, name)


@pytest.mark.parametrize("name", list(R.OPTION_CASES))
def test_options_against_float64(hip_lib, name):
    from recman_amd import ops

    kw = R.OPTION_CASES[name]
    case = R.make_case(**kw)
    assert case["ld"] >= case["D"] + 8 and case["ld"] % 4 == 0 and case["gw"] >= case["D"] + 2
    _check_case(case, ops, name)
    if "reset_at" in kw or "l2_emb" in kw or kw.get("step0", 1) != 1:
        # the option is not a no-op: the float64 result without it lies far outside the bounds
        plain = R.reference(R.make_case(**{k: v for k, v in kw.items() if k not in ("reset_at", "l2_emb", "l2_lin",
                                                                                     "step0")}), F64)
        assert float((plain[-1][0] - R.reference(case, F64)[-1][0]).abs().max()) > 1e-4


@pytest.mark.parametrize("entry", R.ENTRIES)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("which", ["n1", "n2_same_row", "n_odd", "all_skipped", "empty"])
def test_smallest_occurrence_lists(hip_lib, which, kind, entry):
    """n = 1; n = 2 on one row; an odd n (the last lane group has one position); every id skipped and B = 0 (rows,
    moments and padding bit-unchanged: _check_case's untouched-row assertions cover every row)."""
    from recman_amd import ops

    for D in (12, 64):
        case = R.small_case(which, D, kind, entry)
        got = _check_case(case, ops, f"{which} d{D} {kind} {entry}", full=False)
        if which in ("all_skipped", "empty"):
            assert torch.equal(got[0][0].cpu(), case["rows0"])
            assert kind == "sgd" or torch.equal(got[0][1].cpu(), case["mom0"])


DENSE_SIZES = [1, 255, 257, 262144 + 3, 3 * 262144 + 77]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", DENSE_SIZES)
def test_dense_step_against_float64(hip_lib, n, kind):
    """rm_dense_optimizer_step: three persistent steps, then one with reset."""
    from recman_amd import ops

    k = R.kernel_constants()
    blocks = min(R.cdiv(n, k["kBlock"]), k["dense_grid_cap"])
    assert k["dense_grid_cap"] == R.DENSE_GRID_CAP == 1024 and k["kBlock"] == 256
    passes = R.cdiv(n, blocks * k["kBlock"])   # rounds of the grid-stride loop
    assert passes == {1: 1, 255: 1, 257: 1, 262144 + 3: 2, 3 * 262144 + 77: 4}[n]
    g = torch.Generator().manual_seed(n % 1000)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(4)]
    want = R.dense_reference(p0, grads, kind, F64, reset_at=(3,))
    ref32 = R.dense_reference(p0, grads, kind, F32, reset_at=(3,))
    p = p0.cuda()
    m = torch.zeros(n, device="cuda") if kind == "adam" else None
    v = None if kind == "sgd" else torch.full((n,), 0.1 if kind == "adagrad" else 0.0, device="cuda")
    for s in range(4):
        ops.dense_optimizer_step(p, grads[s].cuda(), m, v, s + 1, kind, 0.01, reset=(s == 3))
        got = tuple(None if x is None else x.cpu().double()[None, :] for x in (p, m, v))
        w, r = (tuple(None if x is None else x[None, :] for x in q[s]) for q in (want, ref32))
        bad = R.compare(got, w, r, None, tag=f"dense n={n} {kind} step {s + 1}")
        assert not bad, (n, kind, s, bad)


def _adam_slope(g1, g2, lr):
    """Largest slope, between g1 and g2, of the step an Adam REBUILT every batch takes on a gradient g:
    u(g) = lr_1 (1 - b1) g / (sqrt(1 - b2) |g| + eps) = lr g / (|g| + c), c = eps / sqrt(1 - b2) = 3.16e-6;
    u'(g) = lr c / (|g| + c)^2, largest at the smaller |g|, and at 0 (lr / c = 3,162) when the two differ in sign."""
    c = 1e-7 / (1.0 - 0.999) ** 0.5
    nearest = torch.where(g1 * g2 > 0, torch.minimum(g1.abs(), g2.abs()), torch.zeros_like(g1))
    return lr * c / (nearest + c) ** 2, c


@pytest.mark.parametrize("name", R.KINDS)
@pytest.mark.parametrize("D", [8, 32, 64])
def test_engine_sparse_step_equals_dense_step_when_reset_every_batch(hip_lib, D, name):
    """tests/test_gpu_optim.py's comparison (SparseTableOptimizer + Optimizer against Optimizer on dense_grads(), the
    optimizer rebuilt every batch, three steps) at its own 2e-6 max(1, max |p|), at the minimal row (D = 8: LD = 16 =
    D + 8) and at the widths no engine has stepped row-wise before.

    The bound holds as it is for every parameter the row-wise step writes (the embedding, bias and linear tables:
    4.8e-7 at most in seven runs on the MI355X), for every parameter under Adagrad and SGD, and under Adam for every
    entry of a dense parameter whose gradient lies clear of Adam's kink, |g| >= 100 c.  The dense parameters are
    stepped by the plain-torch Optimizer on BOTH sides; they differ only through the two engines' gradients, and an
    Adam rebuilt every batch moves an entry by u(g) = lr g / (|g| + c), c = eps / sqrt(1 - beta2) = 3.16e-6, whose slope
    lr c / (|g| + c)^2 reaches 3,162 at g = 0.  Measured: dnn_layer_0_bias[1] at D = 64 has g = 3.86e-7 where the
    tensor's largest is 6e-3; the slope there is 2,500; the row-wise side's gradient is 3.855675e-7 in every run, the
    dense side's 3.847e-7 .. 3.853e-7 (dense_grads() densifies with float atomics, so its table rows after step 1
    differ from run to run in the last bit and the later forward passes with them); 2,500 x 8.6e-10 = 2.15e-6, and
    the unconditioned comparison went over 2e-6 in two runs of seven (2.03e-6, 2.15e-6) on an entry the row-wise step
    never writes.  So an entry with |g| < 100 c in some step is allowed, on top of the 2e-6, what the two engines' own
    gradients explain: the sum over the steps so far of (the largest slope of u between the two gradients) x |g1 - g2|,
    a bound on |u(g1) - u(g2)| by the mean value theorem.  At |g| >= 100 c the slope is below lr / (10,000 c) = 0.32
    and the allowance would be of the order of 1e-10: those entries get none."""
    from recman_amd.optim import Optimizer, SparseTableOptimizer
    from tests.cases import make_case
    from tests.test_gpu_optim import _engine

    lr = 0.01
    spec, p, idx, dense, y, hp = make_case("deepfm", B=300, D=D, sizes=[7, 11, 5, 13, 3])
    hp = dict(hp, embedding_l2_reg=0.0, linear_l2_reg=0.0)
    e1, e2 = _engine("deepfm", spec, D, hp, p), _engine("deepfm", spec, D, hp, p)
    assert e2.rows.shape[1] >= D + 8 and (D != 8 or e2.rows.shape[1] == 16)
    dopt = Optimizer(name, lr)
    sopt, sdense = SparseTableOptimizer(e2, name, lr), Optimizer(name, lr)
    idx_d, dense_d, y_d = idx.cuda(), dense.cuda(), y.cuda()
    dense_keys = set(e2.grads)   # what the plain Optimizer steps on the row-wise side; the tables are the rest
    assert dense_keys < set(e1.params) and any("feat_embed" in k for k in set(e1.params) - dense_keys)
    allowance = {k: torch.zeros_like(e1.params[k]) for k in dense_keys}
    for step in range(3):
        e1.fwd_bwd(idx_d, dense_d, y_d)
        dopt.reset()
        g1 = e1.dense_grads(idx_d)
        dopt.step(e1.params, g1)
        e2.fwd_bwd(idx_d, dense_d, y_d)
        sdense.reset()
        sopt.step(idx_d, reset=True)
        if name == "adam":
            for k in dense_keys:
                slope, c = _adam_slope(g1[k], e2.grads[k], lr)
                near = torch.minimum(g1[k].abs(), e2.grads[k].abs()) < 100 * c
                allowance[k] += torch.where(near, slope * (g1[k] - e2.grads[k]).abs(), torch.zeros_like(slope))
        sdense.step(e2.params, e2.grads)
        for k in e1.params:
            a, b = e1.params[k], e2.params[k]
            err = (a - b).abs()
            bound = 2e-6 * max(1.0, float(a.abs().max()))
            extra = allowance[k] if k in dense_keys else torch.zeros_like(a)
            print(f"engine d{D} {name} step {step + 1}: {k} {float(err.max()):.2e}, entries with an allowance "
                  f"{int((extra > 0).sum())} of {a.numel()}, largest {float(extra.max()):.2e}")
            assert bool((err <= bound + extra).all()), (step, k, float(err.max()), float((err - extra).max()))
