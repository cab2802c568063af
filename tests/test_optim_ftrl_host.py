"""CPU: pins tests/optim_ftrl_ref.py, the restatement of FTRL-Proximal and of the two-rule row-wise step that
tests/test_gpu_optim_ftrl.py runs the kernels of csrc/optim.hip against.

  * the float64 restatement equals a second statement of TensorFlow's ApplyFtrl arithmetic (powers, beta folded into
    l2, the soft threshold as a clip) on a few thousand elements over several steps, with l1 / l2 / beta zero and
    non-zero, and after `reset`;
  * the float32 restatement stays within the GPU file's bounds of the float64 one, and five deliberately wrong
    restatements do not: the side entry reading the embedding's n, z and n swapped in the layout, 2 l2 written as
    l2, the L1 test on p instead of z, the side rule applied to the embedding lanes;
  * input conditions of every FTRL case of the GPU file: l1 sits at the median |z| of step 1, and at every step at
    least 10 % of the touched elements lie on each side of |z| > l1 (asserted on the float64 reference alone);
  * the two-rule cases keep their sentinels where a rule keeps no state.
"""
import pytest
import torch

from tests import optim_ftrl_ref as FR
from tests import optim_ref as R

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("l1,l2,beta", [(0.0, 0.0, 0.0), (0.7, 0.0, 0.0), (0.7, 0.3, 0.0), (0.0, 0.3, 2.0),
                                        (1.5, 0.05, 0.5)])
def test_float64_restatement_equals_tf_apply_ftrl(l1, l2, beta):
    g = torch.Generator().manual_seed(11)
    n, lr = 4000, 0.05
    p = torch.randn(n, generator=g, dtype=F64)
    z, acc = torch.zeros(n, dtype=F64), torch.full((n,), R.f32(0.1), dtype=F64)
    var, accum, linear = p.clone(), acc.clone(), z.clone()
    zeros = 0
    for s in range(6):
        grad = torch.randn(n, generator=g, dtype=F64) * (0.2 if s % 2 else 2.0)
        reset = s == 4
        if reset:   # a new optimizer: fresh slots, the variable kept
            accum, linear = torch.full_like(accum, R.f32(0.1)), torch.zeros_like(linear)
        p, z, acc = FR.ftrl_update(p, z, acc, grad, lr, l1, l2, beta, reset)
        var, accum, linear = FR.tf_apply_ftrl(var, accum, linear, grad, lr, l1, l2, beta)
        for a, b in ((p, var), (z, linear), (acc, accum)):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), s
        zeros += int((p == 0).sum())
        assert bool(((p == 0) == (z.abs() <= l1)).all())
    assert (zeros > 0) == (l1 > 0)


def test_dense_form_is_the_same_rule():
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(300, generator=g)
    grads = [torch.randn(300, generator=g) for _ in range(3)]
    out = FR.dense_reference(p0, grads, F64, lr=0.02, l1=0.4, l2=0.1, beta=0.3, reset_at=(2,))
    p, z, n = p0.double(), torch.zeros(300, dtype=F64), torch.full((300,), R.f32(0.1), dtype=F64)
    for s in range(3):
        p, z, n = FR.ftrl_update(p, z, n, grads[s].double(), R.f32(0.02), R.f32(0.4), R.f32(0.1), R.f32(0.3), s == 2)
        assert torch.equal(out[s][0], p) and torch.equal(out[s][1], z) and torch.equal(out[s][2], n)
    ref32 = FR.dense_reference(p0, grads, F32, lr=0.02, l1=0.4, l2=0.1, beta=0.3, reset_at=(2,))
    assert 0 < float((ref32[-1][0] - out[-1][0]).abs().max()) < 1e-4


ALL = {**FR.FTRL_CASES, **FR.SPLIT_CASES, **FR.OPTION_CASES}


@pytest.mark.parametrize("name", [k for k in ALL if k.startswith(("d8_", "d12_", "d64_"))])
def test_input_conditions_of_the_gpu_cases(name):
    """l1 about the median |z| after step 1; >= 10 % of the touched FTRL elements on each side of the threshold at
    every step (l1 = 0: none below); sentinels where a rule keeps nothing."""
    kw = ALL[name]
    case = FR.make_case(**kw)
    D, emb, side = case["D"], case["kind"], case["side"]
    want = FR.reference(case, F64)
    if "ftrl" in (emb, side):
        if kw.get("l1", "median") == "median":
            assert case["l1"] == FR.median_l1(case) > 0
            for s, (over, under) in enumerate(FR.threshold_shares(case, want)):
                assert over >= 0.10 and under >= 0.10, (name, s, over, under)
            over1 = FR.threshold_shares(case, want)[0][0]
            if not (kw.get("no_lin") or kw.get("no_bias")):   # (an entry without a gradient has z = 0: below)
                assert 0.4 <= over1 <= 0.6, (name, over1)
        else:
            assert case["l1"] == 0.0
    assert (case["mom0"] is None) == (emb == "sgd")
    if emb == "adagrad":
        assert bool((R.deinterleave(case["mom0"], D)[0] == R.SENTINEL).all())
    cols = case["rows0"][:, D + 2: D + 6]
    assert bool((cols == R.SENTINEL).all()) == (side == "sgd")
    assert bool((cols[:, :2] == R.SENTINEL).all()) == (side in ("sgd", "adagrad"))
    assert bool((case["rows0"][:, D + 6:] == R.SENTINEL).all())


def _fails(case, want, state32):
    return any(FR.compare(state32[s], want[s], want32, case, show=False)
               for s, want32 in enumerate(FR.reference(case, F32)))


MUTATION_CASES = {
    "side_reads_emb_n": dict(D=8, kind="ftrl", entry="fields"),
    "swap_z_n": dict(D=24, kind="ftrl", entry="pairs"),
    "l2_once": dict(D=12, kind="ftrl", entry="fields", ftrl_l2=0.5, ftrl_beta=1.0),
    "l1_on_p": dict(D=64, kind="adagrad", side="ftrl", entry="rows"),
    "side_rule_on_emb": dict(D=8, kind="adam", side="ftrl", entry="rows"),
}


@pytest.mark.parametrize("mutation", FR.MUTATIONS)
def test_bounds_catch_every_wrong_restatement(mutation):
    """The GPU file's bounds pass the plain float32 restatement (against itself as yardstick: the least any result may
    claim) and fail the mutated one, on a case that has what the mutation touches."""
    case = FR.make_case(**MUTATION_CASES[mutation])
    want = FR.reference(case, F64)
    assert not _fails(case, want, FR.reference(case, F32))
    assert _fails(case, want, FR.reference(case, F32, mutate=mutation)), mutation
    # ... and in float64 the mutation is far outside the bounds, not at their edge
    worst = max(float((a[0] - b[0]).abs().max()) for a, b in zip(FR.reference(case, F64, mutate=mutation), want))
    assert worst > 1e-3, (mutation, worst)


def test_mutations_cover_the_list():
    assert set(MUTATION_CASES) == set(FR.MUTATIONS)


@pytest.mark.parametrize("pair", FR.SPLIT_PAIRS)
def test_split_reference_is_each_rule_on_its_columns(pair):
    """Columns < D of a two-rule case equal the one-rule case of the embedding rule, columns D, D + 1 that of the
    side rule (same occurrences, same l1)."""
    emb, side = pair
    both = FR.make_case(8, emb, "pairs", side=side)
    want = FR.reference(both, F64)
    for rule, sl in ((emb, slice(0, 8)), (side, slice(8, 10))):
        one = FR.make_case(8, rule, "pairs", l1=both["l1"])
        ref = FR.reference(one, F64)
        for s in range(3):
            for i in range(3):
                assert torch.equal(ref[s][i][:, sl], want[s][i][:, sl]), (pair, rule, s, i)
