"""CPU: pins tests/fibinet_ref.py - the float64 restatement of FiBiNET's interaction and model the GPU tests compare the
HIP kernels against.  The tensor form equals explicit Python loops, the written-out backward equals autograd, every
deliberately wrong variant is caught by the forward tolerance on every kernel case, and the cases meet the conditions
their docstrings state (no gate within KINK of its kink, a balanced share of open gates, the special rows)."""
import pytest
import torch

from tests import fibinet_ref as R

F64 = torch.float64
SMALL = [(4, 2, 8, 1, "each"), (3, 3, 8, 1, "all"), (3, 5, 8, 2, "each"), (2, 6, 16, 3, "all"), (2, 4, 32, 4, "each")]
CASE_IDS = lambda s: "B%d_F%d_D%d_R%d_%s" % s  # noqa: E731


@pytest.mark.parametrize("shape", SMALL, ids=CASE_IDS)
def test_tensor_form_equals_the_loops(shape):
    c = R.kernel_case(*shape, seed=3)
    ws = R.case_weights(c)
    loops = R.interact_loops(c["E"], *ws, c["btype"])
    assert loops.shape == c["X"].shape == (shape[0], 2 * R.pairs(shape[1]) * shape[2])
    assert float((loops - c["X"]).abs().max()) <= 1e-12 * max(1.0, float(c["X"].abs().max()))


def test_pair_order_is_itertools_combinations():
    li, lj = R.pair_fields(4)
    assert li.tolist() == [0, 0, 0, 1, 1, 2] and lj.tolist() == [1, 2, 3, 2, 3, 3]
    assert R.pairs(26) == 325 and R.reduction(26, 3) == 8 and R.reduction(2, 3) == 1
    # "each": the LEFT field selects the matrix
    E = torch.zeros(1, 3, 8, dtype=F64)
    E[0, 1], E[0, 2] = 1.0, 1.0
    W = torch.stack([torch.full((8, 8), 1.0, dtype=F64), torch.full((8, 8), 2.0, dtype=F64)])
    x = R.bilinear(E, W, "each").reshape(3, 8)
    assert float(x[0].abs().max()) == 0 and float(x[1].abs().max()) == 0 and torch.equal(x[2], torch.full((8,), 16.0, dtype=F64))


@pytest.mark.parametrize("shape", R.GPU_CASES, ids=CASE_IDS)
def test_written_out_backward_equals_autograd(shape):
    c = R.kernel_case(*shape)
    leaves = [c["E"].clone().requires_grad_(True)] + [w.clone().requires_grad_(True) for w in R.case_weights(c)]
    X = R.interact(*leaves, c["btype"])
    assert torch.equal(X.detach(), c["X"])
    (X * c["dX"]).sum().backward()
    want = [t.grad for t in leaves]
    got = R.interact_bwd(c["E"], *R.case_weights(c), c["btype"], c["dX"])
    for n, g, w in zip(("dE",) + R.PARAMS, got, want):
        assert g.shape == w.shape, n
        assert R.grad_measure(g, w) <= 1e-11, (n, R.grad_measure(g, w))
    assert torch.equal(got[0], c["dE"])


@pytest.mark.parametrize("shape", R.GPU_CASES, ids=CASE_IDS)
def test_case_conditions_and_tolerances(shape):
    B, F, D, Rr, btype = shape
    c = R.kernel_case(*shape)
    dist, share, most_negative = R.gate_conditions(c["E"], c["senet_w1"], c["senet_w2"])
    print(f"{shape}: min |pre-activation| {dist:.2e}, open gates {share:.2f}")
    assert dist >= R.KINK
    assert share > 0 and (most_negative >= 0 if R.one_pair_one_unit(F, Rr) else most_negative < 0)
    if B >= 33:
        assert 0.2 <= share <= 0.8
    for t in (c["E"], c["dX"]) + R.case_weights(c):
        assert torch.equal(t, t.float().double())  # every value is a float32 number
    if B > 8:
        assert float(c["E"][3].abs().max()) == 0 and float(c["X"][3].abs().max()) == 0 and float(c["dE"][3].abs().max()) == 0
        assert float(c["dX"][4].abs().max()) == 0 and float(c["dE"][4].abs().max()) == 0
        assert float(c["E"][5].abs().max()) > 8.0
    # the float32 restatement's own errors sit well inside the tolerances ...
    f32 = R.f32_errors(c)
    print("float32 CPU restatement: X %.2e dE %.2e dW1 %.2e dW2 %.2e dWb %.2e dWsb %.2e" % f32)
    # (X: but for the E x 8 example.  Nearly all its V-branch entries lie far above 1, so the measure is a relative
    # one there and shows every cancelling left product: float32 sums leave 4e-6 .. 9e-5 on that row, which is why the
    # kernels sum the gate and the left products in float64)
    keep = torch.ones(B, dtype=torch.bool)
    if B > 8:
        keep[5] = False
    X32 = R.interact(c["E"].float(), *R.case_weights(c, torch.float32), btype)
    assert R.x_error(X32[keep], c["X"][keep]) <= R.TOL_X / 2 and f32[1] <= R.TOL_GRAD / 2
    assert all(4 * e <= 10 * R.TOL_GRAD for e in f32[2:])
    # ... and every wrong variant far outside the forward's
    ws = R.case_weights(c)
    for wrong in R.WRONG:
        if not R.wrong_applies(wrong, F, Rr, btype):
            assert torch.equal(R.interact(c["E"], *ws, btype, wrong=wrong), c["X"])
            continue
        err = R.x_error(R.interact(c["E"], *ws, btype, wrong=wrong), c["X"])
        assert err > 100 * R.TOL_X, (wrong, err)


def test_relu_gradient_at_zero_is_zero():
    E = torch.zeros(2, 3, 8, dtype=F64)
    E[1] = 1.0
    W1, W2 = torch.ones(3, 1, dtype=F64), torch.ones(1, 3, dtype=F64)
    Wb = torch.eye(8, dtype=F64).unsqueeze(0)
    dX = torch.ones(2, 2 * 3 * 8, dtype=F64)
    dE, dW1, dW2, _, _ = R.interact_bwd(E, W1, W2, Wb, Wb, "all", dX)
    assert float(dE[0].abs().max()) == 0.0  # E = 0: both pre-activations are 0, relu'(0) = 0
    assert float(dE[1].abs().max()) > 0 and float(dW1.abs().max()) > 0 and float(dW2.abs().max()) > 0


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
@pytest.mark.parametrize("use_linear", [True, False])
def test_model_cases(name, use_linear):
    k = R.make_case(*R.MODEL_CASES[name], use_linear=use_linear)
    B, F, D, Dn, ratio, btype = R.MODEL_CASES[name]
    p, spec, hp = k["p"], k["spec"], k["hp"]
    print(f"{name}: min |pre-activation| {k['min_abs_pre']:.2e}")
    assert k["min_abs_pre"] >= R.KINK
    Rr, nW = R.reduction(F, ratio), R.n_matrices(F, btype)
    assert p["senet_w1"].shape == (F, Rr) and p["senet_w2"].shape == (Rr, F)
    assert p["bilinear_w"].shape == (nW, D, D) and p["senet_bilinear_w"].shape == (nW, D, D)
    assert p["dnn_layer_0_weights"].shape[0] == 2 * R.pairs(F) * D + Dn
    loss, logit, pred, grads = R.fwd_bwd(p, spec, k["idx"], k["dense"], k["y"], hp)
    assert logit.shape == (B,) and bool(torch.isfinite(loss))
    assert 0.05 < float(logit.abs().max()) < 20.0  # logits are O(1): the 1e-5 absolute tolerance means something
    for n in R.PARAMS:
        assert float(grads[n].abs().max()) > 0, n
    assert (float(grads["linear_w"].abs().max()) > 0) == use_linear
    # the l2 term covers the four interaction variables
    hp0 = dict(hp, interaction_l2_reg=0.0)
    diff = float(R.fibinet_l2(p, spec, hp) - R.fibinet_l2(p, spec, hp0))
    want = float(sum(1e-4 * 0.5 * p[n].square().sum() for n in R.PARAMS))
    assert abs(diff - want) <= 1e-12
    assert R.make_case(*R.MODEL_CASES[name], use_linear=use_linear) is k  # made once
