"""CPU: the float64 restatement of the field-pair weighted FM family (tests/fmfm_ref.py) pinned against explicit loops,
autograd and plain FM; the float32 restatement's own error on every GPU case against the tolerances the GPU tests use;
the deliberately wrong variants against those tolerances."""
import itertools

import pytest
import torch

from tests import fmfm_ref as R

F64 = torch.float64


@pytest.mark.parametrize("ftype", R.TYPES)
def test_tensor_form_equals_the_loops(ftype):
    for B, F, D in ((3, 2, 8), (4, 5, 8), (2, 7, 16)):
        c = R.kernel_case(B, F, D, ftype, seed=1)
        a, b = R.pair_logit(c["E"], c["W"], ftype), R.pair_logit_loops(c["E"], c["W"], ftype)
        assert float(((a - b).abs() / b.abs().clamp(min=1e-3)).max()) <= 1e-12


def test_pair_order_is_combinations():
    for F in (2, 3, 5, 26, 40):
        li, lj = R.pair_fields(F)
        assert list(zip(li.tolist(), lj.tolist())) == list(itertools.combinations(range(F), 2))
        assert li.numel() == R.pairs(F)
    # a weight that is zero but for pair p picks out exactly fields (i, j) of combinations order, left field on rows
    F, D = 4, 8
    g = torch.Generator().manual_seed(3)
    E = torch.randn(2, F, D, generator=g, dtype=F64)
    for p, (i, j) in enumerate(itertools.combinations(range(F), 2)):
        W = torch.zeros(R.pairs(F), D, D, dtype=F64)
        W[p] = torch.randn(D, D, generator=g, dtype=F64)
        want = torch.einsum("bk,kd,bd->b", E[:, i], W[p], E[:, j])
        assert torch.allclose(R.pair_logit(E, W, "matrix"), want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("ftype", R.TYPES)
def test_written_out_backward_equals_autograd(ftype):
    for B, F, D in ((5, 2, 8), (9, 5, 8), (12, 7, 16), (4, 6, 32)):
        c = R.kernel_case(B, F, D, ftype, seed=2)
        E, W = c["E"].clone().requires_grad_(True), c["W"].clone().requires_grad_(True)
        (R.pair_logit(E, W, ftype) * c["g"]).sum().backward()
        dE, dW = R.pair_bwd(c["E"], c["W"], ftype, c["g"])
        assert R.grad_measure(dE, E.grad) <= 1e-11 and R.grad_measure(dW, W.grad) <= 1e-11
        assert tuple(dW.shape) == R.weight_shape(F, D, ftype)


@pytest.mark.parametrize("ftype", R.TYPES)
def test_initial_weights_are_plain_fm(ftype):
    for B, F, D in ((6, 2, 8), (6, 5, 16), (4, 26, 16)):
        E = R.kernel_case(B, F, D, ftype)["E"]
        W = R.init_weights(F, D, ftype)
        assert tuple(W.shape) == R.weight_shape(F, D, ftype)
        got, want = R.pair_logit(E, W, ftype), R.fm_second_order(E)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("ftype", R.TYPES)
@pytest.mark.parametrize("shape", R.GPU_CASES, ids=lambda s: "B%d_F%d_D%d" % s)
def test_gpu_cases_float32_error_and_wrong_variants(shape, ftype):
    B, F, D = shape
    c = R.kernel_case(B, F, D, ftype)
    assert all(torch.equal(c[n], c[n].float().double()) for n in ("E", "W", "g", "dE_up"))  # float32 numbers
    if B > 8:
        assert float(c["E"][3].abs().max()) == 0 and float(c["g"][4]) == 0
        assert float(c["logit"][3]) == 0 and float(c["dE"][3].abs().max()) == 0 and float(c["dE"][4].abs().max()) == 0
    assert 0.05 < float(c["logit"].abs().max()) < 500  # logits are O(1) (the E x 8 row: x 64)
    e_logit, e_dE, e_dW = R.f32_errors(c)
    print(f"{shape} {ftype}: float32 CPU logit {e_logit:.2e} dE {e_dE:.2e} dW {e_dW:.2e}")
    assert e_logit <= 0.5 * R.TOL_LOGIT and e_dE <= 0.5 * R.TOL_GRAD and e_dW <= 0.5 * R.TOL_GRAD
    for wrong in R.WRONG:
        err = R.logit_error(R.pair_logit(c["E"], c["W"], ftype, wrong), c["logit"])
        if R.wrong_applies(wrong, F, ftype):
            assert err > 100 * R.TOL_LOGIT, (wrong, err)
        else:
            assert err == 0.0, (wrong, err)


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_cases(name):
    ftype, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    k = R.make_case(*R.MODEL_CASES[name])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert k["min_abs_pre"] >= R.KINK and hp["interaction_l2_reg"] == 1e-4
    assert tuple(p["field_pair_w"].shape) == R.weight_shape(F, D, ftype)
    loss, logit, pred, grads = R.fwd_bwd(p, spec, idx, dense, y, hp)
    assert logit.shape == (B,) and 0.01 < float(logit.abs().max()) < 20  # logits are O(1)
    assert set(grads) == set(p) and all(float(g.abs().max()) > 0 for g in grads.values())
    want = 0.5 * 1e-4 * float(p["field_pair_w"].square().sum())
    assert abs(float(R.interaction_l2(p, 1e-4)) - want) <= 1e-15
    hp0 = dict(hp, interaction_l2_reg=0.0)
    assert abs(float(R.fmfm_l2(p, spec, hp)) - float(R.fmfm_l2(p, spec, hp0)) - want) <= 1e-12
    # use_linear=False drops exactly the linear term
    k2 = R.make_case(*R.MODEL_CASES[name], use_linear=False)
    l2 = R.fwd_bwd(k2["p"], spec, idx, dense, y, k2["hp"])[1]
    from oracle import th_layers as TL
    lin = TL.linear_layer(p, spec, idx, dense, None, None).reshape(-1)
    assert torch.equal(k2["idx"], idx) and float((logit - lin - l2).abs().max()) <= 1e-12
