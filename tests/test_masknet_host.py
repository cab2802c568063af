"""CPU: pins the float64 restatement of MaskNet (tests/masknet_ref.py) - its hand-written backward against autograd
and finite differences, its cases against the deliberately wrong variants, the float32 restatement against the GPU
tolerances, the reason for float64 statistics - and the parts of th.MaskNet that need no GPU."""
import pytest
import torch
import torch.nn.functional as Fn
from sklearn.base import clone

from tests import masknet_ref as R

F64 = torch.float64
GROUP_IDS = ["B%d_F%d_D%d_N%d" % s for s in R.GROUP_CASES]
ROW_IDS = ["B%d_H%d" % s for s in R.ROW_CASES]


def _leaves(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


@pytest.mark.parametrize("shape", R.GROUP_CASES, ids=GROUP_IDS)
def test_group_backward_is_autograd_over_layer_norm(shape):
    c = R.kernel_case(*shape)
    B, F, D, N = shape
    E, gamma, beta, *Ms = _leaves(c["E"], c["gamma"], c["beta"], *c["M"])
    V = (Fn.layer_norm(E, (D,), eps=R.EPS) * gamma + beta).reshape(B, F * D)
    Ys = [M * V for M in Ms]
    sum((Y * dY).sum() for Y, dY in zip(Ys, c["dY"])).backward()
    for Y, want in zip(Ys, c["Y"]):
        assert float((Y.detach() - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    for got, want in [(E.grad, c["dE"]), (gamma.grad, c["dgamma"]), (beta.grad, c["dbeta"])] + [
            (M.grad, dM) for M, dM in zip(Ms, c["dM"])]:
        assert R.grad_measure(got, want) <= 1e-9
    if B > 8:  # the special examples
        assert float(c["E"][R.EX_ZERO].abs().max()) == 0 and float(c["dY"][0][R.EX_NO_GRAD].abs().max()) == 0
        want = [M[R.EX_ZERO] * c["beta"].reshape(-1) for M in c["M"]]  # xhat = 0: V = beta, not NaN
        assert all(torch.equal(Y[R.EX_ZERO], w) for Y, w in zip(c["Y"], want))
        assert float(c["dE"][R.EX_NO_GRAD].abs().max()) == 0
        row = c["E"][R.EX_SHIFT, 0]
        assert float(row.mean()) > 49 and float(row.std()) < 0.1
        assert float(c["E"][R.EX_SMALL, -1].std()) < 2e-3
    assert float((c["gamma"] - 1).abs().min()) > 0 and float(c["beta"].abs().min()) > 0
    assert all(torch.equal(c[n], c[n].float().double()) for n in ("E", "gamma", "beta", "dE_up"))  # float32 numbers


@pytest.mark.parametrize("shape", R.ROW_CASES, ids=ROW_IDS)
def test_row_backward_is_autograd_over_layer_norm(shape):
    c = R.row_case(*shape)
    B, H = shape
    Z, gamma, beta = _leaves(c["Z"], c["gamma"], c["beta"])
    h = torch.relu(Fn.layer_norm(Z, (H,), gamma, beta, eps=R.EPS))
    (h * c["dh"]).sum().backward()
    assert float((h.detach() - c["h"]).abs().max()) <= 1e-12 * max(1.0, float(c["h"].abs().max()))
    for got, want in ((Z.grad, c["dZ"]), (gamma.grad, c["dgamma"]), (beta.grad, c["dbeta"])):
        assert R.grad_measure(got, want) <= 1e-9
    assert float(c["pre"].abs().min()) >= R.ROW_KINK and c["attempt"] == R.ROW_ATTEMPTS[shape]
    assert 0.2 < float((c["pre"] > 0).double().mean()) < 0.8  # both sides of the relu are populated


def test_plain_mode_is_autograd():
    for shape in R.PLAIN_CASES:
        c = R.plain_case(*shape)
        X, M = _leaves(c["X"], c["M"])
        ((M * X) * c["dY"]).sum().backward()
        assert torch.equal(c["Y"], c["M"] * c["X"])
        assert R.grad_measure(M.grad, c["dM"]) <= 1e-12 and R.grad_measure(X.grad, c["dX"]) <= 1e-12


def test_backward_matches_central_finite_differences():
    rnd = R._rnd(torch.Generator().manual_seed(5))
    B, F, D, H = 2, 2, 8, 8
    E, gamma, beta = rnd(B, F, D), 1.0 + rnd(F, D, std=0.5), rnd(F, D, std=0.3)
    Ms, dYs = [rnd(B, F * D), rnd(B, F * D)], [rnd(B, F * D), rnd(B, F * D)]
    dMs, dE, dg, db = R.group_bwd(E, gamma, beta, Ms, dYs)

    def f_group(E_, g_, b_):
        return float(sum((Y * dY).sum() for Y, dY in zip(R.group_fwd(E_, g_, b_, Ms), dYs)))

    Z, g2, b2, dh = rnd(B, H), 1.0 + rnd(H, std=0.5), rnd(H, std=0.3), rnd(B, H)
    dZ, dg2, db2 = R.row_bwd(Z, g2, b2, dh)

    def f_row(Z_, g_, b_):
        return float((R.row_fwd(Z_, g_, b_) * dh).sum())

    step = 1e-6
    for f, args, grads in ((f_group, (E, gamma, beta), (dE, dg, db)), (f_row, (Z, g2, b2), (dZ, dg2, db2))):
        for k, (a, want) in enumerate(zip(args, grads)):
            num = torch.zeros_like(a)
            for i in range(a.numel()):
                hi, lo = a.clone(), a.clone()
                hi.view(-1)[i] += step
                lo.view(-1)[i] -= step
                num.view(-1)[i] = (f(*args[:k], hi, *args[k + 1:]) - f(*args[:k], lo, *args[k + 1:])) / (2 * step)
            assert R.grad_measure(num, want) <= 1e-6, (f.__name__, k)


@pytest.mark.parametrize("shape", [s for s in R.GROUP_CASES if s[0] > 8], ids=lambda s: "B%d_F%d_D%d_N%d" % s)
def test_group_cases_tell_the_wrong_variants_apart(shape):
    """The cases that carry the special examples (B > 8) see every wrong variant at the GPU tolerance, in the forward
    output (a wrong forward is a wrong backward: the backward recomputes it).  The B = 1 cases are left out on purpose:
    with F = 1 the flattened vector IS the row, and without the scaled row eps outside the root is a 5e-6 effect."""
    c = R.kernel_case(*shape)
    for wrong in R.WRONG_GROUP:
        err = max(R.logit_error(a, b) for a, b in zip(R.group_fwd(c["E"], c["gamma"], c["beta"], c["M"], wrong), c["Y"]))
        print(f"{shape} {wrong}: {err:.2e}")
        assert err > 10 * R.TOL_Y, (wrong, err)  # (unbiased variance at H = 2048 is a 2.4e-4 effect)


@pytest.mark.parametrize("shape", [s for s in R.ROW_CASES if s[0] > 8], ids=lambda s: "B%d_H%d" % s)
def test_row_cases_tell_the_wrong_variants_apart(shape):
    c = R.row_case(*shape)
    for wrong in R.WRONG_ROW:
        err = R.logit_error(R.row_fwd(c["Z"], c["gamma"], c["beta"], wrong), c["h"])
        print(f"{shape} {wrong}: {err:.2e}")
        assert err > 10 * R.TOL_Y, (wrong, err)  # (unbiased variance at H = 2048 is a 2.4e-4 effect)


@pytest.mark.parametrize("name", ["serial3", "serial3_no_dense"])
def test_serial_blocks_do_not_normalise_their_input_again(name):
    """Every serial model case with a block on a block sees it (serial1 has none)."""
    k = R.make_case(*R.MODEL_CASES[name])
    p, spec, idx, dense, hp = (k[n] for n in ("p", "spec", "idx", "dense", "hp"))
    right = R.masknet_logit(p, spec, idx, dense, hp)
    wrong = R.masknet_logit(p, spec, idx, dense, hp, wrong="renormalised")
    assert R.logit_error(wrong, right) > 10 * R.TOL_Y


def test_float32_statistics_miss_the_tolerance_on_the_shifted_row():
    """Why the kernels sum the statistics in float64: with float32 statistics the row whose mean is 50 and whose
    spread is 0.05 is off by ~1e-4; with float64 statistics rounded once everything is inside the tolerances."""
    c = R.kernel_case(300, 26, 16, 3)
    Y32, dM32, dE32, dg32, db32 = R.f32_stats_group(c)
    fwd32 = max(R.logit_error(a, b) for a, b in zip(Y32, c["Y"]))
    dm32 = max(R.grad_measure(a, b) for a, b in zip(dM32, c["dM"]))
    print(f"float32 statistics: Y {fwd32:.2e} dM {dm32:.2e} dgamma {R.grad_measure(dg32, c['dgamma']):.2e} "
          f"dE {R.grad_measure(dE32, c['dE']):.2e}")
    assert fwd32 > R.TOL_Y and dm32 > R.TOL_GRAD
    err = ((Y32[0].double() - c["Y"][0]).abs() / c["Y"][0].abs().clamp(min=1.0)).view(300, 26, 16)
    worst = int(err.view(-1).argmax())
    assert (worst // (26 * 16), worst // 16 % 26) == (R.EX_SHIFT, 0)  # ... and it is the shifted row
    fwd64, bwd64 = R.group_errors(c, *R.f64_stats_group(c))
    print(f"float64 statistics: Y {fwd64:.2e} gradients {bwd64:.2e}")
    assert fwd64 <= 0.5 * R.TOL_Y and bwd64 <= 0.5 * R.TOL_GRAD


@pytest.mark.parametrize("shape", R.GROUP_CASES, ids=GROUP_IDS)
def test_kernel_numerics_leave_room_under_the_tolerances(shape):
    fwd, bwd = R.group_errors(R.kernel_case(*shape), *R.f64_stats_group(R.kernel_case(*shape)))
    assert fwd <= 0.5 * R.TOL_Y and bwd <= 0.5 * R.TOL_GRAD, (fwd, bwd)


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_cases_in_float32_stay_within_half_the_gpu_tolerances(name):
    order, N, H, ratio, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    assert B <= 256 and F <= 6 and H <= 32
    k = R.make_case(*R.MODEL_CASES[name])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    # relu units within KINK of 0 would be excluded (at most 1 %): the cases are chosen to have none
    assert k["min_abs_pre"] >= R.MODEL_KINK > R.KINK and k["attempt"] == R.MODEL_ATTEMPTS[name]
    widths = R.block_widths(hp, F * D)
    assert [tuple(p[f"block{n}_proj_weights"].shape) for n in range(1, N + 1)] == [
        (R.agg_units(ratio, w), w) for w in widths]
    loss, logit, pred, grads = R.fwd_bwd(p, spec, idx, dense, y, hp)
    assert logit.shape == (B,) and 0.01 < float(logit.abs().max()) < 20
    assert set(grads) == set(p) and all(float(g.abs().max()) > 0 for g in grads.values())
    loss32, logit32, _, grads32 = R.fwd_bwd(R.to_f32(p), spec, idx, dense.float(), y, hp)
    worst = max(R.grad_measure(grads32[n], grads[n]) for n in grads)
    print(f"{name}: float32 CPU logit {R.logit_error(logit32, logit):.2e} worst gradient {worst:.2e}")
    assert float((logit32.double() - logit).abs().max()) <= 0.5e-5 and worst <= 0.5 * R.TOL_GRAD
    assert abs(float(loss32) - float(loss)) <= 0.5e-5
    # use_linear=False drops exactly the linear term
    from oracle import th_layers as TL
    k2 = R.make_case(*R.MODEL_CASES[name], use_linear=False)
    lin = TL.linear_layer(p, spec, idx, dense, None, None).reshape(-1)
    if torch.equal(k2["idx"], idx) and all(torch.equal(k2["p"][n], p[n]) for n in p):
        l2 = R.fwd_bwd(k2["p"], spec, idx, dense, y, k2["hp"])[1]
        assert float((logit - lin - l2).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------- th.MaskNet
def _features():
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    return df, ml_features(df)


def test_constructor_limits_name_the_limit():
    import recman_amd.th as th

    df, fd = _features()
    for kw, match in ((dict(block_order="diagonal"), "'parallel', 'serial'"), (dict(num_blocks=0), r"1\.\.8"),
                      (dict(num_blocks=9), r"1\.\.8"), (dict(block_hidden_units=30), "multiple of 4 in 8..2048"),
                      (dict(block_hidden_units=4), "multiple of 4 in 8..2048"),
                      (dict(block_hidden_units=4096), "multiple of 4 in 8..2048"),
                      (dict(reduction_ratio=0.0), "greater than 0"), (dict(embedding_size=64), "embedding_size 8/16/32"),
                      (dict(embedding_size=12), "embedding_size 8/16/32"), (dict(deep_hidden_units=()), "at least one layer"),
                      (dict(deep_dropout=(0.9, 1)), "deep_dropout")):
        with pytest.raises(ValueError, match=match):
            th.MaskNet(fd, **kw)
    from recman_amd.th import FeatureDictionary, SparseFeat

    wide = FeatureDictionary()
    for i in range(41):
        wide[f"c{i}"] = SparseFeat(name=f"c{i}", feat_size=3)
    with pytest.raises(ValueError, match=r"1\.\.40"):
        th.MaskNet(wide)
    assert "MaskNet" in th.__all__ and th.MaskNet.model == "masknet"


def test_get_params_and_clone_round_trip():
    import recman_amd.th as th

    df, fd = _features()
    kw = dict(embedding_size=16, block_order="serial", num_blocks=2, block_hidden_units=32, reduction_ratio=1.5,
              deep_hidden_units=(64, 32), deep_dropout=(1, 0.9, 0.9), deep_l2_reg=1e-4, epoch=2, batch_size=128)
    m = th.MaskNet(fd, **kw)
    got = m.get_params()
    for n, v in kw.items():
        assert got[n] == v, n
    c = clone(m)
    assert isinstance(c, th.MaskNet) and c is not m and all(c.get_params()[n] == v for n, v in kw.items())
    d = th.MaskNet(fd).get_params()
    assert (d["block_order"], d["num_blocks"], d["block_hidden_units"], d["reduction_ratio"], d["deep_hidden_units"],
            d["use_linear"], d["deep_dropout"]) == ("parallel", 3, 64, 2.0, (128, 128), True, None)
    assert set(m.hparams) >= {"block_order", "num_blocks", "block_hidden_units", "reduction_ratio",
                              "deep_hidden_units", "deep_dropout", "deep_l2_reg", "use_linear"}


def test_row_sharding_is_refused():
    import recman_amd.th as th
    from recman_amd import engine as eng

    df, fd = _features()
    m = th.MaskNet(fd, embedding_size=8)
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m._build()
    assert eng.ENGINES["masknet"] is eng.MaskNetEngine and eng.MaskNetEngine.shardable is False
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.MaskNetEngine.require_shardable()
