"""CPU: pins the restatement of DCN-Mix (tests/crossmix_ref.py) that the GPU tests compare the kernels against, the
tolerances those tests use, and the public surface.  No GPU and no kernel is touched."""
import math
import os

import pytest
import torch

from tests import crossmix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
GRID_STRIDE = (131073, 3, 8)  # tests/test_gpu_cross_mix.py: the grid-stride case
KERNEL_CASES = R.GPU_CASES + [GRID_STRIDE]
ENTRY_POINTS = ("rm_cross_mix_supported", "rm_cross_mix_fwd", "rm_cross_mix_bwd_workspace", "rm_cross_mix_bwd")


def _rand(B, E, r, seed=1):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=F64, generator=g)  # noqa: E731
    return rn(B, E * r), rn(B, E), rn(E, r, r), rn(B, E * r)


@pytest.mark.parametrize("shape", [(4, 1, 2), (4, 2, 3), (5, 3, 4)])
def test_explicit_backward_equals_autograd(shape):
    t, s, C, dm = _rand(*shape)
    tl, sl, Cl = (x.clone().requires_grad_(True) for x in (t, s, C))
    m = R.core_fwd(tl, sl, Cl)
    (m * dm).sum().backward()
    dt, ds, dC = R.core_bwd(t, s, C, dm)
    for got, want in ((dt, tl.grad), (ds, sl.grad), (dC, Cl.grad)):
        assert float((got - want).abs().max()) <= 1e-12
    assert float((R.core_loops(t, s, C) - m.detach()).abs().max()) <= 1e-12
    # the kernels' tanh form is the same function
    assert float((R.core_fwd(t, s, C, R.tanh_exp) - m.detach()).abs().max()) <= 1e-12


def test_hand_computed_example():
    """E = 2, r = 1: t = (0.5, -1), s = (0, ln 3) so p = (1/4, 3/4), C = ((2), (-0.5)), dm = (1, 2)."""
    t, s = torch.tensor([[0.5, -1.0]], dtype=F64), torch.tensor([[0.0, math.log(3.0)]], dtype=F64)
    C, dm = torch.tensor([[[2.0]], [[-0.5]]], dtype=F64), torch.tensor([[1.0, 2.0]], dtype=F64)
    a = [math.tanh(0.5), math.tanh(-1.0)]
    c = [math.tanh(2.0 * a[0]), math.tanh(-0.5 * a[1])]
    p = [0.25, 0.75]
    m = R.core_fwd(t, s, C)
    assert abs(float(m[0, 0]) - p[0] * c[0]) < 1e-15 and abs(float(m[0, 1]) - p[1] * c[1]) < 1e-15
    dp = [1.0 * c[0], 2.0 * c[1]]
    mean = p[0] * dp[0] + p[1] * dp[1]
    dh = [p[0] * 1.0 * (1 - c[0] ** 2), p[1] * 2.0 * (1 - c[1] ** 2)]
    dt, ds, dC = R.core_bwd(t, s, C, dm)
    for i in range(2):
        assert abs(float(ds[0, i]) - p[i] * (dp[i] - mean)) < 1e-15
        assert abs(float(dC[i, 0, 0]) - a[i] * dh[i]) < 1e-15
        assert abs(float(dt[0, i]) - dh[i] * float(C[i, 0, 0]) * (1 - a[i] ** 2)) < 1e-15
    assert abs(float(ds.sum())) < 1e-15  # the softmax's gradient sums to zero


def test_one_expert_has_no_gate_gradient():
    t, s, C, dm = _rand(6, 1, 4)
    for dtype in (F64, torch.float32):
        ds = R.core_bwd(t.to(dtype), s.to(dtype), C.to(dtype), dm.to(dtype))[1]
        assert float(ds.abs().max()) == 0.0
    k = R.make_case(*R.MODEL_CASES["e1_r8"], l2=0.0)
    for p, dense in ((k["p"], k["dense"]), (R.to_f32(k["p"]), k["dense"].float())):
        grads = R.fwd_bwd(p, k["spec"], k["idx"], dense, k["y"], k["hp"])[3]
        assert float(grads["cross_gate"].abs().max()) == 0.0 and float(grads["cross_v"].abs().max()) > 0


@pytest.mark.parametrize("shape", KERNEL_CASES, ids=lambda s: "B%d_E%d_r%d" % s)
def test_float32_restatement_stays_under_half_the_kernel_tolerances(shape):
    case = R.kernel_case(*shape)
    for name, tanh in (("libm", torch.tanh), ("exp form", R.tanh_exp)):
        em, mt, ms, mc = R.f32_errors(case, tanh)
        print(f"{shape} {name}: M {em:.2e}, dT {mt:.2e}, dS {ms:.2e}, dC {mc:.2e}")
        assert em <= 0.5 * R.TOL_M and max(mt, ms) <= 0.5 * R.TOL_GRAD
        # dC is a sum over the batch: its tolerance is max(2e-5, 4 x this restatement's own error), which a float32
        # sum over 131 073 examples needs on some hosts (3e-5 was seen where the library sums in one long chain)
        assert mc <= 0.5 * max(R.TOL_GRAD, 4 * mc) and (shape[0] > 1000 or mc <= 0.5 * R.TOL_GRAD)


@pytest.mark.parametrize("shape", [(33, 3, 8), (64, 4, 32), (65, 2, 64)])
def test_wrong_restatements_exceed_the_tolerances_a_hundredfold(shape):
    case = R.kernel_case(*shape)
    t, s, C, dm = (case[n] for n in ("t", "s", "C", "dm"))
    for wrong in ("no_p", "no_second_tanh", "c_transposed", "blocks_swapped"):
        err = float((R.core_fwd(t, s, C, wrong=wrong) - case["m"]).abs().max())
        assert err > 100 * R.TOL_M, (wrong, err)
    ds = R.core_bwd(t, s, C, dm, wrong="ds_without_mean")[1]
    assert R.grad_measure(ds, case["ds"]) > 100 * R.TOL_GRAD
    # a transposed C in the backward alone
    dt = R.core_bwd(t, s, C.transpose(1, 2), dm)[0]
    assert R.grad_measure(dt, case["dt"]) > 100 * R.TOL_GRAD


@pytest.mark.parametrize("shape", [c for c in KERNEL_CASES if c[0] > 8], ids=lambda s: "B%d_E%d_r%d" % s)
def test_special_rows_are_what_they_claim(shape):
    B, E, r = shape
    case = R.kernel_case(*shape)
    t, s, dm, m = (case[n] for n in ("t", "s", "dm", "m"))
    # saturated: some |tanh(t)| rounds to 1 in float32
    assert float(t[3].abs().max()) > 8.0 and float((1 - torch.tanh(t[3]).abs()).min()) < 2.0 ** -25
    assert float(t[4].abs().max()) == 0.0 and float(m[4].abs().max()) == 0.0
    assert float(case["dt"][4].abs().max()) > 0  # ... while its gradient is alive
    if E >= 2:
        assert float(s[5].abs().max()) > 100
        naive = torch.exp(s[5].float()) / torch.exp(s[5].float()).sum()  # no max-subtraction: inf / inf
        assert not bool(torch.isfinite(naive).all())
    assert bool(torch.isfinite(m[5]).all())
    assert float(s[6].abs().max()) == 0.0
    c6 = torch.tanh(torch.einsum("ij,ijk->ik", torch.tanh(t[6].reshape(E, r)), case["C"]))
    assert float((m[6].reshape(E, r) * E - c6).abs().max()) < 1e-15  # p = 1/E
    assert float(dm[7].abs().max()) == 0.0
    assert float(case["dt"][7].abs().max()) == 0.0 and float(case["ds"][7].abs().max()) == 0.0
    assert torch.equal(case["C"], case["C"].float().double()) and torch.equal(t, t.float().double())


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
@pytest.mark.parametrize("use_linear", [True, False])
def test_float32_model_stays_under_half_the_model_tolerances(name, use_linear):
    k = R.make_case(*R.MODEL_CASES[name], use_linear=use_linear)
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert k["min_abs_pre"] >= R.KINK and hp["cross_layer_l2_reg"] == 1e-4
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp)
    expected = set(p) if use_linear else set(p) - {"linear_w", "linear_w0"}
    assert {n for n, g in ref[3].items() if float(g.abs().max()) > 0} == expected
    for tanh in (torch.tanh, R.tanh_exp):
        got = R.fwd_bwd(R.to_f32(p), spec, idx, dense.float(), y, hp, tanh=tanh)
        err = float((got[1].double() - ref[1]).abs().max())
        worst = max(R.grad_measure(got[3][n], ref[3][n]) for n in ref[3])
        print(f"{name}: logit err {err:.2e}, worst gradient measure {worst:.2e}")
        assert err <= 0.5 * 1e-5 and worst <= 0.5 * R.TOL_GRAD
    # the composition: dnn + cross (+ dnn under strict_reference) (+ linear)
    from oracle import th_layers as TL

    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False)
    x = TL.dnn_input(E, dense)
    dnn = TL.dnn(p, x, 2)
    lin = TL.linear_layer(p, spec, idx, dense) if use_linear else 0.0
    want = dnn + R.cross_mix_net(p, x) + lin
    assert float((R.dcn_mix_logit(p, spec, idx, dense, hp) - want).abs().max()) < 1e-12
    strict = R.dcn_mix_logit(p, spec, idx, dense, dict(hp, strict_reference=True))
    assert float((strict - want - dnn).abs().max()) < 1e-12
    # l2: reg 0.5 sum w^2 over cross_v, cross_gate, cross_c, cross_u, cross_w_out - not cross_b
    l2 = R.cross_mix_l2(p, 1e-4)
    assert abs(float(l2) - 0.5e-4 * sum(float(p[n].square().sum()) for n in R.CROSS_L2_NAMES)) < 1e-15
    assert "cross_b" not in R.CROSS_L2_NAMES and "cross_w" not in p


def test_the_gate_is_per_layer():
    k = R.make_case(*R.MODEL_CASES["e4_r16"])
    p = dict(k["p"])
    x = torch.randn(7, p["cross_v"].shape[1], dtype=F64, generator=torch.Generator().manual_seed(3))
    base = R.cross_mix_net(p, x)
    p["cross_gate"] = p["cross_gate"].clone()
    p["cross_gate"][1] += 1.0 * torch.randn(p["cross_gate"][1].shape, dtype=F64,
                                            generator=torch.Generator().manual_seed(4))
    assert float((R.cross_mix_net(p, x) - base).abs().max()) > 1e-6  # layer 1 has a gate of its own


# ------------------------------------------------------------------------------------------ the public surface
def _fd():
    from recman_amd.th import DenseFeat, FeatureDictionary, SparseFeat

    fd = FeatureDictionary()
    fd["a"], fd["b"], fd["x"] = SparseFeat("a", 5), SparseFeat("b", 7), DenseFeat("x")
    return fd


def test_constructor_defaults_and_clone_round_trip():
    from sklearn.base import clone

    import recman_amd.th as th

    m = th.DCN(_fd())
    assert m.hparams["cross_type"] == "vector" and m.hparams["cross_experts"] == 4 and m.hparams["cross_low_rank"] == 32
    m = th.DCN(_fd(), cross_type="mix", cross_experts=2, cross_low_rank=16, cross_layer_num=2)
    got = m.get_params()
    assert got["cross_type"] == "mix" and got["cross_experts"] == 2 and got["cross_low_rank"] == 16
    c = clone(m)
    assert isinstance(c, th.DCN) and c._engine is None and c.hparams == m.hparams
    # the new keywords come after the existing ones
    import inspect

    names = list(inspect.signature(th.DCN.__init__).parameters)
    assert names[-3:] == ["cross_type", "cross_experts", "cross_low_rank"]
    # the other cross types carry the keywords along and ignore them
    assert th.DCN(_fd(), cross_type="matrix", cross_experts=99).hparams["cross_experts"] == 99


def test_engine_registry_layer_export_and_abi():
    from recman_amd import _lib, engine as eng, ops
    from recman_amd.th import layers as L

    assert eng.ENGINES["dcn"] is eng.DCNEngine and hasattr(eng, "CrossMix")
    assert "CrossNetMix" in L.__all__ and "CrossNet" in L.__all__ and L.CrossNetMix.display_name == "CrossNetMix"
    header = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    bound = dict(_lib.SIGNATURES, **_lib.SIGNATURES_I64)
    for name in ENTRY_POINTS:
        assert name in bound and f" {name}(" in header, name
    assert "rm_cross_mix_bwd_workspace" in _lib.SIGNATURES_I64
    assert len(_lib.SIGNATURES["rm_cross_mix_fwd"]) == 11 and len(_lib.SIGNATURES["rm_cross_mix_bwd"]) == 17
    assert os.path.exists(os.path.join(ROOT, "recman_amd", "csrc", "cross_mix.hip"))
    for fn in ("cross_mix_supported", "cross_mix_fwd", "cross_mix_bwd_workspace", "cross_mix_bwd"):
        assert callable(getattr(ops, fn))
    # the launch constants ops mirrors are the kernel file's own
    src = open(os.path.join(ROOT, "recman_amd", "csrc", "cross_mix.hip")).read()
    assert f"kFwdBlocks = {ops.CROSS_MIX_FWD_BLOCKS};" in src and f"kBwdBlocks = {ops.CROSS_MIX_BWD_BLOCKS};" in src
    assert "kTileFloats = 4096;" in src and "kMaxG = 64;" in src and "kGE = 4;" in src
    assert [ops.cross_mix_tile(E, r) for E, r in ((1, 8), (3, 8), (5, 16), (4, 32), (8, 32))] == [64, 64, 48, 32, 16]
    assert GRID_STRIDE[0] == ops.CROSS_MIX_FWD_BLOCKS * ops.cross_mix_tile(3, 8) + 1
