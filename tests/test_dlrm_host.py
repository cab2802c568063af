"""CPU: pins the DLRM restatement (tests/dlrm_ref.py) the GPU tests compare the kernels against, the kernel tests'
error bound, and the public surface of the feature that needs no GPU (th.DLRM's constructor, the engine registry, the
layer export, the C ABI).  No GPU needed."""
import os

import pytest
import torch

from tests import dlrm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32


def _small(B=4, F=5, D=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    return r(B, F, D), r(B, D), r(B, D + R.pairs(F))


@pytest.mark.parametrize("F,D", [(1, 2), (2, 3), (5, 3), (8, 4)])
def test_the_two_forms_of_interact_agree(F, D):
    E, z, _ = _small(F=F, D=D)
    X = R.interact(E, z)
    assert X.shape == (4, D + R.pairs(F))
    assert float((X - R.interact_loops(E, z)).abs().max()) < 1e-12


@pytest.mark.parametrize("F,D", [(1, 2), (2, 3), (5, 3), (8, 4)])
def test_autograd_equals_the_explicit_backward(F, D):
    E, z, dX = _small(F=F, D=D, seed=1)
    El, zl = E.clone().requires_grad_(True), z.clone().requires_grad_(True)
    (R.interact(El, zl) * dX).sum().backward()
    d_rows, dz = R.interact_bwd(E, z, dX)
    assert float((El.grad - d_rows).abs().max()) < 1e-12 and float((zl.grad - dz).abs().max()) < 1e-12
    # columns past D + P of a wider dX are never used
    wide = torch.cat([dX, torch.full((dX.shape[0], 3), float("nan"), dtype=F64)], dim=1)
    d2, z2 = R.interact_bwd(E, z, wide)
    assert torch.equal(d2, d_rows) and torch.equal(z2, dz)


def test_pair_order_on_a_hand_computed_example():
    """F = 2, D = 2: v_0 = z = (1, 2), v_1 = (3, 4), v_2 = (5, -6).  X = [z | <v1,v0>, <v2,v0>, <v2,v1>]."""
    E = torch.tensor([[[3.0, 4.0], [5.0, -6.0]]], dtype=F64)
    z = torch.tensor([[1.0, 2.0]], dtype=F64)
    assert R.interact(E, z).tolist() == [[1.0, 2.0, 11.0, -7.0, -9.0]]
    assert R.interact_loops(E, z).tolist() == [[1.0, 2.0, 11.0, -7.0, -9.0]]
    assert [R.pair_index(i, j) for i in range(1, 5) for j in range(i)] == list(range(10))
    assert (R.pair_index(1, 0), R.pair_index(2, 0), R.pair_index(2, 1), R.pair_index(3, 0)) == (0, 1, 2, 3)
    assert R.pairs(26) == 351 and R.pairs(1) == 1 and R.pairs(40) == 820
    # backward by hand: dX = (a0, a1, g10, g20, g21) = (0.5, -1, 2, 3, -4)
    dX = torch.tensor([[0.5, -1.0, 2.0, 3.0, -4.0]], dtype=F64)
    d_rows, dz = R.interact_bwd(E, z, dX)
    # dv_1 = g10 v0 + g21 v2 = 2 (1,2) - 4 (5,-6);  dv_2 = g20 v0 + g21 v1 = 3 (1,2) - 4 (3,4)
    assert d_rows.tolist() == [[[-18.0, 28.0], [-9.0, -10.0]]]
    # dz = g10 v1 + g20 v2 + (a0, a1) = 2 (3,4) + 3 (5,-6) + (0.5,-1)
    assert dz.tolist() == [[21.5, -11.0]]


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_cases_keep_clear_of_the_relu_kinks(name):
    kw = R.MODEL_CASES[name]
    k = R.make_case(**kw)
    hp, p = k["hp"], k["p"]
    assert k["model_min_abs_pre"] >= R.KINK, (name, k["model_min_abs_pre"])
    assert min(hp["embedding_l2_reg"], hp["linear_l2_reg"], hp["deep_l2_reg"]) > 0
    D, F = kw["D"], kw["F"]
    assert p["top_dnn_layer_0_weights"].shape[0] == D + R.pairs(F)  # no pad row
    n_bot = len(hp["bottom_hidden_units"]) + 1
    assert p[f"bot_dnn_layer_{n_bot - 1}_weights"].shape[1] == D and f"bot_dnn_layer_{n_bot}_weights" not in p
    loss, logit, pred, grads = R.fwd_bwd(p, k["spec"], k["idx"], k["dense"], k["y"], hp)
    assert set(grads) == set(p) and bool(torch.isfinite(loss))
    used = hp["use_linear"]
    assert (float(grads["linear_w"].abs().max()) > 0) == used and (float(grads["linear_w0"].abs().max()) > 0) == used
    assert all(float(grads[n].abs().max()) > 0 for n in R.deep_l2_names(hp))


def test_model_cases_cover_what_the_issue_names():
    c = R.MODEL_CASES
    assert {kw["D"] for kw in c.values()} >= {8, 16, 32}
    assert any(kw.get("use_linear") for kw in c.values())
    assert any(kw.get("bottom", (16,)) == () for kw in c.values())
    assert any((kw["D"] + R.pairs(kw["F"])) % 4 == 0 for kw in c.values())
    assert any((kw["D"] + R.pairs(kw["F"])) % 4 != 0 for kw in c.values())


def _wrong_restatements(E, z, dX):
    """Four deliberately wrong forms, each as (X, d_rows, dz) with the parts it leaves right taken from the contract."""
    B, F, D = E.shape
    T = F + 1
    V = R.stack_v(E, z)
    gram = torch.bmm(V, V.transpose(1, 2))
    X, (d_rows, dz) = R.interact(E, z), R.interact_bwd(E, z, dX)
    ui, uj = torch.triu_indices(T, T, offset=1)  # upper triangle, row-major: (0,1), (0,2), ..
    li, lj = torch.tril_indices(T, T, offset=0)  # the diagonal included
    out = {"upper_triangle_order": (torch.cat([z, gram[:, ui, uj]], dim=1), d_rows, dz),
           "diagonal_included": (torch.cat([z, gram[:, li, lj][:, : R.pairs(F)]], dim=1), d_rows, dz),
           "pass_through_dropped": (torch.cat([torch.zeros_like(z), X[:, D:]], dim=1), d_rows, dz),
           "dz_without_pass_through": (X, d_rows, dz - dX[:, :D])}
    return out


@pytest.mark.parametrize("shape", [(5, 3, 8), (7, 31, 16), (64, 26, 16)])
def test_the_kernel_bound_catches_wrong_restatements(shape):
    case = R.kernel_case(*shape)
    E, z, dX = case["E"], case["z"], case["dX"]
    assert R.check_fwd(R.interact(E, z), case) == 0.0 and R.check_bwd(*R.interact_bwd(E, z, dX), case) == (0.0, 0.0)
    for name, (X, d_rows, dz) in _wrong_restatements(E, z, dX).items():
        with pytest.raises(AssertionError):
            R.check_fwd(X, case)
            R.check_bwd(d_rows, dz, case)
        # ... and by orders of magnitude, not by a rounding error
        D = case["D"]
        off = max(R._ratio((X[:, D:] - case["X"][:, D:]).abs(), case["bx"]),
                  R._ratio((dz - case["dz"]).abs(), case["bdv"][:, 0]),
                  float("inf") if not torch.equal(X[:, :D], z) else 0.0)
        assert off > 1e3, (name, off)
    # pad columns: anything but +0.0 fails
    for bad in (1.0, -0.0, float("nan")):
        with pytest.raises(AssertionError):
            R.check_fwd(torch.cat([case["X"], torch.full((shape[0], 2), bad, dtype=F64)], dim=1), case)
    R.check_fwd(torch.cat([case["X"], torch.zeros(shape[0], 2, dtype=F64)], dim=1), case)


@pytest.mark.parametrize("shape", [(5, 1, 8), (7, 31, 16), (3, 32, 16), (4, 40, 64), (64, 26, 16)])
def test_the_float32_restatement_stays_inside_the_kernel_bound(shape):
    case = R.kernel_case(*shape)
    E, z, dX = (case[n].to(F32) for n in ("E", "z", "dX"))
    rx = R.check_fwd(R.interact(E, z), case)
    rr, rz = R.check_bwd(*R.interact_bwd(E, z, dX), case)
    print(f"{shape}: float32 CPU err / bound: X {rx:.3f}, d_rows {rr:.3f}, dz {rz:.3f}")
    assert max(rx, rr, rz) <= 0.5


def test_kernel_cases_have_the_zero_examples():
    for shape in R.GPU_CASES[:-1]:
        case = R.kernel_case(*shape)
        assert float(case["E"][1].abs().max()) == 0.0 and float(case["z"][2].abs().max()) == 0.0
        assert float(case["X"][1, case["D"]:].abs().max()) == 0.0  # every pair has an E row
        assert torch.equal(case["dz"][1], case["dX"][1, : case["D"]])  # all E rows zero: dz is the pass-through alone


# ------------------------------------------------------------------------------------------ the public surface
def _fd():
    from recman_amd.th import DenseFeat, FeatureDictionary, SparseFeat

    fd = FeatureDictionary()
    fd["a"], fd["b"], fd["x"] = SparseFeat("a", 5), SparseFeat("b", 7), DenseFeat("x")
    return fd


def test_constructor_checks_deep_dropout_and_round_trips_through_clone():
    from sklearn.base import clone

    import recman_amd.th as th

    assert th.DLRM.model == "dlrm" and "DLRM" in th.__all__
    with pytest.raises(ValueError, match="deep_dropout needs 3"):
        th.DLRM(_fd(), deep_dropout=(1, 0.8))
    m = th.DLRM(_fd(), embedding_size=16, bottom_hidden_units=[24], deep_hidden_units=(16, 8), deep_dropout=(1, 0.9, 0.9),
                use_linear=True, deep_l2_reg=1e-4)
    assert m.hparams["bottom_hidden_units"] == (24,) and m.hparams["deep_hidden_units"] == (16, 8)
    assert m.hparams["deep_dropout"] == (1, 0.9, 0.9) and m.hparams["use_linear"] is True
    assert th.DLRM(_fd()).hparams["deep_dropout"] == (1, 1, 1) and th.DLRM(_fd()).hparams["use_linear"] is False
    assert th.DLRM(_fd()).hparams["bottom_hidden_units"] == (64, 32)
    c = clone(m)
    assert isinstance(c, th.DLRM) and c._engine is None and c.hparams == m.hparams
    got = c.get_params()
    assert got["bottom_hidden_units"] == [24] and got["deep_dropout"] == (1, 0.9, 0.9) and got["use_linear"] is True
    assert clone(th.DLRM(_fd())).get_params()["deep_dropout"] is None
    assert th.DLRM(_fd(), loss_type="mse").task == "regression"


def test_engine_registry_layer_export_and_abi():
    from recman_amd import _lib, engine as eng
    from recman_amd.th import layers as L

    assert eng.ENGINES["dlrm"] is eng.DLRMEngine and eng.DLRMEngine.model == "dlrm"
    assert eng.DLRMEngine.use_bias_tables is False
    assert callable(L.DotInteraction())
    for name in ("rm_dot_interact_supported", "rm_dot_interact_fwd", "rm_dot_interact_bwd"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    for name in ("rm_dot_interact_supported", "rm_dot_interact_fwd", "rm_dot_interact_bwd"):
        assert f"int {name}(" in header
    assert os.path.exists(os.path.join(ROOT, "recman_amd", "csrc", "dot_interact.hip"))
