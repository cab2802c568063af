"""CPU: pins the AutoInt restatement (tests/autoint_ref.py) the GPU tests compare the kernels against, and the public
surface of the feature (th.AutoInt's constructor, the engine registry, the layer export, the C ABI).  No GPU needed."""
import inspect
import math
import os

import pytest
import torch

from oracle import th_layers as TL
from tests import autoint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _small(B=3, F=4, Din=3, H=2, dk=2, seed=0, res=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    HD = H * dk
    X, Wq, Wk, Wv, Wr = r(B, F, Din) * 0.7, r(Din, HD) * 0.6, r(Din, HD) * 0.6, r(Din, HD) * 0.6, r(Din, HD) * 0.6
    return X, Wq, Wk, Wv, (Wr if res else None)


def _loops(X, Wq, Wk, Wv, Wr, H, scale):
    """The contract as a plain-Python triple loop (lists and floats, no tensor arithmetic)."""
    X, Wq, Wk, Wv = X.tolist(), Wq.tolist(), Wk.tolist(), Wv.tolist()
    Wr = Wr.tolist() if Wr is not None else None
    B, F, Din, HD = len(X), len(X[0]), len(Wq), len(Wq[0])
    dk = HD // H
    proj = lambda x, W: [sum(x[i] * W[i][j] for i in range(Din)) for j in range(HD)]  # noqa: E731
    out = []
    for n in range(B):
        Q, K, V = ([proj(X[n][f], W) for f in range(F)] for W in (Wq, Wk, Wv))
        rows = []
        for m in range(F):
            y = []
            for h in range(H):
                cols = range(h * dk, (h + 1) * dk)
                s = [scale * sum(Q[m][j] * K[k][j] for j in cols) for k in range(F)]
                mx = max(s)
                e = [math.exp(v - mx) for v in s]
                den = sum(e)
                y += [sum(e[k] / den * V[k][j] for k in range(F)) for j in cols]
            if Wr is not None:
                y = [a + b for a, b in zip(y, proj(X[n][m], Wr))]
            rows.append([max(v, 0.0) for v in y])
        out.append(rows)
    return torch.tensor(out, dtype=F64)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_restatement_equals_a_plain_triple_loop(res, scale):
    X, Wq, Wk, Wv, Wr = _small(res=res)
    got = R.interacting_layer(X, Wq, Wk, Wv, Wr, 2, scale)
    assert got.shape == (3, 4, 4)
    assert float((got - _loops(X, Wq, Wk, Wv, Wr, 2, scale)).abs().max()) < 1e-12


def test_closed_form_a_single_field():
    """F = 1: the weight is 1 whatever Q and K are, Y = relu(X (Wv + Wr))."""
    X, Wq, Wk, Wv, Wr = _small(F=1, Din=5, H=2, dk=3)
    want = torch.relu(X @ (Wv + Wr))
    assert float((R.interacting_layer(X, Wq, Wk, Wv, Wr, 2) - want).abs().max()) < 1e-14
    leaves = [t.clone().requires_grad_(True) for t in (X, Wq, Wk, Wv, Wr)]
    R.interacting_layer(*leaves, 2).sum().backward()
    assert float(leaves[1].grad.abs().max()) < 1e-15 and float(leaves[2].grad.abs().max()) < 1e-15
    got = R.interacting_layer_bwd(X, Wq, Wk, Wv, Wr, 2, 1.0, torch.ones(3, 1, 6, dtype=F64))
    assert float(got[1].abs().max()) < 1e-15 and float(got[2].abs().max()) < 1e-15


def test_closed_form_uniform_attention_is_the_field_mean():
    """Wq = 0: every score is 0, the weights are uniform, O is the mean of V over the fields."""
    X, Wq, Wk, Wv, _ = _small(F=6, Din=5, H=2, dk=3)
    a, V, pre, _ = R.interacting_parts(X, torch.zeros_like(Wq), Wk, Wv, None, 2)
    assert float((a - 1.0 / 6).abs().max()) < 1e-15
    want = (X @ Wv).mean(dim=1, keepdim=True).expand(-1, 6, -1)
    assert float((pre - want).abs().max()) < 1e-14


def test_a_permutation_of_the_fields_permutes_the_output_and_the_logit_follows():
    X, Wq, Wk, Wv, Wr = _small(F=7, Din=4, H=2, dk=3)
    perm = torch.tensor([3, 0, 6, 1, 5, 2, 4])
    Y, Yp = R.interacting_layer(X, Wq, Wk, Wv, Wr, 2), R.interacting_layer(X[:, perm], Wq, Wk, Wv, Wr, 2)
    assert float((Y[:, perm] - Yp).abs().max()) < 1e-13
    g = torch.Generator().manual_seed(5)
    w, w0 = torch.randn(7, 6, generator=g, dtype=F64), torch.randn(1, generator=g, dtype=F64)
    assert float((R.head(Y, w, w0) - R.head(Yp, w[perm], w0)).abs().max()) < 1e-13
    assert float((R.head(Y, w, w0) - ((Y * w).sum(dim=(1, 2)) + w0)).abs().max()) < 1e-13


def test_gradcheck_float64():
    for res in (True, False):
        X, Wq, Wk, Wv, Wr = _small(B=2, F=3, Din=3, H=2, dk=2, seed=3, res=res)
        leaves = [t.clone().requires_grad_(True) for t in (X, Wq, Wk, Wv) + ((Wr,) if res else ())]
        fn = lambda *a: R.interacting_layer(*a, *(() if res else (None,)), 2, 0.7)  # noqa: E731
        pre = R.interacting_parts(X, Wq, Wk, Wv, Wr, 2, 0.7)[2]
        assert float(pre.abs().min()) > 1e-4  # no unit at its kink: the finite differences stay on one side
        assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("res,up,scale", [(True, False, 1.0), (False, True, 1.0), (True, True, 0.5),
                                          (False, False, 0.5)])
def test_written_out_backward_equals_autograd(res, up, scale):
    X, Wq, Wk, Wv, Wr = _small(B=5, F=6, Din=4, H=2, dk=3, seed=5, res=res)
    g0 = torch.Generator().manual_seed(9)
    dY = torch.randn(5, 6, 6, generator=g0, dtype=F64)
    dX_up = torch.randn(5, 6, 4, generator=g0, dtype=F64) if up else None
    leaves = [t.clone().requires_grad_(True) for t in (X, Wq, Wk, Wv) + ((Wr,) if res else ())]
    (R.interacting_layer(*leaves, *(() if res else (None,)), 2, scale) * dY).sum().backward()
    got = R.interacting_layer_bwd(X, Wq, Wk, Wv, Wr, 2, scale, dY, dX_up)
    want = [t.grad for t in leaves]
    if up:
        want[0] = want[0] + dX_up
    assert (got[4] is None) == (not res)
    for a, c, name in zip(got, want, ("dX", "dWq", "dWk", "dWv", "dWr")):
        assert float((a - c).abs().max()) < 1e-12, name


def test_softmax_is_max_subtracted():
    """Scores in the hundreds: a softmax without max subtraction is not finite, the restatement is, in both types."""
    k = R.gpu_case(R.RANGE_CASES[0], q_scale=R.RANGE_Q_SCALE)
    s = R.interacting_parts(k["X"], k["Wq"], k["Wk"], k["Wv"], k["Wr"], k["H"])[3]
    assert float(s.max()) > 89.0 and float(s.min()) < -89.0  # exp overflows fp32 beyond 88.7
    args = ("X", "Wq", "Wk", "Wv", "Wr")
    y64 = R.interacting_layer(*(k[n] for n in args), k["H"])
    y32 = R.interacting_layer(*(k[n].float() for n in args), k["H"])
    assert bool(torch.isfinite(y32).all()) and float((y32.double() - y64).abs().max()) < 1e-4


def test_model_composition_matches_its_parts():
    k = R.make_case(B=12, F=5, D=8, Dn=2, L=2, H=2, dk=4, seed=2, hidden=(6, 5))
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    loss, logit, pred, grads = R.fwd_bwd(p, spec, idx, dense, y, hp)
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False)
    x = E
    for l in range(2):
        x = R.interacting_layer(x, *(p[n] for n in R.layer_names(l)), 2)
    want = (TL.linear_layer(p, spec, idx, dense).reshape(-1) + R.head(x, p["autoint_w"], p["autoint_w0"])
            + TL.dnn(p, TL.dnn_input(E, dense), 2).reshape(-1))
    assert float((logit - want).abs().max()) < 1e-13
    att = sum(p[n].square().sum() for l in range(2) for n in R.layer_names(l)) + p["autoint_w"].square().sum()
    l2 = 1e-3 * 0.5 * (sum(p[f"{n}_feat_embed"].square().sum() for n in spec.sparse_names)
                       + p["linear_w"].square().sum() + att) + TL.dnn_l2(p, 2, 1e-3)
    assert abs(float(loss) - float(TL.create_loss(y, TL.prediction(want)) + l2)) < 1e-13
    assert set(grads) == set(p) and all(float(g.abs().max()) > 0 for g in grads.values())
    assert not any(n.endswith("_feat_bias") for n in p)
    assert set(R.att_names(hp)) == {n for n in p if n.startswith("autoint") and n != "autoint_w0"}
    # without a DNN and without the residual: fewer variables
    k2 = R.make_case(B=12, F=5, D=8, Dn=2, L=1, H=2, dk=4, seed=2, att_res=False)
    assert not any(n.startswith("dnn") or n.endswith("res_w") for n in k2["p"])
    assert k2["p"]["autoint_layer_0_query_w"].shape == (8, 8) and k2["p"]["autoint_w"].shape == (40, 1)


# ------------------------------------------------------------------------------------------- the kink guard
@pytest.mark.parametrize("case", R.GPU_CASES + [c + ("range",) for c in R.RANGE_CASES])
def test_kink_guard_zeroes_at_most_a_fifth_of_every_gpu_case(case):
    q_scale = R.RANGE_Q_SCALE if case[-1] == "range" else 1.0
    k = R.gpu_case(case[:5], q_scale=q_scale)
    print(f"{case}: zeroed {k['zeroed']:.4f}")
    assert k["zeroed"] <= R.KINK_CAP, k["zeroed"]
    near = k["near"]
    assert bool((k["dY"][near] == 0).all()) and bool((k["dY"][~near].abs().flatten(1).max(dim=1).values > 0).all())


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_cases_have_no_unit_at_its_kink(name):
    assert R.make_case(**R.MODEL_CASES[name])["model_min_abs_pre"] >= R.KINK


# ------------------------------------------------------------------------------------------------- surface
def test_constructor_signature_and_defaults():
    from sklearn.metrics import log_loss, roc_auc_score

    import recman_amd.th as th

    params = list(inspect.signature(th.AutoInt.__init__).parameters.values())[1:]
    want = [("feat_dict", inspect.Parameter.empty), ("embedding_size", 8), ("att_layer_num", 3),
            ("att_embedding_size", 8), ("att_head_num", 2), ("att_res", True), ("att_scaling", False),
            ("att_l2_reg", 0.0), ("deep_hidden_units", ()), ("deep_dropout", None), ("deep_l2_reg", 0.0),
            ("deep_activation", "relu"), ("embedding_l2_reg", 0.00001), ("linear_l2_reg", 0.00001), ("epoch", 10),
            ("batch_size", 256), ("learning_rate", 0.001), ("optimizer", "adam"), ("random_seed", 2019),
            ("loss_type", "logloss"), ("eval_metric", (roc_auc_score, log_loss)), ("what_means_greater", None),
            ("use_interactive_session", True), ("log_dir", "./logs"), ("strict_reference", False), ("device", "cuda")]
    assert [(p.name, p.default) for p in params] == want
    assert th.AutoInt.model == "autoint" and "AutoInt" in th.__all__


def test_engine_is_registered_and_layer_is_exported():
    from recman_amd import engine
    from recman_amd.th import layers

    assert "autoint" in engine.ENGINES and engine.ENGINES["autoint"].model == "autoint"
    assert engine.ENGINES["autoint"].use_bias_tables is False
    assert engine.DeepFMEngine.needs_fm_or_deep is True  # DeepFM keeps its rule
    assert "InteractingLayer" in layers.__all__
    fwd, bwd = engine.AutoIntEngine.autoint_flops(65536, 26, 16, 16)
    assert fwd == 65536 * (8 * 26 * 16 * 16 + 4 * 26 * 26 * 16) and bwd == 3 * fwd


def test_header_declares_and_library_exports_the_kernels(hip_lib):
    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    for name in ("rm_autoint_supported", "rm_autoint_stats_floats", "rm_autoint_layer_fwd", "rm_autoint_layer_bwd",
                 "rm_autoint_layer_bwd_workspace", "rm_autoint_head_fwd", "rm_autoint_head_bwd",
                 "rm_autoint_head_bwd_workspace"):
        assert name + "(" in text and hasattr(hip_lib, name), name
    # the supported set, asked without a GPU
    for F, Din, H, dk in ((26, 16, 2, 8), (1, 8, 1, 8), (40, 64, 8, 8), (40, 64, 1, 64), (5, 8, 2, 4)):
        assert hip_lib.rm_autoint_supported(F, Din, H, dk) == 1
        assert hip_lib.rm_autoint_layer_bwd_workspace(64, F, Din, H, dk) > 0
    for F, Din, H, dk in ((0, 16, 2, 8), (41, 16, 2, 8), (26, 12, 2, 8), (26, 16, 3, 8), (26, 16, 2, 64),
                          (26, 16, 2, 2), (26, 16, 3, 4), (26, 16, 1, 4)):
        assert hip_lib.rm_autoint_supported(F, Din, H, dk) == 0
        assert hip_lib.rm_autoint_layer_bwd_workspace(64, F, Din, H, dk) == 0
    assert hip_lib.rm_autoint_stats_floats(10, 26, 2) == 10 * 26 * 2 * 2
    assert hip_lib.rm_autoint_head_bwd_workspace(64, 416) > 0


def test_ops_reject_host_tensors_before_any_launch(hip_lib):
    from recman_amd import ops

    z = torch.zeros
    with pytest.raises(ValueError, match="GPU"):
        ops.autoint_layer_fwd(z(2, 3, 8), z(8, 8), z(8, 8), z(8, 8), None, 2, 1.0, z(2, 3, 8))
    with pytest.raises(ValueError, match="GPU"):
        ops.autoint_layer_bwd(z(2, 3, 8), z(8, 8), z(8, 8), z(8, 8), None, z(2, 3, 8), z(2, 2, 3, 2), z(2, 3, 8), 2, 1.0,
                              z(2, 3, 8), z(8, 8), z(8, 8), z(8, 8), None, z(1 << 16))
    with pytest.raises(ValueError, match="GPU"):
        ops.autoint_head_fwd(z(2, 3, 8), z(24), z(1), z(2))
    with pytest.raises(ValueError, match="GPU"):
        ops.autoint_head_bwd(z(2, 3, 8), z(24), z(2), z(2, 3, 8), z(24), z(1), z(1 << 16))
    assert ops.autoint_supported(26, 16, 2, 8) and not ops.autoint_supported(26, 16, 3, 8)
    assert ops.autoint_stats_floats(4, 26, 2) == 4 * 26 * 2 * 2
