"""CPU: the float64 restatement of MMoE (tests/mmoe_ref.py) is pinned without a GPU - the mixture's closed-form backward
against autograd and central finite differences, the loss head against oracle.th_layers.create_loss and its rules for
unobserved labels, the whole model's gradients against finite differences, the kink guard of every case the GPU tests
use - and the public surface that needs no GPU."""
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import th_layers as TL
from tests import mmoe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ------------------------------------------------------------------------------------------------- the mixture
@pytest.mark.parametrize("shape", [(5, 3, 2, 8), (4, 1, 1, 4), (3, 4, 3, 12)])
def test_mixture_backward_is_autograd_and_finite_differences(shape):
    B, E, T, H = shape
    c = R.mix_case(*shape, seed=7)
    Z, A = c["Z"].clone().requires_grad_(True), c["A"].clone().requires_grad_(True)
    M, P = R.mix_fwd(Z, A, E, T)
    assert torch.allclose(M.detach(), R.mix_loops(c["Z"], c["A"], E, T), rtol=0, atol=1e-12)
    assert torch.allclose(P.sum(dim=2), torch.ones(B, T, dtype=F64), rtol=0, atol=1e-12)
    (M * c["dM"]).sum().backward()
    assert R.grad_measure(c["dZ"], Z.grad) <= 1e-12 and R.grad_measure(c["dA"], A.grad) <= 1e-10
    if E == 1:
        assert float(c["dA"].abs().max()) == 0.0 and bool((P == 1).all())
    # central finite differences in float64
    f = lambda z, a: float((R.mix_fwd(z, a, E, T)[0] * c["dM"]).sum())  # noqa: E731
    h = 1e-6
    for name, X, want in (("Z", c["Z"], c["dZ"]), ("A", c["A"], c["dA"])):
        fd = torch.zeros_like(X)
        for i in range(X.numel()):
            d = torch.zeros(X.numel(), dtype=F64)
            d[i] = h
            d = d.reshape(X.shape)
            args_p = (X + d, c["A"]) if name == "Z" else (c["Z"], X + d)
            args_m = (X - d, c["A"]) if name == "Z" else (c["Z"], X - d)
            fd.view(-1)[i] = (f(*args_p) - f(*args_m)) / (2 * h)
        assert float((fd - want).abs().max()) <= 1e-7 * max(1.0, float(want.abs().max())), name


def test_mixture_extremes():
    # equal logits: p = 1 / E; logits x 60: one-hot, finite only because the maximum is subtracted
    Z = torch.randn(3, 4 * 8, dtype=F64)
    M, P = R.mix_fwd(Z, torch.full((3, 2 * 4), 5.0, dtype=F64), 4, 2)
    assert bool((P == 0.25).all())
    assert torch.allclose(M[:, :8], Z.reshape(3, 4, 8).mean(dim=1), rtol=0, atol=1e-15)
    c = R.mix_case(33, 4, 2, 8, logit_scale=60.0)
    assert bool(torch.isfinite(c["M"]).all()) and float(c["P"].max(dim=2).values.median()) > 0.999
    assert float(c["A"].abs().max()) > 100  # exp() of these overflows float32


# ----------------------------------------------------------------------------------------------- the loss head
def test_loss_head_with_one_task_is_create_loss():
    g = torch.Generator().manual_seed(3)
    logit = torch.randn(1, 41, generator=g, dtype=F64) * 2
    for kind in ("classification", "regression"):
        y = (torch.rand(41, generator=g) < 0.4).double() if kind == "classification" else torch.randn(41, generator=g,
                                                                                                     dtype=F64)
        loss, loss_t, n_t, pred = R.loss_head(logit, y.reshape(-1, 1), [kind])
        want = TL.create_loss(y, TL.prediction(logit[0], kind), kind)
        assert abs(float(loss) - float(want)) <= 1e-14 and abs(float(loss_t[0]) - float(want)) <= 1e-14
        assert int(n_t[0]) == 41 and torch.equal(pred[0], TL.prediction(logit[0], kind))


def test_loss_head_unobserved_labels_and_weights():
    c = R.loss_case(8, 77)
    T, B, Y = 8, 77, c["Y"]
    seen = ~torch.isnan(Y)
    assert 0.15 < float(seen[:, 1].double().mean()) < 0.5 and not bool(seen[:, 7].any()) and bool(seen[:, 0].all())
    assert c["types"][:3] == ["classification", "regression", "classification"] and c["weights"][1] == 0.75
    # NaN rows: zero gradient, and they do not enter the mean
    assert float(c["dlogit"].t()[~seen].abs().max()) == 0.0
    assert float(c["dlogit"][1][seen[:, 1]].abs().min()) > 0
    rows = seen[:, 1]
    alone = R.loss_head(c["logit"][1:2, rows], Y[rows, 1:2], ["regression"])[0]
    assert abs(float(c["loss_t"][1]) - float(alone)) <= 1e-14 and int(c["n_t"][1]) == int(rows.sum())
    # an all-NaN task: loss 0, zero gradient; pred is still there
    assert float(c["loss_t"][7]) == 0.0 and int(c["n_t"][7]) == 0 and float(c["dlogit"][7].abs().max()) == 0.0
    assert bool(torch.isfinite(c["pred"]).all())
    # weights scale loss and gradient; grad_scale the gradient
    assert abs(float(c["loss"]) - sum(w * float(l) for w, l in zip(c["weights"], c["loss_t"]))) <= 1e-13
    one = R.loss_head_grad(c["logit"], Y, c["types"], [1.0] * T, 1.0)
    for t in range(T):
        assert torch.allclose(c["dlogit"][t], one[4][t] * c["weights"][t] * 0.5, rtol=1e-13, atol=0)
    # the gradient of an observed classification label is (p - y) / n but for the epsilon inside the logs (1e-7 beside
    # p and 1 - p, both above 0.01 here)
    n0 = int(c["n_t"][0])
    p0 = c["pred"][0]
    inside = (p0 > 0.01) & (p0 < 0.99)
    want = (p0 - Y[:, 0]) / n0 * c["weights"][0] * 0.5
    assert float((c["dlogit"][0] - want)[inside].abs().max()) <= 2e-5 * c["weights"][0] * 0.5 / n0


# ---------------------------------------------------------------------------------------------------- the model
def test_model_gradients_against_finite_differences():
    k = R.make_case(("classification", "regression"), 2, (8, 4), (4,), 9, 2, 4, 1, 0.3, 0)
    p, spec, idx, dense, Y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "Y", "hp"))
    assert k["min_abs_pre"] >= 1e-4  # (far enough from every kink for a step of 1e-6)
    loss, logit, pred, grads = R.fwd_bwd(p, spec, idx, dense, Y, hp)
    assert logit.shape == (2, 9) and set(grads) == set(p)
    f = lambda q: float(R.model_loss(q, spec, idx, dense, Y, hp)[0])  # noqa: E731
    h = 1e-6
    gen = torch.Generator().manual_seed(1)
    for n, v in p.items():
        if n in ("linear_w", "linear_w0"):
            assert float(grads[n].abs().max()) == 0.0  # no linear term
            continue
        for i in torch.randperm(v.numel(), generator=gen)[:6].tolist():
            d = torch.zeros(v.numel(), dtype=F64)
            d[i] = h
            d = d.reshape(v.shape)
            fd = (f(dict(p, **{n: v + d})) - f(dict(p, **{n: v - d}))) / (2 * h)
            assert abs(fd - float(grads[n].reshape(-1)[i])) <= 1e-7 * max(1.0, abs(fd)), (n, i)
    # d_rows is the embedding gradient of the data loss, occurrence by occurrence
    dr = R.d_rows(p, spec, idx, dense, Y, hp)
    hp0 = dict(hp, embedding_l2_reg=0.0)
    g0 = R.fwd_bwd(p, spec, idx, dense, Y, hp0)[3]
    for f_, name in enumerate(spec.sparse_names):
        acc = torch.zeros_like(p[f"{name}_feat_embed"]).index_add_(0, idx[:, f_], dr[:, f_])
        assert torch.allclose(acc, g0[f"{name}_feat_embed"], rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES) + ["seq"])
def test_every_gpu_case_keeps_its_distance_from_the_kinks(name):
    if name == "seq":
        k = R.make_seq_case()
        assert k["hp"]["seq_pooling"] == "din" and k["spec"].seq_query == {"hist": "item"}
    else:
        types, NE, units, towers, B, F, D, Dn, nan_share, attempt = R.MODEL_CASES[name]
        k = R.make_case(*R.MODEL_CASES[name])
        # the committed attempt is the FIRST stream that keeps the distance
        for a in range(attempt):
            assert R.make_case(types, NE, units, towers, B, F, D, Dn, nan_share, a)["min_abs_pre"] < R.KINK
        assert k["hp"]["deep_l2_reg"] == 1e-4 and k["hp"]["num_experts"] == NE and k["idx"].shape == (B, F)
        assert bool(torch.isnan(k["Y"]).any()) == bool(nan_share) and not bool(torch.isnan(k["Y"][:, 0]).any())
    p, spec, idx, dense, hp, mv = (k[n] for n in ("p", "spec", "idx", "dense", "hp", "mv"))
    pres = []
    logit, P = R.mmoe_logits(p, spec, idx, dense, hp, mv, pres=pres)
    n_pre = len(hp["expert_hidden_units"]) + len(hp["task_names"]) * len(hp["tower_hidden_units"])
    assert len(pres) == n_pre and min(float(t.abs().min()) for t in pres) == k["min_abs_pre"] >= R.KINK
    assert 0.01 < float(logit.abs().max()) < 20
    if hp["num_experts"] > 1:  # the gates are neither uniform nor one-hot
        assert 0.3 < float(P.max(dim=2).values.mean()) < 0.98
    # the float32 run of the same code stays inside the model tests' bounds (tests/test_gpu_parity.py)
    want = R.fwd_bwd(p, spec, idx, dense, k["Y"], hp, mv)
    got = R.fwd_bwd(R.to_f32(p), spec, idx, dense.float(), k["Y"], hp,
                    None if mv is None else {n: tuple(t for t in e) for n, e in mv.items()})
    assert float((got[1].double() - want[1]).abs().max()) <= 1e-5
    for n in want[3]:
        if not n.startswith("hist_"):
            assert R.grad_measure(got[3][n], want[3][n]) <= R.TOL_GRAD, n


# ---------------------------------------------------------------------------------------------------- the surface
def test_public_surface():
    import recman_amd.th as th
    from recman_amd import _lib, engine as eng, ops

    assert th.MMoE.model == "mmoe" and "MMoE" in th.__all__ and eng.ENGINES["mmoe"] is eng.MMoEEngine
    assert eng.MMoEEngine.use_bias_tables is False and eng.MMoEEngine.shardable is False
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.MMoEEngine.require_shardable()
    sig = inspect.signature(th.MMoE.__init__).parameters
    want = dict(task_names=("ctr", "cvr"), task_types=("classification", "classification"), task_weights=None,
                num_experts=8, expert_hidden_units=(256, 128), tower_hidden_units=(64,), embedding_size=8,
                deep_activation="relu", deep_l2_reg=0.0, embedding_l2_reg=0.00001)
    assert list(sig)[:12] == ["self", "feat_dict"] + list(want) and all(sig[n].default == v for n, v in want.items())
    pnn = inspect.signature(th.PNN.__init__).parameters
    for n in ("epoch", "batch_size", "learning_rate", "optimizer", "random_seed", "eval_metric", "strict_reference",
              "device"):
        assert sig[n].default == pnn[n].default, n
    # the binding table and the header
    assert len(_lib.SIGNATURES["rm_mmoe_mix_fwd"]) == 13 and len(_lib.SIGNATURES["rm_mmoe_mix_bwd"]) == 15
    assert len(_lib.SIGNATURES["rm_multitask_loss"]) == 14
    assert len(_lib.SIGNATURES_I64["rm_multitask_loss_workspace"]) == 2
    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    for s in ("int rm_mmoe_mix_supported(int E, int T, int H);", "int rm_mmoe_mix_fwd(const float *Z, int64_t ldz,",
              "int rm_mmoe_mix_bwd(const float *Z, int64_t ldz,", "int rm_mmoe_mix_tile(int E, int T, int H,",
              "int64_t rm_multitask_loss_workspace(int64_t B, int T);", "int rm_multitask_loss(const float *logit,",
              "NaN in Y means unobserved", "p reaches HBM only when P is given"):
        assert s in text, s


def test_mix_supported_at_the_edges_of_its_limits(hip_lib):
    from recman_amd import ops

    ok = [(1, 1, 4), (16, 8, 512), (16, 1, 4), (1, 8, 512), (8, 2, 128), (3, 2, 36)]
    bad = [(0, 1, 4), (17, 1, 4), (1, 0, 4), (1, 9, 4), (1, 1, 0), (1, 1, 2), (1, 1, 6), (1, 1, 516), (8, 2, 130)]
    assert all(ops.mmoe_mix_supported(*s) for s in ok) and not any(ops.mmoe_mix_supported(*s) for s in bad)
    assert ops.MMOE_H_MIN == 4 and ops.MMOE_H_MAX == 512
    # the tile: 256 threads over lane groups of the power of two >= H / 4 (at most 64)
    assert [ops.mmoe_mix_tile(2, 2, H) for H in (4, 8, 16, 36, 128, 256, 512)] == [256, 128, 64, 16, 8, 4, 4]
    assert ops.mmoe_mix_tile(8, 2, 128, "cap") == 1024 and ops.mmoe_mix_tile(2, 2, 8, backward=True) == 128
    assert ops.mmoe_mix_tile(16, 8, 4) == 64 and ops.mmoe_mix_tile(16, 8, 4, backward=True) == 64  # LDS-bound blocks
    with pytest.raises(ValueError, match="unsupported"):
        ops.mmoe_mix_tile(17, 2, 8)
    assert ops.multitask_loss_workspace(1, 1) > 0
    with pytest.raises(ValueError, match="1 <= T <= 8"):
        ops.multitask_loss_workspace(5, 9)


def test_constructor_errors_need_no_gpu():
    import recman_amd.th as th

    with pytest.raises(ValueError, match="differ in length"):
        th.MMoE(None, task_names=("a", "b", "c"))
    with pytest.raises(ValueError, match="differ in length"):
        th.MMoE(None, task_types=("classification",))
    with pytest.raises(ValueError, match="differ in length"):
        th.MMoE(None, task_weights=(1.0,))
    with pytest.raises(ValueError, match="neither 'classification' nor 'regression'"):
        th.MMoE(None, task_types=("classification", "ranking"))
    for n in (0, 17):
        with pytest.raises(ValueError, match="num_experts"):
            th.MMoE(None, num_experts=n)
    with pytest.raises(ValueError, match="9 tasks"):
        th.MMoE(None, task_names=tuple("abcdefghi"), task_types=("classification",) * 9)
    for units in ((256, 126), (), (6, 8), (1024,)):
        with pytest.raises(ValueError, match="expert_hidden_units"):
            th.MMoE(None, expert_hidden_units=units)
    with pytest.raises(ValueError, match="tower_hidden_units"):
        th.MMoE(None, tower_hidden_units=())
    with pytest.raises(ValueError, match="strict_reference"):
        th.MMoE(None, strict_reference=True)
    with pytest.raises(ValueError, match="unsupported activation"):
        th.MMoE(None, deep_activation="tanh")
    fd = type("NoFeatures", (), {"embedding_feats": []})()  # (the constructor asks it for the grouped metrics' columns)
    m = th.MMoE(fd, task_names=("click", "like", "dwell"), task_types=("classification", "classification",
                                                                         "regression"))
    assert m.metric_names == ["click/roc_auc_score", "click/log_loss", "like/roc_auc_score", "like/log_loss",
                              "dwell/roc_auc_score", "dwell/log_loss"]
    assert [str(x) for x in m.metrics] == m.metric_names and m.hparams["num_experts"] == 8
    # the label cast: [N, T] float32, NaN kept, a classification label outside {0, 1, NaN} refused
    Y = m._labels(np.array([[1, 0, 2.5], [0, np.nan, -1.0]]))
    assert Y.dtype == np.float32 and Y.shape == (2, 3) and np.isnan(Y[1, 1])
    with pytest.raises(ValueError, match="'like' is a classification task"):
        m._labels(np.array([[1, 2, 0.0]]))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        m._labels(np.array([1, 0, 1]))
    # a task metric scores its own column on the observed rows only
    from sklearn.metrics import roc_auc_score

    y = np.array([[1, np.nan], [0, 1], [1, 0], [0, np.nan], [1, 1]])
    pr = np.array([[0.9, 0.1], [0.2, 0.8], [0.4, 0.3], [0.6, 0.9], [0.7, 0.6]])
    tm = th.MMoE(fd).metrics
    assert tm[2](y, pr) == roc_auc_score([1, 0, 1], [0.8, 0.3, 0.6])
    assert tm[0](y, pr) == roc_auc_score(y[:, 0], pr[:, 0])
