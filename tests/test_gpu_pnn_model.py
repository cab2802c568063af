"""GPU: PNNEngine, th.PNN and th.layers.ProductLayer against the float64 restatement (tests/pnn_ref.py), with the rules
of tests/test_gpu_parity.py: logit and inference logit 1e-5 absolute, loss _close, every gradient _close_grad at 2e-5."""
import numpy as np
import pytest
import torch
from sklearn.base import clone
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import pnn_ref as R
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(k, **hp_kw):
    from recman_amd import engine as eng

    spec, hp = k["spec"], dict(k["hp"], **hp_kw)
    e = eng.PNNEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names), hp["embedding_size"], hp)
    e.load_params(R.to_f32(k["p"]))
    return e


def _dev(k):
    return k["idx"].cuda(), k["dense"].to(F32).cuda(), k["y"].cuda()


def _compare(e, idx_d, loss, ref, what=""):
    loss_o, logit_o, pred_o, grads_o = ref
    torch.cuda.synchronize()
    print(f"{what}logit err {float((e.logit.cpu().double() - logit_o).abs().max()):.2e}")
    _close(e.logit, logit_o, rtol=0, atol=1e-5, what=what + "logit")
    _close(loss, loss_o.reshape(1), what=what + "loss")
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o), set(grads) ^ set(grads_o)
    for n in grads_o:
        print(f"{what}{n} measure {R.grad_measure(grads[n], grads_o[n]):.2e}")
        _close_grad(grads[n], grads_o[n], what=f"{what}grad {n}")
    return grads


_REFS = {}


def _ref(name):
    if name not in _REFS:
        k = R.make_case(*R.MODEL_CASES[name])
        _REFS[name] = (k, R.fwd_bwd(*(k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))))
    return _REFS[name]


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_pnn_fwd_bwd_matches_float64(hip_lib, name):
    pr, kt, use_linear, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    k, ref = _ref(name)
    p, spec, idx, hp = (k[n] for n in ("p", "spec", "idx", "hp"))
    assert hp["interaction_l2_reg"] == 1e-4 and hp["deep_l2_reg"] == 1e-4 and k["min_abs_pre"] >= R.KINK
    e = _engine(k)
    assert e.use_linear == use_linear and e.ktype == kt and e.products == pr and e.W == R.width(F, D, pr)
    idx_d, dense_d, y_d = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    what = f"{name}: "
    _compare(e, idx_d, loss, ref, what=what)
    # the row gradients themselves: d_rows is dLoss/dE of every example, scattered into the tables by the step
    leaves = {n: v.detach().clone().requires_grad_(n.endswith("_feat_embed")) for n, v in p.items()}
    E64, _ = TL.feat_embedding_layer(leaves, spec, idx, use_bias=False)
    E64.retain_grad()
    X = R.product_layer(E64, leaves.get("product_kernel"), pr, kt)
    logit = TL.dnn(leaves, TL.dnn_input(X, k["dense"]), len(hidden), "relu")
    if use_linear:
        logit = logit + TL.linear_layer(leaves, spec, idx, k["dense"])
    TL.create_loss(k["y"], TL.prediction(logit)).backward()
    print(f"{what}d_rows measure {R.grad_measure(e.d_rows, E64.grad):.2e}")
    _close_grad(e.d_rows, E64.grad, what=what + "d_rows")
    assert bool((e.X[:, e.W:] == 0).all())  # the pad columns stay +0.0
    train_logit = e.logit.clone()
    logit_i, _ = e.forward(idx_d, dense_d, training=False)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")
    assert torch.equal(logit_i, train_logit)  # no dropout: inference logits are the training logits' bits
    # a second fwd_bwd gives the same bits in every gradient the step computes
    names = [n for n in e.grads if n.startswith(("product_kernel", "dnn_"))]
    first, first_rows = {n: e.grads[n].clone() for n in names}, e.d_rows.clone()
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    assert torch.equal(e.d_rows, first_rows), f"{what}d_rows differs between two runs"
    for n in names:
        assert torch.equal(e.grads[n], first[n]), f"{what}{n} differs between two runs"
    sd = e.state_dict()
    assert set(sd) == set(p) and not any(n.endswith("_feat_bias") for n in sd)
    assert ("product_kernel" in sd) == bool(pr & R.OUTER)


def test_engine_rejects_what_it_cannot_run_and_declares_its_variables(hip_lib):
    from recman_amd import engine as eng

    spec3 = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x"])
    with pytest.raises(ValueError, match="neither use_inner nor use_outer"):
        eng.PNNEngine(spec3, 8, dict(use_inner=False, use_outer=False))
    with pytest.raises(ValueError, match="'mat', 'vec', 'num'"):
        eng.PNNEngine(spec3, 8, dict(use_outer=True, kernel_type="ten"))
    with pytest.raises(ValueError, match=r"not supported.*2\.\.40 embedding features, embedding_size 8/16/32"):
        eng.PNNEngine(spec3, 64, {})
    with pytest.raises(ValueError, match="not supported"):
        eng.PNNEngine(eng.FeatureSpec([f"f{i}" for i in range(41)], [3] * 41), 8, {})
    with pytest.raises(ValueError, match="not supported"):
        eng.PNNEngine(eng.FeatureSpec(["a"], [4]), 8, {})
    with pytest.raises(ValueError, match="deep_hidden_units must name at least one layer"):
        eng.PNNEngine(spec3, 8, dict(deep_hidden_units=()))
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.PNNEngine.require_shardable()
    assert eng.ENGINES["pnn"] is eng.PNNEngine and eng.PNNEngine.use_bias_tables is False
    spec = eng.FeatureSpec([f"f{i}" for i in range(7)], [5] * 7, ["x", "y"])
    e = eng.PNNEngine(spec, 16, dict(deep_hidden_units=(8,)))  # the defaults: inner products only
    assert e.products == 1 and e.ktype == "mat" and e.use_linear is False and "product_kernel" not in e.params
    assert (e.W, e.ldx) == (7 * 16 + 21, 136)
    for kt in R.KERNELS:
        e = eng.PNNEngine(spec, 16, dict(use_outer=True, kernel_type=kt, deep_hidden_units=(8,)))
        assert e.products == 3 and e.W == 7 * 16 + 42
        eng.init_reference(e, 5)
        v = e.params["product_kernel"]
        assert tuple(v.shape) == R.weight_shape(7, 16, kt)
        assert e.decl["product_kernel"] == (("glorot", 16, 16), "interaction_l2_reg")
        assert e.l2_groups["interaction_l2_reg"] == ["product_kernel"]
        std = (2.0 / 32) ** 0.5
        assert 0 < float(v.abs().max()) <= 2 * std + 1e-6
        assert not any(n.endswith("_feat_bias") for n in e.params)


@pytest.mark.parametrize("name", ["inner_only", "inner_mat_criteo_like"])
def test_roofline_probes_list_the_new_kernels(hip_lib, name):
    pr, kt, use_linear, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    k, _ = _ref(name)
    e = _engine(k)
    idx_d, dense_d, y_d = _dev(k)
    probes = e.roofline_probes(idx_d, dense_d, y_d)
    P = R.pairs(F)
    if pr & R.OUTER:
        assert [p["symbol"] for p in probes[:2]] == ["pnn_de_mat_kernel", "pnn_fwd_kernel"]
        assert all(p["bound"] == "mfma" for p in probes[:2])
        assert probes[1]["work"] == 2.0 * B * P * D * D and probes[0]["work"] == 3 * probes[1]["work"]
    else:
        assert [p["symbol"] for p in probes[:2]] == ["pnn_de_valu_kernel", "pnn_fwd_kernel"]
        assert all(p["bound"] == "hbm" for p in probes[:2])
        assert probes[1]["work"] == 4.0 * (B * F * D + B * e.ldx)
    x0, d0 = e.X.clone(), e.d_rows.clone()
    for p in probes:
        p["fn"]()
    torch.cuda.synchronize()
    # the probes recompute on the step's own E and dX: X comes back with the same bits, d_rows is a buffer of theirs
    assert torch.equal(e.X, x0) and torch.equal(e.d_rows, d0)


# --------------------------------------------------------------------------------------------------- ProductLayer
def test_product_layer_under_autograd_matches_the_ops(hip_lib):
    from recman_amd import ops
    from recman_amd.th import layers as L

    for shape, (pr, kt) in (((37, 5, 8), (3, "mat")), ((33, 3, 8), (2, "vec")), ((65, 10, 32), (2, "num")),
                            ((37, 5, 8), (1, "mat"))):
        B, F, D = shape
        case = R.kernel_case(*shape, pr, kt)
        W = case["W"]
        variables = {"product_kernel": case["K"].to(F32).cuda().requires_grad_(True)} if pr & R.OUTER else {}
        layer = L.ProductLayer(variables, bool(pr & R.INNER), bool(pr & R.OUTER), kt, l2_reg=1e-3)
        E = case["E"].to(F32).cuda().requires_grad_(True)
        out = layer(E)
        assert out.shape == (B, W) and layer.display_name == "ProductLayer"
        dX = case["dX"].to(F32).cuda()
        (out * dX).sum().backward()
        # the same entry points, called directly: the same bits
        K = variables.get("product_kernel")
        Kd = K.detach() if K is not None else None
        X, d_rows = torch.empty(B, W, device="cuda"), torch.empty(B, F, D, device="cuda")
        dK = torch.empty_like(Kd) if Kd is not None else None
        ws = torch.empty(max(4, ops.pnn_bwd_workspace(B, F, D, pr, kt)), device="cuda") if Kd is not None else None
        ops.pnn_fwd(E.detach(), Kd, pr, kt, X)
        ops.pnn_bwd(E.detach(), Kd, pr, kt, dX, d_rows, dK, ws)
        assert torch.equal(out.detach(), X) and torch.equal(E.grad, d_rows)
        assert R.x_error(out, case["X"]) <= R.TOL_X and R.grad_measure(E.grad, case["d_rows"]) <= R.TOL_GRAD
        if K is not None:
            assert torch.equal(K.grad, dK) and R.grad_measure(K.grad, case["dK"]) <= R.TOL_GRAD
            want_l2 = float(R.interaction_l2({"product_kernel": case["K"]}, 1e-3))
            assert abs(float(layer.l2().detach()) - want_l2) < 1e-5 * max(1.0, want_l2)
        else:
            assert layer.l2() == 0.0 and layer.weights == []
    # lazily made variable: name, shape, glorot with fan D / D
    for kt in R.KERNELS:
        fresh = {}
        E = torch.randn(6, 7, 8, device="cuda")
        out = L.ProductLayer(fresh, True, True, kt)(E)
        assert out.shape == (6, 56 + 42) and set(fresh) == {"product_kernel"}
        assert tuple(fresh["product_kernel"].shape) == R.weight_shape(7, 8, kt)
        assert 0 < float(fresh["product_kernel"].abs().max()) <= 2 * (2.0 / 16) ** 0.5 + 1e-6
        want = R.product_layer(E.cpu().double(), fresh["product_kernel"].detach().cpu().double(), 3, kt)
        assert R.x_error(out, want) <= R.TOL_X
    assert L.ProductLayer({}, True, False)(torch.randn(4, 3, 8, device="cuda")).shape == (4, 27)
    with pytest.raises(ValueError, match="unsupported"):
        L.ProductLayer({}, True, True, "mat")(torch.randn(4, 3, 12, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        L.ProductLayer({}, True, True, "mat")(torch.randn(4, 24, device="cuda"))


# ---------------------------------------------------------------------------------------------------------- th.PNN
def test_model_surface_on_the_ml100k_slice(hip_lib, tmp_path):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    yv = df["label"].values
    kw = dict(embedding_size=8, use_inner=True, use_outer=True, kernel_type="mat", deep_hidden_units=(32, 32),
              interaction_l2_reg=1e-5, epoch=2, batch_size=256, learning_rate=0.01)
    m = th.PNN(fd, **kw)
    e = m._build()
    assert e.model == "pnn" and e.ktype == "mat" and e.products == 3 and not e.use_linear
    assert set(m.hparams) >= {"embedding_size", "use_inner", "use_outer", "kernel_type", "deep_hidden_units",
                              "deep_dropout", "interaction_l2_reg", "use_linear", "learning_rate", "optimizer"}
    p0 = {n: v.cpu() for n, v in e.state_dict().items()}
    assert tuple(p0["product_kernel"].shape) == R.weight_shape(e.F, 8, "mat")
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, yv)
    idx, dense = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense)
    pred0 = m.predict(df)
    want0 = TL.prediction(R.pnn_logit(p0, spec, idx, dense, m.hparams, training=False)).numpy()
    assert pred0.shape == (len(df),) and np.abs(pred0 - want0.reshape(-1)).max() < 1e-6
    logit_e, pred_e = e.forward(idx.cuda(), dense.cuda(), training=False)
    assert np.abs(pred0 - pred_e.cpu().numpy()).max() < 1e-6  # predict is the engine's inference
    before = log_loss(yv, pred0.astype(np.float64))
    assert m.fit(df, yv, random_seed_for_mini_batch=False) is None  # two epochs
    pred1 = m.predict(df)
    after = log_loss(yv, pred1.astype(np.float64))
    print(f"PNN: training log loss {before:.4f} -> {after:.4f}")
    assert pred1.shape == (len(df),) and after < before
    assert not torch.equal(e.state_dict()["product_kernel"].cpu(), p0["product_kernel"])  # the kernels are trained
    res = m.evaluate(df, yv)
    assert len(res) == 2 and all(np.isfinite(r) for r in res)
    # save / restore round-trips the trained model
    path = str(tmp_path / "model")
    m.save(path)
    m2 = th.PNN(fd, **kw)
    m2.restore(path)
    assert np.array_equal(m2.predict(df), pred1)
    # clone() round-trips the constructor arguments
    c = clone(m)
    assert isinstance(c, th.PNN) and c is not m
    got = c.get_params()
    for n, v in kw.items():
        assert got[n] == v, n
    assert got["deep_dropout"] is None and got["use_linear"] is False


def test_constructor_errors_and_the_row_sharded_refusal(hip_lib):
    import recman_amd.th as th
    from recman_amd.th import FeatureDictionary, SparseFeat
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    with pytest.raises(ValueError, match="not supported"):
        th.PNN(fd, embedding_size=64)._build()
    m = th.PNN(fd, embedding_size=8)
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m._build()
    col = fd.embedding_feats[0].name
    fd1 = FeatureDictionary()
    fd1[col] = SparseFeat(name=col, feat_size=fd.embedding_feats[0].feat_size)
    fd1.initialize(df)
    with pytest.raises(ValueError, match="not supported"):
        th.PNN(fd1, embedding_size=8)._build()  # F = 1: no pair
    e = th.PNN(fd, use_inner=False, use_outer=True, kernel_type="vec", use_linear=True, deep_hidden_units=(16,))._build()
    assert e.products == 2 and e.ktype == "vec" and e.use_linear
    assert th.PNN(fd, deep_hidden_units=(8,), deep_dropout=(0.9, 1))._dropout_masks(5)["dnn"][0].shape[0] == 5
