"""GPU: FmFMEngine, th.FmFM / th.FwFM and th.layers.FieldPairInteraction against the float64 restatement
(tests/fmfm_ref.py), with the rules of tests/test_gpu_parity.py: logit and inference logit 1e-5 absolute, loss _close,
every gradient _close_grad at 2e-5."""
import numpy as np
import pytest
import torch
from sklearn.base import clone
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import fmfm_ref as R
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(k, **hp_kw):
    from recman_amd import engine as eng

    spec, hp = k["spec"], dict(k["hp"], **hp_kw)
    e = eng.FmFMEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names), hp["embedding_size"], hp)
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


@pytest.mark.parametrize("use_linear", [True, False])
@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_fmfm_fwd_bwd_matches_float64(hip_lib, name, use_linear):
    ftype, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    k = R.make_case(*R.MODEL_CASES[name], use_linear=use_linear)
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert hp["interaction_l2_reg"] == 1e-4 and k["min_abs_pre"] >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp)
    e = _engine(k)
    assert e.use_linear == use_linear and e.ftype == ftype and e.use_deep == bool(hidden) and not e.use_fm
    idx_d, dense_d, y_d = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    what = f"{name} linear={use_linear}: "
    _compare(e, idx_d, loss, ref, what=what)
    train_logit = e.logit.clone()
    logit_i, _ = e.forward(idx_d, dense_d, training=False)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")
    assert torch.equal(logit_i, train_logit)  # no dropout: inference logits are the training logits' bits
    # a second fwd_bwd gives the same bits in every gradient the step computes
    names = [n for n in e.grads if n.startswith(("field_pair_w", "dnn_"))]
    first, first_rows = {n: e.grads[n].clone() for n in names}, e.d_rows.clone()
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    assert torch.equal(e.d_rows, first_rows), f"{what}d_rows differs between two runs"
    for n in names:
        assert torch.equal(e.grads[n], first[n]), f"{what}{n} differs between two runs"
    sd = e.state_dict()
    assert set(sd) == set(p) and not any(n.endswith("_feat_bias") for n in sd)
    assert tuple(sd["field_pair_w"].shape) == R.weight_shape(F, D, ftype)


def test_fmfm_deep_dropout_with_given_masks(hip_lib):
    ftype, hidden, B, F, D, Dn = R.MODEL_CASES["vector_dnn"]
    k = R.make_case(*R.MODEL_CASES["vector_dnn"])
    p, spec, idx, dense, y = (k[n] for n in ("p", "spec", "idx", "dense", "y"))
    hp = dict(k["hp"], deep_dropout=(0.9, 0.8, 0.8))
    W = F * D + Dn
    g = torch.Generator().manual_seed(22)
    masks = [(torch.rand(B, d, generator=g) < kp).double() for d, kp in zip((W,) + hidden, hp["deep_dropout"])]
    assert all(bool((m == 0).any()) for m in masks)
    pres = R.fmfm_logit(p, spec, idx, dense, hp, masks={"dnn": masks}, return_pre=True)[1]
    assert len(pres) == 2 and min(float(t.abs().min()) for t in pres) >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, masks={"dnn": masks})
    e = _engine(k, deep_dropout=hp["deep_dropout"])
    idx_d, dense_d, y_d = _dev(k)
    md = {"dnn": [m.to(F32).cuda() for m in masks]}
    loss = e.fwd_bwd(idx_d, dense_d, y_d, masks=md)
    _compare(e, idx_d, loss, ref, what="dropout ")
    drawn = e.dropout_masks(B)
    assert [tuple(m.shape) for m in drawn["dnn"]] == [(B, W), (B, 16), (B, 16)]


def test_engine_rejects_what_it_cannot_run_and_declares_its_variables(hip_lib):
    from recman_amd import engine as eng

    spec3 = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x"])
    with pytest.raises(ValueError, match="'matrix', 'vector', 'scalar'"):
        eng.FmFMEngine(spec3, 8, dict(field_interaction="tensor"))
    with pytest.raises(ValueError, match=r"not supported.*2\.\.40 embedding features, embedding_size 8/16/32"):
        eng.FmFMEngine(spec3, 64, {})
    with pytest.raises(ValueError, match="not supported"):
        eng.FmFMEngine(eng.FeatureSpec([f"f{i}" for i in range(41)], [3] * 41), 8, {})
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.FmFMEngine.require_shardable()
    assert eng.ENGINES["fmfm"] is eng.FmFMEngine
    spec = eng.FeatureSpec([f"f{i}" for i in range(7)], [5] * 7, ["x", "y"])
    for ftype in R.TYPES:
        e = eng.FmFMEngine(spec, 16, dict(field_interaction=ftype))
        assert e.use_linear is True and e.ftype == ftype and e.mlp is None and not e.use_deep and not e.use_fm
        e.params["field_pair_w"].fill_(7.0)
        eng.init_reference(e, 5)
        v = e.params["field_pair_w"]
        assert tuple(v.shape) == R.weight_shape(7, 16, ftype)
        assert torch.equal(v.cpu(), R.init_weights(7, 16, ftype, F32))  # plain FM: identity matrices / ones
        assert e.decl["field_pair_w"] == ("pair_identity", "interaction_l2_reg")
        assert e.l2_groups["interaction_l2_reg"] == ["field_pair_w"]
        assert not any(n.endswith("_feat_bias") for n in e.params)
    assert eng.FmFMEngine(spec, 16, {}).ftype == "matrix"  # the default
    e = eng.FmFMEngine(spec, 16, dict(deep_hidden_units=(8,), use_linear=False))
    assert e.use_deep and e.mlp is not None and e.use_linear is False
    e.decl["field_pair_w"] = (("mystery", 1, 1), None)
    with pytest.raises(ValueError, match="unknown init rule"):
        eng.init_reference(e, 5)


@pytest.mark.parametrize("name", ["scalar_no_dnn", "matrix_criteo_like"])
def test_roofline_probes_list_the_new_kernels(hip_lib, name):
    ftype, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    k = R.make_case(*R.MODEL_CASES[name])
    e = _engine(k)
    idx_d, dense_d, y_d = _dev(k)
    probes = e.roofline_probes(idx_d, dense_d, y_d)
    P = R.pairs(F)
    if ftype == "matrix":
        assert [p["symbol"] for p in probes[:2]] == ["fmfm_de_kernel", "fmfm_fwd_kernel"]
        assert all(p["bound"] == "mfma" for p in probes[:2])
        assert probes[1]["work"] == 2.0 * B * P * D * D and probes[0]["work"] == 3 * probes[1]["work"]
    else:
        assert [p["symbol"] for p in probes[:2]] == ["fmfm_vs_de_kernel", "fmfm_vs_fwd_kernel"]
        assert all(p["bound"] == "hbm" for p in probes[:2])
        assert probes[1]["work"] == 4.0 * (B * F * D + B + P)
    l0, d0, g0 = e.pair_logit.clone(), e.d_rows.clone(), e.grads["field_pair_w"].clone()
    for p in probes:
        p["fn"]()
    torch.cuda.synchronize()
    # the probes recompute on the step's own E and dlogit, into buffers of their own
    assert torch.equal(e.pair_logit, l0) and torch.equal(e.d_rows, d0) and torch.equal(e.grads["field_pair_w"], g0)


# ---------------------------------------------------------------------------------------- FieldPairInteraction
def test_interaction_layer_under_autograd_matches_float64(hip_lib):
    from recman_amd.th import layers as L

    for shape, ftype in (((37, 5, 8), "matrix"), ((33, 3, 8), "vector"), ((65, 10, 32), "scalar")):
        B, F, D = shape
        case = R.kernel_case(*shape, ftype)
        variables = {"field_pair_w": case["W"].to(F32).cuda().requires_grad_(True)}
        layer = L.FieldPairInteraction(variables, ftype, l2_reg=1e-3)
        E = case["E"].to(F32).cuda().requires_grad_(True)
        out = layer(E)
        assert out.shape == (B,) and layer.display_name == "FieldPairInteraction"
        (out * case["g"].to(F32).cuda()).sum().backward()
        assert R.logit_error(out, case["logit"]) <= R.TOL_LOGIT
        assert R.grad_measure(E.grad, case["dE"]) <= R.TOL_GRAD
        assert R.grad_measure(variables["field_pair_w"].grad, case["dW"]) <= R.TOL_GRAD
        want_l2 = float(R.interaction_l2({"field_pair_w": case["W"]}, 1e-3))
        assert abs(float(layer.l2().detach()) - want_l2) < 1e-5 * max(1.0, want_l2)
    # lazily made variable: name, shape, plain FM
    for ftype in R.TYPES:
        fresh = {}
        E = torch.randn(6, 7, 8, device="cuda")
        out = L.FieldPairInteraction(fresh, ftype)(E)
        assert out.shape == (6,) and set(fresh) == {"field_pair_w"}
        assert tuple(fresh["field_pair_w"].shape) == R.weight_shape(7, 8, ftype)
        assert R.logit_error(out, R.fm_second_order(E.cpu().double())) <= R.TOL_LOGIT
    assert "FieldPairInteraction" in L.__all__
    with pytest.raises(ValueError, match="'matrix', 'vector', 'scalar'"):
        L.FieldPairInteraction({}, "tensor")
    with pytest.raises(ValueError, match="unsupported"):
        L.FieldPairInteraction({}, "matrix")(torch.randn(4, 3, 12, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        L.FieldPairInteraction({}, "matrix")(torch.randn(4, 24, device="cuda"))


# ------------------------------------------------------------------------------------------ th.FmFM / th.FwFM
@pytest.mark.parametrize("cls_name,ftype", [("FmFM", "matrix"), ("FwFM", "scalar")])
def test_model_surface_on_the_ml100k_slice(hip_lib, tmp_path, cls_name, ftype):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    cls = getattr(th, cls_name)
    df = ml_frame()
    fd = ml_features(df)
    yv = df["label"].values
    kw = dict(embedding_size=8, interaction_l2_reg=1e-5, epoch=2, batch_size=256, learning_rate=0.01)
    m = cls(fd, **kw)
    e = m._build()
    assert e.model == "fmfm" and e.ftype == ftype and e.use_linear and not e.use_deep
    assert set(m.hparams) >= {"embedding_size", "field_interaction", "deep_hidden_units", "deep_dropout",
                              "interaction_l2_reg", "use_linear", "learning_rate", "optimizer"}
    p0 = {n: v.cpu() for n, v in e.state_dict().items()}
    assert torch.equal(p0["field_pair_w"], R.init_weights(e.F, 8, ftype, F32))
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, yv)
    idx, dense = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense)
    pred0 = m.predict(df)
    want0 = TL.prediction(R.fmfm_logit(p0, spec, idx, dense, m.hparams, training=False)).numpy()
    assert pred0.shape == (len(df),) and np.abs(pred0 - want0.reshape(-1)).max() < 1e-6
    logit_e, pred_e = e.forward(idx.cuda(), dense.cuda(), training=False)
    assert np.abs(pred0 - pred_e.cpu().numpy()).max() < 1e-6  # predict is the engine's inference
    before = log_loss(yv, pred0.astype(np.float64))
    assert m.fit(df, yv, random_seed_for_mini_batch=False) is None  # two epochs
    pred1 = m.predict(df)
    after = log_loss(yv, pred1.astype(np.float64))
    print(f"{cls_name}: training log loss {before:.4f} -> {after:.4f}")
    assert pred1.shape == (len(df),) and after < before
    assert not torch.equal(e.state_dict()["field_pair_w"].cpu(), p0["field_pair_w"])  # the pair weights are trained
    res = m.evaluate(df, yv)
    assert len(res) == 2 and all(np.isfinite(r) for r in res)
    # save / restore round-trips the trained model
    path = str(tmp_path / "model")
    m.save(path)
    m2 = cls(fd, **kw)
    m2.restore(path)
    assert np.array_equal(m2.predict(df), pred1)
    # clone() round-trips the constructor arguments
    c = clone(m)
    assert isinstance(c, cls) and c is not m
    got = c.get_params()
    for n, v in kw.items():
        assert got[n] == v, n
    assert got["field_interaction"] == ftype and got["deep_hidden_units"] == () and got["deep_dropout"] is None
    assert cls_name in th.__all__


def test_constructor_errors_and_the_row_sharded_refusal(hip_lib):
    import recman_amd.th as th
    from recman_amd.th import FeatureDictionary, SparseFeat
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    for cls in (th.FmFM, th.FwFM):
        with pytest.raises(ValueError, match="'matrix', 'vector', 'scalar'"):
            cls(fd, field_interaction="tensor")
        with pytest.raises(ValueError, match="not supported"):
            cls(fd, embedding_size=64)._build()
        with pytest.raises(ValueError, match="deep_dropout"):
            cls(fd, deep_dropout=(0.9, 1))
        m = cls(fd, embedding_size=8)
        m.hparams["table_sharding"] = "row"
        with pytest.raises(NotImplementedError, match="one GPU"):
            m._build()
    col = fd.embedding_feats[0].name
    fd1 = FeatureDictionary()
    fd1[col] = SparseFeat(name=col, feat_size=fd.embedding_feats[0].feat_size)
    fd1.initialize(df)
    with pytest.raises(ValueError, match="not supported"):
        th.FmFM(fd1, embedding_size=8)._build()  # F = 1: no pair
    assert th.FmFM(fd, field_interaction="vector", deep_hidden_units=(16, 16))._build().use_deep
    assert th.FwFM(fd, deep_hidden_units=(8,), deep_dropout=(0.9, 1))._dropout_masks(5)["dnn"][0].shape[0] == 5
