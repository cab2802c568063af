"""GPU: the DLRM engine, th.DLRM and th.layers.DotInteraction against the float64 restatement (tests/dlrm_ref.py), in
the manner and with the tolerances of tests/test_gpu_parity.py and tests/test_gpu_autoint_model.py: logits 1e-5,
predictions 1e-6, every gradient with the gradient measure (_close_grad).  The label-driven upstream gradient of the
model-level cases cannot be zeroed, so their seeds keep every unit of both towers away from its kink (asserted on the
CPU in tests/test_dlrm_host.py, and here for the variants this file builds)."""
import numpy as np
import pytest
import torch
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import dlrm_ref as R
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _f32(p):
    return {n: v.to(F32) for n, v in p.items()}


def _engine(spec, hp, p, task="classification", **spec_kw):
    from recman_amd import engine as eng

    kw = spec_kw or dict(multi_names=spec.multi_names, value_names=spec.value_names)
    e = eng.DLRMEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names, **kw),
                       hp["embedding_size"], hp, task=task)
    e.load_params(_f32(p))
    return e


def _compare(e, idx_d, loss, ref, what=""):
    loss_o, logit_o, pred_o, grads_o = ref
    torch.cuda.synchronize()
    print(f"{what}logit err {float((e.logit.cpu().double() - logit_o).abs().max()):.2e}")
    _close(e.logit, logit_o, rtol=0, atol=1e-5, what=what + "logit")
    _close(e.pred, pred_o, rtol=0, atol=1e-6, what=what + "pred")
    _close(loss, loss_o.reshape(1), what=what + "loss")
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o), set(grads) ^ set(grads_o)
    for k in grads_o:
        print(f"{what}{k} measure {R.grad_measure(grads[k], grads_o[k]):.2e}")
        _close_grad(grads[k], grads_o[k], what=f"{what}grad {k}")


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_dlrm_fwd_bwd_matches_float64(hip_lib, name):
    k = R.make_case(**R.MODEL_CASES[name])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert min(hp["embedding_l2_reg"], hp["linear_l2_reg"], hp["deep_l2_reg"]) > 0
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp)
    e = _engine(spec, hp, p)
    assert not any(n.endswith("_feat_bias") for n in e.params) and e.use_linear == hp["use_linear"]
    assert e.W == hp["embedding_size"] + R.pairs(spec.F) and e.ldx % 4 == 0 and 0 <= e.ldx - e.W < 4
    idx_d, dense_d, y_d = idx.cuda(), dense.to(F32).cuda(), y.cuda()
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    _compare(e, idx_d, loss, ref, what=name + ": ")
    assert torch.equal(e.X[:, : e.D], e.z) and float(e.X[:, e.W:].abs().sum()) == 0.0
    train_logit = e.logit.clone()
    logit_i, _ = e.forward(idx_d, dense_d, training=False)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")
    assert torch.equal(logit_i, train_logit)  # no dropout: inference logits are the training logits' bits
    assert set(e.state_dict()) == set(p)
    for n, v in e.state_dict().items():
        assert torch.equal(v.cpu().reshape(p[n].shape), p[n].to(F32)), n


def test_dlrm_regression_task(hip_lib):
    k = R.make_case(**R.MODEL_CASES["d16"])
    p, spec, idx, dense, hp = (k[n] for n in ("p", "spec", "idx", "dense", "hp"))
    yf = torch.randn(idx.shape[0], generator=torch.Generator().manual_seed(4)).double()
    ref = R.fwd_bwd(p, spec, idx, dense, yf, hp, task="regression")
    e = _engine(spec, hp, p, task="regression")
    loss = e.fwd_bwd(idx.cuda(), dense.to(F32).cuda(), yf.to(F32).cuda())
    _compare(e, idx.cuda(), loss, ref, what="mse ")


def test_dlrm_multi_valued_and_value_features(hip_lib):
    """A SparseValueFeat and a MultiValCsvFeat field: their value-weighted / sqrtn-pooled rows are vectors of the
    interaction like any other."""
    k = R.make_case(**R.MODEL_CASES["linear"])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    B = idx.shape[0]
    vname, mname = spec.sparse_names[1], spec.sparse_names[3]
    spec = TL.Spec(spec.sparse_names, spec.feat_sizes, spec.dense_names, multi_names=[mname], value_names=[vname])
    g = torch.Generator().manual_seed(11)
    vids = torch.randint(0, spec.feat_sizes[1], (B,), generator=g)
    vals = torch.randn(B, generator=g).float().double()
    vals[0] = 0.0
    n = torch.randint(0, 3, (B,), generator=g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    ids = torch.randint(0, spec.feat_sizes[3], (int(n.sum()),), generator=g)
    mv = {vname: (vids, vals), mname: (offsets, ids)}
    assert R.min_abs_pre(p, spec, idx, dense, hp, mv=mv) >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, mv=mv)
    e = _engine(spec, hp, p)
    mv_d = {vname: (torch.arange(B + 1).cuda(), vids.cuda(), vals.to(F32).cuda()), mname: (offsets.cuda(), ids.cuda())}
    loss = e.fwd_bwd(idx.cuda(), dense.to(F32).cuda(), y.cuda(), mv=mv_d)
    _compare(e, idx.cuda(), loss, ref, what="mv ")
    logit_i, _ = e.forward(idx.cuda(), dense.to(F32).cuda(), training=False, mv=mv_d)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")


def test_dlrm_with_a_sequence_feature(hip_lib):
    """A SequenceFeat: its attention-pooled row is a vector of the interaction, and the query / key gradients arrive
    through Engine._seq_bwd."""
    from recman_amd import engine as eng
    from tests import asp_ref as S

    k = S.make_model_case(**S.MODEL_CASES["din_d8"])
    spec, idx, dense, y, mv = k["spec"], k["idx"], k["dense"], k["y"], k["mv"]
    F, D, Dn = spec.F, 8, dense.shape[1]
    hp = dict(k["hp"], bottom_hidden_units=(16,), deep_hidden_units=(32, 32), deep_dropout=(1, 1, 1), deep_l2_reg=1e-3,
              use_linear=True)
    p = {n: v for n, v in k["p"].items() if not n.startswith("dnn_")}
    p.update(R.tower_params(R._rnd(torch.Generator().manual_seed(77)), D, F, Dn, (16,), (32, 32)))

    def step(pp, dn):
        leaves = {n: v.detach().clone().requires_grad_(True) for n, v in pp.items()}
        E = S.embeddings(leaves, spec, idx, mv, hp)
        out, pres = R.logit_from_embeddings(leaves, E, dn, hp, return_pre=True)
        logit = out + TL.linear_layer(leaves, spec.tl, idx[:, spec.plain_cols], dn)
        pred = TL.prediction(logit, "classification")
        l2 = TL.embedding_l2(leaves, spec.tl, 1e-3) + TL.linear_l2(leaves, 1e-3) + R.tower_l2(leaves, hp)
        loss = TL.create_loss(y, pred, "classification") + l2
        loss.backward()
        grads = {n: (v.grad if v.grad is not None else torch.zeros_like(v)) for n, v in leaves.items()}
        return (loss.detach(), logit.detach().reshape(-1), pred.detach(), grads), min(float(t.detach().abs().min()) for t in pres)

    ref, closest = step(p, dense)
    assert closest >= R.KINK and k["min_abs_z"] >= R.KINK
    g32 = step(_f32(p), dense.to(F32))[0][3]
    e = eng.DLRMEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                       seq_query=spec.seq_query, seq_max_len=spec.seq_max_len), D, hp)
    e.load_params(_f32(p))
    mv_d = {n: (o.cuda(), i.cuda()) for n, (o, i) in mv.items()}
    idx_d = idx.cuda()
    loss = e.fwd_bwd(idx_d, dense.to(F32).cuda(), y.cuda(), mv=mv_d)
    torch.cuda.synchronize()
    _close(e.logit, ref[1], rtol=0, atol=1e-5, what="seq logit")
    _close(loss, ref[0].reshape(1), what="seq loss")
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(ref[3])
    for n, want in ref[3].items():
        m, m32 = R.grad_measure(grads[n], want), R.grad_measure(g32[n], want)
        # (the attention unit's batch-summed gradients: the bound of tests/test_gpu_autoint_model.py's sequence test)
        bound = max(2e-5, 4 * m32) if n.startswith("hist_asp_") else 2e-5
        print(f"seq: {n} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        assert m <= bound, n
    assert float(grads["hist_asp_w"].abs().max()) > 0 and float(grads["item_feat_embed"].abs().max()) > 0


def test_dlrm_deep_dropout_with_given_masks(hip_lib):
    k = R.make_case(**R.MODEL_CASES["d16"])
    p, spec, idx, dense, y = (k[n] for n in ("p", "spec", "idx", "dense", "y"))
    hp = dict(k["hp"], deep_dropout=(0.9, 0.8, 0.8))
    B, W = idx.shape[0], 16 + R.pairs(spec.F)
    g = torch.Generator().manual_seed(21)
    masks = [(torch.rand(B, d, generator=g) < kp).double() for d, kp in zip((W, 32, 32), hp["deep_dropout"])]
    assert all(bool((m == 0).any()) for m in masks)
    assert R.min_abs_pre(p, spec, idx, dense, hp, masks={"dnn": masks}) >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, masks={"dnn": masks})
    e = _engine(spec, hp, p)
    idx_d, dense_d = idx.cuda(), dense.to(F32).cuda()
    md = {"dnn": [m.to(F32).cuda() for m in masks]}
    loss = e.fwd_bwd(idx_d, dense_d, y.cuda(), masks=md)
    _compare(e, idx_d, loss, ref, what="dropout ")
    # inference ignores the masks
    plain = R.dlrm_logit(p, spec, idx, dense, hp, training=False).reshape(-1)
    logit_i, _ = e.forward(idx_d, dense_d, training=False, masks=md)
    _close(logit_i, plain, rtol=0, atol=1e-5, what="inference logit")
    assert float((plain - ref[1]).abs().max()) > 1e-4


def test_dlrm_engine_rejects_what_it_cannot_run(hip_lib):
    from recman_amd import engine as eng

    hp = dict(deep_hidden_units=(8,))
    with pytest.raises(ValueError, match="dense feature"):
        eng.DLRMEngine(eng.FeatureSpec(["a", "b"], [4, 5]), 16, hp)
    with pytest.raises(ValueError, match=r"not supported.*1\.\.40 embedding features, embedding_size 8/16/32/64"):
        eng.DLRMEngine(eng.FeatureSpec(["a", "b"], [4, 5], ["x"]), 12, hp)
    with pytest.raises(ValueError, match="not supported"):
        eng.DLRMEngine(eng.FeatureSpec([f"f{i}" for i in range(41)], [3] * 41, ["x"]), 16, hp)
    e = eng.DLRMEngine(eng.FeatureSpec(["a", "b"], [4, 5], ["x", "y"]), 16, hp)  # the defaults
    assert e.use_linear is False and e.bot.widths == [64, 32, 16] and e.W == 19 and e.ldx == 20


def test_init_reference_names_shapes_and_determinism(hip_lib):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x", "y"])
    hp = dict(bottom_hidden_units=(12,), deep_hidden_units=(16, 8))
    e1, e2, e3 = (eng.DLRMEngine(spec, 8, hp) for _ in range(3))
    eng.init_reference(e1, 5), eng.init_reference(e2, 5), eng.init_reference(e3, 6)
    want = {"bot_dnn_layer_0_weights": (2, 12), "bot_dnn_layer_0_bias": (12,), "bot_dnn_layer_1_weights": (12, 8),
            "bot_dnn_layer_1_bias": (8,), "top_dnn_layer_0_weights": (14, 16), "top_dnn_layer_0_bias": (16,),
            "top_dnn_layer_1_weights": (16, 8), "top_dnn_layer_1_bias": (8,), "top_dnn_w": (8, 1), "top_dnn_w0": (1,)}
    assert {n: tuple(v.shape) for n, v in e1.params.items() if n.startswith(("bot_", "top_"))} == want
    assert not any(n.endswith("_feat_bias") or n.startswith("dnn_") for n in e1.params)
    for n, shape in want.items():
        assert torch.equal(e1.params[n], e2.params[n]), n
        if len(shape) == 2:
            std = (2.0 / sum(shape)) ** 0.5
            assert 0 < float(e1.params[n].abs().max()) <= 2 * std + 1e-6 and not torch.equal(e1.params[n], e3.params[n])
        else:
            assert float(e1.params[n].abs().max()) == 0.0


def test_roofline_probes_list_the_two_kernels(hip_lib):
    k = R.make_case(**R.MODEL_CASES["d16"])
    e = _engine(k["spec"], k["hp"], k["p"])
    idx_d, dense_d, y_d = k["idx"].cuda(), k["dense"].to(F32).cuda(), k["y"].cuda()
    probes = e.roofline_probes(idx_d, dense_d, y_d)
    assert [p["symbol"] for p in probes[:2]] == ["dot_bwd_kernel", "dot_fwd_kernel"]
    B, F, D, ldx = idx_d.shape[0], 5, 16, 32
    assert e.ldx == ldx and all(p["bound"] == "hbm" for p in probes[:2])
    assert probes[1]["work"] == 4 * B * (F * D + D + ldx) and probes[0]["work"] == 4 * B * (2 * F * D + 2 * D + ldx)
    x0, d0 = e.X.clone(), e.d_rows.clone()
    for p in probes:
        p["fn"]()
    torch.cuda.synchronize()
    assert torch.equal(e.X, x0) and torch.equal(e.d_rows, d0)  # the probes recompute on the step's own E and z


# -------------------------------------------------------------------------------------------- DotInteraction
def test_dot_interaction_layer_under_autograd_matches_float64(hip_lib):
    from recman_amd.th import layers as L

    for shape in ((131, 26, 16), (6, 7, 16)):
        case = R.kernel_case(*shape)
        E = case["E"].to(F32).cuda().requires_grad_(True)
        z = case["z"].to(F32).cuda().requires_grad_(True)
        X = L.DotInteraction()(E, z)
        assert X.shape == (shape[0], shape[2] + R.pairs(shape[1]))
        (X * case["dX"].to(F32).cuda()).sum().backward()
        R.check_fwd(X, case)
        R.check_bwd(E.grad, z.grad, case)
    assert L.DotInteraction().l2() == 0.0
    with pytest.raises(ValueError, match="unsupported"):
        L.DotInteraction()(torch.randn(4, 3, 12, device="cuda"), torch.randn(4, 12, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        L.DotInteraction()(torch.randn(4, 3, 16, device="cuda"), torch.randn(4, 8, device="cuda"))


# -------------------------------------------------------------------------------------------------- th.DLRM
def _synthetic(n=300, seed=0):
    import pandas as pd
    from sklearn.preprocessing import MinMaxScaler

    from recman_amd.th import DenseFeat, FeatureDictionary, SparseFeat

    rs = np.random.RandomState(seed)
    df = pd.DataFrame({"u": rs.randint(0, 12, n), "i": rs.randint(0, 20, n), "c": rs.randint(0, 4, n),
                       "x": rs.randn(n).astype(np.float32), "t": rs.rand(n).astype(np.float32)})
    score = 0.8 * (df["c"].values - 1.5) + 1.2 * df["x"].values + 0.1 * (df["u"].values % 3) - 0.3
    df["label"] = (score + 0.3 * rs.randn(n) > 0).astype(np.int64)
    fd = FeatureDictionary()
    for c in ("u", "i", "c"):
        fd[c] = SparseFeat(name=c, feat_size=len(np.unique(df[c].values)))
    for c in ("x", "t"):
        fd[c] = DenseFeat(name=c, scaler=MinMaxScaler())
    fd.initialize(df)
    return df, fd


def test_fit_predict_save_restore(hip_lib, tmp_path):
    import recman_amd.th as th

    df, fd = _synthetic()
    yv = df["label"].values
    kw = dict(embedding_size=8, bottom_hidden_units=(16,), deep_hidden_units=(32, 32), epoch=2, batch_size=64,
              learning_rate=0.02, deep_l2_reg=1e-5)
    m = th.DLRM(fd, **kw)
    e = m._build()
    assert e.model == "dlrm" and set(m.hparams) >= {"embedding_size", "bottom_hidden_units", "deep_hidden_units",
                                                    "deep_dropout", "use_linear", "learning_rate", "optimizer"}
    p0 = {k: v.cpu() for k, v in e.state_dict().items()}
    assert float(p0["top_dnn_w"].abs().max()) > 0 and float(p0["bot_dnn_layer_0_weights"].abs().max()) > 0
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, yv)
    idx, dense = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense)
    pred0 = m.predict(df)
    want0 = TL.prediction(R.dlrm_logit(p0, spec, idx, dense, m.hparams, training=False)).numpy()
    assert pred0.shape == (300,) and pred0.dtype == np.float32 and np.abs(pred0 - want0).max() < 1e-6
    before = log_loss(yv, pred0.astype(np.float64))
    assert m.fit(df, yv, random_seed_for_mini_batch=False) is None
    pred1 = m.predict(df)
    after = log_loss(yv, pred1.astype(np.float64))
    print(f"log loss {before:.4f} -> {after:.4f}")
    assert after < before - 0.01
    # predict() is the engine's forward
    _, pe = e.forward(idx.cuda(), dense.cuda(), training=False)
    assert np.array_equal(pe.cpu().numpy(), pred1)
    res = m.evaluate(df, yv)
    assert len(res) == 2 and all(np.isfinite(r) for r in res)
    # save / restore round-trips the variables by name
    path = str(tmp_path / "ckpt.pt")
    m.save(path)
    saved = torch.load(path, weights_only=True)
    assert set(saved) == set(p0) and {"top_dnn_w", "top_dnn_w0", "bot_dnn_layer_1_bias"} <= set(saved)
    m2 = th.DLRM(fd, random_seed=7, **kw)
    assert np.abs(m2.predict(df) - pred1).max() > 1e-4
    m2.restore(path)
    assert np.array_equal(m2.predict(df), pred1)
    for n, v in m2._engine.state_dict().items():
        assert torch.equal(v.cpu(), saved[n]), n


def test_fit_with_deep_dropout(hip_lib):
    import recman_amd.th as th

    df, fd = _synthetic()
    yv = df["label"].values
    d = th.DLRM(fd, embedding_size=8, bottom_hidden_units=(), deep_hidden_units=(16, 16), deep_dropout=(1, 0.8, 0.8),
                use_linear=True, epoch=2, batch_size=64, learning_rate=0.02)
    masks = d._dropout_masks(16)
    assert set(masks) == {"dnn"} and masks["dnn"][0] is None and masks["dnn"][1].shape == (16, 16)
    assert th.DLRM(fd, deep_dropout=(0.9, 1, 1))._dropout_masks(5)["dnn"][0].shape == (5, 8 + R.pairs(3))
    before = log_loss(yv, d.predict(df).astype(np.float64))
    d.fit(df, yv, random_seed_for_mini_batch=False)
    assert log_loss(yv, d.predict(df).astype(np.float64)) < before
    assert np.array_equal(d.predict(df), d.predict(df))  # no dropout outside training


def test_row_sharded_build_is_refused_and_a_dense_feature_is_required(hip_lib):
    import recman_amd.th as th
    from recman_amd.th import FeatureDictionary, SparseFeat

    df, fd = _synthetic()
    m = th.DLRM(fd, embedding_size=8)
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m._build()
    fd2 = FeatureDictionary()
    for c in ("u", "i"):
        fd2[c] = SparseFeat(name=c, feat_size=len(np.unique(df[c].values)))
    fd2.initialize(df)
    with pytest.raises(ValueError, match="dense feature"):
        th.DLRM(fd2, embedding_size=8)._build()
