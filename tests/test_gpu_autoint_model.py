"""GPU: the AutoInt engine, th.AutoInt and th.layers.InteractingLayer against the float64 restatement
(tests/autoint_ref.py), in the manner and with the tolerances of tests/test_gpu_parity.py, tests/test_gpu_models.py and
tests/test_gpu_afm_model.py: logits 1e-5, every gradient with the gradient measure; the batch-summed gradients of the
interacting layers and the last projection use the kernel tests' bound max(2e-5, 4 x the float32 CPU restatement's own
error on the case).  The label-driven upstream gradient of the model-level cases cannot be zeroed, so their seeds keep
every unit of every layer away from its kink (asserted on the CPU in tests/test_autoint_host.py)."""
import numpy as np
import pytest
import torch
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import autoint_ref as R
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(spec, hp, p, task="classification", **spec_kw):
    from recman_amd import engine as eng

    kw = spec_kw or dict(multi_names=spec.multi_names, value_names=spec.value_names)
    e = eng.AutoIntEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names, **kw),
                          hp["embedding_size"], hp, task=task)
    e.load_params({k: v.to(F32) for k, v in p.items()})
    return e


def _compare(e, idx_d, loss, ref, g32, what=""):
    loss_o, logit_o, pred_o, grads_o = ref
    torch.cuda.synchronize()
    err = float((e.logit.cpu().double() - logit_o).abs().max())
    print(f"{what}logit err {err:.2e}")
    _close(e.logit, logit_o, rtol=0, atol=1e-5, what=what + "logit")
    _close(e.pred, pred_o, rtol=0, atol=1e-6, what=what + "pred")
    _close(loss, loss_o.reshape(1), what=what + "loss")
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o), set(grads) ^ set(grads_o)
    for k in grads_o:
        if k.startswith("autoint_"):
            m, m32 = R.grad_measure(grads[k], grads_o[k]), R.grad_measure(g32[k], grads_o[k])
            bound = max(2e-5, 4 * m32)
            print(f"{what}{k} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
            assert m <= bound, f"{what}grad {k}: measure {m:.3e} > {bound:.3e} (float32 CPU {m32:.3e})"
        else:
            _close_grad(grads[k], grads_o[k], what=f"{what}grad {k}")


def _f32(p):
    return {n: v.to(F32) for n, v in p.items()}


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_autoint_fwd_bwd_matches_float64(hip_lib, name):
    k = R.make_case(**R.MODEL_CASES[name])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert min(hp["embedding_l2_reg"], hp["linear_l2_reg"], hp["att_l2_reg"]) > 0
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp)
    g32 = R.fwd_bwd(_f32(p), spec, idx, dense.to(F32), y, hp)[3]
    e = _engine(spec, hp, p)
    assert not any(n.endswith("_feat_bias") for n in e.params)
    assert (e.mlp is not None) == bool(hp["deep_hidden_units"])
    idx_d, dense_d, y_d = idx.cuda(), dense.to(F32).cuda(), y.cuda()
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    _compare(e, idx_d, loss, ref, g32, what=name + ": ")
    logit_i, _ = e.forward(idx_d, dense_d, training=False)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")
    e.forward(idx_d, dense_d, training=True)
    assert torch.equal(e.logit, logit_i)  # forward(training=False) equals the training logits
    assert set(e.state_dict()) == set(p)


def test_autoint_regression_task(hip_lib):
    k = R.make_case(**R.MODEL_CASES["d16"])
    p, spec, idx, dense, hp = (k[n] for n in ("p", "spec", "idx", "dense", "hp"))
    yf = torch.randn(idx.shape[0], generator=torch.Generator().manual_seed(4)).double()
    ref = R.fwd_bwd(p, spec, idx, dense, yf, hp, task="regression")
    g32 = R.fwd_bwd(_f32(p), spec, idx, dense.to(F32), yf.to(F32), hp, task="regression")[3]
    e = _engine(spec, hp, p, task="regression")
    loss = e.fwd_bwd(idx.cuda(), dense.to(F32).cuda(), yf.to(F32).cuda())
    _compare(e, idx.cuda(), loss, ref, g32, what="mse ")


def test_autoint_multi_valued_and_value_features(hip_lib):
    """A SparseValueFeat and a MultiValCsvFeat field: their value-weighted / sqrtn-pooled rows are fields of the
    attention like any other."""
    k = R.make_case(**R.MODEL_CASES["d8"])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    B = idx.shape[0]
    vname, mname = spec.sparse_names[1], spec.sparse_names[3]
    spec = TL.Spec(spec.sparse_names, spec.feat_sizes, spec.dense_names, multi_names=[mname], value_names=[vname])
    g = torch.Generator().manual_seed(11)
    vids = torch.randint(0, spec.feat_sizes[1], (B,), generator=g)
    vals = torch.randn(B, generator=g).double()
    vals[0] = 0.0
    n = torch.randint(0, 3, (B,), generator=g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    ids = torch.randint(0, spec.feat_sizes[3], (int(n.sum()),), generator=g)
    mv = {vname: (vids, vals), mname: (offsets, ids)}
    # (this variant's rows differ from the plain case's: its own distance to the kinks; an all-zero row - an empty
    # bag, a zero value - puts no unit AT zero unless the whole example's pre-activation is, which the seed avoids)
    assert R.min_abs_pre(p, spec, idx, dense, hp, mv=mv) >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, mv=mv)
    g32 = R.fwd_bwd(_f32(p), spec, idx, dense.to(F32), y, hp, mv={vname: (vids, vals.to(F32)), mname: (offsets, ids)})[3]
    e = _engine(spec, hp, p)
    mv_d = {vname: (torch.arange(B + 1).cuda(), vids.cuda(), vals.to(F32).cuda()), mname: (offsets.cuda(), ids.cuda())}
    loss = e.fwd_bwd(idx.cuda(), dense.to(F32).cuda(), y.cuda(), mv=mv_d)
    _compare(e, idx.cuda(), loss, ref, g32, what="mv ")
    logit_i, _ = e.forward(idx.cuda(), dense.to(F32).cuda(), training=False, mv=mv_d)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")


def test_autoint_with_a_sequence_feature(hip_lib):
    """A SequenceFeat: its attention-pooled row is a field of the self-attention, and the query / key gradients
    arrive through Engine._seq_bwd."""
    from recman_amd import engine as eng
    from tests import asp_ref as S

    k = S.make_model_case(**S.MODEL_CASES["din_d8"])
    spec, idx, dense, y, mv = k["spec"], k["idx"], k["dense"], k["y"], k["mv"]
    hp = dict(k["hp"], att_layer_num=2, att_embedding_size=4, att_head_num=2, att_res=True, att_l2_reg=1e-3,
              deep_hidden_units=(), deep_l2_reg=0.0)
    p = {n: v for n, v in k["p"].items() if not n.startswith("dnn_")}
    rnd = R._rnd(torch.Generator().manual_seed(77))
    for l in range(2):
        for n in R.layer_names(l):
            p[n] = R.glorot(rnd, 8, 8)
    p["autoint_w"], p["autoint_w0"] = R.glorot(rnd, spec.F * 8, 1), rnd(1, std=0.1)

    def step(pp, dn):
        leaves = {n: v.detach().clone().requires_grad_(True) for n, v in pp.items()}
        E = S.embeddings(leaves, spec, idx, mv, hp)
        out, pres = R.autoint_stack(leaves, E, hp, return_pre=True)
        logit = TL.linear_layer(leaves, spec.tl, idx[:, spec.plain_cols], dn) + out.reshape(-1, 1)
        pred = TL.prediction(logit, "classification")
        l2 = (TL.embedding_l2(leaves, spec.tl, 1e-3) + TL.linear_l2(leaves, 1e-3)
              + sum(1e-3 * 0.5 * leaves[n].square().sum() for n in R.att_names(hp)))
        loss = TL.create_loss(y, pred, "classification") + l2
        loss.backward()
        grads = {n: (v.grad if v.grad is not None else torch.zeros_like(v)) for n, v in leaves.items()}
        return (loss.detach(), logit.detach().reshape(-1), pred.detach(), grads), min(float(t.detach().abs().min()) for t in pres)

    ref, closest = step(p, dense)
    assert closest >= R.KINK
    g32 = step(_f32(p), dense.to(F32))[0][3]
    e = eng.AutoIntEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                          seq_query=spec.seq_query, seq_max_len=spec.seq_max_len), 8, hp)
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
        bound = 2e-5 if not (n.startswith("autoint_") or n.startswith("hist_asp_")) else max(2e-5, 4 * m32)
        print(f"seq: {n} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        assert m <= bound, n
    assert float(grads["hist_asp_w"].abs().max()) > 0 and float(grads["item_feat_embed"].abs().max()) > 0


def test_autoint_engine_rejects_unsupported_shapes(hip_lib):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6])
    for D, hp in ((12, {}), (16, {"att_head_num": 3}), (16, {"att_embedding_size": 2}),
                  (16, {"att_embedding_size": 64, "att_head_num": 2}), (16, {"att_embedding_size": 12})):
        with pytest.raises(ValueError, match="not supported"):
            eng.AutoIntEngine(spec, D, hp)
    with pytest.raises(ValueError, match="not supported"):
        eng.AutoIntEngine(eng.FeatureSpec([f"f{i}" for i in range(41)], [3] * 41), 16, {})
    with pytest.raises(ValueError, match="att_layer_num"):
        eng.AutoIntEngine(spec, 16, {"att_layer_num": 0})
    # DeepFM keeps its own rule
    with pytest.raises(AssertionError):
        eng.DeepFMEngine(spec, 16, {"use_fm": False, "use_deep": False, "deep_hidden_units": ()})
    e = eng.AutoIntEngine(spec, 16, {})  # the defaults: three layers, two heads of 8, residual, no DNN
    assert e.L == 3 and e.H == 2 and e.dk == 8 and e.res and e.mlp is None and e.scale == 1.0
    assert eng.AutoIntEngine(spec, 16, {"att_scaling": True}).scale == 8 ** -0.5


def test_roofline_probes_list_the_layer_0_kernels(hip_lib):
    k = R.make_case(**R.MODEL_CASES["d16"])
    e = _engine(k["spec"], k["hp"], k["p"])
    idx_d, dense_d, y_d = k["idx"].cuda(), k["dense"].to(F32).cuda(), k["y"].cuda()
    probes = e.roofline_probes(idx_d, dense_d, y_d)
    assert [p["symbol"] for p in probes[:2]] == ["autoint_bwd_kernel", "autoint_fwd_kernel"]
    B, F, D, HD = idx_d.shape[0], 5, 16, 16
    fwd = B * (8 * F * D * HD + 4 * F * F * HD)
    assert probes[1]["work"] == fwd and probes[0]["work"] == 3 * fwd and all(p["bound"] == "mfma" for p in probes[:2])
    y0 = e.att_Y[0].clone()
    for p in probes:
        p["fn"]()
    torch.cuda.synchronize()
    assert torch.equal(e.att_Y[0], y0)  # the forward probe recomputes layer 0 on the step's own E
    assert bool(torch.isfinite(e.grads["autoint_layer_0_query_w"]).all())


def test_init_reference_names_shapes_and_determinism(hip_lib):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x"])
    hp = dict(att_layer_num=2, att_embedding_size=4, att_head_num=4, deep_hidden_units=(8,))
    e1, e2, e3 = (eng.AutoIntEngine(spec, 8, hp) for _ in range(3))
    eng.init_reference(e1, 5), eng.init_reference(e2, 5), eng.init_reference(e3, 6)
    want = {"autoint_layer_0_query_w": (8, 16), "autoint_layer_0_key_w": (8, 16), "autoint_layer_0_value_w": (8, 16),
            "autoint_layer_0_res_w": (8, 16), "autoint_layer_1_query_w": (16, 16), "autoint_layer_1_key_w": (16, 16),
            "autoint_layer_1_value_w": (16, 16), "autoint_layer_1_res_w": (16, 16), "autoint_w": (48, 1),
            "autoint_w0": (1,)}
    assert {n: tuple(v.shape) for n, v in e1.params.items() if n.startswith("autoint")} == want
    assert "dnn_layer_0_weights" in e1.params and not any(n.endswith("_feat_bias") for n in e1.params)
    for n in want:
        assert torch.equal(e1.params[n], e2.params[n]), n
        if n != "autoint_w0":
            std = (2.0 / sum(want[n])) ** 0.5
            assert 0 < float(e1.params[n].abs().max()) <= 2 * std + 1e-6 and not torch.equal(e1.params[n], e3.params[n])
    assert float(e1.params["autoint_w0"].abs().max()) == 0.0
    assert not torch.equal(e1.params["autoint_layer_0_query_w"], e1.params["autoint_layer_0_key_w"])
    no_res = eng.AutoIntEngine(spec, 8, dict(hp, att_res=False, deep_hidden_units=()))
    assert not any(n.endswith("res_w") or n.startswith("dnn") for n in no_res.params)


def test_autoint_sparse_step_equals_dense_step_when_reset_every_batch(hip_lib):
    """Every row touched, no l2, optimizer rebuilt per batch: the row-wise step and the dense-gradient step coincide
    (tests/test_gpu_optim.py shows it for the other models)."""
    from recman_amd.optim import Optimizer, SparseTableOptimizer

    k = R.make_case(B=300, F=5, D=16, Dn=2, L=2, H=2, dk=8, seed=0, hidden=(16,))
    p, spec, idx, dense, y = (k[n] for n in ("p", "spec", "idx", "dense", "y"))
    hp = dict(k["hp"], embedding_l2_reg=0.0, linear_l2_reg=0.0, att_l2_reg=0.0, deep_l2_reg=0.0)
    e1, e2 = _engine(spec, hp, p), _engine(spec, hp, p)
    dopt = Optimizer("adam", 0.01)
    sopt, sdense = SparseTableOptimizer(e2, "adam", 0.01), Optimizer("adam", 0.01)
    idx_d, dense_d, y_d = idx.cuda(), dense.to(F32).cuda(), y.cuda()
    for step in range(3):
        e1.fwd_bwd(idx_d, dense_d, y_d)
        dopt.reset()
        dopt.step(e1.params, e1.dense_grads(idx_d))
        e2.fwd_bwd(idx_d, dense_d, y_d)
        sdense.reset()
        sopt.step(idx_d, reset=True)
        sdense.step(e2.params, e2.grads)
        for name in e1.params:
            a, b = e1.params[name], e2.params[name]
            assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(a.abs().max())), (step, name)


# -------------------------------------------------------------------------------------------- th.AutoInt
def _ml():
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    return df, ml_features(df)


def test_fit_predict_matches_a_torch_training_loop(hip_lib):
    """Two epochs of fit() on the ml-100k golden slice against a torch loop over the restatement with the project's
    Optimizer (same initial weights, shuffles and batches), to the 2e-4 of tests/test_gpu_models.py."""
    from sklearn.utils import check_random_state

    import recman_amd.th as th
    from recman_amd.optim import Optimizer

    df, fd = _ml()
    m = th.AutoInt(fd, embedding_size=8, att_layer_num=2, att_embedding_size=4, learning_rate=0.01, epoch=2,
                   batch_size=256, random_seed=2019)
    e = m._build()
    hp = dict(m.hparams)
    assert set(hp) >= {"embedding_size", "att_layer_num", "att_embedding_size", "att_head_num", "att_res", "att_scaling",
                       "att_l2_reg", "deep_hidden_units", "deep_dropout", "learning_rate", "optimizer"}
    p0 = {k: v.cpu() for k, v in e.state_dict().items()}
    assert set(R.att_names(hp)) <= set(p0) and float(p0["autoint_w0"].abs().max()) == 0.0
    assert all(float(p0[n].abs().max()) > 0 for n in R.att_names(hp))
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, df["label"].values)
    idx, dense, y = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense), torch.from_numpy(inp.y)

    pred0 = m.predict(df)
    want0 = TL.prediction(R.autoint_logit(p0, spec, idx, dense, hp, training=False)).numpy()
    assert pred0.shape == (1024,) and pred0.dtype == np.float32
    assert np.abs(pred0 - want0).max() < 1e-6
    assert m.fit(df, df["label"].values, random_seed_for_mini_batch=False) is None

    p, opt, n = {k: v.clone() for k, v in p0.items()}, Optimizer("adam", 0.01), len(y)
    ix, dn, yy = idx, dense, y
    for _ in range(2):
        perm = np.arange(n)
        check_random_state(2019).shuffle(perm)
        ix, dn, yy = ix[perm], dn[perm], yy[perm]
        for s in range(0, n, 256):
            _, _, _, g = R.fwd_bwd(p, spec, ix[s:s + 256], dn[s:s + 256], yy[s:s + 256], hp)
            opt.step(p, g)
    pred1 = m.predict(df)
    want1 = TL.prediction(R.autoint_logit(p, spec, idx, dense, hp, training=False)).numpy()
    assert np.abs(pred1 - want1).max() < 2e-4, np.abs(pred1 - want1).max()
    assert np.abs(pred1 - pred0).max() > 1e-3  # it did train
    res = m.evaluate(df, df["label"].values)
    assert len(res) == 2 and all(np.isfinite(r) for r in res)


def test_evaluate_on_the_gpu_metrics_path(hip_lib):
    import recman_amd.th as th
    from recman_amd import metrics as gm

    df, fd = _ml()
    on_dev = [f for f in (getattr(gm, "roc_auc_score", None), getattr(gm, "log_loss", None)) if f is not None]
    assert on_dev and all(getattr(f, "on_device", False) for f in on_dev)
    m = th.AutoInt(fd, embedding_size=8, att_layer_num=1, deep_hidden_units=(16, 16), epoch=1, batch_size=256,
                   learning_rate=0.01, eval_metric=tuple(on_dev))
    assert m._metrics_on_device()
    m.fit(df, df["label"].values, random_seed_for_mini_batch=False)
    res = m.evaluate(df, df["label"].values)
    pred = m.predict(df).astype(np.float64)
    from sklearn.metrics import roc_auc_score

    assert abs(res[0] - roc_auc_score(df["label"].values, pred)) < 1e-6
    assert abs(res[1] - log_loss(df["label"].values, pred)) < 1e-5


def test_save_restore_clone_and_best_model_finder(hip_lib, tmp_path):
    from sklearn.base import clone

    import recman_amd.th as th

    df, fd = _ml()
    kw = dict(embedding_size=8, att_layer_num=2, att_head_num=4, att_embedding_size=4, deep_hidden_units=(16,),
              epoch=2, batch_size=256, learning_rate=0.01, eval_metric=(log_loss,))
    m = th.AutoInt(fd, **kw)
    (tmp_path / "best").mkdir()
    finder = th.BestModelFinder(save_model=True, directory=str(tmp_path / "best"))
    tr, va = df.iloc[:768], df.iloc[768:]
    m.fit(tr, tr["label"].values, va, va["label"].values, epoch_callback=finder, random_seed_for_mini_batch=False)
    a = m.predict(df)
    path = str(tmp_path / "ckpt.pt")
    m.save(path)
    m2 = th.AutoInt(fd, random_seed=7, **kw)
    assert np.abs(m2.predict(df) - a).max() > 1e-4
    m2.restore(path)
    assert np.array_equal(m2.predict(df), a)
    c = clone(m)
    assert isinstance(c, th.AutoInt) and c.get_params()["att_head_num"] == 4 and c.get_params()["deep_dropout"] is None
    assert c._engine is None and c.predict(df).shape == (1024,)
    assert finder.best_model is m and finder.best_score is not None
    m3 = th.BestModelFinder.load(th.AutoInt, str(tmp_path / "best"))
    assert m3.hparams == m.hparams
    best_valid = log_loss(va["label"].values, m3.predict(va).astype(np.float64))
    assert abs(best_valid - finder.best_score) < 1e-5


def test_fit_with_the_row_wise_optimizer_and_with_deep_dropout(hip_lib):
    import recman_amd.th as th

    df, fd = _ml()
    yv = df["label"].values
    s = th.AutoInt(fd, embedding_size=8, att_layer_num=2, embedding_l2_reg=0.0, linear_l2_reg=0.0, epoch=3,
                   batch_size=128, learning_rate=0.01)
    s.hparams["sparse_optimizer"] = True
    before = log_loss(yv, s.predict(df).astype(np.float64))
    s.fit(df, yv, random_seed_for_mini_batch=False)
    assert s._sparse_opt is not None and s._sparse_opt.t > 0 and s._dense_fused is not None
    after = log_loss(yv, s.predict(df).astype(np.float64))
    print(f"row-wise optimizer: log loss {before:.4f} -> {after:.4f}")
    assert after < before - 0.01
    d = th.AutoInt(fd, embedding_size=8, att_layer_num=1, deep_hidden_units=(16, 16), deep_dropout=(1, 0.8, 0.8),
                   epoch=2, batch_size=128, learning_rate=0.01)
    assert d.hparams["deep_dropout"] == (1, 0.8, 0.8) and set(d._dropout_masks(16)) == {"dnn"}
    assert th.AutoInt(fd, deep_hidden_units=(16, 16)).hparams["deep_dropout"] == (1, 1, 1)
    before = log_loss(yv, d.predict(df).astype(np.float64))
    d.fit(df, yv, random_seed_for_mini_batch=False)
    assert log_loss(yv, d.predict(df).astype(np.float64)) < before
    assert np.array_equal(d.predict(df), d.predict(df))  # no dropout outside training


def test_row_sharded_build_is_refused(hip_lib):
    import recman_amd.th as th

    df, fd = _ml()
    m = th.AutoInt(fd, embedding_size=8)
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m._build()


# ---------------------------------------------------------------------------------------- InteractingLayer
def test_interacting_layer_under_autograd_matches_float64(hip_lib):
    from recman_amd.th import layers as L

    k = R.gpu_case((130, 26, 16, 2, 16))
    for use_res, scaling in ((True, False), (False, True)):
        variables = {}
        layer = L.InteractingLayer(variables, 16, 2, use_res, scaling, prefix="autoint_layer_0_", seed=3, l2_reg=1e-3)
        X = k["X"].to(F32).cuda().requires_grad_(True)
        names = R.layer_names(0, use_res)
        assert layer(X).shape == (130, 26, 32) and list(variables) == names
        assert not torch.equal(variables[names[0]], variables[names[1]])
        keys = ("Wq", "Wk", "Wv", "Wr")[:len(names)]
        with torch.no_grad():
            for name, key in zip(names, keys):
                variables[name].copy_(k[key].to(F32).cuda())
        Y = layer(X)
        (Y * k["dY"].to(F32).cuda()).sum().backward()
        want = R.layer_reference(k, use_res, False, scaling)
        cpu32 = R.layer_reference(k, use_res, False, scaling, dtype=F32)
        assert float((Y.detach().cpu().double() - want[0]).abs().max()) <= 1e-5
        assert R.grad_measure(X.grad, want[1]) <= 2e-5
        for name, w, c32 in zip(names, want[2:], cpu32[2:]):
            assert R.grad_measure(variables[name].grad, w) <= max(2e-5, 4 * R.grad_measure(c32, w)), name
        assert [id(w) for w in layer.weights] == [id(variables[n]) for n in names]
        want_l2 = 1e-3 * 0.5 * sum(float(k[key].square().sum()) for key in keys)
        assert abs(float(layer.l2().detach()) - want_l2) < 1e-5 * max(1.0, want_l2)


def test_autoint_graph_composed_from_layers(hip_lib):
    """The model from the layer callables: embeddings without bias use, linear + the interacting layers + the last
    projection, PredictionLayer(use_bias=False) - against the restatement and the engine."""
    from recman_amd.th import DataInputs, DenseFeat, FeatureDictionary, SparseFeat
    from recman_amd.th import layers as L

    k = R.make_case(**R.MODEL_CASES["three_layers"])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    fd = FeatureDictionary()
    for n, v in zip(spec.sparse_names, spec.feat_sizes):
        fd[n] = SparseFeat(n, v - 1)
    for n in spec.dense_names:
        fd[n] = DenseFeat(n)
    inp = DataInputs()
    inp.idx, inp.dense, inp.mv = idx.numpy(), dense.to(F32).numpy(), {}
    for f, n in enumerate(spec.sparse_names):
        inp[n] = idx[:, f: f + 1].numpy()
    for j, n in enumerate(spec.dense_names):
        inp[n] = dense[:, j: j + 1].to(F32).numpy()
    inp["y"] = y.numpy()
    variables = {}

    def out():
        emb = L.FeatEmbeddingLayer(variables, fd, hp["embedding_size"], hp["embedding_l2_reg"], use_bias=False)
        x, _ = emb(inp)
        linear_feats = fd.linear_feats
        linear = L.LinearLayer(variables, linear_feats, hp["linear_l2_reg"])
        linear_logit = linear(L.LinearCombiner(linear_feats)(inp))
        layers = [emb, linear]
        for l in range(hp["att_layer_num"]):
            layers.append(L.InteractingLayer(variables, hp["att_embedding_size"], hp["att_head_num"], True, False,
                                             prefix=f"autoint_layer_{l}_", l2_reg=hp["att_l2_reg"]))
            x = layers[-1](x)
        for name, shape in (("autoint_w", (x.shape[1] * x.shape[2], 1)), ("autoint_w0", (1,))):
            if name not in variables:
                variables[name] = torch.zeros(shape, device="cuda").requires_grad_(True)
        logit = linear_logit + x.reshape(x.shape[0], -1) @ variables["autoint_w"] + variables["autoint_w0"]
        return L.PredictionLayer(variables, "classification", use_bias=False)(logit), logit, layers

    out()
    assert set(variables) == set(p)
    with torch.no_grad():
        for name, v in variables.items():
            v.copy_(p[name].to(F32).reshape(v.shape).cuda())
    pred, logit, layers = out()
    l2 = sum(layer.l2() for layer in layers) + hp["att_l2_reg"] * 0.5 * variables["autoint_w"].square().sum()
    loss = L.create_loss(inp.y, pred) + l2
    loss.backward()
    loss_o, logit_o, pred_o, grads_o = R.fwd_bwd(p, spec, idx, dense, y, hp)
    g32 = R.fwd_bwd(_f32(p), spec, idx, dense.to(F32), y, hp)[3]
    _close(logit.detach().reshape(-1), logit_o, rtol=0, atol=1e-5, what="logit")
    _close(pred.detach(), pred_o, rtol=0, atol=1e-6, what="pred")
    _close(loss.detach().reshape(1), loss_o.reshape(1), what="loss")
    for name, v in variables.items():
        got, want = v.grad.reshape(grads_o[name].shape), grads_o[name]
        if name.startswith("autoint_"):
            assert R.grad_measure(got, want) <= max(2e-5, 4 * R.grad_measure(g32[name], want)), name
        else:
            _close_grad(got, want, what=f"grad {name}")
    e = _engine(spec, hp, p)
    e.forward(idx.cuda(), dense.to(F32).cuda(), training=True)
    assert float((e.logit - logit.detach().reshape(-1)).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ timing
def _composed(X, Wq, Wk, Wv, Wr):
    """The comparator: the same arithmetic from torch ops in fp32 (Q, K, V, scores and weights in HBM)."""
    return R.interacting_layer(X, Wq, Wk, Wv, Wr, 2)


def test_fused_kernels_are_faster_than_the_composed_torch_ops(hip_lib):
    """Sanity only: at the Criteo shape one interacting layer's fused forward + backward (median of 20, alternated with
    the comparator in one process) is faster than forward + autograd backward of the same arithmetic composed from
    torch ops.  The comparator's VALUES are checked in pieces of 4096 examples."""
    from recman_amd import ops

    B, F, D, H, dk = 65536, 26, 16, 2, 8
    HD = H * dk
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    X, dY = r(B, F, D) * 0.3, r(B, F, HD)
    W = [r(D, HD) * 0.25 for _ in range(4)]
    Y, st = torch.empty(B, F, HD, device="cuda"), torch.empty(B, H, F, 2, device="cuda")
    dX, dW = torch.empty(B, F, D, device="cuda"), [torch.empty(D, HD, device="cuda") for _ in range(4)]
    ws = torch.empty(ops.autoint_layer_bwd_workspace(B, F, D, H, dk), device="cuda")
    leaves = [t.clone().requires_grad_(True) for t in [X] + W]

    def fused():
        ops.autoint_layer_fwd(X, *W, H, 1.0, Y, stats=st)
        ops.autoint_layer_bwd(X, *W, Y, st, dY, H, 1.0, dX, *dW, ws)

    def composed():
        for t in leaves:
            t.grad = None
        _composed(*leaves).backward(dY)

    for _ in range(3):
        fused()
        composed()
    tf, tc = [], []
    for _ in range(20):
        for fn, acc in ((fused, tf), (composed, tc)):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            acc.append(a.elapsed_time(z))
    mf, mc = sorted(tf)[10], sorted(tc)[10]
    print(f"fused autoint_layer_fwd + autoint_layer_bwd {mf:.3f} ms; composed torch forward + backward {mc:.3f} ms "
          f"(ratio {mc / mf:.2f})")
    # the contenders compute the same thing (gradients: tests/test_gpu_autoint.py, against float64)
    with torch.no_grad():
        for s in range(0, B, 4096):
            assert float((Y[s:s + 4096] - _composed(X[s:s + 4096], *W)).abs().max()) < 1e-5
    assert float((dX - leaves[0].grad).abs().max()) < 1e-4 * max(1.0, float(leaves[0].grad.abs().max()))
    assert mf < mc
