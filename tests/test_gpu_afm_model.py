"""GPU: the AFM engine, th.AFM and th.layers.AFMLayer against the float64 restatement (tests/afm_ref.py), in the
manner and with the tolerances of tests/test_gpu_parity.py and tests/test_gpu_models.py.  The label-driven g of the
model-level cases cannot be zeroed, so their seeds keep every hidden unit away from its kink (asserted on the CPU in
tests/test_afm_host.py)."""
import numpy as np
import pytest
import torch
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import afm_ref as R
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(spec, D, hp, p, task="classification"):
    from recman_amd import engine as eng

    e = eng.AFMEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                      spec.multi_names, spec.value_names), D, hp, task=task)
    e.load_params({k: v.to(F32) for k, v in p.items()})
    return e


def _compare(e, idx_d, loss, ref, what=""):
    loss_o, logit_o, pred_o, grads_o = ref
    torch.cuda.synchronize()
    _close(e.logit, logit_o, rtol=0, atol=1e-5, what=what + "logit")
    _close(e.pred, pred_o, rtol=0, atol=1e-6, what=what + "pred")
    _close(loss, loss_o.reshape(1), what=what + "loss")
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o), set(grads) ^ set(grads_o)
    for k in grads_o:
        _close_grad(grads[k], grads_o[k], what=f"{what}grad {k}")


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_afm_fwd_bwd_matches_float64(hip_lib, name):
    k = R.make_afm_case(**R.MODEL_CASES[name])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert min(hp["embedding_l2_reg"], hp["linear_l2_reg"], hp["att_l2_reg"]) > 0
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp)
    e = _engine(spec, hp["embedding_size"], hp, p)
    assert not any(n.endswith("_feat_bias") for n in e.params)
    idx_d, dense_d, y_d = idx.cuda(), dense.to(F32).cuda(), y.cuda()
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    _compare(e, idx_d, loss, ref)
    logit_i, _ = e.forward(idx_d, dense_d, training=False)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")
    assert set(e.state_dict()) == set(p)


def test_afm_regression_task(hip_lib):
    k = R.make_afm_case(**R.MODEL_CASES["d16"])
    p, spec, idx, dense, hp = (k[n] for n in ("p", "spec", "idx", "dense", "hp"))
    yf = torch.randn(idx.shape[0], generator=torch.Generator().manual_seed(4)).double()
    ref = R.fwd_bwd(p, spec, idx, dense, yf, hp, task="regression")
    e = _engine(spec, 16, hp, p, task="regression")
    loss = e.fwd_bwd(idx.cuda(), dense.to(F32).cuda(), yf.to(F32).cuda())
    _compare(e, idx.cuda(), loss, ref, what="mse ")


def test_afm_dropout_mask_injected_into_both_sides(hip_lib):
    k = R.make_afm_case(**R.MODEL_CASES["d16"], att_dropout=0.8)
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert hp["att_dropout"] == 0.8 and bool((k["mask"] == 0).any())
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, masks={"afm": k["mask"]})
    e = _engine(spec, 16, hp, p)
    idx_d, dense_d = idx.cuda(), dense.to(F32).cuda()
    loss = e.fwd_bwd(idx_d, dense_d, y.cuda(), masks={"afm": k["mask"].to(F32).cuda()})
    _compare(e, idx_d, loss, ref, what="dropout ")
    # inference ignores the mask
    plain = R.afm_logit(p, spec, idx, dense, hp, training=False).reshape(-1)
    logit_i, _ = e.forward(idx_d, dense_d, training=False, masks={"afm": k["mask"].to(F32).cuda()})
    _close(logit_i, plain, rtol=0, atol=1e-5, what="inference logit")
    assert float((plain - ref[1]).abs().max()) > 1e-4


def test_afm_multi_valued_and_value_features(hip_lib):
    """A SparseValueFeat and a MultiValCsvFeat field: the attention consumes the value-weighted / sqrtn-pooled rows."""
    k = R.make_afm_case(**R.MODEL_CASES["d8"])
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
    # (this variant's rows differ from the plain case's: its own distance to the kinks)
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    assert float(R.afm_hidden(E, p["afm_attention_w"], p["afm_attention_b"])[1].abs().min()) >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, mv=mv)
    e = _engine(spec, 8, hp, p)
    _close(e.state_dict()["linear_w"], p["linear_w"], rtol=0, atol=0, what="linear_w round trip")
    mv_d = {vname: (torch.arange(B + 1).cuda(), vids.cuda(), vals.to(F32).cuda()), mname: (offsets.cuda(), ids.cuda())}
    loss = e.fwd_bwd(idx.cuda(), dense.to(F32).cuda(), y.cuda(), mv=mv_d)
    _compare(e, idx.cuda(), loss, ref, what="mv ")
    logit_i, _ = e.forward(idx.cuda(), dense.to(F32).cuda(), training=False, mv=mv_d)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")


def test_afm_engine_rejects_unsupported_shapes(hip_lib):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6])
    with pytest.raises(ValueError, match="not supported"):
        eng.AFMEngine(spec, 12, {})
    with pytest.raises(ValueError, match="not supported"):
        eng.AFMEngine(spec, 16, {"att_factor": 65})
    with pytest.raises(ValueError, match="not supported"):
        eng.AFMEngine(eng.FeatureSpec(["a"], [4]), 16, {})


def test_afm_sparse_step_equals_dense_step_when_reset_every_batch(hip_lib):
    """Every row touched, no l2, optimizer rebuilt per batch: the row-wise step and the dense-gradient step coincide
    (tests/test_gpu_optim.py shows it for the other models)."""
    from recman_amd.optim import Optimizer, SparseTableOptimizer

    k = R.make_afm_case(B=300, F=5, D=16, Dn=2, T=8, seed=0)
    p, spec, idx, dense, y = (k[n] for n in ("p", "spec", "idx", "dense", "y"))
    hp = dict(k["hp"], embedding_l2_reg=0.0, linear_l2_reg=0.0, att_l2_reg=0.0)
    e1, e2 = _engine(spec, 16, hp, p), _engine(spec, 16, hp, p)
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


# ------------------------------------------------------------------------------------------------ th.AFM
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
    m = th.AFM(fd, embedding_size=8, learning_rate=0.01, epoch=2, batch_size=256, random_seed=2019)
    e = m._build()
    hp = dict(m.hparams)
    assert set(hp) >= {"embedding_size", "embedding_l2_reg", "linear_l2_reg", "att_factor", "att_l2_reg",
                       "att_dropout", "learning_rate", "optimizer"}
    p0 = {k: v.cpu() for k, v in e.state_dict().items()}
    assert set(R.AFM_NAMES) <= set(p0) and float(p0["afm_attention_b"].abs().max()) == 0.0
    assert all(float(p0[n].abs().max()) > 0 for n in ("afm_attention_w", "afm_attention_h", "afm_projection_p"))
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, df["label"].values)
    idx, dense, y = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense), torch.from_numpy(inp.y)

    pred0 = m.predict(df)
    want0 = TL.prediction(R.afm_logit(p0, spec, idx, dense, hp, training=False)).numpy()
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
    want1 = TL.prediction(R.afm_logit(p, spec, idx, dense, hp, training=False)).numpy()
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
    m = th.AFM(fd, embedding_size=8, epoch=1, batch_size=256, learning_rate=0.01, eval_metric=tuple(on_dev))
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
    kw = dict(embedding_size=8, att_factor=4, epoch=2, batch_size=256, learning_rate=0.01, eval_metric=(log_loss,))
    m = th.AFM(fd, **kw)
    (tmp_path / "best").mkdir()
    finder = th.BestModelFinder(save_model=True, directory=str(tmp_path / "best"))
    tr, va = df.iloc[:768], df.iloc[768:]
    m.fit(tr, tr["label"].values, va, va["label"].values, epoch_callback=finder, random_seed_for_mini_batch=False)
    a = m.predict(df)
    path = str(tmp_path / "ckpt.pt")
    m.save(path)
    m2 = th.AFM(fd, random_seed=7, **kw)
    assert np.abs(m2.predict(df) - a).max() > 1e-4
    m2.restore(path)
    assert np.array_equal(m2.predict(df), a)
    c = clone(m)
    assert isinstance(c, th.AFM) and c.get_params()["att_factor"] == 4 and c.get_params()["l2_reg"] == 0.1
    assert c._engine is None and c.predict(df).shape == (1024,)
    assert finder.best_model is m and finder.best_score is not None
    m3 = th.BestModelFinder.load(th.AFM, str(tmp_path / "best"))
    assert m3.hparams == m.hparams
    best_valid = log_loss(va["label"].values, m3.predict(va).astype(np.float64))
    assert abs(best_valid - finder.best_score) < 1e-5


def test_fit_with_dropout_and_with_the_row_wise_optimizer(hip_lib):
    import recman_amd.th as th

    df, fd = _ml()
    yv = df["label"].values
    m = th.AFM(fd, embedding_size=8, att_dropout=0.8, epoch=3, batch_size=128, learning_rate=0.01)
    masks = m._dropout_masks(16)
    assert set(masks) == {"afm"} and masks["afm"].shape == (16, 8)
    assert set(np.unique(masks["afm"].cpu().numpy()).round(4)) <= {0.0, 1.25}
    before = log_loss(yv, m.predict(df).astype(np.float64))
    m.fit(df, yv, random_seed_for_mini_batch=False)
    after = log_loss(yv, m.predict(df).astype(np.float64))
    print(f"att_dropout 0.8: log loss {before:.4f} -> {after:.4f}")
    assert after < before
    assert np.array_equal(m.predict(df), m.predict(df))  # no dropout outside training

    s = th.AFM(fd, embedding_size=8, embedding_l2_reg=0.0, linear_l2_reg=0.0, epoch=3, batch_size=128,
               learning_rate=0.01)
    s.hparams["sparse_optimizer"] = True
    before = log_loss(yv, s.predict(df).astype(np.float64))
    s.fit(df, yv, random_seed_for_mini_batch=False)
    assert s._sparse_opt is not None and s._sparse_opt.t > 0
    after = log_loss(yv, s.predict(df).astype(np.float64))
    print(f"row-wise optimizer: log loss {before:.4f} -> {after:.4f}")
    assert after < before - 0.01


def test_row_sharded_build_is_refused(hip_lib):
    import recman_amd.th as th

    df, fd = _ml()
    m = th.AFM(fd, embedding_size=8)
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m._build()


# ---------------------------------------------------------------------------------------------- AFMLayer
def test_afm_layer_under_autograd_matches_float64(hip_lib):
    from recman_amd.th import layers as L

    k = R.gpu_case((130, 26, 16, 32))
    variables = {}
    layer = L.AFMLayer(variables, 32, att_dropout=0.8, l2_reg=1e-3)
    E = k["E"].to(F32).cuda().requires_grad_(True)
    assert layer(E).shape == (130, 1) and set(variables) == set(R.AFM_NAMES)
    assert float(variables["afm_attention_b"].detach().abs().max()) == 0.0
    assert float(variables["afm_attention_w"].detach().abs().max()) > 0
    with torch.no_grad():
        for name, key in zip(R.AFM_NAMES, ("W", "b", "h", "p_vec")):
            variables[name].copy_(k[key].to(F32).reshape(variables[name].shape).cuda())
    for use_mask in (False, True):
        for t in [E] + list(variables.values()):
            t.grad = None
        mask = k["mask"].to(F32).cuda() if use_mask else None
        out = layer(E, training=use_mask, mask=mask)
        (out.reshape(-1) * k["g"].to(F32).cuda()).sum().backward()
        want = R.layer_reference(k, use_mask, False)
        assert float((out.detach().cpu().double().reshape(-1) - want[0]).abs().max()) <= 1e-5
        assert R.grad_measure(E.grad, want[1]) <= 2e-5
        cpu32 = R.layer_reference(k, use_mask, False, dtype=F32)
        for name, w, c32 in zip(R.AFM_NAMES, want[2:], cpu32[2:]):
            got = variables[name].grad.reshape(w.shape)
            assert R.grad_measure(got, w) <= max(2e-5, 4 * R.grad_measure(c32, w)), name
    assert [id(w) for w in layer.weights] == [id(variables[n]) for n in R.AFM_NAMES]
    want_l2 = 1e-3 * 0.5 * float(k["W"].square().sum())
    assert abs(float(layer.l2().detach()) - want_l2) < 1e-6 * max(1.0, want_l2)
    # training=True without a mask draws one: multipliers 0 or 1 / keep change the logits
    assert float((layer(E, training=True) - layer(E)).detach().abs().max()) > 0


def test_afm_graph_composed_from_layers(hip_lib):
    """AFM._init_graph (AFM.py:98-143) from the layer callables: embeddings without bias use, linear + afm,
    PredictionLayer(use_bias=False), create_loss + the three l2 terms - against the restatement and the engine."""
    from recman_amd.th import DataInputs, DenseFeat, FeatureDictionary, SparseFeat
    from recman_amd.th import layers as L

    k = R.make_afm_case(**R.MODEL_CASES["odd_factor"])
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
        feat_embeds, _ = emb(inp)
        linear_feats = fd.linear_feats
        linear = L.LinearLayer(variables, linear_feats, hp["linear_l2_reg"])
        linear_logit = linear(L.LinearCombiner(linear_feats)(inp))
        afm = L.AFMLayer(variables, hp["att_factor"], hp["att_dropout"], l2_reg=hp["att_l2_reg"])
        logit = linear_logit + afm(feat_embeds)
        return L.PredictionLayer(variables, "classification", use_bias=False)(logit), logit, [emb, linear, afm]

    out()
    assert set(variables) == set(p)
    with torch.no_grad():
        for name, v in variables.items():
            v.copy_(p[name].to(F32).reshape(v.shape).cuda())
    pred, logit, layers = out()
    loss = L.create_loss(inp.y, pred) + sum(layer.l2() for layer in layers)
    loss.backward()
    loss_o, logit_o, pred_o, grads_o = R.fwd_bwd(p, spec, idx, dense, y, hp)
    _close(logit.detach().reshape(-1), logit_o, rtol=0, atol=1e-5, what="logit")
    _close(pred.detach(), pred_o, rtol=0, atol=1e-6, what="pred")
    _close(loss.detach().reshape(1), loss_o.reshape(1), what="loss")
    for name, v in variables.items():
        _close_grad(v.grad.reshape(grads_o[name].shape), grads_o[name], what=f"grad {name}")
    e = _engine(spec, hp["embedding_size"], hp, p)
    e.forward(idx.cuda(), dense.to(F32).cuda(), training=True)
    assert float((e.logit - logit.detach().reshape(-1)).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ timing
def _composed(E, W, b, h, p):
    """The comparator: the same arithmetic from torch ops in fp32 (materialises the [B, P, D] pair tensor)."""
    return R.afm_layer(E, W, b, h, p)


def _composed_chunked(E, W, b, h, p, rows=4096):
    """The comparator 4096 examples at a time (a [4096, P, D] pair tensor per piece)."""
    return torch.cat([R.afm_layer(E[s:s + rows], W, b, h, p) for s in range(0, E.shape[0], rows)])


def test_fused_kernels_are_faster_than_the_composed_torch_ops(hip_lib):
    """Sanity only: at the Criteo shape the fused afm_fwd + afm_bwd (median of 20, alternated with the comparators in
    one process) is faster than forward + autograd backward of the same arithmetic composed from torch ops - over the
    whole batch (a 1.36 GB pair tensor) and, beside it, in pieces of 4096 examples.

    The VALUES are checked against the comparator in pieces: composed over the whole batch, torch's own ops returned
    logits that are off by up to 9e-3 past the first 8192 examples on the MI355X (the fused kernel and the piecewise
    composition both agree with float64 on the CPU to 5e-9 there), so that variant is only timed."""
    from recman_amd import ops

    B, F, D, T = 65536, 26, 16, 8
    g0 = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g0)  # noqa: E731
    E, W, b, h, p, g = r(B, F, D) * 0.3, r(D, T) * 0.3, r(T) * 0.1, r(T) * 0.5, r(D) * 0.3, r(B)
    logit, st = torch.empty(B, device="cuda"), torch.empty(B, D + 2, device="cuda")
    d_rows = torch.empty(B, F, D, device="cuda")
    dW, db, dh, dp = torch.empty(D, T, device="cuda"), torch.empty(T, device="cuda"), torch.empty(
        T, device="cuda"), torch.empty(D, device="cuda")
    ws = torch.empty(ops.afm_bwd_workspace(B, F, D, T), device="cuda")
    leaves = [t.clone().requires_grad_(True) for t in (E, W, b, h, p)]

    def fused():
        ops.afm_fwd(E, W, b, h, p, logit, stats=st)
        ops.afm_bwd(E, W, b, h, p, g, logit, st, d_rows, dW, db, dh, dp, ws)

    def composed(fn=_composed):
        for t in leaves:
            t.grad = None
        fn(*leaves).backward(g)

    def chunked():
        composed(_composed_chunked)

    for _ in range(3):
        fused()
        composed()
        chunked()
    tf, tc, tk = [], [], []
    for _ in range(20):
        for fn, acc in ((fused, tf), (composed, tc), (chunked, tk)):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            acc.append(a.elapsed_time(z))
    mf, mc, mk = sorted(tf)[10], sorted(tc)[10], sorted(tk)[10]
    print(f"fused afm_fwd + afm_bwd {mf:.3f} ms; composed torch forward + backward {mc:.3f} ms (ratio {mc / mf:.2f}), "
          f"in pieces of 4096 examples {mk:.3f} ms (ratio {mk / mf:.2f})")
    # the contenders compute the same thing (gradients: tests/test_gpu_afm.py, against float64)
    assert float((logit - _composed_chunked(E, W, b, h, p)).abs().max()) < 1e-5
    assert mf < mc and mf < mk
