"""GPU: MaskNetEngine, th.MaskNet and th.layers.MaskBlock against the float64 restatement (tests/masknet_ref.py), with
the rules of tests/test_gpu_parity.py: logit 1e-5 absolute, loss _close, every gradient _close_grad at 2e-5."""
import numpy as np
import pytest
import torch
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import masknet_ref as R
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(k, spec=None, **hp_kw):
    from recman_amd import engine as eng

    spec, hp = spec or k["spec"], dict(k["hp"], **hp_kw)
    e = eng.MaskNetEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                          multi_names=spec.multi_names, value_names=spec.value_names),
                          hp["embedding_size"], hp)
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


@pytest.mark.parametrize("dense_gemm", ["f32", "bf16x6"])
@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_masknet_fwd_bwd_matches_float64(hip_lib, name, dense_gemm):
    order, N, H, ratio, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    k = R.make_case(*R.MODEL_CASES[name])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert hp["deep_l2_reg"] == 1e-4 and k["min_abs_pre"] >= R.MODEL_KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp)
    e = _engine(k, dense_gemm=dense_gemm)
    assert e.use_linear and e.parallel == (order == "parallel") and (e.N, e.H) == (N, H)
    assert e.A == [R.agg_units(ratio, w) for w in R.block_widths(hp, F * D)]
    assert e.mlp.FD == (N if order == "parallel" else 1) * H and e.mlp.Dn == Dn
    idx_d, dense_d, y_d = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    what = f"{name} {dense_gemm}: "
    _compare(e, idx_d, loss, ref, what=what)
    train_logit = e.logit.clone()
    logit_i, _ = e.forward(idx_d, dense_d, training=False)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")
    assert torch.equal(logit_i, train_logit)  # no dropout: inference logits are the training logits' bits
    # a second fwd_bwd gives the same bits in every gradient the step computes
    names = [n for n in e.grads if n.startswith(("ln_emb_", "block", "dnn_"))]
    assert len(names) == 2 + 7 * N + 2 * len(hidden) + 2
    first, first_rows = {n: e.grads[n].clone() for n in names}, e.d_rows.clone()
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    assert torch.equal(e.d_rows, first_rows), f"{what}d_rows differs between two runs"
    for n in names:
        assert torch.equal(e.grads[n], first[n]), f"{what}{n} differs between two runs"
    sd = e.state_dict()
    assert set(sd) == set(p) and not any(n.endswith("_feat_bias") for n in sd)


def test_masknet_without_the_linear_term(hip_lib):
    k = R.make_case(*R.MODEL_CASES["parallel3"], use_linear=False)
    ref = R.fwd_bwd(*(k[n] for n in ("p", "spec", "idx", "dense", "y", "hp")))
    e = _engine(k)
    assert e.use_linear is False
    idx_d, dense_d, y_d = _dev(k)
    _compare(e, idx_d, e.fwd_bwd(idx_d, dense_d, y_d), ref, what="no linear: ")


@pytest.mark.parametrize("name", ["parallel3", "serial3"])
def test_masknet_deep_dropout_with_given_masks(hip_lib, name):
    order, N, H, ratio, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    k = R.make_case(*R.MODEL_CASES[name])
    p, spec, idx, dense, y = (k[n] for n in ("p", "spec", "idx", "dense", "y"))
    hp = dict(k["hp"], deep_dropout=(0.9, 0.8, 0.8))
    W = (N if order == "parallel" else 1) * H + Dn
    g = torch.Generator().manual_seed(23)
    masks = [(torch.rand(B, d, generator=g) < kp).double() for d, kp in zip((W,) + hidden, hp["deep_dropout"])]
    assert all(bool((m == 0).any()) for m in masks)
    assert R.min_abs_pre(p, spec, idx, dense, hp, masks={"dnn": masks}) >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, masks={"dnn": masks})
    e = _engine(k, deep_dropout=hp["deep_dropout"])
    idx_d, dense_d, y_d = _dev(k)
    md = {"dnn": [m.to(F32).cuda() for m in masks]}
    loss = e.fwd_bwd(idx_d, dense_d, y_d, masks=md)
    _compare(e, idx_d, loss, ref, what=f"dropout {name} ")
    drawn = e.dropout_masks(B)
    assert [tuple(m.shape) for m in drawn["dnn"]] == [(B, W)] + [(B, h) for h in hidden]


@pytest.mark.parametrize("name", ["parallel3", "serial3"])
def test_masknet_with_a_multi_valued_feature(hip_lib, name):
    """A MultiValCsvFeat field: its sqrtn-pooled row is a row of E like any other - normalised, masked and part of
    the masks' input."""
    k = R.make_case(*R.MODEL_CASES[name])
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    B = idx.shape[0]
    mname = spec.sparse_names[3]
    spec = TL.Spec(spec.sparse_names, spec.feat_sizes, spec.dense_names, multi_names=[mname])
    g = torch.Generator().manual_seed(12)
    n = torch.randint(0, 3, (B,), generator=g)  # (an example without ids: an all-zero row of E)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    ids = torch.randint(0, spec.feat_sizes[3], (int(n.sum()),), generator=g)
    mv = {mname: (offsets, ids)}
    assert R.min_abs_pre(p, spec, idx, dense, hp, mv=mv) >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, mv=mv)
    e = _engine(k, spec=spec)
    mv_d = {mname: (offsets.cuda(), ids.cuda())}
    loss = e.fwd_bwd(idx.cuda(), dense.to(F32).cuda(), y.cuda(), mv=mv_d)
    _compare(e, idx.cuda(), loss, ref, what=f"mv {name} ")


def test_engine_rejects_what_it_cannot_run_and_declares_its_variables(hip_lib):
    from recman_amd import engine as eng

    spec3 = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x"])
    for hp, match in ((dict(block_order="diagonal"), "'parallel', 'serial'"), (dict(num_blocks=0), r"1\.\.8"),
                      (dict(num_blocks=9), r"1\.\.8"), (dict(block_hidden_units=30), "multiple of 4 in 8..2048"),
                      (dict(block_hidden_units=4096), "multiple of 4 in 8..2048"),
                      (dict(reduction_ratio=-1.0), "greater than 0"), (dict(deep_hidden_units=()), "at least one layer")):
        with pytest.raises(ValueError, match=match):
            eng.MaskNetEngine(spec3, 8, dict(dict(deep_hidden_units=(8,)), **hp))
    with pytest.raises(ValueError, match=r"not supported.*1\.\.40 embedding features, embedding_size 8/16/32"):
        eng.MaskNetEngine(spec3, 64, dict(deep_hidden_units=(8,)))
    with pytest.raises(ValueError, match="not supported"):
        eng.MaskNetEngine(eng.FeatureSpec([f"f{i}" for i in range(41)], [3] * 41), 8, dict(deep_hidden_units=(8,)))
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.MaskNetEngine.require_shardable()
    e = eng.MaskNetEngine(spec3, 8, dict(deep_hidden_units=(8,), num_blocks=2, block_hidden_units=16,
                                         block_order="serial", reduction_ratio=0.5))
    assert e.A == [12, 8] and e.wout == [24, 16]
    for t in e.params.values():
        t.fill_(7.0)
    eng.init_reference(e, 5)
    for n in ("ln_emb_gamma", "block1_ln_gamma", "block2_ln_gamma"):
        assert e.decl[n] == ("ones", None) and bool((e.params[n] == 1).all())
    for n in ("ln_emb_beta", "block1_ln_beta", "block2_agg_bias", "block1_proj_bias"):
        assert e.decl[n] == ("zeros", None) and bool((e.params[n] == 0).all())
    assert e.decl["block2_agg_weights"] == (("glorot", 25, 8), "deep_l2_reg")
    assert tuple(e.params["block2_hidden_weights"].shape) == (16, 16)
    assert tuple(e.params["block1_hidden_weights"].shape) == (24, 16)
    weights = [f"block{n}_{w}_weights" for n in (1, 2) for w in ("agg", "proj", "hidden")]
    assert set(weights) <= set(e.l2_groups["deep_l2_reg"]) and "ln_emb_gamma" not in e.l2_groups["deep_l2_reg"]
    assert all(0 < float(e.params[n].abs().max()) < 2 for n in weights)


def test_initial_model_is_the_float64_restatement(hip_lib):
    """The only init contract: with its initial parameters the engine computes what the restatement computes from the
    same parameters."""
    from recman_amd import engine as eng

    k = R.make_case(*R.MODEL_CASES["parallel3"])
    spec, idx, dense, y, hp = (k[n] for n in ("spec", "idx", "dense", "y", "hp"))
    e = eng.MaskNetEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names), 8, hp)
    eng.init_reference(e, 2019)
    p0 = {n: v.cpu().double() for n, v in e.state_dict().items()}
    assert bool((p0["ln_emb_gamma"] == 1).all()) and bool((p0["block3_ln_gamma"] == 1).all())
    logit, _ = e.forward(idx.cuda(), dense.to(F32).cuda(), training=False)
    want = R.masknet_logit(p0, spec, idx, dense, hp, training=False).reshape(-1)
    _close(logit, want, rtol=0, atol=1e-5, what="initial logit")


def test_roofline_probes_list_the_new_kernels(hip_lib):
    order, N, H, ratio, hidden, B, F, D, Dn = R.MODEL_CASES["parallel3"]
    k = R.make_case(*R.MODEL_CASES["parallel3"])
    e = _engine(k)
    idx_d, dense_d, y_d = _dev(k)
    probes = e.roofline_probes(idx_d, dense_d, y_d)
    assert [p["symbol"] for p in probes[:4]] == ["masknet_group_bwd_kernel", "masknet_group_fwd_kernel",
                                                 "masknet_row_bwd_kernel", "masknet_row_fwd_kernel"]
    assert all(p["bound"] == "hbm" for p in probes[:4])
    assert probes[1]["work"] == 4.0 * (B * F * D * (1 + 2 * N) + 2 * F * D)
    assert probes[3]["work"] == 4.0 * (2 * B * H + 2 * H)
    d0, g0, x0 = e.d_rows.clone(), e.grads["ln_emb_gamma"].clone(), e.X.clone()
    for p in probes:
        p["fn"]()
    torch.cuda.synchronize()
    # the probes recompute on the step's own buffers, into buffers of their own
    assert torch.equal(e.d_rows, d0) and torch.equal(e.grads["ln_emb_gamma"], g0) and torch.equal(e.X, x0)


# --------------------------------------------------------------------------------------------------- MaskBlock
@pytest.mark.parametrize("name", ["parallel3", "serial3"])
def test_mask_block_layer_agrees_with_the_engine(hip_lib, name):
    from recman_amd.th import layers as L

    order, N, H, ratio, hidden, B, F, D, Dn = R.MODEL_CASES[name]
    k = R.make_case(*R.MODEL_CASES[name])
    p = k["p"]
    e = _engine(k, dense_gemm="f32")
    idx_d, dense_d, y_d = _dev(k)
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    names = [n for n in p if n.startswith(("ln_emb_", "block"))]
    variables = {n: p[n].to(F32).cuda().requires_grad_(True) for n in names}
    E = e.E.clone().requires_grad_(True)
    x = torch.cat([E.view(B, F * D), dense_d], dim=1)
    blocks = [L.MaskBlock(variables, H, ratio, l2_reg=1e-4, prefix=f"block{n}_") for n in range(1, N + 1)]
    if order == "parallel":
        out = torch.cat([b(x, E) for b in blocks], dim=1)
    else:
        out = blocks[0](x, E)
        for b in blocks[1:]:
            out = b(x, out)
    # (the layer multiplies the concatenated x, the engine [xe | xd] in two pieces: the same arithmetic, other bits)
    assert R.logit_error(out, e.X) <= R.TOL_Y, "the layer's forward is the engine's"
    # the engine's dX = dLoss/d[h_1 | .. | h_N] drives the layer's backward: every block gradient, minus the l2 term
    out.backward(e.dX)
    torch.cuda.synchronize()
    for n in names:
        want = e.grads[n] - (1e-4 * e.params[n] if n.endswith("_weights") else 0.0)
        assert R.grad_measure(variables[n].grad, want) <= R.TOL_GRAD, n
    assert R.grad_measure(E.grad, e.d_rows) <= R.TOL_GRAD
    want_l2 = sum(0.5e-4 * float(p[f"block1_{w}_weights"].square().sum()) for w in ("agg", "proj", "hidden"))
    assert abs(float(blocks[0].l2().detach()) - want_l2) < 1e-6 * max(1.0, want_l2)
    assert blocks[0].display_name == "MaskBlock" and "MaskBlock" in L.__all__


def test_mask_block_makes_its_variables_and_refuses_bad_input(hip_lib):
    from recman_amd.th import layers as L

    fresh = {}
    E = torch.randn(6, 5, 8, device="cuda")
    x = torch.cat([E.view(6, 40), torch.randn(6, 3, device="cuda")], dim=1)
    h = L.MaskBlock(fresh, 16, 0.5)(x, E)
    assert h.shape == (6, 16) and bool((h >= 0).all())
    assert set(fresh) == {"ln_emb_gamma", "ln_emb_beta"} | {"block1_" + n for n in L.MaskBlock.NAMES}
    assert tuple(fresh["block1_agg_weights"].shape) == (43, 20) and bool((fresh["ln_emb_gamma"] == 1).all())
    h2 = L.MaskBlock(fresh, 8, 2.0, prefix="block2_")(x, h)
    assert h2.shape == (6, 8) and tuple(fresh["block2_proj_weights"].shape) == (32, 16)
    with pytest.raises(ValueError, match="multiple of 4"):
        L.MaskBlock({}, 30)
    with pytest.raises(ValueError, match="greater than 0"):
        L.MaskBlock({}, 16, 0.0)
    with pytest.raises(ValueError, match="unsupported"):
        L.MaskBlock({}, 16)(x, torch.randn(6, 5, 12, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        L.MaskBlock({}, 16)(x[0], E)


# -------------------------------------------------------------------------------------------------- th.MaskNet
@pytest.mark.parametrize("order", ["parallel", "serial"])
def test_model_surface_on_the_ml100k_slice(hip_lib, tmp_path, order):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    yv = df["label"].values
    kw = dict(embedding_size=8, block_order=order, num_blocks=2, block_hidden_units=16, deep_hidden_units=(16,),
              epoch=2, batch_size=256, learning_rate=0.01)
    m = th.MaskNet(fd, **kw)
    e = m._build()
    assert e.model == "masknet" and e.use_linear and e.parallel == (order == "parallel") and e.N == 2
    p0 = {n: v.cpu() for n, v in e.state_dict().items()}
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, yv)
    idx, dense = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense)
    pred0 = m.predict(df)
    # with its initial parameters the model is the restatement's (in float64, from the same values)
    p64 = {n: v.double() for n, v in p0.items()}
    want0 = TL.prediction(R.masknet_logit(p64, spec, idx, dense.double(), m.hparams, training=False)).numpy()
    assert pred0.shape == (len(df),) and np.abs(pred0 - want0.reshape(-1)).max() < 1e-5
    before = log_loss(yv, pred0.astype(np.float64))
    assert m.fit(df, yv, random_seed_for_mini_batch=False) is None  # two epochs
    pred1 = m.predict(df)
    after = log_loss(yv, pred1.astype(np.float64))
    print(f"MaskNet {order}: training log loss {before:.4f} -> {after:.4f}")
    assert pred1.shape == (len(df),) and after < before
    sd = e.state_dict()
    assert not torch.equal(sd["ln_emb_gamma"].cpu(), p0["ln_emb_gamma"])  # the gains are trained
    assert not torch.equal(sd["block2_hidden_weights"].cpu(), p0["block2_hidden_weights"])
    res = m.evaluate(df, yv)
    assert len(res) == 2 and all(np.isfinite(r) for r in res)
    # save / restore round-trips the trained model
    path = str(tmp_path / "model")
    m.save(path)
    m2 = th.MaskNet(fd, **kw)
    m2.restore(path)
    assert np.array_equal(m2.predict(df), pred1)
