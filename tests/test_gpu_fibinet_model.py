"""GPU: FiBiNETEngine, th.FiBiNET and th.layers.FiBiNETInteraction against the float64 restatement
(tests/fibinet_ref.py), with the rules of tests/test_gpu_parity.py: logit and inference logit 1e-5 absolute, loss
_close, every gradient _close_grad at 2e-5.  dense_gemm="f32" and the default are held to the same numbers.  Also the
DNN's first layer at the Criteo shape's width (K = 10 413) on its own: the wide dense kernels had no committed test at
a K this large."""
import numpy as np
import pytest
import torch
from sklearn.base import clone
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import fibinet_ref as R
from tests import ref_common as C
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(k, **hp_kw):
    from recman_amd import engine as eng

    spec, hp = k["spec"], dict(k["hp"], **hp_kw)
    e = eng.FiBiNETEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names), hp["embedding_size"],
                          hp)
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


@pytest.mark.parametrize("dense_gemm", ["bf16x6", "f32"])
@pytest.mark.parametrize("use_linear", [True, False])
@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_fibinet_fwd_bwd_matches_float64(hip_lib, name, use_linear, dense_gemm):
    k = R.make_case(*R.MODEL_CASES[name], use_linear=use_linear)
    B, F, D, Dn, ratio, btype = R.MODEL_CASES[name]
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert hp["interaction_l2_reg"] == 1e-4 and k["min_abs_pre"] >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp)
    e = _engine(k, dense_gemm=dense_gemm)
    assert e.use_linear == use_linear and e.btype == btype and e.R == R.reduction(F, ratio)
    idx_d, dense_d, y_d = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    what = f"{name} linear={use_linear} {dense_gemm}: "
    g1 = _compare(e, idx_d, loss, ref, what=what)
    train_logit = e.logit.clone()
    logit_i, _ = e.forward(idx_d, dense_d, training=False)
    _close(logit_i, ref[1], rtol=0, atol=1e-5, what="inference logit")
    assert torch.equal(logit_i, train_logit)  # no dropout: inference logits are the training logits' bits
    # a second fwd_bwd gives the same bits in every gradient the step computes (dense_grads' densified table and
    # linear gradients are scatter-added with float atomics afterwards: not compared)
    names = [n for n in e.grads if n.startswith(("senet_", "bilinear_w", "dnn_"))]
    first, first_rows = {n: e.grads[n].clone() for n in names}, e.d_rows.clone()
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    assert torch.equal(e.d_rows, first_rows), f"{what}d_rows differs between two runs"
    for n in names:
        assert torch.equal(e.grads[n], first[n]), f"{what}{n} differs between two runs"
    assert set(R.PARAMS) <= set(names) and g1
    # state_dict(): the contract's names and shapes, no bias tables
    sd = e.state_dict()
    assert set(sd) == set(p) and not any(n.endswith("_feat_bias") for n in sd)
    Rr, nW = R.reduction(F, ratio), R.n_matrices(F, btype)
    assert sd["senet_w1"].shape == (F, Rr) and sd["senet_w2"].shape == (Rr, F)
    assert sd["bilinear_w"].shape == (nW, D, D) and sd["senet_bilinear_w"].shape == (nW, D, D)
    assert sd["dnn_layer_0_weights"].shape == (2 * R.pairs(F) * D + Dn, 32)


def test_fibinet_deep_dropout_with_given_masks(hip_lib):
    k = R.make_case(*R.MODEL_CASES["each_d8"])
    p, spec, idx, dense, y = (k[n] for n in ("p", "spec", "idx", "dense", "y"))
    hp = dict(k["hp"], deep_dropout=(0.9, 0.8, 0.8))
    B, W = idx.shape[0], 2 * R.pairs(5) * 8 + 3
    g = torch.Generator().manual_seed(21)
    masks = [(torch.rand(B, d, generator=g) < kp).double() for d, kp in zip((W, 32, 32), hp["deep_dropout"])]
    assert all(bool((m == 0).any()) for m in masks)
    pres = R.fibinet_logit(p, spec, idx, dense, hp, masks={"dnn": masks}, return_pre=True)[1]
    assert min(float(t.abs().min()) for t in pres) >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp, masks={"dnn": masks})
    e = _engine(k, deep_dropout=hp["deep_dropout"])
    assert e.mlp.FD + e.mlp.Dn == W and len(pres) == 4
    idx_d, dense_d, y_d = _dev(k)
    md = {"dnn": [m.to(F32).cuda() for m in masks]}
    loss = e.fwd_bwd(idx_d, dense_d, y_d, masks=md)
    _compare(e, idx_d, loss, ref, what="dropout ")
    drawn = e.dropout_masks(B)
    assert [tuple(m.shape) for m in drawn["dnn"]] == [(B, W), (B, 32), (B, 32)]


def test_engine_rejects_what_it_cannot_run_and_declares_its_variables(hip_lib):
    from recman_amd import engine as eng

    hp = dict(deep_hidden_units=(8,))
    spec3 = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x"])
    with pytest.raises(ValueError, match="out of scope"):
        eng.FiBiNETEngine(spec3, 8, dict(hp, bilinear_type="interaction"))
    with pytest.raises(ValueError, match="bilinear_type"):
        eng.FiBiNETEngine(spec3, 8, dict(hp, bilinear_type="Each"))
    with pytest.raises(ValueError, match=r"not supported.*2\.\.40 embedding features, embedding_size 8/16/32"):
        eng.FiBiNETEngine(spec3, 64, hp)
    with pytest.raises(ValueError, match="not supported"):
        eng.FiBiNETEngine(eng.FeatureSpec(["a"], [4], ["x"]), 8, hp)
    with pytest.raises(ValueError, match="not supported"):
        eng.FiBiNETEngine(eng.FeatureSpec([f"f{i}" for i in range(41)], [3] * 41), 8, hp)
    with pytest.raises(ValueError, match="deep_hidden_units"):
        eng.FiBiNETEngine(spec3, 8, dict(deep_hidden_units=()))
    with pytest.raises(ValueError, match="reduction_ratio"):
        eng.FiBiNETEngine(spec3, 8, dict(hp, reduction_ratio=0))
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.FiBiNETEngine.require_shardable()
    assert eng.ENGINES["fibinet"] is eng.FiBiNETEngine
    # the defaults; init_reference follows the declared fans, the l2 key is interaction_l2_reg
    spec = eng.FeatureSpec([f"f{i}" for i in range(7)], [5] * 7, ["x", "y"])
    e1, e2 = eng.FiBiNETEngine(spec, 16, hp), eng.FiBiNETEngine(spec, 16, hp)
    assert e1.use_linear is True and e1.btype == "each" and e1.R == 2 and (e1.W, e1.ldx) == (2 * 21 * 16, 2 * 21 * 16)
    eng.init_reference(e1, 5), eng.init_reference(e2, 5)
    fans = {"senet_w1": ((7, 2), 7, 2), "senet_w2": ((2, 7), 2, 7), "bilinear_w": ((6, 16, 16), 16, 16),
            "senet_bilinear_w": ((6, 16, 16), 16, 16)}
    for n, (shape, fi, fo) in fans.items():
        std = (2.0 / (fi + fo)) ** 0.5
        v = e1.params[n]
        assert tuple(v.shape) == shape and torch.equal(v, e2.params[n]), n
        assert 0 < float(v.abs().max()) <= 2 * std + 1e-6, n
        assert e1.decl[n] == (("glorot", fi, fo), "interaction_l2_reg")
    assert e1.l2_groups["interaction_l2_reg"] == list(fans)
    assert not any(n.endswith("_feat_bias") for n in e1.params)
    assert eng.FiBiNETEngine(spec, 16, dict(hp, bilinear_type="all")).params["bilinear_w"].shape == (1, 16, 16)


def test_roofline_probes_list_the_two_kernels(hip_lib):
    k = R.make_case(*R.MODEL_CASES["each_d8"])
    e = _engine(k)
    idx_d, dense_d, y_d = _dev(k)
    probes = e.roofline_probes(idx_d, dense_d, y_d)
    assert [p["symbol"] for p in probes[:2]] == ["fibinet_bwd_kernel", "fibinet_fwd_kernel"]
    B, F, D, ldx = idx_d.shape[0], 5, 8, 160
    assert e.ldx == ldx and all(p["bound"] == "hbm" for p in probes[:2])
    assert probes[1]["work"] == 4 * B * (F * D + ldx) and probes[0]["work"] == 4 * B * (2 * F * D + ldx)
    x0, d0 = e.X.clone(), e.d_rows.clone()
    g0 = {n: e.grads[n].clone() for n in R.PARAMS}
    for p in probes:
        p["fn"]()
    torch.cuda.synchronize()
    assert torch.equal(e.X, x0) and torch.equal(e.d_rows, d0)  # the probes recompute on the step's own E and dX
    assert all(torch.equal(e.grads[n], g0[n]) for n in R.PARAMS)


# ---------------------------------------------------------------------------------------- FiBiNETInteraction
def test_interaction_layer_under_autograd_matches_float64(hip_lib):
    from recman_amd.th import layers as L

    for shape in ((37, 5, 8, 2, "each"), (33, 3, 8, 1, "all")):
        B, F, D, Rr, btype = shape
        case = R.kernel_case(*shape)
        ratio = F // Rr
        assert R.reduction(F, ratio) == Rr
        variables = {n: case[n].to(F32).cuda().requires_grad_(True) for n in R.PARAMS}
        layer = L.FiBiNETInteraction(variables, btype, ratio, l2_reg=1e-3)
        E = case["E"].to(F32).cuda().requires_grad_(True)
        X = layer(E)
        assert X.shape == (B, 2 * R.pairs(F) * D) and layer.display_name == "FiBiNETInteraction"
        (X * case["dX"].to(F32).cuda()).sum().backward()
        assert R.x_error(X, case["X"]) <= R.TOL_X
        assert R.grad_measure(E.grad, case["dE"]) <= R.TOL_GRAD
        f32 = R.f32_errors(case)
        for n, e32 in zip(R.PARAMS, f32[2:]):
            assert R.grad_measure(variables[n].grad, case["d_" + n]) <= max(R.TOL_GRAD, 4 * e32), n
        want_l2 = float(R.interaction_l2({n: case[n] for n in R.PARAMS}, 1e-3))
        assert abs(float(layer.l2().detach()) - want_l2) < 1e-5 * max(1.0, want_l2)
    # lazily made variables: names, shapes
    fresh = {}
    out = L.FiBiNETInteraction(fresh, "each", 3)(torch.randn(6, 7, 8, device="cuda"))
    assert out.shape == (6, 2 * 21 * 8) and set(fresh) == set(R.PARAMS)
    assert fresh["senet_w1"].shape == (7, 2) and fresh["bilinear_w"].shape == (6, 8, 8)
    assert not torch.equal(fresh["bilinear_w"], fresh["senet_bilinear_w"])  # two variables, two draws
    assert not torch.equal(fresh["senet_w1"].reshape(-1), fresh["senet_w2"].reshape(-1))
    assert L.FiBiNETInteraction({}, "all", 3)(torch.randn(6, 7, 8, device="cuda")).shape == (6, 2 * 21 * 8)
    with pytest.raises(ValueError, match="out of scope"):
        L.FiBiNETInteraction({}, "interaction")
    with pytest.raises(ValueError, match="unsupported"):
        L.FiBiNETInteraction({}, "each")(torch.randn(4, 3, 12, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        L.FiBiNETInteraction({}, "each")(torch.randn(4, 24, device="cuda"))


# ------------------------------------------------------------------------------------------------ th.FiBiNET
def test_model_surface_on_the_ml100k_slice(hip_lib):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    yv = df["label"].values
    kw = dict(embedding_size=8, bilinear_type="each", reduction_ratio=2, interaction_l2_reg=1e-5, epoch=2,
              batch_size=256, learning_rate=0.01)
    m = th.FiBiNET(fd, **kw)
    e = m._build()
    assert e.model == "fibinet" and e.btype == "each" and e.use_linear
    assert set(m.hparams) >= {"embedding_size", "bilinear_type", "reduction_ratio", "deep_hidden_units", "deep_dropout",
                              "interaction_l2_reg", "use_linear", "learning_rate", "optimizer"}
    p0 = {n: v.cpu() for n, v in e.state_dict().items()}
    assert all(float(p0[n].abs().max()) > 0 for n in R.PARAMS)
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, yv)
    idx, dense = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense)
    pred0 = m.predict(df)
    want0 = TL.prediction(R.fibinet_logit(p0, spec, idx, dense, m.hparams, training=False)).numpy()
    assert pred0.shape == (len(df),) and np.abs(pred0 - want0.reshape(-1)).max() < 1e-6
    before = log_loss(yv, pred0.astype(np.float64))
    assert m.fit(df, yv, random_seed_for_mini_batch=False) is None  # two epochs
    pred1 = m.predict(df)
    after = log_loss(yv, pred1.astype(np.float64))
    print(f"training log loss {before:.4f} -> {after:.4f}")
    assert pred1.shape == (len(df),) and after < before
    res = m.evaluate(df, yv)
    assert len(res) == 2 and all(np.isfinite(r) for r in res)
    # clone() round-trips the constructor arguments
    c = clone(m)
    assert isinstance(c, th.FiBiNET) and c is not m
    got = c.get_params()
    for n, v in kw.items():
        assert got[n] == v, n
    assert got["deep_hidden_units"] == (32, 32) and got["deep_dropout"] is None and got["use_linear"] is True
    assert "FiBiNET" in th.__all__


def test_constructor_errors_and_the_row_sharded_refusal(hip_lib):
    import recman_amd.th as th
    from recman_amd.th import FeatureDictionary, SparseFeat
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    with pytest.raises(ValueError, match="out of scope"):
        th.FiBiNET(fd, bilinear_type="interaction")._build()
    with pytest.raises(ValueError, match="not supported"):
        th.FiBiNET(fd, embedding_size=64)._build()
    col = fd.embedding_feats[0].name
    fd1 = FeatureDictionary()
    fd1[col] = SparseFeat(name=col, feat_size=fd.embedding_feats[0].feat_size)
    fd1.initialize(df)
    with pytest.raises(ValueError, match="not supported"):
        th.FiBiNET(fd1, embedding_size=8)._build()  # F = 1: no pair
    with pytest.raises(ValueError, match="deep_dropout"):
        th.FiBiNET(fd, deep_dropout=(0.9, 1))
    m = th.FiBiNET(fd, embedding_size=8)
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m._build()
    assert th.FiBiNET(fd, deep_dropout=(0.9, 1, 1))._dropout_masks(5)["dnn"][0].shape[0] == 5


# ------------------------------------------------------------------ the DNN's first layer at the Criteo width
_WIDE = {}


def _wide_case():
    """MLP inputs at FD = 10 400 (F = 26, D = 16: 2 P D), Dn = 13, B = 130, hidden (32, 32), with dropout masks:
    x ~ N(0,1), glorot weights, biases ~ 0.1 N(0,1), every value a float32 number; the first stream in which no unit
    lies within KINK of its kink.  Made once, with its float64 outputs."""
    if _WIDE:
        return _WIDE
    B, FD, Dn, hidden, keep = 130, 10400, 13, (32, 32), (0.9, 0.8, 0.8)
    dims = [FD + Dn] + list(hidden)

    def build(g, rnd):
        x, p = rnd(B, FD + Dn), {}
        C.draw_dnn(rnd, p, dims)
        masks = [(torch.rand(B, d, generator=g) < kp).double() for d, kp in zip(dims, keep)]
        return x, p, masks, rnd(B, std=1.0 / B)

    def clear(k):
        return C.min_abs(C.dnn_pres(k[1], k[0], 2, keep, k[2])) >= R.KINK

    (x, p, masks, gl), _ = C.first_stream(13000, build, clear, attempts=16)
    leaves = {n: v.clone().requires_grad_(True) for n, v in p.items()}
    xl = x.clone().requires_grad_(True)
    logit = TL.dnn(leaves, xl, 2, "relu", list(keep), masks).reshape(-1)
    (logit * gl).sum().backward()
    _WIDE.update(B=B, FD=FD, Dn=Dn, hidden=hidden, keep=keep, x=x, p=p, masks=masks, g=gl, logit=logit.detach(),
                 dxe=xl.grad[:, :FD], grads={n: v.grad for n, v in leaves.items()})
    return _WIDE


@pytest.mark.parametrize("dense_gemm", ["bf16x6", "f32"])
def test_mlp_first_layer_at_the_criteo_width(hip_lib, dense_gemm):
    from recman_amd import engine as eng

    c = _wide_case()
    B, FD, Dn = c["B"], c["FD"], c["Dn"]
    params, grads = {}, {}
    mlp = eng.MLP(params, grads, FD, Dn, c["hidden"], "relu", torch.device("cuda"), dense_gemm=dense_gemm)
    for n, v in c["p"].items():
        params[n].copy_(v.to(F32).reshape(params[n].shape))
    x = c["x"].to(F32).cuda()
    xe, xd = x[:, :FD].contiguous(), x[:, FD:].contiguous()
    masks = [m.to(F32).cuda() for m in c["masks"]]
    logit = mlp.forward(xe, xd, list(c["keep"]), masks)
    assert not mlp.fused  # the wide path: layer by layer on the dense kernels
    dxe = torch.full((B, FD), float("nan"), dtype=F32, device="cuda")
    mlp.backward(c["g"].to(F32).cuda(), dxe)
    torch.cuda.synchronize()
    print(f"{dense_gemm}: logit err {float((logit.cpu().double() - c['logit']).abs().max()):.2e}, dxe measure "
          f"{R.grad_measure(dxe, c['dxe']):.2e}, "
          + ", ".join(f"{n} {R.grad_measure(grads[n].reshape(c['grads'][n].shape), c['grads'][n]):.2e}" for n in grads))
    _close(logit, c["logit"], rtol=0, atol=1e-5, what="logit")
    _close_grad(dxe, c["dxe"], what="grad xe")
    for n in grads:
        _close_grad(grads[n].reshape(c["grads"][n].shape), c["grads"][n], what=f"grad {n}")
