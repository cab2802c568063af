"""GPU: DCNEngine with cross_type="mix", th.DCN and th.layers.CrossNetMix against the float64 restatement
(tests/crossmix_ref.py), with the rules of tests/test_gpu_parity.py: logit and inference logit 1e-5 absolute, loss
_close, every gradient _close_grad at 2e-5.  dense_gemm="f32" and the default are held to the same numbers."""
import gc

import numpy as np
import pytest
import torch
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import crossmix_ref as R
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(k, **hp_kw):
    from recman_amd import engine as eng

    spec, hp = k["spec"], dict(k["hp"], **hp_kw)
    e = eng.DCNEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names), hp["embedding_size"], hp)
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
def test_dcn_mix_fwd_bwd_matches_float64(hip_lib, name, use_linear, dense_gemm):
    k = R.make_case(*R.MODEL_CASES[name], use_linear=use_linear)
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    assert hp["cross_layer_l2_reg"] == 1e-4 and k["min_abs_pre"] >= R.KINK
    ref = R.fwd_bwd(p, spec, idx, dense, y, hp)
    e = _engine(k, dense_gemm=dense_gemm)
    assert e.mix and "cross_w" not in e.params and e.use_linear == use_linear
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
    names = [n for n in e.grads if n.startswith(("cross_", "dnn_"))]
    first, first_rows = {n: e.grads[n].clone() for n in names}, e.d_rows.clone()
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    assert torch.equal(e.d_rows, first_rows), f"{what}d_rows differs between two runs"
    for n in names:
        assert torch.equal(e.grads[n], first[n]), f"{what}{n} differs between two runs"
    assert {"cross_v", "cross_gate", "cross_c", "cross_u", "cross_b", "cross_w_out"} <= set(names) and g1
    assert set(e.state_dict()) == set(p)
    L, E, r = R.mix_dims(p)
    d = spec.F * hp["embedding_size"] + spec.Dn
    sd = e.state_dict()
    assert sd["cross_v"].shape == (L, d, E * r) and sd["cross_gate"].shape == (L, d, E)
    assert sd["cross_c"].shape == (L, E, r, r) and sd["cross_u"].shape == (L, d, E * r)


def test_one_expert_gives_a_zero_gate_gradient_without_l2(hip_lib):
    k = R.make_case(*R.MODEL_CASES["e1_r8"], l2=0.0)
    ref = R.fwd_bwd(k["p"], k["spec"], k["idx"], k["dense"], k["y"], k["hp"])
    assert float(ref[3]["cross_gate"].abs().max()) == 0.0
    e = _engine(k)
    idx_d, dense_d, y_d = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    grads = _compare(e, idx_d, loss, ref, what="E = 1: ")
    assert float(grads["cross_gate"].abs().max()) == 0.0


def test_init_reference_follows_the_declared_fans(hip_lib):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x", "y"])
    hp = dict(deep_hidden_units=(16, 8), cross_type="mix", cross_layer_num=2, cross_experts=3, cross_low_rank=16)
    e1, e2 = eng.DCNEngine(spec, 8, hp), eng.DCNEngine(spec, 8, hp)
    eng.init_reference(e1, 5), eng.init_reference(e2, 5)
    d = 26
    fans = {"cross_v": ((2, d, 48), d, 16), "cross_gate": ((2, d, 3), d, 3), "cross_c": ((2, 3, 16, 16), 16, 16),
            "cross_u": ((2, d, 48), 16, d), "cross_w_out": ((d, 1), d, 1)}
    for n, (shape, fi, fo) in fans.items():
        std = (2.0 / (fi + fo)) ** 0.5
        v = e1.params[n]
        assert tuple(v.shape) == shape and torch.equal(v, e2.params[n]), n
        assert 0.5 * std < float(v.std()) < 1.1 * std and float(v.abs().max()) <= 2 * std + 1e-6, n
        assert e1.decl[n][1] == "cross_layer_l2_reg"
    assert float(e1.params["cross_b"].abs().max()) == 0.0 and e1.decl["cross_b"][1] is None
    for bad in (dict(cross_experts=9), dict(cross_low_rank=12), dict(cross_experts=5, cross_low_rank=64)):
        with pytest.raises(ValueError, match="not supported"):
            eng.DCNEngine(spec, 8, dict(hp, **bad))
    for bad in ("tensor", "Mix", ""):
        with pytest.raises(ValueError, match="cross_type"):
            eng.DCNEngine(spec, 8, dict(hp, cross_type=bad))


def test_step_replayed_from_a_graph_equals_the_eager_one(hip_lib):
    k = R.make_case(*R.MODEL_CASES["e4_r16"])
    e = _engine(k)
    idx_d, dense_d, y_d = _dev(k)
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    names = [n for n in e.grads if n.startswith("cross_")]
    eager = {n: e.grads[n].clone() for n in names}
    eager_rows, eager_logit = e.d_rows.clone(), e.logit.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.current_stream().wait_stream(side)
    gc.collect()
    gc.disable()  # (a collection inside the capture could free device memory: unsafe there)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.fwd_bwd(idx_d, dense_d, y_d)
    finally:
        gc.enable()
    for n in names:
        e.grads[n].fill_(float("nan"))
    e.d_rows.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(e.logit, eager_logit) and torch.equal(e.d_rows, eager_rows)
    for n in names:
        assert torch.equal(e.grads[n], eager[n]), n


def test_cross_net_mix_layer_equals_the_engine(hip_lib):
    from recman_amd.th import layers as Lm

    k = R.make_case(*R.MODEL_CASES["e4_r16"], l2=0.0)
    p, spec, hp = k["p"], k["spec"], k["hp"]
    L, E, r = R.mix_dims(p)
    e = _engine(k)
    idx_d, dense_d, y_d = _dev(k)
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    variables = {n: p[n].to(F32).cuda().requires_grad_(True) for n in Lm.CrossNetMix.NAMES}
    layer = Lm.CrossNetMix(variables, L, E, r, l2_reg=1e-3)
    assert layer.display_name == "CrossNetMix" and [tuple(w.shape) for w in layer.weights] == [
        tuple(p[n].shape) for n in Lm.CrossNetMix.NAMES]
    xe = e.E.detach().clone().view(idx_d.shape[0], -1).requires_grad_(True)
    xd = dense_d.clone().requires_grad_(True)
    logit = layer(Lm.DNNCombiner()([xe, xd]))
    assert logit.shape == (idx_d.shape[0], 1) and torch.equal(logit.view(-1), e.cmix.logit)
    (logit.view(-1) * e.dlogit).sum().backward()
    for n in Lm.CrossNetMix.NAMES:
        assert torch.equal(variables[n].grad, e.grads[n]), n  # (l2 = 0: the engine's buffers hold the data gradient)
    assert torch.equal(xe.grad, e.cmix.cdx0[:, : e.FD]) and torch.equal(xd.grad, e.cmix.cdx0[:, e.FD: e.FD + e.Dn])
    want_l2 = float(R.cross_mix_l2(p, 1e-3))
    assert abs(float(layer.l2().detach()) - want_l2) < 1e-5 * max(1.0, want_l2)
    # lazily made variables: names, shapes, zero bias
    fresh = {}
    out = Lm.CrossNetMix(fresh, 2, 2, 8)(torch.randn(6, 12, device="cuda"))
    assert out.shape == (6, 1) and set(fresh) == set(Lm.CrossNetMix.NAMES)
    assert fresh["cross_v"].shape == (2, 12, 16) and fresh["cross_c"].shape == (2, 2, 8, 8)
    assert float(fresh["cross_b"].abs().max()) == 0.0 and float(fresh["cross_u"].abs().max()) > 0
    with pytest.raises(ValueError, match="unsupported"):
        Lm.CrossNetMix({}, 2, 9, 8)


def test_model_surface_on_the_ml100k_slice(hip_lib, tmp_path):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    yv = df["label"].values
    kw = dict(embedding_size=8, deep_dropout=(1, 1, 1), cross_type="mix", cross_experts=2, cross_low_rank=8,
              cross_layer_num=2, cross_layer_l2_reg=1e-5, epoch=3, batch_size=256, learning_rate=0.01)
    m = th.DCN(fd, **kw)
    e = m._build()
    assert e.model == "dcn" and e.mix and (e.cmix.E, e.cmix.r, e.cmix.L) == (2, 8, 2)
    p0 = {n: v.cpu() for n, v in e.state_dict().items()}
    assert all(float(p0[n].abs().max()) > 0 for n in ("cross_v", "cross_gate", "cross_c", "cross_u", "cross_w_out"))
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, yv)
    idx, dense = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense)
    pred0 = m.predict(df)
    want0 = TL.prediction(R.dcn_mix_logit(p0, spec, idx, dense, m.hparams, training=False)).numpy()
    assert pred0.shape == (1024,) and np.abs(pred0 - want0).max() < 1e-6
    before = log_loss(yv, pred0.astype(np.float64))
    assert m.fit(df, yv, random_seed_for_mini_batch=False) is None
    pred1 = m.predict(df)
    after = log_loss(yv, pred1.astype(np.float64))
    print(f"log loss {before:.4f} -> {after:.4f}")
    assert after < before
    path = str(tmp_path / "ckpt.pt")
    m.save(path)
    saved = torch.load(path, weights_only=True)
    assert set(saved) == set(p0) and "cross_w" not in saved
    m2 = th.DCN(fd, random_seed=7, **kw)
    assert np.abs(m2.predict(df) - pred1).max() > 1e-5
    m2.restore(path)
    assert np.array_equal(m2.predict(df), pred1)
    for bad in (dict(cross_experts=9), dict(cross_low_rank=12)):
        with pytest.raises(ValueError, match="not supported"):
            th.DCN(fd, **dict(kw, **bad))._build()
    with pytest.raises(ValueError, match="cross_type"):
        th.DCN(fd, **dict(kw, cross_type="tensor"))._build()
