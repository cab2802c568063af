"""GPU: MMoEEngine and th.MMoE against the float64 restatement (tests/mmoe_ref.py), with the rules of
tests/test_gpu_parity.py as tests/test_gpu_pnn_model.py applies them: logits 1e-5 absolute per task, loss _close, every
dense gradient and d_rows _close_grad at 2e-5 against the float64 model."""
import numpy as np
import pytest
import torch
from sklearn.base import clone
from sklearn.metrics import log_loss, roc_auc_score

from oracle import th_layers as TL
from tests import mmoe_ref as R
from tests import seq_models_ref as SR
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(k, **hp_kw):
    from recman_amd import engine as eng

    spec, hp = k["spec"], dict(k["hp"], **hp_kw)
    e = eng.MMoEEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                       seq_query=getattr(spec, "seq_query", None),
                                       seq_max_len=getattr(spec, "seq_max_len", None)), hp["embedding_size"], hp)
    e.load_params(R.to_f32(k["p"]))
    return e


def _dev(k):
    mv = None if k["mv"] is None else {n: tuple(t.cuda() for t in ent) for n, ent in k["mv"].items()}
    return k["idx"].cuda(), k["dense"].to(F32).cuda(), k["Y"].to(F32).cuda(), mv


_REFS = {}


def _ref(name):
    if name not in _REFS:
        k = R.make_seq_case() if name == "seq" else R.make_case(*R.MODEL_CASES[name])
        _REFS[name] = (k, R.fwd_bwd(*(k[n] for n in ("p", "spec", "idx", "dense", "Y", "hp", "mv"))))
    return _REFS[name]


def _names(hp):
    n = len(hp["tower_hidden_units"])
    out = ["expert_layer_0_weights", "expert_layer_0_bias", "gate_weights"]
    for l in range(1, len(hp["expert_hidden_units"])):
        out += [f"expert_layer_{l}_weights", f"expert_layer_{l}_bias"]
    for t in hp["task_names"]:
        out += [f"{t}_dnn_w", f"{t}_dnn_w0"]
        for i in range(n):
            out += [f"{t}_dnn_layer_{i}_weights", f"{t}_dnn_layer_{i}_bias"]
    return out


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_mmoe_fwd_bwd_matches_float64(hip_lib, name):
    types, NE, units, towers, B, F, D, Dn, nan_share, _ = R.MODEL_CASES[name]
    k, ref = _ref(name)
    p, spec, idx, hp = (k[n] for n in ("p", "spec", "idx", "hp"))
    assert hp["deep_l2_reg"] == 1e-4 and k["min_abs_pre"] >= R.KINK
    e = _engine(k)
    T = len(types)
    assert (e.T, e.NE, e.H, e.use_linear) == (T, NE, units[-1], False)
    # towers of at most 32 units run the fused skinny-MLP kernels, wider ones layer by layer
    assert all(tw.fused_ok == (max(towers) <= 32) for tw in e.towers)
    idx_d, dense_d, y_d, _ = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    what = f"{name}: "
    loss_o, logit_o, pred_o, grads_o = ref
    assert e.logit.shape == (T, B)
    for t in range(T):
        print(f"{what}logit[{t}] err {float((e.logit[t].cpu().double() - logit_o[t]).abs().max()):.2e}")
        _close(e.logit[t], logit_o[t], rtol=0, atol=1e-5, what=f"{what}logit of task {t}")
        # (a regression task's prediction IS its logit)
        _close(e.pred[t], pred_o[t], rtol=0, atol=1e-6 if types[t] == "classification" else 1e-5, what=what + "pred")
    _close(loss, loss_o.reshape(1), what=what + "loss")
    assert torch.equal(e.n_t.cpu(), (~torch.isnan(k["Y"])).sum(dim=0))
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o), set(grads) ^ set(grads_o)
    for n in grads_o:
        print(f"{what}{n} measure {R.grad_measure(grads[n], grads_o[n]):.2e}")
        _close_grad(grads[n], grads_o[n], what=f"{what}grad {n}")
    want_rows = R.d_rows(p, spec, idx, k["dense"], k["Y"], hp)
    print(f"{what}d_rows measure {R.grad_measure(e.d_rows, want_rows):.2e}")
    _close_grad(e.d_rows, want_rows, what=what + "d_rows")
    # no dropout: inference logits are the training logits' bits
    train_logit = e.logit.clone()
    logit_i, pred_i = e.forward(idx_d, dense_d, training=False)
    assert torch.equal(logit_i, train_logit)
    _close(pred_i, pred_o, rtol=0, atol=1e-5, what=what + "inference pred")
    # a second fwd_bwd gives the same bits in every gradient the step computes
    names = _names(hp)
    first, first_rows = {n: e.grads[n].clone() for n in names}, e.d_rows.clone()
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    assert torch.equal(e.d_rows, first_rows), f"{what}d_rows differs between two runs"
    for n in names:
        assert torch.equal(e.grads[n], first[n]), f"{what}{n} differs between two runs"
    # the documented variable names
    sd = e.state_dict()
    assert set(sd) == set(p) == set(names) | {f"C{i}_feat_embed" for i in range(F)} | {"linear_w", "linear_w0"}
    assert tuple(sd["expert_layer_0_weights"].shape) == (F * D + Dn, NE * units[0])
    assert tuple(sd["gate_weights"].shape) == (F * D + Dn, T * NE)
    # the gate weights: the optional output of the mixture kernel
    P = e.gate_weights(idx_d, dense_d)
    _, P_o = R.mmoe_logits(p, spec, idx, k["dense"], hp)
    assert P.shape == (B, T, NE) and float((P.cpu().double() - P_o).abs().max()) <= 1e-5
    assert float((P.sum(dim=2) - 1).abs().max()) <= 1e-6
    assert torch.equal(e.logit, train_logit)  # M has the same bits with P requested


def test_sequence_feature_key_and_query_gradients(hip_lib):
    """A history feature under din pooling in front of MMoE: the pooled row's gradient leaves one column of d_rows, the
    query gradient is ADDED onto the candidate's column, the key gradients reach the item table - judged by
    tests/seq_models_ref.py:check_grads (the unit's variables keep max(2e-5, 4 x the float32 CPU measure))."""
    k, ref = _ref("seq")
    p, spec, hp = k["p"], k["spec"], k["hp"]
    assert k["min_abs_pre"] >= R.KINK
    e = _engine(k)
    idx_d, dense_d, y_d, mv_d = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
    torch.cuda.synchronize()
    loss_o, logit_o, pred_o, grads_o = ref
    for t in range(e.T):
        _close(e.logit[t], logit_o[t], rtol=0, atol=1e-5, what=f"seq: logit of task {t}")
    _close(loss, loss_o.reshape(1), what="seq: loss")
    grads = e.dense_grads(idx_d, reference_names=True)
    g32 = R.fwd_bwd(R.to_f32(p), spec, k["idx"], k["dense"].float(), k["Y"], hp, k["mv"])[3]
    SR.check_grads(k, grads, grads_o, g32, what="seq: ")
    f = spec.sparse_names.index("hist")
    fq, ids, d_keys = e.seq_key_grads(f)
    assert fq == spec.sparse_names.index("item") and torch.equal(ids.cpu(), k["mv"]["hist"][1])
    assert d_keys.shape == (ids.shape[0], e.D) and float(d_keys.abs().max()) > 0
    logit_i, _ = e.forward(idx_d, dense_d, training=False, mv=mv_d)
    for t in range(e.T):
        _close(logit_i[t], logit_o[t], rtol=0, atol=1e-5, what="seq: inference logit")
    with pytest.raises(ValueError, match="hist"):
        e.forward(idx_d, dense_d, training=False)  # the histories must be handed over


def test_engine_rejects_what_it_cannot_run_and_declares_its_variables(hip_lib):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x"])
    with pytest.raises(ValueError, match="num_experts"):
        eng.MMoEEngine(spec, 8, dict(num_experts=17))
    with pytest.raises(ValueError, match="expert_hidden_units"):
        eng.MMoEEngine(spec, 8, dict(expert_hidden_units=(64, 30)))
    with pytest.raises(ValueError, match="tower_hidden_units"):
        eng.MMoEEngine(spec, 8, dict(expert_hidden_units=(16,), tower_hidden_units=()))
    with pytest.raises(NotImplementedError, match="strict_reference"):
        eng.MMoEEngine(spec, 8, dict(expert_hidden_units=(16,), strict_reference=True))
    with pytest.raises(NotImplementedError, match="without dropout"):
        eng.MMoEEngine(spec, 8, dict(expert_hidden_units=(16,), deep_dropout=(0.9, 1, 1)))
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.MMoEEngine.require_shardable()
    e = eng.MMoEEngine(spec, 8, dict(num_experts=4, expert_hidden_units=(32, 16), tower_hidden_units=(8,),
                                     task_names=("ctr", "cvr", "like"), task_types=("classification",) * 3))
    # glorot with the fans of ONE expert or gate, deep_l2_reg on every matrix, zero biases
    assert e.decl["expert_layer_0_weights"] == (("glorot", 25, 32), "deep_l2_reg")
    assert e.decl["expert_layer_1_weights"] == (("glorot", 32, 16), "deep_l2_reg")
    assert e.decl["gate_weights"] == (("glorot", 25, 4), "deep_l2_reg")
    assert e.decl["expert_layer_1_bias"] == ("zeros", None) and e.decl["cvr_dnn_w"] == (("glorot", 8, 1), "deep_l2_reg")
    assert sorted(e.l2_groups["deep_l2_reg"]) == sorted(
        ["expert_layer_0_weights", "expert_layer_1_weights", "gate_weights"]
        + [f"{t}_dnn_{v}" for t in ("ctr", "cvr", "like") for v in ("layer_0_weights", "w")])
    eng.init_reference(e, 5)
    std = (2.0 / (25 + 4)) ** 0.5
    assert 0 < float(e.params["gate_weights"].abs().max()) <= 2 * std + 1e-6
    assert float(e.params["expert_layer_0_bias"].abs().max()) == 0.0
    assert tuple(e.params["expert_layer_1_weights"].shape) == (4, 32, 16)
    assert not any(n.endswith("_feat_bias") for n in e.params)


# --------------------------------------------------------------------------------------------------------- th.MMoE
def _ml_labels(df):
    """Two labels on the ml-100k slice: the rating label, and - observed on its positives only, as CVR on clicks -
    whether the user is older than the median."""
    y0 = df["label"].values.astype(np.float64)
    y1 = (df["age"].values > np.median(df["age"].values)).astype(np.float64)
    y1[y0 == 0] = np.nan
    return np.stack([y0, y1], axis=1)


def _oracle_fit(p, spec, idx, dense, Y, hp, batch_size, epochs, seed, lr):
    """tests/test_gpu_models.py:oracle_fit on the MMoE restatement, in float64."""
    from sklearn.utils import check_random_state

    from tests.test_gpu_models import keras_adam_cpu

    p = {k: v.clone() for k, v in p.items()}
    state, t, n = {}, 0, len(Y)
    for _ in range(epochs):
        perm = np.arange(n)
        check_random_state(seed).shuffle(perm)
        idx, dense, Y = idx[perm], dense[perm], Y[perm]
        for s in range(0, n, batch_size):
            sl = slice(s, min(n, s + batch_size))
            g = R.fwd_bwd(p, spec, idx[sl], dense[sl], Y[sl], hp)[3]
            t += 1
            keras_adam_cpu(p, g, state, t, lr)
    return p


def test_model_surface_on_the_ml100k_slice(hip_lib, tmp_path):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    Y = _ml_labels(df)
    kw = dict(task_names=("ctr", "cvr"), num_experts=4, expert_hidden_units=(32, 16), tower_hidden_units=(16,),
              embedding_size=8, deep_l2_reg=1e-5, epoch=2, batch_size=256, learning_rate=0.01,
              task_weights=(1.0, 0.5))
    m = th.MMoE(fd, **kw)
    e = m._build()
    assert e.model == "mmoe" and (e.T, e.NE, e.H) == (2, 4, 16)
    assert m.metric_names == ["ctr/roc_auc_score", "ctr/log_loss", "cvr/roc_auc_score", "cvr/log_loss"]
    p0 = {n: v.cpu().double() for n, v in e.state_dict().items()}
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, None)
    idx, dense = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense).double()
    hp = dict(m.hparams)
    pred0 = m.predict(df)
    want0 = torch.sigmoid(R.mmoe_logits(p0, spec, idx, dense, hp)[0]).t().numpy()
    assert pred0.shape == (len(df), 2) and pred0.dtype == np.float32 and np.abs(pred0 - want0).max() < 1e-6
    assert m.fit(df, Y, random_seed_for_mini_batch=False) is None  # two epochs
    p1 = _oracle_fit(p0, spec, idx, dense, torch.from_numpy(Y), hp, 256, 2, 2019, 0.01)
    pred1 = m.predict(df)
    want1 = torch.sigmoid(R.mmoe_logits(p1, spec, idx, dense, hp)[0]).t().numpy()
    print(f"MMoE: two epochs, |pred - float64 loop| {np.abs(pred1 - want1).max():.2e}")
    assert np.abs(pred1 - want1).max() < 2e-4, np.abs(pred1 - want1).max()
    assert np.abs(pred1 - pred0).max() > 1e-3  # it did train
    # evaluate: T x len(metrics) values, task-major, each metric on the task's observed rows
    res = m.evaluate(df, Y)
    seen = ~np.isnan(Y[:, 1])
    want = [roc_auc_score(Y[:, 0], pred1[:, 0]), log_loss(Y[:, 0], pred1[:, 0]),
            roc_auc_score(Y[seen, 1], pred1[seen, 1]), log_loss(Y[seen, 1], pred1[seen, 1])]
    assert 0 < seen.sum() < len(Y) and len(res) == 4 and np.allclose(res, want, rtol=0, atol=1e-12)
    # the same through the device metrics
    from recman_amd.metrics import LogLoss, RocAucScore

    md = th.MMoE(fd, eval_metric=(RocAucScore(), LogLoss()), **kw)
    assert md._metrics_on_device() and md.metric_names == ["ctr/roc_auc", "ctr/logloss", "cvr/roc_auc", "cvr/logloss"]
    path = str(tmp_path / "model")
    m.save(path)
    md.restore(path)
    assert np.array_equal(md.predict(df), pred1)  # save then restore reproduces predict bit for bit
    res_d = md.evaluate(df, Y)
    assert len(res_d) == 4 and abs(res_d[0] - want[0]) < 1e-9 and abs(res_d[2] - want[2]) < 1e-9
    assert abs(res_d[1] - want[1]) < 1e-5 and abs(res_d[3] - want[3]) < 1e-5
    # the gate weights
    gw = m.gate_weights(df)
    assert gw.shape == (len(df), 2, 4) and np.abs(gw.sum(axis=2) - 1).max() <= 1e-6 and gw.min() >= 0
    # clone() round-trips the constructor arguments
    c = clone(m)
    assert isinstance(c, th.MMoE) and c is not m
    got = c.get_params()
    for n, v in kw.items():
        assert got[n] == v, n
    assert got["task_types"] == ("classification", "classification") and got["strict_reference"] is False


def test_fit_with_validation_logs_every_task_metric(hip_lib):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    Y = _ml_labels(df)
    seen = []
    m = th.MMoE(fd, num_experts=2, expert_hidden_units=(16,), tower_hidden_units=(8,), epoch=1, batch_size=256)
    finder = th.BestModelFinder()

    def callback(**kw):
        seen.append(kw["eval_results"])
        finder(**kw)

    rows = np.random.RandomState(3).permutation(len(df))  # (the slice is ordered: both splits need both classes)
    tr_rows, va_rows = rows[:768], rows[768:]
    assert all(len(np.unique(Y[r, 1][~np.isnan(Y[r, 1])])) == 2 for r in (tr_rows, va_rows))
    m.fit(df.iloc[tr_rows], Y[tr_rows], df.iloc[va_rows], Y[va_rows], epoch_callback=callback)
    tr, va = seen[-1]
    assert len(tr) == 4 and len(va) == 4 and all(np.isfinite(r) for r in tr + va)
    assert finder.best_score == va[0] and finder.best_model is m


def test_refusals_through_the_model_surface(hip_lib):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    Y = _ml_labels(df)
    m = th.MMoE(fd, expert_hidden_units=(16,), tower_hidden_units=(8,))
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m._build()
    m = th.MMoE(fd, expert_hidden_units=(16,), tower_hidden_units=(8,))
    m.hparams["feeder"] = "pinned"
    with pytest.raises(NotImplementedError, match="pinned"):
        m.fit(df, Y)
    m = th.MMoE(fd, expert_hidden_units=(16,), tower_hidden_units=(8,))
    bad = Y.copy()
    bad[3, 0] = 2.0
    with pytest.raises(ValueError, match="classification task"):
        m.fit(df, bad)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        m.fit(df, Y[:, 0])
