"""GPU: PLEEngine, the entire-space loss in both multi-task engines, and th.PLE / th.MMoE's new arguments against the
float64 restatement (tests/ple_ref.py), with the rules of tests/test_gpu_mmoe_model.py: logits 1e-5 absolute per task,
loss _close, every dense gradient and d_rows _close_grad at 2e-5 against the float64 model."""
import numpy as np
import pytest
import torch
from sklearn.base import clone
from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score

from oracle import th_layers as TL
from tests import ple_ref as R
from tests import seq_models_ref as SR
from tests.stale_state import lds_pattern  # noqa: F401  (the fixture)
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(k, **hp_kw):
    from recman_amd import engine as eng

    spec, hp = k["spec"], dict(k["hp"], **hp_kw)
    cls = eng.ENGINES["ple" if R.is_ple(hp) else "mmoe"]
    e = cls(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                            seq_query=getattr(spec, "seq_query", None),
                            seq_max_len=getattr(spec, "seq_max_len", None)), hp["embedding_size"], hp)
    e.load_params(R.to_f32(k["p"]))
    return e


def _dev(k):
    mv = None if k["mv"] is None else {n: tuple(t.cuda() for t in ent) for n, ent in k["mv"].items()}
    return k["idx"].cuda(), k["dense"].to(F32).cuda(), k["Y"].to(F32).cuda(), mv


_REFS, _REFS32 = {}, {}


def _ref(name):
    if name not in _REFS:
        k = R.make_seq_case() if name == "seq" else R.make_case(*R.MODEL_CASES[name])
        _REFS[name] = (k, R.fwd_bwd(*(k[n] for n in ("p", "spec", "idx", "dense", "Y", "hp", "mv"))))
    return _REFS[name]


def _ref32(name):
    """The float32 CPU run of the restatement on the case: the yardstick printed beside every GPU measure."""
    if name not in _REFS32:
        k = _ref(name)[0]
        _REFS32[name] = R.fwd_bwd(R.to_f32(k["p"]), k["spec"], k["idx"], k["dense"].float(), k["Y"], k["hp"], k["mv"])
    return _REFS32[name]


def _held(what, got, want, got32):
    """The measure against float64 beside the float32 CPU restatement's own and the project's bound max(2e-5, 4 x
    that); the assertion itself is tests/test_gpu_parity.py's fixed 2e-5, which is never the looser of the two."""
    m, m32 = R.grad_measure(got, want), R.grad_measure(got32, want)
    print(f"{what}: measure {m:.2e}, float32 CPU {m32:.2e}, bound {R.bound(m32):.2e}")
    assert m <= R.bound(m32), f"{what}: {m:.3e} > {R.bound(m32):.3e}"
    _close_grad(got, want, what=what)


def _names(p):
    """The dense variables the step computes a gradient for: everything but the tables and the unused linear term."""
    return sorted(n for n in p if not n.endswith("_feat_embed") and n not in ("linear_w", "linear_w0"))


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_fwd_bwd_matches_float64(hip_lib, name):
    from recman_amd import engine as eng

    types, S, C, L, units, towers, B, F, D, Dn, nan_share, es, _ = R.MODEL_CASES[name]
    k, ref = _ref(name)
    p, spec, idx, hp = (k[n] for n in ("p", "spec", "idx", "hp"))
    assert hp["deep_l2_reg"] == 1e-4 and k["min_abs_pre"] >= R.KINK
    e = _engine(k)
    T = len(types)
    if S:
        assert type(e) is eng.PLEEngine and (e.T, e.S, e.C, e.L, e.H, e.use_linear) == (T, S, C, L, units[-1], False)
    else:
        assert type(e) is eng.MMoEEngine and e.NE == C
    assert e.es == R.es_pair(hp)
    assert all(tw.fused_ok == (max(towers) <= 32) for tw in e.towers)
    idx_d, dense_d, y_d, _ = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    what = f"{name}: "
    loss_o, logit_o, pred_o, grads_o = ref
    loss32, logit32, pred32, grads32 = _ref32(name)
    assert e.logit.shape == (T, B)
    for t in range(T):
        print(f"{what}logit[{t}] err {float((e.logit[t].cpu().double() - logit_o[t]).abs().max()):.2e}, float32 CPU "
              f"{float((logit32[t].double() - logit_o[t]).abs().max()):.2e}")
        _close(e.logit[t], logit_o[t], rtol=0, atol=1e-5, what=f"{what}logit of task {t}")
        _close(e.pred[t], pred_o[t], rtol=0, atol=1e-6 if types[t] == "classification" else 1e-5, what=what + "pred")
    _close(loss, loss_o.reshape(1), what=what + "loss")
    want_n = (~torch.isnan(k["Y"])).sum(dim=0)
    if es is not None:
        c, v = R.es_pair(hp)
        want_n[v] = int(R.es_labels(k["Y"], c, v)[1].sum())
        assert int(want_n[v]) > int((~torch.isnan(k["Y"][:, v])).sum())  # the entire space, not the clicks alone
    assert torch.equal(e.n_t.cpu(), want_n)
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o), set(grads) ^ set(grads_o)
    for n in grads_o:
        _held(f"{what}grad {n}", grads[n], grads_o[n], grads32[n])
    want_rows = R.d_rows(p, spec, idx, k["dense"], k["Y"], hp)
    rows32 = R.d_rows(R.to_f32(p), spec, idx, k["dense"].float(), k["Y"], hp)
    _held(what + "d_rows", e.d_rows, want_rows, rows32)
    # no dropout: inference logits are the training logits' bits
    train_logit = e.logit.clone()
    logit_i, pred_i = e.forward(idx_d, dense_d, training=False)
    assert torch.equal(logit_i, train_logit)
    _close(pred_i, pred_o, rtol=0, atol=1e-5, what=what + "inference pred")
    # a second fwd_bwd gives the same bits in every gradient the step computes
    names = _names(p)
    first, first_rows = {n: e.grads[n].clone() for n in names}, e.d_rows.clone()
    e.fwd_bwd(idx_d, dense_d, y_d)
    torch.cuda.synchronize()
    assert torch.equal(e.d_rows, first_rows), f"{what}d_rows differs between two runs"
    for n in names:
        assert torch.equal(e.grads[n], first[n]), f"{what}{n} differs between two runs"
    sd = e.state_dict()
    assert set(sd) == set(p)
    if not S:
        return
    # the documented variable names and shapes
    N, K0 = T * S + C, F * D + Dn
    for l in range(L):
        K = K0 if l == 0 else units[-1]
        assert tuple(sd[f"level_{l}_expert_layer_0_weights"].shape) == (K, N * units[0])
        assert tuple(sd[f"level_{l}_gate_weights"].shape) == (K, R.widths(T, S, C, l < L - 1)[1])
        for i in range(1, len(units)):
            assert tuple(sd[f"level_{l}_expert_layer_{i}_weights"].shape) == (N, units[i - 1], units[i])
    # the gate weights of every level: the optional output of the mixture kernel
    for level in list(range(L)) + [-1]:
        P = e.gate_weights(idx_d, dense_d, level=level)
        _, P_o = R.ple_logits(p, spec, idx, k["dense"], hp, level=level)
        assert P.shape == (B, T, S + C) and float((P.cpu().double() - P_o).abs().max()) <= 1e-5
        assert float((P.sum(dim=2) - 1).abs().max()) <= 1e-6
        assert torch.equal(e.logit, train_logit)  # M has the same bits with P requested


def test_sequence_feature_key_and_query_gradients(hip_lib):
    """A history feature under din pooling in front of PLE, as tests/test_gpu_mmoe_model.py has it for MMoE."""
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
    with pytest.raises(ValueError, match="hist"):
        e.forward(idx_d, dense_d, training=False)  # the histories must be handed over


def test_engine_rejects_what_it_cannot_run_and_declares_its_variables(hip_lib):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec(["a", "b", "c"], [4, 5, 6], ["x"])
    ok = dict(task_experts=2, num_experts=3, num_levels=2, expert_hidden_units=(32, 16), tower_hidden_units=(8,))
    with pytest.raises(ValueError, match="task_experts=0"):
        eng.PLEEngine(spec, 8, dict(ok, task_experts=0))
    with pytest.raises(ValueError, match="num_levels=5"):
        eng.PLEEngine(spec, 8, dict(ok, num_levels=5))
    with pytest.raises(NotImplementedError, match="strict_reference"):
        eng.PLEEngine(spec, 8, dict(ok, strict_reference=True))
    with pytest.raises(NotImplementedError, match="without dropout"):
        eng.PLEEngine(spec, 8, dict(ok, deep_dropout=(0.9, 1, 1)))
    with pytest.raises(ValueError, match="two distinct classification tasks"):
        eng.MMoEEngine(spec, 8, dict(expert_hidden_units=(16,), entire_space=("ctr", "ctr")))
    e = eng.PLEEngine(spec, 8, dict(ok, task_names=("ctr", "cvr", "like"), task_types=("classification",) * 3))
    # glorot with the fans of ONE expert or gate, deep_l2_reg on every matrix, zero biases
    assert e.decl["level_0_expert_layer_0_weights"] == (("glorot", 25, 32), "deep_l2_reg")
    assert e.decl["level_1_expert_layer_0_weights"] == (("glorot", 16, 32), "deep_l2_reg")
    assert e.decl["level_1_expert_layer_1_weights"] == (("glorot", 32, 16), "deep_l2_reg")
    assert e.decl["level_0_gate_weights"] == (("glorot", 25, 5), "deep_l2_reg")
    assert e.decl["level_1_gate_weights"] == (("glorot", 16, 5), "deep_l2_reg")
    assert e.decl["level_0_expert_layer_1_bias"] == ("zeros", None)
    assert tuple(e.params["level_0_gate_weights"].shape) == (25, 3 * 5 + 9)
    assert tuple(e.params["level_1_gate_weights"].shape) == (16, 3 * 5)
    assert sorted(e.l2_groups["deep_l2_reg"]) == sorted(
        [f"level_{l}_{v}" for l in (0, 1) for v in ("expert_layer_0_weights", "expert_layer_1_weights", "gate_weights")]
        + [f"{t}_dnn_{v}" for t in ("ctr", "cvr", "like") for v in ("layer_0_weights", "w")])
    eng.init_reference(e, 5)
    assert float(e.params["level_1_expert_layer_0_bias"].abs().max()) == 0.0
    assert 0 < float(e.params["level_1_gate_weights"].abs().max()) <= 2 * (2.0 / (16 + 5)) ** 0.5 + 1e-6


def test_default_mmoe_builds_the_mmoe_engine_and_uses_none_of_the_new_entry_points(lds_pattern):  # noqa: F811
    """A th.MMoE without the new arguments: the instance picks MMoEEngine, and an epoch of fit() goes through
    rm_mmoe_mix_* and rm_multitask_loss and through no entry point of recman_hip_multitask.h."""
    import recman_amd.th as th
    from recman_amd import _lib, engine as eng
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    m = th.MMoE(ml_features(df), epoch=1, batch_size=256)
    assert m.model == "mmoe" and (m.task_experts, m.num_levels, m.entire_space) == (0, 1, None)
    e = m._build()
    assert type(e) is eng.MMoEEngine and e.es == (-1, -1) and (e.T, e.NE, e.H) == (2, 8, 128)
    assert m.fit(df, _ml_labels(df)[:, :2]) is None
    torch.cuda.synchronize()
    seen = lds_pattern["seen"]
    assert {"rm_mmoe_mix_fwd", "rm_mmoe_mix_bwd", "rm_multitask_loss"} <= seen
    assert not seen & set(_lib.SIGNATURES_MULTITASK), seen & set(_lib.SIGNATURES_MULTITASK)
    # the same frame through th.PLE: the instance picks PLEEngine and the step the new entry points
    seen.clear()
    mp = th.PLE(ml_features(df), expert_hidden_units=(16,), tower_hidden_units=(8,), epoch=1, batch_size=256)
    assert type(mp._build()) is eng.PLEEngine and mp.fit(df, _ml_labels(df)[:, :2]) is None
    assert {"rm_cgc_mix_fwd", "rm_cgc_mix_bwd", "rm_multitask_loss"} <= seen and "rm_mmoe_mix_fwd" not in seen


# --------------------------------------------------------------------------------------------------------- th.PLE
def _ml_labels(df):
    """Three labels on the ml-100k slice: the rating label as the click; on its positives only - as CVR on clicks -
    whether the user is older than the median; and a regression label."""
    y0 = df["label"].values.astype(np.float64)
    y1 = (df["age"].values > np.median(df["age"].values)).astype(np.float64)
    y1[y0 == 0] = np.nan
    y2 = (df["age"].values - df["age"].values.mean()) / df["age"].values.std()
    return np.stack([y0, y1, y2], axis=1)


def _oracle_steps(p, spec, idx, dense, Y, hp, batch_size, seed, lr):
    """One epoch of tests/test_gpu_models.py:oracle_fit on the PLE restatement, in float64: (p, the steps taken)."""
    from sklearn.utils import check_random_state

    from tests.test_gpu_models import keras_adam_cpu

    p = {k: v.clone() for k, v in p.items()}
    state, t, n = {}, 0, len(Y)
    perm = np.arange(n)
    check_random_state(seed).shuffle(perm)
    idx, dense, Y = idx[perm], dense[perm], Y[perm]
    for s in range(0, n, batch_size):
        sl = slice(s, min(n, s + batch_size))
        g = R.fwd_bwd(p, spec, idx[sl], dense[sl], Y[sl], hp)[3]
        t += 1
        keras_adam_cpu(p, g, state, t, lr)
    return p, t


def test_model_surface_on_the_ml100k_slice(hip_lib, tmp_path):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    Y = _ml_labels(df)
    batch = (len(df) + 2) // 3  # three optimizer steps per epoch
    kw = dict(task_names=("ctr", "cvr", "age"), task_types=("classification", "classification", "regression"),
              expert_hidden_units=(32, 16), tower_hidden_units=(16,), embedding_size=8, deep_l2_reg=1e-5, epoch=1,
              batch_size=batch, learning_rate=0.01, task_weights=(1.0, 0.5, 0.25), entire_space=("ctr", "cvr"))
    m = th.PLE(fd, eval_metric=(mean_squared_error,), **kw)  # (a metric that scores the regression task too)
    e = m._build()
    assert e.model == "ple" and m.model == "ple" and (e.T, e.S, e.C, e.L, e.H, e.es) == (3, 2, 2, 2, 16, (0, 1))
    assert m.metric_names == [f"{t}/mean_squared_error" for t in ("ctr", "cvr", "age", "ctcvr")]
    p0 = {n: v.cpu().double() for n, v in e.state_dict().items()}
    spec = TL.Spec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names)
    inp = th.DataInputs().load(fd, df, None)
    idx, dense = torch.from_numpy(inp.idx), torch.from_numpy(inp.dense).double()
    hp = dict(m.hparams)
    pred0 = m.predict(df)
    logit0 = R.ple_logits(p0, spec, idx, dense, hp)[0]
    want0 = torch.stack([torch.sigmoid(logit0[0]), torch.sigmoid(logit0[1]), logit0[2]], dim=1).numpy()
    assert pred0.shape == (len(df), 3) and pred0.dtype == np.float32 and np.abs(pred0 - want0).max() < 1e-5
    # three optimizer steps equal the twin's loop
    assert m.fit(df, Y, random_seed_for_mini_batch=False) is None
    p1, steps = _oracle_steps(p0, spec, idx, dense, torch.from_numpy(Y), hp, batch, 2019, 0.01)
    assert steps == 3
    pred1 = m.predict(df)
    logit1 = R.ple_logits(p1, spec, idx, dense, hp)[0]
    want1 = torch.stack([torch.sigmoid(logit1[0]), torch.sigmoid(logit1[1]), logit1[2]], dim=1).numpy()
    print(f"PLE: three steps, |pred - float64 loop| {np.abs(pred1 - want1).max():.2e}")
    assert np.abs(pred1 - want1).max() < 2e-4, np.abs(pred1 - want1).max()
    assert np.abs(pred1 - pred0).max() > 1e-3  # it did train
    # predict_ctcvr is the product
    assert np.array_equal(m.predict_ctcvr(df), pred1[:, 0] * pred1[:, 1])
    # evaluate: the tasks' groups on their observed rows (the regression task with its own metric), then ctcvr
    mr = th.PLE(fd, eval_metric=(roc_auc_score, log_loss), **dict(kw, task_names=("ctr", "cvr"), task_types=(
        "classification", "classification"), task_weights=(1.0, 0.5)))
    mr.fit(df, Y[:, :2], random_seed_for_mini_batch=False)
    pr = mr.predict(df)
    res = mr.evaluate(df, Y[:, :2])
    seen = ~np.isnan(Y[:, 1])
    z = np.where(Y[:, 0] == 0, 0.0, Y[:, 1])  # (every click label is observed here: z is observed on every row)
    want = [roc_auc_score(Y[:, 0], pr[:, 0]), log_loss(Y[:, 0], pr[:, 0]),
            roc_auc_score(Y[seen, 1], pr[seen, 1]), log_loss(Y[seen, 1], pr[seen, 1]),
            roc_auc_score(z, pr[:, 0] * pr[:, 1]), log_loss(z, pr[:, 0] * pr[:, 1])]
    assert mr.metric_names[4:] == ["ctcvr/roc_auc_score", "ctcvr/log_loss"]
    assert len(res) == 6 and np.allclose(res, want, rtol=0, atol=1e-12)
    # the same through the device metrics, after save / restore: predict bit for bit
    from recman_amd.metrics import LogLoss, RocAucScore

    md = th.PLE(fd, eval_metric=(RocAucScore(), LogLoss()), **dict(kw, task_names=("ctr", "cvr"), task_types=(
        "classification", "classification"), task_weights=(1.0, 0.5)))
    assert md._metrics_on_device() and md.metric_names[4:] == ["ctcvr/roc_auc", "ctcvr/logloss"]
    path = str(tmp_path / "model")
    mr.save(path)
    md.restore(path)
    assert np.array_equal(md.predict(df), pr)
    res_d = md.evaluate(df, Y[:, :2])
    assert len(res_d) == 6 and all(abs(a - b) < 1e-5 for a, b in zip(res_d, want))
    # the gate weights of both levels
    for level in (0, 1, -1):
        gw = m.gate_weights(df, level=level)
        assert gw.shape == (len(df), 3, 4) and np.abs(gw.sum(axis=2) - 1).max() <= 1e-6 and gw.min() >= 0
    assert np.array_equal(m.gate_weights(df), m.gate_weights(df, level=1))
    # clone() round-trips the constructor arguments
    c = clone(m)
    assert isinstance(c, th.MMoE) and c is not m and c.model == "ple"
    got = c.get_params()
    for n, v in dict(kw, num_experts=2, task_experts=2, num_levels=2).items():
        assert got[n] == v, n


def test_fit_lowers_the_loss_and_logs_the_ctcvr_group(hip_lib):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    Y = _ml_labels(df)[:, :2]
    seen = []
    m = th.PLE(fd, expert_hidden_units=(16,), tower_hidden_units=(8,), epoch=2, batch_size=256, learning_rate=0.01,
               entire_space=("ctr", "cvr"))
    finder = th.BestModelFinder()

    def callback(**kw):
        seen.append(kw["eval_results"])
        finder(**kw)

    rows = np.random.RandomState(3).permutation(len(df))  # (the slice is ordered: both splits need both classes)
    tr_rows, va_rows = rows[:768], rows[768:]
    m.fit(df.iloc[tr_rows], Y[tr_rows], df.iloc[va_rows], Y[va_rows], epoch_callback=callback)
    assert len(seen) == 2
    (tr0, _), (tr1, va1) = seen
    assert len(tr1) == 6 and len(va1) == 6 and all(np.isfinite(r) for r in tr1 + va1)
    # log losses (ctr, cvr, ctcvr) on the training rows: lower after the second epoch
    assert tr1[1] < tr0[1] and tr1[5] < tr0[5], (tr0, tr1)
    assert finder.best_model is m


def test_refusals_through_the_model_surface(hip_lib):
    import recman_amd.th as th
    from tests.test_gpu_models import ml_features, ml_frame

    df = ml_frame()
    fd = ml_features(df)
    Y = _ml_labels(df)[:, :2]
    m = th.PLE(fd, expert_hidden_units=(16,), tower_hidden_units=(8,))
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m._build()
    m = th.PLE(fd, expert_hidden_units=(16,), tower_hidden_units=(8,))
    m.hparams["feeder"] = "pinned"
    with pytest.raises(NotImplementedError, match="pinned"):
        m.fit(df, Y)
    # NaN labels train: the conversion label is unobserved on every non-click
    m = th.PLE(fd, expert_hidden_units=(16,), tower_hidden_units=(8,), epoch=1, batch_size=256)
    assert np.isnan(Y[:, 1]).any() and m.fit(df, Y) is None and np.isfinite(m.predict(df)).all()
    with pytest.raises(ValueError, match="one level of gates"):
        th.MMoE(fd, expert_hidden_units=(16,), tower_hidden_units=(8,)).gate_weights(df, level=1)
