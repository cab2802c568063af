"""GPU: the interest-evolution pooling unit in the engines (DIEN, and DCN / DeepFM / xDeepFM / AFM with
seq_pooling="dien") and th.DIEN against the float64 restatement (tests/dien_ref.py), in the manner and with the
tolerances of tests/test_gpu_bst_model.py.  The unit has no kink, so no seed is special.  The unit's parameter gradients
follow the kernel tests' convention: measure <= max(2e-5, 4 x the float32 CPU restatement's own measure), both printed;
every other gradient keeps the plain 2e-5."""
import functools

import numpy as np
import pytest
import torch
from sklearn.metrics import log_loss

from oracle import th_layers as TL
from tests import dien_ref as R
from tests.test_gpu_din_model import NO_DROP, _features, _frame, _inputs, _slice_mv
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, float64 step, float32 CPU step): computed once, shared and left unchanged."""
    k = R.make_model_case(**R.MODEL_CASES[name])
    ref = R.fwd_bwd(k["model"], k["p"], k["spec"], k["idx"], k["dense"], k["y"], k["hp"], k["mv"])
    g32 = R.fwd_bwd(k["model"], {n: v.to(F32) for n, v in k["p"].items()}, k["spec"], k["idx"], k["dense"].to(F32),
                    k["y"], k["hp"], k["mv"])[3]
    return k, ref, g32


def _engine(k, hp=None, task="classification"):
    from recman_amd import engine as eng

    spec = k["spec"]
    hp = dict(k["hp"] if hp is None else hp)
    e = eng.ENGINES[k["model"]](eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                                seq_query=spec.seq_query, seq_max_len=spec.seq_max_len),
                                hp["embedding_size"], hp, task=task)
    e.load_params({n: v.to(F32) for n, v in k["p"].items()})
    return e


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_fwd_bwd_matches_float64(hip_lib, name):
    k, (loss_o, logit_o, pred_o, grads_o), g32 = _case(name)
    p = k["p"]
    e = _engine(k)
    assert set(e.state_dict()) == set(p) and "hist_feat_embed" not in e.params
    assert not any("_asp_" in n or "_bst_" in n for n in e.state_dict()) and "hist_dien_att_w" in e.state_dict()
    idx_d, dense_d, y_d, mv_d = _inputs(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
    torch.cuda.synchronize()
    err = float((e.logit.cpu().double() - logit_o).abs().max())
    print(f"{name}: logit err {err:.2e}")
    _close(e.logit, logit_o, rtol=0, atol=1e-5, what="logit")
    _close(e.pred, pred_o, rtol=0, atol=1e-6, what="pred")
    _close(loss, loss_o.reshape(1), what="loss")
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o), set(grads) ^ set(grads_o)
    for n in grads_o:
        if n.startswith("hist_dien_"):
            m, m32 = R.grad_measure(grads[n], grads_o[n]), R.grad_measure(g32[n], grads_o[n])
            bound = max(2e-5, 4 * m32)
            print(f"{name}: {n} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
            assert m <= bound, f"grad {n}: measure {m:.3e} > {bound:.3e} (float32 CPU {m32:.3e})"
            continue
        _close_grad(grads[n], grads_o[n], what=f"grad {n}")
    # rows that are a candidate in one example and a history item in another: both gradients arrived
    both = sorted(set(k["idx"][:, 1].tolist()) & set(k["mv"]["hist"][1].tolist()))
    assert both and float(grads_o["item_feat_embed"][both].abs().max()) > 0
    _close_grad(grads["item_feat_embed"][both], grads_o["item_feat_embed"][both], what="candidate-and-history rows")
    # inference: same logits, nothing of the backward needed - and the pooled scratch rows of the inference pass (save
    # off) are the training pass's bit for bit
    rows_train = e.mv_scratch[0].clone()
    e.mv_scratch.fill_(float("nan"))
    logit_i, _ = e.forward(idx_d, dense_d, training=False, mv=mv_d)
    _close(logit_i, logit_o, rtol=0, atol=1e-5, what="inference logit")
    assert torch.equal(e.mv_scratch[0], rows_train) and float(rows_train[:, : e.D].abs().max()) > 0
    with pytest.raises(ValueError, match="hist"):
        e.forward(idx_d, dense_d, training=False)  # the history must be handed over


@pytest.mark.parametrize("model", ["deepfm", "xdeepfm", "afm"])
def test_every_single_gpu_engine_accepts_the_unit(hip_lib, model):
    """The pooled row is a scratch row of the base engine: compare the field's E row with the restatement."""
    from recman_amd import engine as eng

    k = _case("dien_d8")[0]
    spec, hp = k["spec"], dict(k["hp"], cin_cross_layer_units=(8, 4), att_factor=4)
    e = eng.ENGINES[model](eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                           seq_query=spec.seq_query, seq_max_len=spec.seq_max_len), 8, hp)
    eng.init_reference(e, 3)
    for n in R.NAMES:  # biases start at zero, matrices glorot
        t = e.params["hist_dien_" + n]
        assert float(t.abs().max()) == 0.0 if n.endswith("_b") else float(t.abs().min()) > 0, n
    e.load_params({n: v.to(F32) for n, v in k["p"].items() if n in e.params and ("_dien_" in n or n.endswith("_feat_embed"))})
    idx_d, dense_d, y_d, mv_d = _inputs(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
    want = R.embeddings(k["p"], spec, k["idx"], k["mv"], hp)
    assert float((e.E.cpu().double() - want).abs().max()) < 1e-5
    g = e.dense_grads(idx_d)
    assert all(bool(torch.isfinite(t).all()) for t in g.values()) and float(g["hist_dien_augru_u"].abs().max()) > 0


@pytest.mark.parametrize("pooling", [None, "transformer"])
@pytest.mark.parametrize("model", ["din", "dcn", "deepfm", "xdeepfm", "afm"])
def test_the_other_units_declare_no_dien_variable(hip_lib, model, pooling):
    from recman_amd import engine as eng

    spec = _case("dien_d8")[0]["spec"]
    hp = dict(deep_hidden_units=(8, 8), cin_cross_layer_units=(8, 4), att_factor=4)
    if pooling:
        hp["seq_pooling"] = pooling
    e = eng.ENGINES[model](eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                           seq_query=spec.seq_query, seq_max_len=spec.seq_max_len), 8, hp)
    keys = set(e.state_dict())
    assert not any("_dien_" in n for n in keys) and ("hist_bst_pos" if pooling else "hist_asp_w") in keys


@pytest.mark.parametrize("opt", ["adam", "adagrad", "sgd"])
@pytest.mark.parametrize("name", ["dien_d8", "dcn_d16"])
def test_one_row_wise_step_equals_the_dense_path_step(hip_lib, name, opt):
    """Same gradients, one step from fresh optimizer state: the row-wise step (the query feature's own occurrences and
    its history occurrences as ONE occurrence list) and the dense-gradient step coincide, also on the rows that are
    candidate and history item at once."""
    from recman_amd.optim import Optimizer, SparseTableOptimizer

    k = _case(name)[0]
    hp = dict(k["hp"], embedding_l2_reg=0.0, linear_l2_reg=0.0, deep_l2_reg=0.0, cross_layer_l2_reg=0.0)
    e1, e2 = _engine(k, hp), _engine(k, hp)
    sopt = SparseTableOptimizer(e2, opt, 0.01)
    idx_d, dense_d, y_d, mv_d = _inputs(k)
    e1.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
    before = e1.params["item_feat_embed"].clone()
    Optimizer(opt, 0.01).step(e1.params, e1.dense_grads(idx_d))
    e2.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
    sopt.step(idx_d)
    Optimizer(opt, 0.01).step(e2.params, e2.grads)
    torch.cuda.synchronize()
    for n in e1.params:
        a, b = e1.params[n], e2.params[n]
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(a.abs().max())), (opt, n)
    moved = (e1.params["item_feat_embed"] - before).abs().sum(dim=1) > 0
    both = sorted(set(k["mv"]["hist"][1].tolist()) & set(k["idx"][:, 1].tolist()))
    assert both and bool(moved[both].all())  # rows that are candidate and history item at once


# ----------------------------------------------------------------------------------------------------- th.DIEN
def _reference_inputs(th, fd, e, df):
    inp = th.DataInputs().load(fd, df, df["label"].values)
    spec = R.SeqSpec(e.spec.sparse_names, e.spec.feat_sizes, e.spec.dense_names, e.spec.seq_query)
    mv = {"hist": (torch.from_numpy(inp.mv["hist"].offsets), torch.from_numpy(inp.mv["hist"].ids))}
    return inp, spec, torch.from_numpy(inp.idx), torch.from_numpy(inp.dense), torch.from_numpy(inp.y), mv


def test_predict_and_fit_on_batch_track_the_reference_trajectory(hip_lib):
    from recman_amd.optim import Optimizer

    df = _frame()
    th, fd = _features(df)
    m = th.DIEN(fd, embedding_size=8, learning_rate=0.01, batch_size=256, **NO_DROP)
    e = m._build()
    hp = dict(m.hparams)
    p = {k: v.cpu() for k, v in e.state_dict().items()}
    for n in ("gru_w", "gru_u", "att_w", "augru_w", "augru_u"):
        assert float(p["hist_dien_" + n].abs().max()) > 0, n           # glorot from the model seed
    for n in ("gru_b", "augru_b"):
        assert float(p["hist_dien_" + n].abs().max()) == 0.0, n        # zero biases
    assert p["hist_dien_gru_w"].shape == (8, 24) and p["hist_dien_att_w"].shape == (8, 8)
    inp, spec, idx, dense, y, mv = _reference_inputs(th, fd, e, df)

    def want():
        return TL.prediction(R.model_logit("dien", p, spec, idx, dense, hp, mv, training=False)).numpy()

    pred0 = m.predict(df)
    assert pred0.shape == (len(df),) and pred0.dtype == np.float32
    assert np.abs(pred0 - want()).max() < 1e-6
    # predict equals the training forward without dropout
    assert np.array_equal(m.predict(df, training=True), pred0)
    opt = Optimizer("adam", 0.01)
    for s in (0, 200, 400):
        part = df.iloc[s:s + 200]
        m.fit_on_batch(part, part["label"].values)
        _, _, _, g = R.fwd_bwd("dien", p, spec, idx[s:s + 200], dense[s:s + 200], y[s:s + 200], hp, _slice_mv(inp, s, s + 200))
        opt.step(p, g)
    pred1 = m.predict(df)
    assert np.abs(pred1 - want()).max() < 2e-4, np.abs(pred1 - want()).max()
    assert np.abs(pred1 - pred0).max() > 1e-3  # it did train


def test_fit_with_shuffling_pinned_feeder_and_the_row_wise_optimizer(hip_lib):
    df = _frame()
    th, fd = _features(df)
    yv = df["label"].values
    kw = dict(embedding_size=8, learning_rate=0.03, epoch=6, batch_size=128)
    res = {}
    for tag, extra in (("gpu", {"feeder": "gpu"}), ("pinned", {"feeder": "pinned"}),
                       ("row-wise", {"feeder": "gpu", "sparse_optimizer": True})):
        m = th.DIEN(fd, **kw)
        m.hparams.update(extra)
        before = log_loss(yv, m.predict(df).astype(np.float64))
        assert m.fit(df, yv) is None   # a random shuffle per epoch
        after = log_loss(yv, m.predict(df).astype(np.float64))
        print(f"{tag}: log loss {before:.4f} -> {after:.4f}")
        assert after < before - 0.01, (tag, before, after)
        assert np.array_equal(m.predict(df), m.predict(df))
        res[tag] = m
    assert res["row-wise"]._sparse_opt is not None and res["row-wise"]._sparse_opt.t > 0
    # the other model classes take the unit through their hyper-parameters
    for cls in (th.DIN, th.DCN):
        d = cls(fd, embedding_size=8, learning_rate=0.03, epoch=4, batch_size=128)
        d.hparams["seq_pooling"] = "dien"
        before = log_loss(yv, d.predict(df).astype(np.float64))
        d.fit(df, yv)
        assert log_loss(yv, d.predict(df).astype(np.float64)) < before
        assert "hist_dien_att_w" in d._engine.params and "hist_asp_w" not in d._engine.params


def test_save_restore_and_clone(hip_lib, tmp_path):
    from sklearn.base import clone

    df = _frame()
    th, fd = _features(df)
    kw = dict(embedding_size=8, deep_hidden_units=(16, 8), epoch=1, batch_size=256, learning_rate=0.01)
    m = th.DIEN(fd, **kw)
    m.fit(df, df["label"].values, random_seed_for_mini_batch=False)
    a = m.predict(df)
    path = str(tmp_path / "dien.pt")
    m.save(path)
    saved = torch.load(path, weights_only=True)
    assert {"hist_dien_" + n for n in R.NAMES} <= set(saved) and saved["hist_dien_augru_u"].shape == (8, 24)
    assert "hist_feat_embed" not in saved and not any("_asp_" in n or "_bst_" in n for n in saved)
    m2 = th.DIEN(fd, random_seed=7, **kw)
    assert np.abs(m2.predict(df) - a).max() > 1e-4
    m2.restore(path)
    assert np.array_equal(m2.predict(df), a)
    c = clone(m)
    assert isinstance(c, th.DIEN) and c.get_params()["deep_hidden_units"] == (16, 8) and c._engine is None
    assert c.predict(df).shape == (len(df),)


def test_device_metrics_keep_working(hip_lib):
    from sklearn.metrics import roc_auc_score

    from recman_amd import metrics as gm

    df = _frame()
    th, fd = _features(df)
    m = th.DIEN(fd, embedding_size=8, epoch=1, batch_size=256, learning_rate=0.01,
               eval_metric=(gm.roc_auc_score, gm.log_loss))
    assert m._metrics_on_device()
    tr, va = df.iloc[:400], df.iloc[400:]
    m.fit(tr, tr["label"].values, va, va["label"].values, random_seed_for_mini_batch=False)
    res = m.evaluate(df, df["label"].values)
    pred = m.predict(df).astype(np.float64)
    assert abs(res[0] - roc_auc_score(df["label"].values, pred)) < 1e-6
    assert abs(res[1] - log_loss(df["label"].values, pred)) < 1e-5
