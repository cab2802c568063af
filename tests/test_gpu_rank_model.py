"""GPU: the ranking objectives in the engines and in fit() (hparams rank_loss, rank_group_by, rank_loss_weight,
rank_norm) against the float64 twin (tests/rank_ref.py).

Engine.fwd_bwd: loss and dlogit of deepfm (at the one-kernel-step shape, so the fallback to the multi-kernel path is
what runs), dcn, din and dlrm equal the twin evaluated at the engine's own logits; for deepfm the whole chain (the table
gradients that d_rows densifies to, every dense gradient) is held against float64 autograd of the oracle's DeepFM with
the loss swapped.  Tolerance, the convention of tests/test_gpu_asp.py: measure <= max(2e-5, 4 x the float32 CPU
restatement's own measure), both printed."""
import numpy as np
import pytest
import torch
from sklearn.utils import check_random_state

from tests import rank_ref as R
from tests import ref_common as C
from tests.cases import make_case
from tests.test_gpu_models import ml_features, ml_frame
from tests.test_gpu_parity import _engine

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
ALPHA = 0.4
SIZES = [40, 11, 5, 13, 3, 17]  # C0 is the group feature: about 40 ids


def _rank_hp(kind, by="C0", norm="group"):
    return dict(rank_loss=kind, rank_group_by=by, rank_loss_weight=ALPHA, rank_norm=norm)


def _head_twin(logit, y, groups, kind, norm, dtype):
    """(loss, dlogit) of the contract at the given logits: the pointwise head's mean log loss and its gradient, then
    the combination."""
    s = logit.detach().cpu().to(dtype)
    bce, dbce = R.bce(s, y)
    loss, d, _ = R.combine(s, y, groups, kind, norm, ALPHA, 1.0, dbce, bce.reshape(1))
    return loss.reshape(1), d


def _check_head(e, y, groups, kind, norm, tag):
    torch.cuda.synchronize()
    want, c32 = _head_twin(e.logit, y, groups, kind, norm, F64), _head_twin(e.logit, y, groups, kind, norm, F32)
    assert float(e.logit.std()) > 1e-3, f"{tag}: the logits do not vary"
    for name, got, w, c in (("loss", e.loss, want[0], c32[0]), ("dlogit", e.dlogit, want[1], c32[1])):
        m, m32 = C.grad_measure(got, w), C.grad_measure(c, w)
        bound = max(2e-5, 4 * m32)
        print(f"{tag}: {name} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        assert m <= bound, f"{tag}: {name} measure {m:.3e} > {bound:.3e}"
    assert float((e.pred - torch.sigmoid(e.logit)).abs().max()) <= 1e-6  # pred stays sigmoid(logit)


# ----------------------------------------------------------------------------------------------------------- deepfm
def _deepfm_case():
    return make_case("deepfm", B=300, F=6, D=16, Dn=3, hidden=(32, 32), sizes=SIZES, scale=0.3, dtype=F64)


@pytest.mark.parametrize("kind,norm", [("pairwise", "group"), ("listwise", "group"), ("pairwise", "pairs")])
def test_deepfm_leaves_the_one_kernel_step_and_matches_float64(hip_lib, kind, norm):
    spec, p, idx, dense, y, hp = _deepfm_case()
    hp = dict(hp, step_fusion=True)
    p32 = {k: v.to(F32) for k, v in p.items()}
    plain = _engine("deepfm", spec, 16, hp, p32)
    e = _engine("deepfm", spec, 16, dict(hp, **_rank_hp(kind, norm=norm)), p32)
    idx_d, dense_d, y_d = idx.cuda(), dense.to(F32).cuda(), y.cuda()
    plain.fwd_bwd(idx_d, dense_d, y_d)
    loss = e.fwd_bwd(idx_d, dense_d, y_d)
    assert plain._step_ok is True and plain.rank is None           # the shape the one-kernel step takes ...
    assert e._step_fused(None, None) is False and e._step_ok is None  # ... which the ranking term declines
    assert e.rank == dict(kind=kind, norm=norm, alpha=ALPHA, col=0)
    _check_head(e, y, idx[:, 0], kind, norm, f"deepfm {kind}/{norm}")
    ref = R.model_fwd_bwd("deepfm", p, spec, idx, dense, y, e.hp)
    c32 = R.model_fwd_bwd("deepfm", p32, spec, idx, dense.to(F32), y, e.hp)
    assert float((e.logit.cpu().double() - ref[1]).abs().max()) <= 1e-5
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(ref[3])
    for name, got, w, c in [("loss", loss, ref[0].reshape(1), c32[0].reshape(1))] + \
            [(k, grads[k], ref[3][k], c32[3][k]) for k in sorted(ref[3])]:
        m, m32 = C.grad_measure(got, w.reshape(got.shape)), C.grad_measure(c, w)
        bound = max(2e-5, 4 * m32)
        print(f"deepfm {kind}/{norm}: {name} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        assert m <= bound, f"{name}: measure {m:.3e} > {bound:.3e}"


def test_without_rank_loss_every_bit_is_as_before(hip_lib):
    """rank_loss=None (or the keys absent): loss and gradients bit-equal, and the one-kernel step is still taken."""
    spec, p, idx, dense, y, hp = _deepfm_case()
    hp = dict(hp, step_fusion=True)
    p32 = {k: v.to(F32) for k, v in p.items()}
    a = _engine("deepfm", spec, 16, hp, p32)
    b = _engine("deepfm", spec, 16, dict(hp, rank_loss=None, rank_group_by="C0", rank_loss_weight=0.9), p32)
    idx_d, dense_d, y_d = idx.cuda(), dense.to(F32).cuda(), y.cuda()
    la, lb = a.fwd_bwd(idx_d, dense_d, y_d), b.fwd_bwd(idx_d, dense_d, y_d)
    assert b.rank is None and b._step_ok is True and b._step_fused(None, None) is True
    assert not hasattr(b, "_rank_ws")
    assert torch.equal(la, lb) and torch.equal(a.dlogit, b.dlogit) and torch.equal(a.d_rows, b.d_rows)
    for k in a.grads:
        assert torch.equal(a.grads[k], b.grads[k]), k


# ------------------------------------------------------------------------------------------------ dcn, din and dlrm
def _random_engine(model, spec, hp, D):
    from recman_amd import engine as eng

    e = eng.ENGINES[model](spec, D, hp)
    eng.init_reference(e, 2019)
    for name, t in e.params.items():  # (zero-initialised biases and the like stay; the logits vary through the rest)
        assert bool(torch.isfinite(t).all()), name
    return e


def _batch(sizes, B, Dn, seed):
    g = torch.Generator().manual_seed(seed)
    return g, C.draw_idx(g, sizes, B), C.rnd_stream(g)(B, Dn).float(), C.draw_labels(g, B, 0.35)


@pytest.mark.parametrize("kind", R.KINDS)
def test_dcn_loss_and_dlogit_at_its_own_logits(hip_lib, kind):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec([f"C{i}" for i in range(6)], SIZES, ["I0", "I1"])
    hp = dict(embedding_size=8, deep_hidden_units=(16, 8), deep_activation="relu", cross_layer_num=2,
              **_rank_hp(kind, norm="pairs"))
    e = _random_engine("dcn", spec, hp, 8)
    _, idx, dense, y = _batch(SIZES, 400, 2, 31)
    e.fwd_bwd(idx.cuda(), dense.cuda(), y.cuda())
    _check_head(e, y, idx[:, 0], kind, "pairs", f"dcn {kind}")


@pytest.mark.parametrize("kind", R.KINDS)
def test_din_with_its_sequence_feature(hip_lib, kind):
    from recman_amd import engine as eng

    sizes = [40, 11, 0, 5]
    spec = eng.FeatureSpec(["user", "item", "hist", "C2"], sizes, ["I0", "I1"], seq_query={"hist": "item"},
                           seq_max_len={"hist": 6})
    hp = dict(embedding_size=8, deep_hidden_units=(32, 32), deep_activation="relu", att_hidden_units=(80, 40),
              att_activation="sigmoid", **_rank_hp(kind, by="user"))
    e = _random_engine("din", spec, hp, 8)
    g, idx, dense, y = _batch(sizes, 600, 2, 32)
    offsets, ids = C.draw_history(g, 600, 6, 11)
    e.fwd_bwd(idx.cuda(), dense.cuda(), y.cuda(), mv={"hist": (offsets.cuda(), ids.cuda())})
    assert e.rank["col"] == 0
    _check_head(e, y, idx[:, 0], kind, "group", f"din {kind}")
    with pytest.raises(ValueError, match="plain id feature"):
        eng.ENGINES["din"](spec, 8, dict(hp, rank_group_by="hist"))


@pytest.mark.parametrize("kind", R.KINDS)
def test_dlrm_loss_and_dlogit_at_its_own_logits(hip_lib, kind):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec([f"C{i}" for i in range(6)], SIZES, ["I0", "I1", "I2"])
    hp = dict(embedding_size=16, bottom_hidden_units=(16,), deep_hidden_units=(32, 32), deep_dropout=(1, 1, 1),
              deep_activation="relu", use_linear=True, **_rank_hp(kind))
    e = _random_engine("dlrm", spec, hp, 16)
    _, idx, dense, y = _batch(SIZES, 200, 3, 33)
    e.grad_scale = 1.0
    e.fwd_bwd(idx.cuda(), dense.cuda(), y.cuda())
    _check_head(e, y, idx[:, 0], kind, "group", f"dlrm {kind}")
    # a micro-batch share scales dlogit and leaves the loss alone
    d, loss = e.dlogit.clone(), e.loss.clone()
    e.grad_scale = 0.25
    e.fwd_bwd(idx.cuda(), dense.cuda(), y.cuda())
    assert torch.equal(e.loss, loss) and C.grad_measure(e.dlogit, 0.25 * d.double()) <= 1e-6
    e.grad_scale = 1.0


def test_an_engine_refuses_what_it_cannot_rank(hip_lib):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec([f"C{i}" for i in range(6)], SIZES, ["I0"])
    with pytest.raises(ValueError, match="needs 0/1 labels"):
        eng.DeepFMEngine(spec, 16, dict(deep_hidden_units=(32, 32), rank_loss="pairwise"), task="regression")
    with pytest.raises(ValueError, match="rank_norm='mean'"):
        eng.DeepFMEngine(spec, 16, dict(deep_hidden_units=(32, 32), rank_loss="pairwise", rank_norm="mean"))


# --------------------------------------------------------------------------------------------------------------- fit
def _model(df, epoch=2, optimizer="adam", learning_rate=0.01, **hp):
    import recman_amd.th as th

    m = th.DeepFM(ml_features(df), embedding_size=16, deep_dropout=(1, 1, 1), learning_rate=learning_rate,
                  optimizer=optimizer, eval_metric=(), epoch=epoch, batch_size=128, random_seed=2019)
    m.hparams.update(dict(rank_loss="pairwise", rank_group_by="user_id", rank_loss_weight=0.5), **hp)
    return m


def test_fit_is_the_hand_written_loop(hip_lib, monkeypatch):
    """Two epochs of fit() against fwd_bwd + optimizer steps written out.  Not bit for bit: the table gradient is
    densified with float atomics (Engine.dense_grads), so two runs of fit() itself differ in the last bits.  Plain SGD
    keeps that a rounding difference (an adaptive rule turns the sign of a cancelled gradient into a full step): 12
    steps, each gradient a few float32 ulp apart and the difference fed back through the model, stay below 1e-5 of the
    largest entry - three orders of magnitude under the distance to the pointwise model's result."""
    from recman_amd import ops

    df = ml_frame().iloc[:700]
    y = df["label"].values
    calls = []
    real = ops.rank_loss
    monkeypatch.setattr(ops, "rank_loss", lambda *a, **k: (calls.append(a[3:6]), real(*a, **k))[1])
    sgd = dict(optimizer="sgd", learning_rate=0.05)
    a = _model(df, **sgd)
    a.fit(df, y, random_seed_for_mini_batch=False)
    n_fit = len(calls)
    assert n_fit == 2 * 6 and set(calls) == {("pairwise", "group", 0.5)}  # 700 rows in batches of 128, two epochs
    b = _model(df, **sgd)
    idx, dense, yt = b._encode(df, y)
    e = b._build()
    assert e.rank == dict(kind="pairwise", norm="group", alpha=0.5, col=0) and b._sparse_opt is None
    for _ in range(2):
        perm = np.arange(700)
        check_random_state(2019).shuffle(perm)
        pt = torch.from_numpy(perm).to(idx.device)
        idx, dense, yt = idx[pt], dense[pt], yt[pt]
        for s in range(0, 700, 128):
            t = min(s + 128, 700)
            bi = idx[s:t].contiguous()
            e.fwd_bwd(bi, dense[s:t].contiguous(), yt[s:t].contiguous())
            b._opt.step(e.params, e.dense_grads(bi))
    torch.cuda.synchronize()
    sa, sb = a._engine.state_dict(), e.state_dict()
    assert set(sa) == set(sb) and len(calls) == 2 * n_fit
    worst = max(float((sa[k] - sb[k]).abs().max()) / max(1.0, float(sa[k].abs().max())) for k in sa)
    # ... and it is not the pointwise model's result
    c = _model(df, rank_loss=None, **sgd)
    c.fit(df, y, random_seed_for_mini_batch=False)
    sc = c._engine.state_dict()
    apart = max(float((sa[k] - sc[k]).abs().max()) for k in sa)
    print(f"fit() against the hand-written loop {worst:.2e}; against the pointwise model {apart:.2e}")
    assert worst <= 1e-5 and apart >= 1e-2 and len(calls) == 2 * n_fit


def test_fit_on_batch_lowers_the_combined_loss_and_save_restores(hip_lib, tmp_path):
    df = ml_frame().iloc[:256]
    y = df["label"].values
    for kind in R.KINDS:
        m = _model(df, rank_loss=kind)
        losses = [float(m.fit_on_batch(df, y)) for _ in range(20)]
        print(f"{kind}: combined loss {losses[0]:.4f} -> {losses[-1]:.4f}")
        assert np.isfinite(losses).all() and losses[-1] < losses[0]
    path = str(tmp_path / "rank.pt")
    m.save(path)
    m2 = _model(df, rank_loss="listwise")
    m2.restore(path)
    assert np.array_equal(m.predict(df), m2.predict(df))
    assert float(m2.fit_on_batch(df, y)) == float(m.fit_on_batch(df, y))  # (the loss of the forward: before the update)
    with pytest.raises(ValueError, match=r"needs labels in \{0, 1\}"):
        m.fit_on_batch(df, y * 2)
