"""GPU: FTRL-Proximal and the wide-part optimizer through the engines and the model classes.

  * SparseTableOptimizer + FusedDenseOptimizer inside a DeepFM engine at D = 8 (LD = 16, the minimal row), 32 and 64,
    adagrad + ftrl: after one fwd_bwd the stepped table equals the restatement of tests/optim_ftrl_ref.py fed the
    engine's own d_rows / dlogit (optim_ref.compare's bounds, exact zeros included); linear_w_dense moves by FTRL and
    every other dense parameter by Adagrad, every element of the flat buffer exactly once.
  * th.DeepFM and th.DCN (no FM term) with {"optimizer": "adagrad", "linear_optimizer": "ftrl", "ftrl_l1": ..,
    "linear_learning_rate": 0.05} on a few thousand synthetic rows with Zipf ids: the loss is finite and falls;
    linear_sparsity() lies strictly between 0 and 1 for an l1 at the median |z| of the first step, is 0 among the
    touched rows for l1 = 0 and 1 among them for a huge l1; untouched rows keep every column bit for bit;
    optimizer = "ftrl" alone trains and is bit-reproducible.
  * build-time refusals name the hyper-parameter in the way: FM bias dropout, strict_reference with embedding_l2_reg,
    embedding_size = 4.
  * table_sharding = "row" at world size 1 with adagrad + ftrl follows the single-GPU model within tests/test_gpu_dist.py's
    own bound for its sharded-vs-single comparison, 1e-6 max(1, max |want|).
"""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import optim_ftrl_ref as FR
from tests import optim_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------------- engines
@pytest.mark.parametrize("D", [8, 32, 64])
def test_engine_adagrad_plus_ftrl_step_equals_the_restatement(hip_lib, D):
    from recman_amd.optim import FusedDenseOptimizer, SparseTableOptimizer
    from tests.cases import make_case
    from tests.test_gpu_optim import _engine

    lr, side_lr = 0.01, 0.05
    sizes = [60, 35, 25]
    spec, p, idx, dense, y, hp = make_case("deepfm", B=512, F=3, D=D, sizes=sizes)
    hp = dict(hp, embedding_l2_reg=0.0, linear_l2_reg=0.0)
    e = _engine("deepfm", spec, D, hp, p)
    assert e.use_bias_tables and e._has_fm() and e.use_linear   # both side entries have a gradient: dlogit
    LD = e.rows.shape[1]
    assert LD >= D + 8 and (D != 8 or LD == 16)
    idx_d = idx.cuda()
    e.fwd_bwd(idx_d, dense.cuda(), y.cuda())
    # l1 at the median |z| of this very step: z = g - sigma p from z = 0, n = 0.1 (float64, from the engine's dlogit)
    rows_g = (idx + torch.tensor([0] + list(np.cumsum(sizes)[:-1]))[None, :]).reshape(-1)
    g = torch.zeros(sum(sizes), 2, dtype=F64).index_add_(
        0, rows_g, e.dlogit.detach().cpu().double().repeat_interleave(3)[:, None].expand(-1, 2))
    p_side = e.rows[: sum(sizes), D: D + 2].detach().cpu().double()
    z1 = g - ((0.1 + g * g).sqrt() - 0.1 ** 0.5) / side_lr * p_side
    touched = torch.zeros(sum(sizes), dtype=torch.bool)
    touched[rows_g] = True
    l1 = R.f32(float(z1[touched].abs().median()))

    sopt = SparseTableOptimizer(e, "adagrad", lr, side="ftrl", side_lr=side_lr, ftrl_l1=l1)
    dopt = FusedDenseOptimizer(e, "adagrad", lr, side="ftrl", side_lr=side_lr, ftrl_l1=0.0)
    Rn = e.rows.shape[0]
    assert sopt.mom.shape == (Rn, 2 * D)
    z0, n0 = sopt.moments()
    assert float(z0.abs().max()) == 0.0 and bool((n0 == 0.1).all())
    assert bool((e.rows[:, D + 2: D + 4] == 0).all()) and bool((e.rows[:, D + 4: D + 6] == 0.1).all())
    foff = e.field_off.cpu()
    case = dict(D=D, kind="adagrad", side="ftrl", side_lr=side_lr, l1=l1, ftrl_l2=0.0, ftrl_beta=0.0, entry="pairs",
                sizes=sizes, R=Rn, F=3, ld=LD, foff=foff, rows0=e.rows.detach().cpu().clone(),
                mom0=sopt.mom.detach().cpu().clone(), lr=lr, beta1=0.9, beta2=0.999, eps=1e-7, l2_emb=0.0, l2_lin=0.0,
                lin_mask=None, no_bias=False, no_lin=False, step0=1, reset_at=(), prepared_at=(),
                steps=[dict(B=512, idx=idx, d_rows=e.d_rows.detach().cpu().clone(),
                            g_bias=e.dlogit.detach().cpu().clone(), g_lin=e.dlogit.detach().cpu().clone())],
                data_key=("engine ftrl", D, LD))
    dense0 = {k: v.detach().cpu().double().clone() for k, v in e.params.items() if k in e.grads}
    grads = {k: v.detach().cpu().double().clone() for k, v in e.grads.items()}
    sopt.step(idx_d)
    dopt.step()
    torch.cuda.synchronize()

    rows, mom = e.rows.detach().cpu(), sopt.mom.detach().cpu()
    want, ref32 = FR.reference(case, F64)[0], FR.reference(case, F32)[0]
    state = FR.state_of(rows, mom, D, "adagrad", "ftrl")
    bad = FR.compare(state, want, ref32, case, tag=f"engine d{D} adagrad + ftrl")
    assert not bad, bad
    occ = R.occurrence_rows(case, 0)
    touched = torch.zeros(Rn, dtype=torch.bool)
    touched[occ] = True
    assert torch.equal(rows[~touched], case["rows0"][~touched]) and torch.equal(mom[~touched], case["mom0"][~touched])
    assert torch.equal(rows[:, D + 6:], case["rows0"][:, D + 6:])
    assert torch.equal(R.deinterleave(mom, D)[0], torch.zeros(Rn, D))   # Adagrad writes no m half
    zs, ps = want[1][touched][:, D:].abs(), state[0][touched][:, D:]
    below, above = zs <= l1 * (1 - 1e-3), zs >= l1 * (1 + 1e-3)
    assert int(below.sum()) >= 0.1 * zs.numel() and int(above.sum()) >= 0.1 * zs.numel()
    assert bool((ps[below] == 0).all()) and bool((ps[above] != 0).all())

    # the dense parameters: linear_w_dense by FTRL, everything else by Adagrad, every element once
    assert [r[2] for r in dopt.ranges].count("ftrl") == 1
    assert dopt.ranges[0][0] == 0 and dopt.ranges[-1][1] == dopt.p.numel()
    assert all(a[1] == b[0] for a, b in zip(dopt.ranges, dopt.ranges[1:]))
    for k, p0 in dense0.items():
        got = e.params[k].detach().cpu().double()
        if k == "linear_w_dense":
            w = [FR.ftrl_update(p0.to(t), torch.zeros_like(p0, dtype=t), torch.full_like(p0, R.f32(0.1), dtype=t),
                                grads[k].to(t), R.f32(side_lr), 0.0, 0.0, 0.0, False) for t in (F64, F32)]
        else:
            w = [R.update("adagrad", p0.to(t), None, torch.full_like(p0, R.f32(0.1), dtype=t), grads[k].to(t), t,
                          R.f32(lr), None, None, None, R.f32(1e-7), False) for t in (F64, F32)]
        flat = lambda x: None if x is None else x.double().reshape(1, -1)  # noqa: E731
        bad = R.compare((flat(got), None, None), (flat(w[0][0]), None, None), (flat(w[1][0]), None, None), None,
                        tag=f"engine d{D} dense {k}")
        assert not bad, (k, bad)
        assert not torch.equal(got, p0), k
        if k == "linear_w_dense":   # ... and not by the other rule: one Adagrad step lands elsewhere
            other = R.update("adagrad", p0, None, torch.full_like(p0, R.f32(0.1)), grads[k], F64, R.f32(lr), None,
                             None, None, R.f32(1e-7), False)[0]
            assert float((got - other).abs().max()) > 1e-4


# -------------------------------------------------------------------------------------------------- model classes
SIZES = (300, 120, 40)


def _frame(n=3000, seed=0):
    """Synthetic rows with Zipf ids (a few hot ids, a long tail of rare ones) and a label that depends on them."""
    rng = np.random.RandomState(seed)
    cols = {f"c{j}": np.minimum(rng.zipf(1.3, n), v) - 1 for j, v in enumerate(SIZES)}
    eff = [rng.randn(v) for v in SIZES]
    dense = rng.randn(n, 2).astype(np.float32)
    logit = sum(eff[j][cols[f"c{j}"]] for j in range(3)) * 0.8 + 0.5 * dense[:, 0] - 0.3
    df = pd.DataFrame(cols)
    df["x0"], df["x1"] = dense[:, 0], dense[:, 1]
    df["label"] = (rng.rand(n) < 1.0 / (1.0 + np.exp(-logit))).astype(np.int64)
    return df


def _features(df):
    from sklearn.preprocessing import MinMaxScaler

    from recman_amd.th import DenseFeat, FeatureDictionary, SparseFeat

    fd = FeatureDictionary()
    for j in range(3):
        fd[f"c{j}"] = SparseFeat(name=f"c{j}", feat_size=len(np.unique(df[f"c{j}"].values)))
    for c in ("x0", "x1"):
        fd[c] = DenseFeat(name=c, scaler=MinMaxScaler())
    fd.initialize(df)
    return fd


def _model(which, fd, optimizer="adagrad", extra=None, **kw):
    import recman_amd.th as th

    base = dict(embedding_size=8, embedding_l2_reg=0.0, linear_l2_reg=0.0, deep_dropout=(1, 1, 1),
                deep_hidden_units=(16, 16), learning_rate=0.05, optimizer=optimizer, batch_size=512)
    base.update(kw)
    m = (th.DeepFM if which == "deepfm" else th.DCN)(fd, **base)
    m.hparams.update(extra or {})   # (the constructors keep the reference's signature: further keys are hparams)
    return m


def _touched(m, df):
    e = m._build()
    idx, _, _ = m._encode(df)
    t = torch.zeros(e.rows.shape[0], dtype=torch.bool, device=e.rows.device)
    t[(idx + e.field_off[None, :]).reshape(-1)] = True
    return t


def _steps(m, df, k=5, B=512):
    return [float(m.fit_on_batch(df.iloc[:B], df["label"].values[:B])) for _ in range(k)]


@pytest.mark.parametrize("which", ["deepfm", "dcn"])
def test_model_with_ftrl_on_the_wide_part(hip_lib, which):
    df = _frame()
    fd = _features(df)
    batch = df.iloc[:512]
    wide = {"linear_optimizer": "ftrl", "linear_learning_rate": 0.05}

    # l1 = 0: one step; z of the linear entries (the m_l column) gives the median for the next model
    m0 = _model(which, fd, extra=dict(wide, ftrl_l1=0.0))
    e0 = m0._build()
    D = e0.D
    assert m0._sparse_opt is not None and m0._sparse_opt.side == "ftrl" and m0._sparse_opt.name == "adagrad"
    assert m0._dense_fused.side == "ftrl" and e0.rows.numel() <= (1 << 24)   # row-wise whatever the table's size
    start = e0.rows.detach().clone()
    t = _touched(m0, batch)
    _steps(m0, df, k=1)
    z = e0.rows[t][:, D + 3].abs()
    assert float(z.max()) > 0
    l1 = float(z[z > 0].median())
    _steps(m0, df, k=3)
    assert int((e0.rows[t][:, D + 1] == 0).sum()) == 0            # l1 = 0: no touched linear entry is exactly 0
    assert torch.equal(e0.rows[~t], start[~t])                    # untouched rows: every column, bit for bit
    sp0 = m0.linear_sparsity()
    assert set(sp0) == {"c0", "c1", "c2", "overall"} and all(isinstance(v, float) for v in sp0.values())
    n_rows = sum(fd[f"c{j}"].feat_size for j in range(3))
    assert abs(sp0["overall"] - float((e0.rows[:n_rows, D + 1] == 0).float().mean())) < 1e-6
    first = fd["c0"].feat_size
    assert abs(sp0["c0"] - float((e0.rows[:first, D + 1] == 0).float().mean())) < 1e-6   # slot 0 counts like any row

    m1 = _model(which, fd, extra=dict(wide, ftrl_l1=l1))
    e1 = m1._build()
    start = e1.rows.detach().clone()
    losses = _steps(m1, df, k=10)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    share = float((e1.rows[t][:, D + 1] == 0).float().mean())
    print(f"{which}: l1 {l1:.4g}, losses {losses[0]:.4f} -> {losses[-1]:.4f}, zero linear entries among touched "
          f"rows {share:.3f}, linear_sparsity {m1.linear_sparsity()}")
    assert 0.0 < share < 1.0
    assert 0.0 < m1.linear_sparsity()["overall"] < 1.0
    assert torch.equal(e1.rows[~t], start[~t])
    assert not torch.equal(e1.rows[t][:, :D], start[t][:, :D])    # the embeddings train (by Adagrad)
    if "linear_w_dense" in e1.params:
        assert float(e1.params["linear_w_dense"].abs().max()) > 0

    m2 = _model(which, fd, extra=dict(wide, ftrl_l1=1e6))
    losses = _steps(m2, df, k=3)
    assert all(np.isfinite(losses))
    assert bool((m2._engine.rows[t][:, D + 1] == 0).all())        # a huge l1: every touched linear entry is 0.0
    assert m2.linear_sparsity()["overall"] >= float(t.float().mean()) * 0.99


def test_model_with_ftrl_alone_trains_and_is_reproducible(hip_lib):
    df = _frame()
    fd = _features(df)
    runs = []
    for _ in range(2):
        m = _model("deepfm", fd, optimizer="ftrl")
        losses = _steps(m, df, k=10)
        print("ftrl alone, losses:", [round(x, 5) for x in losses])
        assert m._opt is None and m._sparse_opt.name == "ftrl" and m._dense_fused.name == "ftrl"
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, m._engine.rows.detach().clone(), m._dense_fused.p.detach().clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("extra", [{}, {"linear_optimizer": "adagrad", "linear_learning_rate": 0.02}])
def test_ftrl_under_strict_reference_rebuilds_its_state_every_batch(hip_lib, extra):
    """strict_reference (a new optimizer for every batch) with optimizer = "ftrl" and no l2 on the table: there is no
    dict-walking optimizer to reset, the fused steps take reset = True - z = 0, n = 0.1 before every update.  So the
    state after any batch is that of a first step: n = 0.1 + g^2 with no memory of earlier batches, where a persistent
    optimizer has summed every batch's g^2.  Read from the side entries' accumulators (n_b, n_l in the row: their
    gradient is a sum of dlogit, of the order of 1e-3 .. 1e-1; the embedding entries' g^2 is below float32's
    resolution at 0.1)."""
    df = _frame()
    fd = _features(df)
    m = _model("deepfm", fd, optimizer="ftrl", extra=extra, strict_reference=True)
    e = m._build()
    assert m._opt is None and m._sparse_opt is not None
    t = _touched(m, df.iloc[:512])
    losses = _steps(m, df, k=4)
    assert all(np.isfinite(losses)), losses   # (no memory from batch to batch: a falling loss is not implied)
    D = e.D
    g2 = e.rows[t][:, D + 4: D + 6] - 0.1             # what ONE step adds to a fresh accumulator
    assert float(g2.min()) >= -1e-7 and float(g2.max()) > 0
    # a persistent FTRL would have summed four steps' g^2: rebuild the same model without strict_reference
    p = _model("deepfm", fd, optimizer="ftrl", extra=extra)
    p._build()
    _steps(p, df, k=4)
    assert float((p._engine.rows[t][:, D + 4: D + 6] - 0.1).sum()) > 1.5 * float(g2.sum())
    assert bool((e.rows[~t][:, D + 4: D + 6] == 0.1).all())   # untouched rows: the initial state


def test_configurations_without_the_new_keys_build_what_they_did(hip_lib):
    df = _frame(600)
    fd = _features(df)
    m = _model("deepfm", fd, optimizer="adam")
    m._build()
    assert m._sparse_opt is None and m._opt is not None and m._opt.name == "adam"    # a small table: the dense path
    m = _model("deepfm", fd, optimizer="adam", extra={"sparse_optimizer": True})
    m._build()
    assert m._sparse_opt.side == "adam" and m._sparse_opt._rules["side_lr"] == m._sparse_opt.lr
    assert len(m._dense_fused.ranges) == 1


def test_build_refuses_what_the_row_wise_step_cannot_do(hip_lib):
    df = _frame(600)
    fd = _features(df)
    with pytest.raises(ValueError, match="fm_dropout"):
        _model("deepfm", fd, optimizer="ftrl", fm_dropout=(0.5, 1.0))._build()
    with pytest.raises(ValueError, match="fm_dropout"):
        _model("deepfm", fd, extra={"linear_optimizer": "ftrl"}, fm_dropout=(0.5, 1.0))._build()
    with pytest.raises(ValueError, match="embedding_l2_reg"):
        _model("deepfm", fd, optimizer="ftrl", embedding_l2_reg=1e-5, strict_reference=True)._build()
    with pytest.raises(ValueError, match="embedding_size"):
        _model("deepfm", fd, optimizer="ftrl", embedding_size=4)._build()
    with pytest.raises(ValueError, match="embedding_size"):
        _model("dcn", fd, extra={"linear_optimizer": "sgd"}, embedding_size=4)._build()
    with pytest.raises(ValueError, match="linear_optimizer"):
        _model("deepfm", fd, extra={"linear_optimizer": "momentum"})._build()
    # an optimizer without a row-wise step cannot carry a wide rule: refused, never stepped densely without it
    with pytest.raises(ValueError, match="optimizer='momentum'"):
        _model("deepfm", fd, optimizer="momentum", extra={"linear_optimizer": "ftrl"})._build()
    with pytest.raises(ValueError, match="optimizer='momentum'"):
        _model("deepfm", fd, optimizer="momentum", extra={"linear_learning_rate": 0.5})._build()
    with pytest.raises(ValueError, match="ftrl_l1"):
        _model("deepfm", fd, optimizer="ftrl", extra={"ftrl_l1": -1.0})._build()


def test_row_sharded_model_at_world_size_one_follows_the_single_gpu_model(hip_lib):
    df = _frame()
    fd = _features(df)
    extra = {"linear_optimizer": "ftrl", "linear_learning_rate": 0.05, "ftrl_l1": 1e-3}
    single = _model("deepfm", fd, extra=extra)
    shard = _model("deepfm", fd, extra=dict(extra, table_sharding="row"))
    e, es = single._build(), shard._build()
    D, n_rows = e.D, es.st.R
    # the same start: a shard draws its own initial rows (ShardedTable.init_reference), so it takes the single model's
    es.st.load_global(e.rows[:n_rows, :D], bias=e.rows[:n_rows, D], lin=e.rows[:n_rows, D + 1])
    for k, v in es.params.items():
        if k in e.params and k != "table_shard":
            v.copy_(e.params[k])
    for s in range(3):
        part = df.iloc[s * 400: (s + 1) * 400]
        for m in (single, shard):
            m.fit_on_batch(part, part["label"].values)
    assert shard._shard == (0, 1) and shard._shard_opt.side == "ftrl" and shard._shard_opt.dense.side == "ftrl"
    want, got = e.rows[:n_rows, : D + 2].cpu(), es.st.shard[:n_rows, : D + 2].cpu()
    err = float((got - want).abs().max())
    print(f"sharded vs single after 3 steps: {err:.3e}")
    assert err <= 1e-6 * max(1.0, float(want.abs().max()))
    assert bool(((got[:, D + 1] == 0) == (want[:, D + 1] == 0)).all())
    for k, v in e.params.items():
        if k in es.params and k in e.grads:
            w = v.detach().cpu()
            assert float((es.params[k].detach().cpu() - w).abs().max()) <= 1e-6 * max(1.0, float(w.abs().max())), k
    # per feature and overall, from the shard's row map (padding rows of the shard do not count)
    sp, sp1 = shard.linear_sparsity(), single.linear_sparsity()
    assert set(sp) == set(sp1) == {"c0", "c1", "c2", "overall"}
    assert all(abs(sp[k] - sp1[k]) < 1e-9 for k in sp), (sp, sp1)
    assert 0.0 < sp["overall"] < 1.0
