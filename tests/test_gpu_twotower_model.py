"""GPU: TwoTowerEngine and th.TwoTower against the float64 restatement (tests/twotower_ref.py).  Every comparison keeps
the project's bound: measure <= max(2e-5, 4 x the float32 CPU restatement's own measure on the case)."""
import itertools

import numpy as np
import pandas as pd
import pytest
import torch
from sklearn.base import clone

from tests import twotower_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
ARGS = ("p", "spec", "idx", "dense", "y", "hp", "mv")


def _engine(k, **hp_kw):
    from recman_amd import engine as eng

    spec, hp = k["spec"], dict(k["hp"], **hp_kw)
    e = eng.TwoTowerEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                           multi_names=spec.multi_names), hp["embedding_size"], hp)
    e.load_params(R.to_f32(k["p"]))
    return e


def _dev(k):
    mv = {n: tuple(t.cuda() for t in ent) for n, ent in k["mv"].items()}
    y = None if k["y"] is None else k["y"].to(F32).cuda()
    return k["idx"].cuda(), k["dense"].to(F32).cuda(), y, mv


def _check(what, got, want, f32, floor=0.0):
    """floor: a lower limit of the measure's denominators, for a gradient that is a cancelling sum (see below)."""
    m = R.grad_measure(got, want)
    if floor:
        d = (got.detach().cpu().double() - want).abs()
        m = float((d / torch.clamp(want.abs(), min=max(floor, 0.1 * float(want.abs().max())))).max())
    print(f"{what}: measure {m:.2e}, float32 CPU {f32:.2e}, bound {R.bound(f32):.2e}")
    assert m <= R.bound(f32), f"{what}: {m:.3e} > {R.bound(f32):.3e}"


def _f32_run(k):
    """The float32 CPU restatement's (loss, row_loss, rank, grads, d_rows) on case k."""
    p32, y32 = R.to_f32(k["p"]), None if k["y"] is None else k["y"].float()
    out = R.fwd_bwd(p32, k["spec"], k["idx"], k["dense"].float(), y32, k["hp"], k["mv"])
    return out + (R.d_rows(p32, k["spec"], k["idx"], k["dense"].float(), y32, k["hp"], k["mv"]),)


@pytest.mark.parametrize("normalize,masking,logq,labels", list(itertools.product((True, False), repeat=4)))
def test_fwd_bwd_matches_float64(hip_lib, normalize, masking, logq, labels):
    k = R.make_case(normalize, masking, logq, labels)
    assert k["min_abs_pre"] >= R.KINK
    loss_o, row_o, rank_o, grads_o = R.fwd_bwd(*(k[n] for n in ARGS))
    rows_o = R.d_rows(*(k[n] for n in ARGS))
    loss32, row32, _, grads32, rows32 = _f32_run(k)
    e = _engine(k)
    assert (e.H, e.use_linear, e.normalize, e.masking, e.logq_on) == (8, False, normalize, masking, logq)
    idx_d, dense_d, y_d, mv_d = _dev(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
    torch.cuda.synchronize()
    what = f"norm={normalize} mask={masking} logq={logq} labels={labels}: "
    _check(what + "loss", loss, loss_o.reshape(1), R.grad_measure(loss32, loss_o))
    _check(what + "row_loss", e.row_loss, row_o, R.grad_measure(row32, row_o))
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o) - {"item_logq"}, set(grads) ^ set(grads_o)
    # Without the row norm the softmax is invariant under a shift of every item embedding, so the item tower's last
    # bias has the gradient sum_j dV_j = 0 exactly: float64 leaves 1e-17, any float32 sum its rounding.  That sum is
    # judged against the size of its terms, 0.1 x the largest column sum of |dV_j| in float64, not against itself.
    floors = {}
    if not normalize:
        u, v, ids, lq, scale = R.model_parts(*(k[n] for n in ("p", "spec", "idx", "dense", "hp", "mv")))
        dV = R.bwd(u, v, scale, ids, lq, k["y"])[1]
        floors["item_dnn_layer_1_bias"] = 0.1 * float(dV.abs().sum(dim=0).max())
    for n in grads:
        if n in floors:
            _check(what + n, grads[n], grads_o[n], 0.0, floor=floors[n])
            continue
        _check(what + n, grads[n], grads_o[n], R.grad_measure(grads32[n], grads_o[n]))
    _check(what + "d_rows", e.d_rows, rows_o, R.grad_measure(rows32, rows_o))
    # a second fwd_bwd gives the same bits
    first = {n: e.grads[n].clone() for n in e.grads}
    first_rows = e.d_rows.clone()
    e.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
    torch.cuda.synchronize()
    assert torch.equal(e.d_rows, first_rows) and all(torch.equal(e.grads[n], first[n]) for n in first)
    # the documented variable names; item_logq is kept by state_dict() and has no gradient
    sd = e.state_dict()
    assert set(sd) == set(k["p"]) and "item_logq" not in e.grads
    assert torch.equal(sd["item_logq"].cpu(), k["p"]["item_logq"].float())


def test_engine_refusals_and_declarations(hip_lib):
    from recman_amd import engine as eng

    k = R.make_case()
    spec = eng.FeatureSpec(k["spec"].sparse_names, k["spec"].feat_sizes, k["spec"].dense_names, multi_names=["Utags"])
    with pytest.raises(NotImplementedError, match="strict_reference"):
        eng.TwoTowerEngine(spec, 8, dict(k["hp"], strict_reference=True))
    with pytest.raises(ValueError, match="same"):
        eng.TwoTowerEngine(spec, 8, dict(k["hp"], item_hidden_units=(12,)))
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.TwoTowerEngine.require_shardable()
    e = _engine(k)
    assert e.decl["user_dnn_layer_0_weights"] == (("glorot", 25, 16), "deep_l2_reg")
    assert e.decl["item_dnn_layer_1_weights"] == (("glorot", 12, 8), "deep_l2_reg")
    assert e.decl["item_dnn_layer_1_bias"] == ("zeros", None) and e.decl["item_logq"] == ("zeros", None)
    assert sorted(e.l2_groups["deep_l2_reg"]) == sorted(f"{s}_dnn_layer_{i}_weights" for s in ("user", "item")
                                                        for i in (0, 1))
    assert not any(n.endswith("_feat_bias") for n in e.params)
    idx_d, dense_d, _, mv_d = _dev(k)
    with pytest.raises(ValueError, match="float32"):
        e.fwd_bwd(idx_d, dense_d, torch.ones(37, dtype=torch.int64, device="cuda"), mv=mv_d)


# ------------------------------------------------------------------------------------------------------ th.TwoTower
def _frame(k):
    """The case as a DataFrame + FeatureDictionary whose encoding gives back the case's ids (value v of a SparseFeat
    encodes to v), and the encoded inputs of the restatement: (fd, df, idx, dense, mv)."""
    import recman_amd.th as th

    names = k["spec"].sparse_names
    fd = th.FeatureDictionary()
    cols = {}
    for j, n in enumerate(names):
        V = R.SIZES[n]
        if n == "Utags":
            fd[n] = th.MultiValCsvFeat(n, tags=tuple(str(t) for t in range(1, V)))
            off, ids = k["mv"][n]
            cols[n] = ["|".join(str(int(t)) for t in ids[off[b]: off[b + 1]]) or "none" for b in range(len(off) - 1)]
            continue
        fd[n] = th.SparseFeat(n, V - 1)
        fd[n].encoder.fit(np.arange(1, V))
        cols[n] = k["idx"][:, j].numpy()
    for j, n in enumerate(k["spec"].dense_names):
        fd[n] = th.DenseFeat(n, scaler=False)
        cols[n] = k["dense"][:, j].numpy().astype(np.float32)
    df = pd.DataFrame(cols)
    inp = th.DataInputs().load(fd, df, None)
    assert np.array_equal(inp.idx[:, [j for j, n in enumerate(names) if n != "Utags"]],
                          k["idx"][:, [j for j, n in enumerate(names) if n != "Utags"]].numpy())
    mv = {n: (torch.from_numpy(c.offsets), torch.from_numpy(c.ids)) for n, c in inp.mv.items()}
    return fd, df, torch.from_numpy(inp.idx), torch.from_numpy(inp.dense).double(), mv


def _model(k, fd, **kw):
    import recman_amd.th as th

    hp = k["hp"]
    args = dict(user_features=hp["user_features"], item_features=hp["item_features"], item_id_feature="item",
                user_hidden_units=hp["user_hidden_units"], item_hidden_units=hp["item_hidden_units"], embedding_size=8,
                temperature=hp["temperature"], normalize=hp["normalize"],
                mask_accidental_hits=hp["mask_accidental_hits"], logq_correction=hp["logq_correction"],
                deep_l2_reg=hp["deep_l2_reg"], embedding_l2_reg=hp["embedding_l2_reg"], batch_size=64)
    args.update(kw)
    m = th.TwoTower(fd, **args)
    m._build().load_params(R.to_f32(k["p"]))
    return m, args


def test_three_sgd_steps_match_float64(hip_lib):
    k = R.make_case(True, True, True, True)
    fd, df, idx, dense, mv = _frame(k)
    lr = 0.05
    m, _ = _model(k, fd, optimizer="sgd", learning_rate=lr)
    y = k["y"].numpy()
    got = [float(m.fit_on_batch(df, y)) for _ in range(3)]
    want, p_end = R.sgd_steps(k["p"], k["spec"], idx, dense, k["y"], k["hp"], lr, 3, mv)
    want32, _ = R.sgd_steps(R.to_f32(k["p"]), k["spec"], idx, dense.float(), k["y"].float(), k["hp"], lr, 3, mv)
    for s in range(3):
        f32 = abs(want32[s] - want[s]) / abs(want[s])
        err = abs(got[s] - want[s]) / abs(want[s])
        print(f"step {s}: loss {got[s]:.6f}, float64 {want[s]:.6f}, error {err:.2e}, float32 CPU {f32:.2e}")
        assert err <= R.bound(f32)
    assert want[2] < want[0]  # the steps descend
    sd = m.variables
    for n in ("user_dnn_layer_0_weights", "item_dnn_layer_1_weights", "U0_feat_embed", "item_feat_embed"):
        assert R.grad_measure(sd[n], p_end[n]) <= 1e-4, n
    assert torch.equal(sd["item_logq"].cpu(), k["p"]["item_logq"].float())  # not trained


def test_predict_embeddings_evaluate_save_restore(hip_lib, tmp_path):
    import recman_amd.th as th

    k = R.make_case(True, True, True, True)
    fd, df, idx, dense, mv = _frame(k)
    m, args = _model(k, fd, batch_size=16, recall_at=(1, 5))
    e = m._build()
    scale = 1.0 / k["hp"]["temperature"]
    pred = m.predict(df)
    ue, ie = m.user_embeddings(df), m.item_embeddings(df)
    assert pred.shape == (37,) and pred.dtype == np.float32 and ue.shape == ie.shape == (37, 8)
    want = scale * (ue.astype(np.float64) * ie.astype(np.float64)).sum(axis=1)
    assert np.abs(pred - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    u64, v64, _, _, _ = R.model_parts(k["p"], k["spec"], idx, dense, k["hp"], mv)
    assert np.abs(ue - u64.numpy()).max() <= 1e-5 and np.abs(ie - v64.numpy()).max() <= 1e-5
    # a frame with only one tower's columns gives the same bits: only that tower runs
    assert np.array_equal(m.user_embeddings(df[list(R.USER)]), ue)
    assert np.array_equal(m.item_embeddings(df[list(R.ITEM)]), ie)
    with pytest.raises(KeyError, match="user features"):
        m.user_embeddings(df[list(R.ITEM)])
    # evaluate: the kernel's outputs of the same batches (batch_size 16, frame order), weights = labels
    y = k["y"].numpy()
    res = m.evaluate(df, y)
    assert m.metric_names == ["inbatch_loss", "recall@1", "recall@5"] and len(res) == 3
    idx_d, dense_d, y_d, _ = _dev(dict(k, idx=idx, dense=dense, mv=mv))
    num = den = 0.0
    hits = [0, 0]
    want_loss = want_w = want32 = 0.0
    for s in range(0, 37, 16):
        t = min(37, s + 16)
        mvb = {"Utags": tuple(x.cuda() for x in (mv["Utags"][0][s: t + 1] - mv["Utags"][0][s],
                                                  mv["Utags"][1][mv["Utags"][0][s]: mv["Utags"][0][t]]))}
        loss, _, rank = e.evaluate_batch(idx_d[s:t].contiguous(), dense_d[s:t].contiguous(), y_d[s:t].contiguous(),
                                         mv=mvb)
        live = y[s:t] > 0
        num, den = num + float(loss) * live.sum(), den + live.sum()
        rk = rank.cpu().numpy()
        hits = [h + int((rk[live] < kk).sum()) for h, kk in zip(hits, (1, 5))]
        hp0 = dict(k["hp"], embedding_l2_reg=0.0, deep_l2_reg=0.0)
        mvh = {"Utags": tuple(x.cpu() for x in mvb["Utags"])}
        f = R.model_loss(k["p"], k["spec"], idx[s:t], dense[s:t], k["y"][s:t], hp0, mvh)[1]
        f32 = R.model_loss(R.to_f32(k["p"]), k["spec"], idx[s:t], dense[s:t].float(), k["y"][s:t].float(), hp0, mvh)[1]
        want_loss, want_w = want_loss + float(f["loss"]) * live.sum(), want_w + live.sum()
        want32 += float(f32["loss"]) * live.sum()
    assert res == [num / den, hits[0] / den, hits[1] / den]
    want_loss, want32 = want_loss / want_w, want32 / want_w
    assert abs(res[0] - want_loss) / abs(want_loss) <= R.bound(abs(want32 - want_loss) / abs(want_loss))
    assert 0.0 <= res[1] <= res[2] <= 1.0
    assert len(m.evaluate(df)) == 3  # without labels every row counts
    # save / restore, the logQ table included
    path = str(tmp_path / "model")
    m.save(path)
    m2 = th.TwoTower(fd, **args)
    assert float(m2._build().params["item_logq"].abs().max()) == 0.0
    m2.restore(path)
    assert np.array_equal(m2.predict(df), pred) and m2.evaluate(df, y) == res
    assert torch.equal(m2._build().params["item_logq"], e.params["item_logq"])
    c = clone(m)
    assert isinstance(c, th.TwoTower) and c.get_params()["temperature"] == k["hp"]["temperature"]
    # refusals through the model surface
    m3 = th.TwoTower(fd, **args)
    m3.hparams["feeder"] = "pinned"
    with pytest.raises(NotImplementedError, match="pinned"):
        m3.fit(df, y)
    m3 = th.TwoTower(fd, **args)
    m3.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m3._build()


def test_fit_learns_a_separable_set_and_sets_logq(hip_lib):
    """Users prefer the items of their own cluster: the loss of the last five steps is below that of the first five,
    recall@10 after training above recall@10 at the initial weights."""
    import recman_amd.th as th

    rs = np.random.RandomState(7)
    n, users, items, clusters = 2048, 64, 64, 4
    uid = rs.randint(0, users, n)
    iid = (rs.randint(0, items // clusters, n) * clusters + uid % clusters)
    df = pd.DataFrame(dict(uid=uid + 1, iid=iid + 1))
    fd = th.FeatureDictionary()
    fd["uid"], fd["iid"] = th.SparseFeat("uid", users), th.SparseFeat("iid", items)
    fd.initialize(df)
    m = th.TwoTower(fd, user_features=("uid",), item_features=("iid",), item_id_feature="iid",
                    user_hidden_units=(16, 8), item_hidden_units=(16, 8), logq_correction=True, epoch=5,
                    batch_size=256, learning_rate=0.01)
    before = m.evaluate(df)
    losses, step = [], m._fit_encoded
    m._fit_encoded = lambda *a, **kw: losses.append(float(step(*a, **kw)))
    seen = []
    assert m.fit(df, epoch_callback=lambda **kw: seen.append(kw["eval_results"])) is None
    after = m.evaluate(df)
    print(f"loss first five {np.mean(losses[:5]):.4f}, last five {np.mean(losses[-5:]):.4f}; "
          f"recall@10 {before[1]:.3f} -> {after[1]:.3f}")
    assert len(losses) == 5 * 8 and np.mean(losses[-5:]) < np.mean(losses[:5])
    assert after[1] > before[1]
    assert len(seen) == 5 and len(seen[-1][0]) == 2 and seen[-1][1] is None
    # logq[id] = log((count[id] + 1) / (N + V)) over the training frame; unseen ids get the +1 floor
    ids = fd["iid"](df["iid"]).reshape(-1)
    V = fd["iid"].feat_size
    want = np.log((np.bincount(ids, minlength=V) + 1.0) / (n + V)).astype(np.float32)
    got = m._build().params["item_logq"].cpu().numpy()
    assert np.array_equal(got, want) and got[0] == np.float32(np.log(1.0 / (n + V)))
