"""CPU: the two-tower restatement (tests/twotower_ref.py) pinned without a GPU - the closed-form backward against
autograd in float64, a pure-Python-loop restatement, the near-tie cap of every rank case - and the public surface:
th.TwoTower, ENGINES["twotower"], the header's symbols and every twotower_limits error."""
import os
import re

import pytest
import torch

from tests import twotower_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(True, True, True), (False, False, False), (True, False, True), (False, True, False)]


@pytest.mark.parametrize("B,H", [(1, 4), (15, 8), (17, 20), (65, 64)])
@pytest.mark.parametrize("ids,logq,w", VARIANTS)
def test_closed_form_backward_equals_autograd_in_float64(B, H, ids, logq, w):
    k = R.ibs_case(B, H, ids, logq, w)
    loss, dU, dV = R.loss_autograd(k["U"], k["V"], k["scale"], k["item"], k["logq"], k["w"], k["grad_scale"])
    assert abs(float(loss - k["loss"])) <= 1e-12
    for got, want, n in ((k["dU"], dU, "dU"), (k["dV"], dV, "dV")):
        m = R.grad_measure(got, want)
        print(f"B={B} H={H} {n}: closed form vs autograd {m:.2e}")
        assert m <= 1e-12, (n, m)


def test_degenerate_weights_and_ids():
    k = R.ibs_case(17, 8, zero_w=True)
    assert float(k["loss"]) == 0.0 and float(k["dU"].abs().max()) == 0.0 and float(k["dV"].abs().max()) == 0.0
    k = R.ibs_case(17, 8, same_ids=True)
    assert torch.equal(k["lse"], k["S"].diagonal()) and float(k["row_loss"].abs().max()) == 0.0
    assert int(k["rank"].max()) == 0 and float(k["dU"].abs().max()) == 0.0 and float(k["dV"].abs().max()) == 0.0
    k = R.ibs_case(1, 4)
    assert float(k["loss"]) == 0.0 and float(k["dU"].abs().max()) == 0.0


@pytest.mark.parametrize("ids,logq", [(True, True), (False, False)])
def test_python_loops_agree(ids, logq):
    k = R.ibs_case(15, 8, ids, logq, True)
    lse, rl, rank = R.loops(k["U"], k["V"], k["scale"], k["item"], k["logq"])
    assert float((torch.tensor(lse, dtype=torch.float64) - k["lse"]).abs().max()) <= 1e-12
    assert float((torch.tensor(rl, dtype=torch.float64) - k["row_loss"]).abs().max()) <= 1e-12
    assert rank == k["rank"].tolist()
    if ids:  # real duplicates occur and are masked
        assert len(set(k["item"].tolist())) < 15 and bool((~R.allowed(15, k["item"])).any())


def rank_cases():
    """Every case the GPU tests check ranks on (tests/test_gpu_twotower.py imports this list)."""
    out = [(B, H, v) for B, H in R.CASES for v in VARIANTS]
    return out


@pytest.mark.parametrize("B,H,v", rank_cases())
def test_near_tie_cap_holds_on_every_rank_case(B, H, v):
    k = R.ibs_case(B, H, *v)
    share = float((k["ties"] > 0).double().mean())
    print(f"B={B} H={H} {v}: {share:.3f} of the rows have a near tie")
    assert share <= R.TIE_SHARE
    # the float32 restatement's ranks obey the rule the kernels are held to
    f = R.fwd(k["U"].float(), k["V"].float(), k["scale"], k["item"], None if k["logq"] is None else k["logq"].float())
    R.check_ranks(f["rank"], k, what=f"B={B} H={H}: ")


def test_near_tie_cap_holds_on_the_tile_edge_and_split_cases(hip_lib):
    """The cases tests/test_gpu_twotower.py derives from the library's tile heights (host calls: no GPU needed)."""
    from recman_amd import ops

    rows, cols, smax = (ops.inbatch_softmax_tile(16, w) for w in ("rows", "cols", "max_splits"))
    assert rows % 16 == 0 and cols % 32 == 0 and smax >= 2
    assert ops.inbatch_softmax_workspace(130, 36) > 0 and ops.inbatch_softmax_workspace(0, 4) > 0
    for B, H in ((3 * rows + 5, 16), (2 * cols + 1, 16), (5 * cols + 7, 16), (130, 36), (65, 64), (17, 20)):
        k = R.ibs_case(B, H)
        assert float((k["ties"] > 0).double().mean()) <= R.TIE_SHARE, (B, H)


def test_rownorm_closed_form_equals_autograd():
    for B, H in R.ROWNORM_CASES:
        k = R.rownorm_case(B, H)
        x = k["X"].clone().requires_grad_(True)
        (R.rownorm_fwd(x)[0] * k["dY"]).sum().backward()
        assert R.grad_measure(k["dX"], x.grad) <= 1e-12
    Y, inv = R.rownorm_fwd(torch.zeros(2, 4, dtype=torch.float64))
    assert float(Y.abs().max()) == 0.0 and float(inv[0]) == 1.0 / R.EPS
    dY = torch.ones(2, 4, dtype=torch.float64)
    assert torch.equal(R.rownorm_bwd(Y, inv, dY), dY / R.EPS)


@pytest.mark.parametrize("normalize,masking,logq,labels", [(True, True, True, True), (False, False, False, False)])
def test_model_case_is_off_the_relu_kinks_and_differentiable(normalize, masking, logq, labels):
    k = R.make_case(normalize, masking, logq, labels)
    assert k["min_abs_pre"] >= R.KINK
    loss, row_loss, rank, grads = R.fwd_bwd(k["p"], k["spec"], k["idx"], k["dense"], k["y"], k["hp"], k["mv"])
    assert torch.isfinite(loss) and set(grads) == set(k["p"])
    assert float(grads["item_logq"].abs().max()) > 0 if logq else float(grads["item_logq"].abs().max()) == 0
    assert float(grads["user_dnn_layer_0_weights"].abs().max()) > 0
    rows = R.d_rows(k["p"], k["spec"], k["idx"], k["dense"], k["y"], k["hp"], k["mv"])
    assert rows.shape == (37, 5, 8) and float(rows.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ public surface
def test_public_surface():
    import recman_amd.th as th
    from recman_amd import engine as eng

    assert "TwoTower" in th.__all__ and th.TwoTower.model == "twotower"
    assert eng.ENGINES["twotower"] is eng.TwoTowerEngine
    assert eng.TwoTowerEngine.shardable is False and eng.TwoTowerEngine.use_bias_tables is False
    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in ("rm_inbatch_softmax_supported", "rm_inbatch_softmax_tile", "rm_inbatch_softmax_workspace",
                "rm_inbatch_softmax_fwd", "rm_inbatch_softmax_bwd", "rm_rownorm_fwd", "rm_rownorm_bwd"):
        assert re.search(rf"\b{sym}\s*\(", text), sym
    doc = th.TwoTower.evaluate.__doc__
    assert "BATCH COMPOSITION" in doc.upper()


def _spec(**kw):
    from recman_amd import engine as eng

    return eng.FeatureSpec(["u0", "u1", "it", "cat"], [4, 5, 6, 3], ["du", "di"], **kw)


def _hp(**kw):
    hp = dict(user_features=("u0", "u1", "du"), item_features=("it", "cat", "di"), item_id_feature="it",
              user_hidden_units=(16, 8), item_hidden_units=(8,), temperature=0.05)
    hp.update(kw)
    return hp


def test_limits_pass_and_describe_the_layout():
    from recman_amd import engine as eng

    lim = eng.twotower_limits(_hp(), _spec())
    assert lim["H"] == 8 and lim["scale"] == 20.0 and lim["id_col"] == 2
    assert lim["user"] == (0, 2, 0, 1) and lim["item"] == (2, 4, 1, 2)
    assert eng.twotower_limits(_hp())["H"] == 8  # without a spec: the feature-free limits only


@pytest.mark.parametrize("kw,match", [
    (dict(item_hidden_units=(12,)), "same"),
    (dict(user_hidden_units=(6,), item_hidden_units=(6,)), "multiple of 4"),
    (dict(user_hidden_units=(260,), item_hidden_units=(260,)), "multiple of 4"),
    (dict(user_hidden_units=()), "output layer"),
    (dict(temperature=0.0), "temperature"),
    (dict(temperature=-1.0), "temperature"),
    (dict(item_features=()), "both towers"),
    (dict(item_features=("it", "cat", "di", "u0")), "twice"),
    (dict(item_id_feature=None), "item_id_feature"),
    (dict(item_id_feature=None, mask_accidental_hits=False, logq_correction=True), "item_id_feature"),
    (dict(item_id_feature="u0"), "not one of item_features"),
    (dict(item_features=("it", "di")), "partition"),
    (dict(item_features=("it", "cat", "di", "ghost")), "partition"),
    (dict(user_features=("u0", "cat", "du"), item_features=("it", "u1", "di")), "contiguous"),
    (dict(user_features=("du",), item_features=("u0", "u1", "it", "cat", "di")), "no embedding feature"),
])
def test_every_limit_raises_without_a_gpu(kw, match):
    from recman_amd import engine as eng

    with pytest.raises(ValueError, match=match):
        eng.twotower_limits(_hp(**kw), _spec())


def test_limits_on_feature_kinds_and_the_constructor():
    import recman_amd.th as th
    from recman_amd import engine as eng

    with pytest.raises(ValueError, match="plain SparseFeat"):
        eng.twotower_limits(_hp(), _spec(multi_names=["it"]))
    with pytest.raises(ValueError, match="contiguous"):  # the dense features interleave
        eng.twotower_limits(_hp(user_features=("u0", "u1", "du", "dz"), item_features=("it", "cat", "di")),
                            eng.FeatureSpec(["u0", "u1", "it", "cat"], [4, 5, 6, 3], ["du", "di", "dz"]))
    seq = eng.FeatureSpec(["u0", "it", "hist"], [4, 6, 0], [], seq_query={"hist": "it"})
    with pytest.raises(NotImplementedError, match="sequence"):
        eng.twotower_limits(_hp(user_features=("u0", "hist"), item_features=("it",)), seq)
    # without masking and logQ no item id is needed
    assert eng.twotower_limits(_hp(item_id_feature=None, mask_accidental_hits=False), _spec())["id_col"] is None
    # the constructor checks the same limits before any GPU work
    fd = th.FeatureDictionary()
    for n, v in (("u0", 3), ("u1", 4), ("it", 5), ("cat", 2)):
        fd[n] = th.SparseFeat(n, v)
    fd["du"], fd["di"] = th.DenseFeat("du"), th.DenseFeat("di")
    args = dict(user_features=("u0", "u1", "du"), item_features=("it", "cat", "di"), item_id_feature="it",
                user_hidden_units=(16, 8), item_hidden_units=(8,))
    m = th.TwoTower(fd, **args)
    assert m.metric_names == ["inbatch_loss", "recall@10"] and m.limits_["user"] == (0, 2, 0, 1)
    assert m.get_params()["temperature"] == 0.05
    from sklearn.base import clone

    c = clone(th.TwoTower(fd, recall_at=[1, 5], **dict(args, user_features=["u0", "u1", "du"])))
    assert isinstance(c, th.TwoTower) and c.metric_names == ["inbatch_loss", "recall@1", "recall@5"]
    with pytest.raises(ValueError, match="same"):
        th.TwoTower(fd, **dict(args, item_hidden_units=(12,)))
    with pytest.raises(ValueError, match="strict_reference"):
        th.TwoTower(fd, strict_reference=True, **args)
    with pytest.raises(ValueError, match="partition"):
        th.TwoTower(fd, **dict(args, user_features=("u0", "du")))
    with pytest.raises(ValueError, match="recall_at"):
        th.TwoTower(fd, recall_at=(0,), **args)
    with pytest.raises(ValueError, match="0 or 1"):
        m._weights([0, 2, 1], 3)
