"""CPU: the ranking twin (tests/rank_ref.py) and its cases, the C ABI and ledger of include/recman_hip_rank.h, the
limits of rm_rank_loss and every validation error of the public surface (hparams rank_loss, rank_group_by,
rank_loss_weight, rank_norm) - all without a GPU."""
import ctypes
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import gauc_ref as G
from tests import rank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recman_hip_rank.h")
COMBOS = [(k, n) for k in R.KINDS for n in R.NORMS]


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(rm_[a-z0-9_]+)\s*\(", _header_text())))


def _stream_entry_points():
    return {m.group(1) for m in re.finditer(r"\b(rm_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", _header_text(), flags=re.S)
            if re.search(r"\brm_stream_t\s+stream\b", m.group(2))}


# ------------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("kind,norm", COMBOS)
@pytest.mark.parametrize("name", ["sizes_1_to_5_b1000", "group_700_among_singletons", "no_ids_b777", "logits_x60",
                                  "ids_0_and_max", "b2_one_pair"])
def test_closed_form_gradient_is_autograd(name, kind, norm):
    """(Not the tied case: at d = 0 autograd differentiates max(-d, 0) and |d| by their one-sided conventions, -1 and
    0, where the smooth function's derivative is -1/2; test_tied_logits_in_closed_form holds that case.)"""
    c = R.make_case(name)
    s = c["s"].clone().requires_grad_(True)
    R.rank_term(s, c["y"], c["groups"], kind, norm).backward()
    g = R.rank_grad(c["s"], c["y"], c["groups"], kind, norm)
    err = float((g - s.grad).abs().max())
    print(f"{name} {kind}/{norm}: closed form against autograd {err:.2e}, largest |g| {float(g.abs().max()):.2e}")
    assert float(g.abs().max()) > 0 and err <= 1e-12 * float(g.abs().max())


@pytest.mark.parametrize("name", ["sizes_1_to_5_b1000", "group_700_among_singletons", "ids_0_and_max", "tied_logits",
                                  "logits_x60"])
def test_step_function_in_the_group_norm_is_one_minus_gauc(name):
    """[s_i < s_j] + 0.5 [s_i = s_j] for the softplus: the pairwise / "group" term is 1 - GAUC(impressions), which pins
    c_g and the scored-group rule."""
    c = R.make_case(name)
    L = float(R.rank_term(c["s"], c["y"], c["groups"], "pairwise", "group", pair_fn=R.step_neg))
    gauc, scored, weight, _ = G.exact_gauc(c["y"].numpy(), c["s"].numpy(), c["groups"].numpy())
    tot = R.counts(c["y"], c["groups"])
    assert scored == tot["scored_groups"] > 0 and weight == tot["weight"]
    assert abs(L - float(1 - gauc)) <= 1e-12, (L, float(1 - gauc))
    assert isinstance(gauc, Fraction)


@pytest.mark.parametrize("kind,norm", COMBOS)
def test_one_class_gives_zero_and_a_zero_gradient(kind, norm):
    c = R.make_case("single_class_groups")
    assert R.counts(c["y"], c["groups"])["scored_groups"] == 0 and R.counts(c["y"], c["groups"])["groups"] == 60
    for y, groups in ((c["y"], c["groups"]), (torch.ones_like(c["y"]), None), (torch.zeros_like(c["y"]), None)):
        assert float(R.rank_term(c["s"], y, groups, kind, norm)) == 0.0
        g = R.rank_grad(c["s"], y, groups, kind, norm)
        assert float(g.abs().max()) == 0.0 and not bool(torch.signbit(g).any())  # +0.0


@pytest.mark.parametrize("kind,norm", COMBOS)
def test_a_permuted_input_gives_a_permuted_gradient(kind, norm):
    c = R.make_case("sizes_1_to_5_b1000")
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(5))
    g = R.rank_grad(c["s"], c["y"], c["groups"], kind, norm)
    gp = R.rank_grad(c["s"][perm], c["y"][perm], c["groups"][perm], kind, norm)
    assert float((gp - g[perm]).abs().max()) <= 1e-15
    a, b = R.rank_term(c["s"], c["y"], c["groups"], kind, norm), R.rank_term(c["s"][perm], c["y"][perm],
                                                                             c["groups"][perm], kind, norm)
    assert abs(float(a - b)) <= 1e-13 * float(a)


def test_tied_logits_in_closed_form():
    c = R.make_case("tied_logits")
    tot = R.counts(c["y"], c["groups"])
    assert abs(float(R.rank_term(c["s"], c["y"], c["groups"], "pairwise", "pairs")) - R.LN2) <= 1e-14  # log 2 per pair
    g = R.rank_grad(c["s"], c["y"], c["groups"], "pairwise", "group")
    for pos, neg in R.split(c["y"], c["groups"]):
        P, N = len(pos), len(neg)
        if P and N:
            cg = R.coef("pairwise", "group", P, N, tot)
            assert torch.allclose(g[pos], torch.full((P,), -0.5 * cg * N, dtype=torch.float64), rtol=1e-14, atol=0)
            assert torch.allclose(g[neg], torch.full((N,), 0.5 * cg * P, dtype=torch.float64), rtol=1e-14, atol=0)


def test_cases_are_what_their_names_say():
    sizes = lambda c: sorted(np.unique(c["groups"].numpy(), return_counts=True)[1].tolist())  # noqa: E731
    assert R.make_case("b1")["s"].shape == (1,) and R.make_case("b2_one_pair")["y"].tolist() == [1, 0]
    c = R.make_case("sizes_1_to_5_b1000")
    assert c["s"].shape == (1000,) and set(sizes(c)) == {1, 2, 3, 4, 5}
    assert not bool((c["groups"][1:] >= c["groups"][:-1]).all())  # ids in random order
    c = R.make_case("group_300_across_a_tile_edge")
    order = np.sort(c["groups"].numpy())
    big = np.unique(order, return_counts=True)
    gid = big[0][big[1] == 300][0]
    at = np.nonzero(order == gid)[0]
    assert at[0] == 3900 and at[-1] == 4199  # across sorted position 4096: a sort tile, a pair tile and a piece end there
    c = R.make_case("group_700_among_singletons")
    assert sizes(c) == [1] * 800 + [700]
    tot = R.counts(c["y"], c["groups"])
    assert tot["scored_groups"] == 1 and min(tot["pos"], 700 - tot["pos"]) > 256  # both runs span tiles of 256
    c = R.make_case("ids_0_and_max")
    assert sorted(set(c["groups"].tolist())) == [0, 2 ** 32 - 1]
    c = R.make_case("logits_x60")
    assert float(c["s"].abs().max()) > 120 and R.make_case("no_ids_b777")["groups"] is None
    for name in R.CASES:
        c = R.make_case(name)
        assert torch.equal(c["s"].float().double(), c["s"]) and torch.equal(c["dlogit_in"].float().double(), c["dlogit_in"])
    assert R.make_case("b1") is R.make_case("b1")  # made once


def test_combination_is_the_contract():
    c = R.make_case("sizes_1_to_5_b1000")
    s, y, g = c["s"], c["y"], c["groups"]
    loss, d, L = R.combine(s, y, g, "pairwise", "group", 0.3, 0.25, c["dlogit_in"], c["loss_in"])
    assert abs(float(loss) - (0.7 * float(c["loss_in"]) + 0.3 * float(L))) <= 1e-15
    want = 0.25 * (0.7 * c["dlogit_in"] + 0.3 * R.rank_grad(s, y, g, "pairwise", "group"))
    assert float((d - want).abs().max()) <= 1e-18
    bce, dbce = R.bce(s, y)
    p = torch.sigmoid(s)
    assert abs(float(bce) - float(-(y * torch.log(p) + (1 - y) * torch.log1p(-p)).mean())) <= 1e-6
    assert float((dbce - (p - y) / 1000).abs().max()) <= 1e-8  # (the Keras epsilon inside the logs)


# ------------------------------------------------------------------------------------------- the ABI and the ledger
def test_the_header_is_bound_in_its_own_table(hip_lib):
    from recman_amd import _lib

    syms = _declared()
    assert syms == sorted(["rm_rank_loss_workspace", "rm_rank_loss"])
    for name in syms:
        assert hasattr(hip_lib, name), f"{name} declared in recman_hip_rank.h but not exported"
    assert set(_lib.SIGNATURES_RANK) == set(syms)
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_I64) | set(_lib.SIGNATURES_TOPK) | set(_lib.SIGNATURES_MULTITASK)
    assert not set(_lib.SIGNATURES_RANK) & others
    assert hip_lib.rm_rank_loss_workspace.restype is ctypes.c_int64 and hip_lib.rm_rank_loss.restype is ctypes.c_int
    # one argtype per declared parameter
    for name in syms:
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, _header_text(), flags=re.S)
        assert len(_lib.SIGNATURES_RANK[name][1]) == len(m.group(1).split(",")), name
    assert "rm_rank" not in open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    # the record: a double and six int64
    text = open(HEADER).read()
    fields = re.findall(r"^\s+(double|int64_t)\s+(\w+);", text[text.index("typedef struct rm_rank_result"):], flags=re.M)
    assert fields == [("double", "value")] + [("int64_t", n) for n in ("groups", "scored_groups", "pairs", "pos",
                                                                       "weight", "flags")]


def test_ledger_covers_every_entry_point_with_a_stream():
    from tests import test_gpu_rank as T

    entries = _stream_entry_points()
    assert entries == {"rm_rank_loss"}
    assert set(T.COVERED) == entries
    for entry, test in T.COVERED.items():
        fn = getattr(T, test)
        assert "lds_pattern" in inspect.signature(fn).parameters, f"{test} does not run under lds_pattern"


def _call(hip_lib, B=8, kind=0, norm=1, alpha=0.5, grad_scale=1.0, logit=4096, ws=8192, out=None):
    """rm_rank_loss with stand-in pointers: every limit is checked before anything is launched."""
    rc = hip_lib.rm_rank_loss(logit, 4096, None, B, kind, norm, alpha, grad_scale, None, 4096, None, None, out, ws, None)
    return rc, hip_lib.rm_last_error().decode()


@pytest.mark.parametrize("kw,match", [
    (dict(B=0), r"B = 0 outside \[1, 2\^24\]"),
    (dict(B=2 ** 24 + 1), r"B = 16777217 outside \[1, 2\^24\]"),
    (dict(kind=2), r"kind 2 \(0 pairwise, 1 listwise\)"),
    (dict(norm=-1), r"norm -1 \(0 pairs, 1 group\)"),
    (dict(alpha=0.0), r"alpha = 0 outside \(0, 1\]"),
    (dict(alpha=1.5), r"alpha = 1.5 outside \(0, 1\]"),
    (dict(alpha=float("nan")), r"alpha = nan outside"),
    (dict(grad_scale=float("inf")), r"grad_scale is not finite"),
    (dict(logit=None), r"NULL pointer"),
    (dict(ws=None), r"NULL pointer"),
    (dict(ws=8200), r"not 16-byte aligned"),
    (dict(out=4104), r"not 16-byte aligned"),
])
def test_every_limit_raises_without_a_gpu(hip_lib, kw, match):
    rc, msg = _call(hip_lib, **kw)
    assert rc == -1, (rc, msg)  # RM_EINVAL
    assert re.search(match, msg), msg


def test_workspace_is_linear_in_the_batch(hip_lib):
    from recman_amd import ops

    w = [ops.rank_loss_workspace(B) for B in (1, 4096, 1 << 16, 1 << 20, 1 << 24)]
    assert w == sorted(w) and w[-1] <= 160 * (1 << 24) and w[0] < 1 << 16  # O(B): below 160 bytes per example
    for B in (0, -3, (1 << 24) + 1):
        with pytest.raises(ValueError, match=r"outside \[1, 2\^24\]"):
            ops.rank_loss_workspace(B)
        assert hip_lib.rm_rank_loss_workspace(B) == 0


# ------------------------------------------------------------------------------------------------ the public surface
def _fd(th):
    fd = th.FeatureDictionary()
    for n, v in (("user", 40), ("item", 50), ("cat", 7)):
        fd[n] = th.SparseFeat(n, v)
    fd["price"] = th.DenseFeat("price")
    return fd


def _deepfm(th, **hp):
    m = th.DeepFM(_fd(th), embedding_size=16, deep_dropout=(1, 1, 1))
    m.hparams.update(hp)  # a gen-1 class: through model.hparams
    return m


def test_rank_config_resolves_the_hparams_without_a_gpu():
    import recman_amd.th as th

    assert _deepfm(th)._rank_config() is None
    assert th.hparams.xDeepFM().defaults()["rank_loss"] is None
    d = th.hparams.xDeepFM().defaults()
    assert (d["rank_group_by"], d["rank_loss_weight"], d["rank_norm"]) == (None, 0.5, "group")
    m = _deepfm(th, rank_loss="pairwise", rank_group_by="item")
    assert m._rank_config() == dict(kind="pairwise", norm="group", alpha=0.5, col=1)
    m = _deepfm(th, rank_loss="listwise", rank_norm="pairs", rank_loss_weight=1)
    assert m._rank_config() == dict(kind="listwise", norm="pairs", alpha=1.0, col=None)
    # a gen-2 class: in the dict
    x = th.xDeepFM(_fd(th), dict(rank_loss="pairwise", rank_group_by="user", rank_loss_weight=0.25))
    assert x._rank_config() == dict(kind="pairwise", norm="group", alpha=0.25, col=0)
    assert m._engine is None and x._engine is None


@pytest.mark.parametrize("hp,exc,match", [
    (dict(rank_loss="pointwise"), ValueError, "rank_loss='pointwise'.*'pairwise' or 'listwise'"),
    (dict(rank_loss="pairwise", rank_norm="mean"), ValueError, "rank_norm='mean'"),
    (dict(rank_loss="pairwise", rank_loss_weight=0), ValueError, "0 < rank_loss_weight <= 1"),
    (dict(rank_loss="pairwise", rank_loss_weight=1.01), ValueError, "0 < rank_loss_weight <= 1"),
    (dict(rank_loss="listwise", rank_loss_weight="half"), ValueError, "0 < rank_loss_weight <= 1"),
    (dict(rank_loss="pairwise", rank_group_by="nobody"), ValueError, "rank_group_by='nobody' must name a SparseFeat"),
    (dict(rank_loss="pairwise", rank_group_by="price"), ValueError, "rank_group_by='price' must name a SparseFeat"),
    (dict(rank_loss="pairwise", table_sharding="row"), NotImplementedError, "pairs across ranks or micro-batches"),
])
def test_every_validation_error_is_raised_without_a_gpu(hp, exc, match):
    import recman_amd.th as th

    m = _deepfm(th, **hp)
    with pytest.raises(exc, match=match):
        m._rank_config()
    with pytest.raises(exc, match=match):
        m._build()  # before any device work
    assert m._engine is None


def test_regression_and_multi_logit_models_are_refused():
    import recman_amd.th as th

    m = th.DeepFM(_fd(th), embedding_size=16, loss_type="mse")
    m.hparams["rank_loss"] = "pairwise"
    with pytest.raises(ValueError, match="needs 0/1 labels: the task is 'regression'"):
        m._rank_config()
    fd = th.FeatureDictionary()
    for n, v in (("u0", 3), ("u1", 4), ("it", 5), ("cat", 2)):
        fd[n] = th.SparseFeat(n, v)
    tt = th.TwoTower(fd, user_features=("u0", "u1"), item_features=("it", "cat"), item_id_feature="it",
                     user_hidden_units=(16, 8), item_hidden_units=(8,))
    tt.hparams["rank_loss"] = "listwise"
    with pytest.raises(NotImplementedError, match="twotower trains by the in-batch softmax"):
        tt._rank_config()
    for make, model in ((th.MMoE, "mmoe"), (th.PLE, "ple")):
        m = make(fd)
        m.hparams["rank_loss"] = "pairwise"
        assert m.model == model
        with pytest.raises(NotImplementedError, match=f"{model} has one logit per task"):
            m._rank_config()


def test_labels_are_checked_once_on_the_host():
    import recman_amd.th as th

    m = _deepfm(th, rank_loss="pairwise")
    m._check_rank_labels(np.array([0, 1, 1, 0]))
    m._check_rank_labels(None)
    with pytest.raises(ValueError, match=r"needs labels in \{0, 1\}"):
        m._check_rank_labels(np.array([0, 1, 2]))
    with pytest.raises(ValueError, match=r"needs labels in \{0, 1\}"):
        m._check_rank_labels(np.array([0.0, 0.5]))
    _deepfm(th)._check_rank_labels(np.array([0, 3]))  # no ranking objective: nothing to check
    assert "ONE batch" in th.DeepModel._rank_config.__doc__
    assert math.isclose(R.LN2, 0.6931471805599453)
