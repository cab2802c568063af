"""CPU: the PLE / entire-space twin (tests/ple_ref.py) and its cases, the C ABI and ledger of
include/recman_hip_multitask.h, and the host side of the public surface (th.MMoE's new arguments, th.PLE, the limits) -
all without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
from sklearn.base import clone

from oracle import th_layers as TL
from tests import mmoe_ref as M
from tests import ple_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recman_hip_multitask.h")
ENTRY_POINTS = ["rm_cgc_mix_supported", "rm_cgc_mix_tile", "rm_cgc_mix_fwd", "rm_cgc_mix_bwd",
                "rm_multitask_loss_es_workspace", "rm_multitask_loss_es"]


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared():
    return re.findall(r"\b(rm_[a-z0-9_]+)\s*\(", _header_text())


def _stream_entry_points():
    return {m.group(1) for m in re.finditer(r"\b(rm_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", _header_text(), flags=re.S)
            if re.search(r"\brm_stream_t\s+stream\b", m.group(2))}


# ------------------------------------------------------------------------------------------------------ the twin
SMALL = [(5, 2, 2, 2, 8, 1), (3, 1, 1, 1, 4, 0), (4, 3, 1, 2, 12, 1), (2, 8, 3, 8, 4, 1), (6, 2, 4, 1, 8, 0)]


@pytest.mark.parametrize("shape", SMALL)
def test_cgc_fwd_is_the_explicit_loops(shape):
    B, T, S, C, H, sg = shape
    c = R.mix_case(*shape)
    M_, P = R.cgc_fwd(c["Z"], c["A"], T, S, C, sg)
    assert float((M_ - R.cgc_loops(c["Z"], c["A"], T, S, C, sg)).abs().max()) <= 1e-14
    N, AW, G = R.widths(T, S, C, sg)
    assert M_.shape == (B, G * H) and P.shape == (B, AW) and c["Z"].shape == (B, N * H)
    for a0, a1, ex in R.gates(T, S, C, sg):
        assert float((P[:, a0:a1].sum(dim=1) - 1).abs().max()) <= 1e-14 and len(ex) == a1 - a0
    # every expert is in at least one gate; a task's own experts in exactly its gate (and the shared one)
    seen = [sum(e in ex for _, _, ex in R.gates(T, S, C, sg)) for e in range(N)]
    assert seen == [1 + sg] * (T * S) + [T + sg] * C


@pytest.mark.parametrize("shape", SMALL)
def test_closed_form_backward_is_autograd(shape):
    B, T, S, C, H, sg = shape
    c = R.mix_case(*shape)
    Z, A = c["Z"].clone().requires_grad_(True), c["A"].clone().requires_grad_(True)
    (R.cgc_fwd(Z, A, T, S, C, sg)[0] * c["dM"]).sum().backward()
    dZ, dA = R.cgc_bwd(c["Z"], c["A"], T, S, C, sg, c["dM"])
    assert float((dZ - Z.grad).abs().max()) <= 1e-13 and float((dA - A.grad).abs().max()) <= 1e-13
    # the rows of dA sum to 0 per gate (softmax is shift-invariant)
    for a0, a1, _ in R.gates(T, S, C, sg):
        assert float(dA[:, a0:a1].sum(dim=1).abs().max()) <= 1e-13


def test_kernel_cases_are_the_issue_s():
    assert R.MIX_CASES == [(77, 2, 2, 2, 128, 1), (1, 1, 1, 1, 4, 0), (33, 8, 3, 8, 36, 1), (70, 3, 1, 1, 512, 1),
                           (64, 2, 4, 1, 8, 0)]
    assert R.widths(8, 3, 8, 1) == (32, 8 * 11 + 32, 9)
    assert len(R.LOSS_CASES) == 10 and (3, 77, (2, 0)) in R.LOSS_CASES


def test_entire_space_gradient_is_the_finite_difference():
    c = R.es_case(3, 77)
    types, w, es = c["types"], c["weights"], c["es"]
    logit = c["logit"].clamp(-6, 6)  # away from the clip bounds: q and 1 - q stay above 1e-6
    _, _, _, _, g = R.es_loss_head_grad(logit, c["Y"], types, w, es, 1.0)
    h, worst = 1e-6, 0.0
    for t in range(3):
        for i in range(0, 77, 5):
            d = torch.zeros_like(logit)
            d[t, i] = h
            fd = (R.es_loss_head(logit + d, c["Y"], types, w, es)[0]
                  - R.es_loss_head(logit - d, c["Y"], types, w, es)[0]) / (2 * h)
            worst = max(worst, abs(float(fd - g[t, i])))
    print(f"entire-space gradient against central differences: {worst:.2e}")
    assert worst <= 1e-8
    # exactly +0.0 where z is unobserved (task v), and task c then keeps its own term only
    unseen = ~c["z_seen"]
    assert int(unseen.sum()) > 0 and float(g[es[1]][unseen].abs().max()) == 0.0
    plain = M.loss_head_grad(logit, c["Y"], types, w, 1.0)[4]
    assert torch.equal(g[es[0]][unseen], plain[es[0]][unseen]) and torch.equal(g[2], plain[2])


def test_entire_space_reduces_to_the_plain_heads():
    g = torch.Generator().manual_seed(7)
    B = 50
    logit = torch.randn(2, B, generator=g, dtype=torch.float64) * 2
    Y = torch.stack([torch.ones(B, dtype=torch.float64), (torch.rand(B, generator=g) < 0.4).double()], dim=1)
    loss, loss_t, n_t, pred = R.es_loss_head(logit, Y, ["classification"] * 2, None, (0, 1))
    q = torch.sigmoid(logit[0]) * torch.sigmoid(logit[1])
    assert abs(float(loss_t[1] - TL.create_loss(Y[:, 1], q, "classification"))) <= 1e-14 and n_t.tolist() == [B, B]
    assert torch.equal(pred[1], torch.sigmoid(logit[1]))
    # es = (-1, -1): mmoe_ref.loss_head itself
    c = M.loss_case(3, 77)
    a = R.es_loss_head_grad(c["logit"], c["Y"], c["types"], c["weights"], (-1, -1), 0.5)
    b = M.loss_head_grad(c["logit"], c["Y"], c["types"], c["weights"], 0.5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the label rule
    Yl = torch.tensor([[0.0, R.NAN], [0.0, 1.0], [1.0, 1.0], [1.0, 0.0], [1.0, R.NAN], [R.NAN, 1.0], [R.NAN, R.NAN]],
                      dtype=torch.float64)
    z, seen = R.es_labels(Yl, 0, 1)
    assert seen.tolist() == [True, True, True, True, False, False, False] and z[:4].tolist() == [0.0, 0.0, 1.0, 0.0]


def test_loss_cases_cover_what_they_claim():
    for T, B, es in R.LOSS_CASES:
        c = R.es_case(T, B, es)
        Y = c["Y"]
        assert all(c["types"][t] == "classification" for t in es) and c["n_t"][es[1]] == int(c["z_seen"].sum())
        if B >= 77:
            click, conv = Y[:, es[0]], Y[:, es[1]]
            assert 0.2 < float((click == 1).double().mean()) < 0.4 and bool(torch.isnan(conv[click == 0]).all())
            assert bool(torch.isnan(conv[click == 1]).any()) and bool(torch.isnan(click).any())
            assert 0 < int((~c["z_seen"]).sum()) < B
        print(f"T={T} B={B} es={es}: float32 CPU measures {c['f32']}")
        assert max(c["f32"].values()) <= 1e-5


def test_saturation_grid_is_clear_of_the_clamp():
    c = R.saturation_case()
    eps = TL.KERAS_EPS
    for x in (c["q"], c["one_minus_q"]):
        assert bool(((x < eps / 2) | (x > 2 * eps)).all())
    assert c["B"] == 162 and 0 < int(c["clipped"].sum()) < 162 and bool(torch.isfinite(c["dlogit"]).all())
    # autograd through the clamp: the coupled gradient is exactly 0 in the clip region
    assert float(c["dlogit"][1][c["clipped"]].abs().max()) == 0.0
    assert float(c["dlogit"][1][~c["clipped"]].abs().min()) > 0.0
    print(f"saturation grid: float32 CPU measures {c['f32']}")


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES) + ["seq"])
def test_model_cases_keep_their_distance_from_the_kink(name):
    k = R.make_seq_case() if name == "seq" else R.make_case(*R.MODEL_CASES[name])
    p, spec, idx, dense, hp, mv = (k[n] for n in ("p", "spec", "idx", "dense", "hp", "mv"))
    print(f"{name}: the closest pre-activation is {k['min_abs_pre']:.2e} from its kink")
    assert k["min_abs_pre"] >= R.KINK and hp["deep_l2_reg"] in (1e-4, 1e-3)
    logit, P = R.ple_logits(p, spec, idx, dense, hp, mv)
    T = len(hp["task_names"])
    assert logit.shape == (T, idx.shape[0]) and 0.01 < float(logit.abs().max()) < 20
    if R.is_ple(hp):
        S, C, L = hp["task_experts"], hp["num_experts"], hp["num_levels"]
        assert P.shape == (idx.shape[0], T, S + C) and float((P.sum(dim=2) - 1).abs().max()) <= 1e-12
        names = {n for n in p if n.startswith("level_")}
        assert names == ({f"level_{l}_gate_weights" for l in range(L)}
                         | {f"level_{l}_expert_layer_{i}_{v}" for l in range(L) for v in ("weights", "bias")
                            for i in range(len(hp["expert_hidden_units"]))})
        assert p[f"level_{L - 1}_gate_weights"].shape[1] == T * (S + C)  # no shared gate on the last level
    # the float32 run of the same code stays inside the model tests' bounds (tests/test_gpu_parity.py)
    want = R.fwd_bwd(p, spec, idx, dense, k["Y"], hp, mv)
    got = R.fwd_bwd(R.to_f32(p), spec, idx, dense.float(), k["Y"], hp, mv)
    assert float((got[1].double() - want[1]).abs().max()) <= 1e-5
    for n in want[3]:
        if not n.startswith("hist_"):
            assert R.grad_measure(got[3][n], want[3][n]) <= M.TOL_GRAD, n
    if hp["entire_space"] is not None:  # the pair's labels: conversions unobserved on non-clicks
        c, v = R.es_pair(hp)
        assert bool(torch.isnan(k["Y"][:, v][k["Y"][:, c] == 0]).all())
        assert float(want[3][next(n for n in p if n.endswith("gate_weights"))].abs().max()) > 0


# ------------------------------------------------------------------------------------------- the ABI and the ledger
def test_the_header_is_bound_in_its_own_table(hip_lib):
    from recman_amd import _lib

    assert _declared() == ENTRY_POINTS  # exactly these, in this order
    assert list(_lib.SIGNATURES_MULTITASK) == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(hip_lib, name), f"{name} declared in recman_hip_multitask.h but not exported"
        restype, argtypes = _lib.SIGNATURES_MULTITASK[name]
        assert getattr(hip_lib, name).restype is restype
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_I64) | set(_lib.SIGNATURES_TOPK)
    assert not set(_lib.SIGNATURES_MULTITASK) & others
    assert hip_lib.rm_multitask_loss_es_workspace.restype is ctypes.c_int64
    # the argument counts of the declarations
    text = _header_text()
    for name, (_, argtypes) in _lib.SIGNATURES_MULTITASK.items():
        args = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == len(argtypes), name
    # recman_hip.h itself declares none of them
    main = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    assert "rm_cgc" not in main and "rm_multitask_loss_es" not in main


def test_ledger_covers_every_entry_point_with_a_stream():
    from tests import test_gpu_ple as T

    entries = _stream_entry_points()
    assert entries == {"rm_cgc_mix_fwd", "rm_cgc_mix_bwd", "rm_multitask_loss_es"}
    assert set(T.COVERED) == entries
    for entry, test in T.COVERED.items():
        fn = getattr(T, test)
        assert "lds_pattern" in inspect.signature(fn).parameters, f"{test} does not run under lds_pattern"


def test_limits_are_refused_without_a_gpu(hip_lib):
    from recman_amd import ops

    ok = [(1, 1, 1, 4, 0), (8, 3, 8, 512, 1), (2, 2, 2, 128, 1), (7, 4, 4, 36, 1), (2, 4, 1, 8, 0)]
    bad = [(0, 1, 1, 4, 0), (9, 1, 1, 4, 0), (1, 0, 1, 4, 0), (1, 5, 1, 4, 0), (1, 1, 0, 4, 0), (1, 1, 9, 4, 0),
           (8, 4, 1, 4, 0), (1, 1, 1, 6, 0), (1, 1, 1, 516, 0), (1, 1, 1, 0, 0), (1, 1, 1, 4, 2)]
    assert all(ops.cgc_mix_supported(*s) for s in ok) and not any(ops.cgc_mix_supported(*s) for s in bad)
    # the tile: 256 threads over lane groups of the power of two >= H / 4 (at most 64); LDS-bound blocks shrink
    assert [ops.cgc_mix_tile(2, 2, 2, H, 1) for H in (4, 8, 16, 36, 128, 256, 512)] == [256, 128, 64, 16, 8, 4, 4]
    assert ops.cgc_mix_tile(2, 1, 1, 8, 1, "cap") == 1024 and ops.cgc_mix_tile(2, 1, 1, 8, 1, backward=True) == 128
    assert ops.cgc_mix_tile(8, 3, 8, 4, 1) == 128 and ops.cgc_mix_tile(8, 3, 8, 4, 1, backward=True) == 64
    with pytest.raises(ValueError, match="N = T S \\+ C <= 32"):
        ops.cgc_mix_tile(8, 4, 1, 8, 1)
    assert ops.cgc_widths(2, 2, 2, 1) == (6, 14, 3) and ops.cgc_widths(2, 2, 2, 0) == (6, 8, 2)
    # NULL outputs and stand-in operand pointers: nothing can be launched
    rc = hip_lib.rm_cgc_mix_fwd(4096, 48, 8192, 16, 4, 2, 5, 2, 8, 1, None, 0, None, 0, None)
    msg = hip_lib.rm_last_error().decode()
    assert rc == -1 and re.search(r"S=5.*1 <= S <= 4 task experts.*1 <= C <= 8.*N = T S \+ C <= 32.*4\.\.512", msg), msg
    rc = hip_lib.rm_cgc_mix_fwd(4096, 50, 8192, 16, 4, 2, 2, 2, 8, 1, 12288, 24, None, 0, None)
    assert rc == -1 and re.search(r"Z must be 16-byte aligned.*multiple of 4 floats", hip_lib.rm_last_error().decode())
    assert hip_lib.rm_cgc_mix_fwd(None, 0, None, 0, 0, 2, 2, 2, 8, 1, None, 0, None, 0, None) == 0  # B = 0
    assert ops.multitask_loss_es_workspace(77, 3) == ops.multitask_loss_workspace(77, 3)
    types = (ctypes.c_int * 3)(0, 1, 0)
    for c, v in ((0, 0), (0, 3), (-1, 0), (0, 1)):  # equal, out of range, half a pair, a regression task
        rc = hip_lib.rm_multitask_loss_es(4096, None, types, None, 1.0, 5, 3, c, v, 8192, None, None, None, None, None,
                                          None)
        assert rc == -1 and "two distinct classification tasks" in hip_lib.rm_last_error().decode(), (c, v)


# ---------------------------------------------------------------------------------------------------- the surface
def _fd():
    return type("NoFeatures", (), {"embedding_feats": []})()


def test_public_surface():
    import recman_amd.th as th
    from recman_amd import engine as eng

    sig = inspect.signature(th.MMoE.__init__).parameters
    names = list(sig)
    assert names[names.index("device") + 1:] == ["task_experts", "num_levels", "entire_space"]
    assert (sig["task_experts"].default, sig["num_levels"].default, sig["entire_space"].default) == (0, 1, None)
    assert th.MMoE.model == "mmoe" and th.MMoE(_fd()).model == "mmoe"
    assert th.MMoE(_fd(), task_experts=1).model == "ple" and th.MMoE.model == "mmoe"
    assert "PLE" in th.__all__ and inspect.isfunction(th.PLE) and not inspect.isclass(th.PLE)
    m = th.PLE(_fd())
    assert isinstance(m, th.MMoE) and m.model == "ple"
    assert (m.num_experts, m.task_experts, m.num_levels, m.entire_space) == (2, 2, 2, None)
    assert th.PLE(_fd(), num_levels=3, task_experts=1).hparams["num_levels"] == 3
    assert eng.ENGINES["ple"] is eng.PLEEngine and eng.PLEEngine.model == "ple"
    assert eng.PLEEngine.use_bias_tables is False and eng.PLEEngine.shardable is False
    with pytest.raises(NotImplementedError, match="one GPU"):
        eng.PLEEngine.require_shardable()
    doc = " ".join(eng.PLEEngine.__doc__.split())
    for s in ("level_{l}_expert_layer_0_weights", "level_{l}_gate_weights", "{task}_dnn_layer_{i}_weights"):
        assert s in doc, s


def test_every_limit_raises_at_construction():
    import recman_amd.th as th

    with pytest.raises(ValueError, match=r"task_experts=0 with num_levels=2 .*task_experts 1\.\.4.*num_levels 1\.\.4"):
        th.MMoE(None, num_levels=2)
    for kw, match in ((dict(task_experts=5), "task_experts=5"), (dict(task_experts=-1), "task_experts=-1"),
                      (dict(task_experts=1, num_experts=9), "num_experts=9"),
                      (dict(task_experts=1, num_experts=0), "num_experts=0"),
                      (dict(task_experts=1, num_levels=5), "num_levels=5"),
                      (dict(task_experts=1, num_levels=0), "num_levels=0"),
                      (dict(task_experts=4, num_experts=8, task_names=tuple("abcdefg"),
                            task_types=("classification",) * 7), r"= 36 experts per level")):
        with pytest.raises(ValueError, match=match + r".*tasks x task_experts \+ num_experts <= 32"):
            th.MMoE(None, **kw)
    with pytest.raises(ValueError, match="expert_hidden_units"):
        th.PLE(None, expert_hidden_units=(30,))
    for es in (("ctr", "ctr"), ("ctr", "nope"), ("ctr",), ("ctr", "cvr", "x"), "ctr"):
        with pytest.raises(ValueError, match="entire_space=.*two distinct classification tasks"):
            th.MMoE(None, entire_space=es)
    with pytest.raises(ValueError, match="two distinct classification tasks"):
        th.PLE(None, task_types=("classification", "regression"), entire_space=("ctr", "cvr"))


def test_entire_space_front_end_pieces():
    import recman_amd.th as th
    from recman_amd.th.MMoE import entire_space_labels
    from sklearn.metrics import log_loss, roc_auc_score

    m = th.PLE(_fd(), task_names=("like", "click", "buy"), task_types=("regression", "classification",
                                                                       "classification"),
               entire_space=("click", "buy"))
    assert m.es_ == (1, 2)
    assert m.metric_names == ["like/roc_auc_score", "like/log_loss", "click/roc_auc_score", "click/log_loss",
                              "buy/roc_auc_score", "buy/log_loss", "ctcvr/roc_auc_score", "ctcvr/log_loss"]
    assert [str(x) for x in m.metrics] == m.metric_names
    nan = np.nan
    y = np.array([[0.5, 0, nan], [0.1, 1, 1], [0.2, 1, 0], [0.3, 1, nan], [0.0, nan, 1], [1.0, 0, 1], [0.7, 1, 1]])
    pr = np.array([[0, 0.5, 0.5], [0, 0.9, 0.8], [0, 0.4, 0.9], [0, 0.9, 0.9], [0, 0.1, 0.1], [0, 0.3, 0.2],
                   [0, 0.6, 0.7]])
    z, seen = entire_space_labels(y[:, 1], y[:, 2])
    assert seen.tolist() == [True, True, True, False, False, True, True] and z[seen].tolist() == [0, 1, 0, 0, 1]
    q = (pr[:, 1] * pr[:, 2])[seen]
    assert m.metrics[6](y, pr) == roc_auc_score(z[seen], q) and m.metrics[7](y, pr) == log_loss(z[seen], q)
    zt, st = entire_space_labels(torch.tensor(y[:, 1]), torch.tensor(y[:, 2]))
    assert st.tolist() == seen.tolist() and zt[st].tolist() == z[seen].tolist()
    with pytest.raises(ValueError, match="predict_ctcvr needs entire_space"):
        th.MMoE(_fd()).predict_ctcvr(None)


def test_get_params_and_clone_round_trip_the_new_arguments():
    import recman_amd.th as th

    kw = dict(task_names=("ctr", "cvr", "like"), task_types=("classification",) * 3, num_experts=3, task_experts=2,
              num_levels=3, entire_space=("ctr", "cvr"), expert_hidden_units=(16,), tower_hidden_units=(8,))
    m = th.MMoE(_fd(), **kw)
    got = m.get_params()
    for n, v in kw.items():
        assert got[n] == v, n
    c = clone(m)
    assert isinstance(c, th.MMoE) and c is not m and c.model == "ple" and c.es_ == (0, 1)
    assert all(c.get_params()[n] == v for n, v in kw.items())
    assert clone(th.MMoE(_fd())).model == "mmoe"
    for n in ("task_experts", "num_levels", "entire_space"):
        assert m.hparams[n] == kw[n]
