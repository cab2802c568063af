"""CPU: tests/step_ref.py - the float64 restatement of rm_deepfm_step that tests/test_gpu_step_kernel.py holds the
kernel to - pinned against the model oracle (oracle/th_layers.py on .double() parameters, every l2 factor 0), its
packed re-indexing inverted, and the kink selection of every GPU case run without a GPU."""
import pytest
import torch

from oracle import th_layers as T
from tests import step_ref as SR

F64 = torch.float64

# B, F, Dn, H0, H1, table_ld, act, task: an odd H0, an odd H1, Dn = 0, both tasks, every activation, one field, a
# ragged Dn, the Criteo shape
SHAPES = [
    (37, 5, 3, 32, 32, 20, "relu", "classification"),
    (21, 4, 0, 17, 8, 24, "leaky_relu", "regression"),
    (19, 7, 16, 8, 5, 32, "relu", "regression"),
    (33, 26, 13, 31, 1, 36, "leaky_relu", "classification"),
    (5, 1, 1, 1, 32, 20, "identity", "classification"),
    (40, 26, 0, 32, 32, 32, "identity", "regression"),
]


def _rel(got, want, what, rtol=1e-12):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= rtol * scale, f"{what}: {err:.3e} against {scale:.3e}"


@pytest.mark.parametrize("B,F,Dn,H0,H1,ld,act,task", SHAPES)
def test_step_ref_equals_the_model_oracle_in_float64(B, F, Dn, H0, H1, ld, act, task):
    c = SR.make_step_case(B, F, Dn, H0, H1, table_ld=ld, act=act, task=task, seed=7)
    r = SR.ref_of(c)
    p64 = {k: v.double() for k, v in c.p.items()}
    y = c.y.double() if c.y.is_floating_point() else c.y
    dense = c.dense.double() if Dn else torch.zeros(B, 0, dtype=F64)
    loss, logit, pred, grads = T.fwd_bwd("deepfm", p64, c.spec, c.idx, dense, y, c.hp, task=task)
    _rel(r["logit"], logit, "logit")
    _rel(r["pred"], pred, "pred")
    _rel(r["loss"], loss.reshape(1), "loss")
    # the tables: the oracle's dense table gradients are the per-occurrence rows summed by id, the way the engine
    # fuses [embedding | bias entry | linear weight] into one row
    lin_offs, dense_offs, L = c.spec.lin_layout
    d_lin = torch.zeros(L, dtype=F64)
    for f, (n, V) in enumerate(zip(c.spec.sparse_names, c.spec.feat_sizes)):
        ids = c.idx[:, f]
        _rel(torch.zeros(V, SR.D, dtype=F64).index_add(0, ids, r["d_rows"][:, f]), grads[f"{n}_feat_embed"],
             f"table {n}")
        _rel(torch.zeros(V, dtype=F64).index_add(0, ids, r["dlogit"]), grads[f"{n}_feat_bias"][:, 0], f"bias {n}")
        d_lin.index_add_(0, lin_offs[f] + ids, r["dlogit"])
    if Dn:
        d_lin[torch.tensor(dense_offs)] += r["d_lin_w_dense"]
    else:
        assert r["d_lin_w_dense"] is None
    _rel(d_lin, grads["linear_w"][:, 0], "linear_w")
    _rel(r["d_lin_w0"], grads["linear_w0"], "linear_w0")
    for i in range(2):
        _rel(r[f"dW{i}"], grads[f"dnn_layer_{i}_weights"], f"dW{i}")
        _rel(r[f"db{i}"], grads[f"dnn_layer_{i}_bias"], f"db{i}")
    _rel(r["d_w_out"], grads["dnn_w"][:, 0], "dnn_w")
    _rel(r["d_w0_out"], grads["dnn_w0"], "dnn_w0")
    assert set(grads) == ({f"{n}_feat_{s}" for n in c.spec.sparse_names for s in ("embed", "bias")}
                          | {"linear_w", "linear_w0", "dnn_w", "dnn_w0"}
                          | {f"dnn_layer_{i}_{s}" for i in range(2) for s in ("weights", "bias")})


def test_step_ref_grad_scale_scales_every_gradient_and_not_the_loss():
    c = SR.make_step_case(21, 4, 2, 17, 8, act="leaky_relu", task="classification", seed=7)
    a, b = SR.ref_of(c), SR.ref_of(c, grad_scale=0.25)
    for k in ("logit", "pred", "loss"):
        assert torch.equal(a[k], b[k]), k
    for k in ("dlogit", "d_rows") + SR.PARAM_GRADS:
        _rel(b[k], 0.25 * a[k], k)


def test_step_ref_does_not_depend_on_the_row_stride_or_the_padding():
    c = SR.make_step_case(19, 7, 16, 8, 5, table_ld=20, act="relu", task="regression", seed=7)
    a = SR.ref_of(c)
    for ld in (24, 36):
        w = SR.with_stride(c, ld)
        assert w.rows.shape[1] == ld and bool(torch.isnan(w.rows[:, SR.COLS:]).all())
        b = SR.ref_of(w)
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_kink_rule_is_the_one_of_the_steady_state_tests():
    from tests.test_gpu_steady_state import _kink_clear

    g = torch.Generator().manual_seed(1)
    z0 = torch.randn(500, 7, generator=g, dtype=F64)
    terms = torch.rand(500, 7, generator=g, dtype=F64)
    for K in (1, 21, 429):
        z = z0 * 20 * (K + 1) * 2.0 ** -24   # (a fair share of the rows on either side of the rule)
        want = _kink_clear(z, terms, K)
        assert 0 < int(want.sum()) < 500
        assert torch.equal(SR.kink_clear(z, terms, K), want)


@pytest.mark.parametrize("mask", ["none", "ones", "mixed"])
def test_packed_reindexing_inverts(mask):
    c = SR.make_step_case(37, 5, 0, 17, 3, act="relu", task="classification", seed=7)
    r = SR.ref_of(c)
    n = c.B * c.F + SR.PACKED_SPARE
    pos = SR.packed_positions(c.B, c.F, n, seed=3)
    assert pos.unique().numel() == c.B * c.F and int(pos.max()) < n
    m = SR.lin_masks(c.F)[mask]
    buf = SR.pack_ref(r["d_rows"], r["dlogit"], pos, n, m)
    used = torch.zeros(n, dtype=torch.bool)
    used[pos.reshape(-1)] = True
    assert int(used.sum()) == c.B * c.F and bool(torch.isnan(buf[~used]).all()) and not bool(torch.isnan(buf[used]).any())
    d_rows, g_bias, g_lin, pad = SR.unpack_ref(buf, pos)
    g = r["dlogit"].reshape(-1, 1).expand(c.B, c.F)
    assert torch.equal(d_rows, r["d_rows"]) and torch.equal(g_bias, g)
    assert torch.equal(g_lin, g if m is None else g * m.double())
    assert torch.equal(pad, torch.zeros_like(pad))
    if mask == "mixed":
        assert bool((g_lin[:, m == 0] == 0).all()) and torch.equal(g_lin[:, m == 1], g[:, m == 1])


def test_case_lists_cover_what_the_gpu_file_says_they_cover():
    fdn = SR.SLOT_FDN
    assert [F for F, _ in fdn[:26]] == list(range(1, 27)) and {Dn for _, Dn in fdn} == set(range(17))
    assert all(Dn > 0 for F, Dn in fdn if F in (6, 13, 20, 22, 23, 24, 25))
    assert (26, 0) in fdn and (26, 16) in fdn
    for j, F in enumerate((26, 3)):
        cs = [k for k in SR.WIDTH_CASES if k["F"] == F]
        assert [(k["H0"], k["H1"]) for k in cs] == [(H, 33 - H) for H in range(1, 33)]
    for cases in (SR.SLOT_CASES, SR.WIDTH_CASES):
        assert {(k["act"], k["task"]) for k in cases} == {(a, t) for a in SR.ACTS for t in SR.TASKS}
    assert len({k["seed"] for k in SR.GPU_CASES}) == len(SR.GPU_CASES)


@pytest.mark.parametrize("kw", SR.GPU_CASES, ids=lambda k: "B{B}F{F}Dn{Dn}H{H0}x{H1}".format(**k))
def test_every_gpu_case_finds_its_kink_clear_examples(kw):
    """The cap check of make_step_case (it asserts that B of the B + B // 2 examples drawn are clear), run here for
    every case tests/test_gpu_step_kernel.py builds, with the same seeds."""
    c = SR.make_step_case(**kw)
    assert c.idx.shape == (kw["B"], kw["F"]) and c.y.shape == (kw["B"],)
    assert (c.dense is None) == (kw["Dn"] == 0)
    assert int((c.idx + c.field_off).max()) < c.rows.shape[0] and int(c.idx.min()) >= 0
