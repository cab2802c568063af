"""CPU: the float64 references of tests/front_refs.py against the oracle (oracle/th_layers.py) and torch.autograd of
it, and their error bounds against fp32 restatements of the same sums: the bounds must hold for honest fp32
arithmetic in more than one summation order (they are not too tight) and must be violated by a perturbation of 1e-4
of the result's scale (they are not vacuous)."""
import pytest
import torch

from oracle import th_layers as T
from recman_amd.optim import Optimizer
from tests import front_refs as R
from tests.cases import make_case

F32, F64 = torch.float32, torch.float64


def _tables(spec, p, D, bias=True):
    """The oracle's per-feature variables as the C ABI sees them: one concatenated table, field offsets, flat bias
    table, flat linear weights."""
    names = spec.sparse_names
    table = torch.cat([p[f"{n}_feat_embed"] for n in names])
    sizes = torch.tensor(spec.feat_sizes)
    field_off = torch.cumsum(sizes, 0) - sizes
    bias_t = torch.cat([p[f"{n}_feat_bias"] for n in names]).reshape(-1) if bias else None
    lin_off = torch.tensor(spec.lin_layout[0])
    return table, field_off, bias_t, p["linear_w"].reshape(-1), lin_off


def _dbl(p):
    return {k: v.double() for k, v in p.items()}


def _seq_sum32(terms, dim):
    """fp32 sum of `terms` along dim in strict left-to-right order (torch.sum's own order is pairwise)."""
    return terms.to(F32).cumsum(dim).select(dim, -1)


def _rev_sum32(terms, dim):
    return terms.to(F32).flip(dim).cumsum(dim).select(dim, -1)


@pytest.mark.parametrize("masked", [False, True])
def test_embed_fwd_ref_matches_the_oracle_layers(masked):
    spec, p, idx, dense, y, hp = make_case("deepfm", B=53, F=7, D=8, Dn=3)
    table, field_off, bias_t, lin, lin_off = _tables(spec, p, 8)
    g = torch.Generator().manual_seed(5)
    mb = me = None
    if masked:  # FMLayer dropout with keep 0.5: multipliers 0 or 2
        mb = (torch.rand(53, 7, generator=g) < 0.5).float() * 2
        me = (torch.rand(53, 7, 8, generator=g) < 0.5).float() * 2
    dense_w = lin[spec.lin_layout[1][0]:]
    r = R.embed_fwd_ref(idx, table, field_off, 8, bias=bias_t, lin=lin, lin_off=lin_off, lin_w_dense=dense_w,
                        lin_w0=p["linear_w0"], dense=dense, mask_b=mb, mask_e=me)
    p64 = _dbl(p)
    E, bias = T.feat_embedding_layer(p64, spec, idx)
    assert torch.equal(r["E"], E.float())
    masks = (None, None) if not masked else (mb.double().unsqueeze(2) / 2, me.double() / 2)
    fm = T.fm_layer(E, bias, keep=(0.5, 0.5) if masked else (1, 1), masks=masks).reshape(-1)
    torch.testing.assert_close(r["fm_logit"], fm, rtol=1e-12, atol=1e-13)
    Em = E if not masked else E * me.double()
    torch.testing.assert_close(r["fm_sum"], Em.sum(1), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(r["lin_logit"], T.linear_layer(p64, spec, idx, dense.double()).reshape(-1),
                               rtol=1e-12, atol=1e-13)
    assert r["lin_n"] == 7 + 3 + 1
    # rm_linear_fwd is the same linear term
    out, ab, n = R.linear_fwd_ref(idx, lin_off, lin, dense, dense_w, p["linear_w0"])
    assert n == 11 and torch.equal(out, r["lin_logit"]) and torch.equal(ab, r["lin_abs"])


def test_embed_fwd_ref_strides_and_fused_rows():
    """The same values whether bias / linear weight sit in their own tables at a stride or inside the row."""
    spec, p, idx, dense, y, hp = make_case("deepfm", B=31, F=5, D=8, Dn=0)
    table, field_off, bias_t, lin, lin_off = _tables(spec, p, 8)
    base = R.embed_fwd_ref(idx, table, field_off, 8, bias=bias_t, lin=lin, lin_off=lin_off)
    R_ = table.shape[0]
    assert lin_off.tolist() == field_off.tolist()  # no dense block in front: linear rows number like table rows
    fused = torch.zeros(R_, 16)
    fused[:, :8], fused[:, 8], fused[:, 9] = table, bias_t, lin[:R_]
    fr = R.embed_fwd_ref(idx, fused, field_off, 8, bias=fused.reshape(-1)[8:], bias_ld=16,
                         lin=fused.reshape(-1)[9:], lin_ld=16, lin_off=field_off)
    b3 = torch.zeros(R_ * 3)
    b3[::3] = bias_t
    st = R.embed_fwd_ref(idx, torch.cat([table, torch.ones(R_, 4)], 1), field_off, 8, bias=b3, bias_ld=3,
                         lin=lin, lin_off=lin_off)
    for k in ("E", "fm_sum", "fm_logit", "fm_logit_bound", "lin_logit", "lin_abs"):
        assert torch.equal(base[k], fr[k]) and torch.equal(base[k], st[k]), k


@pytest.mark.parametrize("masked", [False, True])
def test_embed_bwd_and_scatter_refs_match_autograd(masked):
    spec, p, idx, dense, y, hp = make_case("deepfm", B=41, F=5, D=8)
    table, field_off, bias_t, lin, lin_off = _tables(spec, p, 8)
    g = torch.Generator().manual_seed(3)
    B, F, D = 41, 5, 8
    g_fm, dE_up = torch.randn(B, generator=g), torch.randn(B, F, D, generator=g)
    mb = (torch.rand(B, F, generator=g) < 0.5).float() * 2 if masked else None
    me = (torch.rand(B, F, D, generator=g) < 0.5).float() * 2 if masked else None
    t64 = table.double().requires_grad_()
    b64 = bias_t.double().requires_grad_()
    rows = idx + field_off
    E = t64[rows]
    E.retain_grad()
    bias = b64[rows]
    bias.retain_grad()
    Em = E * me.double() if masked else E
    bm = bias * mb.double() if masked else bias
    S = Em.sum(1)
    fm = bm.sum(1) + 0.5 * (S.square() - Em.square().sum(1)).sum(1)
    ((g_fm.double() * fm).sum() + (dE_up.double() * E).sum()).backward()
    fwd = R.embed_fwd_ref(idx, table, field_off, D, bias=bias_t, mask_b=mb, mask_e=me)
    S32 = fwd["fm_sum"].float()  # fm_sum reaches the backward as the fp32 the forward stored: one rounding of S
    d_rows, ab, d_bias = R.embed_bwd_ref(fwd["E"], S32, dE_up, g_fm, mb, me)
    torch.testing.assert_close(d_rows, E.grad, rtol=0, atol=8 * R.U * float(ab.max()))
    torch.testing.assert_close(d_bias.double(), bias.grad, rtol=1e-7, atol=0)
    # dense table gradient = scatter-add of the occurrence rows
    prior = torch.randn(table.shape[0], D + 4, generator=g)
    occ = E.grad.float()
    res, sab, n, touched = R.scatter_add_ref(prior, idx, field_off, D, rows=occ)
    want = prior.double()
    want[:, :D] += torch.zeros_like(t64).index_add(0, rows.reshape(-1), occ.double().reshape(-1, D))
    torch.testing.assert_close(res, want, rtol=1e-13, atol=1e-13)
    assert torch.equal(res[:, D:], prior.double()[:, D:]) and torch.equal(res[~touched], prior.double()[~touched])
    assert int(n.max()) == int(torch.bincount(rows.reshape(-1)).max()) + 1
    # g_row form: the bias-table gradient under g_fm
    res1, _, _, _ = R.scatter_add_ref(torch.zeros(table.shape[0]), idx, field_off, 1, g_row=g_fm)
    if not masked:
        torch.testing.assert_close(res1, b64.grad, rtol=1e-12, atol=1e-13)
    # no FM term: pure pass-through, d_bias undefined
    dr, _, db = R.embed_bwd_ref(None, None, dE_up, None)
    assert torch.equal(dr, dE_up.double()) and db is None


def test_linear_dense_bwd_and_rowdot_refs_match_autograd():
    g = torch.Generator().manual_seed(7)
    gg, X = torch.randn(97, generator=g), torch.randn(97, 13, generator=g)
    w = torch.randn(13, generator=g).double().requires_grad_()
    w0 = torch.randn(1, generator=g).double().requires_grad_()
    out = X.double() @ w + w0
    (gg.double() * out).sum().backward()
    dw, ab, d0, ab0 = R.linear_dense_bwd_ref(gg, X)
    torch.testing.assert_close(dw, w.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(d0, w0.grad, rtol=1e-12, atol=1e-13)
    w32, w032 = w.detach().float(), w0.detach().float()
    r, rab = R.rowdot_ref(X, w32, w032)
    torch.testing.assert_close(r, X.double() @ w32.double() + w032.double(), rtol=1e-13, atol=1e-13)
    assert bool((rab >= r.abs() - 1e-12).all()) and bool((ab >= dw.abs() - 1e-12).all())
    dw_, ab_, _, _ = R.linear_dense_bwd_ref(gg, None)
    assert dw_.numel() == 0 and ab_.numel() == 0


@pytest.mark.parametrize("task", ["classification", "regression"])
def test_loss_ref_matches_the_oracle_and_autograd(task):
    g = torch.Generator().manual_seed(11)
    B = 4001
    z = ((torch.rand(B, generator=g) * 24 - 12).float()).double().requires_grad_()
    y = (torch.rand(B, generator=g) < 0.4).long() if task == "classification" else torch.randn(B, generator=g)
    pred = T.prediction(z, task)
    loss = T.create_loss(y, pred, task)
    loss.backward()
    p, dz, term = R.loss_point_ref(z.detach(), y, task)
    torch.testing.assert_close(p, pred.detach(), rtol=1e-12, atol=0)
    # (the oracle holds epsilon as the float64 1e-7, the reference as the fp32 constant of the graph: 1.2e-8 apart)
    torch.testing.assert_close(term.mean(), loss.detach(), rtol=1e-8, atol=0)
    torch.testing.assert_close(dz / B, z.grad, rtol=1e-7, atol=1e-12)
    if task == "classification":
        # clip region: no gradient, the loss term is -log of the clipped probability + epsilon
        zc = torch.tensor([-30.0, -20.0, 20.0, 30.0, -25.0, 25.0])
        yc = torch.tensor([0, 1, 0, 1, 1, 0])
        _, dzc, tc = R.loss_point_ref(zc, yc, task)
        assert torch.equal(dzc, torch.zeros(6, dtype=F64))
        assert bool((tc[[1, 2, 4, 5]] > 15).all()) and bool((tc[[0, 3]] < 1e-6).all())
    a, b = torch.randn(B, generator=g), torch.randn(B, generator=g)
    zz, ab = R.logit_sum_ref([(a, 1.0), (b, 2.0)])
    assert torch.equal(zz, a.double() + 2 * b.double()) and torch.equal(ab, a.double().abs() + 2 * b.double().abs())


def _csr(B, counts, V, g, with_zero=True):
    counts = torch.as_tensor(counts)
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    ids = torch.randint(0, V, (int(offsets[-1]),), generator=g)
    if with_zero and ids.numel():
        ids[::3] = 0
    return offsets, ids


def _pad(vals, pid):
    out = torch.zeros(pid.shape, dtype=vals.dtype)
    out[pid >= 0] = vals  # (row-major order of the present tags is the CSR order)
    return out


def test_pool_refs_match_the_oracle_and_autograd():
    g = torch.Generator().manual_seed(13)
    B, D, LD, V, row0 = 37, 8, 12, 19, 5
    counts = [0, 1, 4, 33] + [int(c) for c in torch.randint(0, 6, (B - 4,), generator=g)]
    offsets, ids = _csr(B, counts, V, g)
    rows = torch.randn(row0 + V, LD, generator=g)
    out, ab, cnt = R.pool_rows_ref(rows, row0, D, offsets, ids)
    sub = rows[row0:].double()
    torch.testing.assert_close(out[:, :D], T.pooled_lookup(sub[:, :D], offsets, ids), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(out[:, D:D + 1], T.pooled_lookup(sub[:, D:D + 1], offsets, ids), rtol=1e-12, atol=1e-13)
    seg = torch.repeat_interleave(torch.arange(B), offsets[1:] - offsets[:-1])
    lin = torch.zeros(B, dtype=F64).index_add(0, seg, sub[ids, D + 1] * (ids >= 1))  # T.linear_layer's multi-hot
    torch.testing.assert_close(out[:, D + 1], lin, rtol=1e-12, atol=1e-13)
    assert torch.equal(out[:, D + 2:], torch.zeros(B, LD - D - 2, dtype=F64))
    assert torch.equal(out[0], torch.zeros(LD, dtype=F64)) and cnt.tolist() == counts
    # padded form = the CSR form
    Tn, nnz = 33, int(offsets[-1])
    pid = torch.full((B, Tn), -1, dtype=torch.int64)
    pos = torch.zeros(B, Tn, dtype=torch.int64)
    recv = torch.randn(nnz + 3, LD, generator=g)
    perm = torch.randperm(nnz, generator=g)
    for b in range(B):
        s, e = int(offsets[b]), int(offsets[b + 1])
        cols = torch.randperm(Tn, generator=g)[: e - s].sort().values  # holes anywhere, list order kept
        pid[b, cols] = ids[s:e]
        pos[b, cols] = perm[s:e]
        recv[perm[s:e]] = rows[row0 + ids[s:e]]
    outp, abp, cntp = R.pool_rows_padded_ref(recv, D, pos, pid)
    torch.testing.assert_close(outp, out, rtol=1e-13, atol=1e-14)
    assert torch.equal(cntp, cnt)
    # value-weighted form: weights on the embedding and linear columns, not on the bias, slot 0 kept, no factor
    vals = torch.randn(ids.numel(), generator=g)
    outv, _, _ = R.pool_rows_ref(rows, row0, D, offsets, ids, vals)
    wv = vals.double()[:, None]
    torch.testing.assert_close(outv[:, :D], torch.zeros(B, D, dtype=F64).index_add(0, seg, sub[ids, :D] * wv))
    torch.testing.assert_close(outv[:, D], torch.zeros(B, dtype=F64).index_add(0, seg, sub[ids, D]))
    torch.testing.assert_close(outv[:, D + 1], torch.zeros(B, dtype=F64).index_add(0, seg, sub[ids, D + 1] * wv[:, 0]))
    # backward = autograd of the forward
    for vv in (None, vals):
        t = rows.double().requires_grad_()
        o, _, _ = R.pool_rows_ref(t, row0, D, offsets, ids, vv)
        d_rows, gb, gl = (torch.randn(B, D + 3, generator=g), torch.randn(B, generator=g),
                          torch.randn(B, generator=g))
        ((o[:, :D] * d_rows[:, :D].double()).sum() + (o[:, D] * gb.double()).sum()
         + (o[:, D + 1] * gl.double()).sum()).backward()
        pt, pb, pl = (torch.randn(row0 + V, D, generator=g), torch.randn(row0 + V, generator=g),
                      torch.randn(row0 + V, generator=g))
        rt, rb, rl = R.pool_rows_bwd_ref(d_rows, gb, gl, D, offsets, ids, vv, row0, pt, pb, pl)
        torch.testing.assert_close(rt[0], pt.double() + t.grad[:, :D], rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(rb[0], pb.double() + t.grad[:, D], rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(rl[0], pl.double() + t.grad[:, D + 1], rtol=1e-12, atol=1e-13)
        assert R.pool_rows_bwd_ref(d_rows, None, gl, D, offsets, ids, vv, row0, pt, pb, None)[1:] == (None, None)
        # the padded backward writes the same per-tag rows, each in its own slot
        sent = torch.full((recv.shape[0], D + 4), 7.0)
        packed = R.pack_pooled_grad_rows_ref(d_rows, gb, gl, D, pos, pid, None if vv is None else _pad(vv, pid), sent)
        acc = torch.zeros(row0 + V, D + 4, dtype=F64)
        present = pid >= 0
        acc.index_add_(0, row0 + pid[present], packed[pos[present]])
        torch.testing.assert_close(acc[:, :D + 2], t.grad[:, :D + 2], rtol=1e-12, atol=1e-13)
        assert torch.equal(packed[pos[present]][:, D + 2:], torch.zeros(nnz, 2, dtype=F64))
        unused = torch.ones(recv.shape[0], dtype=torch.bool)
        unused[pos[present]] = False
        assert int(unused.sum()) == 3 and torch.equal(packed[unused], sent[unused].double())


def test_row_helper_refs():
    g = torch.Generator().manual_seed(17)
    table = torch.randn(23, 12, generator=g)
    rows = torch.tensor([0, 22, -1, 5, 5, -1])
    out = R.gather_rows_ref(table, rows, 8)
    assert torch.equal(out[[0, 1, 3, 4]], table[[0, 22, 5, 5], :8]) and torch.equal(out[[2, 5]], torch.zeros(2, 8))
    src = torch.randn(6, 4, generator=g)
    slot = torch.randperm(6, generator=g)
    fwd = R.permute_rows_ref(src, slot, False, torch.zeros(6, 4))
    back = R.permute_rows_ref(fwd, slot, True, torch.zeros(6, 4))
    assert torch.equal(back, src) and torch.equal(fwd[2], src[slot[2]])
    d_rows, gb, gl = torch.randn(3, 2, 4, generator=g), torch.randn(3, generator=g), torch.randn(3, generator=g)
    pos = torch.tensor([4, -1, 0, 2, -1, 6])
    lm = torch.tensor([1.0, 0.0])
    sent = torch.full((7, 8), 9.0)
    pk = R.pack_grad_rows_ref(d_rows, gb, gl, lm, pos, sent)
    assert torch.equal(pk[[1, 3, 5]], sent[[1, 3, 5]])
    assert torch.equal(pk[4, :4], d_rows[0, 0]) and pk[4, 4] == gb[0] and pk[4, 5] == gl[0] and pk[2, 5] == 0
    assert torch.equal(pk[[4, 0, 2, 6], 6:], torch.zeros(4, 2))
    assert torch.equal(R.pack_grad_rows_ref(d_rows, None, None, None, pos, sent)[[4, 0, 2, 6], 4:], torch.zeros(4, 4))


@pytest.mark.parametrize("kind", ["adam", "adagrad", "sgd"])
def test_dense_opt_ref_matches_the_per_tensor_optimizer(kind):
    g = torch.Generator().manual_seed(19)
    p0 = torch.randn(301, generator=g)
    grads = [torch.randn(301, generator=g) for _ in range(3)]
    opt = Optimizer(kind, 0.01)
    params = {"w": p0.double().clone()}
    fresh_v = torch.full((301,), 0.1) if kind == "adagrad" else torch.zeros(301)
    p, m, v = p0, torch.zeros(301), fresh_v
    for step, gr in enumerate(grads, 1):
        opt.step(params, {"w": gr.double()})
        p, m, v = R.dense_opt_ref(p, gr, m, v, step, kind, 0.01)
        # (the reference takes the hyper-parameters as the fp32 the ABI carries: 0.9f differs from 0.9 by 2.6e-8)
        torch.testing.assert_close(p, params["w"], rtol=0, atol=1e-8)
    # reset ignores the stored moments: equal to a first step from fresh state, whatever is stored
    junk = torch.full((301,), 123.0)
    a = R.dense_opt_ref(p0, grads[0], junk, junk, 7, kind, 0.01, reset=True)   # ... and whatever the step number
    b = R.dense_opt_ref(p0, grads[0], torch.zeros(301), fresh_v, 1, kind, 0.01)
    torch.testing.assert_close(a[0], b[0], rtol=0, atol=1e-9)


def test_elementwise_refs():
    x = torch.tensor([[-1.5, -0.0, 0.0, 2.0]])
    b = torch.tensor([0.5, 0.0, -0.0, -2.0])
    R.assert_bits(R.bias_act_ref32(x, b, "relu"), torch.zeros(1, 4), "relu")
    lk = R.bias_act_ref32(x, b, "leaky_relu")
    assert lk[0, 0] == torch.tensor(-1.0) * torch.tensor(0.2) and lk.dtype == F32
    R.assert_bits(R.bias_act_ref32(x, None, "identity"), torch.tensor([[-1.5, 0.0, 0.0, 2.0]]), "NULL bias adds +0.0")
    da = torch.tensor([[3.0, -3.0, 3.0, 3.0]])
    a = torch.tensor([[1.0, -0.0, 0.0, -1.0]])
    R.assert_bits(R.act_bwd_ref32(da, a, "relu"), torch.tensor([[3.0, -0.0, 0.0, 0.0]]), "relu'")
    R.assert_bits(R.act_bwd_ref32(da, a, "leaky_relu"), da * torch.tensor([[1, .2, .2, .2]]), "leaky'")
    with pytest.raises(AssertionError):
        R.assert_bits(torch.tensor([0.0]), torch.tensor([-0.0]), "signed zero")


# ---------------------------------------------------------------------------------------------------------------
# the bounds against fp32 restatements
def _check_bound(restatements, ref, bound, what, bite=1e-4, scale=None):
    """Every fp32 restatement inside the bound; and the bound is not vacuous: it stays below `bite` (1e-4) of the
    result's scale, so a value off by that much - far less than a dropped term or a wrong tail - cannot pass.
    scale: for sums over a batch, whose random-signed terms cancel to sqrt(n) of sum|terms|, the size of the largest
    sum|terms| is the yardstick (a dropped sweep or block loses a share of the TERMS)."""
    worst = 0.0
    for i, got in enumerate(restatements):
        worst = max(worst, R.assert_within(got, ref, bound, f"{what} (fp32 restatement {i})"))
    scale = float(ref.abs().max()) if scale is None else float(scale)
    b = torch.as_tensor(bound, dtype=F64)
    assert float(b.max()) < bite * scale, f"{what}: bound {float(b.max()):.3e} vs scale {scale:.3e}"
    with pytest.raises(AssertionError):
        R.assert_within(ref + bite * scale, ref, bound, what)
    return worst


@pytest.mark.parametrize("F,D", [(1, 4), (9, 64), (27, 32), (40, 256)])
@pytest.mark.parametrize("masked", [False, True])
def test_fp32_embed_forward_stays_inside_its_bounds(F, D, masked):
    B = 211
    spec, p, idx, dense, y, hp = make_case("deepfm", B=B, F=F, D=D, Dn=13, scale=0.3)
    table, field_off, bias_t, lin, lin_off = _tables(spec, p, D)
    g = torch.Generator().manual_seed(F)
    mb = (torch.rand(B, F, generator=g) < 0.8).float() / 0.8 if masked else None
    me = (torch.rand(B, F, D, generator=g) < 0.8).float() / 0.8 if masked else None
    dense_w = lin[spec.lin_layout[1][0]:]
    r = R.embed_fwd_ref(idx, table, field_off, D, bias=bias_t, lin=lin, lin_off=lin_off, lin_w_dense=dense_w,
                        lin_w0=p["linear_w0"], dense=dense, mask_b=mb, mask_e=me)
    rows = idx + field_off
    m = table[rows] * me if masked else table[rows]          # fp32 throughout from here
    b = bias_t[rows] * mb if masked else bias_t[rows]
    fm32, S32 = [], []
    for ssum in (lambda t, d: t.sum(d), _seq_sum32, _rev_sum32):
        S = ssum(m, 1)
        S32.append(S)
        apart = ssum(S * S, 1) - ssum(ssum(m * m, 1), 1)     # the two sums apart: the order with the most cancellation
        fm32.append(ssum(b, 1) + 0.5 * apart)
        fm32.append(ssum(b, 1) + 0.5 * ssum(S * S - ssum(m * m, 1), 1))
    _check_bound(S32, r["fm_sum"], R.sum_bound(F, r["fm_sum_abs"]), "fm_sum")
    # (the outer sum has n = D (F + 1) + F terms, 10 538 at F = 40, D = 256: the any-order bound is 6e-4 of the sum of
    # its |terms| there, which is why the bite of this one is 1e-2 of the scale, still far below a dropped field)
    _check_bound(fm32, r["fm_logit"], r["fm_logit_bound"], "fm_logit", bite=1e-2)
    lt = torch.cat([lin[idx + lin_off], dense * dense_w, p["linear_w0"].expand(B, 1)], 1)
    _check_bound([lt.sum(1), _seq_sum32(lt, 1), _rev_sum32(lt, 1)], r["lin_logit"],
                 R.sum_bound(r["lin_n"], r["lin_abs"]), "lin_logit")


def test_fp32_backward_sums_stay_inside_their_bounds():
    g = torch.Generator().manual_seed(23)
    B, F, D = 3001, 5, 8
    spec, p, idx, dense, y, hp = make_case("deepfm", B=B, F=F, D=D, Dn=13)
    table, field_off, bias_t, lin, lin_off = _tables(spec, p, D)
    me = (torch.rand(B, F, D, generator=g) < 0.8).float() / 0.8
    fwd = R.embed_fwd_ref(idx, table, field_off, D, mask_e=me)
    S32 = (table[idx + field_off] * me).sum(1)
    g_fm, dE_up = torch.randn(B, generator=g), torch.randn(B, F, D, generator=g)
    d_rows, ab, _ = R.embed_bwd_ref(fwd["E"], S32, dE_up, g_fm, None, me)
    e32 = fwd["E"] * me
    got = dE_up + g_fm[:, None, None] * me * (S32[:, None, :] - e32)
    _check_bound([got], d_rows, R.sum_bound(R.EMBED_BWD_N, ab), "embed_bwd")
    # scatter: a hot row takes a whole field's occurrences (n = B + 1)
    hot = idx.clone()
    hot[:, 2] = 1
    prior = torch.randn(table.shape[0], D, generator=g)
    res, sab, n, touched = R.scatter_add_ref(prior, hot, field_off, D, rows=got)
    assert int(n.max()) == B + 1
    rows = (hot + field_off).reshape(-1)
    fwd_order = prior.clone().index_add_(0, rows, got.reshape(-1, D))
    rev = prior.clone().index_add_(0, rows.flip(0), got.reshape(-1, D).flip(0))
    _check_bound([fwd_order, rev], res, R.sum_bound(n, sab), "scatter_add_rows", bite=1e-3, scale=sab.max())
    # column sums over the batch (n = B) and row dots (n = P + 1)
    X = torch.randn(B, 400, generator=g)
    dw, dab, d0, d0ab = R.linear_dense_bwd_ref(g_fm, X)
    t = g_fm[:, None] * X
    _check_bound([t.sum(0), _seq_sum32(t, 0), _rev_sum32(t, 0)], dw, R.sum_bound(B, dab), "linear_dense_bwd", bite=1e-3, scale=dab.max())
    _check_bound([g_fm.sum().reshape(1), _seq_sum32(g_fm, 0).reshape(1)], d0, R.sum_bound(B, d0ab), "d_w0", bite=1e-3, scale=d0ab.max())
    w, w0 = torch.randn(400, generator=g), torch.randn(1, generator=g)
    out, oab = R.rowdot_ref(X, w, w0)
    t = torch.cat([X * w, w0.expand(B, 1)], 1)
    _check_bound([t.sum(1), _seq_sum32(t, 1), _rev_sum32(t, 1), X @ w + w0], out, R.sum_bound(401, oab), "rowdot")


def test_fp32_pooling_stays_inside_its_bound():
    g = torch.Generator().manual_seed(29)
    B, D, LD, V = 501, 16, 20, 50
    offsets, ids = _csr(B, torch.randint(0, 34, (B,), generator=g), V, g)
    rows, vals = torch.randn(V, LD, generator=g), torch.randn(int(offsets[-1]), generator=g)
    out, ab, cnt = R.pool_rows_ref(rows, 0, D, offsets, ids, vals)
    seg = torch.repeat_interleave(torch.arange(B), offsets[1:] - offsets[:-1])
    t = rows[ids].clone()
    t[:, :D] *= vals[:, None]
    t[:, D + 1] *= vals
    t[:, D + 2:] = 0
    got = torch.zeros(B, LD).index_add_(0, seg, t)
    rev = torch.zeros(B, LD).index_add_(0, seg.flip(0), t.flip(0))
    _check_bound([got, rev], out, R.sum_bound(cnt[:, None], ab), "pool_rows (vals)")


def test_fp32_sqrtn_backward_stays_inside_its_bound():
    """The sqrtn backward: every term is a product with the fp32 rsqrt of the tag count (n + RSQRT_TERMS), thousands
    of occurrences per row."""
    g = torch.Generator().manual_seed(37)
    B, D, V = 20_011, 8, 10
    offsets, ids = _csr(B, torch.randint(0, 6, (B,), generator=g), V, g)
    d_rows, gb, gl = torch.randn(B, D, generator=g), torch.randn(B, generator=g), torch.randn(B, generator=g)
    prior = torch.randn(V, D, generator=g), torch.randn(V, generator=g), torch.randn(V, generator=g)
    (res, ab, n), (rb, abb, nb), _ = R.pool_rows_bwd_ref(d_rows, gb, gl, D, offsets, ids, None, 0, *prior)
    assert int(n.min()) > 3000
    cnt = offsets[1:] - offsets[:-1]
    seg = torch.repeat_interleave(torch.arange(B), cnt)
    inv = cnt.float().rsqrt()[seg]
    t, tb = d_rows[seg] * inv[:, None], gb[seg] * inv
    got = [prior[0].clone().index_add_(0, ids, t), prior[0].clone().index_add_(0, ids.flip(0), t.flip(0))]
    gotb = [prior[1].clone().index_add_(0, ids, tb), prior[1].clone().index_add_(0, ids.flip(0), tb.flip(0))]
    _check_bound(got, res, R.sum_bound(n + R.RSQRT_TERMS, ab), "pool_rows_bwd sqrtn d_table", bite=1e-2, scale=ab.max())
    _check_bound(gotb, rb, R.sum_bound(nb + R.RSQRT_TERMS, abb), "pool_rows_bwd sqrtn d_bias", bite=1e-2, scale=abb.max())


def test_fp32_loss_restatement_meets_the_tolerances():
    """The body (|z| <= 12) at the project's tolerance: pred against the float64 sigmoid, the loss and the gradient
    against the float64 function of the fp32 probability; in the clip region (|z| >= 20) dlogit exactly 0."""
    g = torch.Generator().manual_seed(31)
    B = 100_003
    z = (torch.rand(B, generator=g) * 24 - 12).float()
    y = (torch.rand(B, generator=g) < 0.5).float()
    p = 1.0 / (1.0 + torch.exp(-z))                       # fp32 restatement of the per-example arithmetic
    eps = torch.tensor(1e-7)
    pc = p.clamp(eps, 1 - eps)
    a, c = pc + eps, 1 - pc + eps
    dz = -(y / a - (1 - y) / c) * p * (1 - p)
    term = -(y * torch.log(a) + (1 - y) * torch.log(c))
    p64, dz_z, t_z = R.loss_point_ref(z, y, "classification")
    R.close(p, p64, what="pred")
    _, dz64, t64 = R.loss_point_ref(z, y, "classification", pred=p)
    R.close(dz, dz64, what="dz from the fp32 probability")
    R.close(term.mean(), t64.mean(), what="loss from the fp32 probability")
    print(f"fp32 vs float64-from-z: max |dz err| {float((dz.double() - dz_z).abs().max()):.3e}, "
          f"|loss err| {abs(float(term.double().mean() - t_z.mean())):.3e}")
    zc = torch.cat([20 + torch.rand(500, generator=g) * 20, -20 - torch.rand(500, generator=g) * 20]).float()
    yc = (torch.rand(1000, generator=g) < 0.5).float()
    pcl = 1.0 / (1.0 + torch.exp(-zc))
    _, dzc, tc = R.loss_point_ref(zc, yc, "classification", pred=pcl)
    assert torch.equal(dzc, torch.zeros(1000, dtype=F64))
    pcc = pcl.clamp(eps, 1 - eps)
    t32 = -(yc * torch.log(pcc + eps) + (1 - yc) * torch.log(1 - pcc + eps))
    R.close(t32, tc, what="clip-region loss terms")
