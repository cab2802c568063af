"""Plain float64 references and error bounds for the small kernels that run before and after the big ones
(csrc/embed.hip, loss.hip, pool.hip, route.hip and dense_opt_kernel of optim.hip).  Test infrastructure, like
tests/cases.py: tests/test_front_refs.py checks it on the CPU, tests/test_gpu_front_kernels.py uses it on the GPU.

Every function restates a contract of include/recman_hip.h in torch, in float64, on whatever device its inputs
live on, from the SAME fp32 inputs the kernel gets (widened, never re-rounded).  Nothing here is derived from the
kernels' code: no chunking, no lane mapping, no launch arithmetic.

Bounds.  A reference that sums returns, next to the value, the float64 sum of the |terms| of every output element.
n products summed in fp32 in ANY order, with or without FMA, differ from the exact sum by at most

    (n + 2) * 2^-24 * sum|terms|                                                    (sum_bound)

(n - 1 additions and one product rounding per term, to first order in u = 2^-24, plus a slack of 2 for a final scale
or bias; the second-order terms are below n u times the first-order ones, 1e-5 of the bound at n = 200).  It holds
for float atomics and for two-stage reductions alike.  The n of every use is stated where the bound is called.

fm_logit nests two sums and the bound is applied to both: S_k = sum_f m_fk (m = mask_e * E) carries
(F + 2) u A_k with A_k = sum_f |m_fk|; squaring it moves 0.5 S_k^2 by |S_k| times that; and the outer sum
(D S_k^2 terms, F D squares m_fk^2, F bias terms: n = D (F + 1) + F) carries (n + 2) u times the sum of its |terms|,
0.5 sum_k (S_k^2 + sum_f m_fk^2) + sum_f |mask_b bias|:

    fm_logit bound = u * [ (F + 2) sum_k |S_k| A_k  +  (D (F + 1) + F + 2) (0.5 sum_k (S_k^2 + Q_k) + sum_f |b_f|) ]

Outputs that pass through expf, logf or rsqrtf (pred, dlogit, loss, the sqrtn factor) are not covered by such a
bound: they are compared at the project's tolerance for them (tests/test_gpu_parity.py::_close, rtol 1e-5, atol 1e-6).
"""
import math

import torch

U = 2.0 ** -24
F64 = torch.float64
KERAS_EPS32 = float(torch.tensor(1e-7, dtype=torch.float32))  # Keras backend epsilon() as the fp32 graph holds it
KERAS_HI32 = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-7, dtype=torch.float32))  # 1 - 2^-23


def sum_bound(n, sum_abs):
    """(n + 2) 2^-24 sum|terms|: n may be a number or a tensor broadcastable against sum_abs."""
    return (n + 2) * U * sum_abs


RATIOS = {}  # kernel name -> largest observed |error| / bound over every check made in this process


def assert_within(got, ref, bound, what, key=None):
    """Every element of `got` within `bound` of the float64 `ref`; records the largest error / bound ratio under
    `key`.  Where the bound is 0 (no terms) the value must be exact."""
    got, ref, bound = got.detach().to(F64), ref.detach().to(F64), torch.as_tensor(bound, dtype=F64, device=ref.device)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    bound = bound.expand_as(err)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    bad = err > bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    if key is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    if bool(bad.any()):
        i = int((err - bound).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at flat "
                             f"index {i}: got {got.reshape(-1)[i]:.9e} want {ref.reshape(-1)[i]:.9e} bound "
                             f"{bound.reshape(-1)[i]:.3e} (largest err/bound {ratio:.3f})")
    return ratio


def assert_bits(got, want, what):
    """Bit for bit (distinguishes -0.0 from 0.0, which torch.equal does not)."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    view = {torch.float32: torch.int32, torch.float64: torch.int64}.get(got.dtype)
    a, b = (got.view(view), want.view(view)) if view is not None else (got, want)
    if not torch.equal(a, b):
        ne = (a != b).reshape(-1)
        i = int(ne.nonzero()[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in bits; first at flat index {i}: "
                             f"got {got.reshape(-1)[i].item()!r} want {want.reshape(-1)[i].item()!r}")


def close(got, want, rtol=1e-5, atol=1e-6, what=""):
    """tests/test_gpu_parity.py::_close, device-agnostic: max |err| <= atol + rtol * max(1, max|want|)."""
    got, want = got.detach().to(F64), want.detach().to(F64)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= atol + rtol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e})"


# ------------------------------------------------------------------------------------------------ embedding forward
def embed_fwd_ref(idx, table, field_off, D, *, bias=None, bias_ld=1, lin=None, lin_ld=1, lin_off=None,
                  lin_w_dense=None, lin_w0=None, dense=None, mask_b=None, mask_e=None):
    """rm_embed_fwd.  table [R, table_ld] (the row's first D floats are the embedding); bias / lin: FLAT fp32
    tensors, element r at bias[r * bias_ld] resp. (lin_off[f] + i) * lin_ld - for a fused row pass
    table.reshape(-1)[D:] resp. [D + 1:] with the table's ld.  Returns a dict:
      E [B,F,D] fp32 (pure data movement: compare bit for bit),
      fm_sum [B,D] + fm_sum_abs (n = F),  fm_logit [B] + fm_logit_bound (the nested bound of the module docstring;
      bias absent: its terms are 0),  lin_logit [B] + lin_abs (n = F + Dn + 1; lin absent: the dense part and w0)."""
    B, F = idx.shape
    g = idx + field_off  # global rows [B,F]
    E = table[g][..., :D]
    m = E.to(F64)
    if mask_e is not None:
        m = m * mask_e.to(F64)
    S = m.sum(1)
    A = m.abs().sum(1)
    Q = m.square().sum(1)
    out = dict(E=E.contiguous(), fm_sum=S, fm_sum_abs=A)
    bsum = torch.zeros(B, dtype=F64, device=idx.device)
    babs = torch.zeros_like(bsum)
    if bias is not None:
        b = bias[g * bias_ld].to(F64)
        if mask_b is not None:
            b = b * mask_b.to(F64)
        bsum, babs = b.sum(1), b.abs().sum(1)
    out["fm_logit"] = bsum + 0.5 * (S.square() - Q).sum(1)
    out["fm_logit_bound"] = U * ((F + 2) * (S.abs() * A).sum(1)
                                 + (D * (F + 1) + F + 2) * (0.5 * (S.square() + Q).sum(1) + babs))
    l = torch.zeros(B, dtype=F64, device=idx.device)
    labs = torch.zeros_like(l)
    if lin is not None:
        w = lin[(idx + lin_off) * lin_ld].to(F64)
        l, labs = w.sum(1), w.abs().sum(1)
    if dense is not None and dense.shape[1] > 0:
        t = dense.to(F64) * lin_w_dense.to(F64)
        l, labs = l + t.sum(1), labs + t.abs().sum(1)
    if lin_w0 is not None:
        l, labs = l + lin_w0.to(F64), labs + lin_w0.to(F64).abs()
    out["lin_logit"], out["lin_abs"] = l, labs
    out["lin_n"] = F + (0 if dense is None else dense.shape[1]) + 1
    return out


def linear_fwd_ref(idx, lin_off, w, dense, w_dense, w0):
    """rm_linear_fwd: (out [B], sum|terms| [B], n = F + Dn + 1)."""
    B = dense.shape[0] if idx is None else idx.shape[0]
    dev = dense.device if idx is None else idx.device
    out = torch.zeros(B, dtype=F64, device=dev)
    ab = torch.zeros_like(out)
    n = 1
    if idx is not None and idx.shape[1] > 0:
        t = w[idx + lin_off].to(F64)
        out, ab, n = out + t.sum(1), ab + t.abs().sum(1), n + idx.shape[1]
    if dense is not None and dense.shape[1] > 0:
        t = dense.to(F64) * w_dense.to(F64)
        out, ab, n = out + t.sum(1), ab + t.abs().sum(1), n + dense.shape[1]
    if w0 is not None:
        out, ab = out + w0.to(F64), ab + w0.to(F64).abs()
    return out, ab, n


# ------------------------------------------------------------------------------------- embedding backward, scatter
EMBED_BWD_N = 6  # per element: 3 terms (dE_up, g mk S, g mk mk E), each at most 3 products deep, 2 additions


def embed_bwd_ref(E, fm_sum, dE_up, g_fm, mask_b=None, mask_e=None):
    """rm_embed_bwd: d_rows = dE_up + g_fm * mask_e * (S - mask_e * E), d_bias = g_fm * mask_b.
    Returns (d_rows f64 [B,F,D], sum|terms| - use n = EMBED_BWD_N -, d_bias fp32 or None).  g_fm None: d_rows is
    dE_up itself (data movement) and d_bias is not defined (the kernel leaves the buffer alone).  d_bias is ONE fp32
    product (or a copy): returned in fp32 for a bit-for-bit comparison."""
    if g_fm is None:
        return dE_up.to(F64), dE_up.to(F64).abs(), None
    g = g_fm.to(F64)[:, None, None]
    e, s = E.to(F64), fm_sum.to(F64)[:, None, :]
    mk = torch.ones((), dtype=F64, device=E.device) if mask_e is None else mask_e.to(F64)
    t1, t2 = g * mk * s, g * mk * mk * e
    up = torch.zeros_like(e) if dE_up is None else dE_up.to(F64)
    B, F, _ = E.shape
    d_bias = g_fm[:, None].expand(B, F).contiguous() if mask_b is None else g_fm[:, None] * mask_b
    return up + t1 - t2, up.abs() + t1.abs() + t2.abs(), d_bias


def scatter_add_ref(prior, idx, field_off, width, *, rows=None, g_row=None):
    """rm_scatter_add_rows into prior [R, ld] (or [R] with ld 1): (result f64, sum|terms| incl. the prior content,
    n per element = multiplicity of the row + 1 (the prior content is one more term), touched [R] bool).  Rows that no
    occurrence touches must keep their bits; so must the columns >= width of every row."""
    B, F = idx.shape
    p2 = prior.reshape(prior.shape[0], -1)
    g = (idx + field_off).reshape(-1)
    if g_row is not None:
        vals = g_row.to(F64)[:, None].expand(B, F).reshape(-1, 1)
    else:
        vals = rows.to(F64).reshape(B * F, width)
    res, ab = p2.to(F64).clone(), p2.to(F64).abs()
    res[:, :width] = res[:, :width].index_add(0, g, vals)
    ab[:, :width] = ab[:, :width].index_add(0, g, vals.abs())
    mult = torch.bincount(g, minlength=p2.shape[0])
    n = (mult + 1)[:, None].expand_as(res)
    return res.reshape(prior.shape), ab.reshape(prior.shape), n.reshape(prior.shape), mult > 0


def linear_dense_bwd_ref(g, dense):
    """rm_linear_dense_bwd: (d_w [Dn], its sum|terms|, d_w0 [1], its sum|terms|); n = B for both."""
    g64 = g.to(F64)
    if dense is None or dense.shape[1] == 0:
        dw = ab = torch.zeros(0, dtype=F64, device=g.device)
    else:
        dw, ab = g64 @ dense.to(F64), g64.abs() @ dense.to(F64).abs()
    return dw, ab, g64.sum().reshape(1), g64.abs().sum().reshape(1)


# --------------------------------------------------------------------------------------------------------- loss
def logit_sum_ref(branches):
    """The branch sum of rm_logit_loss: (logit f64 [B], sum|terms|); n = number of branches."""
    z = sum(float(torch.tensor(c, dtype=torch.float32)) * t.to(F64) for t, c in branches)
    ab = sum(abs(float(torch.tensor(c, dtype=torch.float32))) * t.to(F64).abs() for t, c in branches)
    return z, ab


def loss_point_ref(z, t, task, pred=None):
    """PredictionLayer + create_loss of one example in float64 (Keras binary_crossentropy on PROBABILITIES: clip to
    [eps, 1 - eps] with the gradient passing only inside, epsilon inside the logs; eps and 1 - eps are the fp32
    constants of the graph, 1 - eps = 1 - 2^-23) or MSE.  z: the summed logit; t: labels, any dtype.
    Returns (pred, dz = d term / d z - NOT divided by B -, term).  pred given (the fp32 probabilities a kernel
    wrote, widened): the loss and the gradient are taken from THEM, as Keras does from its fp32 sigmoid output -
    1 - p is quantised to 2^-24, 0.5 % of it at |z| = 12, which a float64 sigmoid does not reproduce."""
    z, t = z.to(F64), t.to(F64)
    if task != "classification":
        e = z - t
        return z, 2 * e, e * e
    p = torch.sigmoid(z) if pred is None else pred.to(F64)
    pc = p.clamp(KERAS_EPS32, KERAS_HI32)
    a, c = pc + KERAS_EPS32, 1 - pc + KERAS_EPS32
    inside = (p >= KERAS_EPS32) & (p <= KERAS_HI32)
    dp = torch.where(inside, -(t / a - (1 - t) / c), torch.zeros_like(p))
    return p, dp * p * (1 - p), -(t * torch.log(a) + (1 - t) * torch.log(c))


def rowdot_ref(X, w, w0=None):
    """rm_rowdot: (out [B], sum|terms| [B]); n = P + 1."""
    X64, w64 = X.to(F64), w.to(F64)
    out, ab = X64 @ w64, X64.abs() @ w64.abs()
    if w0 is not None:
        out, ab = out + w0.to(F64), ab + w0.to(F64).abs()
    return out, ab


# ------------------------------------------------------------------- elementwise fp32 (bit for bit, no reassociation)
def _slope(a, act):
    one = torch.ones_like(a)
    if act == "relu":
        return torch.where(a > 0, one, torch.zeros_like(a))
    if act == "leaky_relu":
        return torch.where(a > 0, one, torch.full_like(a, 0.2))
    return one


def bias_act_ref32(x, bias, act):
    """rm_bias_act in fp32: one add, one select (leaky: one multiply by fp32(0.2) on the other side of the select).
    bias None is a bias of +0.0 (include/recman_hip.h): the add still happens, so x = -0.0 comes out as +0.0."""
    v = x + (torch.zeros((), dtype=x.dtype, device=x.device) if bias is None else bias)
    if act == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == "leaky_relu":
        return torch.where(v > 0, v, torch.full_like(v, 0.2) * v)
    return v


def act_bwd_ref32(da, a, act):
    """rm_act_bwd in fp32: da * act'(a), act' in {1, 0 or fp32(0.2)} read off the post-activation value a."""
    return da * _slope(a, act)


# ------------------------------------------------------------------------------------------------------ pooling
def _pool(tag_rows, seg, ids, vals, B, D):
    """tag_rows [nnz, LD] fp32 (the fused row of every tag present), seg [nnz] its example, ids [nnz] its tag id.
    Returns (out f64 [B, LD], sum|terms| of the UNSCALED sums, count [B])."""
    LD = tag_rows.shape[1]
    r = tag_rows.to(F64).clone()
    r[:, D + 2:] = 0
    if vals is not None:
        v = vals.to(F64)[:, None]
        r[:, :D] *= v
        r[:, D + 1:D + 2] *= v
    else:
        r[:, D + 1] *= (ids >= 1).to(F64)
    dev = tag_rows.device
    out = torch.zeros(B, LD, dtype=F64, device=dev).index_add(0, seg, r)
    ab = torch.zeros(B, LD, dtype=F64, device=dev).index_add(0, seg, r.abs())
    cnt = torch.bincount(seg, minlength=B)
    if vals is None:
        out[:, :D + 1] *= (1.0 / cnt.clamp(min=1).to(F64).sqrt())[:, None]
    return out, ab, cnt


def pool_rows_ref(rows, row0, D, offsets, ids, vals=None):
    """rm_pool_rows (CSR): out [B, LD] = [sum emb | sum bias | sum lin | 0 ..]; sqrtn form (vals None): columns
    0..D scaled by 1/sqrt(count), the linear column counts known tags (id >= 1) only; vals form: embedding and linear
    columns weighted, bias not, no factor, slot 0 kept.  Returns (out, sum|terms| before the sqrtn factor, count)."""
    B = offsets.shape[0] - 1
    seg = torch.repeat_interleave(torch.arange(B, device=ids.device), offsets[1:] - offsets[:-1])
    return _pool(rows[row0 + ids], seg, ids, vals, B, D)


def pool_rows_padded_ref(rows, D, pos, ids, vals=None):
    """rm_pool_rows_padded: tags are the columns of ids [B,T] (-1 = none), their rows rows[pos[b,t]]."""
    B, T = ids.shape
    present = ids >= 0
    seg = torch.arange(B, device=ids.device)[:, None].expand(B, T)[present]
    return _pool(rows[pos[present]], seg, ids[present], None if vals is None else vals[present], B, D)


RSQRT_TERMS = 2  # added to n where every term carries the sqrtn factor: rsqrtf is good to 1 ulp = 2 * 2^-24 relative


def _pool_weights(ids, cnt_of_tag, vals):
    """(we, wb, wl) of every tag: the factors of the embedding, bias and linear columns in the backward."""
    if vals is not None:
        v = vals.to(F64)
        return v, torch.ones_like(v), v
    inv = 1.0 / cnt_of_tag.to(F64).sqrt()
    return inv, inv, (ids >= 1).to(F64)


def pool_rows_bwd_ref(d_rows, g_bias, g_lin, D, offsets, ids, vals, row0, d_table, d_bias, d_lin):
    """rm_pool_rows_bwd into the prior contents d_table [R,D], d_bias [R], d_lin [R] (None = skipped):
    per buffer (result f64, sum|terms| incl. the prior content, n = multiplicity + 1), or None.  In the sqrtn form
    (vals None) every term of d_table and d_bias is a product with the fp32 rsqrtf(count): use n + RSQRT_TERMS."""
    B = offsets.shape[0] - 1
    cnt = offsets[1:] - offsets[:-1]
    seg = torch.repeat_interleave(torch.arange(B, device=ids.device), cnt)
    we, wb, wl = _pool_weights(ids, cnt[seg], vals)
    r = row0 + ids

    def add(prior, contrib, skip=None):
        if prior is None or contrib is None:
            return None
        p = prior.to(F64).reshape(prior.shape[0], -1)
        rr = r if skip is None else r[~skip]
        cc = contrib if skip is None else contrib[~skip]
        res = p.clone().index_add(0, rr, cc)
        ab = p.abs().index_add(0, rr, cc.abs())
        n = (torch.bincount(rr, minlength=p.shape[0]) + 1)[:, None].expand_as(res)
        return res.reshape(prior.shape), ab.reshape(prior.shape), n.reshape(prior.shape)

    t = add(d_table, d_rows[:, :D].to(F64)[seg] * we[:, None])
    b = add(d_bias, None if g_bias is None else (g_bias.to(F64)[seg] * wb)[:, None])
    l = add(d_lin, None if g_lin is None else (g_lin.to(F64)[seg] * wl)[:, None], skip=(wl == 0))
    return t, b, l


def pack_pooled_grad_rows_ref(d_rows, g_bias, g_lin, D, pos, ids, vals, out_prior):
    """rm_pack_pooled_grad_rows: out[pos[b,t]] = [d_rows[b] we | g_bias[b] wb | g_lin[b] wl | 0 ..] for every tag
    present with a slot (ids >= 0 and pos >= 0); every other row of out keeps its prior content.  float64."""
    B, T = ids.shape
    cnt = (ids >= 0).sum(1)
    sel = (ids >= 0) & (pos >= 0)
    b_of = torch.arange(B, device=ids.device)[:, None].expand(B, T)[sel]
    we, wb, wl = _pool_weights(ids[sel], cnt[b_of], None if vals is None else vals[sel])
    out = out_prior.to(F64).clone()
    row = torch.zeros(b_of.numel(), out.shape[1], dtype=F64, device=out.device)
    row[:, :D] = d_rows[:, :D].to(F64)[b_of] * we[:, None]
    if g_bias is not None:
        row[:, D] = g_bias.to(F64)[b_of] * wb
    if g_lin is not None:
        row[:, D + 1] = g_lin.to(F64)[b_of] * wl
    out[pos[sel]] = row
    return out


# -------------------------------------------------------------------------------------------------- row helpers
def gather_rows_ref(table, rows, width):
    """rm_gather_rows: out[i] = table[rows[i], :width], a zero row for rows[i] < 0 (fp32, data movement)."""
    out = table[rows.clamp(min=0)][:, :width].clone()
    out[rows < 0] = 0
    return out


def permute_rows_ref(src, slot, inverse, dst_prior):
    """rm_permute_rows: dst[i] = src[slot[i]] (inverse = False) or dst[slot[i]] = src[i] (fp32, data movement)."""
    dst = dst_prior.clone()
    if inverse:
        dst[slot] = src
    else:
        dst[:] = src[slot]
    return dst


def pack_grad_rows_ref(d_rows, g_bias, g_lin, lin_field_mask, pos, out_prior):
    """rm_pack_grad_rows in fp32: out[pos[o]] = [d_rows[o] | g_bias[b] | g_lin[b] * lin_field_mask[f] | 0 ..];
    occurrences with pos < 0 write nothing (their would-be slots keep the prior content).  One fp32 multiply at most
    per element: bit for bit."""
    B, F, D = d_rows.shape
    out = out_prior.clone()
    row = torch.zeros(B * F, out.shape[1], dtype=d_rows.dtype, device=d_rows.device)
    row[:, :D] = d_rows.reshape(B * F, D)
    if g_bias is not None:
        row[:, D] = g_bias[:, None].expand(B, F).reshape(-1)
    if g_lin is not None:
        gl = g_lin[:, None].expand(B, F)
        row[:, D + 1] = (gl if lin_field_mask is None else gl * lin_field_mask[None, :]).reshape(-1)
    keep = pos >= 0
    out[pos[keep]] = row[keep]
    return out


# ---------------------------------------------------------------------------------------------- dense optimizer
def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def dense_opt_ref(p, g, m, v, step, kind, lr, beta1=0.9, beta2=0.999, eps=1e-7, reset=False):
    """rm_dense_optimizer_step in float64 (the hyper-parameters cross the ABI as fp32 and are taken as such):
    Keras Adam (epsilon outside the sqrt, lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)), Adagrad (accumulator starts
    at 0.1 under reset), SGD.  reset: a NEW optimizer's first step - the stored moments are ignored and Adam's bias
    correction is taken at t = 1 whatever `step` says (include/recman_hip.h; the reference builds a new optimizer for
    every batch).  Returns new (p, m, v) in float64 (m / v None where the kind has none)."""
    if reset:
        step = 1
    lr, b1, b2, eps = _f32(lr), _f32(beta1), _f32(beta2), _f32(eps)
    p, g = p.to(F64), g.to(F64)
    if kind == "adam":
        m = torch.zeros_like(p) if reset else m.to(F64)
        v = torch.zeros_like(p) if reset else v.to(F64)
        one_b1, one_b2 = _f32(1.0 - b1), _f32(1.0 - b2)  # the kernel forms 1 - beta in fp32
        lr_t = _f32(lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step))
        m = b1 * m + one_b1 * g
        v = b2 * v + one_b2 * g * g
        return p - lr_t * m / (v.sqrt() + eps), m, v
    if kind == "adagrad":
        v = torch.full_like(p, _f32(0.1)) if reset else v.to(F64)
        v = v + g * g
        return p - lr * g / (v.sqrt() + eps), None, v
    return p - lr * g, None, None
