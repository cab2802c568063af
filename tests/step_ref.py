"""Plain float64 reference, case builder and case lists for the one-kernel DeepFM step (csrc/step.hip:
rm_deepfm_step).  Test infrastructure, like tests/mlp_ref.py: tests/test_step_host.py pins it on the CPU against the
model oracle, tests/test_gpu_step_kernel.py holds the kernel to it through recman_amd.ops.deepfm_step.

step_ref restates the contract of include/recman_hip.h at the level of the C ABI - fused rows, ids, field offsets,
the MLP's variables one by one - in torch, in float64, from the SAME fp32 tensors the kernel gets (widened, never
re-rounded); the backward is autograd of that loss.  Nothing here is derived from the kernel: no tiles, no slot map,
no launch arithmetic.  pack_ref / unpack_ref restate the packed (row-sharded) output as the pure re-indexing it is.

Activation kinks.  fp32 and float64 may take different branches of relu' / leaky_relu' at a pre-activation within
fp32 rounding of 0 and both be right (tests/test_gpu_steady_state.py:_case tells the story): make_step_case draws
B + B // 2 examples and keeps the first B that are clear of the kink by that file's rule - a condition on the inputs,
decided by the reference alone, checked for every GPU case on the CPU (tests/test_step_host.py).
"""
import functools
import types

import torch

from oracle import th_layers as T
from tests.cases import make_case

F64 = torch.float64
D = 16           # the kernel's embedding width
COLS = D + 2     # the columns of a fused row the step reads: [16 embedding | bias entry | linear weight]
ACTS = ("relu", "leaky_relu", "identity")
TASKS = ("classification", "regression")
KERAS_EPS = 1e-7


def _act(z, act):
    if act == "relu":
        return z.clamp(min=0)
    if act == "leaky_relu":  # tf.nn.leaky_relu's alpha
        return torch.where(z > 0, z, 0.2 * z)
    assert act == "identity", act
    return z


def kink_clear(z, terms, K):
    """tests/test_gpu_steady_state.py:_kink_clear, restated with its constants: the examples (dim 0) whose
    pre-activations z all lie outside 2 (K + 1) 2^-24 * terms of 0."""
    return (z.abs() > 2 * (K + 1) * 2.0 ** -24 * terms).flatten(1).all(1)


# ------------------------------------------------------------------------------------------------------ reference
def _gather(rows, idx, field_off):
    """The used rows only, on the host: [B, F, 18] float64 (the table may be several GB on another device)."""
    B, F = idx.shape
    ids = (idx + field_off.reshape(1, F)).reshape(-1).to(rows.device)
    return rows[ids][:, :COLS].cpu().to(F64).reshape(B, F, COLS)


def step_ref(rows, idx, field_off, dense, y, W0, b0, W1, b1, w_out, w0_out, lin_w_dense, lin_w0, act, task,
             grad_scale=1.0):
    """rm_deepfm_step in float64.  rows [R, table_ld] fused rows, idx [B,F] + field_off [F] = row numbers, dense
    [B,Dn] or None, y int64 or float labels.  Forward: logit = linear + FM + DNN (FM second order
    0.5 sum_d (S_d^2 - sum_f E_fd^2) plus the bias entries), PredictionLayer, the mean loss (Keras binary
    cross-entropy on probabilities, or MSE) without l2 terms.  Backward: autograd of grad_scale * loss.
    Returns a dict of float64 tensors: logit, pred, dlogit [B], loss [1], d_rows [B,F,16] per occurrence (duplicates
    not merged), dW0, db0, dW1, db1, d_w_out, d_w0_out, d_lin_w_dense (None when Dn = 0), d_lin_w0."""
    B, F = idx.shape
    X = _gather(rows, idx, field_off)
    E = X[..., :D].clone().requires_grad_(True)
    bias_e, lin_e = X[..., D], X[..., D + 1]
    Dn = 0 if dense is None else dense.shape[1]
    leaf = lambda t: t.detach().cpu().to(F64).clone().requires_grad_(True)
    v = dict(W0=leaf(W0), b0=leaf(b0), W1=leaf(W1), b1=leaf(b1), w_out=leaf(w_out.reshape(-1)),
             w0_out=leaf(w0_out.reshape(1)), lin_w0=leaf(lin_w0.reshape(1)))
    x = E.reshape(B, F * D)
    lin = lin_e.sum(1) + v["lin_w0"]
    if Dn:
        v["lin_w_dense"] = leaf(lin_w_dense.reshape(-1))
        xd = dense.detach().cpu().to(F64)
        lin = lin + xd @ v["lin_w_dense"]
        x = torch.cat([x, xd], 1)
    S = E.sum(1)
    fm = bias_e.sum(1) + 0.5 * (S.square() - E.square().sum(1)).sum(1)
    h0 = _act(x @ v["W0"] + v["b0"], act)
    h1 = _act(h0 @ v["W1"] + v["b1"], act)
    dnn = h1 @ v["w_out"] + v["w0_out"]
    logit = lin + fm + dnn
    logit.retain_grad()
    t = y.detach().cpu().to(F64)
    if task == "classification":
        pred = torch.sigmoid(logit)
        pc = pred.clamp(KERAS_EPS, 1 - KERAS_EPS)
        loss = -(t * torch.log(pc + KERAS_EPS) + (1 - t) * torch.log(1 - pc + KERAS_EPS)).mean()
    else:
        assert task == "regression", task
        pred = logit
        loss = (pred - t).square().mean()
    (loss * grad_scale).backward()
    g = lambda k: v[k].grad if v[k].grad is not None else torch.zeros_like(v[k])
    return dict(logit=logit.detach(), pred=pred.detach(), dlogit=logit.grad, loss=loss.detach().reshape(1),
                d_rows=E.grad, dW0=g("W0"), db0=g("b0"), dW1=g("W1"), db1=g("b1"), d_w_out=g("w_out"),
                d_w0_out=g("w0_out"), d_lin_w_dense=g("lin_w_dense") if Dn else None, d_lin_w0=g("lin_w0"))


PARAM_GRADS = ("dW0", "db0", "dW1", "db1", "d_w_out", "d_w0_out", "d_lin_w_dense", "d_lin_w0")


def pack_ref(d_rows, dlogit, pos, packed_rows, lin_field_mask=None):
    """The packed form's send buffer [packed_rows, 20]: row pos[b,f] = [d_rows[b,f] | dlogit[b] | dlogit[b] *
    lin_field_mask[f] | 0 0]; rows nobody addresses are NaN.  pos [B,F]: distinct positions."""
    B, F, _ = d_rows.shape
    m = torch.ones(F, dtype=d_rows.dtype) if lin_field_mask is None else lin_field_mask.to(d_rows.dtype)
    g = dlogit.reshape(B, 1).expand(B, F)
    z = torch.zeros(B, F, dtype=d_rows.dtype)
    body = torch.cat([d_rows, torch.stack([g, g * m.reshape(1, F), z, z], 2)], 2)
    out = torch.full((packed_rows, D + 4), float("nan"), dtype=d_rows.dtype)
    out[pos.reshape(-1)] = body.reshape(B * F, D + 4)
    return out


def unpack_ref(buf, pos):
    """The inverse gather: (d_rows [B,F,16], g_bias [B,F], g_lin [B,F], pad [B,F,2]) of the rows pos addresses."""
    B, F = pos.shape
    r = buf[pos.reshape(-1)].reshape(B, F, D + 4)
    return r[..., :D], r[..., D], r[..., D + 1], r[..., D + 2:]


# --------------------------------------------------------------------------------------------------- case builder
def default_scale(F):
    """make_case's default 0.3 for up to 10 fields (the reach of its hand-written vocabularies); beyond, the 0.05
    every F = 26 case of tests/test_gpu_step.py and tests/test_gpu_steady_state.py passes to it: the FM term grows
    with F * scale^2, and a logit in the tens leaves fp32 no room for the 1e-5 absolute the kernel is held to."""
    return 0.3 if F <= 10 else 0.05


def fuse_rows(p, spec, table_ld):
    """The fused table as the engine builds it: row off_f + v = [embedding | bias entry | linear weight | NaN ...]
    (the step reads 18 columns of a row; the rest is poison).  Returns (rows [R, table_ld], field_off [F],
    lin_w_dense [Dn])."""
    assert table_ld >= D + 4 and table_ld % 4 == 0
    lin_offs, dense_offs, _ = spec.lin_layout
    lw = p["linear_w"].reshape(-1)
    rows = torch.full((sum(spec.feat_sizes), table_ld), float("nan"), dtype=lw.dtype)
    offs, off = [], 0
    for f, (n, V) in enumerate(zip(spec.sparse_names, spec.feat_sizes)):
        rows[off: off + V, :D] = p[f"{n}_feat_embed"]
        rows[off: off + V, D] = p[f"{n}_feat_bias"][:, 0]
        rows[off: off + V, D + 1] = lw[lin_offs[f]: lin_offs[f] + V]
        offs.append(off)
        off += V
    return rows, torch.tensor(offs, dtype=torch.int64), lw[torch.tensor(dense_offs, dtype=torch.int64)].clone()


@functools.lru_cache(maxsize=4)
def make_step_case(B, F, Dn, H0, H1, table_ld=20, act="relu", task="classification", seed=0):
    """Every argument of rm_deepfm_step for B kink-clear examples (seeded; tests/cases.py:make_case's generators and
    scales, float labels ~ N(0, 1) for regression).  The result is cached and shared: treat it as read-only.
    Fields: rows, idx, field_off, dense (None when Dn = 0), y, W0, b0, W1, b1, w_out, w0_out, lin_w_dense (None when
    Dn = 0), lin_w0, act, task - and spec, p, hp, the oracle's view of the same case (l2 factors 0)."""
    n = B + B // 2
    spec, p, idx, dense, y, hp = make_case("deepfm", B=n, F=F, D=D, Dn=Dn, hidden=(H0, H1), seed=seed,
                                           scale=default_scale(F), hp_extra=dict(deep_activation=act))
    hp.update(embedding_l2_reg=0.0, linear_l2_reg=0.0, deep_l2_reg=0.0)
    if task == "regression":
        y = torch.randn(n, generator=torch.Generator().manual_seed(1000 + seed))
    rows, field_off, lin_w_dense = fuse_rows(p, spec, table_ld)
    Ws = [p[f"dnn_layer_{i}_weights"] for i in range(2)]
    bs = [p[f"dnn_layer_{i}_bias"] for i in range(2)]
    # the kink rule on layer 0 and layer 1, in float64
    a = _gather(rows, idx, field_off)[..., :D].reshape(n, F * D)
    if Dn:
        a = torch.cat([a, dense.to(F64)], 1)
    clear = torch.ones(n, dtype=torch.bool)
    for W, b in zip(Ws, bs):
        W, b = W.to(F64), b.to(F64)
        z = a @ W + b
        clear &= kink_clear(z, a.abs() @ W.abs() + b.abs(), W.shape[0])
        a = _act(z, act)
    sel = clear.nonzero().reshape(-1)[:B]
    assert sel.numel() == B, f"only {sel.numel()} of {B} examples clear of the kink"
    return types.SimpleNamespace(
        B=B, F=F, Dn=Dn, H0=H0, H1=H1, table_ld=table_ld, act=act, task=task, seed=seed, spec=spec, p=p, hp=hp,
        rows=rows, idx=idx[sel].contiguous(), field_off=field_off, dense=dense[sel].contiguous() if Dn else None,
        y=y[sel].contiguous(), W0=Ws[0], b0=bs[0], W1=Ws[1], b1=bs[1], w_out=p["dnn_w"].reshape(-1).clone(),
        w0_out=p["dnn_w0"], lin_w_dense=lin_w_dense if Dn else None, lin_w0=p["linear_w0"])


def with_stride(c, table_ld):
    """The same case with its rows in a table of another row stride."""
    rows = fuse_rows(c.p, c.spec, table_ld)[0]
    assert torch.equal(rows[:, :COLS], c.rows[:, :COLS])
    d = dict(vars(c))
    d.update(rows=rows, table_ld=table_ld)
    return types.SimpleNamespace(**d)


def ref_of(c, grad_scale=1.0):
    return step_ref(c.rows, c.idx, c.field_off, c.dense, c.y, c.W0, c.b0, c.W1, c.b1, c.w_out, c.w0_out,
                    c.lin_w_dense, c.lin_w0, c.act, c.task, grad_scale)


# ------------------------------------------------------------------------------------------------------ case lists
# Keyword arguments of make_step_case for every GPU case of tests/test_gpu_step_kernel.py; tests/test_step_host.py
# builds each of them on the CPU (the kink selection must find its B examples).  Seeds are fixed here.
def _kw(i, B, F, Dn, H0, H1, table_ld=20, seed0=0):
    return dict(B=B, F=F, Dn=Dn, H0=H0, H1=H1, table_ld=table_ld, act=ACTS[i % 3], task=TASKS[i % 2],
                seed=seed0 + i)


SWEEP_B = 37  # three 16-example tiles, the last ragged (5 examples)
# a. every F; Dn = 1..16 and round again, then F = 26 with Dn at its limit and with no dense inputs at all
SLOT_FDN = [(F, (F - 1) % 16 + 1) for F in range(1, 26)] + [(26, 16), (26, 0)]
SLOT_CASES = [_kw(i, SWEEP_B, F, Dn, 32, 32, table_ld=32, seed0=100) for i, (F, Dn) in enumerate(SLOT_FDN)]
# b. (H0, H1) = (H, 33 - H): every width of both layers, at a full and at a nearly empty slot map
WIDTH_CASES = [_kw(H, SWEEP_B, F, Dn, H, 33 - H, table_ld=32, seed0=200 + 40 * j)
               for j, (F, Dn) in enumerate([(26, 13), (3, 5)]) for H in range(1, 33)]
# c. one case, its rows in tables of four strides
STRIDES = (20, 24, 32, 36)
STRIDE_CASE = _kw(1, 53, 9, 4, 32, 32, table_ld=STRIDES[0], seed0=300)
# e. the packed form
PACKED_B = (1, 16, 17, 37, 8200, 17609)
PACKED_CASES = {(B, 26): _kw(i, B, 26, 13, 32, 32, seed0=400) for i, B in enumerate(PACKED_B)}
PACKED_CASES[(8200, 5)] = _kw(1, 8200, 5, 0, 17, 3, seed0=420)
PACKED_SPARE = 1000  # rows of the exchange buffers that no occurrence addresses
# f. rows past 4 GiB
BIG_CASE = _kw(0, SWEEP_B, 26, 13, 32, 32, table_ld=32, seed0=500)
BIG_ROWS, BIG_END = 2 ** 25 + 2 ** 12, 2 ** 11

GPU_CASES = SLOT_CASES + WIDTH_CASES + [STRIDE_CASE] + list(PACKED_CASES.values()) + [BIG_CASE]


def packed_positions(B, F, packed_rows, seed):
    """B * F distinct positions drawn from range(packed_rows), in random order: [B, F] int64."""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(packed_rows, generator=g)[: B * F].reshape(B, F).contiguous()


def lin_masks(F):
    """The three lin_field_mask values of the packed cases: None, all ones, 0/1 with both values present."""
    mixed = (torch.arange(F) % 3 != 1).float()
    if F > 1:
        assert 0 < float(mixed.sum()) < F
    return {"none": None, "ones": torch.ones(F), "mixed": mixed}
