"""Tensor-level wrappers over the C ABI: shape/dtype/device checks in Python (the
reference raises Python asserts before any arithmetic, layers.py:49,85,458,521-522),
raw pointers and sizes across the boundary, kernels enqueued on torch's current
stream.  torch is plumbing here: device memory and streams, nothing else.
"""
import ctypes

import torch

from . import _lib

F32, I64 = torch.float32, torch.int64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name, dtype, shape=None, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError(f"{name} must not be None")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (recman_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr()


def profile_marker(tag=0):
    """An empty marker kernel on the current stream (cuts a rocprofv3 trace, rm_profile_marker)."""
    _lib.call("rm_profile_marker", int(tag), _stream())


def embed_fwd(idx, table, field_off, *, bias_table=None, bias_ld=1, lin_w=None, lin_ld=1,
              lin_off=None, lin_w_dense=None, lin_w0=None, dense=None, mask_b=None, mask_e=None,
              E=None, fm_sum=None, fm_logit=None, lin_logit=None, table_ld=None, D=None,
              bias_col=None, lin_col=None, stream_rows=False):
    """Gather + FM + linear forward (see rm_embed_fwd in include/recman_hip.h).
    stream_rows: RM_EMBED_STREAM_ROWS - non-temporal row loads (ids with little reuse per batch).
    `table` is [R, table_ld]; D defaults to table.shape[1].  bias_col / lin_col: the FM
    bias / sparse linear weight live in that column of the table row itself (fused rows)."""
    B, F = idx.shape
    ld = table.shape[1] if table_ld is None else table_ld
    D = table.shape[1] if D is None else D
    Dn = 0 if dense is None else dense.shape[1]
    tp = _chk(table, "table", F32)
    fo = _chk(field_off, "field_off", I64, (F,))
    bp, bld = _chk(bias_table, "bias_table", F32, allow_none=True), bias_ld
    if bias_col is not None:
        bp, bld = tp + 4 * bias_col, ld
    lp, lld = _chk(lin_w, "lin_w", F32, allow_none=True), lin_ld
    lo = _chk(lin_off, "lin_off", I64, (F,), allow_none=True)
    if lin_col is not None:
        lp, lld, lo = tp + 4 * lin_col, ld, fo
    _lib.call(
        "rm_embed_fwd", _chk(idx, "idx", I64), tp, ld, fo, bp, bld, lp, lld, lo,
        _chk(lin_w_dense, "lin_w_dense", F32, (Dn,), allow_none=True),
        _chk(lin_w0, "lin_w0", F32, (1,), allow_none=True),
        _chk(dense, "dense", F32, (B, Dn), allow_none=True), Dn,
        _chk(mask_b, "mask_b", F32, (B, F), allow_none=True),
        _chk(mask_e, "mask_e", F32, (B, F, D), allow_none=True), B, F, D,
        _chk(E, "E", F32, (B, F, D), allow_none=True),
        _chk(fm_sum, "fm_sum", F32, (B, D), allow_none=True),
        _chk(fm_logit, "fm_logit", F32, (B,), allow_none=True),
        _chk(lin_logit, "lin_logit", F32, (B,), allow_none=True), 1 if stream_rows else 0, _stream())


def linear_fwd(idx, lin_off, w, dense, w_dense, w0, out):
    """out[b] = sum_f w[lin_off[f] + idx[b,f]] + dense[b,:] . w_dense + w0 (rm_linear_fwd)."""
    B = out.shape[0]
    F = 0 if idx is None else idx.shape[1]
    Dn = 0 if dense is None else dense.shape[1]
    _lib.call("rm_linear_fwd", _chk(idx, "idx", I64, (B, F), allow_none=True),
              _chk(lin_off, "lin_off", I64, (F,), allow_none=True), _chk(w, "w", F32, allow_none=True),
              _chk(dense, "dense", F32, (B, Dn), allow_none=True),
              _chk(w_dense, "w_dense", F32, (Dn,), allow_none=True),
              _chk(w0, "w0", F32, (1,), allow_none=True), B, F, Dn, _chk(out, "out", F32, (B,)), _stream())


def embed_bwd(d_rows, *, E=None, fm_sum=None, dE_up=None, g_fm=None, mask_b=None, mask_e=None,
              d_bias=None):
    B, F, D = d_rows.shape
    _lib.call(
        "rm_embed_bwd", _chk(E, "E", F32, (B, F, D), allow_none=True),
        _chk(fm_sum, "fm_sum", F32, (B, D), allow_none=True),
        _chk(dE_up, "dE_up", F32, (B, F, D), allow_none=True),
        _chk(g_fm, "g_fm", F32, (B,), allow_none=True),
        _chk(mask_b, "mask_b", F32, (B, F), allow_none=True),
        _chk(mask_e, "mask_e", F32, (B, F, D), allow_none=True), B, F, D,
        _chk(d_rows, "d_rows", F32), _chk(d_bias, "d_bias", F32, (B, F), allow_none=True),
        _stream())


def scatter_add_rows(d_table, idx, field_off, *, rows=None, g_row=None, width=None, ld=None):
    B, F = idx.shape
    if width is None:
        width = 1 if g_row is not None else rows.shape[-1]
    if ld is None:
        ld = d_table.shape[1] if d_table.dim() == 2 else 1
    _lib.call(
        "rm_scatter_add_rows", _chk(idx, "idx", I64), _chk(field_off, "field_off", I64, (F,)),
        _chk(rows, "rows", F32, allow_none=True), _chk(g_row, "g_row", F32, (B,), allow_none=True),
        B, F, width, ld, _chk(d_table, "d_table", F32), _stream())


def linear_dense_bwd(g, dense, d_w_dense, d_w0, workspace):
    B = g.shape[0]
    Dn = 0 if dense is None else dense.shape[1]
    if workspace.numel() < 256 * (Dn + 1):
        raise ValueError("linear_dense_bwd: workspace too small")
    if Dn > 1023:
        raise ValueError("linear_dense_bwd: at most 1023 columns")
    _lib.call(
        "rm_linear_dense_bwd", _chk(g, "g", F32, (B,)),
        _chk(dense, "dense", F32, (B, Dn), allow_none=True), B, Dn,
        _chk(d_w_dense, "d_w_dense", F32, (Dn,), allow_none=True),
        _chk(d_w0, "d_w0", F32, (1,), allow_none=True), _chk(workspace, "workspace", F32),
        _stream())


def logit_loss(branches, *, y=None, y_f=None, task="classification", logit=None, pred=None,
               dlogit=None, loss=None, workspace=None):
    """branches: up to four (tensor [B], coefficient) pairs."""
    if not 1 <= len(branches) <= 4:
        raise ValueError("logit_loss takes 1..4 branch logits")
    B = branches[0][0].shape[0]
    args = []
    for i in range(4):
        if i < len(branches):
            t, c = branches[i]
            args += [_chk(t, f"logit_{i}", F32, (B,)), float(c)]
        else:
            args += [None, 0.0]
    if loss is not None and (workspace is None or workspace.numel() < 1024):
        raise ValueError("logit_loss: loss needs a workspace of >= 1024 floats")
    _lib.call(
        "rm_logit_loss", *args, _chk(y, "y", I64, (B,), allow_none=True),
        _chk(y_f, "y_f", F32, (B,), allow_none=True), 0 if task == "classification" else 1, B,
        _chk(logit, "logit", F32, (B,), allow_none=True),
        _chk(pred, "pred", F32, (B,), allow_none=True),
        _chk(dlogit, "dlogit", F32, (B,), allow_none=True),
        _chk(loss, "loss", F32, (1,), allow_none=True),
        _chk(workspace, "workspace", F32, allow_none=True), _stream())


def cross_p_ld(L):
    """Row length of the saved dot products p [B, p_ld] (L+1 values, padded to a multiple of 4)."""
    return (L + 4) // 4 * 4


def cross_fwd(xe, xd, w, b, w_out, logit, p_out=None):
    """CrossNet forward (rm_cross_fwd).  p_out [B, cross_p_ld(L)]: the row's dot products
    (x0.w_l, x0.w_out), all the backward needs."""
    B, FD = xe.shape
    Dn = 0 if xd is None else xd.shape[1]
    L, d = w.shape
    if d != FD + Dn:
        raise ValueError(f"cross_fwd: w has d={d}, inputs have {FD}+{Dn}")
    p_ld = 0 if p_out is None else p_out.shape[1]
    _lib.call(
        "rm_cross_fwd", _chk(xe, "xe", F32), _chk(xd, "xd", F32, (B, Dn), allow_none=True), FD, Dn,
        _chk(w, "w", F32), _chk(b, "b", F32, (L, d)), _chk(w_out, "w_out", F32, (d,)), L, B,
        _chk(logit, "logit", F32, (B,)), _chk(p_out, "p_out", F32, (B, p_ld), allow_none=True), p_ld,
        _stream())


def cross_bwd(w, b, w_out, g, p, d_xe, coef, dx_in_e=None):
    """CrossNet backward (rm_cross_bwd): d_xe [B,FD] (+ dx_in_e), coef [B,2L+2]."""
    B, FD = d_xe.shape
    L, d = w.shape
    _lib.call(
        "rm_cross_bwd", FD, d - FD, _chk(w, "w", F32), _chk(b, "b", F32, (L, d)),
        _chk(w_out, "w_out", F32, (d,)), L, B, _chk(g, "g", F32, (B,)),
        _chk(p, "p", F32, (B, p.shape[1])), p.shape[1],
        _chk(dx_in_e, "dx_in_e", F32, (B, FD), allow_none=True), _chk(d_xe, "d_xe", F32, (B, FD)),
        _chk(coef, "coef", F32, (B, 2 * L + 2)), _stream())


def cross_param_grads(P, colsum, w, b, w_out, d_w, d_b, d_w_out):
    L, d = w.shape
    _lib.call(
        "rm_cross_param_grads", _chk(P, "P", F32, (d, L + 1)),
        _chk(colsum, "colsum", F32, (L + 1,)), _chk(w, "w", F32), _chk(b, "b", F32, (L, d)),
        _chk(w_out, "w_out", F32, (d,)), L, d, _chk(d_w, "d_w", F32, (L, d)),
        _chk(d_b, "d_b", F32, (L, d)), _chk(d_w_out, "d_w_out", F32, (d,)), _stream())


def _need_workspace(fn, workspace, need):
    """The caller's workspace must hold the `need` floats the entry point's *_workspace function asks for."""
    if workspace.numel() < need:
        raise ValueError(f"{fn}: workspace too small ({workspace.numel()} floats, needs {need})")


def _strided_rows(t, name, B, width, exact):
    """A float32 device view of B rows with unit column stride, exactly `width` columns (exact) or at least `width`,
    and any row stride >= its columns -> (pointer, stride)."""
    p, ld, cols = _rows2d(t, name)
    if t.shape[0] != B or (cols != width if exact else cols < width):
        raise ValueError(f"{name} {tuple(t.shape)} must be " + (f"[{B},{width}]" if exact else f"[{B}, >= {width}]"))
    if B > 1 and ld < cols:
        raise ValueError(f"{name}: row stride {ld} < {cols} columns")
    return p, max(ld, cols)


def afm_supported(F, D, T):
    """rm_afm_supported: D in {8, 16, 32, 64}, 2 <= F <= 40, 1 <= T <= 64."""
    return bool(_lib.lib().rm_afm_supported(int(F), int(D), int(T)))


def afm_stats_width(D):
    """Row length of the forward's record stats [B, D + 2]: softmax max, denominator, u = mask * v."""
    return D + 2


def afm_fwd(E, W, b, h, p, logit, mask=None, stats=None):
    """AFM attention layer forward (rm_afm_fwd): E [B,F,D], W [D,T], b [T], h [T], p [D], mask [B,D] or None
    -> logit [B]; stats [B, D+2] (training) or None (inference, same logits)."""
    B, F, D = E.shape
    T = W.shape[1]
    _lib.call(
        "rm_afm_fwd", _chk(E, "E", F32), _chk(W, "W", F32, (D, T)), _chk(b, "b", F32, (T,)),
        _chk(h, "h", F32, (T,)), _chk(p, "p", F32, (D,)), _chk(mask, "mask", F32, (B, D), allow_none=True),
        B, F, D, T, _chk(logit, "logit", F32, (B,)),
        _chk(stats, "stats", F32, (B, D + 2), allow_none=True), _stream())


def afm_bwd_workspace(B, F, D, T):
    """Floats of workspace rm_afm_bwd needs (0: unsupported shape)."""
    return int(_lib.lib().rm_afm_bwd_workspace(int(B), int(F), int(D), int(T)))


def afm_bwd(E, W, b, h, p, g, logit, stats, d_rows, dW, db, dh, dp, workspace, mask=None, dE_up=None):
    """AFM attention layer backward (rm_afm_bwd): d_rows [B,F,D] = dLoss/dE (+ dE_up, which may be d_rows
    itself), dW [D,T], db [T], dh [T], dp [D] overwritten.  Deterministic."""
    B, F, D = E.shape
    T = W.shape[1]
    _need_workspace("afm_bwd", workspace, afm_bwd_workspace(B, F, D, T))
    _lib.call(
        "rm_afm_bwd", _chk(E, "E", F32), _chk(W, "W", F32, (D, T)), _chk(b, "b", F32, (T,)),
        _chk(h, "h", F32, (T,)), _chk(p, "p", F32, (D,)), _chk(mask, "mask", F32, (B, D), allow_none=True),
        _chk(g, "g", F32, (B,)), _chk(logit, "logit", F32, (B,)), _chk(stats, "stats", F32, (B, D + 2)),
        _chk(dE_up, "dE_up", F32, (B, F, D), allow_none=True), B, F, D, T,
        _chk(d_rows, "d_rows", F32, (B, F, D)), _chk(dW, "dW", F32, (D, T)), _chk(db, "db", F32, (T,)),
        _chk(dh, "dh", F32, (T,)), _chk(dp, "dp", F32, (D,)), _chk(workspace, "workspace", F32), _stream())


def autoint_supported(F, Din, H, dk):
    """rm_autoint_supported: 1 <= F <= 40, Din in {8, 16, 32, 64}, H in {1, 2, 4, 8}, dk >= 4, H dk in {8, 16, 32, 64}."""
    return bool(_lib.lib().rm_autoint_supported(int(F), int(Din), int(H), int(dk)))


def autoint_stats_floats(B, F, H):
    """Floats of the interacting layer's forward record stats [B, H, F, 2]: softmax row maximum and denominator."""
    return int(_lib.lib().rm_autoint_stats_floats(int(B), int(F), int(H)))


def _autoint_dims(X, Wq, H):
    if X.dim() != 3 or Wq.dim() != 2:
        raise ValueError(f"autoint: X must be [B,F,Din] and Wq [Din,HD], got {tuple(X.shape)} and {tuple(Wq.shape)}")
    B, F, Din = X.shape
    HD, H = Wq.shape[1], int(H)
    if H < 1 or HD % H:
        raise ValueError(f"autoint: {H} heads do not divide HD={HD} (unsupported)")
    return B, F, Din, H, HD // H, HD


def autoint_layer_fwd(X, Wq, Wk, Wv, Wr, H, scale, Y, stats=None):
    """AutoInt interacting layer forward (rm_autoint_layer_fwd): X [B,F,Din], Wq / Wk / Wv [Din,HD], Wr [Din,HD] or
    None, H heads, scale on the scores -> Y [B,F,HD]; stats [B,H,F,2] (training) or None (inference, same Y)."""
    B, F, Din, H, dk, HD = _autoint_dims(X, Wq, H)
    _lib.call(
        "rm_autoint_layer_fwd", _chk(X, "X", F32), _chk(Wq, "Wq", F32, (Din, HD)), _chk(Wk, "Wk", F32, (Din, HD)),
        _chk(Wv, "Wv", F32, (Din, HD)), _chk(Wr, "Wr", F32, (Din, HD), allow_none=True), B, F, Din, H, dk,
        float(scale), _chk(Y, "Y", F32, (B, F, HD)), _chk(stats, "stats", F32, (B, H, F, 2), allow_none=True),
        _stream())


def autoint_layer_bwd_workspace(B, F, Din, H, dk):
    """Floats of workspace rm_autoint_layer_bwd needs (0: unsupported shape)."""
    return int(_lib.lib().rm_autoint_layer_bwd_workspace(int(B), int(F), int(Din), int(H), int(dk)))


def autoint_layer_bwd(X, Wq, Wk, Wv, Wr, Y, stats, dY, H, scale, dX, dWq, dWk, dWv, dWr, workspace, dX_up=None):
    """AutoInt interacting layer backward (rm_autoint_layer_bwd): dX [B,F,Din] = dLoss/dX (+ dX_up, which may be dX
    itself), dWq, dWk, dWv, dWr [Din,HD] overwritten (dWr None exactly when Wr is).  Deterministic."""
    B, F, Din, H, dk, HD = _autoint_dims(X, Wq, H)
    if (Wr is None) != (dWr is None):
        raise ValueError("autoint_layer_bwd: Wr and dWr go together")
    _need_workspace("autoint_layer_bwd", workspace, autoint_layer_bwd_workspace(B, F, Din, H, dk))
    _lib.call(
        "rm_autoint_layer_bwd", _chk(X, "X", F32), _chk(Wq, "Wq", F32, (Din, HD)), _chk(Wk, "Wk", F32, (Din, HD)),
        _chk(Wv, "Wv", F32, (Din, HD)), _chk(Wr, "Wr", F32, (Din, HD), allow_none=True),
        _chk(Y, "Y", F32, (B, F, HD)), _chk(stats, "stats", F32, (B, H, F, 2)), _chk(dY, "dY", F32, (B, F, HD)),
        B, F, Din, H, dk, float(scale), _chk(dX, "dX", F32, (B, F, Din)),
        _chk(dX_up, "dX_up", F32, (B, F, Din), allow_none=True), _chk(dWq, "dWq", F32, (Din, HD)),
        _chk(dWk, "dWk", F32, (Din, HD)), _chk(dWv, "dWv", F32, (Din, HD)),
        _chk(dWr, "dWr", F32, (Din, HD), allow_none=True), _chk(workspace, "workspace", F32), _stream())


def autoint_head_fwd(Y, w, w0, logit):
    """AutoInt's last projection (rm_autoint_head_fwd): Y [B, ...] flattened to [B,K], w [K], w0 [1] -> logit [B]."""
    B, K = Y.shape[0], w.numel()
    if Y.numel() != B * K:
        raise ValueError(f"autoint_head_fwd: Y {tuple(Y.shape)} does not flatten to [B, {K}]")
    _lib.call("rm_autoint_head_fwd", _chk(Y, "Y", F32), _chk(w, "w", F32, (K,)), _chk(w0, "w0", F32, (1,)), B, K,
              _chk(logit, "logit", F32, (B,)), _stream())


def autoint_head_bwd_workspace(B, K):
    """Floats of workspace rm_autoint_head_bwd needs."""
    return int(_lib.lib().rm_autoint_head_bwd_workspace(int(B), int(K)))


def autoint_head_bwd(Y, w, g, dY, dw, dw0, workspace):
    """Backward of the last projection (rm_autoint_head_bwd): g [B] -> dY (Y's shape) = g w, dw [K] = sum g Y,
    dw0 [1] = sum g, overwritten.  Deterministic."""
    B, K = Y.shape[0], w.numel()
    if Y.numel() != B * K:
        raise ValueError(f"autoint_head_bwd: Y {tuple(Y.shape)} does not flatten to [B, {K}]")
    _need_workspace("autoint_head_bwd", workspace, autoint_head_bwd_workspace(B, K))
    _lib.call("rm_autoint_head_bwd", _chk(Y, "Y", F32), _chk(w, "w", F32, (K,)), _chk(g, "g", F32, (B,)), B, K,
              _chk(dY, "dY", F32, tuple(Y.shape)), _chk(dw, "dw", F32, (K,)), _chk(dw0, "dw0", F32, (1,)),
              _chk(workspace, "workspace", F32), _stream())


def dot_interact_supported(F, D):
    """rm_dot_interact_supported: D in {8, 16, 32, 64}, 1 <= F <= 40."""
    return bool(_lib.lib().rm_dot_interact_supported(int(F), int(D)))


def dot_interact_width(F, D):
    """(D + P, ldx): the columns DLRM's interaction writes (z, then the P = F(F+1)/2 pair dot products) and that
    width rounded up to a multiple of 4 floats (16-byte rows for the dense kernels that read X)."""
    W = D + F * (F + 1) // 2
    return W, (W + 3) // 4 * 4


def _dot_interact_args(E, z, X, name):
    if E.dim() != 3:
        raise ValueError(f"E: expected [B,F,D], got {tuple(E.shape)}")
    B, F, D = E.shape
    if not dot_interact_supported(F, D):
        raise ValueError(f"dot_interact: F={F}, D={D} unsupported (1 <= F <= 40, D in 8, 16, 32, 64)")
    W, _ = dot_interact_width(F, D)
    px, ldx = _strided_rows(X, name, B, W, False)
    return B, F, D, _chk(E, "E", F32), _chk(z, "z", F32, (B, D)), px, ldx


def dot_interact_fwd(E, z, X):
    """DLRM's dot interaction (rm_dot_interact_fwd): E [B,F,D], z [B,D] -> X [B, >= D+P] with row stride ldx:
    X[:, :D] = z, X[:, D + i(i-1)/2 + j] = <v_i, v_j> (v_0 = z, v_f = E[:, f-1]; 0 <= j < i <= F); every column
    from D + P up to the row stride is set to +0.0."""
    B, F, D, pe, pz, px, ldx = _dot_interact_args(E, z, X, "X")
    # the kernel writes whole rows of ldx floats: the last one must lie inside X's storage
    if B and X.storage_offset() + B * ldx > X.untyped_storage().nbytes() // 4:
        raise ValueError(f"X: {B} rows of stride {ldx} from offset {X.storage_offset()} exceed its storage")
    _lib.call("rm_dot_interact_fwd", pe, pz, B, F, D, px, ldx, _stream())


def dot_interact_bwd(E, z, dX, d_rows, dz):
    """rm_dot_interact_bwd: dX [B, >= D+P] (row stride ldx; columns >= D+P are never read) -> d_rows [B,F,D] and
    dz [B,D], both overwritten.  Deterministic."""
    B, F, D, pe, pz, px, ldx = _dot_interact_args(E, z, dX, "dX")
    _lib.call("rm_dot_interact_bwd", pe, pz, px, ldx, B, F, D, _chk(d_rows, "d_rows", F32, (B, F, D)),
              _chk(dz, "dz", F32, (B, D)), _stream())


# ---- the core of a DCN-Mix cross layer (csrc/cross_mix.hip) -----------------------------------------------------
# the kernels' launch constants (csrc/cross_mix.hip: kTileFloats, kMaxG, kGE, kFwdBlocks, kBwdBlocks): a block owns
# tiles of cross_mix_tile(E, r) examples and the grids are capped, so the forward walks the batch a second time from
# B > CROSS_MIX_FWD_BLOCKS * tile on, the backward from B > CROSS_MIX_BWD_BLOCKS * tile on
CROSS_MIX_FWD_BLOCKS, CROSS_MIX_BWD_BLOCKS = 2048, 512


def cross_mix_tile(E, r):
    """Examples per tile of the cross_mix kernels (mix_tile of csrc/cross_mix.hip)."""
    return min(4096 // (E * r), 64) // 4 * 4


def cross_mix_supported(E, r):
    """rm_cross_mix_supported: 1 <= E <= 8, r in {8, 16, 32, 64}, E r <= 256."""
    return bool(_lib.lib().rm_cross_mix_supported(int(E), int(r)))


def _cross_mix_dims(C):
    if C.dim() != 3 or C.shape[1] != C.shape[2]:
        raise ValueError(f"C: expected [E,r,r], got {tuple(C.shape)}")
    E, r = int(C.shape[0]), int(C.shape[1])
    if not cross_mix_supported(E, r):
        raise ValueError(f"cross_mix: E={E}, r={r} unsupported (1 <= E <= 8, r in 8, 16, 32, 64, E r <= 256)")
    return E, r, _chk(C, "C", F32)


def cross_mix_fwd(T, S, C, M):
    """rm_cross_mix_fwd: T [B, E r], S [B, E] (column views of any row stride, e.g. of one projection buffer),
    C [E,r,r] -> M [B, E r]: a_i = tanh(t_i), c_i = tanh(a_i C_i), p = softmax(s), m_i = p_i c_i.  Only M's own
    columns are written."""
    E, r, pc = _cross_mix_dims(C)
    B = T.shape[0]
    pt, ldt = _strided_rows(T, "T", B, E * r, True)
    ps, lds = _strided_rows(S, "S", B, E, True)
    pm, ldm = _strided_rows(M, "M", B, E * r, True)
    _lib.call("rm_cross_mix_fwd", pt, ldt, ps, lds, pc, E, r, B, pm, ldm, _stream())


def cross_mix_bwd_workspace(B, E, r):
    """Floats of workspace for cross_mix_bwd (rm_cross_mix_bwd_workspace): the blocks' partial dC."""
    n = int(_lib.lib().rm_cross_mix_bwd_workspace(int(B), int(E), int(r)))
    if n < 0:
        raise ValueError(f"cross_mix: B={B}, E={E}, r={r} unsupported")
    return n


def cross_mix_bwd(T, S, C, dM, dT, dS, dC, workspace):
    """rm_cross_mix_bwd: dM [B, E r] = dLoss/dM -> dT [B, E r], dS [B, E] (column views of any row stride; only
    their own columns are written) and dC [E,r,r] (overwritten).  a, c and p are recomputed.  Deterministic."""
    E, r, pc = _cross_mix_dims(C)
    B = T.shape[0]
    pt, ldt = _strided_rows(T, "T", B, E * r, True)
    ps, lds = _strided_rows(S, "S", B, E, True)
    pdm, lddm = _strided_rows(dM, "dM", B, E * r, True)
    pdt, lddt = _strided_rows(dT, "dT", B, E * r, True)
    pds, ldds = _strided_rows(dS, "dS", B, E, True)
    _need_workspace("cross_mix_bwd", workspace, cross_mix_bwd_workspace(B, E, r))
    _lib.call("rm_cross_mix_bwd", pt, ldt, ps, lds, pc, E, r, B, pdm, lddm, pdt, lddt, pds, ldds,
              _chk(dC, "dC", F32, (E, r, r)), _chk(workspace, "workspace", F32), _stream())


# ---- FiBiNET's interaction: SENET gate + bilinear pairs (csrc/fibinet.hip) ---------------------------------------
# the kernels' grid caps (csrc/fibinet.hip: kFwdBlocks, kBwdBlocks): a block owns tiles of fibinet_tile(...) examples,
# so the forward walks the batch a second time from B > FIBINET_FWD_BLOCKS * tile on, the backward likewise (the
# backward's cap is lower, down to 128 blocks, where 512 sets of partial gradients would pass 32 MB of workspace)
FIBINET_FWD_BLOCKS, FIBINET_BWD_BLOCKS = 512, 512
FIBINET_TYPES = {"all": 0, "each": 1}  # RM_FIBINET_ALL / RM_FIBINET_EACH
_FIBINET_LIMITS = "2 <= F <= 40, D in 8, 16, 32, 1 <= R <= F, type 'all' or 'each'"


def _fibinet_type(bilinear_type):
    if bilinear_type not in FIBINET_TYPES:
        raise ValueError(f"fibinet: bilinear_type {bilinear_type!r} unsupported ({_FIBINET_LIMITS})")
    return FIBINET_TYPES[bilinear_type]


def fibinet_supported(F, D, R, bilinear_type):
    """rm_fibinet_supported: D in {8, 16, 32}, 2 <= F <= 40, 1 <= R <= F, type "all" or "each"."""
    if bilinear_type not in FIBINET_TYPES:
        return False
    return bool(_lib.lib().rm_fibinet_supported(int(F), int(D), int(R), FIBINET_TYPES[bilinear_type]))


def fibinet_width(F, D):
    """(2 P D, ldx): the columns FiBiNET's interaction writes (both bilinear branches over the P = F(F-1)/2 pairs) and
    that width rounded up to a multiple of 4 floats (16-byte rows for the dense kernels that read X)."""
    W = F * (F - 1) * D
    return W, (W + 3) // 4 * 4


def fibinet_tile(F, D, R, bilinear_type, backward=False):
    """Examples per tile of the forward or the backward kernel (rm_fibinet_tile: what the LDS budget leaves)."""
    g = int(_lib.lib().rm_fibinet_tile(int(F), int(D), int(R), _fibinet_type(bilinear_type), int(bool(backward))))
    if g < 0:
        raise ValueError(f"fibinet: F={F}, D={D}, R={R} unsupported ({_FIBINET_LIMITS})")
    return g


def _fibinet_args(E, W1, W2, Wb, Wsb, bilinear_type, X, name):
    """-> (B, F, D, R, type, the five input pointers, X's pointer and row stride)."""
    if E.dim() != 3:
        raise ValueError(f"E: expected [B,F,D], got {tuple(E.shape)}")
    if W1.dim() != 2:
        raise ValueError(f"W1: expected [F,R], got {tuple(W1.shape)}")
    B, F, D = (int(v) for v in E.shape)
    R = int(W1.shape[1])
    typ = _fibinet_type(bilinear_type)
    if not fibinet_supported(F, D, R, bilinear_type):
        raise ValueError(f"fibinet: F={F}, D={D}, R={R} unsupported ({_FIBINET_LIMITS})")
    nW = F - 1 if typ else 1
    W, _ = fibinet_width(F, D)
    px, ldx = _strided_rows(X, name, B, W, False)
    ptrs = (_chk(E, "E", F32), _chk(W1, "W1", F32, (F, R)), _chk(W2, "W2", F32, (R, F)),
            _chk(Wb, "Wb", F32, (nW, D, D)), _chk(Wsb, "Wsb", F32, (nW, D, D)))
    return B, F, D, R, typ, ptrs, px, ldx


def fibinet_fwd(E, W1, W2, Wb, Wsb, bilinear_type, X):
    """rm_fibinet_fwd: E [B,F,D], senet_w1 [F,R], senet_w2 [R,F], bilinear_w and senet_bilinear_w [1 | F-1, D, D] ->
    X [B, >= 2PD] (any row stride): [bilinear(E, Wb) | bilinear(a o E, Wsb)], a = relu(relu(mean_d(E) W1) W2); only
    the first 2PD columns of a row are written."""
    B, F, D, R, typ, ptrs, px, ldx = _fibinet_args(E, W1, W2, Wb, Wsb, bilinear_type, X, "X")
    _lib.call("rm_fibinet_fwd", *ptrs, B, F, D, R, typ, px, ldx, _stream())


def fibinet_bwd_workspace(B, F, D, R, bilinear_type):
    """Floats of workspace for fibinet_bwd (rm_fibinet_bwd_workspace): the blocks' partial parameter gradients."""
    n = int(_lib.lib().rm_fibinet_bwd_workspace(int(B), int(F), int(D), int(R), _fibinet_type(bilinear_type)))
    if n < 0:
        raise ValueError(f"fibinet: B={B}, F={F}, D={D}, R={R} unsupported ({_FIBINET_LIMITS})")
    return n


def fibinet_bwd(E, W1, W2, Wb, Wsb, bilinear_type, dX, dE, dW1, dW2, dWb, dWsb, workspace):
    """rm_fibinet_bwd: dX [B, >= 2PD] (any row stride; columns >= 2PD are never read) -> dE [B,F,D] and the gradients
    of the four weight arrays, all overwritten.  The gate and the left products are recomputed.  Deterministic."""
    B, F, D, R, typ, ptrs, px, ldx = _fibinet_args(E, W1, W2, Wb, Wsb, bilinear_type, dX, "dX")
    _need_workspace("fibinet_bwd", workspace, fibinet_bwd_workspace(B, F, D, R, bilinear_type))
    _lib.call("rm_fibinet_bwd", *ptrs, px, ldx, B, F, D, R, typ, _chk(dE, "dE", F32, (B, F, D)),
              _chk(dW1, "dW1", F32, tuple(W1.shape)), _chk(dW2, "dW2", F32, tuple(W2.shape)),
              _chk(dWb, "dWb", F32, tuple(Wb.shape)), _chk(dWsb, "dWsb", F32, tuple(Wsb.shape)),
              _chk(workspace, "workspace", F32), _stream())


# ---- field-pair weighted FM: FmFM / FvFM / FwFM (csrc/fmfm.hip) ----------------------------------------------------
FMFM_TYPES = {"matrix": 0, "vector": 1, "scalar": 2}  # RM_FMFM_MATRIX / RM_FMFM_VECTOR / RM_FMFM_SCALAR
FMFM_TILE = {"fwd": 0, "de": 1, "dw": 2, "fwd_cap": 3, "de_cap": 4, "dw_cap": 5}  # RM_FMFM_TILE_* / RM_FMFM_CAP_*
_FMFM_LIMITS = "2 <= F <= 40, D in 8, 16, 32, type 'matrix', 'vector' or 'scalar'"


def _fmfm_type(field_interaction):
    if field_interaction not in FMFM_TYPES:
        raise ValueError(f"fmfm: field_interaction {field_interaction!r} unsupported ({_FMFM_LIMITS})")
    return FMFM_TYPES[field_interaction]


def fmfm_supported(F, D, field_interaction):
    """rm_fmfm_supported: D in {8, 16, 32}, 2 <= F <= 40, type "matrix", "vector" or "scalar"."""
    if field_interaction not in FMFM_TYPES:
        return False
    return bool(_lib.lib().rm_fmfm_supported(int(F), int(D), FMFM_TYPES[field_interaction]))


def fmfm_weight_shape(F, D, field_interaction):
    """The shape of field_pair_w: [P,D,D] (matrix), [P,D] (vector) or [P] (scalar), P = F(F-1)/2."""
    P = F * (F - 1) // 2
    return {0: (P, D, D), 1: (P, D), 2: (P,)}[_fmfm_type(field_interaction)]


def fmfm_tile(F, D, field_interaction, which):
    """rm_fmfm_tile: which in FMFM_TILE - the examples per tile of the forward ("fwd"), dE ("de") or dW ("dw") kernel,
    or the cap of their grids / batch slices ("fwd_cap", "de_cap", "dw_cap")."""
    v = int(_lib.lib().rm_fmfm_tile(int(F), int(D), _fmfm_type(field_interaction), FMFM_TILE[which]))
    if v < 0:
        raise ValueError(f"fmfm: F={F}, D={D} unsupported ({_FMFM_LIMITS})")
    return v


def _fmfm_args(E, W, field_interaction):
    """-> (B, F, D, type, E's and W's pointers)."""
    if E.dim() != 3:
        raise ValueError(f"E: expected [B,F,D], got {tuple(E.shape)}")
    B, F, D = (int(v) for v in E.shape)
    typ = _fmfm_type(field_interaction)
    if not fmfm_supported(F, D, field_interaction):
        raise ValueError(f"fmfm: F={F}, D={D} unsupported ({_FMFM_LIMITS})")
    return B, F, D, typ, _chk(E, "E", F32), _chk(W, "W", F32, fmfm_weight_shape(F, D, field_interaction))


def fmfm_fwd(E, W, field_interaction, logit):
    """rm_fmfm_fwd: E [B,F,D], field_pair_w [P,D,D] | [P,D] | [P] -> logit [B] = sum_{i<j} E_i W_(ij) E_j^T."""
    B, F, D, typ, pe, pw = _fmfm_args(E, W, field_interaction)
    _lib.call("rm_fmfm_fwd", pe, pw, typ, B, F, D, _chk(logit, "logit", F32, (B,)), _stream())


def fmfm_bwd_workspace(B, F, D, field_interaction):
    """Floats of workspace for fmfm_bwd (rm_fmfm_bwd_workspace): the batch slices' partial weight gradients."""
    n = int(_lib.lib().rm_fmfm_bwd_workspace(int(B), int(F), int(D), _fmfm_type(field_interaction)))
    if n < 0:
        raise ValueError(f"fmfm: B={B}, F={F}, D={D} unsupported ({_FMFM_LIMITS})")
    return n


def fmfm_bwd(E, W, field_interaction, g, d_rows, dW, workspace, dE_up=None):
    """rm_fmfm_bwd: g [B] = dLoss/dlogit -> d_rows [B,F,D] = dLoss/dE (+ dE_up, which may be d_rows itself) and dW
    (the shape of W), both overwritten.  Deterministic."""
    B, F, D, typ, pe, pw = _fmfm_args(E, W, field_interaction)
    _need_workspace("fmfm_bwd", workspace, fmfm_bwd_workspace(B, F, D, field_interaction))
    _lib.call("rm_fmfm_bwd", pe, pw, typ, _chk(g, "g", F32, (B,)), _chk(dE_up, "dE_up", F32, (B, F, D), allow_none=True),
              B, F, D, _chk(d_rows, "d_rows", F32, (B, F, D)), _chk(dW, "dW", F32, tuple(W.shape)),
              _chk(workspace, "workspace", F32), _stream())


# ---- PNN's product layer: inner products and kernel-form outer products per field pair (csrc/pnn.hip) --------------
PNN_INNER, PNN_OUTER = 1, 2  # RM_PNN_INNER / RM_PNN_OUTER: the bits of `products`
PNN_KERNELS = {"mat": 0, "vec": 1, "num": 2}  # RM_PNN_MAT / RM_PNN_VEC / RM_PNN_NUM
PNN_TILE = {"fwd": 0, "de": 1, "dk": 2, "fwd_cap": 3, "de_cap": 4, "dk_cap": 5}  # RM_PNN_TILE_* / RM_PNN_CAP_*
_PNN_LIMITS = "2 <= F <= 40, D in 8, 16, 32, products 1 (inner), 2 (outer) or 3, kernel_type 'mat', 'vec' or 'num'"


def _pnn_kernel(kernel_type):
    if kernel_type not in PNN_KERNELS:
        raise ValueError(f"pnn: kernel_type {kernel_type!r} unsupported ({_PNN_LIMITS})")
    return PNN_KERNELS[kernel_type]


def _pnn_products(products):
    if products not in (1, 2, 3):
        raise ValueError(f"pnn: products {products!r} unsupported ({_PNN_LIMITS})")
    return int(products)


def pnn_products(use_inner, use_outer):
    """The `products` bit set of the two switches (0 when neither is on: no entry point takes that)."""
    return (PNN_INNER if use_inner else 0) | (PNN_OUTER if use_outer else 0)


def pnn_supported(F, D, products, kernel_type):
    """rm_pnn_supported: D in {8, 16, 32}, 2 <= F <= 40, products 1..3, kernel_type "mat", "vec" or "num"."""
    if kernel_type not in PNN_KERNELS or products not in (1, 2, 3):
        return False
    return bool(_lib.lib().rm_pnn_supported(int(F), int(D), int(products), PNN_KERNELS[kernel_type]))


def pnn_weight_shape(F, D, kernel_type):
    """The shape of product_kernel: [P,D,D] (mat), [P,D] (vec) or [P] (num), P = F(F-1)/2."""
    P = F * (F - 1) // 2
    return {0: (P, D, D), 1: (P, D), 2: (P,)}[_pnn_kernel(kernel_type)]


def pnn_width(F, D, products):
    """(W, ldx): the columns the product layer writes (the F D row floats, then P = F(F-1)/2 per selected product)
    and that width rounded up to a multiple of 4 floats (16-byte rows for the dense kernels that read X)."""
    n = bin(_pnn_products(products)).count("1")
    W = F * D + n * (F * (F - 1) // 2)
    return W, (W + 3) // 4 * 4


def pnn_tile(F, D, products, kernel_type, which):
    """rm_pnn_tile: which in PNN_TILE - the examples per tile of the forward ("fwd"), dE ("de") or dK ("dk") kernel,
    or the cap of their grids / batch slices ("fwd_cap", "de_cap", "dk_cap"); the dK entries are 0 without OUTER."""
    v = int(_lib.lib().rm_pnn_tile(int(F), int(D), _pnn_products(products), _pnn_kernel(kernel_type), PNN_TILE[which]))
    if v < 0:
        raise ValueError(f"pnn: F={F}, D={D} unsupported ({_PNN_LIMITS})")
    return v


def _pnn_args(E, K, products, kernel_type, X, name):
    """-> (B, F, D, products, kernel type, E's and K's pointers, X's pointer and row stride)."""
    if E.dim() != 3:
        raise ValueError(f"E: expected [B,F,D], got {tuple(E.shape)}")
    B, F, D = (int(v) for v in E.shape)
    kt, products = _pnn_kernel(kernel_type), _pnn_products(products)
    if not pnn_supported(F, D, products, kernel_type):
        raise ValueError(f"pnn: F={F}, D={D} unsupported ({_PNN_LIMITS})")
    outer = bool(products & PNN_OUTER)
    pk = _chk(K, "K", F32, pnn_weight_shape(F, D, kernel_type), allow_none=not outer)
    px, ldx = _strided_rows(X, name, B, pnn_width(F, D, products)[0], False)
    return B, F, D, products, kt, _chk(E, "E", F32), pk, px, ldx


def pnn_fwd(E, K, products, kernel_type, X):
    """rm_pnn_fwd: E [B,F,D], product_kernel [P,D,D] | [P,D] | [P] (None without OUTER) -> X [B, >= W] with row
    stride ldx: [E flattened | <E_i, E_j> (INNER) | E_i K_(ij) E_j^T (OUTER)], pairs i < j in combinations order;
    every column from W up to the row stride is set to +0.0."""
    B, F, D, products, kt, pe, pk, px, ldx = _pnn_args(E, K, products, kernel_type, X, "X")
    _lib.call("rm_pnn_fwd", pe, pk, products, kt, B, F, D, px, ldx, _stream())


def pnn_bwd_workspace(B, F, D, products, kernel_type):
    """Floats of workspace for pnn_bwd (rm_pnn_bwd_workspace): the batch slices' partial kernel gradients (0 without
    OUTER)."""
    n = int(_lib.lib().rm_pnn_bwd_workspace(int(B), int(F), int(D), _pnn_products(products), _pnn_kernel(kernel_type)))
    if n < 0:
        raise ValueError(f"pnn: B={B}, F={F}, D={D} unsupported ({_PNN_LIMITS})")
    return n


def pnn_bwd(E, K, products, kernel_type, dX, d_rows, dK, workspace):
    """rm_pnn_bwd: dX [B, >= W] (any row stride; columns >= W are never read) -> d_rows [B,F,D] = dX[:, :FD] + dLoss/dE
    through the products, and dK (the shape of K), both overwritten.  K, dK and workspace may be None without OUTER.
    Deterministic."""
    B, F, D, products, kt, pe, pk, px, ldx = _pnn_args(E, K, products, kernel_type, dX, "dX")
    outer = bool(products & PNN_OUTER)
    if outer:
        if workspace is None:
            raise ValueError("workspace must not be None")
        _need_workspace("pnn_bwd", workspace, pnn_bwd_workspace(B, F, D, products, kernel_type))
    _lib.call("rm_pnn_bwd", pe, pk, products, kt, px, ldx, B, F, D, _chk(d_rows, "d_rows", F32, (B, F, D)),
              _chk(dK, "dK", F32, pnn_weight_shape(F, D, kernel_type), allow_none=not outer),
              _chk(workspace, "workspace", F32, allow_none=not outer), _stream())


# ---- MaskNet: group-LayerNorm times masks, row-LayerNorm + ReLU (csrc/masknet.hip) ----------------------------------
MASKNET_TILE = {"tile": 0, "cap": 1}  # RM_MASKNET_TILE / RM_MASKNET_CAP
_MASKNET_GROUP_LIMITS = ("normalize: 1 <= F <= 40, D in 8, 16, 32, 1..8 masks; normalize=False: one [B,H] input, one "
                         "mask, H a multiple of 4 in 8..2048")
_MASKNET_ROW_LIMITS = "H a multiple of 4 in 8..2048, row strides multiples of 4"


def masknet_group_supported(F, D, N, normalize=True):
    """rm_masknet_group_supported: normalize: D in {8, 16, 32}, 1 <= F <= 40, 1 <= N <= 8; otherwise F = 1, N = 1 and
    D (= H) a multiple of 4 in 8..2048."""
    return bool(_lib.lib().rm_masknet_group_supported(int(F), int(D), int(N), int(bool(normalize))))


def masknet_group_tile(F, D, which, normalize=True):
    """rm_masknet_group_tile: which in MASKNET_TILE - the examples per block pass ("tile") or the grid cap ("cap")."""
    v = int(_lib.lib().rm_masknet_group_tile(int(F), int(D), int(bool(normalize)), MASKNET_TILE[which]))
    if v < 0:
        raise ValueError(f"masknet_group: F={F}, D={D} unsupported ({_MASKNET_GROUP_LIMITS})")
    return v


def _masknet_rows(ts, name, B, W):
    """A list of [B, W] f32 device tensors with unit column stride and ONE common row stride >= W -> (pointer
    array, stride)."""
    ld = None
    for n, t in enumerate(ts):
        if t is None or not t.is_cuda or t.dtype != F32 or t.dim() != 2 or tuple(t.shape) != (B, W) or (
                W > 1 and t.stride(1) != 1):
            raise ValueError(f"{name}[{n}]: expected a [{B},{W}] float32 device tensor with unit column stride")
        s = t.stride(0) if B > 1 else W  # (a single row has no stride to speak of)
        if s < W:
            raise ValueError(f"{name}[{n}]: unsupported row stride {s} < {W}")
        if ld is None:
            ld = s
        elif s != ld:
            raise ValueError(f"{name}: unsupported mix of row strides ({s} != {ld}): one stride per list")
    return _ptr_array(ts), int(W if ld is None else ld)


def _masknet_group_args(X, gamma, beta, N, normalize):
    """-> (B, F, D, X's, gamma's and beta's pointers)."""
    if normalize:
        if X.dim() != 3:
            raise ValueError(f"X: expected [B,F,D], got {tuple(X.shape)}")
        B, F, D = (int(v) for v in X.shape)
    else:
        if X.dim() != 2:
            raise ValueError(f"X: expected [B,H], got {tuple(X.shape)}")
        B, F, D = int(X.shape[0]), 1, int(X.shape[1])
    if not masknet_group_supported(F, D, N, normalize):
        raise ValueError(f"masknet_group: F={F}, D={D}, {N} masks unsupported ({_MASKNET_GROUP_LIMITS})")
    px = _chk(X, "X", F32)
    if not normalize:
        if gamma is not None or beta is not None:
            raise ValueError("masknet_group: normalize=False takes no gamma / beta")
        return B, F, D, px, None, None
    return B, F, D, px, _chk(gamma, "gamma", F32, (F, D)), _chk(beta, "beta", F32, (F, D))


def masknet_group_fwd(X, gamma, beta, M, Y, normalize=True):
    """rm_masknet_group_fwd: X = E [B,F,D], gamma / beta [F,D], M and Y lists of N [B,FD] tensors (rows of any common
    stride: column ranges of a wider buffer are fine) -> Y[n] = M[n] o LN_rows(E).  normalize=False: X = h_prev
    [B,H], one mask: Y[0] = M[0] o X."""
    if len(M) != len(Y):
        raise ValueError("masknet_group_fwd: M and Y differ in length")
    B, F, D, px, pg, pb = _masknet_group_args(X, gamma, beta, len(M), normalize)
    pm, ldm = _masknet_rows(M, "M", B, F * D)
    py, ldy = _masknet_rows(Y, "Y", B, F * D)
    _lib.call("rm_masknet_group_fwd", px, pg, pb, int(bool(normalize)), pm, ldm, len(M), B, F, D, py, ldy, _stream())


def masknet_group_bwd_workspace(B, F, D):
    """Floats of workspace for masknet_group_bwd (rm_masknet_group_bwd_workspace): the partial dgamma | dbeta sets."""
    n = int(_lib.lib().rm_masknet_group_bwd_workspace(int(B), int(F), int(D)))
    if n < 0:
        raise ValueError(f"masknet_group: B={B}, F={F}, D={D} unsupported ({_MASKNET_GROUP_LIMITS})")
    return n


def masknet_group_bwd(X, gamma, beta, M, dY, dM, d_rows, dgamma=None, dbeta=None, workspace=None, dE_up=None,
                      normalize=True):
    """rm_masknet_group_bwd: dM[n] = dY[n] o V (dM[n] may be dY[n] itself), d_rows = the LayerNorm backward of
    sum_n dY[n] o M[n] (+ dE_up, which may be d_rows itself), dgamma / dbeta [F,D]; all overwritten, deterministic.
    normalize=False: dM[0] = dY[0] o X, d_rows [B,H] = dY[0] o M[0] (+ dE_up); no parameters, no workspace."""
    if not (len(M) == len(dY) == len(dM)):
        raise ValueError("masknet_group_bwd: M, dY and dM differ in length")
    B, F, D, px, pg, pb = _masknet_group_args(X, gamma, beta, len(M), normalize)
    pm, ldm = _masknet_rows(M, "M", B, F * D)
    pdy, lddy = _masknet_rows(dY, "dY", B, F * D)
    pdm, lddm = _masknet_rows(dM, "dM", B, F * D)
    pdg = pdb = pws = None
    if normalize:
        pdg, pdb = _chk(dgamma, "dgamma", F32, (F, D)), _chk(dbeta, "dbeta", F32, (F, D))
        pws = _chk(workspace, "workspace", F32)
        _need_workspace("masknet_group_bwd", workspace, masknet_group_bwd_workspace(B, F, D))
    _lib.call("rm_masknet_group_bwd", px, pg, pb, int(bool(normalize)), pm, ldm, pdy, lddy, pdm, lddm, len(M),
              _chk(dE_up, "dE_up", F32, tuple(X.shape), allow_none=True), B, F, D,
              _chk(d_rows, "d_rows", F32, tuple(X.shape)), pdg, pdb, pws, _stream())


def masknet_row_supported(H):
    """rm_masknet_row_supported: H a multiple of 4 in 8..2048."""
    return bool(_lib.lib().rm_masknet_row_supported(int(H)))


def masknet_row_tile(H, which):
    """rm_masknet_row_tile: which in MASKNET_TILE - the rows per block pass ("tile") or the grid cap ("cap")."""
    v = int(_lib.lib().rm_masknet_row_tile(int(H), MASKNET_TILE[which]))
    if v < 0:
        raise ValueError(f"masknet_row: H={H} unsupported ({_MASKNET_ROW_LIMITS})")
    return v


def _masknet_row_args(Z, gamma, beta):
    if Z.dim() != 2:
        raise ValueError(f"Z: expected [B,H], got {tuple(Z.shape)}")
    B, H = (int(v) for v in Z.shape)
    if not masknet_row_supported(H):
        raise ValueError(f"masknet_row: H={H} unsupported ({_MASKNET_ROW_LIMITS})")
    return B, H, _chk(Z, "Z", F32), _chk(gamma, "gamma", F32, (H,)), _chk(beta, "beta", F32, (H,))


def _masknet_strided(t, name, B, H):
    p, ld = _masknet_rows([t], name, B, H)
    if ld % 4 or t.data_ptr() % 16:
        raise ValueError(f"{name}: unsupported row stride {ld} or alignment ({_MASKNET_ROW_LIMITS}, 16-byte aligned)")
    return t.data_ptr(), ld


def masknet_row_fwd(Z, gamma, beta, h):
    """rm_masknet_row_fwd: Z [B,H], gamma / beta [H] -> h [B,H] (row stride >= H, a multiple of 4) = relu(LN(Z))."""
    B, H, pz, pg, pb = _masknet_row_args(Z, gamma, beta)
    ph, ldh = _masknet_strided(h, "h", B, H)
    _lib.call("rm_masknet_row_fwd", pz, pg, pb, B, H, ph, ldh, _stream())


def masknet_row_bwd_workspace(B, H):
    """Floats of workspace for masknet_row_bwd (rm_masknet_row_bwd_workspace)."""
    n = int(_lib.lib().rm_masknet_row_bwd_workspace(int(B), int(H)))
    if n < 0:
        raise ValueError(f"masknet_row: B={B}, H={H} unsupported ({_MASKNET_ROW_LIMITS})")
    return n


def masknet_row_bwd(Z, gamma, beta, dh, dZ, dgamma, dbeta, workspace):
    """rm_masknet_row_bwd: dh [B,H] (row stride >= H) -> dZ [B,H], dgamma / dbeta [H] of h = relu(LN(Z)); the
    statistics are recomputed from Z.  Deterministic."""
    B, H, pz, pg, pb = _masknet_row_args(Z, gamma, beta)
    pdh, lddh = _masknet_strided(dh, "dh", B, H)
    _need_workspace("masknet_row_bwd", workspace, masknet_row_bwd_workspace(B, H))
    _lib.call("rm_masknet_row_bwd", pz, pg, pb, pdh, lddh, B, H, _chk(dZ, "dZ", F32, (B, H)),
              _chk(dgamma, "dgamma", F32, (H,)), _chk(dbeta, "dbeta", F32, (H,)), _chk(workspace, "workspace", F32),
              _stream())


ASP_ACTS = {"relu": 0, "sigmoid": 1}  # RM_ASP_RELU / RM_ASP_SIGMOID


def asp_supported(D, hidden, max_len):
    """rm_asp_supported: D in {8, 16, 32}, one or two hidden layers of 1..128 units, 1 <= max_len <= 256."""
    hidden = [int(h) for h in hidden]
    if not hidden:
        return False
    return bool(_lib.lib().rm_asp_supported(int(D), len(hidden), _int_array(hidden), int(max_len)))


def asp_workspace(D, hidden, nnz, backward):
    """Floats of workspace rm_asp_fwd (backward=False) / rm_asp_bwd need (0: unsupported shape)."""
    return int(_lib.lib().rm_asp_workspace(int(D), len(hidden), _int_array(hidden), int(nnz), 1 if backward else 0))


def _asp_params(D, Ws, bs, w, w0):
    hidden = [int(W.shape[1]) for W in Ws]
    dims = [4 * D] + hidden
    if len(Ws) != len(bs) or not 1 <= len(Ws) <= 2:
        # (rejected here with the library's word: there is no slot for a third layer in the C signature)
        raise _lib.RecmanHipError(f"asp: unsupported number of hidden layers {len(Ws)} (1 or 2)")
    ptr = []
    for i in range(2):
        if i < len(Ws):
            ptr += [_chk(Ws[i], f"W{i}", F32, (dims[i], dims[i + 1])), _chk(bs[i], f"b{i}", F32, (dims[i + 1],))]
        else:
            ptr += [None, None]
    ptr += [_chk(w, "w", F32, (hidden[-1],)), _chk(w0, "w0", F32, (1,))]
    return hidden, ptr


def _seq_args(rows, row0, D, offsets, ids, qrow):
    """The arguments every sequence unit's entry points begin with: the fused table, the history's CSR and the query
    rows -> (B, nnz, LD, [rows, LD, D, row0, offsets, ids, qrow, B, nnz] for the call)."""
    if rows.dim() != 2:
        raise ValueError(f"rows: expected [R, LD], got {tuple(rows.shape)}")
    B, nnz, LD = offsets.shape[0] - 1, int(ids.shape[0]), int(rows.shape[1])
    _chk_csr(offsets, ids, None)
    return B, nnz, LD, [_chk(rows, "rows", F32), LD, int(D), int(row0), _chk(offsets, "offsets", I64),
                        _chk(ids, "ids", I64), _chk(qrow, "qrow", I64, (B,)), B, nnz]


def _seq_workspace(fn, workspace, need, aligned=False):
    """A sequence unit's workspace of `need` floats (0: an unsupported shape, which the library names) -> pointer."""
    if need:
        _need_workspace(fn, workspace, need)
    if aligned and workspace.data_ptr() % 16:
        raise ValueError(f"{fn}: workspace must be 16-byte aligned")
    return _chk(workspace, "workspace", F32)


def _seq_grad_views(fn, B, D, d_out, d_query):
    """The two [B, D] gradient views of a sequence unit's backward (column ranges of a wider buffer) -> [d_out's
    pointer, its row stride, d_query's pointer, its row stride]; a single row has no stride to speak of."""
    ptrs = []
    for t, name in ((d_out, "d_out"), (d_query, "d_query")):
        if not t.is_cuda or t.dtype != F32 or tuple(t.shape) != (B, D) or (D > 1 and t.stride(1) != 1):
            raise ValueError(f"{fn}: {name} must be a float32 [B, D] GPU view with unit stride along D")
        ptrs += [t.data_ptr(), t.stride(0) if B > 1 else max(D, t.stride(0))]
    return ptrs


def _param_struct(struct_cls, names, shapes, params, what, unit):
    """{name: tensor} over exactly `names`, each of its shape in `shapes` -> the C struct of their pointers."""
    if set(params) != set(names):
        raise ValueError(f"{unit}: {what} must hold exactly {names}, got {sorted(params)}")
    return struct_cls(*[_chk(params[n], f"{what}[{n!r}]", F32, shapes[n]) for n in names])


def asp_fwd(rows, row0, D, offsets, ids, qrow, Ws, bs, w, w0, act, norm, out, scores, workspace):
    """Attention-pooled history rows (rm_asp_fwd): rows [R, LD] the fused table, history id -> row row0 + id, the
    example's query row qrow [B] (absolute); Ws = [W0 [4D,H0]] or [W0, W1 [H0,H1]], bs alike, w [H_last], w0 [1];
    act "relu" | "sigmoid"; norm: softmax over the example's positions.  -> out [B, LD] (pooled row in columns
    0..D-1, zeros behind) and scores [nnz] (all the backward keeps).  ids.shape[0] must equal offsets[-1]."""
    B, nnz, LD, seq = _seq_args(rows, row0, D, offsets, ids, qrow)
    hidden, pp = _asp_params(D, Ws, bs, w, w0)
    ws = _seq_workspace("asp_fwd", workspace, asp_workspace(D, hidden, nnz, False))
    _lib.call("rm_asp_fwd", *seq, *pp, len(hidden), _int_array(hidden), ASP_ACTS[act], 1 if norm else 0,
              _chk(out, "out", F32, (B, LD)), _chk(scores, "scores", F32, (nnz,)), ws, _stream())


def asp_bwd(rows, row0, D, offsets, ids, qrow, Ws, bs, w, w0, act, norm, scores, d_out, d_keys, d_query, dWs, dbs, dw,
            dw0, workspace):
    """rm_asp_bwd: d_out [B, D] view (row stride may be larger) = the pooled rows' gradient -> d_keys [nnz, D]
    overwritten; the query gradient ADDED onto d_query [B, D] (a view, row stride may be larger); dWs, dbs, dw, dw0
    overwritten.  Deterministic."""
    B, nnz, _, seq = _seq_args(rows, row0, D, offsets, ids, qrow)
    hidden, pp = _asp_params(D, Ws, bs, w, w0)
    _, gp = _asp_params(D, dWs, dbs, dw, dw0)
    do, do_ld, dq, dq_ld = _seq_grad_views("asp_bwd", B, D, d_out, d_query)
    ws = _seq_workspace("asp_bwd", workspace, asp_workspace(D, hidden, nnz, True), aligned=True)
    _lib.call("rm_asp_bwd", *seq, *pp, len(hidden), _int_array(hidden), ASP_ACTS[act], 1 if norm else 0,
              _chk(scores, "scores", F32, (nnz,)), do, do_ld, _chk(d_keys, "d_keys", F32, (nnz, D)), dq, dq_ld, *gp, ws,
              _stream())


BST_PARAM_NAMES = _lib.BST_PARAM_NAMES
BST_LIMITS = ("embedding_size 8/16/32, att_head_num 1/2/4/8 with embedding_size / att_head_num >= 4, att_ffn_units a "
              "multiple of 4 in 4..128, max_len 1..63")


def bst_supported(D, heads, Hf, max_len):
    """rm_bst_supported: D in {8, 16, 32}, heads in {1, 2, 4, 8} with D / heads >= 4, Hf a multiple of 4 in 4..128,
    1 <= max_len <= 63."""
    return bool(_lib.lib().rm_bst_supported(int(D), int(heads), int(Hf), int(max_len)))


def bst_workspace(D, heads, Hf, max_len, B, backward):
    """Floats of workspace rm_bst_fwd (backward=False) / rm_bst_bwd need for B examples (0: unsupported shape)."""
    return int(_lib.lib().rm_bst_workspace(int(D), int(heads), int(Hf), int(max_len), int(B), 1 if backward else 0))


def bst_param_shapes(D, Hf, max_len):
    """name -> shape of the 17 tensors of the transformer unit, in the order of rm_bst_params."""
    s = {n: (D, D) for n in ("wq", "wk", "wv", "wo")}
    s.update({n: (D,) for n in ("bq", "bk", "bv", "bo")})
    s.update(ffn_w1=(D, Hf), ffn_b1=(Hf,), ffn_w2=(Hf, D), ffn_b2=(D,))
    s.update({n: (D,) for n in ("ln1_gamma", "ln1_beta", "ln2_gamma", "ln2_beta")})
    s["pos"] = (max_len + 1, D)
    return {n: s[n] for n in BST_PARAM_NAMES}


def _bst_struct(params, what, D, Hf, max_len):
    return _param_struct(_lib.BstParams, BST_PARAM_NAMES, bst_param_shapes(D, Hf, max_len), params, what, "bst")


def _bst_args(rows, row0, D, offsets, ids, qrow, params, heads, max_len):
    """-> (B, nnz, LD, Hf, the call's arguments up to max_len)."""
    if "ffn_w1" not in params or params["ffn_w1"].dim() != 2:
        raise ValueError("bst: params['ffn_w1'] must be a [D, Hf] matrix")
    Hf = int(params["ffn_w1"].shape[1])
    ps = _bst_struct(params, "params", int(D), Hf, int(max_len))
    B, nnz, LD, seq = _seq_args(rows, row0, D, offsets, ids, qrow)
    return B, nnz, LD, Hf, seq + [ctypes.byref(ps), int(heads), Hf, int(max_len)]


def bst_fwd(rows, row0, D, offsets, ids, qrow, params, heads, max_len, out, workspace):
    """Transformer-pooled history rows (rm_bst_fwd): rows [R, LD] the fused table, history id -> row row0 + id (oldest
    first), the example's query row qrow [B] (absolute); params: {name: tensor} over BST_PARAM_NAMES (shapes:
    bst_param_shapes).  -> out [B, LD]: the mean of the encoder block's T = n + 1 output rows in columns 0..D-1, zeros
    behind.  Nothing is saved for the backward; inference is the same call.  ids.shape[0] must equal offsets[-1]."""
    B, nnz, LD, Hf, args = _bst_args(rows, row0, D, offsets, ids, qrow, params, heads, max_len)
    ws = _seq_workspace("bst_fwd", workspace, bst_workspace(D, heads, Hf, max_len, B, False))
    _lib.call("rm_bst_fwd", *args, _chk(out, "out", F32, (B, LD)), ws, _stream())


def bst_bwd(rows, row0, D, offsets, ids, qrow, params, heads, max_len, d_out, d_keys, d_query, grads, workspace):
    """rm_bst_bwd: d_out [B, D] view (row stride may be larger) = the pooled rows' gradient -> d_keys [nnz, D]
    overwritten; the candidate's gradient ADDED onto d_query [B, D] (a view, row stride may be larger; it may be other
    columns of d_out's buffer); grads: {name: tensor} over BST_PARAM_NAMES, all overwritten.  Deterministic."""
    B, nnz, _, Hf, args = _bst_args(rows, row0, D, offsets, ids, qrow, params, heads, max_len)
    gs = _bst_struct(grads, "grads", int(D), Hf, int(max_len))
    do, do_ld, dq, dq_ld = _seq_grad_views("bst_bwd", B, D, d_out, d_query)
    ws = _seq_workspace("bst_bwd", workspace, bst_workspace(D, heads, Hf, max_len, B, True), aligned=True)
    _lib.call("rm_bst_bwd", *args, do, do_ld, _chk(d_keys, "d_keys", F32, (nnz, D)), dq, dq_ld, ctypes.byref(gs), ws,
              _stream())


DIEN_PARAM_NAMES = _lib.DIEN_PARAM_NAMES
DIEN_LIMITS = "embedding_size 8/16/32, max_len 1..256"


def dien_supported(D, max_len):
    """rm_dien_supported: D in {8, 16, 32}, 1 <= max_len <= 256."""
    return bool(_lib.lib().rm_dien_supported(int(D), int(max_len)))


def dien_workspace(D, max_len, B, nnz, backward):
    """Floats of workspace rm_dien_fwd needs without (backward=False) / with save, and rm_dien_bwd (backward=True), for
    B examples and nnz history positions (0: unsupported shape)."""
    return int(_lib.lib().rm_dien_workspace(int(D), int(max_len), int(B), int(nnz), 1 if backward else 0))


def dien_param_shapes(D):
    """name -> shape of the 7 tensors of the interest-evolution unit, in the order of rm_dien_params."""
    s = {n: (D, 3 * D) for n in ("gru_w", "gru_u", "augru_w", "augru_u")}
    s.update(gru_b=(3 * D,), augru_b=(3 * D,), att_w=(D, D))
    return {n: s[n] for n in DIEN_PARAM_NAMES}


def _dien_struct(params, what, D):
    return _param_struct(_lib.DienParams, DIEN_PARAM_NAMES, dien_param_shapes(int(D)), params, what, "dien")


def _dien_args(rows, row0, D, offsets, ids, qrow, params, max_len):
    """-> (B, nnz, LD, the call's arguments up to max_len)."""
    ps = _dien_struct(params, "params", D)
    B, nnz, LD, seq = _seq_args(rows, row0, D, offsets, ids, qrow)
    return B, nnz, LD, seq + [ctypes.byref(ps), int(max_len)]


def dien_fwd(rows, row0, D, offsets, ids, qrow, params, max_len, save, out, workspace):
    """Interest-evolution pooling of the history rows (rm_dien_fwd): rows [R, LD] the fused table, history id -> row
    row0 + id (oldest first), the example's query row qrow [B] (absolute); params: {name: tensor} over DIEN_PARAM_NAMES
    (shapes: dien_param_shapes).  -> out [B, LD]: the AUGRU's last state in columns 0..D-1, zeros behind (no history:
    a zero row).  save: keep what dien_bwd needs in the workspace (dien_workspace(.., backward=save) floats); `out` has
    the same bits either way.  ids.shape[0] must equal offsets[-1]."""
    B, nnz, LD, args = _dien_args(rows, row0, D, offsets, ids, qrow, params, max_len)
    ws = _seq_workspace("dien_fwd", workspace, dien_workspace(D, max_len, B, nnz, bool(save)))
    _lib.call("rm_dien_fwd", *args, 1 if save else 0, _chk(out, "out", F32, (B, LD)), ws, _stream())


def dien_bwd(rows, row0, D, offsets, ids, qrow, params, max_len, d_out, d_keys, d_query, grads, workspace):
    """rm_dien_bwd, after dien_fwd(save=True) on the same inputs and workspace: d_out [B, D] view (row stride may be
    larger) = the pooled rows' gradient -> d_keys [nnz, D] overwritten; the query gradient ADDED onto d_query [B, D]
    (a view, row stride may be larger; it may be other columns of d_out's buffer); grads: {name: tensor} over
    DIEN_PARAM_NAMES, all overwritten.  Deterministic."""
    B, nnz, _, args = _dien_args(rows, row0, D, offsets, ids, qrow, params, max_len)
    gs = _dien_struct(grads, "grads", D)
    do, do_ld, dq, dq_ld = _seq_grad_views("dien_bwd", B, D, d_out, d_query)
    ws = _seq_workspace("dien_bwd", workspace, dien_workspace(D, max_len, B, nnz, True), aligned=True)
    _lib.call("rm_dien_bwd", *args, do, do_ld, _chk(d_keys, "d_keys", F32, (nnz, D)), dq, dq_ld, ctypes.byref(gs), ws,
              _stream())


def gather_rows(table, rows, out):
    """out[i, :] = table[rows[i], :width] with width = out.shape[1] <= table.shape[1] (the shard keeps
    optimizer state behind the exchanged columns).  `table` may live in PINNED host memory (th/feeder.py)."""
    n = rows.shape[0]
    width = out.shape[1]
    tp, ld, cols = _rows2d(table, "table", allow_pinned=True)  # (a [:, :width] view of a wider shard is fine)
    if cols < width:
        raise ValueError(f"gather_rows: table has {cols} columns, out needs {width}")
    _lib.call("rm_gather_rows", tp, ld, _chk(rows, "rows", I64, (n,)), n, width,
              _chk(out, "out", F32, (n, width)), _stream())


def permute_rows(src, slot, dst, inverse=False):
    n, width = src.shape
    _lib.call("rm_permute_rows", _chk(src, "src", F32), _chk(slot, "slot", I64, (n,)), n, width,
              1 if inverse else 0, _chk(dst, "dst", F32, (n, width)), _stream())


ACT_IDS = {"identity": 0, "relu": 1, "leaky_relu": 2}


def cin_filter_workspace(m, H, N):
    return int(_lib.lib().rm_cin_filter_workspace(m, H, N))


def cin_filter_workspace6(m, H, N, D):
    """Floats of filter workspace for the bf16x6 form of cin_layer_fwd (0: the shape is not covered)."""
    return int(_lib.lib().rm_cin_filter_workspace6(int(m), int(H), int(N), int(D)))


def cin_layer_fwd(X0, Xk, H, W, bias, act, out, filter_ws, pooled=None, pool_col0=0, pool_from=0, ws6=None,
                  first6=False):
    """One CIN layer forward.  X0 [B,m,D]; Xk [B,Hk,D] of which rows j < H are used;
    W [m*H, N]; out [B,N,D]; pooled [B, P] gets sum_d out[:, pool_from:, :] at pool_col0.
    ws6 (cin_filter_workspace6 floats): on the bf16 matrix pipe with split operands (rm_cin_layer_fwd6) when that
    kernel covers the layer; returns True when it ran."""
    B, m, D = X0.shape
    N = W.shape[1]
    if ws6 is not None and (first6 or Xk.data_ptr() != X0.data_ptr()):
        need = cin_filter_workspace6(m, H, N, D)
        if need > 0 and ws6.numel() >= need:
            if W.shape[0] != m * H or Xk.shape[0] != B or Xk.shape[2] != D or Xk.shape[1] < H:
                raise ValueError("cin_layer_fwd: shape mismatch")
            _lib.call(
                "rm_cin_layer_fwd6", _chk(X0, "X0", F32), _chk(Xk, "Xk", F32), Xk.shape[1] * D,
                _chk(W, "W", F32), _chk(bias, "bias", F32, (N,)), ACT_IDS[act], B, m, H, N, D,
                _chk(out, "out", F32, (B, N, D)), _chk(pooled, "pooled", F32, allow_none=True),
                0 if pooled is None else pooled.shape[1], pool_col0, pool_from,
                _chk(ws6, "ws6", F32), _stream())
            return True
    if W.shape[0] != m * H:
        raise ValueError(f"cin_layer_fwd: filter has {W.shape[0]} rows, expected m*H = {m * H}")
    if Xk.shape[0] != B or Xk.shape[2] != D or Xk.shape[1] < H:
        raise ValueError("cin_layer_fwd: Xk shape mismatch")
    if filter_ws.numel() < cin_filter_workspace(m, H, N):
        raise ValueError("cin_layer_fwd: filter workspace too small")
    _lib.call(
        "rm_cin_layer_fwd", _chk(X0, "X0", F32), _chk(Xk, "Xk", F32), Xk.shape[1] * D,
        _chk(W, "W", F32), _chk(bias, "bias", F32, (N,)), ACT_IDS[act], B, m, H, N, D,
        _chk(out, "out", F32, (B, N, D)), _chk(pooled, "pooled", F32, allow_none=True),
        0 if pooled is None else pooled.shape[1], pool_col0, pool_from,
        _chk(filter_ws, "filter_ws", F32), _stream())


def cin_bwd_workspace(B, m, H, N, D):
    return int(_lib.lib().rm_cin_bwd_workspace(B, m, H, N, D))


def cin_layer_bwd(X0, Xk, H, W, act, out, g, dX0, dW, dbias, workspace, *, xk_is_x0=False,
                  d_hidden=None, cin_w_direct=None, pool_from=0, accumulate_dx0=True, dXk=None, split=False,
                  first6=False):
    """One CIN layer backward (see rm_cin_layer_bwd).  d_hidden [B,pool_from,D] is the next
    layer's dXk; cin_w_direct [N-pool_from] the cin_w entries of this layer's direct half.  split: the dX pass on
    the bf16 matrix pipe with split fp32 operands where csrc/cin6.hip covers the layer."""
    B, m, D = X0.shape
    N = W.shape[1]
    if workspace.numel() < cin_bwd_workspace(B, m, H, N, D):
        raise ValueError("cin_layer_bwd: workspace too small")
    _lib.call(
        "rm_cin_layer_bwd", _chk(X0, "X0", F32), _chk(Xk, "Xk", F32), Xk.shape[1] * D,
        1 if xk_is_x0 else 0, _chk(W, "W", F32, (m * H, N)), ACT_IDS[act],
        _chk(out, "out", F32, (B, N, D)), _chk(d_hidden, "d_hidden", F32, allow_none=True),
        0 if d_hidden is None else d_hidden.shape[1] * D, _chk(g, "g", F32, (B,)),
        _chk(cin_w_direct, "cin_w_direct", F32, (N - pool_from,), allow_none=True), pool_from,
        B, m, H, N, D, _chk(dX0, "dX0", F32, (B, m, D)), (1 if accumulate_dx0 else 0) | (2 if split else 0) | (4 if first6 else 0),
        _chk(dXk, "dXk", F32, allow_none=True), 0 if dXk is None else dXk.shape[1] * D,
        _chk(dW, "dW", F32, (m * H, N)), _chk(dbias, "dbias", F32, (N,)),
        _chk(workspace, "workspace", F32), workspace.numel(), _stream())


def rowdot(X, w, w0, out):
    """out[b] = X[b,:] . w + w0 (the [*,1] output projections)."""
    B, P_ = X.shape
    _lib.call("rm_rowdot", _chk(X, "X", F32), _chk(w, "w", F32, (P_,)),
              _chk(w0, "w0", F32, (1,), allow_none=True), B, P_, _chk(out, "out", F32, (B,)),
              _stream())


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _int_array(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def mlp_supported(FD, Dn, hidden):
    return bool(_lib.lib().rm_mlp_supported(FD, Dn, len(hidden), _int_array(hidden)))


def mlp_bwd_workspace(FD, Dn):
    return int(_lib.lib().rm_mlp_bwd_workspace(FD, Dn))


def mlp_tail(B, branches, coef_mlp, *, y=None, y_f=None, task="classification", grad_scale=1.0,
             logit=None, pred=None, dlogit, loss_partial, loss=None, dh):
    """Builds the rm_mlp_tail struct of the fused training head (see include/recman_hip.h):
    branches = up to two (tensor [B], coefficient) pairs summed BEFORE the MLP's own logit; coef_mlp must be 1
    (dlogit then is the MLP's own output gradient, which the dh chain and mlp_bwd take it for).
    Returns the struct; pass it to mlp_fwd and then to mlp_bwd (the tensors must stay alive)."""
    if len(branches) > 2:
        raise ValueError("mlp_tail takes at most two other branch logits")
    if (y is None) == (y_f is None):
        raise ValueError("mlp_tail needs exactly one of y / y_f")
    if float(coef_mlp) != 1.0:
        raise ValueError("mlp_tail: coef_mlp must be 1 (dlogit is the MLP's own output gradient: see rm_mlp_tail)")
    if loss_partial.numel() < (B + 31) // 32:
        raise ValueError("mlp_tail: loss_partial needs ceil(B/32) floats")
    t = _lib.MlpTail()
    for name, i in (("a", 0), ("b", 1)):
        if i < len(branches):
            setattr(t, f"logit_{name}", _chk(branches[i][0], f"logit_{name}", F32, (B,)))
            setattr(t, f"coef_{name}", float(branches[i][1]))
    t.coef_mlp = float(coef_mlp)
    t.y = _chk(y, "y", I64, (B,), allow_none=True)
    t.y_f = _chk(y_f, "y_f", F32, (B,), allow_none=True)
    t.task = 0 if task == "classification" else 1
    t.grad_scale = float(grad_scale)
    t.logit = _chk(logit, "logit", F32, (B,), allow_none=True)
    t.pred = _chk(pred, "pred", F32, (B,), allow_none=True)
    t.dlogit = _chk(dlogit, "dlogit", F32, (B,))
    t.loss_partial = _chk(loss_partial, "loss_partial", F32)
    t.loss = _chk(loss, "loss", F32, (1,), allow_none=True)
    for l, d in enumerate(dh):
        t.dh[l] = _chk(d, f"dh[{l}]", F32, (B, 32))
    return t


def _tail_ref(tail):
    import ctypes

    return None if tail is None else ctypes.cast(ctypes.pointer(tail), ctypes.c_void_p)


def mlp_fwd(xe, xd, Ws, bs, w_out, w0_out, act, h_out, logit, tail=None):
    """Fused skinny-MLP forward.  Ws[l] / bs[l]: layer weights; h_out[l] [B,32].
    tail (mlp_tail(...)): also the final logit, prediction, loss terms, dLoss/dlogit and the dh chain."""
    B, FD = xe.shape
    Dn = 0 if xd is None else xd.shape[1]
    H = [W.shape[1] for W in Ws]
    for l, W in enumerate(Ws):
        _chk(W, f"W[{l}]", F32, (FD + Dn if l == 0 else H[l - 1], H[l]))
        _chk(bs[l], f"bias[{l}]", F32, (H[l],))
        _chk(h_out[l], f"h_out[{l}]", F32, (B, 32))
    _lib.call("rm_mlp_fwd", _chk(xe, "xe", F32), _chk(xd, "xd", F32, (B, Dn), allow_none=True), FD,
              Dn, len(Ws), _int_array(H), _ptr_array(Ws), _ptr_array(bs),
              _chk(w_out, "w_out", F32, (H[-1],)), _chk(w0_out, "w0_out", F32, (1,)), ACT_IDS[act], B,
              _ptr_array(h_out), _chk(logit, "logit", F32, (B,)), _tail_ref(tail), _stream())


def embed_mlp_fwd_supported(F, D, table_ld, Dn, hidden):
    """rm_embed_mlp_fwd_supported: the one-kernel gather + FM + linear + MLP forward covers this shape."""
    return bool(_lib.lib().rm_embed_mlp_fwd_supported(int(F), int(D), int(table_ld), int(Dn), len(hidden),
                                                      _int_array(list(hidden))))


def embed_mlp_fwd(idx, rows, field_off, D, table_ld, xd, Ws, bs, w_out, w0_out, act, E, h_out, logit,
                  want_bias=False, want_lin=False, lin_w_dense=None, lin_w0=None, fm_sum=None, fm_logit=None,
                  lin_logit=None, stream_rows=False, tail=None):
    """rm_embed_mlp_fwd: rm_embed_fwd (fused rows [D | bias | lin | ...]) + rm_mlp_fwd in one kernel."""
    B, F = idx.shape
    Dn = 0 if xd is None else xd.shape[1]
    H = [W.shape[1] for W in Ws]
    for l, W in enumerate(Ws):
        _chk(W, f"W[{l}]", F32, (F * D + Dn if l == 0 else H[l - 1], H[l]))
        _chk(bs[l], f"bias[{l}]", F32, (H[l],))
        _chk(h_out[l], f"h_out[{l}]", F32, (B, 32))
    if rows.dim() != 2 or rows.shape[1] != table_ld or not rows.is_contiguous():
        raise ValueError("embed_mlp_fwd: rows must be the contiguous fused table [R, table_ld]")
    _lib.call("rm_embed_mlp_fwd", _chk(idx, "idx", I64), _chk(rows, "rows", F32), int(table_ld),
              _chk(field_off, "field_off", I64, (F,)), int(bool(want_bias)), int(bool(want_lin)),
              _chk(lin_w_dense, "lin_w_dense", F32, (Dn,), allow_none=True),
              _chk(lin_w0, "lin_w0", F32, (1,), allow_none=True), _chk(xd, "xd", F32, (B, Dn), allow_none=True),
              Dn, B, F, int(D), _chk(E, "E", F32), _chk(fm_sum, "fm_sum", F32, (B, D), allow_none=True),
              _chk(fm_logit, "fm_logit", F32, (B,), allow_none=True),
              _chk(lin_logit, "lin_logit", F32, (B,), allow_none=True), 1 if stream_rows else 0, len(Ws),
              _int_array(H), _ptr_array(Ws), _ptr_array(bs), _chk(w_out, "w_out", F32, (H[-1],)),
              _chk(w0_out, "w0_out", F32, (1,)), ACT_IDS[act], _ptr_array(h_out), _chk(logit, "logit", F32, (B,)),
              _tail_ref(tail), _stream())


def mlp_bwd(xe, xd, Ws, w_out, act, g, h, d_rows, dh, dW, workspace, fm_sum=None, db=None,
            d_w_out=None, d_w0_out=None, d_xd_wsum=None, d_g_sum=None, tail=None, stream_d_rows=False):
    """tail: the struct the forward ran with - dh is already there (no chain launch) and the
    finishing kernel also reduces the loss.  stream_d_rows: RM_MLP_STREAM_DROWS (non-temporal d_rows
    stores: only when no optimizer step re-reads them)."""
    B, FD = xe.shape
    Dn = 0 if xd is None else xd.shape[1]
    H = [W.shape[1] for W in Ws]
    for l, W in enumerate(Ws):
        _chk(W, f"W[{l}]", F32, (FD + Dn if l == 0 else H[l - 1], H[l]))
        _chk(dW[l], f"dW[{l}]", F32, tuple(W.shape))
        _chk(h[l], f"h[{l}]", F32, (B, 32))
        _chk(dh[l], f"dh[{l}]", F32, (B, 32))
    if workspace.numel() < mlp_bwd_workspace(FD, Dn):
        raise ValueError("mlp_bwd: workspace too small")
    D = 0 if fm_sum is None else fm_sum.shape[1]
    _lib.call("rm_mlp_bwd", _chk(xe, "xe", F32), _chk(xd, "xd", F32, (B, Dn), allow_none=True), FD,
              Dn, len(Ws), _int_array(H), _ptr_array(Ws), _chk(w_out, "w_out", F32, (H[-1],)),
              ACT_IDS[act], B, _chk(g, "g", F32, (B,)), _ptr_array(h),
              _chk(fm_sum, "fm_sum", F32, allow_none=True), D, _chk(d_rows, "d_rows", F32, (B, FD)),
              _ptr_array(dh), _ptr_array(dW), None if db is None else _ptr_array(db),
              _chk(d_w_out, "d_w_out", F32, (H[-1],), allow_none=True),
              _chk(d_w0_out, "d_w0_out", F32, (1,), allow_none=True),
              _chk(d_xd_wsum, "d_xd_wsum", F32, (Dn,), allow_none=True),
              _chk(d_g_sum, "d_g_sum", F32, (1,), allow_none=True),
              _chk(workspace, "workspace", F32), _tail_ref(tail), 1 if stream_d_rows else 0, _stream())


def deepfm_step_supported(F, D, table_ld, Dn, hidden):
    """rm_deepfm_step_supported: the one-kernel DeepFM training step covers this shape."""
    return bool(_lib.lib().rm_deepfm_step_supported(int(F), int(D), int(table_ld), int(Dn), len(hidden),
                                                    _int_array(list(hidden))))


def deepfm_step_workspace(F, Dn):
    return int(_lib.lib().rm_deepfm_step_workspace(int(F), int(Dn)))


def debug_lds_fill(pattern):
    """Test aid (rm_debug_lds_fill): all of every CU's LDS filled with one 32-bit pattern on the current stream - what
    the next kernel finds in LDS before it has written it is known."""
    _lib.call("rm_debug_lds_fill", int(pattern) & 0xFFFFFFFF, _stream())


def debug_lds_probe(pattern, nblocks):
    """Test aid (rm_debug_lds_probe): nblocks workgroups that hold a CU's whole LDS and write none of it; returns
    their counts of words that differ from `pattern` (int32 [nblocks], device)."""
    out = torch.full((int(nblocks),), -1, dtype=torch.int32, device="cuda")
    _lib.call("rm_debug_lds_probe", int(pattern) & 0xFFFFFFFF, out.data_ptr(), int(nblocks), _stream())
    return out


def deepfm_step(idx, rows, field_off, D, table_ld, dense, y, Ws, bs, w_out, w0_out, lin_w_dense, lin_w0, act, task,
                d_rows, logit, pred, dlogit, loss, dW, db, d_w_out, d_w0_out, d_lin_w_dense, d_lin_w0, workspace,
                grad_scale=1.0, stream_rows=False, stream_d_rows=False, skip_finish=False, packed_rows=0,
                lin_field_mask=None):
    """rm_deepfm_step: DeepFM's forward + every gradient in one kernel (+ the finishing reduction; skip_finish =
    measurement only, the parameter gradients and the loss are then not written).  packed_rows > 0: the row-sharded
    form - rows = the received rows [packed_rows, D + 4], idx = positions in it, d_rows = the gradient send buffer
    [packed_rows, D + 4] written in bucketed order (see include/recman_hip.h)."""
    B, F = idx.shape
    Dn = 0 if dense is None else dense.shape[1]
    H = [W.shape[1] for W in Ws]
    for l, W in enumerate(Ws):
        _chk(W, f"W[{l}]", F32, (F * D + Dn if l == 0 else H[l - 1], H[l]))
        _chk(bs[l], f"bias[{l}]", F32, (H[l],))
        _chk(dW[l], f"dW[{l}]", F32, tuple(W.shape))
        _chk(db[l], f"db[{l}]", F32, (H[l],))
    if rows.dim() != 2 or rows.shape[1] != table_ld or not rows.is_contiguous():
        raise ValueError("deepfm_step: rows must be the contiguous fused table [R, table_ld]")
    if packed_rows and (d_rows.numel() < packed_rows * (D + 4) or rows.shape[0] < packed_rows or table_ld != D + 4):
        raise ValueError("deepfm_step: packed form needs rows / d_rows of [packed_rows, D + 4]")
    if rows.shape[0] >= 1 << 32:
        raise ValueError("deepfm_step: the table has more than 2^32 rows")
    if workspace.numel() < deepfm_step_workspace(F, Dn):
        raise ValueError("deepfm_step: workspace too small")
    yk = (_chk(y, "y", I64, (B,)), None) if y.dtype == I64 else (None, _chk(y, "y_f", F32, (B,)))
    _lib.call("rm_deepfm_step", _chk(idx, "idx", I64), _chk(rows, "rows", F32), int(table_ld),
              _chk(field_off, "field_off", I64, (F,)), _chk(dense, "dense", F32, (B, Dn), allow_none=True), Dn,
              yk[0], yk[1], B, F, int(D), len(Ws), _int_array(H), _ptr_array(Ws), _ptr_array(bs),
              _chk(w_out, "w_out", F32, (H[-1],)), _chk(w0_out, "w0_out", F32, (1,)),
              _chk(lin_w_dense, "lin_w_dense", F32, (Dn,), allow_none=True), _chk(lin_w0, "lin_w0", F32, (1,)),
              ACT_IDS[act], 0 if task == "classification" else 1, float(grad_scale),
              _chk(d_rows, "d_rows", F32), _chk(logit, "logit", F32, (B,)), _chk(pred, "pred", F32, (B,)),
              _chk(dlogit, "dlogit", F32, (B,)), _chk(loss, "loss", F32, (1,)), _ptr_array(dW), _ptr_array(db),
              _chk(d_w_out, "d_w_out", F32, (H[-1],)), _chk(d_w0_out, "d_w0_out", F32, (1,)),
              _chk(d_lin_w_dense, "d_lin_w_dense", F32, (Dn,), allow_none=True),
              _chk(d_lin_w0, "d_lin_w0", F32, (1,)), _chk(workspace, "workspace", F32), int(packed_rows),
              _chk(lin_field_mask, "lin_field_mask", F32, (F,), allow_none=True),
              (1 if stream_rows else 0) | (2 if stream_d_rows else 0) | (4 if skip_finish else 0), _stream())


def shard_route(idx, field_off, world, pos, send_ids, counts, workspace):
    B, F = idx.shape
    n = B * F
    need = int(_lib.lib().rm_shard_route_workspace(world))
    if workspace.dtype != torch.int32 or workspace.numel() < need:
        raise ValueError(f"shard_route: workspace must be int32 with >= {need} elements")
    _lib.call("rm_shard_route", _chk(idx, "idx", I64), _chk(field_off, "field_off", I64, (F,)), B, F,
              world, _chk(pos, "pos", I64, (n,)), _chk(send_ids, "send_ids", I64, (n,)),
              _chk(counts, "counts", I64, (world,)), workspace.data_ptr(), _stream())


def shard_route_padded(idx, field_off, world, cap, pos, send_ids, counts, overflow, workspace):
    B, F = idx.shape
    n = B * F
    need = int(_lib.lib().rm_shard_route_workspace(world))
    if workspace.dtype != torch.int32 or workspace.numel() < need:
        raise ValueError(f"shard_route_padded: workspace must be int32 with >= {need} elements")
    if overflow.dtype != torch.int32 or overflow.numel() < 1:
        raise ValueError("shard_route_padded: overflow must be an int32 flag")
    _lib.call("rm_shard_route_padded", _chk(idx, "idx", I64), _chk(field_off, "field_off", I64, (F,)), B, F,
              world, int(cap), _chk(pos, "pos", I64, (n,)), _chk(send_ids, "send_ids", I64, (world * cap,)),
              _chk(counts, "counts", I64, (world,)), overflow.data_ptr(), workspace.data_ptr(), _stream())


def pack_grad_rows(d_rows, g_bias, g_lin, pos, out, lin_field_mask=None):
    B, F, D = d_rows.shape
    n, width = out.shape
    if n < B * F:
        raise ValueError("pack_grad_rows: out must have at least B*F rows")
    _lib.call("rm_pack_grad_rows", _chk(d_rows, "d_rows", F32),
              _chk(g_bias, "g_bias", F32, (B,), allow_none=True),
              _chk(g_lin, "g_lin", F32, (B,), allow_none=True),
              _chk(lin_field_mask, "lin_field_mask", F32, (F,), allow_none=True),
              _chk(pos, "pos", I64, (B * F,)), B, F, D, width, _chk(out, "out", F32), _stream())


OPT_KINDS = {"adam": 0, "adagrad": 1, "gd": 2, "sgd": 2, "ftrl": 3}


def _opt_rule(kind, lr, beta1=0.9, beta2=0.999, eps=1e-7, l1=0.0, l2=0.0, ftrl_beta=0.0):
    """rm_opt_rule of include/recman_hip.h (beta1 / beta2 / eps: Adam, Adagrad; l1 / l2 / ftrl_beta: FTRL)."""
    return _lib.OptRule(OPT_KINDS[kind], float(lr), float(beta1), float(beta2), float(eps), float(l1), float(l2),
                        float(ftrl_beta))


def _opt_rules(kind, lr, beta1, beta2, eps, l1, l2, ftrl_beta, side_kind, side_lr, side_beta1, side_beta2, side_eps,
               side_l1, side_l2, side_ftrl_beta):
    """(embedding rule, side rule) of a row-wise step: every side_* left None takes the embedding rule's value."""
    def pick(x, d):
        return d if x is None else x

    emb = _opt_rule(kind, lr, beta1, beta2, eps, l1, l2, ftrl_beta)
    side = _opt_rule(pick(side_kind, kind), pick(side_lr, lr), pick(side_beta1, beta1), pick(side_beta2, beta2),
                     pick(side_eps, eps), pick(side_l1, l1), pick(side_l2, l2), pick(side_ftrl_beta, ftrl_beta))
    return emb, side


def sparse_optimizer_workspace(n):
    """Bytes of workspace rm_sparse_optimizer_step needs for n occurrences."""
    need = int(_lib.lib().rm_sparse_optimizer_workspace(int(n)))
    if need < 0:
        raise ValueError(f"sparse_optimizer_workspace: bad occurrence count {n}")
    return need


def _opt_ws(workspace, n):
    if workspace.dtype != torch.uint8 or not workspace.is_cuda or workspace.numel() < sparse_optimizer_workspace(n):
        raise ValueError("sparse optimizer: workspace must be a uint8 device tensor of "
                         "sparse_optimizer_workspace(n) bytes")
    return workspace.data_ptr(), workspace.numel()


def sparse_optimizer_prepare(workspace, R, idx=None, field_off=None, row_ids=None, max_field_rows=0):
    """The id-only part of a row-wise step (keys + stable sort) on the current stream
    (rm_sparse_optimizer_prepare); follow it with sparse_optimizer_step(..., prepared=True).
    max_field_rows > 0: the fields own disjoint ascending row ranges of at most that many rows (the sort then runs
    per field on the local ids)."""
    if row_ids is not None:
        n, F = row_ids.numel(), 1
    else:
        n, F = idx.numel(), idx.shape[1]
    wp, wn = _opt_ws(workspace, n)
    _lib.call("rm_sparse_optimizer_prepare", _chk(idx, "idx", I64, allow_none=True),
              _chk(field_off, "field_off", I64, allow_none=True), _chk(row_ids, "row_ids", I64, allow_none=True),
              n, F, int(R), int(max_field_rows), wp, wn, _stream())


def sparse_optimizer_step(idx, field_off, d_rows, rows, mom, workspace, step, kind, lr, D=None,
                          g_bias=None, g_lin=None, reset=False, beta1=0.9, beta2=0.999, eps=1e-7,
                          lin_field_mask=None, prepared=False, l2_embedding=0.0, l2_linear=0.0, max_field_rows=0,
                          l1=0.0, l2=0.0, ftrl_beta=0.0, side_kind=None, side_lr=None, side_beta1=None,
                          side_beta2=None, side_eps=None, side_l1=None, side_l2=None, side_ftrl_beta=None):
    """Lazy row-wise optimizer step on table rows [R, ld] (see rm_sparse_optimizer_step_rules): rows =
    [D emb | bias | lin | m_b | m_l | v_b | v_l | pad], mom [R, 2D] = [m | v] of the embedding ("ftrl": m = z,
    v = n; l1 / l2 / ftrl_beta are its constants).  side_*: another rule for the bias and linear entries (and the
    row's state columns); each one left None takes the value of the embedding rule, so that leaving all of them out
    is one rule for the whole row.  mom may be None when the EMBEDDING rule is "sgd"."""
    B, F, Dg = d_rows.shape
    D = Dg if D is None else D
    R, ld = rows.shape
    if mom is not None:
        _chk(mom, "mom", F32, (R, 2 * D))
    wp, wn = _opt_ws(workspace, B * F)
    emb, side = _opt_rules(kind, lr, beta1, beta2, eps, l1, l2, ftrl_beta, side_kind, side_lr, side_beta1, side_beta2,
                           side_eps, side_l1, side_l2, side_ftrl_beta)
    _lib.call("rm_sparse_optimizer_step_rules", _chk(idx, "idx", I64, (B, F)),
              _chk(field_off, "field_off", I64, (F,)), _chk(d_rows, "d_rows", F32, (B, F, D)),
              _chk(g_bias, "g_bias", F32, (B,), allow_none=True),
              _chk(g_lin, "g_lin", F32, (B,), allow_none=True), B, F, D, R, _chk(rows, "rows", F32), ld,
              None if mom is None else mom.data_ptr(), int(step), ctypes.byref(emb), ctypes.byref(side),
              1 if reset else 0, float(l2_embedding), float(l2_linear),
              _chk(lin_field_mask, "lin_field_mask", F32, (F,), allow_none=True), int(max_field_rows),
              1 if prepared else 0, wp, wn, _stream())


def sparse_optimizer_step_rows(row_ids, grad_rows, D, rows, mom, workspace, step, kind, lr, reset=False,
                               beta1=0.9, beta2=0.999, eps=1e-7, prepared=False, l2_embedding=0.0, l2_linear=0.0,
                               l1=0.0, l2=0.0, ftrl_beta=0.0, side_kind=None, side_lr=None, side_beta1=None,
                               side_beta2=None, side_eps=None, side_l1=None, side_l2=None, side_ftrl_beta=None):
    """The same step from gradient rows that carry their (local) table row: row_ids [n] (< 0: skip),
    grad_rows [n, gw] = [dE | g_bias | g_lin | ...] (rm_sparse_optimizer_step_rows_rules; the rules as in
    sparse_optimizer_step)."""
    n, gw = grad_rows.shape
    R, ld = rows.shape
    if mom is not None:
        _chk(mom, "mom", F32, (R, 2 * D))
    wp, wn = _opt_ws(workspace, n)
    emb, side = _opt_rules(kind, lr, beta1, beta2, eps, l1, l2, ftrl_beta, side_kind, side_lr, side_beta1, side_beta2,
                           side_eps, side_l1, side_l2, side_ftrl_beta)
    _lib.call("rm_sparse_optimizer_step_rows_rules", _chk(row_ids, "row_ids", I64, (n,)),
              _chk(grad_rows, "grad_rows", F32), gw, n, D, R, _chk(rows, "rows", F32), ld,
              None if mom is None else mom.data_ptr(), int(step), ctypes.byref(emb), ctypes.byref(side),
              1 if reset else 0, float(l2_embedding), float(l2_linear), 1 if prepared else 0, wp, wn, _stream())


def dense_optimizer_step(p, g, m, v, step, kind, lr, reset=False, beta1=0.9, beta2=0.999, eps=1e-7, l1=0.0, l2=0.0,
                         ftrl_beta=0.0):
    """One launch over a flat parameter buffer (rm_dense_optimizer_step_rule; "ftrl": m = z, v = n)."""
    n = p.numel()
    rule = _opt_rule(kind, lr, beta1, beta2, eps, l1, l2, ftrl_beta)
    _lib.call("rm_dense_optimizer_step_rule", _chk(p, "p", F32, (n,)), _chk(g, "g", F32, (n,)),
              _chk(m, "m", F32, (n,), allow_none=True), _chk(v, "v", F32, (n,), allow_none=True), n,
              int(step), ctypes.byref(rule), 1 if reset else 0, _stream())


def _chk_csr(offsets, ids, vals):
    if int(offsets.shape[0]) < 1:
        raise ValueError("CSR offsets must have B+1 entries")
    if vals is not None and vals.shape != ids.shape:
        raise ValueError(f"vals {tuple(vals.shape)} must match ids {tuple(ids.shape)}")


def pool_rows(rows, row0, D, offsets, ids, out, vals=None):
    """Pooled fused rows of a multi-valued feature (rm_pool_rows): out [B, LD].  vals=None:
    sqrtn combiner (MultiValCsvFeat); vals [nnz]: value-weighted (SparseValueFeat)."""
    B = offsets.shape[0] - 1
    LD = rows.shape[1]
    _chk_csr(offsets, ids, vals)
    _lib.call("rm_pool_rows", _chk(rows, "rows", F32), int(row0), LD, D, _chk(offsets, "offsets", I64),
              _chk(ids, "ids", I64), _chk(vals, "vals", F32, allow_none=True), B,
              _chk(out, "out", F32, (B, LD)), _stream())


def pool_rows_bwd(d_rows_f, g_bias, g_lin, D, offsets, ids, row0, d_table, d_bias, d_lin, vals=None):
    """d_rows_f: [B, D] view (row stride may be larger) of the pooled rows' gradient."""
    B = offsets.shape[0] - 1
    _chk_csr(offsets, ids, vals)
    if d_rows_f.stride(1) != 1:
        raise ValueError("pool_rows_bwd: d_rows_f must be unit-stride along D")
    _lib.call("rm_pool_rows_bwd", d_rows_f.data_ptr(), d_rows_f.stride(0),
              _chk(g_bias, "g_bias", F32, (B,), allow_none=True),
              _chk(g_lin, "g_lin", F32, (B,), allow_none=True), D, _chk(offsets, "offsets", I64),
              _chk(ids, "ids", I64), _chk(vals, "vals", F32, allow_none=True), B, int(row0),
              _chk(d_table, "d_table", F32),
              _chk(d_bias, "d_bias", F32, allow_none=True), _chk(d_lin, "d_lin", F32, allow_none=True),
              _stream())


def _cols(t, name, dtype, B, T):
    """(data pointer, row stride) of a [B, T] view with unit-stride columns (a column block of a wider matrix)."""
    if t is None:
        return None, 0
    if not t.is_cuda or t.dtype != dtype or tuple(t.shape) != (B, T) or (T > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected a cuda {dtype} [B={B}, T={T}] view with unit-stride columns, got "
                         f"{t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    return t.data_ptr(), t.stride(0)


def pool_rows_padded(rows, D, pos, ids, out, vals=None):
    """rm_pool_rows_padded: pooled rows out [B, LD] from the tag rows rows[pos[b, t]] (ids[b, t] < 0: no tag);
    pos / ids / vals are [B, T] views (column blocks of the occurrence matrix)."""
    B, T = ids.shape
    LD = rows.shape[1]
    pp, pl = _cols(pos, "pos", I64, B, T)
    ip, il = _cols(ids, "ids", I64, B, T)
    vp, vl = _cols(vals, "vals", F32, B, T)
    _lib.call("rm_pool_rows_padded", _chk(rows, "rows", F32), LD, D, pp, pl, ip, il, vp, vl, B, T,
              _chk(out, "out", F32, (B, LD)), _stream())


def pack_pooled_grad_rows(d_rows_f, g_bias, g_lin, D, pos, ids, out, vals=None):
    """rm_pack_pooled_grad_rows: the tags' gradient rows written at out[pos[b, t]] (out [slots, width]);
    d_rows_f: [B, D] view (row stride may be larger) of the pooled rows' gradient."""
    B, T = ids.shape
    if d_rows_f.stride(1) != 1:
        raise ValueError("pack_pooled_grad_rows: d_rows_f must be unit-stride along D")
    pp, pl = _cols(pos, "pos", I64, B, T)
    ip, il = _cols(ids, "ids", I64, B, T)
    vp, vl = _cols(vals, "vals", F32, B, T)
    _lib.call("rm_pack_pooled_grad_rows", d_rows_f.data_ptr(), d_rows_f.stride(0),
              _chk(g_bias, "g_bias", F32, (B,), allow_none=True), _chk(g_lin, "g_lin", F32, (B,), allow_none=True),
              D, pp, pl, ip, il, vp, vl, B, T, out.shape[1], _chk(out, "out", F32), _stream())


def bias_act_(x, bias, act):
    B, N = x.shape
    _lib.call("rm_bias_act", _chk(x, "x", F32), _chk(bias, "bias", F32, (N,), allow_none=True), B, N,
              ACT_IDS[act], _stream())


def outer_actgrad(g, w, a, act, da):
    """da[b,j] = g[b] * w[j] * act'(a[b,j]) (a may be None: no activation factor)."""
    B, N = da.shape
    _lib.call("rm_outer_actgrad", _chk(g, "g", F32, (B,)), _chk(w, "w", F32, (N,)),
              _chk(a, "a", F32, (B, N), allow_none=True), B, N, ACT_IDS[act], _chk(da, "da", F32), _stream())


def outer_actgrad_sums_workspace(B, N):
    return int(_lib.lib().rm_outer_actgrad_sums_workspace(B, N))


def outer_actgrad_sums(g, w, a, act, da, d_w, d_w0, db, workspace):
    """outer_actgrad + d_w[j] = sum_b g[b] a[b,j], d_w0 = sum_b g[b], db[j] = sum_b da[b,j] in one pass."""
    B, N = da.shape
    if workspace.numel() < outer_actgrad_sums_workspace(B, N):
        raise ValueError("outer_actgrad_sums: workspace too small")
    _lib.call("rm_outer_actgrad_sums", _chk(g, "g", F32, (B,)), _chk(w, "w", F32, (N,)),
              _chk(a, "a", F32, (B, N)), B, N, ACT_IDS[act], _chk(da, "da", F32),
              _chk(d_w, "d_w", F32, (N,), allow_none=True), _chk(d_w0, "d_w0", F32, (1,), allow_none=True),
              _chk(db, "db", F32, (N,), allow_none=True), _chk(workspace, "workspace", F32), _stream())


def act_bwd_(da, a, act):
    B, N = da.shape
    _lib.call("rm_act_bwd", _chk(da, "da", F32), _chk(a, "a", F32, (B, N)), B, N, ACT_IDS[act], _stream())


# ---- wide dense layers (csrc/gemm.hip) -------------------------------------------------------
DENSE_BIAS_ACT, DENSE_MUL_ACTGRAD, DENSE_ADD, DENSE_CROSS = 0, 1, 2, 3


def _rows2d(t, name, allow_none=False, allow_pinned=False):
    """A 2-D f32 tensor with unit column stride -> (pointer, leading dimension, columns).  allow_pinned: a
    PINNED host tensor is accepted too (hipHostMalloc'ed memory is mapped into the GPU's address space: a kernel
    reads it over PCIe - the batch feeder's zero-copy gather)."""
    if t is None:
        if allow_none:
            return None, 0, 0
        raise ValueError(f"{name} is required")
    on_dev = t.is_cuda or (allow_pinned and t.is_pinned())
    if t.dtype != F32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or not on_dev:
        raise ValueError(f"{name}: expected a 2-D float32 device tensor with unit column stride, got "
                         f"{t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr(), t.stride(0), t.shape[1]


def dense_filter_workspace(K, N):
    return int(_lib.lib().rm_dense_filter_workspace(int(K), int(N)))


def dense_wgrad_workspace(K, N, M):
    return int(_lib.lib().rm_dense_wgrad_workspace(int(K), int(N), int(M)))


def dense6_workspace(K, N, M):
    """Floats of workspace for the bf16x6 form of dense_fwd (rm_dense6_workspace)."""
    return int(_lib.lib().rm_dense6_workspace(int(K), int(N), int(M)))


def dense_fwd6_supported(a1, a2, epilogue=DENSE_BIAS_ACT, aux2=None, out2=None):
    """Does rm_dense_fwd6 (fp32 operands split into bf16 pieces, csrc/gemm6.hip) take this call?"""
    K1 = a1.shape[1]
    K2 = 0 if a2 is None else a2.shape[1]
    return (epilogue in (DENSE_BIAS_ACT, DENSE_MUL_ACTGRAD, DENSE_ADD) and aux2 is None and out2 is None
            and a1.stride(1) == 1 and a1.stride(0) % 4 == 0 and a1.data_ptr() % 16 == 0 and K1 % 32 + K2 <= 32)


def dense_fwd(a1, a2, W, out, filter_ws, *, transposed=False, bias=None, epilogue=DENSE_BIAS_ACT,
              act="identity", aux1=None, aux2=None, out2=None, ws6=None, dot=None):
    """out[M,N] = epilogue([a1 | a2] @ (W.T if transposed else W)) (rm_dense_fwd).  ws6 (dense6_workspace floats):
    the call runs on the bf16 matrix pipe with split operands (rm_dense_fwd6) when that kernel takes it; returns
    True when it did.  dot = (w [N], w0 [1] or None, out [M]): with rm_dense_fwd6 also out[b] = out_row(b) . w + w0
    (otherwise the caller runs rowdot)."""
    if ws6 is not None and dense_fwd6_supported(a1, a2, epilogue, aux2, out2):
        p1, lda1, K1 = _rows2d(a1, "a1")
        p2, lda2, K2 = _rows2d(a2, "a2", allow_none=True)
        M = a1.shape[0]
        pw, ldw, wc = _rows2d(W, "W")
        K = K1 + K2
        N = W.shape[0] if transposed else wc
        if (wc if transposed else W.shape[0]) != K:
            raise ValueError(f"W {tuple(W.shape)} does not match K={K} (transposed={transposed})")
        pc, ldc, nc = _rows2d(out, "out")
        if out.shape[0] != M or nc != N:
            raise ValueError(f"out {tuple(out.shape)} must be [{M},{N}]")
        px1, ld1, _ = _rows2d(aux1, "aux1", allow_none=True)
        if aux1 is not None and tuple(aux1.shape) != (M, N):
            raise ValueError(f"aux1 {tuple(aux1.shape)} must be [{M},{N}]")
        if ws6.numel() < dense6_workspace(K, N, M):
            raise ValueError("ws6 too small (rm_dense6_workspace)")
        dw, dw0, dout = dot if dot is not None else (None, None, None)
        _lib.call("rm_dense_fwd6", p1, lda1, K1, p2, lda2, K2, pw, ldw, int(bool(transposed)), N,
                  _chk(bias, "bias", F32, (N,), allow_none=True), int(epilogue), ACT_IDS[act], px1, ld1, M, pc, ldc,
                  _chk(dw, "dot w", F32, (N,), allow_none=True), _chk(dw0, "dot w0", F32, (1,), allow_none=True),
                  _chk(dout, "dot out", F32, (M,), allow_none=True), _chk(ws6, "ws6", F32), _stream())
        return True
    p1, lda1, K1 = _rows2d(a1, "a1")
    p2, lda2, K2 = _rows2d(a2, "a2", allow_none=True)
    M = a1.shape[0]
    if a2 is not None and a2.shape[0] != M:
        raise ValueError("a1 and a2 differ in rows")
    pw, ldw, wc = _rows2d(W, "W")
    K = K1 + K2
    N = W.shape[0] if transposed else wc
    if (wc if transposed else W.shape[0]) != K:
        raise ValueError(f"W {tuple(W.shape)} does not match K={K} (transposed={transposed})")
    pc, ldc, nc = _rows2d(out, "out")
    if out.shape[0] != M or nc != N:
        raise ValueError(f"out {tuple(out.shape)} must be [{M},{N}]")
    px1, ld1, _ = _rows2d(aux1, "aux1", allow_none=True)
    px2, ld2, _ = _rows2d(aux2, "aux2", allow_none=True)
    pc2, ldc2, _ = _rows2d(out2, "out2", allow_none=True)
    for t, nm in ((aux1, "aux1"), (aux2, "aux2"), (out2, "out2")):
        if t is not None and tuple(t.shape) != (M, N):
            raise ValueError(f"{nm} {tuple(t.shape)} must be [{M},{N}]")
    if filter_ws.numel() < dense_filter_workspace(K, N):
        raise ValueError("filter_ws too small (rm_dense_filter_workspace)")
    _lib.call("rm_dense_fwd", p1, lda1, K1, p2, lda2, K2, pw, ldw, int(bool(transposed)), N,
              _chk(bias, "bias", F32, (N,), allow_none=True), int(epilogue), ACT_IDS[act], px1, ld1, px2, ld2,
              M, pc, ldc, pc2, ldc2, _chk(filter_ws, "filter_ws", F32), _stream())


def dense_wgrad6_workspace(K, N, M):
    """Floats of workspace for the bf16x6 form of dense_wgrad (rm_dense_wgrad6_workspace)."""
    return int(_lib.lib().rm_dense_wgrad6_workspace(int(K), int(N), int(M)))


def dense_wgrad(a1, a2, G, dW, ws, accumulate=False, db=None, ws6=None, G2=None, dW2=None):
    """dW[K,N] (+)= [a1 | a2].T @ G (rm_dense_wgrad); db [N] = G.sum(0) when given.  ws6 (dense_wgrad6_workspace
    floats): on the bf16 matrix pipe with split operands (rm_dense_wgrad6); there G2 [M,N2] / dW2 [K,N2] add a second
    piece of gradient columns to the same pass (ws6 sized for N + N2)."""
    p1, lda1, K1 = _rows2d(a1, "a1")
    p2, lda2, K2 = _rows2d(a2, "a2", allow_none=True)
    pg, ldg, N = _rows2d(G, "G")
    M = a1.shape[0]
    if G.shape[0] != M or (a2 is not None and a2.shape[0] != M):
        raise ValueError("a1 / a2 / G differ in rows")
    pd, lddw, nd = _rows2d(dW, "dW")
    if dW.shape[0] != K1 + K2 or nd != N:
        raise ValueError(f"dW {tuple(dW.shape)} must be [{K1 + K2},{N}]")
    if G2 is not None and ws6 is None:
        raise ValueError("dense_wgrad: G2 needs the ws6 path")
    if ws6 is not None:
        pg2, ldg2, N2 = _rows2d(G2, "G2", allow_none=True)
        pd2, lddw2, nd2 = _rows2d(dW2, "dW2", allow_none=True)
        if G2 is not None and (G2.shape[0] != M or dW2 is None or dW2.shape[0] != K1 + K2 or nd2 != N2):
            raise ValueError("dense_wgrad: G2 / dW2 shape mismatch")
        _lib.call("rm_dense_wgrad6", p1, lda1, K1, p2, lda2, K2, pg, ldg, N, pg2, ldg2, N2, M, pd, lddw, pd2, lddw2,
                  int(bool(accumulate)), _chk(db, "db", F32, (N,), allow_none=True), _chk(ws6, "ws6", F32),
                  ws6.numel(), _stream())
        return
    _lib.call("rm_dense_wgrad", p1, lda1, K1, p2, lda2, K2, pg, ldg, N, M, pd, lddw, int(bool(accumulate)),
              _chk(db, "db", F32, (N,), allow_none=True), _chk(ws, "ws", F32), ws.numel(), _stream())


# ------------------------------------------------------------------ evaluation metrics (csrc/metrics.hip)
METRIC_BAD_LABEL, METRIC_BAD_SCORE, METRIC_ONE_CLASS, METRIC_PROB_RANGE = 1, 2, 4, 8
FLT_EPSILON = 1.1920928955078125e-07


def metric_workspace(n):
    """Bytes of the workspace rm_roc_auc / rm_log_loss need for n elements (0 outside 1 <= n < 2^31)."""
    return int(_lib.lib().rm_metric_workspace(int(n)))


def _metric_args(x, y, workspace, out, name):
    n = x.shape[0] if x.dim() == 1 else -1
    xp = _chk(x, name, F32, (n,))
    yp = _chk(y, "labels", I64, (n,))
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"{name}: need 1 <= n < 2^31 elements, got {n}")
    need = metric_workspace(n)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"metric workspace too small: {need} bytes needed")
    wp = _chk(workspace, "workspace", workspace.dtype)
    if out is None:
        out = torch.empty(4, dtype=I64, device=x.device)
    op = _chk(out, "out", I64, (4,))
    if wp % 16 or op % 16:
        raise ValueError("metric workspace / out must be 16-byte aligned")
    return n, xp, yp, wp, out, op


def roc_auc(scores, labels, workspace=None, out=None):
    """Exact binary ROC AUC (rm_roc_auc): scores fp32 [n], labels int64 [n] on the GPU.  Returns the device
    record `out` (int64 [4]: value as float64 bits, P, N, flags); read it with read_metric."""
    n, xp, yp, wp, out, op = _metric_args(scores, labels, workspace, out, "scores")
    _lib.call("rm_roc_auc", xp, yp, n, wp, op, _stream())
    return out


def log_loss(pred, labels, eps=FLT_EPSILON, workspace=None, out=None):
    """Binary log loss (rm_log_loss), clipped in fp32 at eps: pred fp32 [n], labels int64 [n] on the GPU.
    Returns the device record `out` as roc_auc does."""
    n, xp, yp, wp, out, op = _metric_args(pred, labels, workspace, out, "pred")
    _lib.call("rm_log_loss", xp, yp, n, float(eps), wp, op, _stream())
    return out


def read_metric(out):
    """(value, P, N, flags) of a metric record: one device-to-host copy."""
    r = out.cpu().numpy()
    return float(r[:1].view("float64")[0]), int(r[1]), int(r[2]), int(r[3])


# ------------------------------------------------------------------------- grouped AUC (csrc/gauc.hip)
METRIC_BAD_GROUP = 16


def group_auc_workspace(n):
    """Bytes of the workspace rm_group_auc needs for n elements (0 outside 1 <= n < 2^31)."""
    return int(_lib.lib().rm_group_auc_workspace(int(n)))


def group_auc(scores, labels, groups, weight_kind=0, workspace=None, out=None, per_group=None):
    """Grouped AUC (rm_group_auc): scores fp32 [n], labels int64 [n], groups int64 [n] on the GPU; weight_kind 0
    weighs a group by its examples, 1 by its positives.  per_group: None, or four int64 [n] tensors (ids, n, pos,
    two_u - the last holds uint64 bits) whose first `groups` entries are written in ascending id order.  Returns
    the device record `out` (int64 [6]: value as float64 bits, groups, scored groups, weight sum, P, flags); read
    it with read_group_auc."""
    n = scores.shape[0] if scores.dim() == 1 else -1
    xp = _chk(scores, "scores", F32, (n,))
    yp = _chk(labels, "labels", I64, (n,))
    gp = _chk(groups, "groups", I64, (n,))
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"scores: need 1 <= n < 2^31 elements, got {n}")
    if weight_kind not in (0, 1):
        raise ValueError(f"weight_kind must be 0 (impressions) or 1 (clicks), got {weight_kind!r}")
    need = group_auc_workspace(n)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=scores.device)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"group_auc workspace too small: {need} bytes needed")
    wp = _chk(workspace, "workspace", workspace.dtype)
    if out is None:
        out = torch.empty(6, dtype=I64, device=scores.device)
    op = _chk(out, "out", I64, (6,))
    if wp % 16 or op % 16:
        raise ValueError("group_auc workspace / out must be 16-byte aligned")
    pg = [None] * 4
    if per_group is not None:
        if len(per_group) != 4:
            raise ValueError("per_group: four int64 [n] tensors (ids, n, pos, two_u)")
        pg = [_chk(t, name, I64, (n,)) for t, name in zip(per_group, ("group_ids", "group_n", "group_pos",
                                                                      "group_2u"))]
    _lib.call("rm_group_auc", xp, yp, gp, n, int(weight_kind), wp, *pg, op, _stream())
    return out


def read_group_auc(out):
    """(value, groups, scored_groups, weight, P, flags) of a grouped-AUC record: one device-to-host copy."""
    r = out.cpu().numpy()
    return (float(r[:1].view("float64")[0]),) + tuple(int(v) for v in r[1:6])


# ------------------------------------------------- grouped top-k ranking metrics (csrc/rankmetrics.hip)
GAIN_MAX_K, GAIN_MAX_CUTOFFS = 1024, 8  # RM_GAIN_MAX_K / RM_GAIN_MAX_CUTOFFS
GAIN_NORMS = {"ideal": 0, "positives": 1, "k": 2}
GAIN_SCORED = {"both_classes": 0, "has_positive": 1}
GAIN_WEIGHTS = {"groups": 0, "impressions": 1, "clicks": 2}
_GAIN_RECORD = GAIN_MAX_CUTOFFS + 5
_discounts = {}


def gain_discounts(device, kind, kmax):
    """The float64 device table of per-rank discounts: kind "log2" is 1 / log2(r + 2) (DCG), "none" is 1 (counts);
    kmax entries.  Built once per (device, kind, kmax)."""
    import numpy as np

    device = torch.device(device)
    key = (device, kind, int(kmax))
    if key not in _discounts:
        if kind == "log2":
            table = 1 / np.log2(np.arange(2, kmax + 2, dtype=np.float64))
        elif kind == "none":
            table = np.ones(kmax, dtype=np.float64)
        else:
            raise ValueError(f"discount kind must be 'log2' or 'none', got {kind!r}")
        _discounts[key] = torch.from_numpy(table).to(device)
    return _discounts[key]


def group_gain_workspace(n):
    """Bytes of the workspace rm_group_gain needs for n elements (0 outside 1 <= n < 2^31)."""
    return int(_lib.lib().rm_group_gain_workspace(int(n)))


def group_gain(scores, labels, groups, disc, cutoffs, norm=0, scored_rule=0, weight_kind=0, workspace=None, out=None,
               per_group=None):
    """Grouped top-k gain (rm_group_gain): scores fp32 [n], labels int64 [n], groups int64 [n] or None (one group)
    on the GPU; disc float64 [>= cutoffs[-1]] on the GPU; cutoffs: 1..8 strictly ascending ints in 1..1024; norm /
    scored_rule / weight_kind: values of GAIN_NORMS / GAIN_SCORED / GAIN_WEIGHTS.  per_group: None, or (ids, n, pos)
    int64 [n] and values float64 [n, len(cutoffs)], whose first `groups` rows are written in ascending id order.
    Returns the device record `out` (int64 [13]: eight values as float64 bits, groups, scored groups, weight sum, P,
    flags); read it with read_group_gain."""
    n = scores.shape[0] if scores.dim() == 1 else -1
    xp = _chk(scores, "scores", F32, (n,))
    yp = _chk(labels, "labels", I64, (n,))
    gp = _chk(groups, "groups", I64, (n,), allow_none=True)
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"scores: need 1 <= n < 2^31 elements, got {n}")
    ks = [int(k) for k in cutoffs]
    if not 1 <= len(ks) <= GAIN_MAX_CUTOFFS:
        raise ValueError(f"cutoffs: 1 to {GAIN_MAX_CUTOFFS} values, got {len(ks)}")
    if any(not 1 <= k <= GAIN_MAX_K for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"cutoffs must be strictly ascending in [1, {GAIN_MAX_K}], got {ks}")
    for name, v, table in (("norm", norm, GAIN_NORMS), ("scored_rule", scored_rule, GAIN_SCORED),
                           ("weight_kind", weight_kind, GAIN_WEIGHTS)):
        if v not in table.values():
            raise ValueError(f"{name} must be one of {table}, got {v!r}")
    dp = _chk(disc, "disc", torch.float64)
    if disc.dim() != 1 or disc.shape[0] < ks[-1]:
        raise ValueError(f"disc: need a 1-D table of at least {ks[-1]} entries, got shape {tuple(disc.shape)}")
    need = group_gain_workspace(n)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=scores.device)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"group_gain workspace too small: {need} bytes needed")
    wp = _chk(workspace, "workspace", workspace.dtype)
    if out is None:
        out = torch.empty(_GAIN_RECORD, dtype=I64, device=scores.device)
    op = _chk(out, "out", I64, (_GAIN_RECORD,))
    if wp % 16 or op % 16:
        raise ValueError("group_gain workspace / out must be 16-byte aligned")
    pg = [None] * 4
    if per_group is not None:
        if len(per_group) != 4:
            raise ValueError("per_group: int64 [n] tensors (ids, n, pos) and float64 [n, len(cutoffs)] values")
        pg = [_chk(t, name, I64, (n,)) for t, name in zip(per_group[:3], ("group_ids", "group_n", "group_pos"))]
        pg.append(_chk(per_group[3], "group_value", torch.float64, (n, len(ks))))
    _lib.call("rm_group_gain", xp, yp, gp, n, dp, (ctypes.c_int * len(ks))(*ks), len(ks), int(norm),
              int(scored_rule), int(weight_kind), wp, *pg, op, _stream())
    return out


def read_group_gain(out, n_cutoffs=GAIN_MAX_CUTOFFS):
    """(values, groups, scored_groups, weight, P, flags) of a grouped-gain record, values a tuple of the first
    n_cutoffs floats: one device-to-host copy."""
    r = out.cpu().numpy()
    values = tuple(float(v) for v in r[:GAIN_MAX_CUTOFFS].view("float64")[:n_cutoffs])
    return (values,) + tuple(int(v) for v in r[GAIN_MAX_CUTOFFS:_GAIN_RECORD])


# ---- multi-task learning: the gate mixtures of MMoE and of PLE / CGC, the loss head for several labels, plain and
# ---- with ESMM's entire-space pair (csrc/multitask.hip) ---------------------------------------------------------
MMOE_TILE = {"tile": 0, "cap": 1}  # RM_MMOE_TILE / RM_MMOE_CAP
MMOE_LIMITS = "1 <= E <= 16 experts, 1 <= T <= 8 tasks, H a multiple of 4 in 4..512, row strides multiples of 4 floats"
MMOE_H_MIN, MMOE_H_MAX = 4, 512
CGC_TILE = {"tile": 0, "cap": 1}  # RM_CGC_TILE / RM_CGC_CAP
CGC_LIMITS = ("1 <= T <= 8 tasks, 1 <= S <= 4 task experts, 1 <= C <= 8 shared experts, N = T S + C <= 32, H a "
              "multiple of 4 in 4..512, shared_gate 0 or 1, row strides multiples of 4 floats")
CGC_H_MIN, CGC_H_MAX = 4, 512
TASK_TYPES = {"classification": 0, "regression": 1}


def mmoe_mix_supported(E, T, H):
    """rm_mmoe_mix_supported: 1 <= E <= 16, 1 <= T <= 8, H a multiple of 4 in 4..512."""
    return bool(_lib.lib().rm_mmoe_mix_supported(int(E), int(T), int(H)))


def cgc_mix_supported(T, S, C, H, shared_gate):
    """rm_cgc_mix_supported: 1 <= T <= 8, 1 <= S <= 4, 1 <= C <= 8, T S + C <= 32, H a multiple of 4 in 4..512."""
    return bool(_lib.lib().rm_cgc_mix_supported(int(T), int(S), int(C), int(H), int(shared_gate)))


def mmoe_mix_tile(E, T, H, which="tile", backward=False):
    """rm_mmoe_mix_tile: "tile" = the examples a block of the mixture kernels owns per tile, "cap" = the cap of their
    grids (a block walks the batch again from B > cap * tile on)."""
    n = int(_lib.lib().rm_mmoe_mix_tile(int(E), int(T), int(H), int(bool(backward)), MMOE_TILE[which]))
    if n < 0:
        raise ValueError(f"mmoe_mix: E={E}, T={T}, H={H} unsupported ({MMOE_LIMITS})")
    return n


def cgc_mix_tile(T, S, C, H, shared_gate, which="tile", backward=False):
    """rm_cgc_mix_tile: "tile" = the examples a block of the mixture kernels owns per tile, "cap" = the cap of their
    grids (a block walks the batch again from B > cap * tile on)."""
    n = int(_lib.lib().rm_cgc_mix_tile(int(T), int(S), int(C), int(H), int(shared_gate), int(bool(backward)),
                                       CGC_TILE[which]))
    if n < 0:
        raise ValueError(f"cgc_mix: T={T}, S={S}, C={C}, H={H}, shared_gate={shared_gate} unsupported ({CGC_LIMITS})")
    return n


def cgc_widths(T, S, C, shared_gate):
    """(N experts, gate-logit columns T (S + C) + shared_gate N, gates T + shared_gate) of one extraction level."""
    T, S, C, sg = int(T), int(S), int(C), int(bool(shared_gate))
    N = T * S + C
    return N, T * (S + C) + sg * N, T + sg


def _mmoe_dims(Z, A, E, T):
    E, T = int(E), int(T)
    if Z.dim() != 2 or A.dim() != 2 or E < 1 or T < 1 or Z.shape[1] % E or A.shape[1] != T * E:
        raise ValueError(f"mmoe_mix: Z {tuple(Z.shape)} must be [B, E H] and A {tuple(A.shape)} [B, T E] "
                         f"(E={E}, T={T})")
    return int(Z.shape[0]), E, T, int(Z.shape[1]) // E


def _cgc_dims(Z, A, T, S, C, shared_gate):
    T, S, C, sg = int(T), int(S), int(C), int(shared_gate)
    if sg not in (0, 1) or min(T, S, C) < 1:
        raise ValueError(f"cgc_mix: T={T}, S={S}, C={C}, shared_gate={shared_gate} unsupported ({CGC_LIMITS})")
    N, AW, G = cgc_widths(T, S, C, sg)
    if Z.dim() != 2 or A.dim() != 2 or Z.shape[1] % N or A.shape[1] != AW:
        raise ValueError(f"cgc_mix: Z {tuple(Z.shape)} must be [B, N H] and A {tuple(A.shape)} [B, T (S + C) + "
                         f"shared_gate N] (T={T}, S={S}, C={C}, shared_gate={sg}: N={N}, {AW} gate logits)")
    return int(Z.shape[0]), T, S, C, sg, N, AW, G, int(Z.shape[1]) // N


def mmoe_mix_fwd(Z, A, E, T, M, P=None):
    """rm_mmoe_mix_fwd: Z [B, E H] expert outputs, A [B, T E] gate logits -> M [B, T H], M_t = softmax(A_t) Z, and -
    when given - P [B, T E], the gate weights.  Every operand may be a column range of a wider buffer (16-byte aligned,
    row stride a multiple of 4 floats); only the own columns are written.  The limits are checked by the library."""
    B, E, T, H = _mmoe_dims(Z, A, E, T)
    pz, ldz = _strided_rows(Z, "Z", B, E * H, True)
    pa, lda = _strided_rows(A, "A", B, T * E, True)
    pm, ldm = _strided_rows(M, "M", B, T * H, True)
    pp, ldp = (None, 0) if P is None else _strided_rows(P, "P", B, T * E, True)
    _lib.call("rm_mmoe_mix_fwd", pz, ldz, pa, lda, B, E, T, H, pm, ldm, pp, ldp, _stream())


def mmoe_mix_bwd(Z, A, E, T, dM, dZ, dA):
    """rm_mmoe_mix_bwd: dM [B, T H] = dLoss/dM -> dZ [B, E H] and dA [B, T E] (column ranges as in mmoe_mix_fwd; only
    their own columns are written).  The gate weights are recomputed.  No workspace; deterministic."""
    B, E, T, H = _mmoe_dims(Z, A, E, T)
    pz, ldz = _strided_rows(Z, "Z", B, E * H, True)
    pa, lda = _strided_rows(A, "A", B, T * E, True)
    pdm, lddm = _strided_rows(dM, "dM", B, T * H, True)
    pdz, lddz = _strided_rows(dZ, "dZ", B, E * H, True)
    pda, ldda = _strided_rows(dA, "dA", B, T * E, True)
    _lib.call("rm_mmoe_mix_bwd", pz, ldz, pa, lda, pdm, lddm, B, E, T, H, pdz, lddz, pda, ldda, _stream())


def cgc_mix_fwd(Z, A, T, S, C, shared_gate, M, P=None):
    """rm_cgc_mix_fwd: Z [B, N H] the expert outputs of a level (S own experts per task, then C shared ones), A the
    gate logits [B, T (S + C) + shared_gate N] -> M [B, (T + shared_gate) H], M_g = softmax(A_g) over the experts gate
    g sees, and - when given - P (A's layout), the gate weights.  Every operand may be a column range of a wider buffer
    (16-byte aligned, row stride a multiple of 4 floats); only the own columns are written.  The limits are checked by
    the library."""
    B, T, S, C, sg, N, AW, G, H = _cgc_dims(Z, A, T, S, C, shared_gate)
    pz, ldz = _strided_rows(Z, "Z", B, N * H, True)
    pa, lda = _strided_rows(A, "A", B, AW, True)
    pm, ldm = _strided_rows(M, "M", B, G * H, True)
    pp, ldp = (None, 0) if P is None else _strided_rows(P, "P", B, AW, True)
    _lib.call("rm_cgc_mix_fwd", pz, ldz, pa, lda, B, T, S, C, H, sg, pm, ldm, pp, ldp, _stream())


def cgc_mix_bwd(Z, A, T, S, C, shared_gate, dM, dZ, dA):
    """rm_cgc_mix_bwd: dM [B, (T + shared_gate) H] = dLoss/dM -> dZ [B, N H] and dA (A's layout), both written once
    (column ranges as in cgc_mix_fwd).  The gate weights are recomputed.  No workspace; deterministic."""
    B, T, S, C, sg, N, AW, G, H = _cgc_dims(Z, A, T, S, C, shared_gate)
    pz, ldz = _strided_rows(Z, "Z", B, N * H, True)
    pa, lda = _strided_rows(A, "A", B, AW, True)
    pdm, lddm = _strided_rows(dM, "dM", B, G * H, True)
    pdz, lddz = _strided_rows(dZ, "dZ", B, N * H, True)
    pda, ldda = _strided_rows(dA, "dA", B, AW, True)
    _lib.call("rm_cgc_mix_bwd", pz, ldz, pa, lda, pdm, lddm, B, T, S, C, H, sg, pdz, lddz, pda, ldda, _stream())


def _loss_workspace(op, B, T):
    n = int(getattr(_lib.lib(), f"rm_{op}_workspace")(int(B), int(T)))
    if n < 0:
        raise ValueError(f"{op}: B={B}, T={T} unsupported (B >= 1, 1 <= T <= 8 tasks)")
    return n


def multitask_loss_workspace(B, T):
    """Floats of workspace for multitask_loss (rm_multitask_loss_workspace)."""
    return _loss_workspace("multitask_loss", B, T)


def multitask_loss_es_workspace(B, T):
    """Floats of workspace for multitask_loss_es (rm_multitask_loss_es_workspace)."""
    return _loss_workspace("multitask_loss_es", B, T)


def _multitask_loss(op, logit, task_types, pred, es, Y, task_weights, grad_scale, dlogit, n_t, loss_t, loss,
                    workspace):
    """The loss head through entry point rm_{op}; es: () for rm_multitask_loss, the pair (c, v) for the other."""
    if logit.dim() != 2:
        raise ValueError(f"logit: expected [T, B], got {tuple(logit.shape)}")
    T, B = int(logit.shape[0]), int(logit.shape[1])
    if len(task_types) != T:
        raise ValueError(f"{op}: {len(task_types)} task types for {T} rows of logits")
    pair = tuple(int(i) for i in es)
    if pair and pair != (-1, -1):
        c, v = pair
        if not (0 <= c < T and 0 <= v < T and c != v and task_types[c] == task_types[v] == "classification"):
            raise ValueError(f"{op}: es={tuple(es)!r} must be two distinct classification tasks below T={T}, "
                             "or (-1, -1)")
    types = _int_array([TASK_TYPES[t] for t in task_types])
    train = any(t is not None for t in (dlogit, n_t, loss_t, loss))
    weights = None
    if train:
        if Y is None or workspace is None:
            raise ValueError(f"{op}: the loss and its gradient need labels Y and a workspace")
        w = [1.0] * T if task_weights is None else [float(x) for x in task_weights]
        if len(w) != T:
            raise ValueError(f"{op}: {len(w)} task weights for {T} tasks")
        weights = (ctypes.c_float * T)(*w)
        _need_workspace(op, workspace, _loss_workspace(op, B, T))
    _lib.call(f"rm_{op}", _chk(logit, "logit", F32), _chk(Y, "Y", F32, (B, T), allow_none=not train), types, weights,
              float(grad_scale), B, T, *pair, _chk(pred, "pred", F32, (T, B)),
              _chk(dlogit, "dlogit", F32, (T, B), allow_none=True), _chk(n_t, "n_t", I64, (T,), allow_none=True),
              _chk(loss_t, "loss_t", F32, (T,), allow_none=True), _chk(loss, "loss", F32, (1,), allow_none=True),
              _chk(workspace, "workspace", F32, allow_none=True), _stream())


def multitask_loss(logit, task_types, pred, *, Y=None, task_weights=None, grad_scale=1.0, dlogit=None, n_t=None,
                   loss_t=None, loss=None, workspace=None):
    """rm_multitask_loss: logit [T, B], task_types T names ("classification" / "regression") -> pred [T, B]; with
    labels Y [B, T] (float32, NaN = unobserved) and task_weights (T floats) also dlogit [T, B] = w_t dl/dlogit / n_t *
    grad_scale (0 where unobserved), n_t [T] int64, loss_t [T] and loss [1] = sum_t w_t loss_t."""
    _multitask_loss("multitask_loss", logit, task_types, pred, (), Y, task_weights, grad_scale, dlogit, n_t, loss_t,
                    loss, workspace)


def multitask_loss_es(logit, task_types, pred, *, es=(-1, -1), Y=None, task_weights=None, grad_scale=1.0, dlogit=None,
                      n_t=None, loss_t=None, loss=None, workspace=None):
    """rm_multitask_loss_es: multitask_loss with the entire-space pair es = (c, v), two distinct classification tasks:
    task v is trained through pred_c pred_v against z (0 where Y[:, c] == 0, Y[:, v] where Y[:, c] == 1, unobserved
    otherwise) over all those rows, and its gradient reaches both logits.  es = (-1, -1): multitask_loss's bits."""
    _multitask_loss("multitask_loss_es", logit, task_types, pred, es, Y, task_weights, grad_scale, dlogit, n_t, loss_t,
                    loss, workspace)


# ---- two-tower retrieval: the in-batch softmax loss and the row normalisation (csrc/inbatch.hip) -------------------
IBS_TILE = {"rows": 0, "cols": 1, "max_splits": 2}  # RM_IBS_ROWS / RM_IBS_COLS / RM_IBS_MAX_SPLITS
IBS_LIMITS = "H a multiple of 4 in 4..256, row strides multiples of 4 floats, col_splits 0..8"
IBS_H_MIN, IBS_H_MAX = 4, 256


def inbatch_softmax_supported(H):
    """rm_inbatch_softmax_supported: H a multiple of 4 in 4..256."""
    return bool(_lib.lib().rm_inbatch_softmax_supported(int(H)))


def inbatch_softmax_tile(H, which="rows"):
    """rm_inbatch_softmax_tile: "rows" = the rows a block of the score kernels owns, "cols" = the rows of a streamed
    tile, "max_splits" = the largest col_splits."""
    n = int(_lib.lib().rm_inbatch_softmax_tile(int(H), IBS_TILE[which]))
    if n < 0:
        raise ValueError(f"inbatch_softmax: H={H} unsupported ({IBS_LIMITS})")
    return n


def inbatch_softmax_workspace(B, H):
    """Floats of workspace for inbatch_softmax_fwd / _bwd (rm_inbatch_softmax_workspace; any col_splits)."""
    n = int(_lib.lib().rm_inbatch_softmax_workspace(int(B), int(H)))
    if n < 0:
        raise ValueError(f"inbatch_softmax: B={B}, H={H} unsupported ({IBS_LIMITS})")
    return n


def _ibs_operands(U, V, item_id, logq, w, workspace, fn):
    if U.dim() != 2 or V.dim() != 2 or tuple(U.shape) != tuple(V.shape):
        raise ValueError(f"{fn}: U {tuple(U.shape)} and V {tuple(V.shape)} must both be [B, H]")
    B, H = int(U.shape[0]), int(U.shape[1])
    pu, ldu = _strided_rows(U, "U", B, H, True)
    pv, ldv = _strided_rows(V, "V", B, H, True)
    _need_workspace(fn, workspace, inbatch_softmax_workspace(B, H))
    return (B, H, pu, ldu, pv, ldv, _chk(item_id, "item_id", I64, (B,), allow_none=True),
            _chk(logq, "logq", F32, (B,), allow_none=True), _chk(w, "w", F32, (B,), allow_none=True))


def inbatch_softmax_fwd(U, V, scale, lse, row_loss, loss, workspace, *, item_id=None, logq=None, w=None, rank=None,
                        col_splits=0):
    """rm_inbatch_softmax_fwd: U, V [B, H] (column ranges of wider buffers work), S = scale U V^T - logq with the
    accidental hits of item_id masked out -> lse [B], row_loss [B] = lse_i - S_ii, rank [B] int32 (optional: the
    number of allowed j != i with S_ij > S_ii) and loss [1] = sum_i w_i row_loss_i / sum_i w_i.  col_splits: 0 = the
    library's choice.  The limits are checked by the library."""
    B, H, pu, ldu, pv, ldv, pid, pq, pw = _ibs_operands(U, V, item_id, logq, w, workspace, "inbatch_softmax_fwd")
    _lib.call("rm_inbatch_softmax_fwd", pu, ldu, pv, ldv, pid, pq, pw, float(scale), B, H, int(col_splits),
              _chk(lse, "lse", F32, (B,)), _chk(row_loss, "row_loss", F32, (B,)),
              _chk(rank, "rank", torch.int32, (B,), allow_none=True), _chk(loss, "loss", F32, (1,)),
              _chk(workspace, "workspace", F32), _stream())


def inbatch_softmax_bwd(U, V, scale, lse, dU, dV, workspace, *, item_id=None, logq=None, w=None, grad_scale=1.0,
                        col_splits=0):
    """rm_inbatch_softmax_bwd: the gradient of grad_scale * loss with the scores recomputed from U, V and the
    forward's lse -> dU, dV [B, H] (column ranges work; only their own columns are written).  Deterministic."""
    B, H, pu, ldu, pv, ldv, pid, pq, pw = _ibs_operands(U, V, item_id, logq, w, workspace, "inbatch_softmax_bwd")
    pdu, lddu = _strided_rows(dU, "dU", B, H, True)
    pdv, lddv = _strided_rows(dV, "dV", B, H, True)
    _lib.call("rm_inbatch_softmax_bwd", pu, ldu, pv, ldv, pid, pq, pw, float(scale), float(grad_scale), B, H,
              int(col_splits), _chk(lse, "lse", F32, (B,)), pdu, lddu, pdv, lddv, _chk(workspace, "workspace", F32),
              _stream())


def rownorm_fwd(X, Y, inv_norm, eps=1e-12):
    """rm_rownorm_fwd: Y = X / max(|X|_2, eps) row by row, inv_norm [B] = 1 / max(|X|_2, eps); X, Y [B, H] (column
    ranges work)."""
    if X.dim() != 2:
        raise ValueError(f"X: expected [B, H], got {tuple(X.shape)}")
    B, H = int(X.shape[0]), int(X.shape[1])
    px, ldx = _strided_rows(X, "X", B, H, True)
    py, ldy = _strided_rows(Y, "Y", B, H, True)
    _lib.call("rm_rownorm_fwd", px, ldx, B, H, float(eps), py, ldy, _chk(inv_norm, "inv_norm", F32, (B,)), _stream())


def rownorm_bwd(Y, inv_norm, dY, dX):
    """rm_rownorm_bwd: dX = inv_norm (dY - Y <Y, dY>) row by row; dX may be dY itself."""
    if Y.dim() != 2:
        raise ValueError(f"Y: expected [B, H], got {tuple(Y.shape)}")
    B, H = int(Y.shape[0]), int(Y.shape[1])
    py, ldy = _strided_rows(Y, "Y", B, H, True)
    pdy, lddy = _strided_rows(dY, "dY", B, H, True)
    pdx, lddx = _strided_rows(dX, "dX", B, H, True)
    _lib.call("rm_rownorm_bwd", py, ldy, _chk(inv_norm, "inv_norm", F32, (B,)), pdy, lddy, B, H, pdx, lddx, _stream())


# ---- exact top-k retrieval by inner product over an item catalogue (csrc/topk.hip, include/recman_hip_topk.h) -----
TOPK_TILE = {"rows": 0, "cols": 1, "max_splits": 2}  # RM_TOPK_ROWS / RM_TOPK_COLS / RM_TOPK_MAX_SPLITS
TOPK_LIMITS = "H a multiple of 4 in 4..256, k in 1..1024, row strides multiples of 4 floats, item_splits 0..64"


def topk_ip_supported(H, k):
    """rm_topk_ip_supported: H a multiple of 4 in 4..256 and k in 1..1024."""
    return bool(_lib.lib().rm_topk_ip_supported(int(H), int(k)))


def topk_ip_tile(H, which="rows"):
    """rm_topk_ip_tile: "rows" = the query rows a block owns, "cols" = the catalogue rows of a streamed tile,
    "max_splits" = the largest item_splits."""
    n = int(_lib.lib().rm_topk_ip_tile(int(H), TOPK_TILE[which]))
    if n < 0:
        raise ValueError(f"topk_ip: H={H} unsupported ({TOPK_LIMITS})")
    return n


def topk_ip_workspace(Nq, N, H, k):
    """Floats of workspace for topk_ip over Nq queries and N catalogue rows (rm_topk_ip_workspace; any item_splits).
    Linear in Nq: a caller with many queries bounds it by processing them in groups."""
    n = int(_lib.lib().rm_topk_ip_workspace(int(Nq), int(N), int(H), int(k)))
    if n < 0:
        raise ValueError(f"topk_ip: Nq={Nq}, N={N}, H={H}, k={k} unsupported ({TOPK_LIMITS})")
    return n


def _sorted_exclusions(exclude, Nq):
    """(offsets [Nq + 1], rows [nnz]) int64 device tensors -> the same CSR with every query's rows ascending, or
    (None, None) when it holds no row."""
    if exclude is None:
        return None, None
    offsets, rows = exclude
    _chk(offsets, "exclude offsets", I64, (Nq + 1,))
    _chk(rows, "exclude rows", I64)
    if rows.dim() != 1 or rows.numel() == 0:
        if rows.dim() != 1:
            raise ValueError(f"exclude rows: expected a 1-D tensor, got {tuple(rows.shape)}")
        return None, None
    counts = offsets[1:] - offsets[:-1]
    if bool((counts < 0).any()) or int(offsets[0]) != 0 or int(offsets[-1]) != rows.numel():
        raise ValueError("exclude: offsets must rise from 0 to the number of rows")
    seg = torch.repeat_interleave(torch.arange(Nq, device=rows.device), counts)
    by_row = torch.sort(rows, stable=True).indices
    by_seg = torch.sort(seg[by_row], stable=True).indices
    return offsets, rows[by_row][by_seg].contiguous()


def topk_ip(Q, C, k, scale, out_rows, out_scores, workspace, *, exclude=None, item_splits=0):
    """rm_topk_ip: per query row i of Q [Nq, H] the best min(k, available) rows j of the catalogue C [N, H] by
    s_ij = fl(scale <Q_i, C_j>) (fp32, the same value for a pair wherever it is computed), sorted by score descending,
    then row ascending, NaN last -> out_rows int64 / out_scores float32 [Nq, >= k] with one row stride (columns past k
    untouched; slots past the available rows hold -1 / -inf).  Q and C may be column ranges of wider buffers.
    exclude: None or (offsets [Nq + 1], rows) int64 device tensors, the catalogue rows query i must not get back
    (sorted here; rows outside [0, N) are ignored, duplicates allowed).  item_splits: 0 = the library's choice; the
    result is the same bits for every split count.  The limits are checked by the library."""
    if Q.dim() != 2 or C.dim() != 2 or Q.shape[1] != C.shape[1]:
        raise ValueError(f"topk_ip: Q {tuple(Q.shape)} and C {tuple(C.shape)} must be [Nq, H] and [N, H]")
    Nq, N, H = int(Q.shape[0]), int(C.shape[0]), int(Q.shape[1])
    pq, ldq = _strided_rows(Q, "Q", Nq, H, True)
    pc, ldc = _strided_rows(C, "C", N, H, True)
    for t, name, dt in ((out_rows, "out_rows", I64), (out_scores, "out_scores", F32)):
        if not t.is_cuda or t.dtype != dt or t.dim() != 2 or t.shape[0] != Nq or t.shape[1] < k or \
                (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"topk_ip: {name} must be a {dt} device tensor [{Nq}, >= {k}] with unit column stride, "
                             f"got {t.dtype} {tuple(t.shape)}")
    ldo = out_rows.stride(0) if Nq > 1 else int(k)
    if Nq > 1 and out_scores.stride(0) != ldo:
        raise ValueError(f"topk_ip: out_rows and out_scores must share one row stride ({ldo} != "
                         f"{out_scores.stride(0)})")
    _need_workspace("topk_ip", workspace, topk_ip_workspace(Nq, N, H, k) if topk_ip_supported(H, k) else 0)
    eo, er = _sorted_exclusions(exclude, Nq)
    _lib.call("rm_topk_ip", pq, ldq, pc, ldc, Nq, N, H, float(scale), int(k),
              None if eo is None else eo.data_ptr(), None if er is None else er.data_ptr(), int(item_splits),
              out_rows.data_ptr(), out_scores.data_ptr(), int(ldo), _chk(workspace, "workspace", F32), _stream())


# ---- grouped ranking objectives next to the pointwise loss (csrc/rank.hip, include/recman_hip_rank.h) -------------
RANK_KINDS = {"pairwise": 0, "listwise": 1}  # RM_RANK_PAIRWISE / RM_RANK_LISTWISE
RANK_NORMS = {"pairs": 0, "group": 1}        # RM_RANK_NORM_PAIRS / RM_RANK_NORM_GROUP
RANK_MAX_B = 1 << 24


def rank_loss_workspace(B):
    """Bytes of the workspace rm_rank_loss needs for B examples (1 <= B <= 2^24)."""
    n = int(_lib.lib().rm_rank_loss_workspace(int(B)))
    if n <= 0:
        raise ValueError(f"rank_loss: B={B} outside [1, 2^24]")
    return n


def rank_loss(logit, y, groups, kind, norm, alpha, dlogit_out, *, grad_scale=1.0, dlogit_in=None, loss_in=None,
              loss_out=None, out=None, workspace=None):
    """rm_rank_loss: the pairwise (RankNet / BPR) or listwise (ListNet softmax) term L over the examples of the batch
    that share a group id (groups int64 [B], or None: one group), combined with the pointwise head's results:
        dlogit_out = grad_scale ((1 - alpha) dlogit_in + alpha dL/dlogit),   loss_out = (1 - alpha) loss_in + alpha L
    (dlogit_in / loss_in None: the ranking term alone; dlogit_out may be dlogit_in, loss_out may be loss_in).  logit
    float32 [B], y int64 [B] in {0, 1}.  out: int64 [7], the device record (read_rank_loss); workspace: uint8 of
    rank_loss_workspace(B) bytes (allocated when None).  Returns `out` (None when none was given)."""
    B = logit.shape[0] if logit.dim() == 1 else -1
    if kind not in RANK_KINDS:
        raise ValueError(f"rank_loss: kind must be one of {sorted(RANK_KINDS)}, got {kind!r}")
    if norm not in RANK_NORMS:
        raise ValueError(f"rank_loss: norm must be one of {sorted(RANK_NORMS)}, got {norm!r}")
    lp = _chk(logit, "logit", F32, (B,))
    need = rank_loss_workspace(B)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=logit.device)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"rank_loss: workspace too small: {need} bytes needed")
    wp = _chk(workspace, "workspace", workspace.dtype)
    op = _chk(out, "out", I64, (7,), allow_none=True)
    if wp % 16 or (op or 0) % 16:
        raise ValueError("rank_loss: workspace / out must be 16-byte aligned")
    _lib.call("rm_rank_loss", lp, _chk(y, "y", I64, (B,)), _chk(groups, "groups", I64, (B,), allow_none=True), B,
              RANK_KINDS[kind], RANK_NORMS[norm], float(alpha), float(grad_scale),
              _chk(dlogit_in, "dlogit_in", F32, (B,), allow_none=True), _chk(dlogit_out, "dlogit_out", F32, (B,)),
              _chk(loss_in, "loss_in", F32, (1,), allow_none=True),
              _chk(loss_out, "loss_out", F32, (1,), allow_none=True), op, wp, _stream())
    return out


def read_rank_loss(out):
    """(value, groups, scored_groups, pairs, pos, weight, flags) of a ranking-loss record: one device-to-host copy."""
    r = out.cpu().numpy()
    return (float(r[:1].view("float64")[0]),) + tuple(int(v) for v in r[1:7])
