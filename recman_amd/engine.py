"""Explicit forward+backward engines for DeepFM / DCN / xDeepFM / AFM on one MI355X.

No autograd and no tracing compiler: each engine owns its parameters (laid out
for the kernels: ONE concatenated embedding table in HBM, per-feature variables
are views of it), a workspace sized once per batch size, and enqueues a fixed
sequence of HIP kernels (recman_amd/ops.py -> librecman_hip.so) on the current
stream - which is meant to make a whole step capturable in a hipGraph, as bench.py's
time_steps captures it.  A capture requires:
  * fwd_bwd and forward to enqueue on the current stream only, with no host read of
    device data, and the engine warmed at that batch size first (the first call at a
    batch size allocates the workspaces);
  * the optimizers' step (recman_amd/optim.py) outside the graph - it takes the step
    count t by value - and the optimizers built before the capture;
  * no call at another batch size between capture and replay (_alloc releases the
    buffers the graph points to).

The MLP ("DNN", layers.py:576-609) runs on hand-written f32-MFMA kernels as well:
csrc/mlp.hip (all layers fused, hidden widths <= 32) or csrc/gemm.hip (one launch per
GEMM with fused epilogues, any width); no library GEMM is left on the path.

Variable names are the reference's (layers.py:96,106,318,324,533,541,548,558,564,
572,663,673,687,693) so state_dict() round-trips with its checkpoints' keys.
"""
import torch

from . import ops

F32, I64 = torch.float32, torch.int64

_ACTS = {"relu": 0.0, "leaky_relu": 0.2}


def act_name(a):
    """Maps the reference's activation argument (a TF callable such as tf.nn.relu,
    DeepFM.py:40, or a name) to a name this package knows."""
    if a is None:
        return "identity"
    if isinstance(a, str):
        name = a
    else:
        name = getattr(a, "__name__", str(a))
    name = name.lower()
    for k in ("leaky_relu", "relu", "identity", "linear"):
        if k in name:
            return "identity" if k == "linear" else k
    raise ValueError(f"unsupported activation {a!r} (relu, leaky_relu, identity)")


class FeatureSpec:
    """Host-side description of the inputs: embedding (sparse) features in
    FeatureDictionary order (inputs.py:13-15) with their feat_size (null slot
    included, inputs.py:166) and the dense feature names."""

    def __init__(self, sparse_names, feat_sizes, dense_names=(), multi_names=(), value_names=(),
                 linear_names=None, seq_query=None, seq_max_len=None):
        self.sparse_names = list(sparse_names)
        self.feat_sizes = [int(v) for v in feat_sizes]
        self.dense_names = list(dense_names)
        # the hyper-parameter linear_features (get_linear_features, utils.py:27-30): the features of
        # the linear term in the order given; None = every feature in the default order (:31-36)
        self.linear_names = list(linear_names) if linear_names else None
        if self.linear_names is not None:
            known = set(self.sparse_names) | set(self.dense_names)
            bad = [n for n in self.linear_names if n not in known]
            if bad or len(set(self.linear_names)) != len(self.linear_names):
                raise ValueError(f"linear_features: unknown or repeated features {bad or self.linear_names}")
        # embedding features that are multi-valued (MultiValCsvFeat): sqrtn-pooled lookup
        self.multi_names = list(multi_names)
        # embedding features that carry a value (SparseValueFeat): value-weighted lookup
        self.value_names = list(value_names)
        if len(self.sparse_names) != len(self.feat_sizes):
            raise ValueError("sparse_names and feat_sizes differ in length")
        # embedding features that are behaviour histories (SequenceFeat): name -> the feature whose table rows
        # they look up and whose row of the example is the attention's query; they own no rows (feat_size 0)
        self.seq_query = dict(seq_query or {})
        self.seq_max_len = {n: int((seq_max_len or {}).get(n, 256)) for n in self.seq_query}
        size = dict(zip(self.sparse_names, self.feat_sizes))
        for n, q in self.seq_query.items():
            if n not in size or size[n] != 0:
                raise ValueError(f"sequence feature {n!r} must be an embedding feature with feat_size 0")
            if q not in size or q in self.seq_query or q in self.multi_names or q in self.value_names:
                raise ValueError(f"sequence feature {n!r}: its query feature {q!r} must be a plain sparse feature")

    @property
    def F(self):
        return len(self.sparse_names)

    @property
    def Dn(self):
        return len(self.dense_names)

    @property
    def rows(self):
        return sum(self.feat_sizes)

    def offsets(self):
        off, out = 0, []
        for v in self.feat_sizes:
            out.append(off)
            off += v
        return out

    def lin_ref_blocks(self):
        """(row offset in the table, size) of each feature's one-hot block in the order the
        reference's linear_w stacks them (utils.py:27-36): sparse feats, value feats, then
        multi-valued."""
        at = dict(zip(self.sparse_names, zip(self.offsets(), self.feat_sizes)))
        special = set(self.multi_names) | set(self.value_names)
        order = ([n for n in self.sparse_names if n not in special]
                 + [n for n in self.sparse_names if n in self.value_names]
                 + [n for n in self.sparse_names if n in self.multi_names])
        return [at[n] for n in order]

    def lin_ref_layout(self):
        """The reference's linear_w as a list of pieces in ITS order: ("s", first table row, size)
        for an embedding feature's one-hot block, ("d", j) for dense column j."""
        if self.linear_names is None:
            return [("s", o, n) for o, n in self.lin_ref_blocks()] + [("d", j) for j in range(self.Dn)]
        at = dict(zip(self.sparse_names, zip(self.offsets(), self.feat_sizes)))
        dj = {n: j for j, n in enumerate(self.dense_names)}
        return [("s",) + at[n] if n in at else ("d", dj[n]) for n in self.linear_names]

    def lin_masks(self):
        """(per-field 0/1 list, per-dense-column 0/1 list): which features the linear term uses;
        (None, None) when it uses all of them."""
        if self.linear_names is None:
            return None, None
        sel = set(self.linear_names)
        return ([1.0 if n in sel else 0.0 for n in self.sparse_names],
                [1.0 if n in sel else 0.0 for n in self.dense_names])

    @property
    def scratch_names(self):
        """Features whose per-example row is computed into scratch rows before the gather."""
        return self.multi_names + self.value_names + self.seq_names

    @property
    def seq_names(self):
        return [n for n in self.sparse_names if n in self.seq_query]


def _declare(params, grads, decl, name, shape, device, init="zeros", l2=None):
    """One dense variable: its zero-filled params / grads pair and, in `decl`, name -> (init, l2).
    init: "zeros", ("glorot", fan_in, fan_out) (the +-2 sigma truncated normal) or ("glorot_uniform", fan_in,
    fan_out) - what init_reference applies; l2: the hyper-parameter key whose coefficient regularises it, or None."""
    params[name] = torch.zeros(shape, dtype=F32, device=device)
    grads[name] = torch.zeros(shape, dtype=F32, device=device)
    decl[name] = (init, l2)


def _declare_layers(params, grads, decl, prefix, dims, device):
    """{prefix}dnn_layer_{i}_weights [dims[i], dims[i+1]] (glorot, deep_l2_reg) and _bias (zeros, no l2)."""
    for i in range(len(dims) - 1):
        _declare(params, grads, decl, f"{prefix}dnn_layer_{i}_weights", (dims[i], dims[i + 1]), device,
                 ("glorot", dims[i], dims[i + 1]), "deep_l2_reg")
        _declare(params, grads, decl, f"{prefix}dnn_layer_{i}_bias", (dims[i + 1],), device)


def _dense_workspaces(dims, B, device, dense_gemm, wgrad6_pad=0):
    """(fws, wws, fws6, wws6) for a chain of wide dense layers of widths `dims` at batch B: the filter and
    weight-gradient workspaces of csrc/gemm.hip and - with dense_gemm = "bf16x6", the bf16 matrix pipe with split
    fp32 operands (rm_dense_fwd6, csrc/gemm6.hip) - those of the split-operand kernels, else None ("f32": the f32
    MFMA kernel).  wgrad6_pad: further gradient columns the first layer's weight-gradient pass may carry."""
    n = len(dims) - 1
    fw = max(ops.dense_filter_workspace(max(dims[i], dims[i + 1]), max(dims[i], dims[i + 1])) for i in range(n))
    ww = max(ops.dense_wgrad_workspace(dims[i], dims[i + 1], B) for i in range(n))
    fws = torch.empty(fw, dtype=F32, device=device)
    wws = torch.empty(max(ww, 1), dtype=F32, device=device)
    fws6 = wws6 = None
    if dense_gemm == "bf16x6":
        kmax = max(dims)
        fws6 = torch.empty(ops.dense6_workspace(kmax, kmax, B), dtype=F32, device=device)
        wws6 = torch.empty(max(ops.dense_wgrad6_workspace(dims[i], dims[i + 1] + wgrad6_pad, B) for i in range(n)),
                           dtype=F32, device=device)
    return fws, wws, fws6, wws6


class MLP:
    """DNN.__call__ (layers.py:576-609) with an explicit backward.  x = [xe | xd] is
    never concatenated: layer 0 is two GEMMs accumulating into one output.
    self.decl: its variables' name -> (init rule, l2 key), for the engine that adopts it."""

    def __init__(self, params, grads, FD, Dn, hidden, activation, device, prefix="", stream_d_rows=False,
                 dense_gemm="bf16x6"):
        self.FD, self.Dn = FD, Dn
        self.hidden = list(hidden)
        self.act = act_name(activation)
        if self.act not in ("relu", "leaky_relu", "identity"):
            raise ValueError(self.act)
        self.p, self.g, self.prefix = params, grads, prefix
        dims = [FD + Dn] + self.hidden
        self.decl = {}
        _declare_layers(params, grads, self.decl, prefix, dims, device)
        _declare(params, grads, self.decl, f"{prefix}dnn_w", (dims[-1], 1), device, ("glorot", dims[-1], 1),
                 "deep_l2_reg")
        _declare(params, grads, self.decl, f"{prefix}dnn_w0", (1,), device)
        self._B = None
        # the wide path's workspaces (_alloc_dense) and rm_outer_actgrad_sums' (backward): made on first use
        self._ws = self._ones = self._fws = self._wws = self._fws6 = self._wws6 = self._wws_B = self._sums_ws = None
        # hand-written fused f32-MFMA path for skinny MLPs (csrc/mlp.hip); wider ones (DCN's
        # [400,400]) and any MLP under dropout run layer by layer on the wide dense kernels
        # (csrc/gemm.hip: bias / activation / activation-gradient fused, x = [xe | xd] in place)
        self.fused_ok = bool(FD % 4 == 0 and ops.mlp_supported(FD, Dn, self.hidden))
        self.fused = False
        # hp["d_rows_reuse"] = "stream": the row gradients leave the caches (non-temporal stores) - only
        # for a bare forward+backward; the default keeps them cached for the optimizer step that
        # gathers them right after (fit(), and the benchmark: it times what training runs)
        self.stream_d_rows = bool(stream_d_rows)
        # wide layers: "bf16x6" (the split-operand kernels) or "f32" (_dense_workspaces)
        self.dense_gemm = dense_gemm

    def vars(self, d):
        """(Ws, bs, w_out, w0) out of the params or the grads dict."""
        pre, n = self.prefix, len(self.hidden)
        return ([d[f"{pre}dnn_layer_{i}_weights"] for i in range(n)], [d[f"{pre}dnn_layer_{i}_bias"] for i in range(n)],
                d[f"{pre}dnn_w"].view(-1), d[f"{pre}dnn_w0"])

    def _alloc(self, B, device):
        if self._B == B:
            return
        self._B = B
        if self.fused_ok:
            self.hb = [torch.zeros(B, 32, dtype=F32, device=device) for _ in self.hidden]
            self.dhb = [torch.zeros(B, 32, dtype=F32, device=device) for _ in self.hidden]
            self.fws = torch.empty(ops.mlp_bwd_workspace(self.FD, self.Dn), dtype=F32, device=device)
            self.ones = torch.ones(B, dtype=F32, device=device)
            self.tmp32 = torch.empty(32, dtype=F32, device=device)
        self.a = [torch.empty(B, h, dtype=F32, device=device) for h in self.hidden]
        self.da = [torch.empty(B, h, dtype=F32, device=device) for h in self.hidden]
        self.out = torch.empty(B, 1, dtype=F32, device=device)

    def _act_(self, h):
        if self.act == "relu":
            torch.relu_(h)
        elif self.act == "leaky_relu":
            torch.nn.functional.leaky_relu_(h, 0.2)
        return h

    def forward(self, xe, xd, keep=None, masks=None, head=None):
        """xe [B,FD], xd [B,Dn] or None -> logit [B] (a view of an internal buffer).
        keep/masks: DNN dropout keep-probabilities and 0/1 masks (layers.py:589,602).
        head: keyword arguments of ops.mlp_tail (minus dh) - when the fused kernel runs, the final
        logit, prediction, loss and dLoss/dlogit are produced in its epilogue together with the dh
        chain (self.head_done tells the caller; otherwise it runs rm_logit_loss as usual)."""
        B = xe.shape[0]
        self._alloc(B, xe.device)
        Ws, bs, w_out, w0 = self.vars(self.p)
        n = len(self.hidden)
        self.keep = keep if keep is not None else [1] * (n + 1)
        self.masks = masks if masks is not None else [None] * (n + 1)
        self.xe, self.xd = xe, xd
        dropping = any(k < 1 and mk is not None for k, mk in zip(self.keep, self.masks))
        self.fused = self.fused_ok and not dropping
        self.head_done, self.tail = False, None
        if self.fused:
            if head is not None:
                self.tail = ops.mlp_tail(B, dh=self.dhb, **head)
                self.head_done = True
            ops.mlp_fwd(xe, xd if self.Dn else None, Ws, bs, w_out, w0, self.act, self.hb, self.out.view(B),
                        tail=self.tail)
            return self.out.view(B)
        if self.keep[0] < 1 and self.masks[0] is not None:
            m = self.masks[0] / self.keep[0]
            xe = xe * m[:, : self.FD]
            xd = xd * m[:, self.FD:] if xd is not None else None
            self.xe, self.xd = xe, xd
        self._alloc_dense(xe.device)
        dotted = False
        for i in range(n):
            W, b = Ws[i], bs[i]
            a = self.a[i]
            if i == 0:
                ops.dense_fwd(xe, xd if self.Dn else None, W, a, self._fws, bias=b, act=self.act, ws6=self._fws6)
            else:
                # the last layer's kernel also forms the output projection a . dnn_w + dnn_w0 from its registers
                dot = None
                if i == n - 1 and not (self.keep[n] < 1 and self.masks[n] is not None):
                    dot = (w_out, w0, self.out.view(B))
                dotted = ops.dense_fwd(self.a[i - 1], None, W, a, self._fws, bias=b, act=self.act, ws6=self._fws6,
                                       dot=dot) and dot is not None
            if self.keep[i + 1] < 1 and self.masks[i + 1] is not None:
                a.mul_(self.masks[i + 1] / self.keep[i + 1])
        if not dotted:
            ops.rowdot(self.a[-1], w_out, w0, self.out.view(B))
        return self.out.view(B)

    def _alloc_dense(self, device):
        if self._fws is not None and self._fws.device == device and self._wws_B == self._B:
            return
        # (+ 16 columns: DCN rides the cross net's coefficient columns along the first layer's pass, wgrad0)
        self._fws, self._wws, self._fws6, self._wws6 = _dense_workspaces(
            [self.FD + self.Dn] + self.hidden, self._B, device, self.dense_gemm, wgrad6_pad=16)
        self._wws_B = self._B
        self._ws = torch.empty(256 * 1024, dtype=F32, device=device)
        self._ones = torch.ones(self._B, dtype=F32, device=device)

    def wgrad0(self, G2=None, dW2=None):
        """The first layer's weight gradient of a backward(..., defer_wgrad0=True) call, optionally with a second piece
        of gradient columns G2 [B, N2] -> dW2 [K, N2] against the SAME x = [xe | xd] in the same pass (DCN: the cross
        net's coefficient columns - x0 is then read once, rm_dense_wgrad6)."""
        da, gW, db = self._deferred
        self._deferred = None
        ops.dense_wgrad(self.xe, self.xd if self.Dn else None, da, gW, self._wws, db=db, ws6=self._wws6, G2=G2, dW2=dW2)

    def can_defer_wgrad0(self):
        """backward(defer_wgrad0=True) + wgrad0(G2, dW2) is available: wide layers on the split-operand path, no input
        dropout (the MLP's x is then the caller's x0 itself)."""
        return (not self.fused_ok and self._wws6 is not None
                and not (self.keep[0] < 1 and self.masks[0] is not None))

    def backward(self, g, dxe, fm_sum=None, lin_grads=None, defer_wgrad0=False):
        """g [B] = dLoss/dlogit; writes dLoss/dxe into dxe [B,FD] and the parameter
        gradients into self.g.  (No gradient is needed for the dense inputs.)
        fm_sum [B,D]: also add the FM second-order gradient g*(S - E) (fused path only;
        returns True when it was added).  lin_grads = (d_w_dense [Dn], d_w0 [1]): the linear
        term's dense-weight gradients g^T xd and sum g ride along too (fused path, Dn <= 32):
        self.lin_done tells the caller whether they were written."""
        (Ws, _, w_out, _), (gWs, gbs, g_w_out, g_w0) = self.vars(self.p), self.vars(self.g)
        n = len(self.hidden)
        self.lin_done = False
        if self.fused:
            ops.mlp_bwd(self.xe, self.xd if self.Dn else None, Ws, w_out, self.act,
                        g, self.hb, dxe, self.dhb, gWs, self.fws, fm_sum=fm_sum,
                        db=gbs, d_w_out=g_w_out, d_w0_out=g_w0,
                        d_xd_wsum=lin_grads[0] if (lin_grads and 1 <= self.Dn <= 32) else None,
                        d_g_sum=lin_grads[1] if (lin_grads and 1 <= self.Dn <= 32) else None,
                        tail=self.tail if self.head_done else None,
                        stream_d_rows=self.stream_d_rows)
            self.lin_done = bool(lin_grads and 1 <= self.Dn <= 32)
            return fm_sum is not None
        # d(pre-activation of the last layer) = (g w_out^T) o mask o act'(a): one elementwise pass
        # (rm_outer_actgrad; widths that are not a multiple of 4 take the K = 1 GEMM instead)
        da = self.da[-1]
        last_drop = self.keep[n] < 1 and self.masks[n] is not None
        plain = last_drop or self.act == "identity"
        # ... which, without dropout on that layer, also reduces the columns it reads and writes:
        # d dnn_w = a^T g, d dnn_w0 = sum g and the last hidden layer's bias gradient
        sums = (not plain) and da.shape[1] % 4 == 0 and da.shape[1] >= 64
        if sums:
            need = ops.outer_actgrad_sums_workspace(da.shape[0], da.shape[1])
            if self._sums_ws is None or self._sums_ws.numel() < need:
                self._sums_ws = torch.empty(need, dtype=F32, device=da.device)
            ops.outer_actgrad_sums(g, w_out, self.a[-1], self.act, da, g_w_out, g_w0, gbs[n - 1], self._sums_ws)
        else:
            ops.linear_dense_bwd(g, self.a[-1], g_w_out, g_w0, self._ws)
        if sums:
            pass
        elif da.shape[1] % 4 == 0:
            ops.outer_actgrad(g, w_out, None if plain else self.a[-1], self.act, da)
        else:
            ops.dense_fwd(g.view(-1, 1), None, w_out.view(-1, 1), da, self._fws, transposed=True,
                          epilogue=ops.DENSE_ADD if plain else ops.DENSE_MUL_ACTGRAD,
                          act=self.act, aux1=None if plain else self.a[-1])
        if last_drop:
            da.mul_(self.masks[n] / self.keep[n])
            if self.act != "identity":
                ops.act_bwd_(da, self.a[-1], self.act) if da.numel() % 4 == 0 else da.mul_(
                    torch.where(self.a[-1] > 0, 1.0, _ACTS[self.act] or 0.0))
        for i in range(n - 1, -1, -1):
            W, gW = Ws[i], gWs[i]
            # the bias gradient colsum(da): from rm_outer_actgrad_sums for the last layer, otherwise
            # it rides along in the weight-gradient kernel (which stages da in LDS anyway)
            db = None if (sums and i == n - 1) else gbs[i]
            if i == 0:
                if defer_wgrad0:
                    self._deferred = (da, gW, db)
                else:
                    ops.dense_wgrad(self.xe, self.xd if self.Dn else None, da, gW, self._wws, db=db, ws6=self._wws6)
                # dLoss/dxe = da W[:FD]^T (the dense inputs need no gradient)
                ops.dense_fwd(da, None, W[: self.FD], dxe, self._fws, transposed=True, epilogue=ops.DENSE_ADD,
                              ws6=self._fws6)
                if self.keep[0] < 1 and self.masks[0] is not None:
                    dxe.mul_(self.masks[0][:, : self.FD] / self.keep[0])
            else:
                prev = self.a[i - 1]
                ops.dense_wgrad(prev, None, da, gW, self._wws, db=db, ws6=self._wws6)
                dropped = self.keep[i] < 1 and self.masks[i] is not None
                # d(pre-activation of layer i-1) = (da W^T) o mask o act'(prev), act' from the stored
                # post-activation values (dropped positions are zeroed by the mask)
                ops.dense_fwd(da, None, W, self.da[i - 1], self._fws, transposed=True,
                              epilogue=ops.DENSE_MUL_ACTGRAD if self.act != "identity" else ops.DENSE_ADD,
                              act=self.act, aux1=prev if self.act != "identity" else None, ws6=self._fws6)
                da = self.da[i - 1]
                if dropped:
                    da.mul_(self.masks[i] / self.keep[i])
        return False


class DinUnit:
    """One sequence feature's pooling unit of kind "din": DIN's local activation unit (csrc/asp.hip, arXiv
    1706.06978).  Variables {name}_asp_layer_{i}_weights [4D | H_{i-1}, H_i], {name}_asp_layer_{i}_bias, {name}_asp_w
    [H_last, 1], {name}_asp_w0 [1] (absent from the reference, DIN.py:6: glorot weights and an output projection like
    dnn_w; no l2).  hp: att_hidden_units (80, 40), att_activation "sigmoid" (the reference's Dice, activation.py,
    uses undefined names), att_weight_normalization False.

    The interface of a pooling unit (SEQ_UNITS): __init__(var, hp, D, name, max_len) reads its hyper-parameters,
    rejects an unsupported shape and declares its variables through var (Engine._var); workspace(B, nnz) is the
    floats its backward needs; forward(seq, params, save, out, buf) and backward(seq, params, grads, d_out, d_keys,
    d_query, buf) take seq = (rows, row0, D, offsets, ids, qrow) and the field's buffers buf (Engine._seq_fwd);
    keeps_scores asks for buf["scores"], one float per occurrence."""
    keeps_scores = True

    def __init__(self, var, hp, D, name, max_len):
        self.D, self.name, self.max_len = D, name, max_len
        self.hidden = [int(h) for h in hp.get("att_hidden_units", (80, 40))]
        act = hp.get("att_activation", "sigmoid")
        act = act if isinstance(act, str) else getattr(act, "__name__", str(act))
        self.act = act.lower()
        if self.act == "dice":
            raise NotImplementedError("att_activation='dice': the reference's Dice (activation.py) uses undefined "
                                      "names and has no arithmetic to follow; use 'sigmoid' or 'relu'")
        if self.act not in ops.ASP_ACTS:
            raise ValueError(f"att_activation {act!r}: 'relu' or 'sigmoid'")
        self.norm = bool(hp.get("att_weight_normalization", False))
        if not ops.asp_supported(D, self.hidden, max_len):
            raise ValueError(f"sequence feature {name!r}: embedding_size={D}, att_hidden_units={self.hidden}, "
                             f"max_len={max_len} is not supported by rm_asp_fwd (embedding_size 8/16/32, "
                             "one or two hidden layers of 1..128 units, max_len 1..256)")
        dims = [4 * D] + self.hidden
        for i in range(len(self.hidden)):
            var(f"{name}_asp_layer_{i}_weights", (dims[i], dims[i + 1]), ("glorot", dims[i], dims[i + 1]))
            var(f"{name}_asp_layer_{i}_bias", (dims[i + 1],))
        var(f"{name}_asp_w", (dims[-1], 1), ("glorot", dims[-1], 1))
        var(f"{name}_asp_w0", (1,))

    def _vars(self, d):
        """(Ws, bs, w, w0) out of the params or the grads dict."""
        layers, name = range(len(self.hidden)), self.name
        return ([d[f"{name}_asp_layer_{i}_weights"] for i in layers], [d[f"{name}_asp_layer_{i}_bias"] for i in layers],
                d[f"{name}_asp_w"].view(-1), d[f"{name}_asp_w0"])

    def workspace(self, B, nnz):
        return ops.asp_workspace(self.D, self.hidden, nnz, True)

    def forward(self, seq, params, save, out, buf):
        ops.asp_fwd(*seq, *self._vars(params), self.act, self.norm, out, buf["scores"][: buf["nnz"]], buf["ws"])

    def backward(self, seq, params, grads, d_out, d_keys, d_query, buf):
        ops.asp_bwd(*seq, *self._vars(params), self.act, self.norm, buf["scores"][: buf["nnz"]], d_out, d_keys, d_query,
                    *self._vars(grads), buf["ws"])


class TransformerUnit:
    """Kind "transformer" (the interface: DinUnit): one post-norm encoder block over the history and the candidate,
    mean-pooled (csrc/bst.hip; Behavior Sequence Transformer, arXiv 1905.06874).  Variables {name}_bst_{wq|wk|wv|wo}
    [D, D], {name}_bst_{bq|bk|bv|bo} [D], {name}_bst_ffn_w1 [D, Hf], _ffn_b1 [Hf], _ffn_w2 [Hf, D], _ffn_b2 [D],
    {name}_bst_ln{1|2}_{gamma|beta} [D], {name}_bst_pos [max_len + 1, D] (absent from the reference: glorot matrices
    and position table, zero biases, LayerNorm gains "ones"; no l2).  hp: att_head_num 2, att_ffn_units 4 D."""
    keeps_scores = False

    def __init__(self, var, hp, D, name, max_len):
        self.D, self.name, self.max_len = D, name, max_len
        self.heads = int(hp.get("att_head_num", 2))
        ffn = hp.get("att_ffn_units")
        self.ffn = int(ffn) if ffn is not None else 4 * D
        if not ops.bst_supported(D, self.heads, self.ffn, max_len):
            raise ValueError(f"sequence feature {name!r}: embedding_size={D}, att_head_num={self.heads}, "
                             f"att_ffn_units={self.ffn}, max_len={max_len} is not supported by rm_bst_fwd "
                             f"({ops.BST_LIMITS})")
        for v, shape in ops.bst_param_shapes(D, self.ffn, max_len).items():
            if len(shape) == 2:
                init = ("glorot", shape[0], shape[1])
            else:
                init = "ones" if v.endswith("_gamma") else "zeros"
            var(f"{name}_bst_{v}", shape, init)

    def _vars(self, d):
        """{member: tensor} out of the params or the grads dict."""
        return {v: d[f"{self.name}_bst_{v}"] for v in ops.BST_PARAM_NAMES}

    def workspace(self, B, nnz):
        return ops.bst_workspace(self.D, self.heads, self.ffn, self.max_len, B, True)

    def forward(self, seq, params, save, out, buf):
        ops.bst_fwd(*seq, self._vars(params), self.heads, self.max_len, out, buf["ws"])

    def backward(self, seq, params, grads, d_out, d_keys, d_query, buf):
        ops.bst_bwd(*seq, self._vars(params), self.heads, self.max_len, d_out, d_keys, d_query, self._vars(grads),
                    buf["ws"])


class DienUnit:
    """Kind "dien" (the interface: DinUnit): a GRU over the history, the candidate's attention over its states and an
    attention-gated GRU whose last state is the row (csrc/dien.hip; Deep Interest Evolution Network, arXiv
    1809.03672, hidden size D, no auxiliary loss).  Variables {name}_dien_{gru|augru}_{w|u} [D, 3D],
    {name}_dien_{gru|augru}_b [3D], {name}_dien_att_w [D, D] (absent from the reference: glorot matrices, zero
    biases; no l2).  No hyper-parameter.  Its forward keeps what the backward needs in the workspace (save)."""
    keeps_scores = False

    def __init__(self, var, hp, D, name, max_len):
        self.D, self.name, self.max_len = D, name, max_len
        if not ops.dien_supported(D, max_len):
            raise ValueError(f"sequence feature {name!r}: embedding_size={D}, max_len={max_len} is not supported by "
                             f"rm_dien_fwd ({ops.DIEN_LIMITS})")
        for v, shape in ops.dien_param_shapes(D).items():
            var(f"{name}_dien_{v}", shape, ("glorot", shape[0], shape[1]) if len(shape) == 2 else "zeros")

    def _vars(self, d):
        """{member: tensor} out of the params or the grads dict."""
        return {v: d[f"{self.name}_dien_{v}"] for v in ops.DIEN_PARAM_NAMES}

    def workspace(self, B, nnz):
        return ops.dien_workspace(self.D, self.max_len, B, nnz, True)

    def forward(self, seq, params, save, out, buf):
        ops.dien_fwd(*seq, self._vars(params), self.max_len, save, out, buf["ws"])

    def backward(self, seq, params, grads, d_out, d_keys, d_query, buf):
        ops.dien_bwd(*seq, self._vars(params), self.max_len, d_out, d_keys, d_query, self._vars(grads), buf["ws"])


SEQ_UNITS = {"din": DinUnit, "transformer": TransformerUnit, "dien": DienUnit}


def init_reference(engine, seed=2019):
    """Initial values with the reference's distributions (TF's RNG stream itself cannot be reproduced): every
    variable of engine.params, in insertion order, by the rule it was declared with (Engine._var) - embedding
    tables, DNN and CIN weights truncated-normal glorot (utils.py:180-183; layers.py:99-101,536,551,567,666), cin_w
    glorot-uniform (layers.py:690), biases zeros (layers.py:109,321,327,544,561,574,676,695); the layers absent from
    the reference (cross net, attention units, interacting layers, DLRM's towers) glorot weights like dnn_w and zero
    biases; the field-pair weights of FmFM / FvFM / FwFM ("pair_identity") identity matrices or ones; MaskNet's
    LayerNorm gains "ones".  A variable without a declared rule is a KeyError."""
    import math

    g = torch.Generator(device=engine.device).manual_seed(int(seed))
    for name, t in engine.params.items():
        if name not in engine.decl:
            raise KeyError(f"variable {name!r} was never declared: it has no init rule")
        init = engine.decl[name][0]
        if init == "zeros":
            t.zero_()
            continue
        if init == "ones":
            t.fill_(1.0)  # LayerNorm gains (MaskNet)
            continue
        if init == "pair_identity":
            # the field-pair weights start the model at plain FM: identity matrices [P,D,D], all-ones vectors [P,D]
            # and scalars [P]
            if t.dim() == 3:
                t.copy_(torch.eye(t.shape[1], dtype=t.dtype, device=t.device).expand_as(t))
            else:
                t.fill_(1.0)
            continue
        kind, fan_in, fan_out = init
        if kind == "glorot":
            std = math.sqrt(2.0 / (fan_in + fan_out))
            torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std, generator=g)
        elif kind == "glorot_uniform":
            b = math.sqrt(6.0 / (fan_in + fan_out))
            t.uniform_(-b, b, generator=g)
        else:
            raise ValueError(f"variable {name!r}: unknown init rule {init!r}")


class Engine:
    """Shared storage + the embedding / linear / loss plumbing.  Subclasses add the
    model-specific branches and define `_branches_fwd` / `_branches_bwd`."""

    model = "base"
    use_bias_tables = False
    shardable = False  # recman_amd/dist.py has a row-sharded engine for this model

    @classmethod
    def require_shardable(cls):
        if not cls.shardable:
            raise NotImplementedError(
                f"{cls.model} runs on one GPU: there is no row-sharded engine for it (table_sharding='row' or a "
                "multi-rank torch.distributed job); use table_sharding='none'")

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("recman_amd engines need a GPU (MI355X); there is no CPU path")
        self.spec, self.D, self.hp, self.task = spec, int(embedding_size), dict(hp), task
        self.device = torch.device(device)
        dev = self.device
        F, R, Dn = spec.F, spec.rows, spec.Dn
        self.F, self.Dn, self.FD = F, Dn, F * self.D
        self.params, self.grads = {}, {}
        # every variable's name -> (init rule, l2 key) in declaration order (_var / _view / _adopt), and the names
        # each l2 hyper-parameter regularises.  NAMES only: the optimizers and recman_amd/dist.py re-home the
        # tensors of params / grads, and the sharded engine swaps self.hp for a scaled copy per call
        self.decl, self.l2_groups = {}, {}
        self.mlp = None
        self.grad_scale = 1.0   # this batch's share of a step's gradient (micro-batches, recman_amd/dist.py)
        self._head_req = None   # fwd_bwd's offer of the fused head to the model's last DNN (_mlp_last)
        self.d_bias = None      # per-occurrence bias-table gradients [B,F] (FM bias dropout only)
        self.rank = self._rank_objective()  # the ranking term next to the log loss (None: not configured)
        self._probe_ready = None
        self._alloc_tables()
        self._var("linear_w0", (1,))
        self.grads["linear_w_dense"] = torch.zeros(Dn, dtype=F32, device=dev)
        self._B = None
        self.use_linear = True
        self._init_seq()

    def _rank_objective(self):
        """hp["rank_loss"] ("pairwise" | "listwise"; None: no ranking term) with rank_norm, rank_loss_weight and the
        group ids - hp["rank_group_col"], a column of idx, or hp["rank_group_by"], the name of a plain id feature; None:
        the whole batch is one list - as dict(kind, norm, alpha, col).  th.DeepModel._rank_config is the checked public
        surface; this is what an engine built directly accepts."""
        hp = self.hp
        kind = hp.get("rank_loss")
        if kind is None:
            return None
        if self.model in ("mmoe", "ple", "twotower"):
            raise NotImplementedError(f"rank_loss={kind!r}: {self.model} has no single logit with a 0/1 label to rank")
        if getattr(self, "sharded", False):
            raise NotImplementedError(f"rank_loss={kind!r} runs on one GPU: pairs across ranks or micro-batches are not "
                                      "built; use table_sharding='none'")
        if self.task != "classification":
            raise ValueError(f"rank_loss={kind!r} needs 0/1 labels: the task is {self.task!r}")
        norm, alpha = hp.get("rank_norm", "group"), float(hp.get("rank_loss_weight", 0.5))
        if kind not in ops.RANK_KINDS or norm not in ops.RANK_NORMS or not 0 < alpha <= 1:
            raise ValueError(f"rank_loss={kind!r}, rank_norm={norm!r}, rank_loss_weight={alpha!r}: expected "
                             f"{sorted(ops.RANK_KINDS)}, {sorted(ops.RANK_NORMS)} and 0 < rank_loss_weight <= 1")
        col, by = hp.get("rank_group_col"), hp.get("rank_group_by")
        if col is None and by is not None:
            if by not in self.spec.sparse_names or by in self.spec.scratch_names:
                raise ValueError(f"rank_group_by={by!r} must name a plain id feature")
            col = self.spec.sparse_names.index(by)
        return dict(kind=kind, norm=norm, alpha=alpha, col=None if col is None else int(col))

    def _rank_step(self, idx, y, scale):
        """After rm_logit_loss: loss <- (1 - alpha) loss + alpha L, dlogit <- scale ((1 - alpha) dlogit + alpha
        dL/dlogit) over the groups of THIS batch (rm_rank_loss).  The device record is not asked for: no sync."""
        r = self.rank
        groups = None if r["col"] is None else idx[:, r["col"]].contiguous()
        ops.rank_loss(self.logit, y, groups, r["kind"], r["norm"], r["alpha"], self.dlogit, grad_scale=scale,
                      dlogit_in=self.dlogit, loss_in=self.loss, loss_out=self.loss, workspace=self._rank_ws)

    def _var(self, name, shape, init="zeros", l2=None):
        """Declares a dense variable of this engine (_declare): params / grads pair, init rule, l2 key."""
        _declare(self.params, self.grads, self.decl, name, shape, self.device, init, l2)
        if l2 is not None:
            self.l2_groups.setdefault(l2, []).append(name)

    def _view(self, name, t, init="zeros"):
        """Declares a variable that is a view of storage laid out elsewhere (the table): no l2 key, no grads entry."""
        self.params[name] = t
        self.decl[name] = (init, None)

    def _adopt(self, net):
        """Takes over the declarations of an MLP / Tower built on self.params / self.grads; returns it."""
        self.decl.update(net.decl)
        for name, (_, l2) in net.decl.items():
            if l2 is not None:
                self.l2_groups.setdefault(l2, []).append(name)
        return net

    def _dnn(self, FD, Dn, hidden, default_activation, prefix="", stream_d_rows=None):
        """The model's DNN on this engine's variables, with the hyper-parameters every model passes it."""
        hp = self.hp
        if stream_d_rows is None:
            stream_d_rows = hp.get("d_rows_reuse", "cache") == "stream"
        return self._adopt(MLP(self.params, self.grads, FD, Dn, hidden, hp.get("deep_activation", default_activation),
                               self.device, prefix=prefix, stream_d_rows=stream_d_rows,
                               dense_gemm=hp.get("dense_gemm", "bf16x6")))

    def _dnn_keep(self, training):
        """The DNN's keep probabilities for this call (deep_dropout; all ones outside training)."""
        n = len(self.mlp.hidden)
        return list(self.hp.get("deep_dropout") or [1] * (n + 1)) if training else [1] * (n + 1)

    def _init_seq(self):
        """One pooling unit per sequence feature, of the kind hp["seq_pooling"] names (SEQ_UNITS; default "din").
        att_dropout must be all ones under every kind."""
        spec, hp = self.spec, self.hp
        self._seq_units, self._seq_buf, self._seq_save = {}, {}, False
        self.seq_pooling = str(hp.get("seq_pooling", "din")).lower()
        if self.seq_pooling not in SEQ_UNITS:
            raise ValueError(f"seq_pooling {hp.get('seq_pooling')!r}: 'din', 'transformer' or 'dien'")
        if not spec.seq_names:
            return
        if not hasattr(self, "rows") or self.rows.dim() != 2 or self.rows.shape[0] != spec.rows:
            raise NotImplementedError("sequence features (SequenceFeat) need the whole table on one GPU: there is "
                                      "no row-sharded path for them (use table_sharding='none')")
        self._check_att_dropout()
        for n in spec.seq_names:
            self._seq_units[spec.sparse_names.index(n)] = SEQ_UNITS[self.seq_pooling](
                self._var, hp, self.D, n, int(spec.seq_max_len[n]))

    def _check_att_dropout(self):
        drop = self.hp.get("att_dropout", 1)
        drop = list(drop) if isinstance(drop, (list, tuple)) else [drop]
        if any(float(k) != 1.0 for k in drop):
            raise NotImplementedError("att_dropout: the attention unit runs without dropout (every keep "
                                      f"probability must be 1, got {self.hp.get('att_dropout')!r})")

    def _seq_fwd(self, j, f, idx):
        """Sequence field f (scratch block j): its unit pools the history rows into the scratch rows.  The field's
        buffers - key gradients (and scores, if the unit keeps them) per occurrence, the unit's workspace - grow when
        a batch has more occurrences or needs more workspace than any before; the CSR is kept for _seq_bwd."""
        unit = self._seq_units[f]
        offsets, ids, _ = self._mv_entry(f)
        fq = self.spec.sparse_names.index(self.spec.seq_query[unit.name])
        row0 = int(self.field_off_host[fq])
        B, nnz = int(idx.shape[0]), int(ids.shape[0])
        buf = self._seq_buf.get(f)
        if buf is None or buf["cap"] < nnz or buf["ws"].numel() < unit.workspace(B, nnz):
            cap = max(nnz, 1)
            buf = dict(cap=cap, d_keys=torch.empty(cap, self.D, dtype=F32, device=self.device),
                       ws=torch.empty(max(4, unit.workspace(B, cap)), dtype=F32, device=self.device))
            if unit.keeps_scores:
                buf["scores"] = torch.empty(cap, dtype=F32, device=self.device)
            self._seq_buf[f] = buf
        buf.update(csr=(offsets, ids, idx[:, fq] + row0), nnz=nnz, row0=row0, fq=fq)
        unit.forward((self.rows, row0, self.D, *buf["csr"]), self.params, self._seq_save, self.mv_scratch[j], buf)

    def _seq_bwd(self):
        """After the model's backward filled d_rows: every sequence field's pooled-row gradient goes through its
        unit - key gradients per history occurrence (kept for dense_grads / the row-wise optimizer), the query
        gradient ADDED onto the query field's rows of d_rows, the unit's parameter gradients."""
        for f in self.mv_fields:
            unit = self._seq_units.get(f)
            if unit is None:
                continue
            b = self._seq_buf[f]
            unit.backward((self.rows, b["row0"], self.D, *b["csr"]), self.params, self.grads, self.d_rows[:, f, :],
                          b["d_keys"][: b["nnz"]], self.d_rows[:, b["fq"], :], b)

    def seq_key_grads(self, f):
        """(field of the query feature, history ids [nnz], their gradient rows [nnz, D]) of sequence field f after
        the last fwd_bwd."""
        b = self._seq_buf[f]
        return b["fq"], b["csr"][1], b["d_keys"][: b["nnz"]]

    def _alloc_tables(self):
        """HBM layout: ONE table of fused rows [R, LD], LD = 2*D floats (a power of two, so a
        row never straddles a 128-byte line): columns 0..D-1 the embedding, column D the FM
        bias-table entry, column D+1 the sparse linear weight, the rest padding.  One line
        fetch per lookup serves all three (tools/bench_embed.py: as separate tables the two
        4-byte gathers cost as much as the row gather).  The reference's per-feature
        variables are strided views of it; `linear_w` is assembled by state_dict().
        (recman_amd/dist.py overrides this with the row-sharded layout.)"""
        spec, dev, Dn, D = self.spec, self.device, self.Dn, self.D
        R = spec.rows
        self.LD = 2 * D
        self.rows = torch.zeros(R, self.LD, dtype=F32, device=dev)
        self.table = self.rows
        self.linear_w_dense = torch.zeros(Dn, dtype=F32, device=dev)
        offs = spec.offsets()
        self.field_off_host = offs
        self._mv = None
        self.field_off = torch.tensor(offs, dtype=I64, device=dev)
        self.lin_off = self.field_off  # sparse one-hot blocks share the table's row numbering
        for name, off, V in zip(spec.sparse_names, offs, spec.feat_sizes):
            if name in spec.seq_query:
                continue  # a history shares its query feature's rows
            self._view(f"{name}_feat_embed", self.rows[off: off + V, :D], ("glorot", V, D))
            if self.use_bias_tables:
                self._view(f"{name}_feat_bias", self.rows[off: off + V, D: D + 1])
        self._view("linear_w_sparse", self.rows[:, D + 1])
        self._view("linear_w_dense", self.linear_w_dense)
        self._set_lin_masks()

    def storage(self):
        """The distinct parameter buffers (for initialisers that fill storage in place)."""
        seen, out = set(), []
        for t in self.params.values():
            base = t if t._base is None else t._base
            if base.data_ptr() not in seen:
                seen.add(base.data_ptr())
                out.append(base)
        return out

    # ------------------------------------------------------------------ storage
    def load_params(self, params):
        """Copies a name -> tensor dict (reference variable names) into the engine."""
        R = self.spec.rows
        for k, v in params.items():
            v = torch.as_tensor(v).to(self.device, F32)
            if k == "linear_w":  # the reference's stacked one-hot blocks / dense columns
                vs, vd = self._lin_from_ref(v.reshape(-1))
                self.params["linear_w_sparse"].copy_(vs)
                self.params["linear_w_dense"].copy_(vd)
                continue
            if k not in self.params:
                raise KeyError(f"unknown variable {k!r}")
            dst = self.params[k]
            dst.copy_(v.reshape(dst.shape))

    def state_dict(self):
        """name -> tensor under the reference's variable names (contiguous copies)."""
        out = {}
        for k, v in self.params.items():
            if k in ("linear_w_sparse", "linear_w_dense"):
                continue
            out[k] = v.detach().clone().contiguous()
        if "linear_w_sparse" in self.params:
            out["linear_w"] = self._lin_to_ref(self.params["linear_w_sparse"].detach().reshape(-1),
                                               self.params["linear_w_dense"].detach().reshape(-1)).view(-1, 1)
        return out

    def _set_lin_masks(self):
        """linear_features subsets: the linear weights of the other features stay at their zero
        initial value (W is zero-initialised, layers.py:318-328) because their gradient is masked."""
        mf, md = self.spec.lin_masks()
        dev = self.device
        self.lin_field_mask = None if mf is None else torch.tensor(mf, dtype=F32, device=dev)
        self.lin_dense_mask = None if (md is None or not md) else torch.tensor(md, dtype=F32, device=dev)

    def _lin_to_ref(self, v_rows, v_dense):
        """([R] in table-row order, [Dn]) -> the reference's linear_w: its one-hot blocks and dense
        columns in its order (default: sparse, value, multi-valued, dense; or `linear_features`)."""
        if self.spec.linear_names is None and not self.spec.scratch_names:
            return torch.cat([v_rows, v_dense])
        return torch.cat([v_rows[p[1]: p[1] + p[2]] if p[0] == "s" else v_dense[p[1]: p[1] + 1]
                          for p in self.spec.lin_ref_layout()])

    def _lin_from_ref(self, v_ref):
        """The inverse: (rows [R], dense [Dn]); entries of features outside `linear_features` are 0."""
        R, Dn = self.spec.rows, self.Dn
        if self.spec.linear_names is None and not self.spec.scratch_names:
            return v_ref[:R], v_ref[R:]
        vs, vd = v_ref.new_zeros(R), v_ref.new_zeros(Dn)
        at = 0
        for p in self.spec.lin_ref_layout():
            if p[0] == "s":
                vs[p[1]: p[1] + p[2]] = v_ref[at: at + p[2]]
                at += p[2]
            else:
                vd[p[1]] = v_ref[at]
                at += 1
        if at != v_ref.numel():
            raise ValueError(f"linear_w has {v_ref.numel()} entries, the linear features need {at}")
        return vs, vd

    def to_reference_names(self, d):
        """Merges the internal linear_w_sparse / linear_w_dense entries into `linear_w`."""
        d = dict(d)
        if "linear_w_sparse" in d:
            d["linear_w"] = self._lin_to_ref(d.pop("linear_w_sparse").reshape(-1),
                                             d.pop("linear_w_dense").reshape(-1)).view(-1, 1)
        return d

    def _alloc(self, B):
        if self._B == B:
            return
        self._B = B
        dev = self.device
        self.E = torch.empty(B, self.F, self.D, dtype=F32, device=dev)
        self.d_rows = torch.empty(B, self.F, self.D, dtype=F32, device=dev)
        self.fm_sum = torch.empty(B, self.D, dtype=F32, device=dev)
        self.fm_logit = torch.empty(B, dtype=F32, device=dev)
        self.lin_logit = torch.empty(B, dtype=F32, device=dev)
        self.logit = torch.empty(B, dtype=F32, device=dev)
        self.pred = torch.empty(B, dtype=F32, device=dev)
        self.dlogit = torch.empty(B, dtype=F32, device=dev)
        self.loss = torch.zeros(1, dtype=F32, device=dev)
        self.loss_part = torch.empty((B + 31) // 32, dtype=F32, device=dev)  # fused head: per-tile loss sums
        self.ws = torch.empty(256 * 1024, dtype=F32, device=dev)
        if self.rank is not None:
            self._rank_ws = torch.empty(ops.rank_loss_workspace(B), dtype=torch.uint8, device=dev)
        self.mv_fields = [f for f, n in enumerate(self.spec.sparse_names) if n in self.spec.scratch_names]
        self._alloc_mv(B)
        self._alloc_model(B)

    def _alloc_mv(self, B):
        dev = self.device
        if self.mv_fields:
            # per-batch pooled rows of the multi-valued features live in a scratch block that is
            # addressed AS ROWS OF THE TABLE: its start is aligned so that (scratch - table) is a
            # whole number of rows, and the gather kernel reads row `base + b` like any other
            LD = self.LD
            raw = torch.zeros((len(self.mv_fields) * B + 2) * LD, dtype=F32, device=dev)
            shift = ((self.rows.data_ptr() - raw.data_ptr()) // 4) % LD
            self._mv_raw = raw
            self.mv_scratch = raw[shift: shift + len(self.mv_fields) * B * LD].view(len(self.mv_fields), B, LD)
            base = (self.mv_scratch.data_ptr() - self.rows.data_ptr()) // (4 * LD)
            assert (self.mv_scratch.data_ptr() - self.rows.data_ptr()) % (4 * LD) == 0
            self.field_off_mv = self.field_off.clone()
            for j, f in enumerate(self.mv_fields):
                self.field_off_mv[f] = base + j * B
            self.idx_mv = torch.zeros(B, self.F, dtype=I64, device=dev)
            self._arange = torch.arange(B, dtype=I64, device=dev)

    def _alloc_model(self, B):
        pass

    # ------------------------------------------------------------------ forward
    def _embed(self, idx, dense, want_fm, masks, lin_w=None):
        m = masks or {}
        fm_masks = m.get("fm", (None, None))
        D = self.D
        foff = self.field_off
        if self.mv_fields:
            mv = self._mv
            if mv is None:
                raise ValueError(f"features {self.spec.scratch_names} need their ids / values (mv=...)")
            self.idx_mv.copy_(idx)
            for j, f in enumerate(self.mv_fields):
                if self.spec.sparse_names[f] in self.spec.seq_query:
                    self._seq_fwd(j, f, idx)
                    self.idx_mv[:, f] = self._arange
                    continue
                offsets, ids, vals = self._mv_entry(f)
                ops.pool_rows(self.rows, int(self.field_off_host[f]), D, offsets, ids, self.mv_scratch[j],
                              vals=vals)
                self.idx_mv[:, f] = self._arange
            idx, foff = self.idx_mv, self.field_off_mv
        ops.embed_fwd(
            idx, self.rows, foff, D=D, table_ld=self.LD,
            bias_col=D if (want_fm and self.use_bias_tables) else None,
            lin_col=D + 1 if self.use_linear else None,
            lin_w_dense=self.linear_w_dense if (self.use_linear and self.Dn) else None,
            dense=dense if (self.use_linear and self.Dn) else None,
            lin_w0=self.params["linear_w0"] if self.use_linear else None,
            mask_b=fm_masks[0] if want_fm else None, mask_e=fm_masks[1] if want_fm else None,
            E=self.E, fm_sum=self.fm_sum if want_fm else None,
            fm_logit=self.fm_logit if want_fm else None,
            lin_logit=self.lin_logit if self.use_linear else None,
            # hp["table_row_reuse"] = "stream" (default): ids touch a row about once per batch
            # (hashed ids over a table far beyond the caches) -> non-temporal row loads keep E in the
            # caches for the MLP / CIN kernels; "cache": heavy id reuse (Zipf-like), plain loads
            stream_rows=self.hp.get("table_row_reuse", "stream") == "stream")

    def _embed_plain(self, idx, dense, training, masks, lin_w):
        """The opening of a _branches_fwd without an FM term: the masks of this call (none outside training), then
        the plain embed (E and the linear logit); returns the masks."""
        m = (masks or {}) if training else {}
        self._embed(idx, dense, False, m, lin_w)
        return m

    def _mv_entry(self, f):
        """(offsets, ids, vals) of scratch-row field f from the mv dict: a multi-valued feature
        gives (offsets, ids); a value feature (offsets, ids, vals) with one id per example."""
        name = self.spec.sparse_names[f]
        ent = self._mv[name]
        vals = ent[2] if len(ent) > 2 else None
        if (name in self.spec.value_names) != (vals is not None):
            raise ValueError(f"feature {name}: value features take (offsets, ids, vals), "
                             "multi-valued ones (offsets, ids)")
        return ent[0], ent[1], vals

    def forward(self, idx, dense=None, training=False, masks=None, manual_weights=None, mv=None):
        """-> (logit [B], pred [B]).  training=False disables dropout and (as the
        reference does, layers.py:338-345) adds the per-feature manual weights (a vector in
        the reference's linear_w order).  mv: name -> (offsets, ids) device tensors of the
        multi-valued features."""
        self._alloc(idx.shape[0])
        self._mv = mv
        self._seq_save = bool(training)
        backup = None
        if manual_weights is not None:
            # W + weights for this call only: exact restore from a copy (an add/subtract pair
            # would drift by an ulp per predict call)
            mw = manual_weights.to(self.device, F32).reshape(-1)
            R = self.spec.rows
            backup = (self.params["linear_w_sparse"].clone(), self.linear_w_dense.clone())
            ms, md = self._lin_from_ref(mw)
            self.params["linear_w_sparse"].add_(ms)
            self.linear_w_dense.add_(md)
        try:
            branches = self._branches_fwd(idx, dense, training, masks, None)
            ops.logit_loss(branches, task=self.task, logit=self.logit, pred=self.pred)
        finally:
            if backup is not None:
                self.params["linear_w_sparse"].copy_(backup[0])
                self.linear_w_dense.copy_(backup[1])
        return self.logit, self.pred

    # --------------------------------------------------------- forward+backward
    def fwd_bwd(self, idx, dense, y, masks=None, mv=None):
        """One training step's forward + backward.  Returns the loss tensor [1]
        (data loss + l2 terms).  Gradients: self.grads (dense parameters),
        self.d_rows [B,F,D] + idx (embedding rows, IndexedSlices form), self.dlogit
        (per-occurrence gradient of the bias-table / sparse linear entries)."""
        B = idx.shape[0]
        self._alloc(B)
        self._mv = mv
        self._seq_save = True
        yk = dict(y=y) if y.dtype == I64 else dict(y_f=y)
        scale = self.grad_scale
        # models whose DNN is the last branch of the forward offer it the fused head (rm_mlp_tail):
        # final logit, prediction, loss and dLoss/dlogit in the MLP kernel's epilogue.  Not with a ranking term: it
        # needs every logit of the batch before any dlogit exists, so the head is rm_logit_loss + rm_rank_loss
        self._head_req = None if self.rank is not None else dict(
            task=self.task, grad_scale=scale, logit=self.logit, pred=self.pred, dlogit=self.dlogit,
            loss_partial=self.loss_part, loss=self.loss, **yk)
        self._head_done = False
        try:
            branches = self._branches_fwd(idx, dense, True, masks, None)
        finally:
            self._head_req = None
        if not self._head_done:
            ops.logit_loss(branches, task=self.task, logit=self.logit, pred=self.pred,
                           dlogit=self.dlogit, loss=self.loss, workspace=self.ws, **yk)
            if self.rank is not None:
                self._rank_step(idx, y, scale)
            elif scale != 1.0:
                # this batch is one of several micro-batches of a step: its gradients are its share
                # of the full-batch mean (recman_amd/dist.py)
                self.dlogit.mul_(scale)
        self._lin_done = False
        self._branches_bwd(idx, dense, self.dlogit, masks)
        self._add_l2_grads()
        self._seq_bwd()
        if self.use_linear and not self._lin_done:
            ops.linear_dense_bwd(self.dlogit, dense if self.Dn else None,
                                 self.grads["linear_w_dense"] if self.Dn else None,
                                 self.grads["linear_w0"], self.ws)
        if self.use_linear and self.Dn and self.lin_dense_mask is not None:
            self.grads["linear_w_dense"].mul_(self.lin_dense_mask)  # linear_features subset
        return self._add_l2(self.loss)

    fuse_head = True  # tests switch it off to compare against rm_logit_loss + the chain kernel

    def _mlp_last(self, mlp, xe, xd, keep, masks, others):
        """The DNN as the LAST branch of the forward: `others` = the (logit, coefficient) pairs
        already computed.  Hands the fused head to the MLP when fwd_bwd asked for it and at most two
        other branches exist; returns the DNN logit."""
        req = self._head_req if self.fuse_head else None
        head = dict(req, branches=others, coef_mlp=1.0) if (req is not None and len(others) <= 2) else None
        out = mlp.forward(xe, xd, keep, masks, head=head)
        self._head_done = bool(head is not None and mlp.head_done)
        return out

    def _lin_grads(self):
        """(d linear_w_dense, d linear_w0) for MLP.backward to fill when the linear term is on."""
        if not (self.use_linear and self.Dn):
            return None
        return (self.grads["linear_w_dense"], self.grads["linear_w0"])

    def _add_l2(self, loss):
        hp = self.hp
        total = loss
        if hp.get("lazy_l2", False):
            # LAZY l2 (the row-wise optimizer adds reg * row for the rows a batch touches): the
            # table's l2 terms are neither summed into the loss (a pass over the whole table per step) nor turned
            # into a dense gradient; the linear term's DENSE weights keep their exact l2 gradient
            reg = hp.get("linear_l2_reg", 0.0)
            if reg and self.use_linear and self.Dn:
                self.grads["linear_w_dense"].add_(self.linear_w_dense, alpha=reg)
                total = total + reg * 0.5 * self.linear_w_dense.square().sum()
            return self._add_l2_model(total)
        reg = hp.get("embedding_l2_reg", 0.0)
        if reg:
            total = total + reg * 0.5 * self.rows[:, : self.D].square().sum()
        reg = hp.get("linear_l2_reg", 0.0)
        if reg and self.use_linear:
            total = total + reg * 0.5 * (self.params["linear_w_sparse"].square().sum()
                                         + self.linear_w_dense.square().sum())
        return self._add_l2_model(total)

    def _add_l2_model(self, total):
        """+ the l2 value of the model's own variables: per declared key, reg / 2 * sum w^2 over its group
        (layers.py:611-628).  Coefficients from self.hp and tensors from self.params at call time."""
        for key, names in self.l2_groups.items():
            reg = self.hp.get(key, 0.0)
            if reg:
                total = total + sum(reg * 0.5 * self.params[n].square().sum() for n in names)
        return total

    def _add_l2_grads(self):
        """+ the l2 gradient reg * w of the same groups onto self.grads."""
        for key, names in self.l2_groups.items():
            reg = self.hp.get(key, 0.0)
            if reg:
                for n in names:
                    self.grads[n].add_(self.params[n], alpha=reg)

    # ---------------------------------------------------------------- dropout
    def dropout_masks(self, B):
        """0/1 keep masks for the configured keep-probabilities (tf.nn.dropout, layers.py:461,466,589,602), drawn
        on the GPU: masks["dnn"] for the model's DNN, then the model's own (_model_masks); None when there are none."""
        masks = {}
        keep = self.hp.get("deep_dropout")
        if keep is not None and any(k < 1 for k in keep) and self.mlp is not None:
            dims = [self.mlp.FD + self.mlp.Dn] + self.mlp.hidden
            masks["dnn"] = [(torch.rand(B, d, device=self.device) < k).float() if k < 1 else None
                            for d, k in zip(dims, keep)]
        self._model_masks(B, masks)
        return masks or None

    def _model_masks(self, B, masks):
        pass

    # ------------------------------------------------------------ measurement
    def roofline_probes(self, idx, dense, y):
        """The hand-written hot kernels of this model as [{name, symbol, fn, work, bound}], the
        dominant one first: `fn` launches the kernel once on the current stream, `work` is its
        algorithmic bytes (bound "hbm") or flops (bound "mfma") per launch, `symbol`
        the kernel's name in a rocprofv3 trace."""
        self._alloc(idx.shape[0])
        fm = self._has_fm()
        return [dict(name="embed_fwd_fused_kernel (rm_embed_fwd: gather + FM + linear)",
                     symbol="embed_fwd_fused_kernel", fn=lambda: self._embed(idx, dense, fm, None),
                     work=self._embed_fwd_bytes(idx.shape[0], fm), bound="hbm")]

    def _probes(self, idx, dense, y, *own):
        """A model's probe list: its own kernels as (name, symbol, fn, work, bound), the dominant one first (by habit
        the backward kernel, then the forward kernel), followed by the base's gather probe."""
        return ([dict(zip(("name", "symbol", "fn", "work", "bound"), p)) for p in own]
                + Engine.roofline_probes(self, idx, dense, y))

    def _probe_fill(self, idx, dense, y):
        """One fwd_bwd per batch size, so that the kernels a probe launches on their own find their inputs."""
        B = idx.shape[0]
        self._alloc(B)
        if self._probe_ready != B:
            self.fwd_bwd(idx, dense, y)
            self._probe_ready = B

    def roofline_probe_all(self, idx, dense, y, iters=20):
        """Times every roofline_probes() kernel with HIP events on the stream it is launched on and
        prices it against its roofline."""
        out = []
        for p in self.roofline_probes(idx, dense, y):
            fn = p["fn"]
            # warm-up by TIME, not by count: the chip raises its clock only after ~10 ms of sustained load
            # (in-kernel s_memtime / s_memrealtime: a 0.37 ms GEMM launch runs at 1.97 GHz after 15
            # back-to-back launches and at 2.35 GHz after 30, profiles/r02_dense_gemm.md) - the training
            # loop the kernel belongs to runs sustained, so it is priced at the sustained clock
            t_warm = torch.cuda.Event(enable_timing=True)
            t_warm.record()
            for _ in range(3):
                fn()
            while True:
                for _ in range(5):
                    fn()
                t_now = torch.cuda.Event(enable_timing=True)
                t_now.record()
                t_now.synchronize()
                if t_warm.elapsed_time(t_now) >= 40.0:
                    break
            iters_p = max(iters, 50) if p["bound"] == "hbm" else iters  # (the MFMA kernels take milliseconds each)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(iters_p)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            ts = sorted(a.elapsed_time(b) for a, b in ev)
            ms = sum(ts) / len(ts)
            if p["bound"] == "hbm":
                achieved, peak, unit = p["work"] / (ms * 1e-3) / 1e9, 8000.0, "GB/s"
            else:
                # (peak: the dense f32 MFMA rate, or the probe's own - the bf16 pipe for the split-operand GEMM)
                achieved, peak, unit = p["work"] / (ms * 1e-3) / 1e12, p.get("peak", 157.3), "TFLOP/s"
            rec = {"kernel": p["name"], "symbol": p["symbol"], "bound": p["bound"],
                   "achieved": round(achieved, 2), "peak": peak, "unit": unit,
                   "frac": round(achieved / peak, 4), "traffic": None,
                   "avg_launch_us": round(ms * 1e3, 2), "min_launch_us": round(ts[0] * 1e3, 2),
                   "median_launch_us": round(ts[len(ts) // 2] * 1e3, 2), "algorithmic_per_launch": p["work"],
                   "timing": f"hipEvent pairs, {iters_p} launches (mean; min and median beside it)"}
            if "extra" in p:
                rec.update(p["extra"](ms))
            if "work_min" in p:
                # the same launch priced on the bytes the fused kernel itself has to move
                rec["algorithmic_min_per_launch"] = p["work_min"]
                rec["frac_min"] = round(p["work_min"] / (ms * 1e-3) / 1e9 / 8000.0, 4)
            out.append(rec)
        return out

    def roofline_probe(self, idx, dense, y, iters=20):
        """The dominant kernel's roofline record (roofline_probe_all()[0])."""
        return self.roofline_probe_all(idx, dense, y, iters)[0]

    def optimizer_probe(self, idx, iters=10, more_ids=(), name="adam", side=None, lr=1e-3, **rules):
        """Times the separately-reported optimizer step on the gradients of the last fwd_bwd: the
        row-wise step on the touched table rows + the dense parameters in one launch; checks that two
        identical steps from the same state give bit-identical tables.  more_ids: further id batches -
        the timed steps then cycle through all of them (every step touches other rows, as in fit()).
        name / side / lr / rules: the optimizers' arguments (optim.SparseTableOptimizer: side, side_lr, ftrl_l1, ..);
        the default is Adam for every parameter."""
        from .optim import FusedDenseOptimizer, SparseTableOptimizer

        ids = [idx] + list(more_ids)
        sopt = SparseTableOptimizer(self, name, lr, side=side, **rules)
        dopt = FusedDenseOptimizer(self, name, lr, side=side, **rules)
        # determinism: the same step twice from the same state (rows + moments restored in between)
        mom = sopt.mom if sopt.mom is not None else self.rows.new_zeros(1)  # (an SGD embedding rule keeps none)
        rows0, mom0 = self.rows.clone(), mom.clone()
        sopt.step(idx)
        rows1, mom1 = self.rows.clone(), mom.clone()
        self.rows.copy_(rows0)
        mom.copy_(mom0)
        sopt.t = 0
        sopt.step(idx)
        same = bool(torch.equal(self.rows, rows1) and torch.equal(mom, mom1))
        del rows0, mom0, rows1, mom1
        iters = max(iters, 2 * len(ids))
        for i in range(3):
            sopt.step(ids[i % len(ids)])
            dopt.step()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        for i in range(iters):
            sopt.step(ids[i % len(ids)])
        ev[1].record()
        for _ in range(iters):
            dopt.step()
        ev[2].record()
        for i in range(iters):
            sopt.prepare(ids[i % len(ids)])
        ev[3].record()
        torch.cuda.synchronize()
        sopt._prepared = None
        ms_s, ms_d = ev[0].elapsed_time(ev[1]) / iters, ev[1].elapsed_time(ev[2]) / iters
        ms_p = ev[2].elapsed_time(ev[3]) / iters
        return {"ms": round(ms_s + ms_d, 4), "sparse_rows_ms": round(ms_s, 4), "dense_params_ms": round(ms_d, 4),
                "sort_ms": round(ms_p, 4), "apply_ms": round(ms_s - ms_p, 4),
                "bit_identical_rerun": same, "id_batches_rotated": len(ids),
                "rules": {"optimizer": name, "linear_optimizer": sopt.side},
                "dense_launches": len(dopt.ranges),
                "what": "row-wise lazy step on the touched table rows by the rules under `rules` "
                        "(rm_sparse_optimizer_step_rules: stable sort by row, duplicates summed in occurrence order, "
                        "no float atomics), then the step on the dense "
                        "parameters (rm_dense_optimizer_step_rule: one launch over the flat buffer, or "
                        "`dense_launches` of them around linear_w_dense when the wide part has a rule of its own), "
                        "timed back to back; sort_ms is the "
                        "id-only part (rm_sparse_optimizer_prepare) that fit() issues on a side stream beside "
                        "fwd+bwd; NOT part of value",
                "roofline": sopt.roofline(idx, ms_s)}

    def _embed_fwd_bytes(self, B, fm):
        F, D, Dn = self.F, self.D, self.Dn
        per = F * 8 + 2 * F * 4 * D  # idx read, rows read, E written
        if fm:
            per += F * 4 + 4 * D + 4  # bias entries, S written, fm_logit written
        if self.use_linear:
            per += F * 4 + Dn * 4 + 4  # linear entries, dense columns, lin_logit
        return B * per

    # ----------------------------------------------- dense views of the sparse grads
    def dense_grads(self, idx, reference_names=False):
        """Densifies the sparse gradients of the last fwd_bwd (scatter-add with float
        atomics) and adds the l2 terms: name -> tensor with the keys / shapes of self.params
        (or of state_dict() with reference_names=True).  What TF's IndexedSlices + dense l2
        gradient add up to (layers.py:188-193)."""
        hp, D = self.hp, self.D
        out = {k: v.clone() for k, v in self.grads.items()}
        R = self.spec.rows
        foff = self.field_off
        if self.mv_fields:
            # occurrences of multi-valued fields go to a dummy row R here; their gradient is
            # scattered to the tag rows below (rm_pool_rows_bwd)
            idx = idx.clone()
            foff = self.field_off.clone()
            for f in self.mv_fields:
                idx[:, f] = 0
                foff[f] = R
        d_table = torch.zeros(R + 1, D, dtype=F32, device=self.device)
        ops.scatter_add_rows(d_table, idx, foff, rows=self.d_rows)
        offs = self.spec.offsets()
        d_bias = None
        g_bias_occ = None
        if self.use_bias_tables:
            d_bias = torch.zeros(R + 1, dtype=F32, device=self.device)
            if self._has_fm():
                if self.d_bias is not None:
                    ops.scatter_add_rows(d_bias, idx, foff, rows=self.d_bias, width=1, ld=1)
                    g_bias_occ = self.d_bias
                else:
                    ops.scatter_add_rows(d_bias, idx, foff, g_row=self.dlogit)
        d_lin = torch.zeros(R + 1, dtype=F32, device=self.device)
        if self.use_linear:
            ops.scatter_add_rows(d_lin, idx, foff, g_row=self.dlogit)
        for f in self.mv_fields:
            if self.spec.sparse_names[f] in self.spec.seq_query:
                # history occurrences: their key-gradient rows go to the query feature's block (no bias / linear term)
                fq, ids, d_keys = self.seq_key_grads(f)
                if ids.numel():
                    ops.scatter_add_rows(d_table, ids.view(-1, 1), self.field_off[fq: fq + 1].contiguous(),
                                         rows=d_keys.view(-1, 1, D))
                continue
            offsets, ids, vals = self._mv_entry(f)
            gb = None
            if d_bias is not None and self._has_fm():
                gb = g_bias_occ[:, f].contiguous() if g_bias_occ is not None else self.dlogit
            ops.pool_rows_bwd(self.d_rows[:, f, :], gb, self.dlogit if self.use_linear else None, D,
                              offsets, ids, offs[f], d_table, d_bias if gb is not None else None,
                              d_lin if self.use_linear else None, vals=vals)
        d_table, d_lin = d_table[:R], d_lin[:R]
        if self.lin_field_mask is not None:  # linear_features subset
            for f, (off, V) in enumerate(zip(offs, self.spec.feat_sizes)):
                if self.spec.sparse_names[f] not in self.spec.linear_names:
                    d_lin[off: off + V] = 0
        if d_bias is not None:
            d_bias = d_bias[:R]
        reg = hp.get("embedding_l2_reg", 0.0)
        if reg:
            d_table.add_(self.rows[:, :D], alpha=reg)
        for name, off, V in zip(self.spec.sparse_names, offs, self.spec.feat_sizes):
            if name in self.spec.seq_query:
                continue
            out[f"{name}_feat_embed"] = d_table[off: off + V]
            if d_bias is not None:
                out[f"{name}_feat_bias"] = d_bias[off: off + V].view(V, 1)
        if self.use_linear:
            reg = hp.get("linear_l2_reg", 0.0)
            if reg:
                d_lin.add_(self.params["linear_w_sparse"], alpha=reg)
                out["linear_w_dense"] = out["linear_w_dense"] + reg * self.linear_w_dense
        else:
            out["linear_w0"] = torch.zeros_like(self.grads["linear_w0"])
            out["linear_w_dense"] = torch.zeros_like(self.grads["linear_w_dense"])
        out["linear_w_sparse"] = d_lin
        self._dense_grads_model(out)
        return self.to_reference_names(out) if reference_names else out

    def _dense_grads_model(self, out):
        pass

    def _has_fm(self):
        return False


# DeepFM's fwd_bwd through rm_deepfm_step (one kernel) where it applies; False = rm_embed_mlp_fwd + rm_mlp_bwd
STEP_FUSION_DEFAULT = True


class DeepFMEngine(Engine):
    """DeepFM._init_graph (DeepFM.py:107-158): final = linear + fm + dnn."""

    model = "deepfm"
    use_bias_tables = True
    shardable = True
    needs_fm_or_deep = True  # DeepFM.py:54; a subclass with a branch of its own over E may run without either

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, hp, task, device)
        self.use_fm = bool(hp.get("use_fm", True))
        self.use_deep = bool(hp.get("use_deep", True))
        assert self.use_fm or self.use_deep or not self.needs_fm_or_deep  # DeepFM.py:54
        if self.use_deep:
            self.mlp = self._dnn(self.FD, self.Dn, hp["deep_hidden_units"], "relu")
        # whether the one-kernel front / step take this engine's shapes (asked once), and the step's workspace
        self._front_ok = self._step_ok = self._step_ws = None

    def _model_masks(self, B, masks):
        fk = self.hp.get("fm_dropout")
        if fk is not None and any(k < 1 for k in fk):
            dev = self.device
            mb = (torch.rand(B, self.F, device=dev) < fk[0]).float() / fk[0] if fk[0] < 1 else None
            me = (torch.rand(B, self.F, self.D, device=dev) < fk[1]).float() / fk[1] if fk[1] < 1 else None
            masks["fm"] = (mb, me)

    def _has_fm(self):
        return self.use_fm

    def _front_fused(self, m, lin_w):
        """The one-kernel front (rm_embed_mlp_fwd: gather + FM + linear + MLP + head) covers this call:
        plain id features on the fused-row table, a skinny MLP, no dropout masks."""
        hp = self.hp
        if not (self.use_deep and self.use_linear and hp.get("front_fusion", True)) or self.mv_fields:
            return False
        if lin_w is not None or m.get("dnn") is not None or any(x is not None for x in m.get("fm", (None, None))):
            return False
        if self._front_ok is None:
            self._front_ok = bool(self.mlp.fused_ok and ops.embed_mlp_fwd_supported(
                self.F, self.D, self._front_ld(), self.Dn, self.mlp.hidden))
        return self._front_ok

    def _front_ld(self):
        return self.LD

    def _front_table(self, idx):
        """(ids, rows, field offsets, row stride, non-temporal row loads) the one-kernel front gathers from."""
        return idx, self.rows, self.field_off, self.LD, self.hp.get("table_row_reuse", "stream") == "stream"

    def _front_fwd(self, idx, dense, branches):
        mlp, p = self.mlp, self.params
        B, n = idx.shape[0], len(self.mlp.hidden)
        mlp._alloc(B, idx.device)
        mlp.keep, mlp.masks = [1] * (n + 1), [None] * (n + 1)
        mlp.xe, mlp.xd, mlp.fused = self.E.view(-1, self.FD), (dense if self.Dn else None), True
        req = self._head_req if self.fuse_head else None
        head = dict(req, branches=branches, coef_mlp=1.0) if req is not None else None
        mlp.tail = ops.mlp_tail(B, dh=mlp.dhb, **head) if head is not None else None
        mlp.head_done = head is not None
        ids, rows, foff, ld, stream_rows = self._front_table(idx)
        ops.embed_mlp_fwd(
            ids, rows, foff, self.D, ld, dense if self.Dn else None, *mlp.vars(p), mlp.act, self.E, mlp.hb,
            mlp.out.view(B),
            want_bias=self.use_fm and self.use_bias_tables, want_lin=True,
            lin_w_dense=self.linear_w_dense if self.Dn else None, lin_w0=p["linear_w0"],
            fm_sum=self.fm_sum if self.use_fm else None, fm_logit=self.fm_logit if self.use_fm else None,
            lin_logit=self.lin_logit, stream_rows=stream_rows, tail=mlp.tail)
        self._head_done = mlp.head_done
        return mlp.out.view(B)

    # ---- the whole step in one kernel (rm_deepfm_step)
    step_fusable = True  # the row-sharded subclass keeps its own fwd_bwd (recman_amd/dist.py)

    def _step_fused(self, masks, mv):
        """rm_deepfm_step covers this call: everything _front_fused asks for, plus FM + bias tables on, two
        hidden layers, no dropout masks.  hp["step_fusion"] overrides STEP_FUSION_DEFAULT."""
        if not (self.step_fusable and self.hp.get("step_fusion", STEP_FUSION_DEFAULT)) or masks or mv is not None:
            return False
        if self.rank is not None:  # (the step kernel's head is the pointwise loss alone)
            return False
        if not (self.use_fm and self.use_bias_tables and self._front_fused({}, None)):
            return False
        if self._step_ok is None:
            self._step_ok = bool(ops.deepfm_step_supported(self.F, self.D, self.LD, self.Dn, self.mlp.hidden))
        return self._step_ok

    def _step_call(self, idx, dense, y, skip_finish=False):
        mlp, p, g = self.mlp, self.params, self.grads
        if self._step_ws is None:
            self._step_ws = torch.zeros(ops.deepfm_step_workspace(self.F, self.Dn), dtype=F32, device=self.device)
        ops.deepfm_step(
            idx, self.rows, self.field_off, self.D, self.LD, dense if self.Dn else None, y,
            *mlp.vars(p), self.linear_w_dense if self.Dn else None, p["linear_w0"],
            mlp.act, self.task, self.d_rows, self.logit, self.pred, self.dlogit, self.loss,
            *mlp.vars(g), g["linear_w_dense"] if self.Dn else None, g["linear_w0"],
            self._step_ws, grad_scale=self.grad_scale,
            # (plain row loads unless asked otherwise: the reason for streaming them - keeping E in the caches for the
            # MLP kernels - is gone with E; measured 97 vs 102 us per step, uniform ids)
            stream_rows=self.hp.get("step_row_loads", "cache") == "stream",
            stream_d_rows=self.hp.get("d_rows_reuse", "cache") == "stream", skip_finish=skip_finish)

    def fwd_bwd(self, idx, dense, y, masks=None, mv=None):
        B = idx.shape[0]
        self._alloc(B)
        if not self._step_fused(masks, mv):
            return super().fwd_bwd(idx, dense, y, masks=masks, mv=mv)
        self._mv = None
        self._step_call(idx, dense, y)
        self.d_bias = None
        self._head_done = self._lin_done = True
        g = self.grads
        if self.Dn and self.lin_dense_mask is not None:
            g["linear_w_dense"].mul_(self.lin_dense_mask)  # linear_features subset
        self._add_l2_grads()
        return self._add_l2(self.loss)

    def roofline_probes(self, idx, dense, y):
        probes = super().roofline_probes(idx, dense, y)
        self._alloc(idx.shape[0])
        if self._step_fused(None, None):
            # the step's dominant (only large) kernel.  Algorithmic bytes: SURVEY.md 8d's embed+FM forward AND
            # backward figure, 8,952 B per example at F = 26, D = 16 (idx, rows, E, S, g, dE, gradient rows) - the
            # path this kernel replaces end to end; `work_min` = what the fused kernel itself has to move (ids, 72
            # useful bytes per looked-up row, dense inputs, labels in; row gradients, logit / pred / dlogit out)
            B, F, D, Dn = idx.shape[0], self.F, self.D, self.Dn
            fwd = B * F * (8 + 4 * D + 4) + B * 4 + B * F * 4 * D
            bwd = B * F * (8 + 4 * D + 4 * D + 4 * D + 4) + B * 4
            work_min = B * (F * (8 + 4 * D + 8) + 4 * Dn + y.element_size() + F * 4 * D + 3 * 4)
            step = [dict(name="deepfm_step_kernel (rm_deepfm_step: gather + FM + linear + MLP + loss + every gradient)",
                         symbol="deepfm_step_kernel", fn=lambda: self._step_call(idx, dense, y, skip_finish=True),
                         work=fwd + bwd, work_min=work_min, bound="hbm")]
            return step + probes
        if not self._front_fused({}, None):
            return probes
        # the step's dominant kernel is the one-kernel front; its algorithmic bytes = rm_embed_fwd's
        #  + what the MLP and the head move per example on top of x: the dense columns when
        # the linear term has not already counted them, h_l written, dh_l written, the label, logit /
        # pred / dlogit written (E is NOT read back: that is the point of the fusion)
        B, n = idx.shape[0], len(self.mlp.hidden)
        yk = dict(y=y) if y.dtype == I64 else dict(y_f=y)

        def run():
            self._head_req = dict(task=self.task, grad_scale=1.0, logit=self.logit, pred=self.pred,
                                  dlogit=self.dlogit, loss_partial=self.loss_part, loss=self.loss, **yk)
            try:
                branches = [(self.lin_logit, 1.0)] + ([(self.fm_logit, 1.0)] if self.use_fm else [])
                self._front_fwd(idx, dense, branches)
            finally:
                self._head_req = None

        work = self._embed_fwd_bytes(B, self._has_fm()) + B * (2 * n * 32 * 4 + y.element_size() + 4 * 4)
        return [dict(name="embed_mlp_fwd_kernel (rm_embed_mlp_fwd: gather + FM + linear + MLP + head)",
                     symbol="embed_mlp_fwd_kernel", fn=run, work=work, bound="hbm")] + probes

    def _branches_fwd(self, idx, dense, training, masks, lin_w):
        m = masks or {}
        if not training:
            m = {}
        if self._front_fused(m, lin_w):
            branches = [(self.lin_logit, 1.0)]
            if self.use_fm:
                branches.append((self.fm_logit, 1.0))
            self.dnn_logit = self._front_fwd(idx, dense, list(branches))
            branches.append((self.dnn_logit, 1.0))
            return branches
        self._embed(idx, dense, self.use_fm, m, lin_w)
        branches = [(self.lin_logit, 1.0)]
        if self.use_fm:
            branches.append((self.fm_logit, 1.0))
        if self.use_deep:
            self.dnn_logit = self._mlp_last(self.mlp, self.E.view(-1, self.FD), dense if self.Dn else None,
                                            self._dnn_keep(training), m.get("dnn"), list(branches))
            branches.append((self.dnn_logit, 1.0))
        return branches

    def _branches_bwd(self, idx, dense, g, masks):
        m = masks or {}
        fm_masks = m.get("fm", (None, None))
        dE_up = None
        fm_done = False
        self.d_bias = None
        if self.use_deep:
            # fused path: the FM gradient g*(S - E) rides along in the MLP backward
            fuse_fm = self.use_fm and fm_masks[0] is None and fm_masks[1] is None
            fm_done = self.mlp.backward(g, self.d_rows.view(-1, self.FD),
                                        fm_sum=self.fm_sum if fuse_fm else None,
                                        lin_grads=self._lin_grads())
            self._lin_done = self.mlp.lin_done
            dE_up = self.d_rows
        if self.use_fm and fm_masks[0] is not None:
            self.d_bias = torch.empty(idx.shape[0], self.F, dtype=F32, device=self.device)
        if self.use_fm and not fm_done:
            ops.embed_bwd(self.d_rows, E=self.E, fm_sum=self.fm_sum, dE_up=dE_up, g_fm=g,
                          mask_b=fm_masks[0], mask_e=fm_masks[1], d_bias=self.d_bias)


class CrossMix:
    """The DCN-Mix cross stack (DCN-V2, arXiv 2008.13535 eq. 4-5) with an explicit backward, on the variables
    {prefix}cross_v [L,d,E r], cross_gate [L,d,E], cross_c [L,E,r,r], cross_u [L,d,E r], cross_b [L,d], cross_w_out
    [d,1] of a params / grads pair: per layer a projection GEMM x_l -> [t | s] over a packed copy of V_l | G_l
    (refreshed from the variables every forward, on the device), the fused core (csrc/cross_mix.hip) and the output
    GEMM m U_l^T with the cross update in its epilogue (RM_DENSE_CROSS).  The GEMMs run on the f32 MFMA kernels, as
    the matrix form's do.  Every buffer is sized once per batch size (alloc): no allocation inside a step."""

    def __init__(self, params, grads, FD, Dn, L, E, r, device, prefix=""):
        self.p, self.g, self.prefix = params, grads, prefix
        self.FD, self.Dn, self.d, self.L, self.E, self.r, self.device = FD, Dn, FD + Dn, L, E, r, device
        self._B = None

    def alloc(self, B):
        if self._B == B:
            return
        self._B = B
        dev, L, d, E, r = self.device, self.L, self.d, self.E, self.r
        W, N = E * r, E * r + E
        dp, ldp = (d + 3) // 4 * 4, (N + 3) // 4 * 4
        z = lambda cols: torch.zeros(B, cols, dtype=F32, device=dev)  # noqa: E731
        self.logit = torch.empty(B, dtype=F32, device=dev)
        # rows padded to a multiple of 4 floats (16-byte rows for the GEMM loaders); the pad columns stay zero
        self.cx = [z(dp) for _ in range(L + 1)]   # x_0 .. x_L
        self.cu = [z(dp) for _ in range(L)]       # u_l = m_l U_l^T + b_l
        self.cts = [z(ldp) for _ in range(L)]     # [t_l | s_l] = x_l [V_l | G_l]: one projection buffer
        self.cm = [z(W) for _ in range(L)]        # m_l
        self.cg = [z(dp), z(dp)]                  # dLoss/dx_l, ping-pong
        self.cdu, self.cdx0 = z(dp), z(dp)        # dLoss/du_l, dLoss/dx0
        self.cdm, self.cdts = z(W), z(ldp)        # dLoss/dm_l, [dt_l | ds_l]
        self.cvg = torch.zeros(L, d, N, dtype=F32, device=dev)   # [V_l | G_l]
        self.cdvg = torch.zeros(d, N, dtype=F32, device=dev)     # its gradient, one layer at a time
        self.cdut = torch.zeros(W, d, dtype=F32, device=dev)     # dU_l^T
        self.w_out_p = torch.zeros(dp, dtype=F32, device=dev)
        fw = max(ops.dense_filter_workspace(k, n) for k, n in ((d, N), (W, d), (d, W), (N, d)))
        ww = max(ops.dense_wgrad_workspace(k, n, B) for k, n in ((W, d), (d, N), (d, 1)))
        self._fws = torch.empty(fw, dtype=F32, device=dev)
        self._wws = torch.empty(max(1, ww), dtype=F32, device=dev)
        self._core_ws = torch.empty(max(1, ops.cross_mix_bwd_workspace(B, E, r)), dtype=F32, device=dev)

    def _vars(self, d):
        return {n: d[self.prefix + "cross_" + n] for n in ("v", "gate", "c", "u", "b", "w_out")}

    def forward(self, xe, xd):
        """x0 = [xe | xd] -> self.logit [B] (the cross logit)."""
        p, d, W, N = self._vars(self.p), self.d, self.E * self.r, self.E * self.r + self.E
        self.alloc(xe.shape[0])
        x0 = self.cx[0]
        x0[:, : self.FD].copy_(xe)
        if self.Dn:
            x0[:, self.FD: d].copy_(xd)
        self.cvg[:, :, :W].copy_(p["v"])
        self.cvg[:, :, W:].copy_(p["gate"])
        for l in range(self.L):
            ts = self.cts[l]
            ops.dense_fwd(self.cx[l][:, :d], None, self.cvg[l], ts[:, :N], self._fws)
            ops.cross_mix_fwd(ts[:, :W], ts[:, W:N], p["c"][l], self.cm[l])
            ops.dense_fwd(self.cm[l], None, p["u"][l], self.cx[l + 1][:, :d], self._fws,
                          transposed=True, bias=p["b"][l], epilogue=ops.DENSE_CROSS,
                          aux1=x0[:, :d], aux2=self.cx[l][:, :d], out2=self.cu[l][:, :d])
        self.w_out_p[:d].copy_(p["w_out"].view(-1))
        ops.rowdot(self.cx[self.L], self.w_out_p, None, self.logit)
        return self.logit

    def backward(self, g):
        """g [B] = dLoss/dlogit -> the six variables' gradients (overwritten) and self.cdx0[:, :d] = dLoss/dx0."""
        p, gr, d, L, W, N = self._vars(self.p), self._vars(self.g), self.d, self.L, self.E * self.r, self.E * self.r + self.E
        x0 = self.cx[0]
        ops.dense_wgrad(self.cx[L][:, :d], None, g.view(-1, 1), gr["w_out"], self._wws)  # x_L^T g
        gc, gn = self.cg
        torch.mul(g.view(-1, 1), self.w_out_p.view(1, -1), out=gc)  # dLoss/dx_L
        self.cdx0.zero_()
        for l in range(L - 1, -1, -1):
            ts, dts = self.cts[l], self.cdts
            torch.mul(gc, x0, out=self.cdu)                 # dLoss/du_l = g_{l+1} o x0
            self.cdx0.addcmul_(gc, self.cu[l])              # dLoss/dx0 += g_{l+1} o u_l
            # dU_l^T = m_l^T du_l, and db_l = the column sums of du_l from the same pass
            ops.dense_wgrad(self.cm[l], None, self.cdu[:, :d], self.cdut, self._wws, db=gr["b"][l])
            gr["u"][l].copy_(self.cdut.t())
            ops.dense_fwd(self.cdu[:, :d], None, p["u"][l], self.cdm, self._fws)  # dLoss/dm_l = du_l U_l
            ops.cross_mix_bwd(ts[:, :W], ts[:, W:N], p["c"][l], self.cdm, dts[:, :W], dts[:, W:N], gr["c"][l],
                              self._core_ws)
            ops.dense_wgrad(self.cx[l][:, :d], None, dts[:, :N], self.cdvg, self._wws)  # x_l^T [dt | ds]
            gr["v"][l].copy_(self.cdvg[:, :W])
            gr["gate"][l].copy_(self.cdvg[:, W:])
            # dLoss/dx_l = [dt | ds] [V_l | G_l]^T + g_{l+1}
            ops.dense_fwd(dts[:, :N], None, self.cvg[l], gn[:, :d], self._fws, transposed=True,
                          epilogue=ops.DENSE_ADD, aux1=gc[:, :d])
            gc, gn = gn, gc
        self.cdx0.add_(gc)


class DCNEngine(Engine):
    """DCN._init_graph (DCN.py:99-144): dnn_input feeds the DNN and the CrossNet;
    final = dnn + cross (+ dnn again under strict_reference, DCN.py:140-142)
    (+ linear if use_linear).  CrossNet is absent from the reference (DCN.py:7):
    cross_type "vector" = DCN-v1, x_{l+1} = x0 (x_l . w_l) + b_l + x_l, all layers fused in
    csrc/cross.hip; cross_type "matrix" = x_{l+1} = x0 o (W_l x_l + b_l) + x_l, one f32-MFMA
    GEMM per layer with the cross update as its epilogue (csrc/gemm.hip, RM_DENSE_CROSS);
    cross_type "mix" = DCN-Mix (DCN-V2, arXiv 2008.13535 eq. 4-5), cross_experts low-rank experts of rank
    cross_low_rank per layer under a per-layer softmax gate: x_{l+1} = x0 o (m U_l^T + b_l) + x_l with
    m = [p_i tanh(tanh(x_l V_l,i) C_l,i)]_i, p = softmax(x_l G_l) - two skinny GEMMs per layer around the fused
    core of csrc/cross_mix.hip."""

    model = "dcn"
    use_bias_tables = False
    shardable = True

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, hp, task, device)
        self.use_linear = bool(hp.get("use_linear", True))
        self.L = int(hp.get("cross_layer_num", 3))
        self.dnn_coef = 2.0 if hp.get("strict_reference", False) else 1.0
        d = self.FD + self.Dn
        self.mlp = self._dnn(self.FD, self.Dn, hp["deep_hidden_units"], "relu")
        self.cross_type = hp.get("cross_type", "vector")
        if self.cross_type not in ("vector", "matrix", "mix"):
            raise ValueError(f"cross_type {self.cross_type!r}: 'vector', 'matrix' or 'mix'")
        self.matrix = self.cross_type == "matrix"
        self.mix = self.cross_type == "mix"
        # (absent from the reference: glorot-normal weights, zero biases)
        if self.mix:
            E, r = int(hp.get("cross_experts", 4)), int(hp.get("cross_low_rank", 32))
            if not ops.cross_mix_supported(E, r):
                raise ValueError(f"cross_type 'mix': cross_experts={E}, cross_low_rank={r} is not supported "
                                 "(1 <= cross_experts <= 8, cross_low_rank in 8, 16, 32, 64, their product <= 256)")
            self.mix_E, self.mix_r = E, r
            l2 = "cross_layer_l2_reg"
            self._var("cross_v", (self.L, d, E * r), ("glorot", d, r), l2)
            self._var("cross_gate", (self.L, d, E), ("glorot", d, E), l2)
            self._var("cross_c", (self.L, E, r, r), ("glorot", r, r), l2)
            self._var("cross_u", (self.L, d, E * r), ("glorot", r, d), l2)
            self.cmix = CrossMix(self.params, self.grads, self.FD, self.Dn, self.L, E, r, self.device)
        else:
            self._var("cross_w", (self.L, d, d) if self.matrix else (self.L, d),
                      ("glorot", d, d if self.matrix else 1), "cross_layer_l2_reg")
        self._var("cross_b", (self.L, d))
        self._var("cross_w_out", (d, 1), ("glorot", d, 1), "cross_layer_l2_reg")

    def _alloc_model(self, B):
        dev = self.device
        L = self.L
        if self.mix:
            self.dxe_dnn = torch.empty(B, self.FD, dtype=F32, device=dev)
            self.cmix.alloc(B)
            return
        self.cross_logit = torch.empty(B, dtype=F32, device=dev)
        self.cross_p = torch.empty(B, ops.cross_p_ld(L), dtype=F32, device=dev)  # x0.w_l, x0.w_out
        self.coef = torch.empty(B, 2 * L + 2, dtype=F32, device=dev)
        self._coef_sum = torch.empty(2 * L + 2, dtype=F32, device=dev)
        self._ones_b = torch.ones(B, dtype=F32, device=dev)
        self._cross_wws = torch.empty(max(1, ops.dense_wgrad_workspace(self.FD + self.Dn, L + 1, B)),
                                      dtype=F32, device=dev)
        self.P = torch.empty(self.FD + self.Dn, L + 1, dtype=F32, device=dev)
        self.dxe_dnn = torch.empty(B, self.FD, dtype=F32, device=dev)
        if self.matrix:
            # activations of the matrix cross: rows padded to a multiple of 4 floats (16-byte rows
            # for the GEMM loaders); the pad columns stay zero
            d = self.FD + self.Dn
            dp = (d + 3) // 4 * 4
            z = lambda: torch.zeros(B, dp, dtype=F32, device=dev)  # noqa: E731
            self.cx = [z() for _ in range(L + 1)]   # x_0 .. x_L
            self.cu = [z() for _ in range(L)]       # u_l = W_l x_l + b_l
            self.cg = [z(), z()]                    # dLoss/dx_l, ping-pong
            self.cdu, self.cdx0 = z(), z()
            self.w_out_p = torch.zeros(dp, dtype=F32, device=dev)
            self._dcol = torch.empty(dp, dtype=F32, device=dev)
            self._cfws = torch.empty(ops.dense_filter_workspace(d, d), dtype=F32, device=dev)
            self._cwws = torch.empty(max(1, ops.dense_wgrad_workspace(d, d, B)), dtype=F32, device=dev)

    # ---- matrix cross (DCN-v2 form): one GEMM per layer, cross update in the epilogue ----
    def _cross_matrix_fwd(self, xe, xd):
        p, d = self.params, self.FD + self.Dn
        x0 = self.cx[0]
        x0[:, : self.FD].copy_(xe)
        if self.Dn:
            x0[:, self.FD: d].copy_(xd)
        for l in range(self.L):
            ops.dense_fwd(self.cx[l][:, :d], None, p["cross_w"][l], self.cx[l + 1][:, :d], self._cfws,
                          transposed=True, bias=p["cross_b"][l], epilogue=ops.DENSE_CROSS,
                          aux1=x0[:, :d], aux2=self.cx[l][:, :d], out2=self.cu[l][:, :d])
        self.w_out_p[:d].copy_(p["cross_w_out"].view(-1))
        ops.rowdot(self.cx[self.L], self.w_out_p, None, self.cross_logit)

    def _cross_matrix_bwd(self, g):
        p, gr, d, L = self.params, self.grads, self.FD + self.Dn, self.L
        x0 = self.cx[0]
        ops.linear_dense_bwd(g, self.cx[L], self._dcol, None, self.ws)  # d_w_out = x_L^T g
        gr["cross_w_out"].view(-1).copy_(self._dcol[:d])
        gc, gn = self.cg
        torch.mul(g.view(-1, 1), self.w_out_p.view(1, -1), out=gc)  # dLoss/dx_L
        self.cdx0.zero_()
        for l in range(L - 1, -1, -1):
            torch.mul(gc, x0, out=self.cdu)                 # dLoss/du_l = g_{l+1} o x0
            self.cdx0.addcmul_(gc, self.cu[l])              # dLoss/dx0 += g_{l+1} o u_l
            ops.dense_wgrad(self.cdu[:, :d], None, self.cx[l][:, :d], gr["cross_w"][l], self._cwws)
            ops.linear_dense_bwd(self._ones_b, self.cdu, self._dcol, None, self.ws)
            gr["cross_b"][l].copy_(self._dcol[:d])
            # dLoss/dx_l = du_l W_l + g_{l+1}
            ops.dense_fwd(self.cdu[:, :d], None, p["cross_w"][l], gn[:, :d], self._cfws,
                          epilogue=ops.DENSE_ADD, aux1=gc[:, :d])
            gc, gn = gn, gc
        self.cdx0.add_(gc)
        torch.add(self.cdx0[:, : self.FD], self.dxe_dnn, out=self.d_rows.view(-1, self.FD))

    def _branches_fwd(self, idx, dense, training, masks, lin_w):
        m = self._embed_plain(idx, dense, training, masks, lin_w)
        xe, xd = self.E.view(-1, self.FD), (dense if self.Dn else None)
        self.dnn_logit = self.mlp.forward(xe, xd, self._dnn_keep(training), m.get("dnn"))
        p = self.params
        if self.mix:
            self.cross_logit = self.cmix.forward(xe, xd)
        elif self.matrix:
            self._cross_matrix_fwd(xe, xd)
        else:
            ops.cross_fwd(xe, xd, p["cross_w"], p["cross_b"], p["cross_w_out"].view(-1),
                          self.cross_logit, self.cross_p)
        branches = [(self.dnn_logit, self.dnn_coef), (self.cross_logit, 1.0)]
        if self.use_linear:
            branches.append((self.lin_logit, 1.0))
        return branches

    def _branches_bwd(self, idx, dense, g, masks):
        p, gr = self.params, self.grads
        xe, xd = self.E.view(-1, self.FD), (dense if self.Dn else None)
        g_dnn = g if self.dnn_coef == 1.0 else g * self.dnn_coef
        L = self.L
        # the first dense layer's dW = x0^T dA0 and the cross net's P = x0^T coef read the same x0: one pass
        # (rm_dense_wgrad6 with a second piece of gradient columns) once both operands exist
        fold = (not self.matrix and not self.mix and L + 1 <= 16 and self.mlp.can_defer_wgrad0()
                and self.hp.get("dcn_fold_cross_wgrad", True))
        self.mlp.backward(g_dnn, self.dxe_dnn, defer_wgrad0=fold)
        if self.mix:
            self.cmix.backward(g)
            torch.add(self.cmix.cdx0[:, : self.FD], self.dxe_dnn, out=self.d_rows.view(-1, self.FD))
            return
        if self.matrix:
            self._cross_matrix_bwd(g)
            return
        # cross backward adds the DNN's dx and writes straight into the row-gradient
        # buffer: with no FM term d_rows IS dLoss/dE (no separate embed_bwd launch)
        ops.cross_bwd(p["cross_w"], p["cross_b"], p["cross_w_out"].view(-1), g,
                      self.cross_p, self.d_rows.view(-1, self.FD), self.coef, dx_in_e=self.dxe_dnn)
        # P = x0^T coef[:, :L+1]: a batch-reduction GEMM with x0 = [xe | xd] read in place, and the
        # column sums of coef in one pass (rm_linear_dense_bwd with unit weights)
        if fold:
            self.mlp.wgrad0(G2=self.coef[:, : L + 1], dW2=self.P)
        else:
            ops.dense_wgrad(xe, xd if self.Dn else None, self.coef[:, : L + 1], self.P, self._cross_wws)
        ops.linear_dense_bwd(self._ones_b, self.coef, self._coef_sum, None, self.ws)
        colsum = self._coef_sum[L + 1:]
        ops.cross_param_grads(self.P, colsum, p["cross_w"], p["cross_b"],
                              p["cross_w_out"].view(-1), gr["cross_w"], gr["cross_b"],
                              gr["cross_w_out"].view(-1))

    def roofline_probes(self, idx, dense, y):
        # the MLP GEMMs dominate the DCN step: layer 0 of the wide DNN, x = [xe | xd] -> H0 (bias +
        # activation fused), on the f32 MFMA roofline; the fused cross kernels on the HBM roofline
        if self.mlp.fused_ok:
            return super().roofline_probes(idx, dense, y)
        B = idx.shape[0]
        self._probe_fill(idx, dense, y)  # E, the layer scalars s, dlogit, dxe_dnn
        xe, xd = self.E.view(-1, self.FD), (dense if self.Dn else None)
        W, b = self.params["dnn_layer_0_weights"], self.params["dnn_layer_0_bias"]
        m, p, L, d = self.mlp, self.params, self.L, self.FD + self.Dn
        K, N = W.shape
        m._alloc_dense(xe.device)
        if m._fws6 is not None and ops.dense_fwd6_supported(xe, xd):
            # the product path: fp32 operands split into three bf16 pieces, SIX bf16 MFMAs per k-step (csrc/gemm6.hip)
            # - priced on the bf16 pipe with the six products counted; the fp32 GEMM it stands for beside it
            flops = 2.0 * B * K * N
            probes = [dict(name=f"dense_nn6_kernel (rm_dense_fwd6, DNN layer 0: [{B},{K}] x [{K},{N}] + bias + {m.act}; "
                                "fp32 operands as 3 bf16 pieces, 6 piece products per k-step on the bf16 matrix pipe)",
                           symbol="dense_nn6_kernel",
                           fn=lambda: ops.dense_fwd(xe, xd, W, m.a[0], m._fws, bias=b, act=m.act, ws6=m._fws6),
                           work=6.0 * flops, bound="mfma", peak=2500.0,
                           extra=lambda ms: {"fp32_gemm_tflops": round(flops / (ms * 1e-3) / 1e12, 2),
                                             "fp32_gemm_vs_f32_mfma_peak_157": round(flops / (ms * 1e-3) / 1e12 / 157.3, 4),
                                             "note": "peak = dense bf16 MFMA (2.5 PFLOP/s); achieved counts the six "
                                                     "bf16 products per fp32 product; fp32_gemm_tflops = 2 M K N / time"})]
        else:
            probes = [dict(name=f"dense_nn_kernel (rm_dense_fwd, DNN layer 0: [{B},{K}] x [{K},{N}] + bias + {m.act})",
                           symbol="dense_nn_kernel",
                           fn=lambda: ops.dense_fwd(xe, xd, W, m.a[0], m._fws, bias=b, act=m.act),
                           work=2.0 * B * K * N, bound="mfma")]
        if not self.matrix and not self.mix:
            probes.append(dict(
                name=f"cross_fwd_kernel (rm_cross_fwd, {L} layers fused: x0 [{B},{d}] read once -> logit, p)",
                symbol="cross_fwd_kernel",
                fn=lambda: ops.cross_fwd(xe, xd, p["cross_w"], p["cross_b"], p["cross_w_out"].view(-1),
                                         self.cross_logit, self.cross_p),
                work=B * (d * 4 + 4 + 4 * (L + 1)), bound="hbm"))
            probes.append(dict(
                name="cross_bwd_kernel (rm_cross_bwd: the DNN's dx [B,FD] + the p row read, dx0 written once)",
                symbol="cross_bwd_kernel",
                fn=lambda: ops.cross_bwd(p["cross_w"], p["cross_b"], p["cross_w_out"].view(-1),
                                         self.dlogit, self.cross_p, self.d_rows.view(-1, self.FD),
                                         self.coef, dx_in_e=self.dxe_dnn),
                work=B * (2 * self.FD * 4 + 4 * (2 * L + 2) + 4 * (L + 1) + 4), bound="hbm"))
        return probes


class XDeepFMEngine(Engine):
    """xDeepFM._out (xDeepFM.py:47-104): embeddings without bias tables,
    final = linear + cin + dnn.  CIN (layers.py:697-760) runs on the f32 MFMA, one
    kernel per layer forward, three MFMA passes per layer backward (csrc/cin.hip)."""

    model = "xdeepfm"
    use_bias_tables = False
    shardable = True

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, hp, task, device)
        self.units = [int(u) for u in hp["cin_cross_layer_units"]]
        assert len(self.units) > 0  # layers.py:656
        self.cin_act = act_name(hp.get("cin_activation", "leaky_relu"))
        keep = hp.get("cin_dropout")
        if keep is not None and any(k < 1 for k in keep):
            assert len(keep) == len(self.units) + 1  # layers.py:657 (checked only when it matters)
        self.mlp = self._dnn(self.FD, self.Dn, hp["deep_hidden_units"], "leaky_relu")
        self._cin_drop = None  # (keep, masks, which layers) of the last forward's cin_dropout
        m = self.F
        self.Hs, self.pool_from, self.pool_col0 = [m], [], []
        final = 0
        for i, size in enumerate(self.units):
            last = i == len(self.units) - 1
            if not last and size % 2:
                raise ValueError("CIN layer sizes before the last must be even (split in halves, layers.py:742-746)")
            H = self.Hs[-1]
            self._var(f"cin_filter_{i}", (1, m * H, size), ("glorot", m * H, size), "cin_l2_reg")
            self._var(f"cin_bias_{i}", (size,))
            self.pool_from.append(0 if last else size // 2)
            self.pool_col0.append(final)
            final += size if last else size // 2
            self.Hs.append(size // 2)
        self.P = final
        self._var("cin_w", (final, 1), ("glorot_uniform", final, 1), "cin_l2_reg")
        self._var("cin_w0", (1,))

    def _model_masks(self, B, masks):
        ck = self.hp.get("cin_dropout")
        if ck is not None and any(k < 1 for k in ck):
            shapes = [(B, self.F, self.D)] + [(B, n, self.D) for n in self.units]
            masks["cin"] = [(torch.rand(*sh, device=self.device) < k).float() if k < 1 else None
                            for sh, k in zip(shapes, ck)]

    def _alloc_model(self, B):
        dev, m, D = self.device, self.F, self.D
        self.maps = [torch.empty(B, n, D, dtype=F32, device=dev) for n in self.units]
        self.dxk = [None] + [torch.empty(B, self.Hs[i], D, dtype=F32, device=dev)
                             for i in range(1, len(self.units))]
        self.pooled = torch.empty(B, self.P, dtype=F32, device=dev)
        self.cin_logit = torch.empty(B, dtype=F32, device=dev)
        fw = max(ops.cin_filter_workspace(m, self.Hs[i], n) for i, n in enumerate(self.units))
        bw = max(ops.cin_bwd_workspace(B, m, self.Hs[i], n, D) for i, n in enumerate(self.units))
        self.cin_fws = torch.empty(fw, dtype=F32, device=dev)
        self.cin_bws = torch.empty(bw, dtype=F32, device=dev)
        # the layers rm_cin_layer_fwd6 covers run on the bf16 matrix pipe with split fp32 operands (csrc/cin6.hip)
        # unless cin_gemm = "f32"
        self.cin_fws6 = None
        if self.hp.get("cin_gemm", "bf16x6") == "bf16x6":
            f6 = max(ops.cin_filter_workspace6(m, self.Hs[i], n, D) for i, n in enumerate(self.units))
            if f6 > 0:
                self.cin_fws6 = torch.empty(f6, dtype=F32, device=dev)

    def _cin_fwd(self, keep=None, masks=None):
        """CIN.__call__ (layers.py:697-760).  keep / masks: the L+1 keep probabilities and 0/1
        masks of cin_dropout (input E, then every layer's maps, layers.py:708,740); a dropped
        layer is scaled in place after its kernel and its pooled columns are re-summed."""
        p = self.params
        L = len(self.units)
        on = [bool(keep is not None and masks is not None and keep[i] < 1 and masks[i] is not None)
              for i in range(L + 1)]
        self._cin_drop = (keep, masks, on) if any(on) else None
        X0 = self.E
        if on[0]:
            self.E_cin = self.E * (masks[0] / keep[0])
            X0 = self.E_cin
        self._cin_x0 = X0
        xk = X0
        for i, n in enumerate(self.units):
            ops.cin_layer_fwd(X0, xk, self.Hs[i], p[f"cin_filter_{i}"][0], p[f"cin_bias_{i}"],
                              self.cin_act, self.maps[i], self.cin_fws,
                              pooled=None if on[i + 1] else self.pooled,
                              pool_col0=self.pool_col0[i], pool_from=self.pool_from[i], ws6=self.cin_fws6,
                              first6=self.hp.get("cin_first_layer", "bf16x6") == "bf16x6")
            if on[i + 1]:
                pf, c0 = self.pool_from[i], self.pool_col0[i]
                self.maps[i].mul_(masks[i + 1] / keep[i + 1])
                torch.sum(self.maps[i][:, pf:, :], dim=2, out=self.pooled[:, c0: c0 + n - pf])
            xk = self.maps[i]
        ops.rowdot(self.pooled, p["cin_w"].view(-1), p["cin_w0"], self.cin_logit)

    def _branches_fwd(self, idx, dense, training, masks, lin_w):
        hp = self.hp
        m = self._embed_plain(idx, dense, training, masks, lin_w)
        ck = list(hp.get("cin_dropout") or []) if training else []
        self._cin_fwd(ck if ck and any(k < 1 for k in ck) else None, m.get("cin"))
        self.dnn_logit = self._mlp_last(self.mlp, self.E.view(-1, self.FD), dense if self.Dn else None,
                                        self._dnn_keep(training), m.get("dnn"),
                                        [(self.lin_logit, 1.0), (self.cin_logit, 1.0)])
        return [(self.lin_logit, 1.0), (self.cin_logit, 1.0), (self.dnn_logit, 1.0)]

    def _branches_bwd(self, idx, dense, g, masks):
        p, gr = self.params, self.grads
        # DNN first: it STORES dLoss/dE into d_rows; every CIN layer then accumulates
        self.mlp.backward(g, self.d_rows.view(-1, self.FD), lin_grads=self._lin_grads())
        self._lin_done = self.mlp.lin_done
        ops.linear_dense_bwd(g, self.pooled, gr["cin_w"].view(-1), gr["cin_w0"], self.ws)
        cw = p["cin_w"].view(-1)
        L = len(self.units)
        drop = self._cin_drop
        keep, cmasks, on = drop if drop else (None, None, [False] * (L + 1))
        X0 = self._cin_x0
        dX0 = self.d_rows
        if on[0]:  # dropped input: collect dLoss/d(dropped E) apart, then scale and add
            self._dx0_cin = torch.zeros_like(self.E)
            dX0 = self._dx0_cin
        for i in range(L - 1, -1, -1):
            n = self.units[i]
            pf, c0 = self.pool_from[i], self.pool_col0[i]
            d_hidden = self.dxk[i + 1] if i + 1 < L else None
            cwd, pfa = cw[c0: c0 + n - pf], pf
            if on[i + 1]:
                # dropped layer: the whole upstream gradient of its maps, built explicitly
                # ([next layer's dXk | g x cin_w]) and scaled by mask / keep, goes in as "hidden"
                up = torch.empty_like(self.maps[i])
                if pf:
                    up[:, :pf] = d_hidden
                up[:, pf:] = g.view(-1, 1, 1) * cw[c0: c0 + n - pf].view(1, -1, 1)  # broadcast over D
                up.mul_(cmasks[i + 1] / keep[i + 1])
                d_hidden, cwd, pfa = up, None, n
            ops.cin_layer_bwd(
                X0, X0 if i == 0 else self.maps[i - 1], self.Hs[i], p[f"cin_filter_{i}"][0],
                self.cin_act, self.maps[i], g, dX0, gr[f"cin_filter_{i}"][0],
                gr[f"cin_bias_{i}"], self.cin_bws, xk_is_x0=(i == 0),
                d_hidden=d_hidden, cin_w_direct=cwd, pool_from=pfa, accumulate_dx0=True,
                dXk=self.dxk[i] if i > 0 else None, split=self.hp.get("cin_gemm", "bf16x6") == "bf16x6",
                first6=self.hp.get("cin_first_layer", "bf16x6") == "bf16x6")
        if on[0]:
            self.d_rows.addcmul_(self._dx0_cin, cmasks[0] / keep[0])

    def roofline_probes(self, idx, dense, y):
        # the heaviest CIN forward layer on the f32 MFMA roofline
        B, m, D = idx.shape[0], self.F, self.D
        self._alloc(B)
        i = max(range(len(self.units)), key=lambda k: self.Hs[k] * self.units[k])
        H, n = self.Hs[i], self.units[i]
        xk = self.E if i == 0 else self.maps[i - 1]
        p = self.params
        self._embed(idx, dense, False, None)
        self._cin_fwd()

        def fn():
            return ops.cin_layer_fwd(self.E, xk, H, p[f"cin_filter_{i}"][0], p[f"cin_bias_{i}"],
                                     self.cin_act, self.maps[i], self.cin_fws, pooled=self.pooled,
                                     pool_col0=self.pool_col0[i], pool_from=self.pool_from[i], ws6=self.cin_fws6)

        flops = 2.0 * B * D * m * H * n
        if fn() is True:
            # the product path of this layer: fp32 operands as three bf16 pieces, six piece products per k-step
            # (csrc/cin6.hip) - priced on the bf16 pipe with the six products counted, the fp32 GEMM beside it
            return [dict(name=f"cin_fwd6_kernel (rm_cin_layer_fwd6, layer {i}: m={m} H={H} N={n}; Z = fl(x0 * xk) split "
                              "into 3 bf16 pieces, 6 piece products per k-step on the bf16 matrix pipe)",
                         symbol="cin_fwd6_kernel", fn=fn, work=6.0 * flops, bound="mfma", peak=2500.0,
                         extra=lambda ms: {"fp32_gemm_tflops": round(flops / (ms * 1e-3) / 1e12, 2),
                                           "fp32_gemm_vs_f32_mfma_peak_157": round(flops / (ms * 1e-3) / 1e12 / 157.3, 4),
                                           "note": "peak = dense bf16 MFMA (2.5 PFLOP/s); achieved counts the six bf16 "
                                                   "products per fp32 product; the backward kernels (cin_dx / cin_dw: "
                                                   "f32 MFMA, 0.77-0.79 of 157.3 TFLOP/s) are now the longer launches"})]
        return [dict(name=f"cin_fwd_kernel (rm_cin_layer_fwd, layer {i}: m={m} H={H} N={n})",
                     symbol="cin_fwd_kernel", fn=fn, work=flops, bound="mfma")]


class AFMEngine(Engine):
    """AFM._init_graph (AFM.py:80-150): final = linear + afm, PredictionLayer(use_bias=False).  The attention
    layer is absent from the reference (AFM.py:7 comments the import out, AFM.py:119-122 uses it); arithmetic
    per arXiv 1708.04617 eq. (4)-(6), forward and backward fused in csrc/afm.hip:
        a_ij = softmax_ij(h . relu(W^T (E_i * E_j) + b)),  afm_logit = p . (m * sum_ij a_ij E_i * E_j)
    Variables (names chosen here): afm_attention_w [D,T], afm_attention_b [T], afm_attention_h [T,1],
    afm_projection_p [D,1].  l2: embeddings, linear weights and - as in the paper - the attention matrix W only
    (att_l2_reg).  The first-order bias tables AFM.py:102-109 gathers are never used: none are created.
    att_dropout is a KEEP probability (layers.py:461) applied to the pooled vector; masks["afm"] [B,D] carries the
    multiplier (0 or 1/keep)."""

    model = "afm"
    use_bias_tables = False

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, hp, task, device)
        self.T = int(hp.get("att_factor", 8))
        if not ops.afm_supported(self.F, self.D, self.T):
            raise ValueError(f"AFM: {self.F} embedding features, embedding_size={self.D}, att_factor={self.T} is not "
                             "supported by rm_afm_fwd (2..40 features, embedding_size 8/16/32/64, att_factor 1..64)")
        # (the attention layer is absent from the reference, AFM.py:7: glorot like dnn_w / cross_w_out)
        D, T = self.D, self.T
        self._var("afm_attention_w", (D, T), ("glorot", D, T), "att_l2_reg")
        self._var("afm_attention_b", (T,))
        self._var("afm_attention_h", (T, 1), ("glorot", T, 1))
        self._var("afm_projection_p", (D, 1), ("glorot", D, 1))

    def _model_masks(self, B, masks):
        ak = self.hp.get("att_dropout", 1)
        if ak is not None and ak < 1:
            masks["afm"] = (torch.rand(B, self.D, device=self.device) < ak).float() / ak

    def _alloc_model(self, B):
        dev = self.device
        self.afm_logit = torch.empty(B, dtype=F32, device=dev)
        self.afm_stats = torch.empty(B, ops.afm_stats_width(self.D), dtype=F32, device=dev)
        self.afm_ws = torch.empty(max(4, ops.afm_bwd_workspace(B, self.F, self.D, self.T)), dtype=F32, device=dev)

    def _afm_params(self):
        p = self.params
        return (p["afm_attention_w"], p["afm_attention_b"], p["afm_attention_h"].view(-1),
                p["afm_projection_p"].view(-1))

    def _afm_mask(self, masks, training):
        m = (masks or {}).get("afm") if training else None
        return m if (m is not None and self.hp.get("att_dropout", 1) < 1) else None

    def _branches_fwd(self, idx, dense, training, masks, lin_w):
        self._embed_plain(idx, dense, training, masks, lin_w)
        self._mask = self._afm_mask(masks, training)
        ops.afm_fwd(self.E, *self._afm_params(), self.afm_logit, mask=self._mask,
                    stats=self.afm_stats if training else None)
        return [(self.lin_logit, 1.0), (self.afm_logit, 1.0)]

    def _branches_bwd(self, idx, dense, g, masks):
        gr = self.grads
        # with no other branch over E, d_rows IS dLoss/dE (the linear term's gradients come from the base class)
        ops.afm_bwd(self.E, *self._afm_params(), g, self.afm_logit, self.afm_stats, self.d_rows,
                    gr["afm_attention_w"], gr["afm_attention_b"], gr["afm_attention_h"].view(-1),
                    gr["afm_projection_p"].view(-1), self.afm_ws, mask=self._mask)

    @staticmethod
    def afm_flops(B, F, D, T):
        """(forward, backward) flops of the attention kernels: per pair D multiplies, the 2 D T score product,
        2 T for h . relu, 2 D for the pooling; the backward recomputes that and adds three products of the score
        product's size (W dz, P dz^T, and dP * E twice)."""
        P = F * (F - 1) // 2
        fwd = B * P * (D + 2 * D * T + 2 * T + 2 * D)
        bwd = fwd + B * P * (2 * (2 * D * T) + 4 * D)
        return fwd, bwd

    def roofline_probes(self, idx, dense, y):
        B = idx.shape[0]
        self._probe_fill(idx, dense, y)  # E, stats, dlogit
        fwd, bwd = self.afm_flops(B, self.F, self.D, self.T)
        gr = self.grads
        return self._probes(
            idx, dense, y,
            (f"afm_bwd_kernel (rm_afm_bwd: F={self.F} D={self.D} T={self.T}; recompute + dE + dW, db, dh, "
             "dp; flops = forward + W dz, P dz^T, dP * E)", "afm_bwd_kernel",
             lambda: ops.afm_bwd(self.E, *self._afm_params(), self.dlogit, self.afm_logit, self.afm_stats,
                                 self.d_rows, gr["afm_attention_w"], gr["afm_attention_b"],
                                 gr["afm_attention_h"].view(-1), gr["afm_projection_p"].view(-1), self.afm_ws),
             float(bwd), "mfma"),
            (f"afm_fwd_kernel (rm_afm_fwd: F={self.F} D={self.D} T={self.T}; flops = P (D + 2 D T + 2 T "
             "+ 2 D) per example, on the vector ALU - priced against the fp32 peak both pipes share)",
             "afm_fwd_kernel",
             lambda: ops.afm_fwd(self.E, *self._afm_params(), self.afm_logit, stats=self.afm_stats),
             float(fwd), "mfma"))


class DINEngine(DeepFMEngine):
    """DIN._init_graph (DIN.py, which stops after the pooling layer): final = linear + DNN([E | dense]), where E holds
    the plain features' rows and ONE attention-pooled interest row per sequence feature (Engine._seq_fwd; Deep
    Interest Network, arXiv 1706.06978) - the DeepFM engine without its FM term and without bias tables."""

    model = "din"
    use_bias_tables = False
    shardable = False
    _model_masks = Engine._model_masks  # (no FM term: no fm_dropout masks)

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, dict(hp, use_fm=False, use_deep=True), task, device)


class BSTEngine(DINEngine):
    """Behavior Sequence Transformer (arXiv 1905.06874): final = linear + DNN([E | dense]) as DIN, with every sequence
    feature pooled by the transformer unit (seq_pooling is forced to "transformer"; csrc/bst.hip): one post-norm
    encoder block over the history and the candidate with a position table by distance from the candidate, mean
    over the tokens.  hp: att_head_num 2, att_ffn_units 4 * embedding_size."""

    model = "bst"

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, dict(hp, seq_pooling="transformer"), task, device)


class DIENEngine(DINEngine):
    """Deep Interest Evolution Network (arXiv 1809.03672): final = linear + DNN([E | dense]) as DIN, with every
    sequence feature pooled by the interest-evolution unit (seq_pooling is forced to "dien"; csrc/dien.hip): a GRU
    over the history, the candidate's softmax attention over its states, and an attention-gated GRU (AUGRU) whose
    last state is the feature's row.  Hidden size = embedding_size; no auxiliary loss; no hyper-parameter."""

    model = "dien"

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, dict(hp, seq_pooling="dien"), task, device)


class AutoIntEngine(DeepFMEngine):
    """AutoInt (arXiv 1810.11921): final = linear + autoint (+ DNN([E | dense]) with a non-empty deep_hidden_units:
    AutoInt+), PredictionLayer(use_bias=False).  Nothing in the reference implements it.  L interacting layers of
    multi-head self-attention over the F rows of E, forward and backward fused in csrc/autoint.hip:
        Q, K, V = X Wq, X Wk, X Wv;  a^h_m. = softmax_k(<Q^h_m, K^h_k> c);  Y_m = relu(concat_h sum_k a^h_mk V^h_k + X_m Wr)
        autoint_logit = flatten(Y_L) . autoint_w + autoint_w0
    Variables (names chosen here): autoint_layer_{l}_query_w / _key_w / _value_w [Din, H dk], autoint_layer_{l}_res_w
    (att_res only), autoint_w [F H dk, 1], autoint_w0 [1]; Din = embedding_size for layer 0, H dk after it.
    l2: att_l2_reg over every matrix above.  No bias tables; the dense features enter the linear term and the DNN
    only.  The attention needs E in HBM: the one-kernel step is never selected (no FM term) and the DNN runs behind
    the interacting layers so that its fused head sees the attention's logit."""

    model = "autoint"
    use_bias_tables = False
    shardable = False
    needs_fm_or_deep = False
    _model_masks = Engine._model_masks  # (no FM term: no fm_dropout masks)

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        hidden = tuple(hp.get("deep_hidden_units") or ())
        n = len(hidden)
        keep = hp.get("deep_dropout")
        hp = dict(hp, use_fm=False, use_deep=n > 0, deep_hidden_units=hidden,
                  deep_dropout=tuple(keep) if keep is not None else (1,) * (n + 1))
        super().__init__(spec, embedding_size, hp, task, device)
        self.L = int(hp.get("att_layer_num", 3))
        self.dk = int(hp.get("att_embedding_size", 8))
        self.H = int(hp.get("att_head_num", 2))
        self.res = bool(hp.get("att_res", True))
        self.HD = self.H * self.dk
        self.scale = float(self.dk) ** -0.5 if hp.get("att_scaling", False) else 1.0
        if self.L < 1:
            raise ValueError(f"AutoInt: att_layer_num={self.L} must be at least 1")
        dins = [self.D] + [self.HD] * (self.L - 1)
        for din in dins:
            if not ops.autoint_supported(self.F, din, self.H, self.dk):
                raise ValueError(
                    f"AutoInt: {self.F} embedding features, layer input width {din}, att_head_num={self.H}, "
                    f"att_embedding_size={self.dk} is not supported by rm_autoint_layer_fwd (1..40 features, "
                    "embedding_size 8/16/32/64, att_head_num 1/2/4/8, att_embedding_size >= 4, att_head_num * "
                    "att_embedding_size 8/16/32/64)")
        self.dins = dins
        # (the interacting layers are absent from the reference: glorot like dnn_w)
        for l, din in enumerate(dins):
            for kind in ("query", "key", "value") + (("res",) if self.res else ()):
                self._var(f"autoint_layer_{l}_{kind}_w", (din, self.HD), ("glorot", din, self.HD), "att_l2_reg")
        self._var("autoint_w", (self.F * self.HD, 1), ("glorot", self.F * self.HD, 1), "att_l2_reg")
        self._var("autoint_w0", (1,))

    def _alloc_model(self, B):
        dev, F, H = self.device, self.F, self.H
        self.att_Y = [torch.empty(B, F, self.HD, dtype=F32, device=dev) for _ in range(self.L)]
        self.att_stats = [torch.empty(B, H, F, 2, dtype=F32, device=dev) for _ in range(self.L)]
        self.att_dY = torch.empty(B, F, self.HD, dtype=F32, device=dev)
        self.att_dX = torch.empty(B, F, self.HD, dtype=F32, device=dev) if self.L > 1 else None
        self.att_logit = torch.empty(B, dtype=F32, device=dev)
        need = max([ops.autoint_layer_bwd_workspace(B, F, din, H, self.dk) for din in self.dins]
                   + [ops.autoint_head_bwd_workspace(B, F * self.HD), 4])
        self.att_ws = torch.empty(need, dtype=F32, device=dev)

    def _att_weights(self, l, src):
        return [src.get(f"autoint_layer_{l}_{kind}_w") for kind in ("query", "key", "value", "res")]

    def _att_fwd(self, training):
        x = self.E
        for l in range(self.L):
            ops.autoint_layer_fwd(x, *self._att_weights(l, self.params), self.H, self.scale, self.att_Y[l],
                                  stats=self.att_stats[l] if training else None)
            x = self.att_Y[l]
        ops.autoint_head_fwd(x, self.params["autoint_w"].view(-1), self.params["autoint_w0"], self.att_logit)

    def _att_bwd(self, g, dx_up):
        """The head and the layers in reverse; layer 0 writes d_rows (= dx_up + its own when the DNN ran first)."""
        p, gr = self.params, self.grads
        ops.autoint_head_bwd(self.att_Y[-1], p["autoint_w"].view(-1), g, self.att_dY, gr["autoint_w"].view(-1),
                             gr["autoint_w0"], self.att_ws)
        dy, spare = self.att_dY, self.att_dX  # two buffers of one shape take turns: a layer's dX is the next one's dY
        for l in reversed(range(self.L)):
            x = self.att_Y[l - 1] if l else self.E
            dx = spare if l else self.d_rows
            ops.autoint_layer_bwd(x, *self._att_weights(l, p), self.att_Y[l], self.att_stats[l], dy, self.H,
                                  self.scale, dx, *self._att_weights(l, gr), self.att_ws,
                                  dX_up=dx_up if l == 0 else None)
            dy, spare = dx, dy

    def _branches_fwd(self, idx, dense, training, masks, lin_w):
        m = self._embed_plain(idx, dense, training, masks, lin_w)
        self._att_fwd(training)
        branches = [(self.lin_logit, 1.0), (self.att_logit, 1.0)]
        if self.use_deep:
            self.dnn_logit = self._mlp_last(self.mlp, self.E.view(-1, self.FD), dense if self.Dn else None,
                                            self._dnn_keep(training), m.get("dnn"), list(branches))
            branches.append((self.dnn_logit, 1.0))
        return branches

    def _branches_bwd(self, idx, dense, g, masks):
        super()._branches_bwd(idx, dense, g, masks)  # the DNN (when there is one) writes d_rows
        self._att_bwd(g, self.d_rows if self.use_deep else None)

    @staticmethod
    def autoint_flops(B, F, Din, HD):
        """(forward, backward) flops of one interacting layer: 8 F Din HD for the four projections plus 4 F^2 HD for
        the scores and the weighted sums; the backward recomputes the forward and adds about twice that."""
        fwd = B * (8 * F * Din * HD + 4 * F * F * HD)
        return fwd, 3 * fwd

    def roofline_probes(self, idx, dense, y):
        B = idx.shape[0]
        self._probe_fill(idx, dense, y)  # E, Y, stats
        fwd, bwd = self.autoint_flops(B, self.F, self.D, self.HD)
        p, gr = self.params, self.grads
        dy = torch.randn(B, self.F, self.HD, dtype=F32, device=self.device)
        dx = torch.empty_like(self.E)
        shape = f"F={self.F} Din={self.D} H={self.H} dk={self.dk}"
        return self._probes(
            idx, dense, y,
            (f"autoint_bwd_kernel (rm_autoint_layer_bwd, layer 0: {shape}; recompute + dX + dWq, dWk, dWv, "
             "dWr; flops = 3 x forward)", "autoint_bwd_kernel",
             lambda: ops.autoint_layer_bwd(self.E, *self._att_weights(0, p), self.att_Y[0], self.att_stats[0],
                                           dy, self.H, self.scale, dx, *self._att_weights(0, gr), self.att_ws),
             float(bwd), "mfma"),
            (f"autoint_fwd_kernel (rm_autoint_layer_fwd, layer 0: {shape}; flops = 8 F Din HD + 4 F^2 HD per "
             "example, on the vector ALU - priced against the fp32 peak both pipes share)", "autoint_fwd_kernel",
             lambda: ops.autoint_layer_fwd(self.E, *self._att_weights(0, p), self.H, self.scale, self.att_Y[0],
                                           stats=self.att_stats[0]),
             float(fwd), "mfma"))


class Tower:
    """A plain MLP tower in front of an interaction layer (DLRM's bottom MLP, the two towers of TwoTower): a_0 = x
    [B,K0], a_{l+1} = act(a_l W_l + b_l) for every layer, the last one included; no dropout, no output projection.
    linear_last: the last layer is a_L W_L + b_L without the activation (an embedding head).
    Variables {prefix}dnn_layer_{l}_weights / _bias.  Layer by layer on the wide dense kernels (csrc/gemm.hip,
    csrc/gemm6.hip): bias and activation in the epilogue, the bf16x6 path where `dense_gemm` allows it and the
    kernel takes the call - the choice MLP's wide path makes."""

    def __init__(self, params, grads, K0, widths, activation, device, prefix, dense_gemm="bf16x6", linear_last=False):
        self.K0, self.widths = int(K0), [int(w) for w in widths]
        self.act = act_name(activation)
        if self.act not in ("relu", "leaky_relu", "identity"):
            raise ValueError(self.act)
        self.linear_last = bool(linear_last)
        self.p, self.g, self.prefix = params, grads, prefix
        self.dims = [self.K0] + self.widths
        self.decl = {}
        _declare_layers(params, grads, self.decl, prefix, self.dims, device)
        self.dense_gemm = dense_gemm
        self._B = None

    def _alloc(self, B, device):
        if self._B == B:
            return
        self._B = B
        self.a = [torch.empty(B, h, dtype=F32, device=device) for h in self.widths]
        self.da = [torch.empty(B, h, dtype=F32, device=device) for h in self.widths[:-1]]
        self._fws, self._wws, self._fws6, self._wws6 = _dense_workspaces(self.dims, B, device, self.dense_gemm)

    def forward(self, x, x2=None):
        """[x | x2] [B,K0] -> a_last [B, widths[-1]] (an internal buffer); x and x2 (optional) may be column ranges
        of wider buffers."""
        self._alloc(x.shape[0], x.device)
        self.x, self.x2 = x, x2
        p, pre = self.p, self.prefix
        prev, last = x, len(self.widths) - 1
        for i in range(len(self.widths)):
            ops.dense_fwd(prev, x2 if i == 0 else None, p[f"{pre}dnn_layer_{i}_weights"], self.a[i], self._fws,
                          bias=p[f"{pre}dnn_layer_{i}_bias"],
                          act="identity" if (self.linear_last and i == last) else self.act, ws6=self._fws6)
            prev = self.a[i]
        return prev

    def backward(self, dz, dx=None):
        """dz [B, widths[-1]] = dLoss/da_last (turned into the last pre-activation's gradient in place); writes
        the parameter gradients.  dx [B, K] (K <= K0; a column range of a wider buffer works), when given, receives
        dLoss/d(the first K columns of the input); without it no gradient is formed for the input."""
        p, gr, pre = self.p, self.g, self.prefix
        ident = self.act == "identity"
        da = dz
        if not ident and not self.linear_last:
            ops.act_bwd_(da, self.a[-1], self.act)
        for i in range(len(self.widths) - 1, -1, -1):
            prev = self.a[i - 1] if i else self.x
            ops.dense_wgrad(prev, None if i else self.x2, da, gr[f"{pre}dnn_layer_{i}_weights"], self._wws,
                            db=gr[f"{pre}dnn_layer_{i}_bias"], ws6=self._wws6)
            if i:
                ops.dense_fwd(da, None, p[f"{pre}dnn_layer_{i}_weights"], self.da[i - 1], self._fws, transposed=True,
                              epilogue=ops.DENSE_ADD if ident else ops.DENSE_MUL_ACTGRAD, act=self.act,
                              aux1=None if ident else prev, ws6=self._fws6)
                da = self.da[i - 1]
            elif dx is not None:
                ops.dense_fwd(da, None, p[f"{pre}dnn_layer_0_weights"][: dx.shape[1]], dx, self._fws, transposed=True,
                              epilogue=ops.DENSE_ADD, ws6=self._fws6)


class InteractionEngine(Engine):
    """The flow DLRM, FiBiNET and PNN share: E -> one fused interaction kernel -> X [B, ldx] -> DNN([X | dense]);
    final = DNN logit (+ linear if use_linear).  The DNN's dX is no table-row gradient: d_rows comes from the
    interaction's backward, and since no other branch reads E it IS dLoss/dE.  X and dX are [B, ldx] buffers, ldx = W
    rounded up to what the kernels' row loads need; the kernels and the DNN see the [:, :W] views, and the pad columns
    are written once, as +0.0, when the buffers are made - never again.
    A model plugs in with
        _interaction(hp)          its limit checks and variable declarations -> (W, ldx)
        _alloc_interaction(B)     its further per-batch-size buffers (optional)
        _interact_fwd(dense, X)   E (and whatever it makes of dense) -> X
        _interact_bwd(dX)         dX -> d_rows and its own variables' gradients
    and the class attributes below."""

    title = None               # the model's name in its error messages
    linear_default = True      # hp["use_linear"] when it is absent
    dnn_reads_dense = True     # DNN([X | dense]); False: DNN(X)
    dnn_prefix = ""            # in front of the DNN's variable names
    dnn_noun = "DNN"           # what the error message calls it

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, hp, task, device)
        self.use_linear = bool(hp.get("use_linear", self.linear_default))
        self.W, self.ldx = self._interaction(hp)
        hidden = tuple(hp.get("deep_hidden_units") or ())
        if not hidden:
            raise ValueError(f"{self.title}: deep_hidden_units must name at least one layer of the {self.dnn_noun}")
        # (the DNN reads the interaction's output, not [E | dense]; its dX is no table-row gradient)
        self.mlp = self._dnn(self.W, self.Dn if self.dnn_reads_dense else 0, hidden, "relu", prefix=self.dnn_prefix,
                             stream_d_rows=False)

    def _alloc_model(self, B):
        self.X = torch.zeros(B, self.ldx, dtype=F32, device=self.device)
        self.dX = torch.zeros(B, self.ldx, dtype=F32, device=self.device)
        self._alloc_interaction(B)

    def _alloc_interaction(self, B):
        pass

    def _branches_fwd(self, idx, dense, training, masks, lin_w):
        m = self._embed_plain(idx, dense, training, masks, lin_w)
        X = self.X[:, : self.W]
        self._interact_fwd(dense, X)
        branches = [(self.lin_logit, 1.0)] if self.use_linear else []
        self.dnn_logit = self._mlp_last(self.mlp, X, dense if self.mlp.Dn else None, self._dnn_keep(training),
                                        m.get("dnn"), list(branches))
        branches.append((self.dnn_logit, 1.0))
        return branches

    def _branches_bwd(self, idx, dense, g, masks):
        dX = self.dX[:, : self.W]
        self.mlp.backward(g, dX)
        self._interact_bwd(dX)


class DLRMEngine(InteractionEngine):
    """DLRM (arXiv 1906.00091, the MLPerf recommendation model): the dense features go through a bottom tower to
    one embedding-wide vector z; the interaction takes every pairwise dot product among z and the F rows of E;
    [z | dots] feeds the top MLP.  final = top logit (+ linear if use_linear).  Nothing in the reference implements it.
        a_0 = dense;  a_{l+1} = act(a_l W_l + b_l), widths bottom_hidden_units + (embedding_size,);  z = a_last
        v_0 = z, v_f = E[:, f-1];  X = [z | <v_i, v_j> for 0 <= j < i <= F]          (csrc/dot_interact.hip)
        logit = DNN_top(X)
    Variables (names chosen here): bot_dnn_layer_{l}_weights / _bias, top_dnn_layer_{l}_weights / _bias, top_dnn_w,
    top_dnn_w0.  deep_activation applies to both towers, deep_dropout to the top one, deep_l2_reg to every weight
    matrix of both and top_dnn_w.  No bias tables.  X and dX live in buffers whose rows are padded to a multiple
    of 4 floats; the top MLP sees the [B, D + P] view."""

    model, title = "dlrm", "DLRM"
    use_bias_tables = False
    linear_default = False
    dnn_reads_dense, dnn_prefix, dnn_noun = False, "top_", "top tower"

    def _interaction(self, hp):
        limits = "at least one dense feature, 1..40 embedding features, embedding_size 8/16/32/64"
        if self.Dn < 1:
            raise ValueError(f"DLRM: the bottom tower needs a dense feature, there is none ({limits})")
        if not ops.dot_interact_supported(self.F, self.D):
            raise ValueError(f"DLRM: {self.F} embedding features of embedding_size={self.D} are not supported by "
                             f"rm_dot_interact_fwd ({limits})")
        self.bot = self._adopt(Tower(self.params, self.grads, self.Dn,
                                     tuple(hp.get("bottom_hidden_units", (64, 32))) + (self.D,),
                                     hp.get("deep_activation", "relu"), self.device, "bot_",
                                     dense_gemm=hp.get("dense_gemm", "bf16x6")))
        return ops.dot_interact_width(self.F, self.D)

    def _alloc_interaction(self, B):
        self.dz = torch.empty(B, self.D, dtype=F32, device=self.device)

    def _interact_fwd(self, dense, X):
        self.z = self.bot.forward(dense)
        ops.dot_interact_fwd(self.E, self.z, X)

    def _interact_bwd(self, dX):
        ops.dot_interact_bwd(self.E, self.z, dX, self.d_rows, self.dz)
        self.bot.backward(self.dz)

    def roofline_probes(self, idx, dense, y):
        self._probe_fill(idx, dense, y)  # E, z, dX
        B, F, D, ldx = idx.shape[0], self.F, self.D, self.ldx
        X, dX = self.X[:, : self.W], self.dX[:, : self.W]
        d_rows, dz = torch.empty_like(self.d_rows), torch.empty_like(self.dz)
        shape = f"F={F} D={D} ldx={ldx}"
        return self._probes(
            idx, dense, y,
            (f"dot_bwd_kernel (rm_dot_interact_bwd, {shape}: E, z, dX read once, d_rows and dz written once)",
             "dot_bwd_kernel", lambda: ops.dot_interact_bwd(self.E, self.z, dX, d_rows, dz),
             B * 4 * (2 * F * D + 2 * D + ldx), "hbm"),
            (f"dot_fwd_kernel (rm_dot_interact_fwd, {shape}: E and z read once, X written once)",
             "dot_fwd_kernel", lambda: ops.dot_interact_fwd(self.E, self.z, X), B * 4 * (F * D + D + ldx), "hbm"))


class FiBiNETEngine(InteractionEngine):
    """FiBiNET (arXiv 1905.09433): a squeeze-excitation gate re-weights the F rows of E, a bilinear interaction runs
    over every field pair of the raw and of the re-weighted rows, and the DNN reads both.  final = DNN([X | dense])
    (+ linear if use_linear, the default).  Nothing in the reference implements it.
        z_f = mean_d E[f,d];  s = relu(z senet_w1);  a = relu(s senet_w2);  V[f] = a_f E[f]
        bilinear(Y, W)[(i,j), d] = (Y_i W_(i))[d] Y_j[d], i < j;  W_(i) = W[0] ("all") or W[i] ("each")
        X = [bilinear(E, bilinear_w) | bilinear(V, senet_bilinear_w)]                    (csrc/fibinet.hip)
    Variables (names chosen here): senet_w1 [F,R], senet_w2 [R,F], R = max(1, F // reduction_ratio), bilinear_w and
    senet_bilinear_w [1 | F-1, D, D] - glorot, l2 key interaction_l2_reg.  No bias tables.  X and dX are [B, 2PD]
    buffers: 2PD = F(F-1)D is a multiple of 8, so their rows need no pad."""

    model, title = "fibinet", "FiBiNET"
    use_bias_tables = False

    def _interaction(self, hp):
        limits = "2..40 embedding features, embedding_size 8/16/32, bilinear_type 'all' or 'each'"
        self.btype = hp.get("bilinear_type", "each")
        if self.btype == "interaction":
            raise ValueError("FiBiNET: bilinear_type='interaction' (one matrix per field pair) is out of scope: "
                             f"use 'all' or 'each' ({limits})")
        if self.btype not in ops.FIBINET_TYPES:
            raise ValueError(f"FiBiNET: bilinear_type {self.btype!r} is not supported ({limits})")
        ratio = int(hp.get("reduction_ratio", 3))
        if ratio < 1:
            raise ValueError(f"FiBiNET: reduction_ratio={ratio} must be at least 1")
        F, D = self.F, self.D
        self.R = R = max(1, F // ratio)
        if not ops.fibinet_supported(F, D, R, self.btype):
            raise ValueError(f"FiBiNET: {F} embedding features of embedding_size={D} are not supported by "
                             f"rm_fibinet_fwd ({limits})")
        nW = F - 1 if self.btype == "each" else 1
        l2 = "interaction_l2_reg"
        self._var("senet_w1", (F, R), ("glorot", F, R), l2)
        self._var("senet_w2", (R, F), ("glorot", R, F), l2)
        self._var("bilinear_w", (nW, D, D), ("glorot", D, D), l2)
        self._var("senet_bilinear_w", (nW, D, D), ("glorot", D, D), l2)
        return ops.fibinet_width(F, D)

    def _alloc_interaction(self, B):
        self.fib_ws = torch.empty(max(4, ops.fibinet_bwd_workspace(B, self.F, self.D, self.R, self.btype)),
                                  dtype=F32, device=self.device)

    def _fib_vars(self, d):
        return d["senet_w1"], d["senet_w2"], d["bilinear_w"], d["senet_bilinear_w"]

    def _interact_fwd(self, dense, X):
        ops.fibinet_fwd(self.E, *self._fib_vars(self.params), self.btype, X)

    def _interact_bwd(self, dX):
        ops.fibinet_bwd(self.E, *self._fib_vars(self.params), self.btype, dX, self.d_rows,
                        *self._fib_vars(self.grads), self.fib_ws)

    def roofline_probes(self, idx, dense, y):
        self._probe_fill(idx, dense, y)  # E, dX
        B, F, D, ldx = idx.shape[0], self.F, self.D, self.ldx
        X, dX = self.X[:, : self.W], self.dX[:, : self.W]
        d_rows = torch.empty_like(self.d_rows)
        dws = [torch.empty_like(t) for t in self._fib_vars(self.grads)]
        shape = f"F={F} D={D} R={self.R} {self.btype} ldx={ldx}"
        return self._probes(
            idx, dense, y,
            (f"fibinet_bwd_kernel (rm_fibinet_bwd, {shape}: E and dX read once from HBM, d_rows written once)",
             "fibinet_bwd_kernel",
             lambda: ops.fibinet_bwd(self.E, *self._fib_vars(self.params), self.btype, dX, d_rows, *dws, self.fib_ws),
             B * 4 * (2 * F * D + ldx), "hbm"),
            (f"fibinet_fwd_kernel (rm_fibinet_fwd, {shape}: E read once, X written once)", "fibinet_fwd_kernel",
             lambda: ops.fibinet_fwd(self.E, *self._fib_vars(self.params), self.btype, X),
             B * 4 * (F * D + ldx), "hbm"))


class FmFMEngine(DeepFMEngine):
    """Field-pair weighted FM - FwFM (arXiv 1806.03514), FvFM and FmFM (arXiv 2102.12994): final = linear (use_linear,
    the default) + pair (+ DNN([E | dense]) with a non-empty deep_hidden_units: DeepFwFM and its kin),
    PredictionLayer(use_bias=False).  Nothing in the reference implements them.  Over the P = F(F-1)/2 field pairs
    i < j in itertools.combinations order, forward and backward fused in csrc/fmfm.hip:
        pair_logit = sum_{i<j} E_i W_(ij) E_j^T
        field_interaction "matrix": W_(ij) = field_pair_w[p] [P,D,D] (the left field on the rows);  "vector":
        diag(field_pair_w[p]) [P,D];  "scalar": field_pair_w[p] I [P]
    field_pair_w starts at plain FM (identity matrices / ones); l2 key interaction_l2_reg.  No bias tables; the dense
    features enter the linear term and the DNN only.  The pair kernels need E in HBM: the one-kernel step is never
    selected (no FM term) and the DNN runs behind them so that its fused head sees the pair logit."""

    model = "fmfm"
    use_bias_tables = False
    shardable = False
    needs_fm_or_deep = False
    _model_masks = Engine._model_masks  # (no FM term: no fm_dropout masks)

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        hidden = tuple(hp.get("deep_hidden_units") or ())
        n = len(hidden)
        keep = hp.get("deep_dropout")
        hp = dict(hp, use_fm=False, use_deep=n > 0, deep_hidden_units=hidden,
                  deep_dropout=tuple(keep) if keep is not None else (1,) * (n + 1))
        super().__init__(spec, embedding_size, hp, task, device)
        self.use_linear = bool(hp.get("use_linear", True))
        self.ftype = hp.get("field_interaction", "matrix")
        if self.ftype not in ops.FMFM_TYPES:
            raise ValueError(f"FmFM: field_interaction {self.ftype!r} is not one of 'matrix', 'vector', 'scalar'")
        if not ops.fmfm_supported(self.F, self.D, self.ftype):
            raise ValueError(f"FmFM: {self.F} embedding features of embedding_size={self.D} are not supported by "
                             "rm_fmfm_fwd (2..40 embedding features, embedding_size 8/16/32)")
        self.P = self.F * (self.F - 1) // 2
        self._var("field_pair_w", ops.fmfm_weight_shape(self.F, self.D, self.ftype), "pair_identity",
                  "interaction_l2_reg")

    def _alloc_model(self, B):
        dev = self.device
        self.pair_logit = torch.empty(B, dtype=F32, device=dev)
        self.pair_ws = torch.empty(max(4, ops.fmfm_bwd_workspace(B, self.F, self.D, self.ftype)), dtype=F32,
                                   device=dev)

    def _branches_fwd(self, idx, dense, training, masks, lin_w):
        m = self._embed_plain(idx, dense, training, masks, lin_w)
        ops.fmfm_fwd(self.E, self.params["field_pair_w"], self.ftype, self.pair_logit)
        branches = ([(self.lin_logit, 1.0)] if self.use_linear else []) + [(self.pair_logit, 1.0)]
        if self.use_deep:
            self.dnn_logit = self._mlp_last(self.mlp, self.E.view(-1, self.FD), dense if self.Dn else None,
                                            self._dnn_keep(training), m.get("dnn"), list(branches))
            branches.append((self.dnn_logit, 1.0))
        return branches

    def _branches_bwd(self, idx, dense, g, masks):
        super()._branches_bwd(idx, dense, g, masks)  # the DNN (when there is one) writes d_rows
        ops.fmfm_bwd(self.E, self.params["field_pair_w"], self.ftype, g, self.d_rows, self.grads["field_pair_w"],
                     self.pair_ws, dE_up=self.d_rows if self.use_deep else None)

    def roofline_probes(self, idx, dense, y):
        B, F, D, P = idx.shape[0], self.F, self.D, self.P
        self._probe_fill(idx, dense, y)  # E, dlogit
        w, dw = self.params["field_pair_w"], torch.empty_like(self.grads["field_pair_w"])
        d_rows = torch.empty_like(self.d_rows)
        shape = f"F={F} D={D} {self.ftype}"
        if self.ftype == "matrix":
            fwd, bwd, bound = 2.0 * B * P * D * D, 6.0 * B * P * D * D, "mfma"
            names = ("fmfm_de_kernel", "fmfm_fwd_kernel")
            what = "flops = 2 B P D^2 forward, three times that backward (dE both ways + dM)"
        else:
            # algorithmic bytes: E read once and the logit written; E and g read once, d_rows written once (+ W, dW)
            fwd, bwd, bound = 4.0 * (B * F * D + B + w.numel()), 4.0 * (2 * B * F * D + B + 2 * w.numel()), "hbm"
            names = ("fmfm_vs_de_kernel", "fmfm_vs_fwd_kernel")
            what = "algorithmic bytes: E (+ g) in, logit / d_rows out, the weights and their gradient"
        return self._probes(
            idx, dense, y,
            (f"{names[0]} + dW kernels (rm_fmfm_bwd, {shape}; {what})", names[0],
             lambda: ops.fmfm_bwd(self.E, w, self.ftype, self.dlogit, d_rows, dw, self.pair_ws), bwd, bound),
            (f"{names[1]} (rm_fmfm_fwd, {shape}; {what})", names[1],
             lambda: ops.fmfm_fwd(self.E, w, self.ftype, self.pair_logit), fwd, bound))


class PNNEngine(InteractionEngine):
    """Product-based Neural Network (PNN, arXiv 1611.00144) with the kernel-form product layer of the widely used
    open-source PNN (use_inner, use_outter, kernel_type mat / vec / num) - NOT the paper's sum-pooled outer-product
    shortcut.  final = DNN([X | dense]) (+ linear if use_linear; off by default).  Nothing in the reference implements
    it.  Over the P = F(F-1)/2 field pairs i < j in itertools.combinations order, fused in csrc/pnn.hip:
        X = [ E flattened | <E_i, E_j> (use_inner) | E_i K_(ij) E_j^T (use_outer) ]
        kernel_type "mat": K_(ij) = product_kernel[p] [P,D,D] (the left field on the rows);  "vec":
        diag(product_kernel[p]) [P,D];  "num": product_kernel[p] I [P]
    Variable (with use_outer only): product_kernel, glorot with fan D / D for all three kernel types, l2 key
    interaction_l2_reg.  No bias tables.  X and dX are [B, ldx] buffers, ldx = W rounded up to 4 floats; the pad
    columns stay +0.0.  The DNN's dX is no table-row gradient: d_rows comes from rm_pnn_bwd, which adds the row part
    of dX to the products' gradient and writes it once."""

    model, title = "pnn", "PNN"
    use_bias_tables = False
    shardable = False
    linear_default = False

    def _interaction(self, hp):
        limits = ("2..40 embedding features, embedding_size 8/16/32, use_inner or use_outer, kernel_type 'mat', 'vec' "
                  "or 'num'")
        self.ktype = hp.get("kernel_type", "mat")
        self.products = ops.pnn_products(hp.get("use_inner", True), hp.get("use_outer", False))
        if not self.products:
            raise ValueError(f"PNN: neither use_inner nor use_outer is set: the product layer would be empty ({limits})")
        if self.ktype not in ops.PNN_KERNELS:
            raise ValueError(f"PNN: kernel_type {self.ktype!r} is not one of 'mat', 'vec', 'num' ({limits})")
        F, D = self.F, self.D
        if not ops.pnn_supported(F, D, self.products, self.ktype):
            raise ValueError(f"PNN: {F} embedding features of embedding_size={D} are not supported by rm_pnn_fwd "
                             f"({limits})")
        self.P = F * (F - 1) // 2
        self.outer = bool(self.products & ops.PNN_OUTER)
        if self.outer:
            self._var("product_kernel", ops.pnn_weight_shape(F, D, self.ktype), ("glorot", D, D), "interaction_l2_reg")
        return ops.pnn_width(F, D, self.products)

    def _alloc_interaction(self, B):
        self.pnn_ws = (torch.empty(max(4, ops.pnn_bwd_workspace(B, self.F, self.D, self.products, self.ktype)),
                                   dtype=F32, device=self.device) if self.outer else None)

    def _interact_fwd(self, dense, X):
        ops.pnn_fwd(self.E, self.params.get("product_kernel"), self.products, self.ktype, X)

    def _interact_bwd(self, dX):
        ops.pnn_bwd(self.E, self.params.get("product_kernel"), self.products, self.ktype, dX, self.d_rows,
                    self.grads.get("product_kernel"), self.pnn_ws)

    def roofline_probes(self, idx, dense, y):
        self._probe_fill(idx, dense, y)  # E, dX
        B, F, D, P, ldx = idx.shape[0], self.F, self.D, self.P, self.ldx
        X, dX = self.X[:, : self.W], self.dX[:, : self.W]
        k = self.params.get("product_kernel")
        dk = torch.empty_like(k) if k is not None else None
        d_rows = torch.empty_like(self.d_rows)
        shape = f"F={F} D={D} products={self.products} {self.ktype} ldx={ldx}"
        if self.outer and self.ktype == "mat":
            fwd, bwd, bound = 2.0 * B * P * D * D, 6.0 * B * P * D * D, "mfma"
            names = ("pnn_de_mat_kernel", "pnn_fwd_kernel")
            what = "flops = 2 B P D^2 forward, three times that backward (dE both ways + dK)"
        else:
            # algorithmic bytes: E read once and X written; E and dX read once, d_rows written once (+ K, dK)
            nk = k.numel() if k is not None else 0
            fwd, bwd, bound = 4.0 * (B * F * D + B * ldx + nk), 4.0 * (2 * B * F * D + B * ldx + 2 * nk), "hbm"
            names = ("pnn_de_valu_kernel", "pnn_fwd_kernel")
            what = "algorithmic bytes: E (+ dX) in, X / d_rows out, the kernel and its gradient"
        return self._probes(
            idx, dense, y,
            (f"{names[0]} + dK kernels (rm_pnn_bwd, {shape}; {what})", names[0],
             lambda: ops.pnn_bwd(self.E, k, self.products, self.ktype, dX, d_rows, dk, self.pnn_ws), bwd, bound),
            (f"{names[1]} (rm_pnn_fwd, {shape}; {what})", names[1],
             lambda: ops.pnn_fwd(self.E, k, self.products, self.ktype, X), fwd, bound))


def masknet_limits(hp, F, D):
    """MaskNet's limits in one place (th.MaskNet checks them at construction, MaskNetEngine when it is built): a
    ValueError naming the limit, or (block_order, num_blocks, block_hidden_units, reduction_ratio, deep_hidden_units)."""
    order = hp.get("block_order", "parallel")
    if order not in ("parallel", "serial"):
        raise ValueError(f"MaskNet: block_order {order!r} is not one of 'parallel', 'serial'")
    N = int(hp.get("num_blocks", 3))
    if not 1 <= N <= 8:
        raise ValueError(f"MaskNet: num_blocks={N} is outside 1..8")
    H = int(hp.get("block_hidden_units", 64))
    if H % 4 or not 8 <= H <= 2048:
        raise ValueError(f"MaskNet: block_hidden_units={H} must be a multiple of 4 in 8..2048")
    ratio = float(hp.get("reduction_ratio", 2.0))
    if not ratio > 0:
        raise ValueError(f"MaskNet: reduction_ratio={ratio} must be greater than 0")
    if D not in (8, 16, 32) or not 1 <= F <= 40:
        raise ValueError(f"MaskNet: {F} embedding features of embedding_size={D} are not supported by "
                         "rm_masknet_group_fwd (1..40 embedding features, embedding_size 8/16/32)")
    hidden = tuple(hp.get("deep_hidden_units") or ())
    if not hidden:
        raise ValueError("MaskNet: deep_hidden_units must name at least one layer of the DNN")
    return order, N, H, ratio, hidden


class MaskNetEngine(Engine):
    """MaskNet (arXiv 2102.07619): instance-guided masks multiply a LayerNorm'ed embedding (or the previous block's
    output), a dense layer, a LayerNorm and a ReLU follow; the blocks feed the DNN.  final = DNN logit (+ linear if
    use_linear, the default).  Nothing in the reference implements it.  x = [flatten(E) | dense] of width K:
        mask_n(x) = relu(x agg_n + agg_b_n) proj_n + proj_b_n              [K,A] then [A,Wout], A = max(1,
                                                                            round(reduction_ratio * Wout))
        V[f,:]    = ln_emb_gamma[f,:] o LN(E[f,:]) + ln_emb_beta[f,:]       (per field row; eps 1e-5, biased variance)
        embedding block (Wout = F D):  h_n = relu(LN_H((mask_n(x) o V) hidden_n))          hidden_n [F D, H], no bias
        block on a block (Wout = H):   h_n = relu(LN_H((mask_n(x) o h_{n-1}) hidden_n))    hidden_n [H, H]
    block_order "parallel": num_blocks embedding blocks share one V, DNN([h_1 | .. | h_N | dense]);  "serial": block 1
    on the embedding, blocks 2..N each on their predecessor, DNN([h_N | dense]).
    Variables (names chosen here): ln_emb_gamma / ln_emb_beta [F,D], block{n}_agg_weights / _agg_bias,
    block{n}_proj_weights / _proj_bias, block{n}_hidden_weights, block{n}_ln_gamma / _ln_beta [H] (n = 1..N), the DNN's
    dnn_*.  Gains start at one ("ones"), weights glorot, l2 key deep_l2_reg on the weight matrices.  No bias tables.
    The normalise-and-mask passes are csrc/masknet.hip; the dense layers run one by one on ops.dense_fwd /
    ops.dense_wgrad (bias + ReLU in the aggregation layer's epilogue, the bf16x6 path under dense_gemm).  The N
    aggregation layers are NOT batched into one GEMM: each block's weights are a variable of their own, so no
    [K, N A] matrix exists to multiply by."""

    model = "masknet"
    use_bias_tables = False
    shardable = False

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, hp, task, device)
        self.use_linear = bool(hp.get("use_linear", True))
        F, D, FD, Dn = self.F, self.D, self.FD, self.Dn
        self.order, self.N, self.H, ratio, hidden = masknet_limits(hp, F, D)
        self.parallel = self.order == "parallel"
        N, H = self.N, self.H
        K = FD + Dn
        self._var("ln_emb_gamma", (F, D), "ones")
        self._var("ln_emb_beta", (F, D))
        l2 = "deep_l2_reg"
        self.wout, self.A = [], []
        for n in range(1, N + 1):
            wout = FD if (self.parallel or n == 1) else H
            A = max(1, round(ratio * wout))
            self.wout.append(wout)
            self.A.append(A)
            self._var(f"block{n}_agg_weights", (K, A), ("glorot", K, A), l2)
            self._var(f"block{n}_agg_bias", (A,))
            self._var(f"block{n}_proj_weights", (A, wout), ("glorot", A, wout), l2)
            self._var(f"block{n}_proj_bias", (wout,))
            self._var(f"block{n}_hidden_weights", (wout, H), ("glorot", wout, H), l2)
            self._var(f"block{n}_ln_gamma", (H,), "ones")
            self._var(f"block{n}_ln_beta", (H,))
        self.dense_gemm = hp.get("dense_gemm", "bf16x6")
        # (the DNN reads the blocks' outputs, not [E | dense]; its dX is no table-row gradient)
        self.mlp = self._dnn((N if self.parallel else 1) * H, Dn, hidden, "relu", stream_d_rows=False)

    def _alloc_model(self, B):
        dev, H, N = self.device, self.H, self.N
        K = self.FD + self.Dn

        def buf(w):
            return torch.empty(B, w, dtype=F32, device=dev)

        # per block: the aggregation layer's output T (rows padded to a multiple of 4 floats), the mask M, the masked
        # input Y (later dY, then dM, in place) and the hidden layer's output Z
        self.T = [buf((a + 3) // 4 * 4)[:, :a] for a in self.A]
        self.dT = buf((max(self.A) + 3) // 4 * 4)
        self.M = [buf(w) for w in self.wout]
        self.Y = [buf(w) for w in self.wout]
        self.Z = [buf(H) for _ in range(N)]
        self.dZ = buf(H)
        nx = N if self.parallel else 1
        self.X = buf(nx * H)
        self.dX = buf(nx * H)
        if not self.parallel:
            # h_1 .. h_{N-1} (h_N is X) and the gradient that comes back to each
            self.hs = [buf(H) for _ in range(N - 1)]
            self.dhs = [buf(H) for _ in range(N - 1)]
        self.dx_tmp = buf(self.FD)
        self.group_ws = torch.empty(max(4, ops.masknet_group_bwd_workspace(B, self.F, self.D)), dtype=F32, device=dev)
        self.row_ws = torch.empty(max(4, ops.masknet_row_bwd_workspace(B, H)), dtype=F32, device=dev)
        # the dense kernels' workspaces, sized for the widest block of either kind
        a_e = max(a for a, w in zip(self.A, self.wout) if w == self.FD)
        chains = [[K, a_e, self.FD, H]]
        if any(w == H for w in self.wout):
            chains.append([K, max(a for a, w in zip(self.A, self.wout) if w == H), H, H])
        wss = [_dense_workspaces(c, B, dev, self.dense_gemm) for c in chains]
        self._fws, self._wws, self._fws6, self._wws6 = (
            None if any(w[i] is None for w in wss) else max((w[i] for w in wss), key=lambda t: t.numel())
            for i in range(4))

    def _bp(self, d, n):
        """Block n's (1-based) variables out of the params or the grads dict."""
        p = f"block{n}_"
        return (d[p + "agg_weights"], d[p + "agg_bias"], d[p + "proj_weights"], d[p + "proj_bias"],
                d[p + "hidden_weights"], d[p + "ln_gamma"], d[p + "ln_beta"])

    def _mask_fwd(self, n, xe, xd):
        """M[n-1] = relu(x agg + agg_b) proj + proj_b."""
        Wa, ba, Wp, bp = self._bp(self.params, n)[:4]
        T = self.T[n - 1]
        ops.dense_fwd(xe, xd, Wa, T, self._fws, bias=ba, act="relu", ws6=self._fws6)
        ops.dense_fwd(T, None, Wp, self.M[n - 1], self._fws, bias=bp, act="identity", ws6=self._fws6)

    def _hidden_fwd(self, n, out):
        """out = relu(LN_H(Y[n-1] hidden))."""
        Wh, g, b = self._bp(self.params, n)[4:]
        ops.dense_fwd(self.Y[n - 1], None, Wh, self.Z[n - 1], self._fws, act="identity", ws6=self._fws6)
        ops.masknet_row_fwd(self.Z[n - 1], g, b, out)

    def _blocks_fwd(self, dense):
        B, H, N = self.E.shape[0], self.H, self.N
        xe, xd = self.E.view(B, self.FD), dense if self.Dn else None
        p = self.params
        if self.parallel:
            for n in range(1, N + 1):
                self._mask_fwd(n, xe, xd)
            ops.masknet_group_fwd(self.E, p["ln_emb_gamma"], p["ln_emb_beta"], self.M, self.Y)
            for n in range(1, N + 1):
                self._hidden_fwd(n, self.X[:, (n - 1) * H: n * H])
            return
        outs = self.hs + [self.X]
        self._mask_fwd(1, xe, xd)
        ops.masknet_group_fwd(self.E, p["ln_emb_gamma"], p["ln_emb_beta"], self.M[:1], self.Y[:1])
        self._hidden_fwd(1, outs[0])
        for n in range(2, N + 1):
            self._mask_fwd(n, xe, xd)
            ops.masknet_group_fwd(outs[n - 2], None, None, [self.M[n - 1]], [self.Y[n - 1]], normalize=False)
            self._hidden_fwd(n, outs[n - 1])

    def _branches_fwd(self, idx, dense, training, masks, lin_w):
        m = self._embed_plain(idx, dense, training, masks, lin_w)
        self._blocks_fwd(dense)
        branches = [(self.lin_logit, 1.0)] if self.use_linear else []
        self.dnn_logit = self._mlp_last(self.mlp, self.X, dense if self.Dn else None, self._dnn_keep(training),
                                        m.get("dnn"), list(branches))
        branches.append((self.dnn_logit, 1.0))
        return branches

    def _hidden_bwd(self, n, dh):
        """dh = dLoss/dh_n -> the hidden layer's and LN_H's gradients; Y[n-1] <- dLoss/dY."""
        Wh, g, b = self._bp(self.params, n)[4:]
        dWh, dg, db = self._bp(self.grads, n)[4:]
        ops.masknet_row_bwd(self.Z[n - 1], g, b, dh, self.dZ, dg, db, self.row_ws)
        ops.dense_wgrad(self.Y[n - 1], None, self.dZ, dWh, self._wws, ws6=self._wws6)
        ops.dense_fwd(self.dZ, None, Wh, self.Y[n - 1], self._fws, transposed=True, epilogue=ops.DENSE_ADD,
                      ws6=self._fws6)

    def _dx_next(self):
        """The buffer the next pass writes the accumulated dLoss/dE to (never the one it reads, self._dx): the two
        alternate so that the last of the N + 1 passes lands in d_rows."""
        B = self.E.shape[0]
        d_rows = self.d_rows.view(B, self.FD)
        if self._dx is None:
            return d_rows if self.N % 2 == 0 else self.dx_tmp
        return self.dx_tmp if self._dx.data_ptr() == d_rows.data_ptr() else d_rows

    def _mask_bwd(self, n, xe, xd):
        """Y[n-1] holds dLoss/dM_n: the two mask layers' gradients, and the mask's share of dLoss/dE."""
        Wa, _, Wp, _ = self._bp(self.params, n)[:4]
        dWa, dba, dWp, dbp = self._bp(self.grads, n)[:4]
        T, dM = self.T[n - 1], self.Y[n - 1]
        dT = self.dT[:, : T.shape[1]]
        ops.dense_wgrad(T, None, dM, dWp, self._wws, db=dbp, ws6=self._wws6)
        ops.dense_fwd(dM, None, Wp, dT, self._fws, transposed=True, epilogue=ops.DENSE_MUL_ACTGRAD, act="relu",
                      aux1=T, ws6=self._fws6)
        ops.dense_wgrad(xe, xd, dT, dWa, self._wws, db=dba, ws6=self._wws6)
        # (the dense features are inputs: no gradient for them)
        dst = self._dx_next()
        ops.dense_fwd(dT, None, Wa[: self.FD], dst, self._fws, transposed=True, epilogue=ops.DENSE_ADD,
                      aux1=self._dx, ws6=self._fws6)
        self._dx = dst

    def _group_bwd(self, n_masks):
        p, gr = self.params, self.grads
        dst = self._dx_next()
        shape = tuple(self.E.shape)
        ops.masknet_group_bwd(self.E, p["ln_emb_gamma"], p["ln_emb_beta"], self.M[:n_masks], self.Y[:n_masks],
                              self.Y[:n_masks], dst.view(shape), gr["ln_emb_gamma"], gr["ln_emb_beta"], self.group_ws,
                              dE_up=None if self._dx is None else self._dx.view(shape))
        self._dx = dst

    def _branches_bwd(self, idx, dense, g, masks):
        B, H, N = self.E.shape[0], self.H, self.N
        xe, xd = self.E.view(B, self.FD), dense if self.Dn else None
        self.mlp.backward(g, self.dX)
        self._dx = None
        if self.parallel:
            for n in range(1, N + 1):
                self._hidden_bwd(n, self.dX[:, (n - 1) * H: n * H])
            self._group_bwd(N)
            for n in range(1, N + 1):
                self._mask_bwd(n, xe, xd)
        else:
            outs, douts = self.hs + [self.X], self.dhs + [self.dX]
            for n in range(N, 1, -1):
                self._hidden_bwd(n, douts[n - 1])
                ops.masknet_group_bwd(outs[n - 2], None, None, [self.M[n - 1]], [self.Y[n - 1]], [self.Y[n - 1]],
                                      douts[n - 2], normalize=False)
                self._mask_bwd(n, xe, xd)
            self._hidden_bwd(1, douts[0])
            self._group_bwd(1)
            self._mask_bwd(1, xe, xd)
        # no other branch reads E: d_rows IS dLoss/dE
        assert self._dx.data_ptr() == self.d_rows.data_ptr()

    def roofline_probes(self, idx, dense, y):
        self._probe_fill(idx, dense, y)  # E, M, Y (= dM), Z, dX
        B, F, D, H, FD = idx.shape[0], self.F, self.D, self.H, self.FD
        p = self.params
        n = self.N if self.parallel else 1
        M, Y = self.M[:n], [torch.empty_like(t) for t in self.Y[:n]]
        dY = [torch.randn_like(t) for t in Y]
        d_rows = torch.empty_like(self.d_rows)
        dg, db = torch.empty_like(p["ln_emb_gamma"]), torch.empty_like(p["ln_emb_beta"])
        g1, b1 = p["block1_ln_gamma"], p["block1_ln_beta"]
        dg1, db1 = torch.empty_like(g1), torch.empty_like(b1)
        h, dZ = torch.empty_like(self.Z[0]), torch.empty_like(self.Z[0])
        dh = self.dX[:, :H]
        shape = f"F={F} D={D} N={n}"
        return self._probes(
            idx, dense, y,
            (f"masknet_group_bwd_kernel (rm_masknet_group_bwd, {shape}: E, M_n, dY_n in, dM_n, d_rows out)",
             "masknet_group_bwd_kernel",
             lambda: ops.masknet_group_bwd(self.E, p["ln_emb_gamma"], p["ln_emb_beta"], M, dY, dY, d_rows, dg, db,
                                           self.group_ws),
             4.0 * (B * FD * (2 + 3 * n) + 4 * FD), "hbm"),
            (f"masknet_group_fwd_kernel (rm_masknet_group_fwd, {shape}: E and M_n in, Y_n out)",
             "masknet_group_fwd_kernel",
             lambda: ops.masknet_group_fwd(self.E, p["ln_emb_gamma"], p["ln_emb_beta"], M, Y),
             4.0 * (B * FD * (1 + 2 * n) + 2 * FD), "hbm"),
            (f"masknet_row_bwd_kernel (rm_masknet_row_bwd, H={H}: Z and dh in, dZ out)", "masknet_row_bwd_kernel",
             lambda: ops.masknet_row_bwd(self.Z[0], g1, b1, dh, dZ, dg1, db1, self.row_ws),
             4.0 * (3 * B * H + 4 * H), "hbm"),
            (f"masknet_row_fwd_kernel (rm_masknet_row_fwd, H={H}: Z in, h out)", "masknet_row_fwd_kernel",
             lambda: ops.masknet_row_fwd(self.Z[0], g1, b1, h), 4.0 * (2 * B * H + 2 * H), "hbm"))


def entire_space_pair(hp, names, types):
    """hp["entire_space"] = (ctr task, cvr task) -> their indices (c, v) for rm_multitask_loss_es; (-1, -1) without
    it.  A ValueError unless it names two distinct classification tasks (ESMM, Ma et al., SIGIR 2018)."""
    es = hp.get("entire_space")
    if es is None:
        return (-1, -1)
    es = tuple(es) if isinstance(es, (list, tuple)) else (es,)
    if (len(es) != 2 or es[0] == es[1] or any(n not in names for n in es)
            or any(types[names.index(n)] != "classification" for n in es)):
        raise ValueError(f"MMoE: entire_space={hp.get('entire_space')!r} must name two distinct classification tasks "
                         f"of task_names {names!r}: (the click task, the conversion task)")
    return names.index(es[0]), names.index(es[1])


def _multitask_loss_step(e, y):
    """The loss head of a training step of a multi-task engine `e` on labels y [B, T]: rm_multitask_loss, or - with
    hp["entire_space"] - rm_multitask_loss_es."""
    kw = dict(Y=y, task_weights=e.task_weights, grad_scale=e.grad_scale, dlogit=e.dlogit, n_t=e.n_t, loss_t=e.loss_t,
              loss=e.loss, workspace=e.loss_ws)
    if e.es == (-1, -1):
        ops.multitask_loss(e.logit, e.task_types, e.pred, **kw)
    else:
        ops.multitask_loss_es(e.logit, e.task_types, e.pred, es=e.es, **kw)


def mmoe_limits(hp):
    """MMoE's limits in one place (th.MMoE checks them at construction, MMoEEngine when it is built): a ValueError
    naming the limit, or (task_names, task_types, task_weights, num_experts, expert_hidden_units, tower_hidden_units)."""
    names = tuple(hp.get("task_names") or ("ctr", "cvr"))
    types = tuple(hp.get("task_types") or ("classification",) * len(names))
    weights = hp.get("task_weights")
    weights = (1.0,) * len(names) if weights is None else tuple(float(w) for w in weights)
    limits = ("1..8 tasks with one name, type and weight each, num_experts 1..16, expert_hidden_units multiples of 4 "
              "with the last in 4..512, a non-empty tower_hidden_units")
    if not 1 <= len(names) <= 8:
        raise ValueError(f"MMoE: {len(names)} tasks ({limits})")
    if len(types) != len(names) or len(weights) != len(names):
        raise ValueError(f"MMoE: task_names, task_types and task_weights differ in length: {len(names)}, {len(types)}, "
                         f"{len(weights)} ({limits})")
    if len(set(names)) != len(names) or not all(isinstance(n, str) and n for n in names):
        raise ValueError(f"MMoE: task_names {names!r} must be distinct non-empty strings")
    for t in types:
        if t not in ops.TASK_TYPES:
            raise ValueError(f"MMoE: task type {t!r} is neither 'classification' nor 'regression'")
    E = hp.get("num_experts", 8)
    if not isinstance(E, int) or not 1 <= E <= 16:
        raise ValueError(f"MMoE: num_experts={E!r} ({limits})")
    experts = tuple(int(h) for h in (hp.get("expert_hidden_units", (256, 128)) or ()))
    towers = tuple(int(h) for h in (hp.get("tower_hidden_units", (64,)) or ()))
    if not experts or any(h < 4 or h % 4 for h in experts) or not ops.MMOE_H_MIN <= experts[-1] <= ops.MMOE_H_MAX:
        raise ValueError(f"MMoE: expert_hidden_units={experts!r} ({limits})")
    if not towers or any(h < 1 for h in towers):
        raise ValueError(f"MMoE: tower_hidden_units={towers!r}: every task tower needs at least one hidden layer "
                         f"({limits})")
    return names, types, weights, E, experts, towers


def ple_limits(hp):
    """PLE's limits in one place (th.MMoE checks them at construction, PLEEngine when it is built): a ValueError naming
    the limit, or (task_names, task_types, task_weights, task_experts S, shared experts C, num_levels L,
    expert_hidden_units, tower_hidden_units).  The tasks and the units are under mmoe_limits."""
    names, types, weights, _, experts, towers = mmoe_limits({**hp, "num_experts": 1})
    S, C, L = hp.get("task_experts", 0), hp.get("num_experts", 2), hp.get("num_levels", 1)
    limits = ("PLE: task_experts 1..4 per task, num_experts (the shared experts of a level) 1..8, "
              "tasks x task_experts + num_experts <= 32, num_levels 1..4; task_experts=0 with num_levels=1 is MMoE")
    if not isinstance(L, int) or isinstance(L, bool) or not 1 <= L <= 4:
        raise ValueError(f"MMoE: num_levels={L!r} ({limits})")
    if not isinstance(S, int) or isinstance(S, bool) or not 1 <= S <= 4:
        raise ValueError(f"MMoE: task_experts={S!r} with num_levels={L!r} ({limits})")
    if not isinstance(C, int) or isinstance(C, bool) or not 1 <= C <= 8:
        raise ValueError(f"MMoE: num_experts={C!r} with task_experts={S!r} ({limits})")
    if len(names) * S + C > 32:
        raise ValueError(f"MMoE: {len(names)} tasks x task_experts={S} + num_experts={C} = {len(names) * S + C} "
                         f"experts per level ({limits})")
    return names, types, weights, S, C, L, experts, towers


class _MultiTaskEngine(Engine):
    """The body of MMoEEngine and PLEEngine: T tasks over one set of embedding tables, L levels of N = T S + C stacked
    experts (S per task, then C shared) mixed by T task gates and - on every level but the last - one shared gate,
    then one tower per task and the loss head for several labels.  MMoE is S = 0, L = 1.  A subclass gives `model`,
    `who` (the prefix of its messages), its limits as (names, types, weights, S, C, L, expert units, tower units),
    the prefix of a level's variable names, and its pair of mixture ops; its docstring has the arithmetic and the
    variable names."""

    use_bias_tables = False
    shardable = False

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, hp, task, device)
        self.use_linear = False
        (self.task_names, self.task_types, self.task_weights, self.S, self.C, self.L, self.expert_units,
         self.tower_units) = self._limits(hp)
        self.es = entire_space_pair(hp, self.task_names, self.task_types)
        if hp.get("strict_reference"):
            raise NotImplementedError(f"{self.who}: strict_reference reproduces quirks of the reference, which has no "
                                      "multi-task model")
        for key in ("deep_dropout", "expert_dropout", "tower_dropout"):
            keep = hp.get(key)
            if keep is not None and any(float(k) != 1.0 for k in keep):
                raise NotImplementedError(f"{self.who}: {key}={keep!r}: the experts and towers run without dropout")
        T, S, C, units = len(self.task_names), self.S, self.C, self.expert_units
        self.T, self.H, self.N, self.W, self.NE = T, units[-1], T * S + C, S + C, C  # (NE: hp["num_experts"])
        self._check_mix()
        self.act = act_name(hp.get("deep_activation", "relu"))
        self.dense_gemm = hp.get("dense_gemm", "bf16x6")
        K0, N, H = self.FD + self.Dn, self.N, self.H
        self.K0 = K0
        self._gemms = []
        for l in range(self.L):
            K, AW, pre = (K0 if l == 0 else H), self._aw(l), self._prefix(l)
            self._var(f"{pre}expert_layer_0_weights", (K, N * units[0]), ("glorot", K, units[0]), "deep_l2_reg")
            self._var(f"{pre}expert_layer_0_bias", (N * units[0],))
            for k in range(1, len(units)):
                self._var(f"{pre}expert_layer_{k}_weights", (N, units[k - 1], units[k]),
                          ("glorot", units[k - 1], units[k]), "deep_l2_reg")
                self._var(f"{pre}expert_layer_{k}_bias", (N, units[k]))
            self._var(f"{pre}gate_weights", (K, AW), ("glorot", K, self.W), "deep_l2_reg")
            # the GEMM shapes (K, N) of this level: the workspaces are sized for the largest
            self._gemms += [(K, N * units[0]), (K, AW)] + [(units[k - 1], units[k]) for k in range(1, len(units))]
        self.towers = [self._dnn(H, 0, self.tower_units, "relu", prefix=f"{n}_", stream_d_rows=False)
                       for n in self.task_names]

    # ------------------------------------------------------------------ the layout of a level
    def _sg(self, l):
        """shared_gate of level l: every level but the last."""
        return int(l < self.L - 1)

    def _aw(self, l):
        return ops.cgc_widths(self.T, self.S, self.C, self._sg(l))[1]

    def _group(self, s, h):
        """The columns of group s (a task's experts, s = T: the shared ones) in a stacked buffer of expert width h."""
        first = s * self.S
        return first * h, (first + (self.S if s < self.T else self.C)) * h

    def _gate(self, g):
        """The columns of gate g (g = T: the shared gate) in A."""
        return (g * self.W, (g + 1) * self.W) if g < self.T else (self.T * self.W, self.T * self.W + self.N)

    def _stream(self, buf, s):
        return buf[:, s * self.H: (s + 1) * self.H]

    @staticmethod
    def _ws6(ws6, *operands):
        """The split-operand GEMMs load and store whole float4s of their activation, gradient and output rows: they
        take only 16-byte aligned column ranges (with S + C no multiple of 4 a gate starts unaligned in A; it runs on
        the plain kernels).  The weights are read, and their gradients written, element by element on both paths."""
        ok = all(t is None or (t.data_ptr() % 16 == 0 and (t.dim() < 2 or t.stride(0) % 4 == 0 or t.shape[0] == 1))
                 for t in operands)
        return ws6 if ok else None

    def _alloc_model(self, B):
        dev, N, T, H, L = self.device, self.N, self.T, self.H, self.L
        buf = lambda *shape: torch.empty(*shape, dtype=F32, device=dev)  # noqa: E731
        pad4 = lambda n: (n + 3) // 4 * 4  # noqa: E731  (the mixture kernels take rows of whole float4s)
        # per level: the stacked expert activations (Z = ha[l][-1]) and dLoss/d(pre-activation) of the same
        self.ha = [[buf(B, N * h) for h in self.expert_units] for _ in range(L)]
        self.dha = [[buf(B, N * h) for h in self.expert_units] for _ in range(L)]
        self.A = [buf(B, pad4(self._aw(l)))[:, : self._aw(l)] for l in range(L)]
        self.dA = [buf(B, pad4(self._aw(l)))[:, : self._aw(l)] for l in range(L)]
        self.M = [buf(B, (T + self._sg(l)) * H) for l in range(L)]
        self.dM = [buf(B, (T + self._sg(l)) * H) for l in range(L)]
        self.P = None                                            # gate weights of one level: made by gate_weights()
        self.dx = buf(B, self.FD)
        self.dxg = buf(B, H) if L > 1 else None                  # a gate's input gradient, before its experts' is added
        self.logit, self.pred, self.dlogit = buf(T, B), buf(T, B), buf(T, B)
        self.n_t = torch.zeros(T, dtype=I64, device=dev)
        self.loss_t = torch.zeros(T, dtype=F32, device=dev)
        self.loss_ws = buf(ops.multitask_loss_workspace(B, T))
        # a tower on the fused skinny-MLP kernels reads and writes contiguous rows: its own copy of M_t / dM_t
        copies = T > 1
        self.Mc = [buf(B, H) if (copies and tw.fused_ok) else None for tw in self.towers]
        self.dMc = [buf(B, H) if (copies and tw.fused_ok) else None for tw in self.towers]
        for t, tw in enumerate(self.towers):
            tw._alloc(B, dev)
            tw.out = self.logit[t].view(B, 1)  # the tower's logit lands in its row of the [T, B] buffer
        side = max(d for kn in self._gemms for d in kn)
        self._fws = buf(max(ops.dense_filter_workspace(max(k, n), max(k, n)) for k, n in self._gemms))
        self._wws = buf(max(1, max(ops.dense_wgrad_workspace(k, n, B) for k, n in self._gemms)))
        self._fws6 = self._wws6 = None
        if self.dense_gemm == "bf16x6":
            self._fws6 = buf(ops.dense6_workspace(side, side, B))
            self._wws6 = buf(max(ops.dense_wgrad6_workspace(k, n, B) for k, n in self._gemms))

    def _fwd(self, a1, a2, W, out, **kw):
        ops.dense_fwd(a1, a2, W, out, self._fws, ws6=self._ws6(self._fws6, a1, out, kw.get("aux1")), **kw)

    def _wgrad(self, a1, a2, G, dW, db=None):
        ops.dense_wgrad(a1, a2, G, dW, self._wws, db=db, ws6=self._ws6(self._wws6, a1, G))

    def _tower_in(self, t):
        M_t = self._stream(self.M[-1], t)
        if self.Mc[t] is None:
            return M_t
        self.Mc[t].copy_(M_t)
        return self.Mc[t]

    def _model_fwd(self, idx, dense, p_level=None):
        """Embedding lookup, the extraction levels and the towers: self.logit [T, B].  p_level: the level whose gate
        weights go to self.P."""
        if self.spec.Dn and dense is None:
            raise ValueError(f"{self.who}: the dense features are missing")
        self._embed(idx, dense, False, {}, None)
        p, T, units = self.params, self.T, self.expert_units
        xe, xd = self.E.view(-1, self.FD), (dense if self.Dn else None)
        for l in range(self.L):
            sg, ha, pre = self._sg(l), self.ha[l], self._prefix(l)
            W0, b0, Gw = p[f"{pre}expert_layer_0_weights"], p[f"{pre}expert_layer_0_bias"], p[f"{pre}gate_weights"]
            if l == 0:
                self._fwd(xe, xd, W0, ha[0], bias=b0, act=self.act)
                self._fwd(xe, xd, Gw, self.A[0], act="identity")
            else:
                X = self.M[l - 1]
                for s in range(T + 1):
                    c0, c1 = self._group(s, units[0])
                    self._fwd(self._stream(X, s), None, W0[:, c0:c1], ha[0][:, c0:c1], bias=b0[c0:c1], act=self.act)
                for g in range(T + sg):
                    a0, a1 = self._gate(g)
                    self._fwd(self._stream(X, g), None, Gw[:, a0:a1], self.A[l][:, a0:a1], act="identity")
            for k in range(1, len(units)):
                W, b = p[f"{pre}expert_layer_{k}_weights"], p[f"{pre}expert_layer_{k}_bias"]
                for e in range(self.N):
                    self._fwd(ha[k - 1][:, e * units[k - 1]: (e + 1) * units[k - 1]], None, W[e],
                              ha[k][:, e * units[k]: (e + 1) * units[k]], bias=b[e], act=self.act)
            P = None
            if p_level == l:
                aw = self._aw(l)
                self.P = P = torch.empty(idx.shape[0], (aw + 3) // 4 * 4, dtype=F32, device=self.device)[:, :aw]
            self._mix_fwd(l, P)
        for t, tw in enumerate(self.towers):
            tw.forward(self._tower_in(t), None)

    def forward(self, idx, dense=None, training=False, masks=None, manual_weights=None, mv=None, gate_level=None):
        """-> (logit [T, B], pred [T, B]); pred_t = sigmoid(logit_t) for a classification task, logit_t for a
        regression task.  gate_level = l also leaves the gate weights of level l in self.P (A's layout)."""
        if manual_weights is not None:
            raise NotImplementedError(f"{self.who} has no linear term: manual feature weights do not apply")
        self._alloc(idx.shape[0])
        self._mv = mv
        self._seq_save = bool(training)
        self._model_fwd(idx, dense, p_level=gate_level)
        ops.multitask_loss(self.logit, self.task_types, self.pred)
        return self.logit, self.pred

    def fwd_bwd(self, idx, dense, y, masks=None, mv=None):
        """One training step's forward + backward on labels y [B, T] (float32, NaN = unobserved).  Returns the loss
        tensor [1] (the weighted task losses + the l2 terms); self.loss_t [T] and self.n_t [T] hold the tasks' mean
        losses and observed counts.  Gradients: self.grads, self.d_rows [B,F,D] + idx."""
        B = idx.shape[0]
        self._alloc(B)
        self._mv = mv
        self._seq_save = True
        if y.dtype != F32 or tuple(y.shape) != (B, self.T):
            raise ValueError(f"{self.who}: labels must be float32 [B, {self.T}] (NaN = unobserved), got {y.dtype} "
                             f"{tuple(y.shape)}")
        self._model_fwd(idx, dense)
        _multitask_loss_step(self, y)
        p, g, T, units = self.params, self.grads, self.T, self.expert_units
        ident = self.act == "identity"
        for t, tw in enumerate(self.towers):
            dM_t = self._stream(self.dM[-1], t)
            if self.dMc[t] is None:
                tw.backward(self.dlogit[t], dM_t)
            else:
                tw.backward(self.dlogit[t], self.dMc[t])
                dM_t.copy_(self.dMc[t])
        xe, xd = self.E.view(-1, self.FD), (dense if self.Dn else None)
        for l in range(self.L - 1, -1, -1):
            sg, ha, dha, dA, pre = self._sg(l), self.ha[l], self.dha[l], self.dA[l], self._prefix(l)
            self._mix_bwd(l)
            if not ident:
                ops.act_bwd_(dha[-1], ha[-1], self.act)
            for k in range(len(units) - 1, 0, -1):
                W = p[f"{pre}expert_layer_{k}_weights"]
                gW, gb = g[f"{pre}expert_layer_{k}_weights"], g[f"{pre}expert_layer_{k}_bias"]
                for e in range(self.N):
                    prev = ha[k - 1][:, e * units[k - 1]: (e + 1) * units[k - 1]]
                    da = dha[k][:, e * units[k]: (e + 1) * units[k]]
                    self._wgrad(prev, None, da, gW[e], db=gb[e])
                    self._fwd(da, None, W[e], dha[k - 1][:, e * units[k - 1]: (e + 1) * units[k - 1]],
                              transposed=True, epilogue=ops.DENSE_ADD if ident else ops.DENSE_MUL_ACTGRAD,
                              act=self.act, aux1=None if ident else prev)
            W0, Gw = p[f"{pre}expert_layer_0_weights"], p[f"{pre}gate_weights"]
            gW0, gb0, gG = g[f"{pre}expert_layer_0_weights"], g[f"{pre}expert_layer_0_bias"], g[f"{pre}gate_weights"]
            if l == 0:
                self._wgrad(xe, xd, dha[0], gW0, db=gb0)
                self._wgrad(xe, xd, dA, gG)
                # dLoss/dx of the gates and of the experts, summed into d_rows (the dense inputs need no gradient)
                self._fwd(dA, None, Gw[: self.FD], self.dx, transposed=True, epilogue=ops.DENSE_ADD)
                self._fwd(dha[0], None, W0[: self.FD], self.d_rows.view(-1, self.FD), transposed=True,
                          epilogue=ops.DENSE_ADD, aux1=self.dx)
                continue
            X, dX = self.M[l - 1], self.dM[l - 1]
            for s in range(T + 1):
                xs, dxs = self._stream(X, s), self._stream(dX, s)
                c0, c1 = self._group(s, units[0])
                das = dha[0][:, c0:c1]
                self._wgrad(xs, None, das, gW0[:, c0:c1], db=gb0[c0:c1])
                gated = s < T + sg  # (on the last level the shared stream has experts and no gate)
                if gated:
                    a0, a1 = self._gate(s)
                    self._wgrad(xs, None, dA[:, a0:a1], gG[:, a0:a1])
                    self._fwd(dA[:, a0:a1], None, Gw[:, a0:a1], self.dxg, transposed=True, epilogue=ops.DENSE_ADD)
                # dX_s = the experts' input gradient (+ the gate's, added in the epilogue)
                self._fwd(das, None, W0[:, c0:c1], dxs, transposed=True, epilogue=ops.DENSE_ADD,
                          aux1=self.dxg if gated else None)
        self._add_l2_grads()
        self._seq_bwd()
        return self._add_l2(self.loss)

    def gate_weights(self, idx, dense=None, mv=None, level=-1):
        """The task gates' weights p [B, T, S + C] of a level of a batch (an inference forward with the mixture's
        optional output): per task its own S experts first, then the C shared ones."""
        l = range(self.L)[level]
        self.forward(idx, dense, mv=mv, gate_level=l)
        return self.P[:, : self.T * self.W].reshape(idx.shape[0], self.T, self.W)


class MMoEEngine(_MultiTaskEngine):
    """Multi-gate Mixture-of-Experts (MMoE, Ma et al., KDD 2018): T tasks over one set of embedding tables.  Nothing in
    the reference implements it (it knows one label per example).  x = [E | dense] [B, K0], never concatenated:
        experts e < E:  h_e^0 = x;  h_e^{l+1} = act(h_e^l W_e^l + b_e^l) over expert_hidden_units;  Z_e = h_e^L [B, H]
        gates t < T:    A_t = x G_t [B, E] (no bias, no hidden layer);  p_t = softmax(A_t)
        mixture:        M_t = sum_e p_te Z_e                                         (csrc/multitask.hip)
        towers:         logit_t = DNN_t(M_t), tower_hidden_units + the output projection
        loss = sum_t w_t * mean over the examples whose label t is observed (not NaN) of l_t  + the l2 terms
               (hp["entire_space"] = (ctr task, cvr task): the cvr task through pred_ctr pred_cvr, rm_multitask_loss_es)
    num_experts = 1 is the shared-bottom model.  Layout: the experts are STACKED - layer l of all experts is one
    [B, E H_l] buffer, expert e at columns e H_l ..; layer 0 is one GEMM over x, deeper layers run per expert on the
    column ranges; all gates are one GEMM x -> [B, T E]; M is one [B, T H] buffer whose column range t the tower of
    task t reads in place (a tower narrow enough for the fused skinny-MLP kernels, which take contiguous rows, gets a
    copy).  The gate weights p never reach HBM in training.
    Variables (names chosen here): expert_layer_0_weights [K0, E H_1] / _bias [E H_1]; expert_layer_{l}_weights
    [E, H_l, H_{l+1}] / _bias [E, H_{l+1}] for l >= 1; gate_weights [K0, T E] (task t at columns t E ..); per task the
    tower's "{task}_dnn_layer_{i}_weights" / _bias, "{task}_dnn_w", "{task}_dnn_w0".  Every matrix is glorot with the
    fans of ONE expert or gate and under deep_l2_reg; biases start at zero.  No bias tables, no linear term, no
    dropout, one GPU.  logit / pred / dlogit are [T, B]."""

    model = "mmoe"
    who = "MMoE"

    @staticmethod
    def _limits(hp):
        names, types, weights, E, experts, towers = mmoe_limits(hp)
        return names, types, weights, 0, E, 1, experts, towers

    @staticmethod
    def _prefix(l):
        return ""

    def _check_mix(self):
        if not ops.mmoe_mix_supported(self.NE, self.T, self.H):
            raise ValueError(f"MMoE: {self.NE} experts, {self.T} tasks, expert width {self.H} are not supported by "
                             f"rm_mmoe_mix_fwd ({ops.MMOE_LIMITS})")

    def _mix_fwd(self, l, P):
        ops.mmoe_mix_fwd(self.ha[l][-1], self.A[l], self.NE, self.T, self.M[l], P=P)

    def _mix_bwd(self, l):
        ops.mmoe_mix_bwd(self.ha[l][-1], self.A[l], self.NE, self.T, self.dM[l], self.dha[l][-1], self.dA[l])


class PLEEngine(_MultiTaskEngine):
    """Progressive Layered Extraction (PLE, Tang et al., RecSys 2020; one level is CGC, Customized Gate Control): T
    tasks over one set of embedding tables, with task-specific experts beside the shared ones and L = num_levels
    extraction levels.  Nothing in the reference implements it.  Streams s = 0..T-1 are the tasks', s = T the shared
    one; X_s^0 = x = [E | dense] [B, K0], never concatenated.  Per level l, N = T S + C experts (S per task, then C
    shared), group s = the experts of stream s:
        experts of group s:  a DNN of expert_hidden_units over X_s^l (bias, deep_activation)  ->  Z^l [B, N H]
        gates g:             A_g = X_g^l G_g^l (no bias); task gate t over its own S experts and the C shared ones,
                             and - on every level but the last - the shared gate g = T over all N
        mixture:             X_g^{l+1} = M_g = sum_e p_ge Z_e, p_g = softmax(A_g)            (csrc/multitask.hip)
        towers:              logit_t = DNN_t(X_t^L), tower_hidden_units + the output projection
        loss: MMoEEngine's; with hp["entire_space"] = (ctr task, cvr task) the cvr task is trained through
              pred_ctr pred_cvr over all impressions (rm_multitask_loss_es)
    Layout: the experts of a level are STACKED as in MMoEEngine - layer k of all experts is one [B, N H_k] buffer,
    expert e at columns e H_k ..  Level 0: layer 0 is one GEMM over x, all gates are one GEMM.  Levels >= 1: the
    experts and the gate of stream s read column range s of the previous level's M in place - one GEMM per group for
    layer 0, one per gate.  Deeper layers run per expert on the column ranges.  In the backward dX_s^l is the sum of
    the input gradients of group s's experts and of gate s: the second GEMM adds the first one's result in its
    epilogue.  The gate weights p never reach HBM in training.
    Variables (names chosen here), per level l with K = K0 at level 0 and H above:
        level_{l}_expert_layer_0_weights [K, N H_1] / _bias [N H_1] (expert e at columns e H_1 ..);
        level_{l}_expert_layer_{k}_weights [N, H_k, H_{k+1}] / _bias [N, H_{k+1}] for k >= 1;
        level_{l}_gate_weights [K, T (S + C) + shared_gate N] (rm_cgc_mix_fwd's layout of A);
        per task the tower's "{task}_dnn_layer_{i}_weights" / _bias, "{task}_dnn_w", "{task}_dnn_w0".
    Every matrix is glorot with the fans of ONE expert or gate (a gate's fan-out is S + C) and under deep_l2_reg;
    biases start at zero.  No bias tables, no linear term, no dropout, one GPU.  logit / pred / dlogit are [T, B]."""

    model = "ple"
    who = "PLE"
    _limits = staticmethod(ple_limits)

    @staticmethod
    def _prefix(l):
        return f"level_{l}_"

    def _check_mix(self):
        if not ops.cgc_mix_supported(self.T, self.S, self.C, self.H, 1):
            raise ValueError(f"PLE: {self.T} tasks, {self.S} task experts, {self.C} shared experts, expert width "
                             f"{self.H} are not supported by rm_cgc_mix_fwd ({ops.CGC_LIMITS})")

    def _mix_fwd(self, l, P):
        ops.cgc_mix_fwd(self.ha[l][-1], self.A[l], self.T, self.S, self.C, self._sg(l), self.M[l], P=P)

    def _mix_bwd(self, l):
        ops.cgc_mix_bwd(self.ha[l][-1], self.A[l], self.T, self.S, self.C, self._sg(l), self.dM[l], self.dha[l][-1],
                        self.dA[l])


def _one_run(positions, what, side):
    """positions (sorted) must be one contiguous run -> (first, last + 1); (0, 0) when empty."""
    if not positions:
        return 0, 0
    if positions[-1] - positions[0] + 1 != len(positions):
        raise ValueError(f"TwoTower: the {what} features of the {side} tower are not one contiguous run of the "
                         f"FeatureDictionary's {what} features (positions {positions}): each tower reads its columns "
                         "of the batch in place, so order the dictionary with every user feature before every item "
                         "feature (or the other way round)")
    return positions[0], positions[-1] + 1


def twotower_limits(hp, spec=None):
    """TwoTower's limits in one place (th.TwoTower checks them at construction, before any GPU work, TwoTowerEngine
    when it is built): a ValueError naming the limit (NotImplementedError for a sequence feature), or a dict with H,
    user_units, item_units, scale and - with spec, a FeatureSpec - `user` / `item` = (a, b, c, d): the tower reads the
    embedding features [a, b) and the dense columns [c, d); id_col the column of idx of item_id_feature (or None)."""
    user = tuple(hp.get("user_features") or ())
    item = tuple(hp.get("item_features") or ())
    uu = tuple(int(h) for h in (hp.get("user_hidden_units", (256, 128)) or ()))
    iu = tuple(int(h) for h in (hp.get("item_hidden_units", (256, 128)) or ()))
    limits = (f"the last units of both towers equal, a multiple of 4 in {ops.IBS_H_MIN}..{ops.IBS_H_MAX}; "
              "temperature > 0; user_features and item_features partition the FeatureDictionary")
    if not uu or not iu or any(h < 1 for h in uu + iu):
        raise ValueError(f"TwoTower: user_hidden_units={uu!r}, item_hidden_units={iu!r}: every tower needs at least "
                         f"its output layer ({limits})")
    H = uu[-1]
    if iu[-1] != H:
        raise ValueError(f"TwoTower: the towers end in {uu[-1]} and {iu[-1]} units: both embeddings must have the same "
                         f"width ({limits})")
    if H % 4 or not ops.IBS_H_MIN <= H <= ops.IBS_H_MAX:
        raise ValueError(f"TwoTower: embedding width {H} ({limits})")
    temp = hp.get("temperature", 0.05)
    if not isinstance(temp, (int, float)) or not temp > 0 or temp != temp or temp == float("inf"):
        raise ValueError(f"TwoTower: temperature={temp!r} must be a positive finite number ({limits})")
    if not user or not item:
        raise ValueError(f"TwoTower: user_features={user!r}, item_features={item!r}: both towers need features "
                         f"({limits})")
    both = sorted(set(user) & set(item))
    if both or len(set(user)) != len(user) or len(set(item)) != len(item):
        raise ValueError(f"TwoTower: features {both or list(user + item)} are named twice ({limits})")
    idf = hp.get("item_id_feature")
    masking, logq = bool(hp.get("mask_accidental_hits", True)), bool(hp.get("logq_correction", False))
    if idf is None and (masking or logq):
        raise ValueError("TwoTower: mask_accidental_hits / logq_correction need item_id_feature, the SparseFeat of the "
                         "item tower that identifies the item")
    if idf is not None and idf not in item:
        raise ValueError(f"TwoTower: item_id_feature={idf!r} is not one of item_features {item!r}")
    out = dict(H=H, user_units=uu, item_units=iu, scale=1.0 / float(temp), id_col=None)
    if spec is None:
        return out
    if spec.seq_names:
        raise NotImplementedError(f"TwoTower: sequence features {spec.seq_names} are not supported: a history's "
                                  "query would cross the towers")
    known = list(spec.sparse_names) + list(spec.dense_names)
    named = set(user) | set(item)
    missing, unknown = [n for n in known if n not in named], sorted(named - set(known))
    if missing or unknown:
        raise ValueError(f"TwoTower: user_features and item_features must partition the FeatureDictionary: "
                         f"{missing} are in neither list, {unknown} are not in the dictionary")
    for side, names in (("user", user), ("item", item)):
        a, b = _one_run([j for j, n in enumerate(spec.sparse_names) if n in names], "embedding", side)
        c, d = _one_run([j for j, n in enumerate(spec.dense_names) if n in names], "dense", side)
        if b == a:
            raise ValueError(f"TwoTower: the {side} tower has no embedding feature (it needs at least one)")
        out[side] = (a, b, c, d)
    if idf is not None:
        if idf not in spec.sparse_names or idf in spec.scratch_names:
            raise ValueError(f"TwoTower: item_id_feature={idf!r} must be a plain SparseFeat (not a dense, multi-valued "
                             "or value feature)")
        out["id_col"] = spec.sparse_names.index(idf)
    return out


class TwoTowerEngine(Engine):
    """Two-tower retrieval (DSSM / YouTube-DNN; the logQ correction of Yi et al., RecSys 2019).  Nothing in the
    reference implements it: every model of it scores one (user, item) row.  x = [E | dense] [B, K0], never
    concatenated; the user tower reads its columns (E.view(B, FD)[:, a D : b D], dense[:, c : d]) in place, the item
    tower its own:
        u = tower_user(x_user), v = tower_item(x_item): hidden layers with deep_activation, a final linear layer to H
        normalize: u <- u / max(|u|, 1e-12), the same for v                                (rm_rownorm_fwd)
        S_ij = <u_i, v_j> / temperature - logq[item_j];  accidental hits (item_j == item_i, j != i) masked out
        loss = sum_i w_i (logsumexp_j S_ij - S_ii) / sum_i w_i  + the l2 terms             (rm_inbatch_softmax_fwd)
    Labels y [B] (0/1), when given, are the row weights w: a row with 0 has no loss term of its own, its item still
    serves as a negative.  The [B, B] scores never reach HBM (csrc/inbatch.hip).  Variables: user_dnn_layer_{l}_weights
    / _bias, item_dnn_layer_{l}_weights / _bias (glorot / zeros, deep_l2_reg on every matrix) and item_logq [V of
    item_id_feature], the log sampling probabilities - a table set from data (set_logq), not trained, kept by
    state_dict() / load_params().  hp["col_splits"] (default 0: the library's choice) is handed to the kernels.  No
    bias tables, no linear term, no dropout, one GPU (no row sharding, no cross-device negatives), a fixed temperature,
    no sequence features."""

    model = "twotower"
    use_bias_tables = False
    shardable = False
    EPS = 1e-12

    def __init__(self, spec, embedding_size, hp, task="classification", device="cuda"):
        super().__init__(spec, embedding_size, hp, task, device)
        self.use_linear = False
        if hp.get("strict_reference"):
            raise NotImplementedError("TwoTower: strict_reference reproduces quirks of the reference, which has no "
                                      "retrieval model")
        lim = twotower_limits(hp, spec)
        self.H, self.scale, self.id_col = lim["H"], lim["scale"], lim["id_col"]
        if not ops.inbatch_softmax_supported(self.H):
            raise ValueError(f"TwoTower: embedding width {self.H} is not supported by rm_inbatch_softmax_fwd "
                             f"({ops.IBS_LIMITS})")
        self.normalize = bool(hp.get("normalize", True))
        self.masking = bool(hp.get("mask_accidental_hits", True))
        self.logq_on = bool(hp.get("logq_correction", False))
        self.col_splits = int(hp.get("col_splits", 0))
        self.cols = {s: lim[s] for s in ("user", "item")}
        self.towers = {}
        for side in ("user", "item"):
            a, b, c, d = self.cols[side]
            self.towers[side] = self._adopt(Tower(self.params, self.grads, (b - a) * self.D + (d - c),
                                                  lim[f"{side}_units"], hp.get("deep_activation", "relu"), self.device,
                                                  f"{side}_", dense_gemm=hp.get("dense_gemm", "bf16x6"),
                                                  linear_last=True))
        if self.id_col is not None:
            self._view("item_logq", torch.zeros(spec.feat_sizes[self.id_col], dtype=F32, device=self.device))

    def set_logq(self, logq):
        """The log sampling probability of every encoded id of item_id_feature ([V] floats)."""
        self.params["item_logq"].copy_(torch.as_tensor(logq).to(self.device, F32).reshape(-1))

    def _alloc_model(self, B):
        dev, H = self.device, self.H
        buf = lambda *shape: torch.empty(*shape, dtype=F32, device=dev)  # noqa: E731
        self.emb = {s: buf(B, H) for s in self.towers}      # the normalised embeddings (normalize)
        self.inv = {s: buf(B) for s in self.towers}
        self.d_emb = {s: buf(B, H) for s in self.towers}
        self.lse, self.row_loss = buf(B), buf(B)
        self.rank = torch.zeros(B, dtype=torch.int32, device=dev)
        self.loss_ws = buf(ops.inbatch_softmax_workspace(B, H))
        for tw in self.towers.values():
            tw._alloc(B, dev)

    def _tower_fwd(self, side, dense):
        """The tower of one side over the gathered batch -> its embeddings [B, H]."""
        a, b, c, d = self.cols[side]
        D = self.D
        if d > c and dense is None:
            raise ValueError("TwoTower: the dense features are missing")
        out = self.towers[side].forward(self.E.view(-1, self.FD)[:, a * D: b * D], dense[:, c:d] if d > c else None)
        if not self.normalize:
            return out
        ops.rownorm_fwd(out, self.emb[side], self.inv[side], self.EPS)
        return self.emb[side]

    def embeddings(self, side, idx, dense=None, mv=None):
        """The embeddings [B, H] of one tower ("user" or "item"): only that tower runs (the other side's columns of idx
        and dense are gathered and ignored)."""
        self._alloc(idx.shape[0])
        self._mv = mv
        self._seq_save = False
        self._embed(idx, dense, False, {}, None)
        return self._tower_fwd(side, dense)

    def _side_inputs(self, idx):
        """(item ids or None, logq of the batch's items or None)."""
        col = idx[:, self.id_col].contiguous() if self.id_col is not None else None
        ids = col if self.masking else None
        logq = self.params["item_logq"][col].contiguous() if self.logq_on else None
        return ids, logq

    def _weights(self, y, B):
        if y is None:
            return None
        if y.dtype != F32 or tuple(y.shape) != (B,):
            raise ValueError(f"TwoTower: labels must be float32 [B] (the row weights), got {y.dtype} {tuple(y.shape)}")
        return y

    def forward(self, idx, dense=None, training=False, masks=None, manual_weights=None, mv=None):
        """-> (score [B], score [B]): score_i = <u_i, v_i> / temperature of the row's own pair (no logQ, no
        sigmoid; a row-wise product of the two embedding buffers, summed in double and rounded once)."""
        if manual_weights is not None:
            raise NotImplementedError("TwoTower has no linear term: manual feature weights do not apply")
        u = self.embeddings("user", idx, dense, mv)
        v = self._tower_fwd("item", dense)
        self.pred.copy_(torch.linalg.vecdot(u.double(), v.double()) * self.scale)
        return self.pred, self.pred

    def evaluate_batch(self, idx, dense=None, y=None, mv=None):
        """The forward kernel's outputs for one batch: (loss [1], row_loss [B], rank [B] int32) - engine buffers,
        valid until the next call.  No l2 terms."""
        B = idx.shape[0]
        u = self.embeddings("user", idx, dense, mv)
        v = self._tower_fwd("item", dense)
        ids, logq = self._side_inputs(idx)
        ops.inbatch_softmax_fwd(u, v, self.scale, self.lse, self.row_loss, self.loss, self.loss_ws, item_id=ids,
                                logq=logq, w=self._weights(y, B), rank=self.rank, col_splits=self.col_splits)
        return self.loss, self.row_loss, self.rank

    def fwd_bwd(self, idx, dense, y, masks=None, mv=None):
        """One training step's forward + backward; y [B] float32 row weights or None.  Returns the loss tensor [1]
        (the in-batch softmax loss + the l2 terms).  Gradients: self.grads, self.d_rows [B,F,D] + idx."""
        B = idx.shape[0]
        self._alloc(B)
        self._mv = mv
        self._seq_save = True
        w = self._weights(y, B)
        self._embed(idx, dense, False, {}, None)
        u, v = self._tower_fwd("user", dense), self._tower_fwd("item", dense)
        ids, logq = self._side_inputs(idx)
        kw = dict(item_id=ids, logq=logq, w=w, col_splits=self.col_splits)
        ops.inbatch_softmax_fwd(u, v, self.scale, self.lse, self.row_loss, self.loss, self.loss_ws, rank=self.rank,
                                **kw)
        ops.inbatch_softmax_bwd(u, v, self.scale, self.lse, self.d_emb["user"], self.d_emb["item"], self.loss_ws,
                                grad_scale=self.grad_scale, **kw)
        D = self.D
        for side, tw in self.towers.items():
            g = self.d_emb[side]
            if self.normalize:
                ops.rownorm_bwd(self.emb[side], self.inv[side], g, g)
            a, b, _, _ = self.cols[side]
            tw.backward(g, self.d_rows.view(-1, self.FD)[:, a * D: b * D])
        self._add_l2_grads()
        self._seq_bwd()
        return self._add_l2(self.loss)

    TOPK_WS_FLOATS = 1 << 26  # topk()'s workspace bound: 256 MB

    def topk(self, u, items, k, exclude=None):
        """Exact retrieval (rm_topk_ip): per row of u [n, H] the k rows of the catalogue items [N, H] with the highest
        <u_i, items_j> / temperature (no logQ), sorted by score descending, then row ascending -> (rows int64 [n, k],
        scores float32 [n, k]) device tensors; -1 / -inf past the available rows.  exclude: None or (offsets [n + 1],
        rows) int64 device tensors, the catalogue rows each query must not get back.  The queries go in groups of
        whole 64-row query tiles, as many as keep the workspace within TOPK_WS_FLOATS floats (one tile at the least,
        whose workspace is at most 64 x 64 x 2048 x 2 floats = 64 MiB for k = 1024); the result does not depend on the
        grouping."""
        n, N, H = int(u.shape[0]), int(items.shape[0]), int(items.shape[1])
        if not ops.topk_ip_supported(H, k):
            raise ValueError(f"TwoTower.topk: k={k} with H={H} is not supported by rm_topk_ip ({ops.TOPK_LIMITS})")
        rows = torch.empty(n, k, dtype=torch.int64, device=self.device)
        scores = torch.empty(n, k, dtype=F32, device=self.device)
        if n == 0:
            return rows, scores
        tile = ops.topk_ip_tile(H)
        per_tile = max(1, ops.topk_ip_workspace(tile, N, H, k))
        group = min(n, max(1, self.TOPK_WS_FLOATS // per_tile) * tile)
        ws = torch.empty(ops.topk_ip_workspace(group, N, H, k), dtype=F32, device=self.device)
        off = None if exclude is None else exclude[0].tolist()
        for s in range(0, n, group):
            t = min(s + group, n)
            ex = None
            if exclude is not None:
                ex = ((exclude[0][s:t + 1] - off[s]).contiguous(), exclude[1][off[s]:off[t]].contiguous())
            ops.topk_ip(u[s:t], items, k, self.scale, rows[s:t], scores[s:t], ws, exclude=ex)
        return rows, scores


ENGINES = {"deepfm": DeepFMEngine, "dcn": DCNEngine, "xdeepfm": XDeepFMEngine, "afm": AFMEngine, "din": DINEngine,
           "autoint": AutoIntEngine, "dlrm": DLRMEngine, "fibinet": FiBiNETEngine, "fmfm": FmFMEngine, "pnn": PNNEngine,
           "masknet": MaskNetEngine, "bst": BSTEngine, "dien": DIENEngine, "mmoe": MMoEEngine, "ple": PLEEngine,
           "twotower": TwoTowerEngine}
