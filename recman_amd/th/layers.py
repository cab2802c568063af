"""The reference's layer callables (recman/tf/core/layers.py) on the HIP kernels: the seam the
reference's models are composed at - `Layer(variables, ...)(tensor) -> tensor`, `layer.l2() -> scalar`,
variables upserted lazily by name into one shared dict (layers.py:95-110, 317-328, 532-574, 659-695,
789-794) - for users who build their own model the way xDeepFM._out does (xDeepFM.py:49-104,
DeepFM.py:107-163, DCN.py:99-149).  recman/th/layers.py, the file this fills, is 0 bytes in the reference.

    variables = {}
    emb = FeatEmbeddingLayer(variables, feat_dict, 16, l2, use_bias=False)
    E, _ = emb(inputs)                                   # inputs: th.inputs.DataInputs
    lin = SparseLinearLayer(variables, feats, l2)(SparseLinearCombiner(feats)(inputs))
    cin = CIN(variables, [128, 128], "leaky_relu", [1, 1, 1], l2)(E)
    dnn = DNN(variables, (32, 32), [1, 1, 1], "relu", l2)(DNNCombiner()([E] + inputs.dense_inputs(feat_dict)))
    pred = PredictionLayer(variables, "classification")(lin + cin + dnn)
    loss = create_loss(inputs.y, pred) + emb.l2() + ...
    loss.backward();  torch.optim.Adam(variables.values()).step()

Each layer is a torch.autograd.Function over recman_amd/ops.py (the C ABI, librecman_hip.so): forward and
backward are the same hand-written kernels the engines use (csrc/embed.hip, mlp.hip, gemm.hip, cin.hip,
cross.hip, afm.hip, autoint.hip, dot_interact.hip, loss.hip); torch is the plumbing in between - autograd's tape, the l2 terms, the bias-table
lookup and the loss on probabilities are plain torch ops.  Variables are float32 CUDA leaf tensors
under the reference's names, so `variables` is at once the parameter list of a torch optimizer and the
state dict of a checkpoint.  There is no CPU path.

This is the COMPOSABLE surface, not the fast one: every layer is its own launch group and the embedding
gradient comes back dense per feature (what TF's IndexedSlices + the dense l2 term add up to,
layers.py:188-193).  The model classes (th.DeepFM / DCN / xDeepFM) run the fused engines instead.
Supported features: SparseFeat and DenseFeat (multi-valued / value features: use the model classes).
CIN dropout is not offered here (keep-probabilities must be 1; the engines implement it)."""
import math

import numpy as np
import torch

from .. import engine as eng
from .. import ops
from .inputs import DenseFeat, MultiValCsvFeat, SparseFeat, SparseValueFeat

F32, I64 = torch.float32, torch.int64
KERAS_EPS = 1e-7


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("recman_amd.th.layers needs a GPU (MI355X); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _leaf(t):
    return t.to(_device(), F32).contiguous().requires_grad_(True)


def glorot_normal(shape, seed=2019):
    """utils.py:156-183: truncated normal(0, sqrt(2 / (fan_in + fan_out))), +-2 sigma; fans as calc_fan
    computes them (the last two dimensions, times the product of the others)."""
    shape = tuple(int(s) for s in shape)
    k = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    fan_in, fan_out = shape[-2] * k, shape[-1] * k
    std = math.sqrt(2.0 / (fan_in + fan_out))
    g = torch.Generator(device=_device()).manual_seed(int(seed))
    t = torch.empty(shape, device=_device(), dtype=F32)
    torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std, generator=g)
    return t


def glorot_uniform(shape, seed=None):
    """utils.py:186-189 (unseeded in the reference, layers.py:690)."""
    shape = tuple(int(s) for s in shape)
    b = math.sqrt(6.0 / (shape[-2] + shape[-1]))
    g = None if seed is None else torch.Generator(device=_device()).manual_seed(int(seed))
    return torch.empty(shape, device=_device(), dtype=F32).uniform_(-b, b, generator=g)


def _dev_inputs(inputs, feat_dict=None):
    """(idx [B,F] int64, dense [B,Dn] f32) of a DataInputs on the GPU, cached on the object."""
    cached = getattr(inputs, "_dev_cache", None)
    if cached is None:
        idx = torch.from_numpy(np.ascontiguousarray(inputs.idx)).to(_device())
        dense = torch.from_numpy(np.ascontiguousarray(inputs.dense)).to(_device())
        cached = inputs._dev_cache = (idx, dense)
    return cached


def _keep_mask(shape, keep):
    """tf.nn.dropout(x, rate = 1 - keep): a 0/1 mask; kept entries are scaled by 1 / keep by the caller."""
    return (torch.rand(*shape, device=_device()) < keep).to(F32)


# ------------------------------------------------------------------------------------------------
# embedding gather
# ------------------------------------------------------------------------------------------------
class _GatherFn(torch.autograd.Function):
    """E[b,f,:] = table[field_off[f] + idx[b,f]] (rm_embed_fwd; backward rm_scatter_add_rows)."""

    @staticmethod
    def forward(ctx, table, idx, field_off):
        B, F = idx.shape
        D = table.shape[1]
        E = torch.empty(B, F, D, device=table.device, dtype=F32)
        ops.embed_fwd(idx, table.detach(), field_off, E=E, D=D, table_ld=D)
        ctx.save_for_backward(idx, field_off)
        ctx.R = table.shape[0]
        return E

    @staticmethod
    def backward(ctx, dE):
        idx, field_off = ctx.saved_tensors
        d_table = torch.zeros(ctx.R, dE.shape[2], device=dE.device, dtype=F32)
        ops.scatter_add_rows(d_table, idx, field_off, rows=dE.contiguous())
        return d_table, None, None


def _csr_dev(inputs, name):
    """(offsets, ids, vals or None) of a multi-valued / value feature on the GPU (DataInputs.mv holds the CSR)."""
    cache = inputs.__dict__.setdefault("_mv_dev_cache", {})
    if name not in cache:
        c = inputs.mv[name]
        dev = _device()
        cache[name] = (torch.from_numpy(np.ascontiguousarray(c.offsets)).to(dev),
                       torch.from_numpy(np.ascontiguousarray(c.ids)).to(dev),
                       None if c.vals is None else torch.from_numpy(np.ascontiguousarray(c.vals)).to(dev, F32))
    return cache[name]


class _PoolFn(torch.autograd.Function):
    """One multi-valued (MultiValCsvFeat: sqrtn combiner, layers.py:144-169) or value (SparseValueFeat: value *
    row, bias unscaled, layers.py:129-142) feature: (E_f [B,D], bias_f [B]) through rm_pool_rows over a temporary
    fused copy [V, D + 4] of the feature's table and bias table; backward rm_pool_rows_bwd."""

    @staticmethod
    def forward(ctx, table, bias, offsets, ids, vals):
        V, D = table.shape
        B = offsets.shape[0] - 1
        fused = torch.zeros(V, D + 4, device=table.device, dtype=F32)
        fused[:, :D] = table.detach()
        if bias is not None:
            fused[:, D] = bias.detach().reshape(-1)
        out = torch.empty(B, D + 4, device=table.device, dtype=F32)
        ops.pool_rows(fused, 0, D, offsets, ids, out, vals=vals)
        ctx.save_for_backward(offsets, ids, vals)
        ctx.shape, ctx.has_bias = (V, D), bias is not None
        return out[:, :D].contiguous(), out[:, D].contiguous()

    @staticmethod
    def backward(ctx, dE, dbias):
        offsets, ids, vals = ctx.saved_tensors
        V, D = ctx.shape
        d_table = torch.zeros(V, D, device=dE.device, dtype=F32)
        d_bias = torch.zeros(V, device=dE.device, dtype=F32) if ctx.has_bias else None
        ops.pool_rows_bwd(dE.contiguous(), dbias.contiguous() if ctx.has_bias else None, None, D, offsets, ids, 0,
                          d_table, d_bias, None, vals=vals)
        return d_table, (d_bias.view(V, 1) if ctx.has_bias else None), None, None, None


class FeatEmbedding:
    """layers.py:68-193: one feature's table (+ bias table).  SparseFeat (:117-128) features are gathered
    together by FeatEmbeddingLayer; MultiValCsvFeat (:144-169) and SparseValueFeat (:129-142) through _PoolFn."""

    display_name = "FeatEmbedding"

    def __init__(self, variables, feat, embedding_size, l2_reg=0.00001, use_bias=True, prefix="", seed=2019):
        assert not isinstance(feat, DenseFeat)  # layers.py:85
        if not isinstance(feat, (SparseFeat, MultiValCsvFeat, SparseValueFeat)):
            raise NotImplementedError(f"feature {feat.name}: th.layers embeds SparseFeat, MultiValCsvFeat and "
                                      "SparseValueFeat (the reference raises for the others too)")
        self.variables, self.feat, self.embedding_size = variables, feat, int(embedding_size)
        self.l2_reg, self.use_bias, self.prefix, self.seed = l2_reg, use_bias, prefix, seed

    def _upsert_variables(self):
        name = f"{self.prefix}{self.feat.name}_feat_embed"
        if name not in self.variables:
            self.variables[name] = _leaf(glorot_normal([self.feat.feat_size, self.embedding_size], self.seed))
        name = f"{self.prefix}{self.feat.name}_feat_bias"
        if name not in self.variables and self.use_bias:
            self.variables[name] = _leaf(torch.zeros(self.feat.feat_size, 1))

    def l2(self):
        return self.l2_reg * 0.5 * self.variables[f"{self.prefix}{self.feat.name}_feat_embed"].square().sum()


class FeatEmbeddingLayer:
    """layers.py:196-267: all embedding features -> (E [B,F,D], bias [B,F,1] or None), field order =
    feat_dict.embedding_feats.  The per-feature tables are the variables; they are concatenated for the
    one gather launch (a copy per call - the model classes keep one fused table instead)."""

    display_name = "FeatEmbeddingLayer"

    def __init__(self, variables, feat_dict, embedding_size, l2_reg=0.00001, use_bias=True, prefix="", seed=2019):
        if int(embedding_size) % 4:
            raise ValueError("embedding_size must be a multiple of 4 on the HIP path")
        self.variables, self.feat_dict, self.embedding_size = variables, feat_dict, int(embedding_size)
        self.l2_reg, self.use_bias, self.prefix, self.seed = l2_reg, use_bias, prefix, seed
        self.feat_embeds = dict((feat, FeatEmbedding(variables, feat, embedding_size, l2_reg, use_bias=use_bias,
                                                     prefix=prefix, seed=seed))
                                for feat in feat_dict.embedding_feats)

    def __call__(self, inputs):
        feats = list(self.feat_embeds)
        for fe in self.feat_embeds.values():
            fe._upsert_variables()
        idx, _ = _dev_inputs(inputs)
        if idx.shape[1] != len(feats):
            raise ValueError("inputs were not loaded with this feature dictionary")
        mv = getattr(inputs, "mv", None) or {}
        plain = [j for j, f in enumerate(feats) if f.name not in mv]
        cols_e, cols_b = [None] * len(feats), [None] * len(feats)
        if plain:  # the id features: ONE gather launch over their concatenated tables
            pf = [feats[j] for j in plain]
            sizes = [f.feat_size for f in pf]
            offs = torch.tensor(np.concatenate(([0], np.cumsum(sizes)[:-1])), dtype=I64, device=idx.device)
            table = torch.cat([self.variables[f"{self.prefix}{f.name}_feat_embed"] for f in pf], 0)
            pidx = idx if len(plain) == len(feats) else idx[:, plain].contiguous()
            Ep = _GatherFn.apply(table, pidx, offs)
            bp = None
            if self.use_bias:
                btab = torch.cat([self.variables[f"{self.prefix}{f.name}_feat_bias"] for f in pf], 0)
                bp = btab[(pidx + offs)]  # [B,Fp,1] (a torch lookup: B*Fp scalars)
            if len(plain) == len(feats):
                return Ep, bp
            for k, j in enumerate(plain):
                cols_e[j] = Ep[:, k]
                cols_b[j] = bp[:, k] if bp is not None else None
        for j, f in enumerate(feats):  # multi-valued / value features: pooled rows, one launch each
            if f.name in mv:
                offsets, ids, vals = _csr_dev(inputs, f.name)
                bt = self.variables[f"{self.prefix}{f.name}_feat_bias"] if self.use_bias else None
                e, b = _PoolFn.apply(self.variables[f"{self.prefix}{f.name}_feat_embed"], bt, offsets, ids, vals)
                cols_e[j], cols_b[j] = e, b.view(-1, 1)
        E = torch.stack(cols_e, 1)
        bias = torch.stack(cols_b, 1) if self.use_bias else None
        return E, bias

    def l2(self):
        return sum(fe.l2() for fe in self.feat_embeds.values())


# ------------------------------------------------------------------------------------------------
# linear term
# ------------------------------------------------------------------------------------------------
class _LinearInput:
    """What the combiners hand to the linear layers instead of a [B, sum V] one-hot matrix (26,000,039
    columns at the Criteo shape): the ids, their offsets into linear_w, the dense columns."""

    def __init__(self, idx, lin_off, dense, dense_pos, width):
        self.idx, self.lin_off, self.dense, self.dense_pos, self.width = idx, lin_off, dense, dense_pos, width
        self.shape = (idx.shape[0] if idx is not None else dense.shape[0], width)


class LinearCombiner:
    """layers.py:270-298 (and SparseLinearCombiner :357-386): the linear features in the order given;
    a sparse feature owns feat_size one-hot columns, a dense feature one column."""

    display_name = "LinearCombiner"

    def __init__(self, linear_feats, prefix=""):
        self.linear_feats, self.prefix = list(linear_feats), prefix

    def __call__(self, inputs):
        dev = _device()
        cols, offs, dcols, dpos, mvs = [], [], [], [], []
        at = 0
        for feat in self.linear_feats:
            if isinstance(feat, DenseFeat):
                dcols.append(np.asarray(inputs[feat.name], dtype=np.float32).reshape(-1, 1))
                dpos.append(at)
            elif isinstance(feat, (MultiValCsvFeat, SparseValueFeat)):
                # multi-hot count without slot 0 (utils.py:86-108) / value * one-hot (utils.py:70-71): weighted ids
                offsets, ids, vals = _csr_dev(inputs, feat.name)
                wts = vals if vals is not None else (ids >= 1).to(F32)
                seg = torch.repeat_interleave(torch.arange(offsets.shape[0] - 1, device=dev), offsets[1:] - offsets[:-1])
                mvs.append((at, ids, wts, seg))
            elif isinstance(feat, SparseFeat):
                cols.append(np.asarray(inputs[feat.name], dtype=np.int64).reshape(-1, 1))
                offs.append(at)
            else:
                raise NotImplementedError(f"feature {feat.name}: th.layers handles SparseFeat / SparseValueFeat / "
                                          "MultiValCsvFeat / DenseFeat")
            at += feat.feat_size
        idx = torch.from_numpy(np.concatenate(cols, 1)).to(dev) if cols else None
        dense = torch.from_numpy(np.concatenate(dcols, 1)).to(dev) if dcols else None
        self.output = _LinearInput(idx, torch.tensor(offs, dtype=I64, device=dev) if cols else None, dense,
                                   torch.tensor(dpos, dtype=I64, device=dev) if dcols else None, at)
        self.output.mvs = mvs
        return self.output


class SparseLinearCombiner(LinearCombiner):
    display_name = "SparseLinearCombiner"


class _LinearFn(torch.autograd.Function):
    """rm_linear_fwd; backward rm_scatter_add_rows (g_row form) + rm_linear_dense_bwd."""

    @staticmethod
    def forward(ctx, w, w0, idx, lin_off, dense, dense_pos):
        B = idx.shape[0] if idx is not None else dense.shape[0]
        wf = w.detach().reshape(-1)
        wd = wf[dense_pos].contiguous() if dense is not None else None
        out = torch.empty(B, device=w.device, dtype=F32)
        ops.linear_fwd(idx, lin_off, wf if idx is not None else None, dense, wd, w0.detach(), out)
        ctx.save_for_backward(idx, lin_off, dense, dense_pos)
        ctx.n = wf.numel()
        return out.view(B, 1)

    @staticmethod
    def backward(ctx, g):
        idx, lin_off, dense, dense_pos = ctx.saved_tensors
        g = g.reshape(-1).contiguous()
        d_w = torch.zeros(ctx.n, device=g.device, dtype=F32)
        if idx is not None:
            ops.scatter_add_rows(d_w, idx, lin_off, g_row=g, width=1, ld=1)
        ws = torch.empty(256 * 1024, device=g.device, dtype=F32)
        d_w0 = torch.empty(1, device=g.device, dtype=F32)
        Dn = 0 if dense is None else dense.shape[1]
        d_wd = torch.empty(Dn, device=g.device, dtype=F32) if Dn else None
        ops.linear_dense_bwd(g, dense, d_wd, d_w0, ws)
        if Dn:
            d_w[dense_pos] = d_wd
        return d_w.view(-1, 1), d_w0, None, None, None, None


class LinearLayer:
    """layers.py:301-354 (SparseLinearLayer :389-446): logit = one_hot(inputs) @ W + W0 in gather form;
    W, W0 zero-initialised (:317-328); training=False adds the features' manual weights (:338-345)."""

    display_name = "LinearRegression"

    def __init__(self, variables, linear_feats, l2_reg=0.00001, prefix="", training=True):
        self.variables, self.linear_feats = variables, list(linear_feats)
        self.l2_reg, self.prefix, self.training = l2_reg, prefix, training

    def _upsert_variables(self, input_shape):
        name = f"{self.prefix}linear_w0"
        if name not in self.variables:
            self.variables[name] = _leaf(torch.zeros(1))
        name = f"{self.prefix}linear_w"
        if name not in self.variables:
            self.variables[name] = _leaf(torch.zeros(input_shape[1], 1))

    def __call__(self, inputs):
        self._upsert_variables(inputs.shape)
        W = self.variables[f"{self.prefix}linear_w"]
        if not self.training:
            if any(getattr(f, "_weights", None) for f in self.linear_feats):
                mw = np.concatenate([np.asarray(f.weights, dtype=np.float64).reshape(-1) for f in self.linear_feats])
                W = W + torch.from_numpy(mw.astype(np.float32)).to(W.device).view(-1, 1)
        out = _LinearFn.apply(W, self.variables[f"{self.prefix}linear_w0"], inputs.idx, inputs.lin_off,
                              inputs.dense, inputs.dense_pos)
        for at, ids, wts, seg in getattr(inputs, "mvs", ()):  # multi-valued / value features: weighted ids
            part = torch.zeros(out.shape[0], device=out.device, dtype=F32)
            out = out + part.index_add(0, seg, W.view(-1)[at + ids] * wts).view(-1, 1)
        return out

    def l2(self):
        return self.l2_reg * 0.5 * self.variables[f"{self.prefix}linear_w"].square().sum()


class SparseLinearLayer(LinearLayer):
    display_name = "SparseLinearRegression"


# ------------------------------------------------------------------------------------------------
# FM
# ------------------------------------------------------------------------------------------------
class _FMFn(torch.autograd.Function):
    """FMLayer on a given E [B,F,D] (+ bias [B,F,1]): rm_embed_fwd with E itself as the table and the
    identity index (its gather + FM reduction is the FM layer); backward rm_embed_bwd."""

    @staticmethod
    def forward(ctx, E, bias, mask_b, mask_e):
        B, F, D = E.shape
        Ed = E.detach().contiguous()
        ident = torch.arange(B * F, device=E.device, dtype=I64).view(B, F)
        zoff = torch.zeros(F, device=E.device, dtype=I64)
        S = torch.empty(B, D, device=E.device, dtype=F32)
        out = torch.empty(B, device=E.device, dtype=F32)
        ops.embed_fwd(ident, Ed.view(B * F, D), zoff, D=D, table_ld=D,
                      bias_table=bias.detach().reshape(-1).contiguous() if bias is not None else None, bias_ld=1,
                      mask_b=mask_b, mask_e=mask_e, fm_sum=S, fm_logit=out)
        ctx.save_for_backward(Ed, S, mask_b, mask_e)
        ctx.has_bias = bias is not None
        return out.view(B, 1)

    @staticmethod
    def backward(ctx, g):
        Ed, S, mask_b, mask_e = ctx.saved_tensors
        B, F, D = Ed.shape
        g = g.reshape(-1).contiguous()
        dE = torch.empty_like(Ed)
        d_bias = torch.empty(B, F, device=g.device, dtype=F32)
        ops.embed_bwd(dE, E=Ed, fm_sum=S, g_fm=g, mask_b=mask_b, mask_e=mask_e, d_bias=d_bias)
        return dE, (d_bias.view(B, F, 1) if ctx.has_bias else None), None, None


class FMLayer:
    """layers.py:449-481: y = sum_f bias_f + 1/2 sum_k [(sum_f E_fk)^2 - sum_f E_fk^2]; `dropout` holds
    KEEP probabilities (bias, embeddings), rate = 1 - keep (:461,466)."""

    def __init__(self, dropout=(1, 1)):
        self.dropout = dropout

    def __call__(self, embeddings, embedding_bias):
        assert embeddings.dim() == 3  # layers.py:458
        B, F, D = embeddings.shape
        kb, ke = self.dropout
        mask_b = _keep_mask((B, F), kb) / kb if (kb < 1 and embedding_bias is not None) else None
        mask_e = _keep_mask((B, F, D), ke) / ke if ke < 1 else None
        return _FMFn.apply(embeddings, embedding_bias, mask_b, mask_e)

    def l2(self):
        return 0.0  # layers.py:480-481


# ------------------------------------------------------------------------------------------------
# DNN
# ------------------------------------------------------------------------------------------------
class _Concat:
    """x = [xe | xd] as the pair the kernels take (never concatenated in memory)."""

    def __init__(self, xe, xd):
        self.xe, self.xd = xe, xd
        self.shape = (xe.shape[0], xe.shape[1] + (0 if xd is None else xd.shape[1]))


class DNNCombiner:
    """layers.py:484-501: [flatten(E) | dense_1 .. dense_Dn]."""

    def __init__(self, prefix=""):
        self.prefix = prefix

    def __call__(self, inputs: list):
        E = inputs[0]
        xe = E.reshape(E.shape[0], -1)
        dense = [d if torch.is_tensor(d) else torch.from_numpy(np.asarray(d, dtype=np.float32)) for d in inputs[1:]]
        xd = torch.cat([d.reshape(xe.shape[0], -1).to(xe.device, F32) for d in dense], 1).contiguous() if dense else None
        return _Concat(xe, xd)


def _as_concat(x):
    if isinstance(x, _Concat):
        return x
    if x.shape[1] % 4:
        raise ValueError("a plain DNN / CrossNet input needs a multiple of 4 columns; pass DNNCombiner's output")
    return _Concat(x, None)


class _DNNFn(torch.autograd.Function):
    """engine.MLP (rm_mlp_fwd / rm_mlp_bwd fused for widths <= 32, rm_dense_fwd / rm_dense_wgrad otherwise)."""

    @staticmethod
    def forward(ctx, core, keep, masks, xe, xd, *params):
        out = core.mlp.forward(xe.detach().contiguous(), None if xd is None else xd.detach().contiguous(), keep, masks)
        ctx.core = core
        return out.clone().view(-1, 1)

    @staticmethod
    def backward(ctx, g):
        mlp = ctx.core.mlp
        dxe = torch.empty(g.shape[0], mlp.FD, device=g.device, dtype=F32)
        mlp.backward(g.reshape(-1).contiguous(), dxe)
        return (None, None, None, dxe, None) + tuple(mlp.g[n].clone() for n in ctx.core.names)


class DNN:
    """layers.py:504-628: x -> dropout -> [dense + bias + activation + dropout]* -> x @ dnn_w + dnn_w0.
    `dropout`: len(hidden_units) + 1 KEEP probabilities (:522); hidden_units=None -> the 2/3 rule of
    compute_hidden_units_s2 (utils.py:135-139)."""

    display_name = "DeepNeuralNetwork"

    def __init__(self, variables, hidden_units, dropout, activation, l2_reg=0.00001, prefix="", seed=2019):
        self.variables, self.hidden_units, self.dropout = variables, hidden_units, list(dropout)
        self.activation, self.l2_reg, self.prefix, self.seed = activation, l2_reg, prefix, seed
        self.mlp, self.names = None, None
        if hidden_units is not None:
            assert len(self.dropout) == len(hidden_units) + 1  # layers.py:522

    def _build(self, FD, Dn):
        hidden = self.hidden_units
        if hidden is None:  # utils.py:135-139
            h = (FD + Dn) * 2 // 3
            hidden = (h, h)
            assert len(self.dropout) == 3
        self.hidden = [int(h) for h in hidden]
        pre, dims = self.prefix, [FD + Dn] + self.hidden
        tmp_p, tmp_g = {}, {}
        self.mlp = eng.MLP(tmp_p, tmp_g, FD, Dn, self.hidden, self.activation, _device(), prefix=pre)
        self.names = list(tmp_p)
        for n in self.names:  # upsert under the reference's names and distributions (:532-574)
            if n not in self.variables:
                shape = tmp_p[n].shape
                init = glorot_normal(shape, self.seed) if (n.endswith("_weights") or n.endswith("dnn_w")) else torch.zeros(shape)
                self.variables[n] = _leaf(init)
        self.mlp.p = self.variables

    def __call__(self, x):
        x = _as_concat(x)
        FD, Dn = x.xe.shape[1], 0 if x.xd is None else x.xd.shape[1]
        if self.mlp is None or (self.mlp.FD, self.mlp.Dn) != (FD, Dn):
            self._build(FD, Dn)
        keep = self.dropout
        dims = [FD + Dn] + self.hidden
        masks = None
        if any(k < 1 for k in keep):
            masks = [_keep_mask((x.xe.shape[0], d), k) if k < 1 else None for d, k in zip(dims, keep)]
        return _DNNFn.apply(self, keep, masks, x.xe, x.xd, *[self.variables[n] for n in self.names])

    def l2(self):
        ws = [self.variables[f"{self.prefix}dnn_layer_{i}_weights"] for i in range(len(self.hidden))]
        ws.append(self.variables[f"{self.prefix}dnn_w"])
        return sum(self.l2_reg * 0.5 * w.square().sum() for w in ws)  # layers.py:611-628


# ------------------------------------------------------------------------------------------------
# CIN
# ------------------------------------------------------------------------------------------------
class _CINFn(torch.autograd.Function):
    """rm_cin_layer_fwd per layer + rm_rowdot; backward rm_cin_layer_bwd per layer (csrc/cin.hip, f32 MFMA).
    masks: None, or the L + 1 keep masks of cin_dropout (the input E, layers.py:707-708, then every layer's maps
    behind the activation, :740): a dropped layer's maps are scaled in place after its kernel and its pooled
    columns re-summed; in the backward its upstream gradient ([next layer's dXk | g x cin_w]) is built explicitly
    and scaled by mask / keep - as the xDeepFM engine does (engine.XDeepFMEngine._cin_fwd / _branches_bwd)."""

    @staticmethod
    def forward(ctx, core, masks, E, *params):
        c = core
        B, m, D = E.shape
        c._alloc(B, m, D)
        L = len(c.units)
        keep = c.dropout
        on = [bool(masks is not None and masks[i] is not None and keep[i] < 1) for i in range(L + 1)]
        X0 = E.detach().contiguous()
        if on[0]:
            X0 = X0 * (masks[0] / keep[0])
        xk = X0
        for i, n in enumerate(c.units):
            ops.cin_layer_fwd(X0, xk, c.Hs[i], c.variables[c.fname(i)].detach()[0], c.variables[c.bname(i)].detach(),
                              c.act, c.maps[i], c.fws, pooled=None if on[i + 1] else c.pooled,
                              pool_col0=c.pool_col0[i], pool_from=c.pool_from[i], ws6=c.fws6)
            if on[i + 1]:
                pf, c0 = c.pool_from[i], c.pool_col0[i]
                c.maps[i].mul_(masks[i + 1] / keep[i + 1])
                torch.sum(c.maps[i][:, pf:, :], dim=2, out=c.pooled[:, c0: c0 + n - pf])
            xk = c.maps[i]
        out = torch.empty(B, device=E.device, dtype=F32)
        ops.rowdot(c.pooled, c.variables[c.prefix + "cin_w"].detach().view(-1), c.variables[c.prefix + "cin_w0"].detach(), out)
        ctx.core, ctx.X0, ctx.masks, ctx.on = core, X0, masks, on
        return out.view(B, 1)

    @staticmethod
    def backward(ctx, g):
        c, X0, masks, on = ctx.core, ctx.X0, ctx.masks, ctx.on
        keep = c.dropout
        B, m, D = X0.shape
        g = g.reshape(-1).contiguous()
        L = len(c.units)
        dX0 = torch.zeros_like(X0)
        grads = {}
        d_cw, d_cw0 = torch.empty(c.P, device=g.device, dtype=F32), torch.empty(1, device=g.device, dtype=F32)
        ops.linear_dense_bwd(g, c.pooled, d_cw, d_cw0, c.ws)
        cw = c.variables[c.prefix + "cin_w"].detach().view(-1)
        for i in range(L - 1, -1, -1):
            n, pf, c0 = c.units[i], c.pool_from[i], c.pool_col0[i]
            dW = torch.empty(m * c.Hs[i], n, device=g.device, dtype=F32)
            db = torch.empty(n, device=g.device, dtype=F32)
            d_hidden = c.dxk[i + 1] if i + 1 < L else None
            cwd, pfa = cw[c0: c0 + n - pf], pf
            if on[i + 1]:
                up = torch.empty_like(c.maps[i])
                if pf:
                    up[:, :pf] = d_hidden
                up[:, pf:] = g.view(-1, 1, 1) * cw[c0: c0 + n - pf].view(1, -1, 1)
                up.mul_(masks[i + 1] / keep[i + 1])
                d_hidden, cwd, pfa = up, None, n
            ops.cin_layer_bwd(X0, X0 if i == 0 else c.maps[i - 1], c.Hs[i], c.variables[c.fname(i)].detach()[0], c.act,
                              c.maps[i], g, dX0, dW, db, c.bws, xk_is_x0=(i == 0),
                              d_hidden=d_hidden, cin_w_direct=cwd,
                              pool_from=pfa, accumulate_dx0=True, dXk=c.dxk[i] if i > 0 else None)
            grads[c.fname(i)], grads[c.bname(i)] = dW.view(1, m * c.Hs[i], n), db
        if on[0]:
            dX0 = dX0 * (masks[0] / keep[0])
        grads[c.prefix + "cin_w"], grads[c.prefix + "cin_w0"] = d_cw.view(-1, 1), d_cw0
        return (None, None, dX0) + tuple(grads[n] for n in c.names)


class CIN:
    """layers.py:631-777: per layer Z = X0 (x) Xk (never formed), 1x1 convolution with the layer's filter,
    activation BEFORE the split, first half -> next hidden / second half -> direct (last layer: all
    direct), sum over D, @ cin_w + cin_w0.  Non-final layer sizes must be even (the reference silently
    drops a map otherwise, :681,742)."""

    display_name = "CompressedInteractionNetwork"

    def __init__(self, variables, cross_layer_units, activation, dropout, l2_reg=0.00001, prefix="", seed=2019):
        self.variables, self.cross_layer_units = variables, [int(u) for u in cross_layer_units]
        self.activation, self.dropout, self.l2_reg, self.prefix, self.seed = activation, list(dropout), l2_reg, prefix, seed
        assert len(self.cross_layer_units) > 0  # layers.py:656
        assert len(self.cross_layer_units) + 1 == len(self.dropout)  # :657
        self.units, self.act = self.cross_layer_units, eng.act_name(activation)
        self._shape = None

    def fname(self, i):
        return f"{self.prefix}cin_filter_{i}"

    def bname(self, i):
        return f"{self.prefix}cin_bias_{i}"

    def _upsert_variables(self, field_size):
        m = field_size
        self.Hs, self.pool_from, self.pool_col0 = [m], [], []
        final = 0
        for i, size in enumerate(self.units):
            last = i == len(self.units) - 1
            if not last and size % 2:
                raise ValueError("CIN layer sizes before the last must be even (split in halves, layers.py:742-746)")
            H = self.Hs[-1]
            if self.fname(i) not in self.variables:  # :663-676
                self.variables[self.fname(i)] = _leaf(glorot_normal([1, m * H, size], self.seed))
            if self.bname(i) not in self.variables:
                self.variables[self.bname(i)] = _leaf(torch.zeros(size))
            self.pool_from.append(0 if last else size // 2)
            self.pool_col0.append(final)
            final += size if last else size // 2
            self.Hs.append(size // 2)
        self.P = final
        if self.prefix + "cin_w" not in self.variables:  # :687-695 (glorot_uniform, unseeded)
            self.variables[self.prefix + "cin_w"] = _leaf(glorot_uniform([final, 1]))
        if self.prefix + "cin_w0" not in self.variables:
            self.variables[self.prefix + "cin_w0"] = _leaf(torch.zeros(1))
        self.names = ([n for i in range(len(self.units)) for n in (self.fname(i), self.bname(i))]
                      + [self.prefix + "cin_w", self.prefix + "cin_w0"])

    def _alloc(self, B, m, D):
        if self._shape == (B, m, D):
            return
        self._shape = (B, m, D)
        dev = _device()
        self.maps = [torch.empty(B, n, D, dtype=F32, device=dev) for n in self.units]
        self.dxk = [None] + [torch.empty(B, self.Hs[i], D, dtype=F32, device=dev) for i in range(1, len(self.units))]
        self.pooled = torch.empty(B, self.P, dtype=F32, device=dev)
        fw = max(ops.cin_filter_workspace(m, self.Hs[i], n) for i, n in enumerate(self.units))
        bw = max(ops.cin_bwd_workspace(B, m, self.Hs[i], n, D) for i, n in enumerate(self.units))
        self.fws = torch.empty(fw, dtype=F32, device=dev)
        self.bws = torch.empty(bw, dtype=F32, device=dev)
        f6 = max(ops.cin_filter_workspace6(m, self.Hs[i], n, D) for i, n in enumerate(self.units))
        self.fws6 = torch.empty(f6, dtype=F32, device=dev) if f6 > 0 else None  # (rm_cin_layer_fwd6, csrc/cin6.hip)
        self.ws = torch.empty(256 * 1024, dtype=F32, device=dev)

    def __call__(self, inputs):
        assert inputs.dim() == 3  # layers.py:698
        self._upsert_variables(inputs.shape[1])
        masks = None
        if any(k < 1 for k in self.dropout):  # tf.nn.dropout on the input (:707-708) and on every layer's maps (:740)
            B, _, D = inputs.shape
            shapes = [tuple(inputs.shape)] + [(B, n, D) for n in self.units]
            masks = [_keep_mask(sh, k) if k < 1 else None for sh, k in zip(shapes, self.dropout)]
        return _CINFn.apply(self, masks, inputs, *[self.variables[n] for n in self.names])

    def l2(self):
        ws = [self.variables[self.fname(i)] for i in range(len(self.units))] + [self.variables[self.prefix + "cin_w"]]
        return sum(self.l2_reg * 0.5 * w.square().sum() for w in ws)  # layers.py:762-777


# ------------------------------------------------------------------------------------------------
# CrossNet
# ------------------------------------------------------------------------------------------------
class _CrossFn(torch.autograd.Function):
    """rm_cross_fwd / rm_cross_bwd (all layers fused) + rm_dense_wgrad / rm_cross_param_grads for the
    parameter gradients, as the DCN engine runs them."""

    @staticmethod
    def forward(ctx, core, xe, xd, w, b, w_out):
        B = xe.shape[0]
        L = w.shape[0]
        xe_, xd_ = xe.detach().contiguous(), None if xd is None else xd.detach().contiguous()
        logit = torch.empty(B, device=xe.device, dtype=F32)
        p = torch.empty(B, ops.cross_p_ld(L), device=xe.device, dtype=F32)
        ops.cross_fwd(xe_, xd_, w.detach(), b.detach(), w_out.detach().view(-1), logit, p)
        ctx.save_for_backward(xe_, xd_, w.detach(), b.detach(), w_out.detach(), p)
        return logit.view(B, 1)

    @staticmethod
    def backward(ctx, g):
        xe, xd, w, b, w_out, p = ctx.saved_tensors
        B, FD = xe.shape
        L, d = w.shape
        g = g.reshape(-1).contiguous()
        dev = g.device
        d_xe = torch.empty(B, FD, device=dev, dtype=F32)
        coef = torch.empty(B, 2 * L + 2, device=dev, dtype=F32)
        ops.cross_bwd(w, b, w_out.view(-1), g, p, d_xe, coef)
        P = torch.empty(d, L + 1, device=dev, dtype=F32)
        wws = torch.empty(max(1, ops.dense_wgrad_workspace(d, L + 1, B)), device=dev, dtype=F32)
        ops.dense_wgrad(xe, xd, coef[:, : L + 1], P, wws)
        csum = torch.empty(2 * L + 2, device=dev, dtype=F32)
        ops.linear_dense_bwd(torch.ones(B, device=dev, dtype=F32), coef, csum, None,
                             torch.empty(256 * 1024, device=dev, dtype=F32))
        dw, db, dwo = torch.empty_like(w), torch.empty_like(b), torch.empty(d, device=dev, dtype=F32)
        ops.cross_param_grads(P, csum[L + 1:].contiguous(), w, b, w_out.view(-1), dw, db, dwo)
        return None, d_xe, None, dw, db, dwo.view(-1, 1)


class CrossNet:
    """The class DCN.py:7 imports commented out and DCN.py:134-137 uses: CrossNet(layer_num, l2_reg)(x) ->
    logit [B,1], `.weights`, `.l2()`.  Arithmetic: arXiv 1708.05123 eq. (3) (the paper README.md:6 cites),
    x_{l+1} = x0 (x_l . w_l) + b_l + x_l, logit = x_L . w_out.  Variables (names chosen here - the
    reference has none): cross_w [L,d], cross_b [L,d], cross_w_out [d,1]."""

    display_name = "CrossNet"

    def __init__(self, variables, layer_num, l2_reg=0.0, prefix="", seed=2019):
        self.variables, self.layer_num, self.l2_reg, self.prefix, self.seed = variables, int(layer_num), l2_reg, prefix, seed

    def _upsert_variables(self, d):
        L, pre = self.layer_num, self.prefix
        if pre + "cross_w" not in self.variables:
            self.variables[pre + "cross_w"] = _leaf(glorot_normal([L, d, 1], self.seed).view(L, d))
        if pre + "cross_b" not in self.variables:
            self.variables[pre + "cross_b"] = _leaf(torch.zeros(L, d))
        if pre + "cross_w_out" not in self.variables:
            self.variables[pre + "cross_w_out"] = _leaf(glorot_normal([d, 1], self.seed))

    @property
    def weights(self):
        return [self.variables[self.prefix + n] for n in ("cross_w", "cross_b", "cross_w_out")]

    def __call__(self, x):
        x = _as_concat(x)
        self._upsert_variables(x.shape[1])
        w, b, wo = self.weights
        return _CrossFn.apply(self, x.xe, x.xd, w, b, wo)

    def l2(self):
        return self.l2_reg * 0.5 * (self.variables[self.prefix + "cross_w"].square().sum()
                                    + self.variables[self.prefix + "cross_w_out"].square().sum())


class _CrossMixFn(torch.autograd.Function):
    """engine.CrossMix (rm_dense_fwd / rm_cross_mix_fwd / rm_cross_mix_bwd / rm_dense_wgrad), as the DCN engine runs
    it under cross_type="mix"."""

    @staticmethod
    def forward(ctx, layer, xe, xd, v, gate, c, u, b, w_out):
        names = ("cross_v", "cross_gate", "cross_c", "cross_u", "cross_b", "cross_w_out")
        params = {n: t.detach().contiguous() for n, t in zip(names, (v, gate, c, u, b, w_out))}
        grads = {n: torch.empty_like(t) for n, t in params.items()}
        core = eng.CrossMix(params, grads, xe.shape[1], 0 if xd is None else xd.shape[1], layer.layer_num, layer.experts,
                        layer.low_rank, xe.device)
        logit = core.forward(xe.detach().contiguous(), None if xd is None else xd.detach().contiguous())
        ctx.core, ctx.has_xd = core, xd is not None
        return logit.clone().view(-1, 1)

    @staticmethod
    def backward(ctx, g):
        core = ctx.core
        core.backward(g.reshape(-1).contiguous())
        dx0 = core.cdx0
        d_xd = dx0[:, core.FD: core.d].clone() if ctx.has_xd else None
        gr = core.g
        return (None, dx0[:, : core.FD].clone(), d_xd, gr["cross_v"], gr["cross_gate"], gr["cross_c"], gr["cross_u"],
                gr["cross_b"], gr["cross_w_out"])


class CrossNetMix:
    """CrossNet's low-rank mixture-of-experts form (DCN-Mix, DCN-V2 arXiv 2008.13535 eq. 4-5):
    CrossNetMix(variables, layer_num, experts, low_rank, l2_reg)(x) -> logit [B,1], `.weights`, `.l2()`.  Per layer
    t = x_l V_l, s = x_l G_l, m = [softmax(s)_i tanh(tanh(t_i) C_l,i)]_i, x_{l+1} = x0 o (m U_l^T + b_l) + x_l;
    logit = x_L . w_out.  The gate G_l is per layer.  Variables: cross_v [L,d,E r] (glorot fans (d, r)), cross_gate
    [L,d,E] (d, E), cross_c [L,E,r,r] (r, r), cross_u [L,d,E r] (r, d), cross_b [L,d] zeros, cross_w_out [d,1]."""

    display_name = "CrossNetMix"
    NAMES = ("cross_v", "cross_gate", "cross_c", "cross_u", "cross_b", "cross_w_out")

    def __init__(self, variables, layer_num, experts, low_rank, l2_reg=0.0, prefix="", seed=2019):
        if not ops.cross_mix_supported(experts, low_rank):
            raise ValueError(f"CrossNetMix: experts={experts}, low_rank={low_rank} unsupported (1 <= experts <= 8, "
                             "low_rank in 8, 16, 32, 64, their product <= 256)")
        self.variables, self.layer_num, self.experts, self.low_rank = variables, int(layer_num), int(experts), int(low_rank)
        self.l2_reg, self.prefix, self.seed = l2_reg, prefix, seed

    def _upsert_variables(self, d):
        L, E, r, pre = self.layer_num, self.experts, self.low_rank, self.prefix

        def normal(shape, fan_in, fan_out):
            std = math.sqrt(2.0 / (fan_in + fan_out))
            g = torch.Generator(device=_device()).manual_seed(int(self.seed))
            t = torch.empty(shape, device=_device(), dtype=F32)
            torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std, generator=g)
            return t

        made = {"cross_v": lambda: normal((L, d, E * r), d, r), "cross_gate": lambda: normal((L, d, E), d, E),
                "cross_c": lambda: normal((L, E, r, r), r, r), "cross_u": lambda: normal((L, d, E * r), r, d),
                "cross_b": lambda: torch.zeros(L, d), "cross_w_out": lambda: glorot_normal([d, 1], self.seed)}
        for n in self.NAMES:
            if pre + n not in self.variables:
                self.variables[pre + n] = _leaf(made[n]())

    @property
    def weights(self):
        return [self.variables[self.prefix + n] for n in self.NAMES]

    def __call__(self, x):
        x = _as_concat(x)
        self._upsert_variables(x.shape[1])
        return _CrossMixFn.apply(self, x.xe, x.xd, *self.weights)

    def l2(self):
        return sum(self.l2_reg * 0.5 * self.variables[self.prefix + n].square().sum()
                   for n in self.NAMES if n != "cross_b")


# ------------------------------------------------------------------------------------------------
# AFM attention layer
# ------------------------------------------------------------------------------------------------
class _AFMFn(torch.autograd.Function):
    """rm_afm_fwd / rm_afm_bwd (csrc/afm.hip), as the AFM engine runs them."""

    @staticmethod
    def forward(ctx, E, W, b, h, p, mask):
        B, F, D = E.shape
        E_ = E.detach().contiguous()
        W_, b_, h_, p_ = (W.detach().contiguous(), b.detach().contiguous(), h.detach().reshape(-1).contiguous(),
                          p.detach().reshape(-1).contiguous())
        logit = torch.empty(B, device=E.device, dtype=F32)
        stats = torch.empty(B, ops.afm_stats_width(D), device=E.device, dtype=F32)
        ops.afm_fwd(E_, W_, b_, h_, p_, logit, mask=mask, stats=stats)
        ctx.save_for_backward(E_, W_, b_, h_, p_, logit, stats)
        ctx.mask = mask
        return logit.view(B, 1)

    @staticmethod
    def backward(ctx, g):
        E, W, b, h, p, logit, stats = ctx.saved_tensors
        B, F, D = E.shape
        T = W.shape[1]
        dev = E.device
        dE = torch.empty_like(E)
        dW, db, dh, dp = torch.empty_like(W), torch.empty_like(b), torch.empty_like(h), torch.empty_like(p)
        ws = torch.empty(max(4, ops.afm_bwd_workspace(B, F, D, T)), device=dev, dtype=F32)
        ops.afm_bwd(E, W, b, h, p, g.reshape(-1).contiguous(), logit, stats, dE, dW, db, dh, dp, ws, mask=ctx.mask)
        return dE, dW, db, dh.view(-1, 1), dp.view(-1, 1), None


class AFMLayer:
    """The class AFM.py:7 imports commented out and AFM.py:119-122 uses: AFMLayer(att_factor, att_dropout)(feat_embeds)
    -> logit [B,1], `.weights`, `.l2()`.  Arithmetic: arXiv 1708.04617 eq. (4)-(6): over the field pairs i < j,
    a_ij = softmax(h . relu(W^T (E_i * E_j) + b)), logit = p . dropout(sum_ij a_ij E_i * E_j).  Variables (names
    chosen here - the reference has none): afm_attention_w [D,T], afm_attention_b [T], afm_attention_h [T,1],
    afm_projection_p [D,1].  att_dropout is a KEEP probability, applied when called with training=True (or with an
    explicit `mask` [B,D] of multipliers, 0 or 1/keep).  l2(): the attention matrix only, as in the paper."""

    display_name = "AFM"
    names = ("afm_attention_w", "afm_attention_b", "afm_attention_h", "afm_projection_p")

    def __init__(self, variables, att_factor, att_dropout=1, l2_reg=0.0, prefix="", seed=2019):
        self.variables, self.att_factor, self.att_dropout = variables, int(att_factor), att_dropout
        self.l2_reg, self.prefix, self.seed = l2_reg, prefix, seed

    def _upsert_variables(self, D):
        T, pre, v = self.att_factor, self.prefix, self.variables
        if pre + "afm_attention_w" not in v:
            v[pre + "afm_attention_w"] = _leaf(glorot_normal([D, T], self.seed))
        if pre + "afm_attention_b" not in v:
            v[pre + "afm_attention_b"] = _leaf(torch.zeros(T))
        if pre + "afm_attention_h" not in v:
            v[pre + "afm_attention_h"] = _leaf(glorot_normal([T, 1], self.seed))
        if pre + "afm_projection_p" not in v:
            v[pre + "afm_projection_p"] = _leaf(glorot_normal([D, 1], self.seed))

    @property
    def weights(self):
        return [self.variables[self.prefix + n] for n in self.names]

    def __call__(self, E, training=False, mask=None):
        B, F, D = E.shape
        if not ops.afm_supported(F, D, self.att_factor):
            raise ValueError(f"AFMLayer: F={F}, D={D}, att_factor={self.att_factor} unsupported "
                             "(2..40 fields, D in 8/16/32/64, att_factor 1..64)")
        self._upsert_variables(D)
        if mask is None and training and self.att_dropout < 1:
            mask = _keep_mask((B, D), self.att_dropout) / self.att_dropout
        if mask is not None:
            mask = mask.detach().to(E.device, F32).contiguous()
        W, b, h, p = self.weights
        return _AFMFn.apply(E, W, b, h, p, mask)

    def l2(self):
        return self.l2_reg * 0.5 * self.variables[self.prefix + "afm_attention_w"].square().sum()


# ------------------------------------------------------------------------------------------------
# AutoInt interacting layer
# ------------------------------------------------------------------------------------------------
class _InteractingFn(torch.autograd.Function):
    """rm_autoint_layer_fwd / rm_autoint_layer_bwd (csrc/autoint.hip), as the AutoInt engine runs them."""

    @staticmethod
    def forward(ctx, X, Wq, Wk, Wv, Wr, H, scale):
        B, F, _ = X.shape
        X_ = X.detach().contiguous()
        Ws = [None if W is None else W.detach().contiguous() for W in (Wq, Wk, Wv, Wr)]
        Y = torch.empty(B, F, Ws[0].shape[1], device=X.device, dtype=F32)
        stats = torch.empty(B, H, F, 2, device=X.device, dtype=F32)
        ops.autoint_layer_fwd(X_, *Ws, H, scale, Y, stats=stats)
        ctx.save_for_backward(X_, Y, stats, *[W for W in Ws if W is not None])
        ctx.H, ctx.scale, ctx.res = H, scale, Ws[3] is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, Y, stats, *Ws = ctx.saved_tensors
        Ws = list(Ws) + ([] if ctx.res else [None])
        B, F, Din = X.shape
        dX = torch.empty_like(X)
        dWs = [None if W is None else torch.empty_like(W) for W in Ws]
        ws = torch.empty(max(4, ops.autoint_layer_bwd_workspace(B, F, Din, ctx.H, Ws[0].shape[1] // ctx.H)),
                         device=X.device, dtype=F32)
        ops.autoint_layer_bwd(X, *Ws, Y, stats, dY.contiguous(), ctx.H, ctx.scale, dX, *dWs, ws)
        return (dX, *dWs, None, None)


class InteractingLayer:
    """One interacting layer of AutoInt (arXiv 1810.11921 eq. (5)-(8); nothing in the reference implements it):
    InteractingLayer(variables, att_embedding_size, head_num, use_res, scaling)(X [B,F,Din]) -> Y [B,F,H dk],
        Q, K, V = X Wq, X Wk, X Wv;  a^h_m. = softmax_k(<Q^h_m, K^h_k> c);  Y_m = relu(concat_h sum_k a^h_mk V^h_k + X_m Wr)
    with c = 1, or 1/sqrt(dk) under `scaling`.  Variables (created on the first call, glorot-normal): {prefix}query_w,
    {prefix}key_w, {prefix}value_w and, with use_res, {prefix}res_w, each [Din, H dk]; the engine's layer l uses the
    prefix "autoint_layer_{l}_".  l2(): every matrix."""

    display_name = "Interacting"

    def __init__(self, variables, att_embedding_size=8, head_num=2, use_res=True, scaling=False,
                 prefix="autoint_layer_0_", seed=2019, l2_reg=0.0):
        self.variables, self.att_embedding_size, self.head_num = variables, int(att_embedding_size), int(head_num)
        self.use_res, self.scaling, self.prefix, self.seed, self.l2_reg = bool(use_res), bool(scaling), prefix, seed, l2_reg

    @property
    def names(self):
        return ("query_w", "key_w", "value_w") + (("res_w",) if self.use_res else ())

    @property
    def weights(self):
        return [self.variables[self.prefix + n] for n in self.names]

    def __call__(self, X):
        B, F, Din = X.shape
        H, dk = self.head_num, self.att_embedding_size
        if not ops.autoint_supported(F, Din, H, dk):
            raise ValueError(f"InteractingLayer: F={F}, Din={Din}, head_num={H}, att_embedding_size={dk} unsupported "
                             "(1..40 fields, Din in 8/16/32/64, head_num 1/2/4/8, att_embedding_size >= 4, head_num * "
                             "att_embedding_size in 8/16/32/64)")
        for i, n in enumerate(self.names):  # (a seed per matrix: equal shapes must not mean equal values)
            if self.prefix + n not in self.variables:
                self.variables[self.prefix + n] = _leaf(glorot_normal([Din, H * dk], self.seed + i))
        W = self.weights + ([] if self.use_res else [None])
        return _InteractingFn.apply(X, *W, H, float(dk) ** -0.5 if self.scaling else 1.0)

    def l2(self):
        return self.l2_reg * 0.5 * sum(w.square().sum() for w in self.weights)


# ------------------------------------------------------------------------------------------------
# DLRM dot interaction
# ------------------------------------------------------------------------------------------------
class _DotInteractFn(torch.autograd.Function):
    """rm_dot_interact_fwd / rm_dot_interact_bwd (csrc/dot_interact.hip), as the DLRM engine runs them."""

    @staticmethod
    def forward(ctx, E, z):
        E_, z_ = E.detach().contiguous(), z.detach().contiguous()
        B, F, D = E_.shape
        X = torch.empty(B, ops.dot_interact_width(F, D)[0], device=E.device, dtype=F32)
        ops.dot_interact_fwd(E_, z_, X)
        ctx.save_for_backward(E_, z_)
        return X

    @staticmethod
    def backward(ctx, dX):
        E, z = ctx.saved_tensors
        dE, dz = torch.empty_like(E), torch.empty_like(z)
        ops.dot_interact_bwd(E, z, dX.contiguous(), dE, dz)
        return dE, dz


class DotInteraction:
    """DLRM's interaction layer (arXiv 1906.00091; nothing in the reference implements it):
    DotInteraction()(feat_embeds [B,F,D], z [B,D]) -> [B, D + F(F+1)/2] = [z | <v_i, v_j> for 0 <= j < i <= F] with
    v_0 = z and v_f = feat_embeds[:, f-1] - the strict lower triangle, row-major, no diagonal.  No variables."""

    display_name = "DotInteraction"

    def __call__(self, feat_embeds, z):
        if feat_embeds.dim() != 3 or z.dim() != 2 or tuple(z.shape) != (feat_embeds.shape[0], feat_embeds.shape[2]):
            raise ValueError(f"DotInteraction: feat_embeds [B,F,D] and z [B,D] expected, got "
                             f"{tuple(feat_embeds.shape)} and {tuple(z.shape)}")
        _, F, D = feat_embeds.shape
        if not ops.dot_interact_supported(F, D):
            raise ValueError(f"DotInteraction: F={F}, D={D} unsupported (1..40 fields, D in 8/16/32/64)")
        return _DotInteractFn.apply(feat_embeds, z)

    def l2(self):
        return 0.0


# ------------------------------------------------------------------------------------------------
# FiBiNET interaction: SENET gate + bilinear pairs
# ------------------------------------------------------------------------------------------------
class _FiBiNETFn(torch.autograd.Function):
    """rm_fibinet_fwd / rm_fibinet_bwd (csrc/fibinet.hip), as the FiBiNET engine runs them."""

    @staticmethod
    def forward(ctx, btype, E, w1, w2, wb, wsb):
        ts = [t.detach().contiguous() for t in (E, w1, w2, wb, wsb)]
        B, F, D = ts[0].shape
        X = torch.empty(B, ops.fibinet_width(F, D)[0], device=E.device, dtype=F32)
        ops.fibinet_fwd(*ts, btype, X)
        ctx.save_for_backward(*ts)
        ctx.btype = btype
        return X

    @staticmethod
    def backward(ctx, dX):
        ts = ctx.saved_tensors
        B, F, D = ts[0].shape
        grads = [torch.empty_like(t) for t in ts]
        ws = torch.empty(max(4, ops.fibinet_bwd_workspace(B, F, D, ts[1].shape[1], ctx.btype)), device=dX.device,
                         dtype=F32)
        ops.fibinet_bwd(*ts, ctx.btype, dX.contiguous(), *grads, ws)
        return (None, *grads)


class FiBiNETInteraction:
    """FiBiNET's interaction layer (arXiv 1905.09433; nothing in the reference implements it):
    FiBiNETInteraction(variables, bilinear_type, reduction_ratio, l2_reg)(feat_embeds [B,F,D]) -> [B, 2 P D] =
    [bilinear(E) | bilinear(a o E)], P = F(F-1)/2 pairs i < j in itertools.combinations order, d fastest:
    a = relu(relu(mean_d(E) senet_w1) senet_w2), bilinear(Y)[(i,j)] = (Y_i W_(i)) o Y_j with W_(i) = W[0] ("all") or
    W[i] ("each").  Variables: senet_w1 [F,R], senet_w2 [R,F], R = max(1, F // reduction_ratio), bilinear_w and
    senet_bilinear_w [1 | F-1, D, D], all glorot; `.weights`, `.l2()`."""

    display_name = "FiBiNETInteraction"
    NAMES = ("senet_w1", "senet_w2", "bilinear_w", "senet_bilinear_w")

    def __init__(self, variables, bilinear_type="each", reduction_ratio=3, l2_reg=0.0, prefix="", seed=2019):
        if bilinear_type not in ops.FIBINET_TYPES:
            raise ValueError(f"FiBiNETInteraction: bilinear_type {bilinear_type!r} unsupported ('all' or 'each'; "
                             "'interaction', one matrix per pair, is out of scope)")
        if int(reduction_ratio) < 1:
            raise ValueError(f"FiBiNETInteraction: reduction_ratio={reduction_ratio} must be at least 1")
        self.variables, self.bilinear_type, self.reduction_ratio = variables, bilinear_type, int(reduction_ratio)
        self.l2_reg, self.prefix, self.seed = l2_reg, prefix, seed

    def _upsert_variables(self, F, D):
        R = max(1, F // self.reduction_ratio)
        nW = F - 1 if self.bilinear_type == "each" else 1
        g = torch.Generator(device=_device()).manual_seed(int(self.seed))  # one stream for the four variables

        def normal(shape, fan_in, fan_out):
            std = math.sqrt(2.0 / (fan_in + fan_out))
            t = torch.empty(shape, device=_device(), dtype=F32)
            torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std, generator=g)
            return t

        made = {"senet_w1": lambda: normal((F, R), F, R), "senet_w2": lambda: normal((R, F), R, F),
                "bilinear_w": lambda: normal((nW, D, D), D, D), "senet_bilinear_w": lambda: normal((nW, D, D), D, D)}
        for n in self.NAMES:
            if self.prefix + n not in self.variables:
                self.variables[self.prefix + n] = _leaf(made[n]())

    @property
    def weights(self):
        return [self.variables[self.prefix + n] for n in self.NAMES]

    def __call__(self, feat_embeds):
        if feat_embeds.dim() != 3:
            raise ValueError(f"FiBiNETInteraction: feat_embeds [B,F,D] expected, got {tuple(feat_embeds.shape)}")
        _, F, D = feat_embeds.shape
        if not ops.fibinet_supported(F, D, max(1, F // self.reduction_ratio), self.bilinear_type):
            raise ValueError(f"FiBiNETInteraction: F={F}, D={D} unsupported (2..40 fields, D in 8/16/32)")
        self._upsert_variables(F, D)
        return _FiBiNETFn.apply(self.bilinear_type, feat_embeds, *self.weights)

    def l2(self):
        return sum(self.l2_reg * 0.5 * self.variables[self.prefix + n].square().sum() for n in self.NAMES)


# ------------------------------------------------------------------------------------------------
# field-pair weighted FM: FmFM / FvFM / FwFM
# ------------------------------------------------------------------------------------------------
class _FieldPairFn(torch.autograd.Function):
    """rm_fmfm_fwd / rm_fmfm_bwd (csrc/fmfm.hip), as the FmFM engine runs them."""

    @staticmethod
    def forward(ctx, ftype, E, w):
        E, w = E.detach().contiguous(), w.detach().contiguous()
        logit = torch.empty(E.shape[0], device=E.device, dtype=F32)
        ops.fmfm_fwd(E, w, ftype, logit)
        ctx.save_for_backward(E, w)
        ctx.ftype = ftype
        return logit

    @staticmethod
    def backward(ctx, g):
        E, w = ctx.saved_tensors
        B, F, D = E.shape
        dE, dw = torch.empty_like(E), torch.empty_like(w)
        ws = torch.empty(max(4, ops.fmfm_bwd_workspace(B, F, D, ctx.ftype)), device=g.device, dtype=F32)
        ops.fmfm_bwd(E, w, ctx.ftype, g.contiguous(), dE, dw, ws)
        return None, dE, dw


class FieldPairInteraction:
    """The pair term of FmFM / FvFM / FwFM (arXiv 2102.12994, 1806.03514; nothing in the reference implements it):
    FieldPairInteraction(variables, field_interaction, l2_reg)(feat_embeds [B,F,D]) -> [B] =
    sum_{i<j} E_i W_(ij) E_j^T over the P = F(F-1)/2 pairs in itertools.combinations order, W_(ij) = field_pair_w[p]
    ("matrix", [P,D,D], the left field on the rows), diag(field_pair_w[p]) ("vector", [P,D]) or field_pair_w[p] I
    ("scalar", [P]).  The variable starts at plain FM (identity matrices / ones); `.weights`, `.l2()`."""

    display_name = "FieldPairInteraction"
    NAMES = ("field_pair_w",)

    def __init__(self, variables, field_interaction="matrix", l2_reg=0.0, prefix=""):
        if field_interaction not in ops.FMFM_TYPES:
            raise ValueError(f"FieldPairInteraction: field_interaction {field_interaction!r} is not one of 'matrix', "
                             "'vector', 'scalar'")
        self.variables, self.field_interaction, self.l2_reg, self.prefix = variables, field_interaction, l2_reg, prefix

    def _upsert_variables(self, F, D):
        name = self.prefix + "field_pair_w"
        if name not in self.variables:
            shape = ops.fmfm_weight_shape(F, D, self.field_interaction)
            t = torch.eye(D).expand(shape).clone() if len(shape) == 3 else torch.ones(shape)
            self.variables[name] = _leaf(t)

    @property
    def weights(self):
        return [self.variables[self.prefix + n] for n in self.NAMES]

    def __call__(self, feat_embeds):
        if feat_embeds.dim() != 3:
            raise ValueError(f"FieldPairInteraction: feat_embeds [B,F,D] expected, got {tuple(feat_embeds.shape)}")
        _, F, D = feat_embeds.shape
        if not ops.fmfm_supported(F, D, self.field_interaction):
            raise ValueError(f"FieldPairInteraction: F={F}, D={D} unsupported (2..40 fields, D in 8/16/32)")
        self._upsert_variables(F, D)
        return _FieldPairFn.apply(self.field_interaction, feat_embeds, *self.weights)

    def l2(self):
        return sum(self.l2_reg * 0.5 * self.variables[self.prefix + n].square().sum() for n in self.NAMES)


# ------------------------------------------------------------------------------------------------
# PNN's product layer
# ------------------------------------------------------------------------------------------------
class _ProductFn(torch.autograd.Function):
    """rm_pnn_fwd / rm_pnn_bwd (csrc/pnn.hip), as the PNN engine runs them."""

    @staticmethod
    def forward(ctx, products, ktype, E, k):
        E = E.detach().contiguous()
        k = k.detach().contiguous() if k is not None else None
        B, F, D = E.shape
        X = torch.empty(B, ops.pnn_width(F, D, products)[0], device=E.device, dtype=F32)
        ops.pnn_fwd(E, k, products, ktype, X)
        ctx.save_for_backward(*((E,) if k is None else (E, k)))
        ctx.products, ctx.ktype = products, ktype
        return X

    @staticmethod
    def backward(ctx, dX):
        E, k = (tuple(ctx.saved_tensors) + (None,))[:2]
        B, F, D = E.shape
        dE = torch.empty_like(E)
        dk = ws = None
        if k is not None:
            dk = torch.empty_like(k)
            ws = torch.empty(max(4, ops.pnn_bwd_workspace(B, F, D, ctx.products, ctx.ktype)), device=dX.device,
                             dtype=F32)
        ops.pnn_bwd(E, k, ctx.products, ctx.ktype, dX.contiguous(), dE, dk, ws)
        return None, None, dE, dk


class ProductLayer:
    """PNN's product layer (arXiv 1611.00144) in the kernel form of the widely used open-source PNN - not the paper's
    sum-pooled outer-product shortcut; nothing in the reference implements it:
    ProductLayer(variables, use_inner, use_outer, kernel_type, l2_reg)(feat_embeds [B,F,D]) -> [B, F D + n P] =
    [E flattened | <E_i, E_j> (use_inner) | E_i K_(ij) E_j^T (use_outer)] over the P = F(F-1)/2 pairs in
    itertools.combinations order, K_(ij) = product_kernel[p] ("mat", [P,D,D], the left field on the rows),
    diag(product_kernel[p]) ("vec", [P,D]) or product_kernel[p] I ("num", [P]).  The variable (with use_outer only)
    is glorot with fan D / D; `.weights`, `.l2()`."""

    display_name = "ProductLayer"
    NAMES = ("product_kernel",)

    def __init__(self, variables, use_inner=True, use_outer=False, kernel_type="mat", l2_reg=0.0, prefix="", seed=2019):
        if kernel_type not in ops.PNN_KERNELS:
            raise ValueError(f"ProductLayer: kernel_type {kernel_type!r} is not one of 'mat', 'vec', 'num'")
        self.products = ops.pnn_products(use_inner, use_outer)
        if not self.products:
            raise ValueError("ProductLayer: neither use_inner nor use_outer is set")
        self.variables, self.kernel_type, self.l2_reg, self.prefix, self.seed = variables, kernel_type, l2_reg, prefix, seed
        self.outer = bool(self.products & ops.PNN_OUTER)

    def _upsert_variables(self, F, D):
        name = self.prefix + "product_kernel"
        if self.outer and name not in self.variables:
            std = math.sqrt(2.0 / (D + D))
            t = torch.empty(ops.pnn_weight_shape(F, D, self.kernel_type), device=_device(), dtype=F32)
            g = torch.Generator(device=_device()).manual_seed(int(self.seed))
            torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std, generator=g)
            self.variables[name] = _leaf(t)

    @property
    def weights(self):
        return [self.variables[self.prefix + n] for n in self.NAMES] if self.outer else []

    def __call__(self, feat_embeds):
        if feat_embeds.dim() != 3:
            raise ValueError(f"ProductLayer: feat_embeds [B,F,D] expected, got {tuple(feat_embeds.shape)}")
        _, F, D = feat_embeds.shape
        if not ops.pnn_supported(F, D, self.products, self.kernel_type):
            raise ValueError(f"ProductLayer: F={F}, D={D} unsupported (2..40 fields, D in 8/16/32)")
        self._upsert_variables(F, D)
        return _ProductFn.apply(self.products, self.kernel_type, feat_embeds, *(self.weights or [None]))

    def l2(self):
        return sum((self.l2_reg * 0.5 * w.square().sum() for w in self.weights), 0.0)


# ------------------------------------------------------------------------------------------------
# MaskNet's MaskBlock
# ------------------------------------------------------------------------------------------------
def _mask_gemm(a, W, out, **kw):
    """ops.dense_fwd on the f32 kernel with a workspace of its own: allocated per call (a layer for composing models
    by hand, not the engine's hot path), sized for the square of the larger side as _dense_workspaces does, which
    covers the layer and its transposed use."""
    K, N = (W.shape[1], W.shape[0]) if kw.get("transposed") else W.shape
    fws = torch.empty(ops.dense_filter_workspace(max(K, N), max(K, N)), device=a.device, dtype=F32)
    ops.dense_fwd(a, None, W, out, fws, **kw)
    return out


def _mask_wgrad(a, G, db=None):
    dW = torch.empty(a.shape[1], G.shape[1], device=a.device, dtype=F32)
    ws = torch.empty(max(1, ops.dense_wgrad_workspace(a.shape[1], G.shape[1], a.shape[0])), device=a.device, dtype=F32)
    ops.dense_wgrad(a, None, G, dW, ws, db=db)
    return dW


class _MaskBlockFn(torch.autograd.Function):
    """One MaskBlock as the MaskNet engine runs it: the two mask layers and the hidden layer on ops.dense_fwd /
    ops.dense_wgrad, the normalise-and-mask passes on csrc/masknet.hip."""

    @staticmethod
    def forward(ctx, x, inp, Wa, ba, Wp, bp, Wh, g, b, eg, eb):
        x, inp = x.detach().contiguous(), inp.detach().contiguous()
        Wa, ba, Wp, bp, Wh, g, b = (t.detach().contiguous() for t in (Wa, ba, Wp, bp, Wh, g, b))
        norm = eg is not None
        if norm:
            eg, eb = eg.detach().contiguous(), eb.detach().contiguous()
        B, dev = x.shape[0], x.device
        A, wout, H = Wa.shape[1], Wp.shape[1], Wh.shape[1]
        T = torch.empty(B, (A + 3) // 4 * 4, device=dev, dtype=F32)[:, :A]
        _mask_gemm(x, Wa, T, bias=ba, act="relu")
        M = _mask_gemm(T, Wp, torch.empty(B, wout, device=dev, dtype=F32), bias=bp, act="identity")
        Y = torch.empty_like(M)
        ops.masknet_group_fwd(inp, eg, eb, [M], [Y], normalize=norm)
        Z = _mask_gemm(Y, Wh, torch.empty(B, H, device=dev, dtype=F32), act="identity")
        h = torch.empty_like(Z)
        ops.masknet_row_fwd(Z, g, b, h)
        ctx.save_for_backward(x, inp, Wa, Wp, Wh, g, b, T, M, Y, Z, *((eg, eb) if norm else ()))
        ctx.norm = norm
        return h

    @staticmethod
    def backward(ctx, dh):
        x, inp, Wa, Wp, Wh, g, b, T, M, Y, Z, *e = ctx.saved_tensors
        B, dev, H = x.shape[0], x.device, Z.shape[1]
        dh = dh.contiguous()
        dZ, dg, db = torch.empty_like(Z), torch.empty_like(g), torch.empty_like(b)
        ops.masknet_row_bwd(Z, g, b, dh, dZ, dg, db,
                            torch.empty(max(4, ops.masknet_row_bwd_workspace(B, H)), device=dev, dtype=F32))
        dWh = _mask_wgrad(Y, dZ)
        dY = _mask_gemm(dZ, Wh, torch.empty_like(Y), transposed=True, epilogue=ops.DENSE_ADD)
        dinp = torch.empty_like(inp)
        deg = deb = None
        if ctx.norm:
            deg, deb = torch.empty_like(e[0]), torch.empty_like(e[1])
            ws = torch.empty(max(4, ops.masknet_group_bwd_workspace(*inp.shape)), device=dev, dtype=F32)
            ops.masknet_group_bwd(inp, e[0], e[1], [M], [dY], [dY], dinp, deg, deb, ws)
        else:
            ops.masknet_group_bwd(inp, None, None, [M], [dY], [dY], dinp, normalize=False)
        dM = dY  # (in place)
        dbp, dba = torch.empty(Wp.shape[1], device=dev, dtype=F32), torch.empty(Wa.shape[1], device=dev, dtype=F32)
        dWp = _mask_wgrad(T, dM, dbp)
        dT = torch.empty(B, (T.shape[1] + 3) // 4 * 4, device=dev, dtype=F32)[:, : T.shape[1]]
        _mask_gemm(dM, Wp, dT, transposed=True, epilogue=ops.DENSE_MUL_ACTGRAD, act="relu", aux1=T)
        dWa = _mask_wgrad(x, dT, dba)
        dx = _mask_gemm(dT, Wa, torch.empty_like(x), transposed=True, epilogue=ops.DENSE_ADD)
        return dx, dinp, dWa, dba, dWp, dbp, dWh, dg, db, deg, deb


class MaskBlock:
    """MaskNet's block (arXiv 2102.07619; nothing in the reference implements it):
    MaskBlock(variables, hidden_units, reduction_ratio, l2_reg, prefix)(x [B,K], inputs) -> [B, hidden_units] =
    relu(LN((mask(x) o V) hidden_weights)), mask(x) = relu(x agg_weights + agg_bias) proj_weights + proj_bias with
    A = max(1, round(reduction_ratio * width of V)) aggregation units.  inputs [B,F,D] (the embedding rows): V is their
    per-field LayerNorm with the SHARED variables ln_emb_gamma / ln_emb_beta [F,D]; inputs [B,H'] (a previous
    block's output): V = inputs.  Variables {prefix}agg_weights / agg_bias / proj_weights / proj_bias /
    hidden_weights / ln_gamma / ln_beta, created on first use (glorot weights, zero biases, unit gains);
    `.weights`, `.l2()` over the three weight matrices."""

    display_name = "MaskBlock"
    NAMES = ("agg_weights", "agg_bias", "proj_weights", "proj_bias", "hidden_weights", "ln_gamma", "ln_beta")
    L2_NAMES = ("agg_weights", "proj_weights", "hidden_weights")

    def __init__(self, variables, hidden_units=64, reduction_ratio=2.0, l2_reg=0.0, prefix="block1_", seed=2019):
        if not ops.masknet_row_supported(hidden_units):
            raise ValueError(f"MaskBlock: hidden_units={hidden_units} must be a multiple of 4 in 8..2048")
        if not reduction_ratio > 0:
            raise ValueError(f"MaskBlock: reduction_ratio={reduction_ratio} must be greater than 0")
        self.variables, self.H, self.ratio, self.l2_reg = variables, int(hidden_units), float(reduction_ratio), l2_reg
        self.prefix, self.seed = prefix, seed

    def _upsert_variables(self, K, wout, emb_shape):
        v, pre, H = self.variables, self.prefix, self.H
        A = max(1, round(self.ratio * wout))
        made = {"agg_weights": lambda: glorot_normal([K, A], self.seed), "agg_bias": lambda: torch.zeros(A),
                "proj_weights": lambda: glorot_normal([A, wout], self.seed + 1),
                "proj_bias": lambda: torch.zeros(wout),
                "hidden_weights": lambda: glorot_normal([wout, H], self.seed + 2),
                "ln_gamma": lambda: torch.ones(H), "ln_beta": lambda: torch.zeros(H)}
        for n in self.NAMES:
            if pre + n not in v:
                v[pre + n] = _leaf(made[n]())
        if emb_shape is not None:
            if "ln_emb_gamma" not in v:
                v["ln_emb_gamma"] = _leaf(torch.ones(emb_shape))
            if "ln_emb_beta" not in v:
                v["ln_emb_beta"] = _leaf(torch.zeros(emb_shape))

    @property
    def weights(self):
        return [self.variables[self.prefix + n] for n in self.NAMES]

    def __call__(self, x, inputs):
        if x.dim() != 2 or inputs.dim() not in (2, 3) or inputs.shape[0] != x.shape[0]:
            raise ValueError(f"MaskBlock: x [B,K] and inputs [B,F,D] or [B,H] expected, got {tuple(x.shape)} and "
                             f"{tuple(inputs.shape)}")
        emb = inputs.dim() == 3
        F, D = (inputs.shape[1], inputs.shape[2]) if emb else (1, inputs.shape[1])
        if not ops.masknet_group_supported(F, D, 1, emb):
            raise ValueError(f"MaskBlock: inputs {tuple(inputs.shape)} unsupported (1..40 fields of 8/16/32, or a "
                             "width that is a multiple of 4 in 8..2048)")
        self._upsert_variables(x.shape[1], F * D, (F, D) if emb else None)
        ln = (self.variables["ln_emb_gamma"], self.variables["ln_emb_beta"]) if emb else (None, None)
        return _MaskBlockFn.apply(x, inputs, *self.weights, *ln)

    def l2(self):
        return sum(self.l2_reg * 0.5 * self.variables[self.prefix + n].square().sum() for n in self.L2_NAMES)


# ------------------------------------------------------------------------------------------------
# prediction + loss
# ------------------------------------------------------------------------------------------------
class _SigmoidFn(torch.autograd.Function):
    """PredictionLayer's sigmoid through rm_logit_loss (csrc/loss.hip)."""

    @staticmethod
    def forward(ctx, z):
        zf = z.detach().reshape(-1).contiguous()
        pred, logit = torch.empty_like(zf), torch.empty_like(zf)
        ops.logit_loss([(zf, 1.0)], task="classification", logit=logit, pred=pred)
        ctx.save_for_backward(pred)
        return pred

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return (g * p * (1 - p)).view(-1, 1)


class PredictionLayer:
    """layers.py:780-808: optional global bias, sigmoid for classification, reshape to [B]."""

    display_name = "Prediction"

    def __init__(self, variables, task="classification", use_bias=False, prefix=""):
        self.task, self.use_bias, self.prefix, self.variables = task, use_bias, prefix, variables

    def __call__(self, inputs):
        output = inputs.reshape(-1, 1)
        if self.use_bias:
            name = f"{self.prefix}global_bias"
            if name not in self.variables:
                self.variables[name] = _leaf(torch.zeros(1))
            output = output + self.variables[name]
        if self.task == "classification":
            return _SigmoidFn.apply(output)
        return output.reshape(-1)


def create_loss(y, pred, task="classification"):
    """create_loss (utils.py:192-198): Keras binary_crossentropy on PROBABILITIES (clip to
    [1e-7, 1 - 1e-7], epsilon inside the logs), mean over the batch; or MSE."""
    y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(pred.device, pred.dtype).reshape(-1)
    if task == "classification":
        pc = pred.clamp(KERAS_EPS, 1 - KERAS_EPS)
        return (-(y * torch.log(pc + KERAS_EPS) + (1 - y) * torch.log(1 - pc + KERAS_EPS))).mean()
    if task == "regression":
        return (pred - y).square().mean()
    raise ValueError(f"unknown task {task!r}")  # utils.py:198


__all__ = ["FeatEmbedding", "FeatEmbeddingLayer", "LinearCombiner", "LinearLayer", "SparseLinearCombiner",
           "SparseLinearLayer", "FMLayer", "DNNCombiner", "DNN", "CIN", "CrossNet", "CrossNetMix", "AFMLayer", "InteractingLayer",
           "FieldPairInteraction", "ProductLayer", "MaskBlock", "PredictionLayer",
           "create_loss", "glorot_normal", "glorot_uniform"]
