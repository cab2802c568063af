"""CPU PyTorch restatement (dtype-generic, autograd) of the attention-pooled sequence lookup (SequenceFeat) and of
the models that use it (DIN; DCN with a sequence feature).

TEST INFRASTRUCTURE.  The reference has no code for the layer (recman/tf/core/DIN.py:6 imports ASPCombiner / ASPLayer,
which exist nowhere), so the arithmetic is the paper's local activation unit (arXiv 1706.06978) as the project's
contract states it.  Per example b with query row q and history rows k_1..k_n (n = the CSR length):

    x_l = [q, k_l, q - k_l, q * k_l]                       (4D)
    z   = act(.. act(x_l W0 + b0) .. W_{m-1} + b_{m-1})    m = 1 or 2
    s_l = z . w + w0
    a_l = s_l  (norm off)   or   softmax_{l <= n}(s_l)  (norm on, max-subtracted)
    out_b = sum_l a_l k_l                                   n = 0 -> 0

The models are composed from the public functions of oracle.th_layers, imported and not modified.
tests/test_asp_host.py pins this file without a GPU; the GPU tests compare the HIP kernels against it in float64.
"""
import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK  # noqa: F401  (part of this module's interface)
from tests.ref_common import grad_measure_or_empty as grad_measure  # noqa: F401  (a batch may hold no history item)

KINK_CAP = 0.20    # largest share of examples the guard may zero

# kernel-level GPU cases of tests/test_gpu_asp.py (keyword arguments of make_asp_case); tests/test_asp_host.py asserts
# the kink guard's cap on every one of them
GPU_CASES = {
    "d16_80x40_sigmoid": dict(B=37, D=16, hidden=(80, 40), act="sigmoid", norm=False, max_len=10),
    "d16_80x40_relu_norm": dict(B=37, D=16, hidden=(80, 40), act="relu", norm=True, max_len=10),
    "d8_36_relu": dict(B=130, D=8, hidden=(36,), act="relu", norm=False, max_len=50),
    "d8_36_sigmoid_norm": dict(B=130, D=8, hidden=(36,), act="sigmoid", norm=True, max_len=50),
    "d32_16x8_sigmoid_norm": dict(B=45, D=32, hidden=(16, 8), act="sigmoid", norm=True, max_len=256),
    "d32_16x8_relu": dict(B=45, D=32, hidden=(16, 8), act="relu", norm=False, max_len=256),
    "d16_80x40_grid_stride": dict(B=3001, D=16, hidden=(80, 40), act="sigmoid", norm=False, max_len=50),
    "d16_80x40_relu_many_tiles": dict(B=701, D=16, hidden=(80, 40), act="relu", norm=True, max_len=50),
    "d32_128x128_relu_norm": dict(B=45, D=32, hidden=(128, 128), act="relu", norm=True, max_len=20),
    "d32_128x64_sigmoid": dict(B=77, D=32, hidden=(128, 64), act="sigmoid", norm=False, max_len=20),
    "d8_128_sigmoid_norm": dict(B=33, D=8, hidden=(128,), act="sigmoid", norm=True, max_len=7),
}
# large scores under the softmax: w times RANGE_SCALE
RANGE_CASES = {
    "d16_80x40_sigmoid_norm": dict(B=64, D=16, hidden=(80, 40), act="sigmoid", norm=True, max_len=30),
    "d8_36_relu_norm": dict(B=64, D=8, hidden=(36,), act="relu", norm=True, max_len=30),
}
RANGE_SCALE = 4000.0

# model-level GPU cases of tests/test_gpu_din_model.py: keyword arguments of make_model_case.  Their gradient comes
# from the labels and cannot be zeroed: with att_activation "relu" the seed is one under which no attention unit lies
# within KINK of 0 (asserted on the CPU in tests/test_asp_host.py)
MODEL_CASES = {
    "din_d8": dict(model="din", B=37, D=8, Dn=2, seed=0),
    "din_d16_norm": dict(model="din", B=61, D=16, Dn=3, seed=1, att_weight_normalization=True),
    "din_d32_relu": dict(model="din", B=37, D=32, Dn=0, seed=2, att_activation="relu", att_hidden_units=(16, 8)),
    "din_one_layer": dict(model="din", B=45, D=16, Dn=1, seed=3, att_hidden_units=(36,)),
    "dcn_d16": dict(model="dcn", B=37, D=16, Dn=2, seed=4),
}


def act_fn(name):
    if name == "relu":
        return torch.relu
    if name == "sigmoid":
        return torch.sigmoid
    raise NotImplementedError(name)


def segments(offsets):
    """The example index of every CSR position."""
    n = offsets[1:] - offsets[:-1]
    return torch.repeat_interleave(torch.arange(offsets.shape[0] - 1, device=offsets.device), n)


def asp_hidden(Q, K, offsets, Ws, bs, act):
    """Pre-activations of every hidden layer, per position: [z_0 [nnz,H0], ..]."""
    seg = segments(offsets)
    q = Q[seg]
    x = torch.cat([q, K, q - K, q * K], dim=1)
    f = act_fn(act)
    pre = []
    for W, b in zip(Ws, bs):
        pre.append(x @ W + b)
        x = f(pre[-1])
    return pre


def asp_scores(Q, K, offsets, Ws, bs, w, w0, act):
    pre = asp_hidden(Q, K, offsets, Ws, bs, act)
    return act_fn(act)(pre[-1]) @ w.reshape(-1) + w0.reshape(())


def asp_pool(s, K, offsets, norm):
    """Scores s [nnz] and history rows K [nnz,D] -> the pooled rows [B,D]."""
    B = offsets.shape[0] - 1
    seg = segments(offsets)
    if norm:
        m = torch.full((B,), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, seg, s.detach(), "amax")
        e = torch.exp(s - m[seg])
        den = torch.zeros(B, dtype=s.dtype, device=s.device).index_add(0, seg, e)
        a = e / den[seg]
    else:
        a = s
    return torch.zeros(B, K.shape[1], dtype=K.dtype, device=K.device).index_add(0, seg, a.unsqueeze(1) * K)


def asp_layer(Q, K, offsets, Ws, bs, w, w0, act="sigmoid", norm=False):
    """Q [B,D] the examples' query rows, K [nnz,D] the history rows in CSR order -> the pooled rows [B,D]."""
    return asp_pool(asp_scores(Q, K, offsets, Ws, bs, w, w0, act), K, offsets, norm)


def score_grad_abs_sum(case):
    """sum_l |dLoss/ds_l| of a kernel-level case in float64.  Under the softmax dw0 = sum_l dLoss/ds_l is
    analytically ZERO (a shift of every score changes nothing): what any implementation returns for it is the rounding
    residue of these terms, so they are the scale its dw0 is judged against."""
    D = case["D"]
    Q, K = case["table"][case["qidx"], :D], case["table"][case["ids"], :D]
    s = asp_scores(Q, K, case["offsets"], case["Ws"], case["bs"], case["w"], case["w0"], case["act"])
    s = s.detach().requires_grad_(True)
    (asp_pool(s, K, case["offsets"], case["norm"]) * case["g"]).sum().backward()
    return float(s.grad.abs().sum())


# ------------------------------------------------------------------------------------------------ layer-level cases
def make_asp_params(D, hidden, g, prefix="", w_scale=1.0):
    rnd = C.rnd_stream(g)
    dims = [4 * D] + list(hidden)
    p = {}
    for i in range(len(hidden)):
        p[f"{prefix}asp_layer_{i}_weights"] = C.glorot(rnd, (dims[i], dims[i + 1]), dims[i], dims[i + 1])
        p[f"{prefix}asp_layer_{i}_bias"] = rnd(dims[i + 1], std=0.1)
    p[f"{prefix}asp_w"] = (C.glorot(rnd, (dims[-1], 1), dims[-1], 1) * w_scale).float().double()
    p[f"{prefix}asp_w0"] = rnd(1, std=0.1)
    return p


def asp_vars(p, prefix, m):
    return ([p[f"{prefix}asp_layer_{i}_weights"] for i in range(m)], [p[f"{prefix}asp_layer_{i}_bias"] for i in range(m)],
            p[f"{prefix}asp_w"], p[f"{prefix}asp_w0"])


def make_asp_case(B, D, hidden, act, norm, max_len, V=23, seed=0, w_scale=1.0):
    """A seeded kernel-level case.  table [V, 2D]: fused rows ~ 0.3 N(0,1) in EVERY column (the kernels must read
    columns 0..D-1 only); qidx [B]; CSR offsets / ids (lengths 0, 1, max_len present; the max_len example repeats an
    id); glorot parameters (w times w_scale); g [B, D] the pooled rows' gradient - ZERO for every example that has a
    ReLU unit with a pre-activation within KINK of 0 in float64 (`near`, `zeroed` = their share); dq_up [B, D] what the
    query-gradient buffer holds before the backward adds to it."""
    g = torch.Generator().manual_seed(7000 + seed)
    rnd = C.rnd_stream(g)
    table, qidx, offsets, ids = C.draw_lookup(g, rnd, B, D, max_len, V)
    p = make_asp_params(D, hidden, g, w_scale=w_scale)
    gl = rnd(B, D)
    dq_up = rnd(B, D, std=0.1)
    Ws, bs, w, w0 = asp_vars(p, "", len(hidden))
    near = torch.zeros(B, dtype=torch.bool)
    if act == "relu":
        seg = segments(offsets)
        for z in asp_hidden(table[qidx, :D], table[ids, :D], offsets, Ws, bs, act):
            hit = (z.abs() < KINK).any(dim=1)
            near[seg[hit]] = True
    gl = torch.where(near.unsqueeze(1), torch.zeros_like(gl), gl)
    return dict(B=B, D=D, hidden=tuple(hidden), act=act, norm=norm, max_len=max_len, table=table, qidx=qidx,
                offsets=offsets, ids=ids, Ws=Ws, bs=bs, w=w, w0=w0, g=gl, dq_up=dq_up, near=near,
                zeroed=float(near.double().mean()))


def layer_reference(case, dtype=torch.float64):
    """asp_layer + autograd on a case in `dtype`: (out [B,D], d_keys [nnz,D], d_query [B,D] = dq_up + the query
    gradient, [dW_i ..], [db_i ..], dw, dw0), all as float64."""
    D = case["D"]
    c = lambda t: t.to(dtype).clone().requires_grad_(True)  # noqa: E731
    Q, K = c(case["table"][case["qidx"], :D]), c(case["table"][case["ids"], :D])
    Ws, bs = [c(W) for W in case["Ws"]], [c(b) for b in case["bs"]]
    w, w0 = c(case["w"]), c(case["w0"])
    out = asp_layer(Q, K, case["offsets"], Ws, bs, w, w0, case["act"], case["norm"])
    (out * case["g"].to(dtype)).sum().backward()
    z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).detach().double()  # noqa: E731
    return (out.detach().double(), z(K), case["dq_up"].to(dtype).double() + z(Q), [z(W) for W in Ws],
            [z(b) for b in bs], z(w), z(w0))


# ---------------------------------------------------------------------------------------------------- the models
class SeqSpec:
    """Embedding features in dictionary order; a sequence feature has feat_size 0 and names its query feature."""

    def __init__(self, sparse_names, feat_sizes, dense_names, seq_query, seq_max_len=None):
        self.sparse_names, self.feat_sizes, self.dense_names = list(sparse_names), list(feat_sizes), list(dense_names)
        self.seq_query = dict(seq_query)
        self.seq_max_len = dict(seq_max_len or {})
        self.plain = [n for n in self.sparse_names if n not in self.seq_query]
        # what oracle.th_layers sees: the features that own rows and linear entries
        self.tl = TL.Spec(self.plain, [v for n, v in zip(self.sparse_names, self.feat_sizes) if n not in self.seq_query],
                          self.dense_names)
        self.plain_cols = [f for f, n in enumerate(self.sparse_names) if n not in self.seq_query]

    @property
    def F(self):
        return len(self.sparse_names)


def embeddings(p, spec, idx, mv, hp):
    """E [B, F, D]: table rows of the plain features, the attention-pooled history of the sequence features."""
    m = len(hp["att_hidden_units"])
    cols = []
    for f, n in enumerate(spec.sparse_names):
        if n in spec.seq_query:
            qn = spec.seq_query[n]
            T = p[f"{qn}_feat_embed"]
            offsets, ids = mv[n]
            cols.append(asp_layer(T[idx[:, spec.sparse_names.index(qn)]], T[ids], offsets, *asp_vars(p, f"{n}_", m),
                                  hp.get("att_activation", "sigmoid"), hp.get("att_weight_normalization", False)))
        else:
            cols.append(p[f"{n}_feat_embed"][idx[:, f]])
    return torch.stack(cols, dim=1)


def model_logit(model, p, spec, idx, dense, hp, mv, training=True, masks=None):
    """DIN: linear + DNN([E | dense]).  DCN (DCN.py:99-144): dnn + cross (+ linear)."""
    from tests import seq_models_ref as S  # (imports this module: what the three units' models share lives there)

    return S.unit_model_logit("din", embeddings(p, spec, idx, mv, hp), model, p, spec, idx, dense, hp, training, masks)


def model_l2(model, p, spec, hp):
    out = TL.embedding_l2(p, spec.tl, hp.get("embedding_l2_reg", 0.0)) + TL.dnn_l2(
        p, len(hp["deep_hidden_units"]), hp.get("deep_l2_reg", 0.0))
    if model == "din" or hp.get("use_linear", True):
        out = out + TL.linear_l2(p, hp.get("linear_l2_reg", 0.0))
    if model == "dcn":
        out = out + TL.cross_l2(p, hp.get("cross_layer_l2_reg", 0.0))
    return out


def fwd_bwd(model, p, spec, idx, dense, y, hp, mv, task="classification", masks=None):
    """One forward+backward: (loss, logit [B], pred [B], grads) - the twin of oracle.th_layers.fwd_bwd."""
    from tests import seq_models_ref as S

    return S.unit_fwd_bwd(model_logit, "din", model, p, spec, idx, dense, y, hp, mv, task, masks)


def make_model_case(model, B, D, Dn, seed=0, att_hidden_units=(80, 40), att_activation="sigmoid",
                    att_weight_normalization=False, max_len=6, dtype=torch.float64):
    """A seeded model-level case (seq_models_ref.make_unit_model_case: its front and what it returns) of DIN or of DCN
    over the din unit, with min_abs_z = the attention unit's pre-activation closest to 0.  Item ids come from a small
    range, so rows are target in one example and history item in another."""
    from tests import seq_models_ref as S

    def probe(p, idx, offsets, ids):
        T = p["item_feat_embed"]
        Ws, bs = asp_vars(p, "hist_", len(att_hidden_units))[:2]
        pre = asp_hidden(T[idx[:, 1]], T[ids], offsets, Ws, bs, att_activation)
        return min(float(z.abs().min()) for z in pre)

    unit_hp = dict(att_hidden_units=tuple(att_hidden_units), att_activation=att_activation,
                   att_weight_normalization=att_weight_normalization)
    return S.make_unit_model_case(9000, "din", model, B, D, Dn, seed, max_len, dtype, unit_hp,
                                  lambda g: make_asp_params(D, att_hidden_units, g, prefix="hist_"), probe)
