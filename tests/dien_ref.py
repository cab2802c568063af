"""CPU PyTorch restatement (dtype-generic, autograd) of the interest-evolution sequence lookup (SequenceFeat with
seq_pooling="dien"; Deep Interest Evolution Network, arXiv 1809.03672) and of the models that use it (DIEN; DCN with
such a sequence feature).

TEST INFRASTRUCTURE.  The reference has no code for the layer, so the arithmetic is the project's contract
(include/recman_hip.h).  Matrices are [in, out], the column blocks of a [D, 3D] matrix are [u | r | c].  Per example
with query row q and history rows k_1..k_n (CSR order, oldest first):

    cell(x, h; W, U, b, a):  u = sigmoid(x Wu + h Uu + bu),  r = sigmoid(x Wr + h Ur + br)
                             c = tanh(x Wc + r * (h Uc) + bc),  u = a u,  return (1 - u) h + u c
    h_0 = 0,  h_t = cell(k_t, h_{t-1}; gru_w, gru_u, gru_b, 1)
    s_t = h_t . (att_w q),  a = softmax_t(s)                         max-subtracted, over the example's n positions
    g_0 = 0,  g_t = cell(h_t, g_{t-1}; augru_w, augru_u, augru_b, a_t)
    out = g_n                                                        n = 0 -> 0, no gradient

computed on examples padded to the longest history with a mask: a finished example keeps its state.
tests/test_dien_host.py pins this file without a GPU - the extractor against torch.nn.GRU, the gradients against
central differences; the GPU tests compare the HIP kernels against it in float64.  The models are composed from the
public functions of oracle.th_layers, imported and not modified."""
import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.asp_ref import RANGE_SCALE, SeqSpec, segments  # noqa: F401  (the sequence front and its case limits)
from tests.ref_common import grad_measure_or_empty as grad_measure  # noqa: F401  (a batch may hold no history item)

NAMES = ("gru_w", "gru_u", "gru_b", "att_w", "augru_w", "augru_u", "augru_b")
BIG_BIAS = 100.0

# kernel-level GPU cases of tests/test_gpu_dien.py (keyword arguments of make_dien_case)
GPU_CASES = {
    "d16": dict(B=37, D=16, max_len=10),                 # the default shape
    "d8_long": dict(B=33, D=8, max_len=256),             # the longest recurrence and BPTT
    "d32": dict(B=45, D=32, max_len=50),                 # the widest weights
    "d16_len1": dict(B=35, D=16, max_len=1),             # a = 1 everywhere
    "d8_many": dict(B=130, D=8, max_len=5),              # many short examples per group
    "d16_grid_stride": dict(B=3001, D=16, max_len=20),   # several steps per block, block-order finish
}
# large scores under the softmax and saturated gates: att_w times RANGE_SCALE (tests/asp_ref.py: 4000) and every
# second bias entry of both GRUs +-100 with alternating sign.  The recurrent weights are NOT scaled: that would make
# the map chaotic, and no yardstick would mean anything.
RANGE_CASES = {
    "d16": dict(B=37, D=16, max_len=10),
    "d8_len30": dict(B=37, D=8, max_len=30),
}

# model-level GPU cases of tests/test_gpu_dien_model.py: keyword arguments of make_model_case
MODEL_CASES = {
    "dien_d8": dict(model="dien", B=37, D=8, Dn=2, seed=0),
    "dien_d16": dict(model="dien", B=61, D=16, Dn=3, seed=1, max_len=9),
    "dien_d32_dn0": dict(model="dien", B=37, D=32, Dn=0, seed=2),
    "dcn_d16": dict(model="dcn", B=37, D=16, Dn=2, seed=4),
}


def cell(x, h, W, U, b, a=None, pre=None):
    """One GRU step on rows: x, h [B, D]; a [B] scales the update gate (the AUGRU).  pre: a list that receives the
    three pre-activations [B, 3D]."""
    D = x.shape[1]
    xw, hu = x @ W + b, h @ U
    pu, pr = xw[:, :D] + hu[:, :D], xw[:, D:2 * D] + hu[:, D:2 * D]
    r = torch.sigmoid(pr)
    pc = xw[:, 2 * D:] + r * hu[:, 2 * D:]
    u = torch.sigmoid(pu)
    if a is not None:
        u = a.unsqueeze(1) * u
    if pre is not None:
        pre.append(torch.cat([pu, pr, pc], dim=1))
    return (1 - u) * h + u * torch.tanh(pc)


def dien_trace(Q, K, offsets, p):
    """The unit on padded examples: dict(out [B, D], H [B, T, D] the extractor's states, s [B, T] the scores (-inf on
    the padding), a [B, T], valid [B, T], pre_gru / pre_augru [B, T, 3D] the pre-activations), T = the longest
    history of the batch."""
    B, D = Q.shape
    n = offsets[1:] - offsets[:-1]
    T = int(n.max()) if B else 0
    dev = Q.device
    zero = torch.zeros(B, D, dtype=Q.dtype, device=dev)
    if T == 0:
        e, e3 = torch.zeros(B, 0, dtype=Q.dtype, device=dev), torch.zeros(B, 0, 3 * D, dtype=Q.dtype, device=dev)
        return dict(out=zero, H=e3[:, :, :D], s=e, a=e, valid=e.bool(), pre_gru=e3, pre_augru=e3)
    seg = segments(offsets)
    i = torch.arange(K.shape[0], device=dev) - offsets[:-1][seg]
    X = torch.zeros(B, T, D, dtype=Q.dtype, device=dev).index_put((seg, i), K)
    valid = torch.arange(T, device=dev).unsqueeze(0) < n.unsqueeze(1)
    h, Hs, pre1, pre2 = zero, [], [], []
    for t in range(T):
        h = torch.where(valid[:, t: t + 1], cell(X[:, t], h, p["gru_w"], p["gru_u"], p["gru_b"], None, pre1), h)
        Hs.append(h)
    H = torch.stack(Hs, dim=1)
    s = (H * (Q @ p["att_w"].T).unsqueeze(1)).sum(dim=2).masked_fill(~valid, float("-inf"))
    m = s.detach().amax(dim=1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    den = e.sum(dim=1, keepdim=True)
    a = e / torch.where(n.unsqueeze(1) > 0, den, torch.ones_like(den))
    g = zero
    for t in range(T):
        g = torch.where(valid[:, t: t + 1],
                        cell(H[:, t], g, p["augru_w"], p["augru_u"], p["augru_b"], a[:, t], pre2), g)
    return dict(out=g, H=H, s=s, a=a, valid=valid, pre_gru=torch.stack(pre1, 1), pre_augru=torch.stack(pre2, 1))


def dien_layer(Q, K, offsets, p):
    """Q [B,D] the examples' query rows, K [nnz,D] the history rows in CSR order, p: {name: tensor} over NAMES
    -> the pooled rows [B,D]."""
    return dien_trace(Q, K, offsets, p)["out"]


# ------------------------------------------------------------------------------------------------ layer-level cases
def make_dien_params(D, g, att_scale=1.0, big_bias=False):
    """Glorot matrices, biases ~ 0.1 N.  att_scale multiplies att_w; big_bias sets every second bias entry of both
    GRUs to +-BIG_BIAS with alternating sign."""
    rnd = C.rnd_stream(g)
    p = {}
    for n in ("gru", "augru"):
        p[n + "_w"] = rnd(D, 3 * D, std=(2.0 / (4 * D)) ** 0.5)
        p[n + "_u"] = rnd(D, 3 * D, std=(2.0 / (4 * D)) ** 0.5)
        b = rnd(3 * D, std=0.1)
        if big_bias:
            b[0::4], b[2::4] = BIG_BIAS, -BIG_BIAS
        p[n + "_b"] = b
    p["att_w"] = (rnd(D, D, std=(1.0 / D) ** 0.5) * att_scale).float().double()
    return {n: p[n] for n in NAMES}


def make_dien_case(B, D, max_len, V=23, seed=0, att_scale=1.0, big_bias=False):
    """A seeded kernel-level case.  table [V, 2D]: fused rows ~ 0.3 N(0,1) in EVERY column (the kernels must read
    columns 0..D-1 only); qidx [B]; CSR offsets / ids (lengths 0, 1, max_len first; the max_len example repeats an id);
    p: the 7 parameters; g [B, D] the pooled rows' gradient; dq_up [B, D] what the query-gradient buffer holds before
    the backward adds to it.  Every value is a float32 number."""
    g = torch.Generator().manual_seed(17000 + seed)
    rnd = C.rnd_stream(g)
    table, qidx, offsets, ids = C.draw_lookup(g, rnd, B, D, max_len, V)
    p = make_dien_params(D, g, att_scale, big_bias)
    return dict(B=B, D=D, max_len=max_len, table=table, qidx=qidx, offsets=offsets, ids=ids, p=p, g=rnd(B, D),
                dq_up=rnd(B, D, std=0.1))


def layer_reference(case, dtype=torch.float64):
    """dien_layer + autograd on a case in `dtype`: (out [B,D], d_keys [nnz,D], d_query [B,D] = dq_up + the query
    gradient, {name: gradient} over NAMES), all as float64."""
    D = case["D"]
    c = lambda t: t.to(dtype).clone().requires_grad_(True)  # noqa: E731
    Q, K = c(case["table"][case["qidx"], :D]), c(case["table"][case["ids"], :D])
    p = {n: c(v) for n, v in case["p"].items()}
    out = dien_layer(Q, K, case["offsets"], p)
    if out.requires_grad:
        (out * case["g"].to(dtype)).sum().backward()
    z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).detach().double()  # noqa: E731
    return out.detach().double(), z(K), case["dq_up"].to(dtype).double() + z(Q), {n: z(v) for n, v in p.items()}


# ---------------------------------------------------------------------------------------------------- the models
def dien_vars(p, prefix):
    return {n: p[f"{prefix}dien_{n}"] for n in NAMES}


def embeddings(p, spec, idx, mv, hp):
    """E [B, F, D]: table rows of the plain features, the evolved interest of the sequence features."""
    cols = []
    for f, n in enumerate(spec.sparse_names):
        if n in spec.seq_query:
            qn = spec.seq_query[n]
            T = p[f"{qn}_feat_embed"]
            offsets, ids = mv[n]
            cols.append(dien_layer(T[idx[:, spec.sparse_names.index(qn)]], T[ids], offsets, dien_vars(p, f"{n}_")))
        else:
            cols.append(p[f"{n}_feat_embed"][idx[:, f]])
    return torch.stack(cols, dim=1)


def model_logit(model, p, spec, idx, dense, hp, mv, training=True, masks=None):
    """DIEN: linear + DNN([E | dense]) (as DIN).  DCN (DCN.py:99-144): dnn + cross (+ linear)."""
    from tests import seq_models_ref as S  # (imports this module: what the three units' models share lives there)

    return S.unit_model_logit("dien", embeddings(p, spec, idx, mv, hp), model, p, spec, idx, dense, hp, training, masks)


def fwd_bwd(model, p, spec, idx, dense, y, hp, mv, task="classification", masks=None):
    """One forward+backward: (loss, logit [B], pred [B], grads) - the twin of oracle.th_layers.fwd_bwd."""
    from tests import seq_models_ref as S

    return S.unit_fwd_bwd(model_logit, "dien", model, p, spec, idx, dense, y, hp, mv, task, masks)


def make_model_case(model, B, D, Dn, seed=0, max_len=6, dtype=torch.float64):
    """A seeded model-level case (seq_models_ref.make_unit_model_case: its front and what it returns) of DIEN or of
    DCN over the dien unit; no unit of it has a kink, so there is no min_abs_z.  Item ids come from a small range, so
    rows are candidate in one example and history item in another."""
    from tests import seq_models_ref as S

    def draw_unit(g):
        return {f"hist_dien_{n}": v for n, v in make_dien_params(D, g).items()}

    return S.make_unit_model_case(19000, "dien", model, B, D, Dn, seed, max_len, dtype, dict(seq_pooling="dien"),
                                  draw_unit)
