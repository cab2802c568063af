"""CPU PyTorch restatement (dtype-generic, autograd) of the transformer-pooled sequence lookup (SequenceFeat with
seq_pooling="transformer"; Behavior Sequence Transformer, arXiv 1905.06874) and of the models that use it (BST; DCN with
such a sequence feature).

TEST INFRASTRUCTURE.  The reference has no code for the layer, so the arithmetic is the project's contract
(include/recman_hip.h).  Per example b with query row q and history rows k_0..k_{n-1} (CSR order, oldest first), T = n + 1:

    x_i = k_i + P[n - i]  (i < n),   x_n = q + P[0]                    P [max_len + 1, D]: by distance from the candidate
    Q, K, V = X Wq + bq, X Wk + bk, X Wv + bv                          heads h, dk = D / h
    a^h = softmax_j(Q^h_i . K^h_j / sqrt(dk))                          max-subtracted, every token real
    O = concat_h(a^h V^h) Wo + bo
    Y = LayerNorm(X + O; g1, b1)                                       eps 1e-5, biased variance
    Z = LayerNorm(Y + relu(Y W1 + c1) W2 + c2; g2, b2)
    out_b = (1 / T) sum_i Z_i                                          n = 0 -> Z_0 of the candidate alone

computed on examples padded to max_len + 1 tokens with a key mask (the padding's rows are dropped by the pooling).
tests/test_bst_host.py pins this file without a GPU - against torch.nn.TransformerEncoderLayer, example by example;
the GPU tests compare the HIP kernels against it in float64.  The models are composed from the public functions of
oracle.th_layers, imported and not modified."""
import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.asp_ref import KINK_CAP, RANGE_SCALE, SeqSpec, segments  # noqa: F401  (the sequence front, its case limits)
from tests.ref_common import KINK  # noqa: F401  (part of this module's interface; here the units are the FFN's)
from tests.ref_common import grad_measure_or_empty as grad_measure  # noqa: F401  (a batch may hold no history item)

NAMES = ("wq", "wk", "wv", "wo", "bq", "bk", "bv", "bo", "ffn_w1", "ffn_b1", "ffn_w2", "ffn_b2", "ln1_gamma", "ln1_beta",
         "ln2_gamma", "ln2_beta", "pos")
LN_EPS = 1e-5

# kernel-level GPU cases of tests/test_gpu_bst.py (keyword arguments of make_bst_case); tests/test_bst_host.py asserts the
# kink guard's cap on every one of them
GPU_CASES = {
    "d16_h2_f64": dict(B=37, D=16, heads=2, Hf=64, max_len=10),            # the default shape
    "d8_h1_f32_full": dict(B=130, D=8, heads=1, Hf=32, max_len=63),        # T = 64 fills a tile; single head
    "d32_h8_f128": dict(B=45, D=32, heads=8, Hf=128, max_len=20),          # dk = 4, widest FFN
    "d16_h4_f20": dict(B=61, D=16, heads=4, Hf=20, max_len=63),            # Hf not a multiple of 16 or 32
    "d8_h2_f128_short": dict(B=33, D=8, heads=2, Hf=128, max_len=5),       # many examples per tile
    "d16_grid_stride": dict(B=3001, D=16, heads=2, Hf=64, max_len=20),     # several steps per block, block-order finish
}
# large scores under the softmax: wq times RANGE_SCALE (tests/asp_ref.py: 4000).  The float32 CPU restatement is finite
# at that scale on both cases (asserted in tests/test_bst_host.py), so no smaller scale is needed.
RANGE_CASES = ("d16_h2_f64", "d8_h2_f128_short")

# model-level GPU cases of tests/test_gpu_bst_model.py: keyword arguments of make_model_case.  Their gradient comes from
# the labels and cannot be zeroed: the seeds are ones under which no FFN unit lies within KINK of 0 (asserted on the
# CPU in tests/test_bst_host.py)
MODEL_CASES = {
    "bst_d8": dict(model="bst", B=37, D=8, Dn=2, seed=0),
    "bst_d16_h4": dict(model="bst", B=61, D=16, Dn=3, seed=1, att_head_num=4, att_ffn_units=24),
    "bst_d32_dn0": dict(model="bst", B=37, D=32, Dn=0, seed=2, att_head_num=8),
    "dcn_d16": dict(model="dcn", B=37, D=16, Dn=2, seed=4),
}


def layer_norm(x, gamma, beta):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + LN_EPS) * gamma + beta


def bst_tokens(Q, K, offsets, P):
    """X [B, Tm, D] (Tm = P.shape[0]: history items first, the candidate behind them, zeros behind that) and the mask
    of the real tokens [B, Tm]."""
    B, Tm = Q.shape[0], P.shape[0]
    n = offsets[1:] - offsets[:-1]
    seg = segments(offsets)
    dev = Q.device
    i = torch.arange(K.shape[0], device=dev) - offsets[:-1][seg]
    X = torch.zeros(B, Tm, Q.shape[1], dtype=Q.dtype, device=dev)
    X = X.index_put((seg, i), K + P[n[seg] - i])
    X = X.index_put((torch.arange(B, device=dev), n), Q + P[0])
    return X, torch.arange(Tm, device=dev).unsqueeze(0) <= n.unsqueeze(1)


def bst_block(X, valid, p, heads, k_probe=None):
    """The encoder block on padded examples: (Z [B, Tm, D], the FFN pre-activations [B, Tm, Hf]).  k_probe [B, Tm, D]
    (zeros) is added to the projected keys: its gradient is the gradient of every token's key row."""
    B, Tm, D = X.shape
    dk = D // heads
    split = lambda t: t.reshape(B, Tm, heads, dk).transpose(1, 2)  # noqa: E731
    proj = {c: X @ p["w" + c] + p["b" + c] for c in "qkv"}
    if k_probe is not None:
        proj["k"] = proj["k"] + k_probe
    q, k, v = (split(proj[c]) for c in "qkv")
    s = (q @ k.transpose(2, 3)) / dk ** 0.5
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    a = torch.exp(s - s.detach().amax(dim=-1, keepdim=True))
    a = a / a.sum(dim=-1, keepdim=True)
    O = (a @ v).transpose(1, 2).reshape(B, Tm, D) @ p["wo"] + p["bo"]
    Y = layer_norm(X + O, p["ln1_gamma"], p["ln1_beta"])
    pre = Y @ p["ffn_w1"] + p["ffn_b1"]
    Z = layer_norm(Y + torch.relu(pre) @ p["ffn_w2"] + p["ffn_b2"], p["ln2_gamma"], p["ln2_beta"])
    return Z, pre


def bst_pool(Z, valid):
    T = valid.sum(dim=1, keepdim=True).to(Z.dtype)
    return torch.where(valid.unsqueeze(2), Z, torch.zeros_like(Z)).sum(dim=1) / T


def bst_layer(Q, K, offsets, p, heads, k_probe=None):
    """Q [B,D] the examples' query rows, K [nnz,D] the history rows in CSR order, p: {name: tensor} over NAMES
    -> the pooled rows [B,D].  k_probe: see bst_block."""
    X, valid = bst_tokens(Q, K, offsets, p["pos"])
    return bst_pool(bst_block(X, valid, p, heads, k_probe)[0], valid)


def ffn_kink_distance(Q, K, offsets, p, heads):
    """Per example, the smallest |FFN pre-activation| over its real tokens [B]."""
    X, valid = bst_tokens(Q, K, offsets, p["pos"])
    pre = bst_block(X, valid, p, heads)[1].abs().amin(dim=2)
    return torch.where(valid, pre, torch.full_like(pre, float("inf"))).amin(dim=1)


def key_grad_abs_sum(case):
    """sum over the tokens of |dLoss/dK_token| per column [D] of a kernel-level case in float64.  The key bias bk
    shifts every score of a query by the same Q_i . bk, which the softmax removes: d_bk = sum over the tokens of
    dLoss/dK_token is analytically ZERO, and what any implementation returns for it is the rounding residue of these
    terms, so they are the scale its d_bk is judged against (as dw0 under the softmax in tests/asp_ref.py)."""
    D = case["D"]
    X, valid = bst_tokens(case["table"][case["qidx"], :D], case["table"][case["ids"], :D], case["offsets"],
                          case["p"]["pos"])
    probe = torch.zeros_like(X).requires_grad_(True)
    out = bst_pool(bst_block(X, valid, case["p"], case["heads"], probe)[0], valid)
    (out * case["g"]).sum().backward()
    return probe.grad.abs().sum(dim=(0, 1))


# ------------------------------------------------------------------------------------------------ layer-level cases
def make_bst_params(D, heads, Hf, max_len, g, wq_scale=1.0):
    """Random and non-trivial in every member: glorot matrices, biases ~ 0.1 N, gains ~ 1 + 0.3 N, P ~ 0.3 N."""
    rnd = C.rnd_stream(g)
    p = {}
    for n in ("wq", "wk", "wv", "wo"):
        p[n] = rnd(D, D, std=(1.0 / D) ** 0.5)
    p["wq"] = (p["wq"] * wq_scale).float().double()
    for n in ("bq", "bk", "bv", "bo"):
        p[n] = rnd(D, std=0.1)
    p["ffn_w1"], p["ffn_b1"] = rnd(D, Hf, std=(2.0 / (D + Hf)) ** 0.5), rnd(Hf, std=0.1)
    p["ffn_w2"], p["ffn_b2"] = rnd(Hf, D, std=(2.0 / (D + Hf)) ** 0.5), rnd(D, std=0.1)
    for n in ("ln1", "ln2"):
        p[n + "_gamma"] = (1.0 + rnd(D, std=0.3)).float().double()
        p[n + "_beta"] = rnd(D, std=0.1)
    p["pos"] = rnd(max_len + 1, D, std=0.3)
    return {n: p[n] for n in NAMES}


def make_bst_case(B, D, heads, Hf, max_len, V=23, seed=0, wq_scale=1.0):
    """A seeded kernel-level case.  table [V, 2D]: fused rows ~ 0.3 N(0,1) in EVERY column (the kernels must read
    columns 0..D-1 only); qidx [B]; CSR offsets / ids (lengths 0, 1, max_len first; the max_len example repeats an id);
    p: the 17 parameters (wq times wq_scale); g [B, D] the pooled rows' gradient - ZERO for every example with an FFN
    unit whose pre-activation is within KINK of 0 in float64 (`near`, `zeroed` = their share); dq_up [B, D] what the
    query-gradient buffer holds before the backward adds to it.  Every value is a float32 number."""
    g = torch.Generator().manual_seed(11000 + seed)
    rnd = C.rnd_stream(g)
    table, qidx, offsets, ids = C.draw_lookup(g, rnd, B, D, max_len, V)
    p = make_bst_params(D, heads, Hf, max_len, g, wq_scale)
    gl = rnd(B, D)
    dq_up = rnd(B, D, std=0.1)
    near = ffn_kink_distance(table[qidx, :D], table[ids, :D], offsets, p, heads) < KINK
    gl = torch.where(near.unsqueeze(1), torch.zeros_like(gl), gl)
    return dict(B=B, D=D, heads=heads, Hf=Hf, max_len=max_len, table=table, qidx=qidx, offsets=offsets, ids=ids, p=p,
                g=gl, dq_up=dq_up, near=near, zeroed=float(near.double().mean()))


def layer_reference(case, dtype=torch.float64):
    """bst_layer + autograd on a case in `dtype`: (out [B,D], d_keys [nnz,D], d_query [B,D] = dq_up + the query
    gradient, {name: gradient} over NAMES), all as float64."""
    D = case["D"]
    c = lambda t: t.to(dtype).clone().requires_grad_(True)  # noqa: E731
    Q, K = c(case["table"][case["qidx"], :D]), c(case["table"][case["ids"], :D])
    p = {n: c(v) for n, v in case["p"].items()}
    out = bst_layer(Q, K, case["offsets"], p, case["heads"])
    (out * case["g"].to(dtype)).sum().backward()
    z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).detach().double()  # noqa: E731
    return out.detach().double(), z(K), case["dq_up"].to(dtype).double() + z(Q), {n: z(v) for n, v in p.items()}


# ---------------------------------------------------------------------------------------------------- the models
def bst_vars(p, prefix):
    return {n: p[f"{prefix}bst_{n}"] for n in NAMES}


def embeddings(p, spec, idx, mv, hp, k_probe=None):
    """E [B, F, D]: table rows of the plain features, the transformer-pooled history of the sequence features.
    k_probe [B, Tm, D] (zeros): added to the projected keys of every sequence feature (bst_block)."""
    cols = []
    for f, n in enumerate(spec.sparse_names):
        if n in spec.seq_query:
            qn = spec.seq_query[n]
            T = p[f"{qn}_feat_embed"]
            offsets, ids = mv[n]
            cols.append(bst_layer(T[idx[:, spec.sparse_names.index(qn)]], T[ids], offsets, bst_vars(p, f"{n}_"),
                                  hp.get("att_head_num", 2), k_probe))
        else:
            cols.append(p[f"{n}_feat_embed"][idx[:, f]])
    return torch.stack(cols, dim=1)


def model_logit(model, p, spec, idx, dense, hp, mv, training=True, masks=None, k_probe=None):
    """BST: linear + DNN([E | dense]) (as DIN).  DCN (DCN.py:99-144): dnn + cross (+ linear)."""
    from tests import seq_models_ref as S  # (imports this module: what the three units' models share lives there)

    E = embeddings(p, spec, idx, mv, hp, k_probe)
    return S.unit_model_logit("bst", E, model, p, spec, idx, dense, hp, training, masks)


def fwd_bwd(model, p, spec, idx, dense, y, hp, mv, task="classification", masks=None):
    """One forward+backward: (loss, logit [B], pred [B], grads) - the twin of oracle.th_layers.fwd_bwd."""
    from tests import seq_models_ref as S

    return S.unit_fwd_bwd(model_logit, "bst", model, p, spec, idx, dense, y, hp, mv, task, masks)


def model_key_grad_abs_sum(k, task="classification"):
    """key_grad_abs_sum for a model-level case (make_model_case): sum over the tokens of |dLoss/dK_token| per column
    [D] in float64 - the scale the analytically zero gradient of hist_bst_bk is judged against."""
    B, Tm, D = k["idx"].shape[0], k["spec"].seq_max_len["hist"] + 1, k["hp"]["embedding_size"]
    probe = torch.zeros(B, Tm, D, dtype=torch.float64, requires_grad=True)
    logit = model_logit(k["model"], k["p"], k["spec"], k["idx"], k["dense"], k["hp"], k["mv"], True, None, probe)
    TL.create_loss(k["y"], TL.prediction(logit, task), task).backward()
    return probe.grad.abs().sum(dim=(0, 1))


def make_model_case(model, B, D, Dn, seed=0, att_head_num=2, att_ffn_units=None, max_len=6, dtype=torch.float64):
    """A seeded model-level case (seq_models_ref.make_unit_model_case: its front and what it returns) of BST or of DCN
    over the transformer unit, with min_abs_z = the FFN pre-activation closest to 0 over the real tokens.  Item ids
    come from a small range, so rows are candidate in one example and history item in another."""
    from tests import seq_models_ref as S

    Hf = int(att_ffn_units or 4 * D)

    def draw_unit(g):
        return {f"hist_bst_{n}": v for n, v in make_bst_params(D, att_head_num, Hf, max_len, g).items()}

    def probe(p, idx, offsets, ids):
        T = p["item_feat_embed"]
        return float(ffn_kink_distance(T[idx[:, 1]], T[ids], offsets, bst_vars(p, "hist_"), att_head_num).min())

    unit_hp = dict(seq_pooling="transformer", att_head_num=att_head_num, att_ffn_units=Hf)
    return S.make_unit_model_case(13000, "bst", model, B, D, Dn, seed, max_len, dtype, unit_hp, draw_unit, probe)
