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

KINK = 1e-6        # a ReLU unit whose float64 pre-activation is this close to 0 may flip in fp32
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


def grad_measure(got, want):
    """The project's gradient measure (tests/test_gpu_parity.py:_close_grad) as a number: the largest
    |got - want| / max(|want|, 0.1 max|want|); an all-zero `want` demands an all-zero `got` (inf otherwise)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    if want.numel() == 0:
        return 0.0
    scale = float(want.abs().max())
    if scale == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float(((got - want).abs() / torch.clamp(want.abs(), min=0.1 * scale)).max())


# ------------------------------------------------------------------------------------------------ layer-level cases
def _rnd(g):
    def rnd(*shape, std=1.0):
        # (every value is a float32 number: the kernels, the float32 restatement and float64 see the same inputs)
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * std).float().double()
    return rnd


def make_lengths(B, max_len, g):
    """History lengths in 0..max_len; the first examples are 0, 1 and max_len long."""
    n = torch.randint(0, max_len + 1, (B,), generator=g)
    forced = [0, 1, max_len][:B]
    n[: len(forced)] = torch.tensor(forced)
    return n


def make_asp_params(D, hidden, g, prefix="", w_scale=1.0):
    rnd = _rnd(g)
    dims = [4 * D] + list(hidden)
    p = {}
    for i in range(len(hidden)):
        p[f"{prefix}asp_layer_{i}_weights"] = rnd(dims[i], dims[i + 1], std=(2.0 / (dims[i] + dims[i + 1])) ** 0.5)
        p[f"{prefix}asp_layer_{i}_bias"] = rnd(dims[i + 1], std=0.1)
    p[f"{prefix}asp_w"] = (rnd(dims[-1], 1, std=(2.0 / (dims[-1] + 1)) ** 0.5) * w_scale).float().double()
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
    rnd = _rnd(g)
    table = rnd(V, 2 * D, std=0.3)
    qidx = torch.randint(0, V, (B,), generator=g)
    n = make_lengths(B, max_len, g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    ids = torch.randint(0, V, (int(n.sum()),), generator=g)
    if B >= 3 and max_len >= 2:
        ids[int(offsets[2]) + 1] = ids[int(offsets[2])]  # a repeated id inside one history
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
    masks = masks or {}
    E = embeddings(p, spec, idx, mv, hp)
    x = TL.dnn_input(E, dense)
    n = len(hp["deep_hidden_units"])
    keep = hp.get("deep_dropout", [1] * (n + 1)) if training else [1] * (n + 1)
    dnn = TL.dnn(p, x, n, hp.get("deep_activation", "relu"), keep, masks.get("dnn"))
    lin = TL.linear_layer(p, spec.tl, idx[:, spec.plain_cols], dense)
    if model == "din":
        return lin + dnn
    assert model == "dcn"
    logit = dnn + TL.cross_net(p, x)
    return logit + lin if hp.get("use_linear", True) else logit


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
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logit = model_logit(model, leaves, spec, idx, dense, hp, mv, True, masks)
    pred = TL.prediction(logit, task)
    loss = TL.create_loss(y, pred, task) + model_l2(model, leaves, spec, hp)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return loss.detach(), logit.detach().reshape(-1), pred.detach(), grads


def make_model_case(model, B, D, Dn, seed=0, att_hidden_units=(80, 40), att_activation="sigmoid",
                    att_weight_normalization=False, max_len=6, dtype=torch.float64):
    """A seeded model-level case: plain features C0 (7), item (11), C2 (5), the history `hist` of `item` between them
    (so the pooled row is not the last field), Dn dense features.  Item ids come from a small range, so rows are
    target in one example and history item in another.  Returns spec, p (reference variable names), idx (the
    sequence's column is a placeholder 0), dense, y, hp, mv = {"hist": (offsets, ids)}, min_abs_z (the attention
    unit's pre-activation closest to 0)."""
    g = torch.Generator().manual_seed(9000 + seed)
    rnd = _rnd(g)
    names, sizes = ["C0", "item", "hist", "C2"], [7, 11, 0, 5]
    spec = SeqSpec(names, sizes, [f"I{j}" for j in range(Dn)], {"hist": "item"}, {"hist": max_len})
    p = {}
    for n, V in zip(names, sizes):
        if V:
            p[f"{n}_feat_embed"] = rnd(V, D, std=0.3)
    p["linear_w"] = rnd(spec.tl.lin_layout[2], 1, std=0.1)
    p["linear_w0"] = rnd(1, std=0.1)
    hidden = (32, 32) if model == "din" else (24, 16)
    d_in = len(names) * D + Dn
    dims = [d_in] + list(hidden)
    for i in range(len(hidden)):
        p[f"dnn_layer_{i}_weights"] = rnd(dims[i], dims[i + 1], std=(2.0 / (dims[i] + dims[i + 1])) ** 0.5)
        p[f"dnn_layer_{i}_bias"] = rnd(dims[i + 1], std=0.1)
    p["dnn_w"] = rnd(dims[-1], 1, std=(2.0 / (dims[-1] + 1)) ** 0.5)
    p["dnn_w0"] = rnd(1, std=0.1)
    hp = dict(embedding_size=D, embedding_l2_reg=1e-3, linear_l2_reg=1e-3, deep_hidden_units=hidden,
              deep_l2_reg=1e-3, deep_activation="relu", att_hidden_units=tuple(att_hidden_units),
              att_activation=att_activation, att_weight_normalization=att_weight_normalization)
    if model == "dcn":
        L = 2
        p["cross_w"], p["cross_b"] = rnd(L, d_in, std=0.15), rnd(L, d_in, std=0.15)
        p["cross_w_out"] = rnd(d_in, 1, std=0.15)
        hp.update(cross_layer_num=L, cross_layer_l2_reg=1e-3, use_linear=True)
    p.update(make_asp_params(D, att_hidden_units, g, prefix="hist_"))
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) if v else torch.zeros(B, dtype=torch.int64)
                       for v in sizes], 1)
    n = make_lengths(B, max_len, g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    ids = torch.randint(0, sizes[1], (int(n.sum()),), generator=g)
    dense = rnd(B, Dn)
    y = (torch.rand(B, generator=g) < 0.3).long()
    T = p["item_feat_embed"]
    pre = asp_hidden(T[idx[:, 1]], T[ids], offsets, *asp_vars(p, "hist_", len(att_hidden_units))[:2], att_activation)
    c = lambda t: t.to(dtype) if t.is_floating_point() else t  # noqa: E731
    return dict(model=model, spec=spec, p={k: c(v) for k, v in p.items()}, idx=idx, dense=c(dense), y=y, hp=hp,
                mv={"hist": (offsets, ids)}, min_abs_z=min(float(z.abs().min()) for z in pre))
