"""What every float64 twin (tests/<model>_ref.py) needs besides its own arithmetic: the seeded float32-representable
streams, the measures the kernels are held to, the loss / backward wrapper and the scaffolding of a seeded case.

TEST INFRASTRUCTURE, a plain module.  A new model's twin starts here and adds only what is its own: its arithmetic, its
kernel cases, its logit and l2 composition, its hp.

THE DRAW ORDER IS FROZEN.  A case is made once and never changed: the tolerances in the tests and in profiles/*.md were
measured on these exact streams.  Every draw_* helper consumes the generator in the order written here, and a twin calls
them in its own sequence; tests/test_ref_common_host.py holds one fingerprint per family, so that a changed order fails
on a CPU instead of shifting a tolerance unnoticed.
"""
import functools
import inspect
import itertools

import torch

from oracle import th_layers as TL

KINK = 1e-6  # a relu unit whose float64 pre-activation is this close to 0 may flip in fp32


# ------------------------------------------------------------------------------------------ streams and measures
def rnd_stream(g):
    """rnd(*shape, std=1.0): N(0, std^2) draws from the generator g in float64, rounded to float32 values."""
    def rnd(*shape, std=1.0):
        # (every value is a float32 number: the kernels, the float32 restatement and float64 see the same inputs)
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * std).float().double()
    return rnd


def glorot(rnd, shape, fan_in, fan_out):
    return rnd(*shape, std=(2.0 / (fan_in + fan_out)) ** 0.5)


def to_f32(p):
    return {n: v.float() for n, v in p.items()}


def grad_measure(got, want):
    """The project's gradient measure (tests/test_gpu_parity.py:_close_grad) as a number: the largest
    |got - want| / max(|want|, 0.1 max|want|); an all-zero `want` demands an all-zero `got` (inf otherwise)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    scale = float(want.abs().max())
    if scale == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float(((got - want).abs() / torch.clamp(want.abs(), min=0.1 * scale)).max())


def grad_measure_or_empty(got, want):
    """grad_measure for the sequence units and the optimizers, where a gradient may have no entry at all (a batch
    without a history item): an empty `want` measures 0, where grad_measure itself raises."""
    return 0.0 if want.numel() == 0 else grad_measure(got, want)


def rel_error(got, want):
    """max |got - want| / max(1, |want|) over the elements: the forward's measure."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float(((got - want).abs() / want.abs().clamp(min=1.0)).max()) if got.numel() else 0.0


def memo(make):
    """make(*args, **kw) computed once per set of argument values (a case is made once, never changed), however they
    are passed: positional or by keyword, defaults left out or given, sequences as lists or tuples."""
    sig, cases = inspect.signature(make), {}

    def freeze(v):
        if isinstance(v, dict):
            return tuple(sorted((k, freeze(x)) for k, x in v.items()))
        return tuple(freeze(x) for x in v) if isinstance(v, (list, tuple)) else v

    @functools.wraps(make)
    def made_once(*args, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        key = freeze(bound.arguments)
        if key not in cases:
            cases[key] = make(*args, **kw)
        return cases[key]
    return made_once


# -------------------------------------------------------------------------------------------- loss and backward
def model_loss(logit_fn, l2_fn, p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None, **kw):
    """(loss + l2, logit [B,1], pred) of a model given by its *_logit and *_l2; kw goes to the logit."""
    logit = logit_fn(p, spec, idx, dense, hp, True, masks, mv=mv, **kw)
    pred = TL.prediction(logit, task)
    return TL.create_loss(y, pred, task) + l2_fn(p, spec, hp), logit, pred


def backward(loss_fn, p, *args, **kw):
    """loss_fn(leaves of p, *args, **kw) -> (loss, ..): the backward of the loss.  -> ((loss, ..) detached, grads);
    a variable the loss does not reach has a zero gradient."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    loss, *out = loss_fn(leaves, *args, **kw)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return (loss.detach(),) + tuple(t.detach() for t in out), grads


def fwd_bwd(loss_fn, p, *args, **kw):
    """One forward+backward of loss_fn -> (loss, logit [B,1], pred): (loss, logit [B], pred [B], grads) - the twin of
    oracle.th_layers.fwd_bwd."""
    (loss, logit, pred), grads = backward(loss_fn, p, *args, **kw)
    return loss, logit.reshape(-1), pred, grads


# ------------------------------------------------------------------------------------------ shared model pieces
def base_l2(p, spec, hp, n_dnn, use_linear):
    """The l2 terms every model has, in the order every model adds them: embeddings (+ linear) (+ the DNN's n_dnn
    layers and dnn_w; n_dnn None: no DNN)."""
    out = TL.embedding_l2(p, spec, hp.get("embedding_l2_reg", 0.0))
    if use_linear:
        out = out + TL.linear_l2(p, hp.get("linear_l2_reg", 0.0))
    if n_dnn is not None:
        out = out + TL.dnn_l2(p, n_dnn, hp.get("deep_l2_reg", 0.0))
    return out


def param_l2(names, p, l2_reg):
    """l2_reg / 2 times the sum of squares of the variables `names` that p holds (0.0 if it holds none)."""
    return sum((l2_reg * 0.5 * p[n].square().sum() for n in names if n in p), 0.0)


def pairs(F):
    """P = F(F-1)/2: the field pairs (i, j), 0 <= i < j < F."""
    return F * (F - 1) // 2


def pair_fields(F):
    """(left fields, right fields) of the P pairs in itertools.combinations order, as index tensors."""
    li, lj = zip(*itertools.combinations(range(F), 2))
    return torch.tensor(li), torch.tensor(lj)


def dnn_keep(hp, n, training):
    """The DNN's n + 1 keep probabilities: deep_dropout in training, all 1 otherwise."""
    return list(hp.get("deep_dropout") or [1] * (n + 1)) if training else [1] * (n + 1)


def dnn_pres(p, x, n, keep=None, dm=None):
    """The pre-activations of the relu DNN's n hidden layers on the input x, with oracle.th_layers.dnn's dropout."""
    keep, dm = keep or [1] * (n + 1), dm or [None] * (n + 1)
    pres, y = [], TL.dropout(x, keep[0], dm[0])
    for i in range(n):
        pres.append(y @ p[f"dnn_layer_{i}_weights"] + p[f"dnn_layer_{i}_bias"])
        y = TL.dropout(torch.relu(pres[-1]), keep[i + 1], dm[i + 1])
    return pres


def min_abs(pres):
    """The distance of the closest unit to its kink: the smallest |entry| of the non-empty tensors (inf for none)."""
    return min([float(t.abs().min()) for t in pres if t.numel()] + [float("inf")])


# --------------------------------------------------------------------------------------------- case scaffolding
def field_sizes(F):
    """The table sizes of F plain fields."""
    return [7, 11, 5, 13, 3, 17, 4, 9, 6, 8][:F] if F <= 10 else [5 + (i * 7) % 23 for i in range(F)]


def plain_spec(F, Dn):
    """F plain fields C0.. of field_sizes(F) and Dn dense features I0..: (spec, sizes)."""
    sizes = field_sizes(F)
    return TL.Spec([f"C{i}" for i in range(F)], sizes, [f"I{j}" for j in range(Dn)]), sizes


def draw_front(rnd, spec, D, std):
    """The tables ~ std N(0,1) of the features that own rows, then linear_w and linear_w0 ~ 0.1 N(0,1)."""
    p = {f"{n}_feat_embed": rnd(V, D, std=std) for n, V in zip(spec.sparse_names, spec.feat_sizes) if V}
    p["linear_w"] = rnd(getattr(spec, "tl", spec).lin_layout[2], 1, std=0.1)
    p["linear_w0"] = rnd(1, std=0.1)
    return p


def draw_dnn(rnd, p, dims, head=True, prefix=""):
    """Into p: {prefix}dnn_layer_{i}_weights (glorot) and _bias (0.1 N(0,1)) layer by layer, then with `head` the last
    projection {prefix}dnn_w (glorot) and {prefix}dnn_w0."""
    for i in range(len(dims) - 1):
        p[f"{prefix}dnn_layer_{i}_weights"] = glorot(rnd, (dims[i], dims[i + 1]), dims[i], dims[i + 1])
        p[f"{prefix}dnn_layer_{i}_bias"] = rnd(dims[i + 1], std=0.1)
    if head:
        p[f"{prefix}dnn_w"] = glorot(rnd, (dims[-1], 1), dims[-1], 1)
        p[f"{prefix}dnn_w0"] = rnd(1, std=0.1)


def draw_idx(g, sizes, B):
    """idx [B, F]: uniform ids per field; a field without rows (size 0) holds the placeholder 0 and draws nothing."""
    return torch.stack([torch.randint(0, v, (B,), generator=g) if v else torch.zeros(B, dtype=torch.int64)
                        for v in sizes], 1)


def draw_labels(g, B, p_pos=0.3):
    return (torch.rand(B, generator=g) < p_pos).long()


def draw_batch(g, rnd, sizes, B, Dn, p_pos=0.3):
    """idx, then dense ~ N(0,1), then the labels (a share p_pos positive)."""
    return draw_idx(g, sizes, B), rnd(B, Dn), draw_labels(g, B, p_pos)


def first_stream(seed0, build, ok, attempts=64):
    """build(g, rnd) on the generators seeded seed0, seed0 + 1, ..: (the first result ok() accepts, its attempt)."""
    for attempt in range(attempts):
        g = torch.Generator().manual_seed(seed0 + attempt)
        out = build(g, rnd_stream(g))
        if ok(out):
            return out, attempt
    raise AssertionError("no stream met the case conditions")


# ------------------------------------------------------------------------------------------- sequence features
def draw_lengths(g, B, max_len):
    """History lengths in 0..max_len; the first examples are 0, 1 and max_len long."""
    n = torch.randint(0, max_len + 1, (B,), generator=g)
    forced = [0, 1, max_len][:B]
    n[: len(forced)] = torch.tensor(forced)
    return n


def draw_history(g, B, max_len, V):
    """B histories in CSR form: (offsets [B+1] of draw_lengths, then ids [nnz] uniform below V)."""
    n = draw_lengths(g, B, max_len)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    return offsets, torch.randint(0, V, (int(n.sum()),), generator=g)


def draw_lookup(g, rnd, B, D, max_len, V):
    """What a pooling unit's kernel case looks up: table [V, 2D], fused rows ~ 0.3 N(0,1) in EVERY column (the kernels
    must read columns 0..D-1 only); qidx [B]; a history per example (the max_len example repeats an id)."""
    table = rnd(V, 2 * D, std=0.3)
    qidx = torch.randint(0, V, (B,), generator=g)
    offsets, ids = draw_history(g, B, max_len, V)
    if B >= 3 and max_len >= 2:
        ids[int(offsets[2]) + 1] = ids[int(offsets[2])]  # a repeated id inside one history
    return table, qidx, offsets, ids
