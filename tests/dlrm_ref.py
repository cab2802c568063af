"""CPU PyTorch restatement (dtype-generic, autograd) of DLRM's dot interaction and of the model.

TEST INFRASTRUCTURE.  Nothing in the reference implements the model, so the arithmetic is the paper's (arXiv 1906.00091)
as the project's contract states it.  With v_0 = z [B,D] and v_f = E[:, f-1] (f = 1..F), T = F + 1, P = F(F+1)/2:

    X[:, 0:D] = z;   X[:, D + i(i-1)/2 + j] = <v_i, v_j>  for 0 <= j < i <= F   (strict lower triangle, row-major)
    backward: G_ij = G_ji = dX[:, D + p(i,j)], G_ii = 0;  dV = G V;  d_rows = dV[:, 1:];  dz = dV[:, 0] + dX[:, 0:D]

    bottom tower: a_0 = dense, a_{l+1} = act(a_l W_l + b_l), widths bottom_hidden_units + (D,), z = a_last
    top tower:    DNN(X) with the variables top_dnn_layer_{l}_weights / _bias, top_dnn_w, top_dnn_w0
    logit = top (+ linear with use_linear)

The model is composed from the public functions of oracle.th_layers, imported and not modified.
tests/test_dlrm_host.py pins this file without a GPU; the GPU tests compare the HIP kernels against it in float64.
"""
from functools import partial

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK, grad_measure  # noqa: F401  (part of this module's interface)
from tests.ref_common import rnd_stream as _rnd  # noqa: F401  (tests/test_gpu_dlrm_model.py draws with it)

# kernel-level GPU cases (B, F, D) of tests/test_gpu_dot_interact.py
GPU_CASES = [(3, 1, 8), (5, 2, 16), (6, 7, 16), (5, 5, 32), (9, 31, 16), (9, 32, 16), (4, 40, 64), (131, 26, 16),
             (70001, 3, 8)]
EPS23 = 2.0 ** -23

# model-level GPU cases of tests/test_gpu_dlrm_model.py: keyword arguments of make_case.  The label-driven upstream
# gradient cannot be zeroed, so the seeds are such that no unit of either tower (z's own pre-activation included) lies
# within KINK of 0 (asserted on the CPU in tests/test_dlrm_host.py).  Every case has non-zero l2 terms.
MODEL_CASES = {
    "d8": dict(B=37, F=5, D=8, Dn=2, seed=0),
    "d16": dict(B=37, F=5, D=16, Dn=3, seed=0),
    "d32": dict(B=29, F=6, D=32, Dn=2, seed=0),
    "linear": dict(B=37, F=5, D=16, Dn=2, seed=1, use_linear=True),
    "no_bottom_hidden": dict(B=41, F=4, D=8, Dn=3, seed=0, bottom=()),
    "no_pad": dict(B=45, F=7, D=16, Dn=2, seed=0),  # D + P = 44: the interaction's rows need no pad column
    "criteo_like": dict(B=150, F=26, D=16, Dn=13, seed=0, bottom=(64, 32), hidden=(32, 32)),
}


def pairs(F):
    """P = F(F+1)/2."""
    return F * (F + 1) // 2


def pair_index(i, j):
    """p(i, j) for 0 <= j < i."""
    assert 0 <= j < i
    return i * (i - 1) // 2 + j


def stack_v(E, z):
    return torch.cat([z.unsqueeze(1), E], dim=1)  # [B,T,D]


def interact(E, z):
    """E [B,F,D], z [B,D] -> X [B, D+P]: bmm + triangular indices."""
    V = stack_v(E, z)
    T = V.shape[1]
    gram = torch.bmm(V, V.transpose(1, 2))
    li, lj = torch.tril_indices(T, T, offset=-1)  # row-major over the strict lower triangle: (1,0), (2,0), (2,1), ..
    return torch.cat([z, gram[:, li, lj]], dim=1)


def interact_loops(E, z):
    """The same as explicit Python loops over (i, j) (lists and floats, no tensor arithmetic)."""
    El, zl = E.tolist(), z.tolist()
    out = []
    for b in range(len(El)):
        v = [zl[b]] + El[b]
        row = list(zl[b])
        for i in range(1, len(v)):
            for j in range(i):
                row.append(sum(a * c for a, c in zip(v[i], v[j])))
        out.append(row)
    return torch.tensor(out, dtype=E.dtype).reshape(len(El), -1)


def gram_grad(dX, F, D):
    """dX [B, >= D+P] -> the symmetric G [B,T,T] with a zero diagonal."""
    T = F + 1
    li, lj = torch.tril_indices(T, T, offset=-1)
    G = dX.new_zeros(dX.shape[0], T, T)
    G[:, li, lj] = dX[:, D: D + pairs(F)]
    return G + G.transpose(1, 2)


def interact_bwd(E, z, dX):
    """The backward of the contract, written out (no autograd): -> (d_rows [B,F,D], dz [B,D])."""
    _, F, D = E.shape
    dV = torch.bmm(gram_grad(dX, F, D), stack_v(E, z))
    return dV[:, 1:], dV[:, 0] + dX[:, :D]


def fwd_bound(E, z):
    """[B,P]: D 2^-23 sum_k |v_ik v_jk| - the textbook n 2^-24 sum |a b| of a length-D dot product in any summation
    order (and of an fmaf chain), doubled for the neglected second-order term."""
    V = stack_v(E, z).abs()
    T, D = V.shape[1], V.shape[2]
    li, lj = torch.tril_indices(T, T, offset=-1)
    return D * EPS23 * torch.bmm(V, V.transpose(1, 2))[:, li, lj]


def bwd_bound(E, z, dX):
    """[B,T,D]: (T+1) 2^-23 sum_j |G_ij| |v_jk| (row 0: dz, whose sum has the pass-through term as a T-th addend)."""
    _, F, D = E.shape
    Ga = gram_grad(dX, F, D).abs()
    b = torch.bmm(Ga, stack_v(E, z).abs())
    b[:, 0] += dX[:, :D].abs()
    return (F + 2) * EPS23 * b


def glorot(rnd, fan_in, fan_out):
    """A [fan_in, fan_out] matrix."""
    return C.glorot(rnd, (fan_in, fan_out), fan_in, fan_out)


@C.memo
def kernel_case(B, F, D, seed=0):
    """A seeded kernel-level case in float64 (made once per shape, never changed): E, z, dX ~ N(0,1); example 1 has all
    its E rows zero, example 2 has z = 0.  With the float64 outputs X, d_rows, dz and the bounds."""
    rnd = C.rnd_stream(torch.Generator().manual_seed(5000 + seed))
    E, z, dX = rnd(B, F, D), rnd(B, D), rnd(B, D + pairs(F))
    E[1 % B] = 0.0
    z[2 % B] = 0.0
    d_rows, dz = interact_bwd(E, z, dX)
    return dict(B=B, F=F, D=D, E=E, z=z, dX=dX, X=interact(E, z), d_rows=d_rows, dz=dz, bx=fwd_bound(E, z),
                bdv=bwd_bound(E, z, dX))


def _ratio(err, bound):
    """max err / bound; an entry with a zero bound must have a zero error (inf otherwise)."""
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0))
    return float(r.max()) if r.numel() else 0.0


def check_fwd(X, case, what=""):
    """The kernel test's forward assertions on X [B, ldx >= D+P] (any float dtype): X[:, :D] is z's bits, columns from
    D+P on are +0.0, everything finite, |X - X64| <= the bound elementwise.  Returns the worst err / bound."""
    D, W = case["D"], case["X"].shape[1]
    X = X.detach().cpu()
    assert X.shape[0] == case["B"] and X.shape[1] >= W, f"{what}X has shape {tuple(X.shape)}"
    assert bool(torch.isfinite(X).all()), f"{what}X is not finite"
    assert torch.equal(X[:, :D].double(), case["z"]), f"{what}X[:, :D] is not z bit for bit"
    pad = X[:, W:]
    assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any()), f"{what}columns >= D+P are not +0.0"
    r = _ratio((X[:, D:W].double() - case["X"][:, D:]).abs(), case["bx"])
    assert r <= 1.0, f"{what}|X - X64| is {r:.3g} x the bound"
    return r


def check_bwd(d_rows, dz, case, what=""):
    """The kernel test's backward assertions: finite, |dV - dV64| <= the bound elementwise.  Returns the worst
    err / bound of (d_rows, dz)."""
    d_rows, dz = d_rows.detach().cpu(), dz.detach().cpu()
    assert d_rows.shape == case["d_rows"].shape and dz.shape == case["dz"].shape, f"{what}shapes"
    assert bool(torch.isfinite(d_rows).all()) and bool(torch.isfinite(dz).all()), f"{what}gradients are not finite"
    rr = _ratio((d_rows.double() - case["d_rows"]).abs(), case["bdv"][:, 1:])
    rz = _ratio((dz.double() - case["dz"]).abs(), case["bdv"][:, 0])
    assert rr <= 1.0, f"{what}|d_rows - d_rows64| is {rr:.3g} x the bound"
    assert rz <= 1.0, f"{what}|dz - dz64| is {rz:.3g} x the bound"
    return rr, rz


# ---------------------------------------------------------------------------------------------------- the model
def bottom_widths(hp):
    return list(hp.get("bottom_hidden_units", (64, 32))) + [hp["embedding_size"]]


def bottom_tower(p, dense, hp):
    """-> (z [B,D], the pre-activation of every layer): the activation follows every layer, the last one included."""
    act = TL.act_fn(hp.get("deep_activation", "relu"))
    a, pres = dense, []
    for l in range(len(bottom_widths(hp))):
        pre = a @ p[f"bot_dnn_layer_{l}_weights"] + p[f"bot_dnn_layer_{l}_bias"]
        pres.append(pre)
        a = act(pre)
    return a, pres


def top_tower(p, X, hp, keep=None, masks=None):
    """DNN.__call__ (layers.py:576-609) under the prefix top_: -> (logit [B,1], the pre-activation of every layer)."""
    n = len(hp["deep_hidden_units"])
    keep = keep or [1] * (n + 1)
    masks = masks or [None] * (n + 1)
    act = TL.act_fn(hp.get("deep_activation", "relu"))
    y, pres = TL.dropout(X, keep[0], masks[0]), []
    for l in range(n):
        pre = y @ p[f"top_dnn_layer_{l}_weights"] + p[f"top_dnn_layer_{l}_bias"]
        pres.append(pre)
        y = TL.dropout(act(pre), keep[l + 1], masks[l + 1])
    return y @ p["top_dnn_w"] + p["top_dnn_w0"], pres


def logit_from_embeddings(p, E, dense, hp, training=True, masks=None, return_pre=False):
    """The towers and the interaction on given embedding rows E [B,F,D]: the top logit [B,1]."""
    z, pres = bottom_tower(p, dense, hp)
    keep = C.dnn_keep(hp, len(hp["deep_hidden_units"]), training)
    out, pres_top = top_tower(p, interact(E, z), hp, keep, (masks or {}).get("dnn"))
    return (out, pres + pres_top) if return_pre else out


def dlrm_logit(p, spec, idx, dense, hp, training=True, masks=None, manual_weights=None, mv=None):
    """logit = top tower (+ linear with use_linear); no bias tables."""
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    logit = logit_from_embeddings(p, E, dense, hp, training, masks)
    if hp.get("use_linear", False):
        logit = logit + TL.linear_layer(p, spec, idx, dense, manual_weights, mv)
    return logit


def deep_l2_names(hp):
    """Every matrix deep_l2_reg covers: the weights of both towers and top_dnn_w."""
    return ([f"bot_dnn_layer_{l}_weights" for l in range(len(bottom_widths(hp)))]
            + [f"top_dnn_layer_{l}_weights" for l in range(len(hp["deep_hidden_units"]))] + ["top_dnn_w"])


def tower_l2(p, hp):
    return C.param_l2(deep_l2_names(hp), p, hp.get("deep_l2_reg", 0.0))


def dlrm_l2(p, spec, hp):
    out = TL.embedding_l2(p, spec, hp.get("embedding_l2_reg", 0.0)) + tower_l2(p, hp)
    if hp.get("use_linear", False):
        out = out + TL.linear_l2(p, hp.get("linear_l2_reg", 0.0))
    return out


# (p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None) -> (loss, logit [B,1], pred)
model_loss = partial(C.model_loss, dlrm_logit, dlrm_l2)
# ... -> (loss, logit [B], pred [B], grads): one forward+backward, the twin of oracle.th_layers.fwd_bwd
fwd_bwd = partial(C.fwd_bwd, model_loss)


def tower_params(rnd, D, F, Dn, bottom, hidden):
    """The variables of both towers: glorot weights, biases ~ 0.1 N(0,1)."""
    p = {}
    C.draw_dnn(rnd, p, [Dn] + list(bottom) + [D], head=False, prefix="bot_")
    C.draw_dnn(rnd, p, [D + pairs(F)] + list(hidden), prefix="top_")
    return p


def make_case(B, F, D, Dn, seed=0, bottom=(16,), hidden=(32, 32), use_linear=False, dtype=torch.float64):
    """A seeded model-level case: spec, p (the variable names of the contract), idx, dense, y, hp; `model_min_abs_pre`
    is the distance of the closest unit of either tower to its kink."""
    spec, sizes = C.plain_spec(F, Dn)
    g = torch.Generator().manual_seed(7000 + seed)
    rnd = C.rnd_stream(g)
    p = C.draw_front(rnd, spec, D, std=0.3)
    p.update(tower_params(rnd, D, F, Dn, bottom, hidden))
    idx, dense, y = C.draw_batch(g, rnd, sizes, B, Dn)
    hp = dict(embedding_size=D, embedding_l2_reg=1e-3, linear_l2_reg=1e-3, bottom_hidden_units=tuple(bottom),
              deep_hidden_units=tuple(hidden), deep_dropout=(1,) * (len(hidden) + 1), deep_l2_reg=1e-3,
              deep_activation="relu", use_linear=use_linear)
    c = lambda t: t.to(dtype) if t.is_floating_point() else t  # noqa: E731
    out = dict(spec=spec, p={k: c(v) for k, v in p.items()}, idx=idx, dense=c(dense), y=y, hp=hp)
    out["model_min_abs_pre"] = min_abs_pre(p, spec, idx, dense, hp)
    return out


def min_abs_pre(p, spec, idx, dense, hp, mv=None, E=None, masks=None):
    """The smallest |pre-activation| of the model on a batch: every unit of every layer of both towers."""
    if E is None:
        E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    pres = logit_from_embeddings(p, E, dense, hp, True, masks, return_pre=True)[1]
    return min(float(t.detach().abs().min()) for t in pres)
