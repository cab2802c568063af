"""CPU PyTorch restatement (dtype-generic, autograd) of AutoInt's interacting layer, its last projection and the model.

TEST INFRASTRUCTURE.  Nothing in the reference implements the layer, so the arithmetic is the paper's (arXiv 1810.11921
eq. (5)-(8)) as the project's contract states it.  One layer maps X [B,F,Din] to Y [B,F,HD], HD = H dk:

    Q = X Wq, K = X Wk, V = X Wv;  s^h_mk = <Q^h_m, K^h_k> c;  a^h_m. = softmax_k(s^h_m.)  (max-subtracted, k = m included)
    O_m = concat_h sum_k a^h_mk V^h_k;  Y_m = relu(O_m + X_m Wr)   (Wr None: relu(O_m))
    autoint_logit = flatten(Y_L) . autoint_w + autoint_w0

The model is composed from the public functions of oracle.th_layers, imported and not modified.
tests/test_autoint_host.py pins this file without a GPU; the GPU tests compare the HIP kernels against it in float64.
"""
from functools import partial

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK, grad_measure  # noqa: F401  (part of this module's interface)
from tests.ref_common import rnd_stream as _rnd  # noqa: F401  (tests/test_gpu_autoint_model.py draws with it)

# kernel-level GPU cases (B, F, Din, H, dk) of tests/test_gpu_autoint.py; tests/test_autoint_host.py asserts the kink
# guard's cap on every one of them (the two softmax-range cases again with Wq x 400)
GPU_CASES = [(37, 5, 8, 2, 4), (64, 26, 16, 2, 8), (130, 26, 16, 2, 16), (9, 39, 64, 4, 16), (300, 40, 32, 1, 16),
             (70, 26, 32, 8, 8), (33, 2, 8, 1, 8), (1, 6, 8, 2, 4), (2, 6, 8, 2, 4), (3, 6, 8, 2, 4),
             (4100, 26, 16, 2, 8), (150, 1, 16, 2, 8)]
RANGE_CASES = [(64, 26, 16, 2, 8), (130, 26, 16, 2, 16)]
RANGE_Q_SCALE = 400.0
# (KINK: here the pre-activation is O + X Wr)
KINK_CAP = 0.20    # largest share of examples the guard may zero

# model-level GPU cases of tests/test_gpu_autoint_model.py: keyword arguments of make_case.  Their upstream gradient
# comes from the labels and cannot be zeroed, so the seeds are such that no unit of any layer lies within KINK of 0
# (asserted on the CPU in tests/test_autoint_host.py)
MODEL_CASES = {
    "d8": dict(B=37, F=5, D=8, Dn=2, L=2, H=2, dk=4, seed=0),
    "d16": dict(B=37, F=5, D=16, Dn=2, L=2, H=2, dk=8, seed=0),
    "d32": dict(B=37, F=5, D=32, Dn=2, L=1, H=4, dk=4, seed=0),
    "d64": dict(B=21, F=7, D=64, Dn=2, L=2, H=2, dk=16, seed=0),
    "one_layer": dict(B=37, F=6, D=16, Dn=1, L=1, H=2, dk=8, seed=0),
    "three_layers": dict(B=45, F=9, D=8, Dn=1, L=3, H=2, dk=8, seed=0),
    "no_res": dict(B=37, F=5, D=16, Dn=2, L=2, H=2, dk=8, seed=0, att_res=False),
    "scaling": dict(B=37, F=5, D=16, Dn=2, L=2, H=2, dk=8, seed=0, att_scaling=True),
    "no_dense": dict(B=37, F=5, D=8, Dn=0, L=2, H=1, dk=8, seed=0),
    "plus": dict(B=41, F=6, D=16, Dn=3, L=2, H=2, dk=8, seed=0, hidden=(32, 32)),
    "criteo_like": dict(B=150, F=26, D=16, Dn=13, L=3, H=2, dk=8, seed=1),
}


def att_scale(dk, scaling):
    return float(dk) ** -0.5 if scaling else 1.0


def interacting_parts(X, Wq, Wk, Wv, Wr, H, scale=1.0):
    """(a [B,H,F,F], V heads [B,H,F,dk], pre-activation O + X Wr [B,F,HD], scores [B,H,F,F])."""
    B, F, _ = X.shape
    HD = Wq.shape[1]
    dk = HD // H
    heads = lambda t: t.reshape(B, F, H, dk).permute(0, 2, 1, 3)  # noqa: E731
    Q, K, V = heads(X @ Wq), heads(X @ Wk), heads(X @ Wv)
    s = (Q @ K.transpose(2, 3)) * scale
    a = torch.softmax(s, dim=3)  # max-subtracted
    O = (a @ V).permute(0, 2, 1, 3).reshape(B, F, HD)
    pre = O if Wr is None else O + X @ Wr
    return a, V, pre, s


def interacting_layer(X, Wq, Wk, Wv, Wr, H, scale=1.0):
    """X [B,F,Din], Wq / Wk / Wv [Din,HD], Wr [Din,HD] or None -> Y [B,F,HD]."""
    return torch.relu(interacting_parts(X, Wq, Wk, Wv, Wr, H, scale)[2])


def head(Y, w, w0):
    """flatten(Y) . w + w0 -> [B]."""
    return Y.reshape(Y.shape[0], -1) @ w.reshape(-1) + w0.reshape(())


def interacting_layer_bwd(X, Wq, Wk, Wv, Wr, H, scale, dY, dX_up=None):
    """The backward of the contract, written out (no autograd): -> (dX, dWq, dWk, dWv, dWr or None)."""
    B, F, Din = X.shape
    HD = Wq.shape[1]
    dk = HD // H
    heads = lambda t: t.reshape(B, F, H, dk).permute(0, 2, 1, 3)  # noqa: E731
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B, F, HD)  # noqa: E731
    a, V, pre, _ = interacting_parts(X, Wq, Wk, Wv, Wr, H, scale)
    Q, K = heads(X @ Wq), heads(X @ Wk)
    dP = dY * (pre > 0).to(X.dtype)
    dO = heads(dP)
    da = dO @ V.transpose(2, 3)
    ds = a * (da - (a * da).sum(dim=3, keepdim=True))
    dQ, dK, dV = flat(ds @ K) * scale, flat(ds.transpose(2, 3) @ Q) * scale, flat(a.transpose(2, 3) @ dO)
    x2 = X.reshape(B * F, Din)
    dX = dQ @ Wq.t() + dK @ Wk.t() + dV @ Wv.t()
    if Wr is not None:
        dX = dX + dP @ Wr.t()
    if dX_up is not None:
        dX = dX + dX_up
    mm = lambda d: x2.t() @ d.reshape(B * F, HD)  # noqa: E731
    return dX, mm(dQ), mm(dK), mm(dV), (mm(dP) if Wr is not None else None)


# ---------------------------------------------------------------------------------------------------- the model
def layer_names(l, att_res=True):
    return [f"autoint_layer_{l}_{k}_w" for k in ("query", "key", "value") + (("res",) if att_res else ())]


def att_names(hp):
    """Every matrix att_l2_reg covers."""
    out = []
    for l in range(hp["att_layer_num"]):
        out += layer_names(l, hp.get("att_res", True))
    return out + ["autoint_w"]


def autoint_stack(p, E, hp, return_pre=False):
    """The L interacting layers and the last projection on E: autoint_logit [B] (and every layer's pre-activation)."""
    x, pres = E, []
    for l in range(hp["att_layer_num"]):
        W = [p[n] for n in layer_names(l, hp.get("att_res", True))] + ([] if hp.get("att_res", True) else [None])
        pre = interacting_parts(x, *W, hp["att_head_num"], att_scale(hp["att_embedding_size"], hp.get("att_scaling")))[2]
        pres.append(pre)
        x = torch.relu(pre)
    out = head(x, p["autoint_w"], p["autoint_w0"])
    return (out, pres) if return_pre else out


def autoint_logit(p, spec, idx, dense, hp, training=True, masks=None, manual_weights=None, mv=None):
    """logit = linear + autoint (+ dnn([E | dense]) with a non-empty deep_hidden_units); no bias tables."""
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    logit = TL.linear_layer(p, spec, idx, dense, manual_weights, mv)
    logit = logit + autoint_stack(p, E, hp).reshape(-1, 1)
    n = len(hp.get("deep_hidden_units") or ())
    if n:
        logit = logit + TL.dnn(p, TL.dnn_input(E, dense), n, hp.get("deep_activation", "relu"),
                               C.dnn_keep(hp, n, training), (masks or {}).get("dnn"))
    return logit


def autoint_l2(p, spec, hp):
    out = C.base_l2(p, spec, hp, None, True)  # (the DNN's term comes behind the attention's here)
    out = out + C.param_l2(att_names(hp), p, hp.get("att_l2_reg", 0.0))
    n = len(hp.get("deep_hidden_units") or ())
    if n:
        out = out + TL.dnn_l2(p, n, hp.get("deep_l2_reg", 0.0))
    return out


# (p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None) -> (loss, logit [B,1], pred)
model_loss = partial(C.model_loss, autoint_logit, autoint_l2)
# ... -> (loss, logit [B], pred [B], grads): one forward+backward, the twin of oracle.th_layers.fwd_bwd
fwd_bwd = partial(C.fwd_bwd, model_loss)


# -------------------------------------------------------------------------------------------------------- cases
def glorot(rnd, fan_in, fan_out):
    """A [fan_in, fan_out] matrix."""
    return C.glorot(rnd, (fan_in, fan_out), fan_in, fan_out)


def make_layer_case(B, F, Din, H, dk, seed=0, q_scale=1.0):
    """A seeded layer-level case: X ~ 0.3 N(0,1), glorot Wq (times q_scale) / Wk / Wv / Wr, dY ~ N(0,1), dX_up ~ 0.1
    N(0,1), head w glorot [F HD] and w0, g ~ N(0,1).  dY is ZERO for every example that has a pre-activation
    O + X Wr (with the residual) or O (without) within KINK of 0 in float64, at either scale of the scores: `near`
    marks them, `zeroed` is their share."""
    g = torch.Generator().manual_seed(2000 + seed)
    rnd = C.rnd_stream(g)
    HD = H * dk
    X = rnd(B, F, Din, std=0.3)
    Wq = (glorot(rnd, Din, HD) * q_scale).float().double()
    Wk, Wv, Wr = glorot(rnd, Din, HD), glorot(rnd, Din, HD), glorot(rnd, Din, HD)
    dY, dX_up = rnd(B, F, HD), rnd(B, F, Din, std=0.1)
    w, w0, gl = glorot(rnd, F * HD, 1).reshape(-1), rnd(1, std=0.1), rnd(B)
    near = torch.zeros(B, dtype=torch.bool)
    for res in (Wr, None):
        for scaling in (False, True):
            pre = interacting_parts(X, Wq, Wk, Wv, res, H, att_scale(dk, scaling))[2]
            near |= (pre.abs() < KINK).flatten(1).any(dim=1)
    dY = torch.where(near.view(B, 1, 1), torch.zeros_like(dY), dY)
    return dict(X=X, Wq=Wq, Wk=Wk, Wv=Wv, Wr=Wr, dY=dY, dX_up=dX_up, w=w, w0=w0, g=gl, H=H, dk=dk, near=near,
                zeroed=float(near.double().mean()))


@C.memo
def gpu_case(c, q_scale=1.0):
    """make_layer_case for a kernel-level (B, F, Din, H, dk) of GPU_CASES / RANGE_CASES (made once, never changed)."""
    return make_layer_case(*c, seed=0, q_scale=q_scale)


def layer_reference(case, use_res, use_up, scaling, dtype=torch.float64):
    """interacting_layer + autograd on a case's tensors in `dtype`: (Y, dX, dWq, dWk, dWv[, dWr]) as float64."""
    names = ("X", "Wq", "Wk", "Wv") + (("Wr",) if use_res else ())
    leaves = [case[k].to(dtype).clone().requires_grad_(True) for k in names]
    Y = interacting_layer(*leaves, *(() if use_res else (None,)), case["H"], att_scale(case["dk"], scaling))
    (Y * case["dY"].to(dtype)).sum().backward()
    grads = [t.grad for t in leaves]
    if use_up:
        grads[0] = grads[0] + case["dX_up"].to(dtype)
    return tuple(t.detach().double() for t in [Y] + grads)


def head_reference(case, Y, dtype=torch.float64):
    """head + autograd on Y [B,F,HD]: (logit, dY, dw, dw0) as float64."""
    Yl, w, w0 = (t.to(dtype).clone().requires_grad_(True) for t in (Y, case["w"], case["w0"]))
    out = head(Yl, w, w0)
    (out * case["g"].to(dtype)).sum().backward()
    return tuple(t.detach().double() for t in (out, Yl.grad, w.grad, w0.grad))


def make_case(B, F, D, Dn, L, H, dk, seed=0, att_res=True, att_scaling=False, hidden=(), dtype=torch.float64):
    """A seeded model-level case: spec, p (the variable names of the contract), idx, dense, y, hp; `model_min_abs_pre`
    is the distance of the closest unit of any layer (and, with a DNN, of any hidden unit) to its kink."""
    spec, sizes = C.plain_spec(F, Dn)
    g = torch.Generator().manual_seed(3000 + seed)
    rnd = C.rnd_stream(g)
    HD = H * dk
    p = C.draw_front(rnd, spec, D, std=0.3)
    for l in range(L):
        for n in layer_names(l, att_res):
            p[n] = glorot(rnd, D if l == 0 else HD, HD)
    p["autoint_w"] = glorot(rnd, F * HD, 1)
    p["autoint_w0"] = rnd(1, std=0.1)
    C.draw_dnn(rnd, p, [F * D + Dn] + list(hidden), head=bool(hidden))
    idx, dense, y = C.draw_batch(g, rnd, sizes, B, Dn)
    hp = dict(embedding_size=D, embedding_l2_reg=1e-3, linear_l2_reg=1e-3, att_layer_num=L, att_embedding_size=dk,
              att_head_num=H, att_res=att_res, att_scaling=att_scaling, att_l2_reg=1e-3,
              deep_hidden_units=tuple(hidden), deep_dropout=(1,) * (len(hidden) + 1), deep_l2_reg=1e-3 if hidden else 0.0,
              deep_activation="relu")
    c = lambda t: t.to(dtype) if t.is_floating_point() else t  # noqa: E731
    out = dict(spec=spec, p={k: c(v) for k, v in p.items()}, idx=idx, dense=c(dense), y=y, hp=hp)
    out["model_min_abs_pre"] = min_abs_pre(p, spec, idx, dense, hp)
    return out


def min_abs_pre(p, spec, idx, dense, hp, mv=None):
    """The smallest |pre-activation| of the model on a batch: every unit of every interacting layer and DNN layer."""
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    pres = autoint_stack(p, E, hp, return_pre=True)[1]
    return C.min_abs(pres + C.dnn_pres(p, TL.dnn_input(E, dense), len(hp.get("deep_hidden_units") or ())))
