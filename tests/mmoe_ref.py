"""CPU PyTorch restatement (dtype-generic) of multi-task learning with MMoE (Multi-gate Mixture-of-Experts, Ma et al.,
KDD 2018): the gate-softmax + expert mixture, the loss head for several labels, and the model built on them.

TEST INFRASTRUCTURE.  Nothing in the reference implements MMoE (it knows one label per example), so the arithmetic is
the project's contract (include/recman_hip.h, engine.MMoEEngine).  Per example, E experts of width H, T tasks:

    p_t = softmax_e(A_t);   M_t = sum_e p_te Z_e         Z [B, E H] (expert e at columns e H ..), A [B, T E], M [B, T H]
    backward, given dM:     dZ_e = sum_t p_te dM_t;  c_te = <dM_t, Z_e>;  dA_te = p_te (c_te - sum_e' p_te' c_te')
    loss head:              pred_t = sigmoid(logit_t) | logit_t;  l_t = create_loss's term (Keras BCE on clipped
                            probabilities | squared error);  loss = sum_t w_t * mean over the labels of task t that are
                            observed (not NaN) of l_t;  a task without an observed label gives 0
    model:                  x = [E | dense];  experts h^{l+1}_e = act(h^l_e W^l_e + b^l_e), layer 0 stacked [K0, E H_1];
                            gates A = x gate_weights [K0, T E];  logit_t = DNN_t(M_t) with the variables "{task}_dnn_*"

The embedding, DNN and loss pieces are oracle.th_layers' public functions; the sequence front is tests/asp_ref.py's.
tests/test_mmoe_host.py pins this file without a GPU; the GPU tests compare the HIP kernels and the engine against it in
float64, with the float32 run of the same code as the yardstick of the tolerances:
    measure <= max(TOL_GRAD, 4 x the float32 CPU restatement's own measure on the case)      (tests/test_gpu_asp.py)
"""
import math

import torch

from oracle import th_layers as TL
from tests import asp_ref
from tests import ref_common as C
from tests.ref_common import KINK, glorot, grad_measure, to_f32  # noqa: F401  (part of this module's interface)

TOL_GRAD = 2e-5
NAN = float("nan")

# kernel-level GPU cases (B, E, T, H): the default with B no multiple of any tile; every minimum (p = 1, dA exactly 0);
# both maxima with H no power of two; the widest H (two column vectors per lane); whole tiles only
MIX_CASES = [(77, 8, 2, 128), (1, 1, 1, 4), (33, 16, 8, 36), (70, 3, 2, 512), (64, 4, 3, 8)]
# loss-head cases: T x B
LOSS_T, LOSS_B = (1, 2, 8), (1, 77, 4099)


def bound(f32_measure):
    return max(TOL_GRAD, 4.0 * f32_measure)


# ------------------------------------------------------------------------------------------------- the mixture
def gate_softmax(A, E, T):
    """A [B, T E] -> p [B, T, E], max-subtracted."""
    return torch.softmax(A.reshape(A.shape[0], T, E), dim=2)


def mix_fwd(Z, A, E, T):
    """-> (M [B, T H], p [B, T, E])."""
    B = Z.shape[0]
    p = gate_softmax(A, E, T)
    M = torch.einsum("bte,beh->bth", p, Z.reshape(B, E, -1))
    return M.reshape(B, -1), p


def mix_bwd(Z, A, E, T, dM):
    """The closed-form backward of the contract (no autograd): -> (dZ [B, E H], dA [B, T E])."""
    B = Z.shape[0]
    Zr, dMr = Z.reshape(B, E, -1), dM.reshape(B, T, -1)
    p = gate_softmax(A, E, T)
    dZ = torch.einsum("bte,bth->beh", p, dMr)
    c = torch.einsum("bth,beh->bte", dMr, Zr)
    dA = p * (c - (p * c).sum(dim=2, keepdim=True))
    return dZ.reshape(B, -1), dA.reshape(B, -1)


def mix_loops(Z, A, E, T):
    """mix_fwd as explicit Python loops over floats (no tensor arithmetic)."""
    out = []
    for z, a in zip(Z.tolist(), A.tolist()):
        H = len(z) // E
        row = []
        for t in range(T):
            mx = max(a[t * E: (t + 1) * E])
            w = [math.exp(v - mx) for v in a[t * E: (t + 1) * E]]
            s = sum(w)
            row += [sum(w[e] / s * z[e * H + h] for e in range(E)) for h in range(H)]
        out.append(row)
    return torch.tensor(out, dtype=Z.dtype)


@C.memo
def mix_case(B, E, T, H, seed=0, logit_scale=1.0):
    """A seeded kernel-level case in float64 (made once per key, never changed): Z, dM ~ N(0,1), A ~ logit_scale
    N(0,1); with the float64 outputs M, P, dZ, dA and the float32 CPU restatement's own measures `f32` (M, dZ, dA)."""
    rnd = C.rnd_stream(torch.Generator().manual_seed(31000 + 97 * seed + B + 7 * E + 13 * T + H))
    Z, A, dM = rnd(B, E * H), (rnd(B, T * E) * logit_scale).float().double(), rnd(B, T * H)
    M, P = mix_fwd(Z, A, E, T)
    dZ, dA = mix_bwd(Z, A, E, T, dM)
    M32, _ = mix_fwd(Z.float(), A.float(), E, T)
    dZ32, dA32 = mix_bwd(Z.float(), A.float(), E, T, dM.float())
    f32 = dict(M=grad_measure(M32, M), dZ=grad_measure(dZ32, dZ), dA=grad_measure(dA32, dA))
    return dict(B=B, E=E, T=T, H=H, Z=Z, A=A, dM=dM, M=M, P=P, dZ=dZ, dA=dA, f32=f32)


# ----------------------------------------------------------------------------------------------- the loss head
def loss_terms(logit_t, y_t, kind):
    """Per example: (pred, l) of one task - PredictionLayer and create_loss's term before the mean."""
    pred = TL.prediction(logit_t, kind)
    y_t = y_t.to(pred.dtype)
    if kind == "classification":
        pc = pred.clamp(TL.KERAS_EPS, 1 - TL.KERAS_EPS)
        return pred, -(y_t * torch.log(pc + TL.KERAS_EPS) + (1 - y_t) * torch.log(1 - pc + TL.KERAS_EPS))
    return pred, (pred - y_t).square()


def loss_head(logit, Y, types, weights=None):
    """logit [T, B], Y [B, T] (NaN = unobserved) -> (loss, loss_t [T], n_t [T], pred [T, B])."""
    T = logit.shape[0]
    weights = [1.0] * T if weights is None else weights
    total, loss_t, n_t, preds = logit.new_zeros(()), [], [], []
    for t in range(T):
        seen = ~torch.isnan(Y[:, t])
        y = torch.where(seen, Y[:, t], torch.zeros_like(Y[:, t]))
        pred, l = loss_terms(logit[t], y, types[t])
        n = int(seen.sum())
        lt = (l * seen.to(l.dtype)).sum() / n if n else logit.new_zeros(())
        total = total + weights[t] * lt
        loss_t.append(lt)
        n_t.append(n)
        preds.append(pred)
    return total, torch.stack(loss_t), torch.tensor(n_t), torch.stack(preds)


def loss_head_grad(logit, Y, types, weights=None, grad_scale=1.0):
    """(loss, loss_t, n_t, pred, dlogit [T, B] = grad_scale dloss/dlogit) by autograd."""
    leaf = logit.detach().clone().requires_grad_(True)
    loss, loss_t, n_t, pred = loss_head(leaf, Y, types, weights)
    if leaf.grad is None and loss.requires_grad:
        loss.backward()
    g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
    return loss.detach(), loss_t.detach(), n_t, pred.detach(), g * grad_scale


@C.memo
def loss_case(T, B, seed=0):
    """A seeded loss-head case in float64 (made once, never changed): logits ~ 2 N(0,1); tasks alternate classification
    and regression (task 0 classification); weights 0.5 + 0.25 t; with T > 1, about 70 % of task 1's labels are NaN and
    the LAST task (T > 2) has no observed label at all; grad_scale 0.5.  With the float64 outputs and the float32 CPU
    restatement's own measures `f32` (pred, dlogit, loss_t)."""
    g = torch.Generator().manual_seed(32000 + 101 * seed + 17 * T + B)
    rnd = C.rnd_stream(g)
    types = ["classification" if t % 2 == 0 else "regression" for t in range(T)]
    weights = [0.5 + 0.25 * t for t in range(T)]
    logit = rnd(T, B, std=2.0)
    Y = torch.empty(B, T, dtype=torch.float64)
    for t, kind in enumerate(types):
        Y[:, t] = (torch.rand(B, generator=g) < 0.3).double() if kind == "classification" else rnd(B)
    if T > 1:
        Y[torch.rand(B, generator=g) < 0.7, 1] = NAN
    if T > 2:
        Y[:, T - 1] = NAN
    want = loss_head_grad(logit, Y, types, weights, 0.5)
    got32 = loss_head_grad(logit.float(), Y.float(), types, weights, 0.5)
    f32 = dict(pred=grad_measure(got32[3], want[3]), dlogit=grad_measure(got32[4], want[4]),
               loss_t=grad_measure(got32[1], want[1]))
    return dict(T=T, B=B, types=types, weights=weights, grad_scale=0.5, logit=logit, Y=Y, loss=want[0],
                loss_t=want[1], n_t=want[2], pred=want[3], dlogit=want[4], f32=f32)


# ---------------------------------------------------------------------------------------------------- the model
def tower_vars(p, task):
    pre = f"{task}_"
    return {n[len(pre):]: v for n, v in p.items() if n.startswith(pre + "dnn_")}


def embeddings(p, spec, idx, hp, mv=None):
    if hasattr(spec, "seq_query"):
        return asp_ref.embeddings(p, spec, idx, mv, hp)
    return TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)[0]


def mmoe_logits(p, spec, idx, dense, hp, mv=None, pres=None, E_in=None):
    """-> (logit [T, B], gate weights [B, T, E]).  pres: a list that receives every expert and tower pre-activation.
    E_in: the embeddings [B, F, D] to use instead of the lookup (to take their gradient)."""
    names = hp["task_names"]
    NE, T, units = hp["num_experts"], len(names), list(hp["expert_hidden_units"])
    act = TL.act_fn(hp.get("deep_activation", "relu"))
    x = TL.dnn_input(embeddings(p, spec, idx, hp, mv) if E_in is None else E_in, dense)
    B = x.shape[0]
    pre = x @ p["expert_layer_0_weights"] + p["expert_layer_0_bias"]
    if pres is not None:
        pres.append(pre)
    h = act(pre)
    for l in range(1, len(units)):
        W, b = p[f"expert_layer_{l}_weights"], p[f"expert_layer_{l}_bias"]
        pre = torch.einsum("bek,ekn->ben", h.reshape(B, NE, units[l - 1]), W) + b
        if pres is not None:
            pres.append(pre)
        h = act(pre).reshape(B, NE * units[l])
    M, P = mix_fwd(h, x @ p["gate_weights"], NE, T)
    H, n = units[-1], len(hp["tower_hidden_units"])
    logits = []
    for t, name in enumerate(names):
        tv = tower_vars(p, name)
        y = M[:, t * H: (t + 1) * H]
        if pres is not None:
            for i in range(n):
                pres.append(y @ tv[f"dnn_layer_{i}_weights"] + tv[f"dnn_layer_{i}_bias"])
                y = act(pres[-1])
        logits.append(TL.dnn(tv, M[:, t * H: (t + 1) * H], n, hp.get("deep_activation", "relu")).reshape(-1))
    return torch.stack(logits), P


def mmoe_l2(p, spec, hp):
    tl = spec.tl if hasattr(spec, "tl") else spec
    out = TL.embedding_l2(p, tl, hp.get("embedding_l2_reg", 0.0))
    reg = hp.get("deep_l2_reg", 0.0)
    ws = [v for n, v in p.items() if n == "gate_weights" or (n.startswith("expert_layer_") and n.endswith("_weights"))]
    for name in hp["task_names"]:
        tv = tower_vars(p, name)
        ws += [v for n, v in tv.items() if n.endswith("_weights") or n == "dnn_w"]
    return out + sum(reg * 0.5 * w.square().sum() for w in ws)


def model_loss(p, spec, idx, dense, Y, hp, mv=None, E_in=None):
    logit, _ = mmoe_logits(p, spec, idx, dense, hp, mv, E_in=E_in)
    loss, loss_t, n_t, pred = loss_head(logit, Y.to(logit.dtype), hp["task_types"], hp.get("task_weights"))
    return loss + mmoe_l2(p, spec, hp), logit, pred


def fwd_bwd(p, spec, idx, dense, Y, hp, mv=None):
    """One forward+backward: (loss, logit [T, B], pred [T, B], grads) - the twin of oracle.th_layers.fwd_bwd."""
    out, grads = C.backward(model_loss, p, spec, idx, dense, Y, hp, mv)
    return out + (grads,)


def d_rows(p, spec, idx, dense, Y, hp, mv=None):
    """dLoss/dE [B, F, D] of the data loss (no l2): what the engine's d_rows holds - for a sequence field the pooled
    row's gradient, for its query field the model's own gradient only (the unit adds its query gradient later)."""
    E = embeddings(p, spec, idx, hp, mv).detach().clone().requires_grad_(True)
    logit, _ = mmoe_logits(p, spec, idx, dense, hp, mv, E_in=E)
    loss_head(logit, Y.to(logit.dtype), hp["task_types"], hp.get("task_weights"))[0].backward()
    return E.grad


# model-level cases: (task_types, num_experts, expert_hidden_units, tower_hidden_units, B, F, D, Dn, nan_share, attempt)
# `attempt` is the first stream of make_case whose every expert and tower ReLU pre-activation is at least KINK from 0 in
# float64 (tests/test_mmoe_host.py asserts it); towers of (8,) run the fused skinny-MLP kernels, (40,) and (64, 16)
# the layer-by-layer path
C2 = ("classification", "classification")
MODEL_CASES = {
    "two_tasks": (C2, 4, (32, 16), (8,), 70, 5, 8, 3, 0.0, 0),
    "two_tasks_no_dense": (C2, 3, (16,), (40,), 67, 3, 16, 0, 0.0, 0),
    "three_tasks_nan": (("classification", "regression", "classification"), 4, (24, 16), (64, 16), 71, 7, 8, 2, 0.6, 0),
    "shared_bottom": (C2, 1, (32, 16), (8,), 70, 4, 8, 1, 0.3, 0),
    "three_layer_experts": (C2, 2, (32, 16, 8), (40,), 69, 5, 16, 2, 0.0, 1),
    "one_task": (("classification",), 3, (16,), (8,), 66, 4, 8, 2, 0.0, 0),
}
SEQ_CASE = (C2, 3, (16, 8), (40,), 0)  # over tests/asp_ref.py's front (B = 37, D = 8, two dense features): + attempt


def task_names(T):
    return ("ctr", "cvr", "like", "dwell", "t4", "t5", "t6", "t7")[:T]


def _model_vars(rnd, p, K0, names, NE, units, towers):
    p["expert_layer_0_weights"] = glorot(rnd, (K0, NE * units[0]), K0, units[0])
    p["expert_layer_0_bias"] = rnd(NE * units[0], std=0.1)
    for l in range(1, len(units)):
        p[f"expert_layer_{l}_weights"] = glorot(rnd, (NE, units[l - 1], units[l]), units[l - 1], units[l])
        p[f"expert_layer_{l}_bias"] = rnd(NE, units[l], std=0.1)
    p["gate_weights"] = rnd(K0, len(names) * NE, std=0.3)  # (wide enough that the gates are not all near 1 / E)
    for name in names:
        C.draw_dnn(rnd, p, [units[-1]] + list(towers), prefix=f"{name}_")


def _labels(g, rnd, B, types, nan_share):
    Y = torch.empty(B, len(types), dtype=torch.float64)
    for t, kind in enumerate(types):
        Y[:, t] = (torch.rand(B, generator=g) < 0.3).double() if kind == "classification" else rnd(B)
        if nan_share and t > 0:
            Y[torch.rand(B, generator=g) < nan_share, t] = NAN
    return Y


def _hp(types, NE, units, towers, D, l2):
    names = task_names(len(types))
    return dict(embedding_size=D, embedding_l2_reg=l2, deep_l2_reg=l2, task_names=names, task_types=tuple(types),
                task_weights=tuple(1.0 - 0.25 * t for t in range(len(types))), num_experts=NE,
                expert_hidden_units=tuple(units), tower_hidden_units=tuple(towers), deep_activation="relu")


def min_abs_pre(p, spec, idx, dense, hp, mv=None):
    pres = []
    with torch.no_grad():
        mmoe_logits(p, spec, idx, dense, hp, mv, pres=pres)
    return C.min_abs(pres)


@C.memo
def make_case(types, NE, units, towers, B, F, D, Dn, nan_share, attempt, l2=1e-4):
    """A seeded model-level case in float64 (made once, never changed): spec, p (the contract's variable names, with
    the unused linear_w / linear_w0 of every state_dict), idx, dense, Y [B, T], hp.  Embeddings ~ N(0, 0.3^2), dense ~
    N(0,1); `min_abs_pre` is the distance of the closest expert or tower unit to its kink."""
    spec, sizes = C.plain_spec(F, Dn)
    hp = _hp(types, NE, units, towers, D, l2)
    g = torch.Generator().manual_seed(33000 + attempt)
    rnd = C.rnd_stream(g)
    # (its own draw of the front: the linear term is unused, so linear_w and linear_w0 are zeros and draw nothing)
    p = {f"{name}_feat_embed": rnd(V, D, std=0.3) for name, V in zip(spec.sparse_names, sizes)}
    p["linear_w"] = torch.zeros(spec.lin_layout[2], 1, dtype=torch.float64)
    p["linear_w0"] = torch.zeros(1, dtype=torch.float64)
    _model_vars(rnd, p, F * D + Dn, hp["task_names"], NE, units, towers)
    idx, dense = C.draw_idx(g, sizes, B), rnd(B, Dn)
    Y = _labels(g, rnd, B, types, nan_share)
    return dict(spec=spec, p=p, idx=idx, dense=dense, Y=Y, hp=hp, mv=None,
                min_abs_pre=min_abs_pre(p, spec, idx, dense, hp))


@C.memo
def make_seq_case(types=SEQ_CASE[0], NE=SEQ_CASE[1], units=SEQ_CASE[2], towers=SEQ_CASE[3], attempt=SEQ_CASE[4],
                  l2=1e-3):
    """MMoE over the front of tests/asp_ref.py:make_model_case - C0 (7), item (11), hist -> item (max_len 6, din
    pooling), C2 (5); B = 37, D = 8, two dense features: the embedding tables, the unit's variables, ids, histories and
    dense values are that case's, the MMoE variables and labels are drawn here."""
    u = asp_ref.make_model_case("din", B=37, D=8, Dn=2, seed=attempt, max_len=6)
    spec = u["spec"]
    p = {n: v for n, v in u["p"].items() if not n.startswith("dnn_")}
    hp = _hp(types, NE, units, towers, 8, l2)
    hp.update({n: u["hp"][n] for n in ("att_hidden_units", "att_activation", "att_weight_normalization")},
              seq_pooling="din")
    g = torch.Generator().manual_seed(34000 + attempt)
    rnd = C.rnd_stream(g)
    _model_vars(rnd, p, spec.F * 8 + 2, hp["task_names"], NE, units, towers)
    Y = _labels(g, rnd, 37, types, 0.3)
    return dict(model="mmoe", spec=spec, p=p, idx=u["idx"], dense=u["dense"], Y=Y, hp=hp, mv=u["mv"],
                min_abs_pre=min_abs_pre(p, spec, u["idx"], u["dense"], hp, u["mv"]))
