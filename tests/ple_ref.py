"""CPU PyTorch restatement (dtype-generic) of multi-task learning beyond MMoE: the grouped gate mixture of one extraction
level of PLE / CGC (Progressive Layered Extraction, Tang et al., RecSys 2020), ESMM's entire-space loss head (Ma et al.,
SIGIR 2018), and the model built on them.

TEST INFRASTRUCTURE, on tests/ref_common.py and tests/mmoe_ref.py.  Nothing in the reference implements any of it, so
the arithmetic is the project's contract (include/recman_hip_multitask.h, engine.PLEEngine).  Per example, T tasks, S
experts per task, C shared experts, N = T S + C experts of width H, W = S + C:

    gate g < T sees the experts g S .. g S + S - 1 and T S .. N - 1; the shared gate g = T (shared_gate = 1) sees all N
    p_g = softmax(A_g);   M_g = sum_{e in g} p_ge Z_e        Z [B, N H], A [B, T W + shared_gate N], M [B, G H]
    backward, given dM:   dZ_e = sum_{g with e} p_ge dM_g;  c_ge = <dM_g, Z_e>;  dA_g = p_g o (c_g - <p_g, c_g>)
    entire space (c, v):  z = 0 where y_c == 0, y_v where y_c == 1, unobserved otherwise;  q = p_c p_v;
                          l_v = Keras BCE(z, q) over the observed z; every other task as in mmoe_ref.loss_head
    model:                X_s^0 = x; per level the experts of group s and gate s read X_s; X_g^{l+1} = M_g; towers on X_t^L

tests/test_ple_host.py pins this file without a GPU; the GPU tests compare the HIP kernels and the engine against it in
float64, with the float32 run of the same code as the yardstick of the tolerances (mmoe_ref.bound):
    measure <= max(2e-5, 4 x the float32 CPU restatement's own measure on the case)
"""
import math

import torch

from oracle import th_layers as TL
from tests import asp_ref
from tests import mmoe_ref as R
from tests import ref_common as C
from tests.mmoe_ref import bound, embeddings, loss_terms, tower_vars  # noqa: F401  (part of this module's interface)
from tests.ref_common import KINK, grad_measure, to_f32  # noqa: F401

NAN = float("nan")

# kernel-level GPU cases (B, T, S, C, H, shared_gate): the default with B no multiple of a tile; every minimum; N = 32
# with every maximum and H no power of two; the widest H; whole tiles in the last-level form
MIX_CASES = [(77, 2, 2, 2, 128, 1), (1, 1, 1, 1, 4, 0), (33, 8, 3, 8, 36, 1), (70, 3, 1, 1, 512, 1),
             (64, 2, 4, 1, 8, 0)]
# entire-space loss cases: T x B with the pair (0, 1), and once (2, 0)
LOSS_T, LOSS_B = (2, 3, 8), (1, 77, 4099)
LOSS_CASES = [(T, B, (0, 1)) for T in LOSS_T for B in LOSS_B] + [(3, 77, (2, 0))]
SAT_GRID = (-20.0, -12.0, -7.0, -2.0, 0.0, 2.0, 7.0, 12.0, 20.0)


# ------------------------------------------------------------------------------------------------- the mixture
def widths(T, S, C, sg):
    """(N, gate-logit columns, gates) of a level."""
    N = T * S + C
    return N, T * (S + C) + (N if sg else 0), T + (1 if sg else 0)


def gates(T, S, C, sg):
    """Per gate: (first column of A, one past its last, the experts it sees in the order of its logits)."""
    N, W = T * S + C, S + C
    out = [(g * W, (g + 1) * W, list(range(g * S, (g + 1) * S)) + list(range(T * S, N))) for g in range(T)]
    return out + ([(T * W, T * W + N, list(range(N)))] if sg else [])


def cgc_fwd(Z, A, T, S, C, sg):
    """-> (M [B, G H], P [B, T W + sg N] in A's layout)."""
    B, N = Z.shape[0], T * S + C
    Zr = Z.reshape(B, N, -1)
    Ms, Ps = [], []
    for a0, a1, ex in gates(T, S, C, sg):
        p = torch.softmax(A[:, a0:a1], dim=1)
        Ms.append(torch.einsum("be,beh->bh", p, Zr[:, ex]))
        Ps.append(p)
    return torch.cat(Ms, dim=1), torch.cat(Ps, dim=1)


def cgc_bwd(Z, A, T, S, C, sg, dM):
    """The closed-form backward of the contract (no autograd): -> (dZ [B, N H], dA in A's layout)."""
    B, N = Z.shape[0], T * S + C
    Zr = Z.reshape(B, N, -1)
    H = Zr.shape[2]
    dZ, dAs = torch.zeros_like(Zr), []
    for g, (a0, a1, ex) in enumerate(gates(T, S, C, sg)):
        p = torch.softmax(A[:, a0:a1], dim=1)
        dMg = dM[:, g * H: (g + 1) * H]
        dZ[:, ex] = dZ[:, ex] + p.unsqueeze(2) * dMg.unsqueeze(1)
        c = torch.einsum("bh,beh->be", dMg, Zr[:, ex])
        dAs.append(p * (c - (p * c).sum(dim=1, keepdim=True)))
    return dZ.reshape(B, -1), torch.cat(dAs, dim=1)


def cgc_loops(Z, A, T, S, C, sg):
    """cgc_fwd's M as explicit Python loops over floats (no tensor arithmetic)."""
    N, W = T * S + C, S + C
    out = []
    for z, a in zip(Z.tolist(), A.tolist()):
        H = len(z) // N
        row = []
        for g in range(T + (1 if sg else 0)):
            if g < T:
                logits = a[g * W: (g + 1) * W]
                experts = [g * S + j for j in range(S)] + [T * S + j for j in range(C)]
            else:
                logits, experts = a[T * W: T * W + N], list(range(N))
            mx = max(logits)
            w = [math.exp(v - mx) for v in logits]
            s = sum(w)
            row += [sum(w[i] / s * z[e * H + h] for i, e in enumerate(experts)) for h in range(H)]
        out.append(row)
    return torch.tensor(out, dtype=Z.dtype)


@C.memo
def mix_case(B, T, S, C_, H, sg, seed=0, logit_scale=1.0):
    """A seeded kernel-level case in float64 (made once per key, never changed): Z, dM ~ N(0,1), A ~ logit_scale
    N(0,1); with the float64 outputs M, P, dZ, dA and the float32 CPU restatement's own measures `f32` (M, dZ, dA)."""
    N, AW, G = widths(T, S, C_, sg)
    rnd = C.rnd_stream(torch.Generator().manual_seed(36000 + 97 * seed + B + 7 * T + 13 * S + 29 * C_ + H + 3 * sg))
    Z, A, dM = rnd(B, N * H), (rnd(B, AW) * logit_scale).float().double(), rnd(B, G * H)
    M, P = cgc_fwd(Z, A, T, S, C_, sg)
    dZ, dA = cgc_bwd(Z, A, T, S, C_, sg, dM)
    M32, _ = cgc_fwd(Z.float(), A.float(), T, S, C_, sg)
    dZ32, dA32 = cgc_bwd(Z.float(), A.float(), T, S, C_, sg, dM.float())
    f32 = dict(M=grad_measure(M32, M), dZ=grad_measure(dZ32, dZ), dA=grad_measure(dA32, dA))
    return dict(B=B, T=T, S=S, C=C_, H=H, sg=sg, N=N, AW=AW, G=G, Z=Z, A=A, dM=dM, M=M, P=P, dZ=dZ, dA=dA, f32=f32)


# ------------------------------------------------------------------------------------------ the entire-space loss
def es_labels(Y, c, v):
    """-> (z [B], observed [B]): 0 where y_c == 0 (whatever y_v is), y_v where y_c == 1 and y_v is observed."""
    yc, yv = Y[:, c], Y[:, v]
    seen = (yc == 0) | ((yc == 1) & ~torch.isnan(yv))
    z = torch.where(yc == 0, torch.zeros_like(yv), yv)
    return torch.where(seen, z, torch.zeros_like(z)), seen


def es_loss_head(logit, Y, types, weights=None, es=(-1, -1)):
    """mmoe_ref.loss_head with the entire-space pair es = (c, v): logit [T, B], Y [B, T] (NaN = unobserved) ->
    (loss, loss_t [T], n_t [T], pred [T, B]).  pred[v] stays sigmoid(logit[v])."""
    if tuple(es) == (-1, -1):
        return R.loss_head(logit, Y, types, weights)
    c, v = es
    T = logit.shape[0]
    weights = [1.0] * T if weights is None else weights
    total, loss_t, n_t, preds = logit.new_zeros(()), [], [], []
    for t in range(T):
        if t == v:
            z, seen = es_labels(Y, c, v)
            pred = torch.sigmoid(logit[v])
            q = torch.sigmoid(logit[c]) * pred
            qc = q.clamp(TL.KERAS_EPS, 1 - TL.KERAS_EPS)
            z = z.to(q.dtype)
            l = -(z * torch.log(qc + TL.KERAS_EPS) + (1 - z) * torch.log(1 - qc + TL.KERAS_EPS))
        else:
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


def es_loss_head_grad(logit, Y, types, weights=None, es=(-1, -1), grad_scale=1.0):
    """(loss, loss_t, n_t, pred, dlogit [T, B] = grad_scale dloss/dlogit) by autograd."""
    leaf = logit.detach().clone().requires_grad_(True)
    loss, loss_t, n_t, pred = es_loss_head(leaf, Y, types, weights, es)
    if leaf.grad is None and loss.requires_grad:
        loss.backward()
    g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
    return loss.detach(), loss_t.detach(), n_t, pred.detach(), g * grad_scale


def _es_case(logit, Y, types, weights, es, grad_scale):
    want = es_loss_head_grad(logit, Y, types, weights, es, grad_scale)
    got32 = es_loss_head_grad(logit.float(), Y.float(), types, weights, es, grad_scale)
    f32 = dict(pred=grad_measure(got32[3], want[3]), dlogit=grad_measure(got32[4], want[4]),
               loss_t=grad_measure(got32[1], want[1]))
    return dict(T=logit.shape[0], B=logit.shape[1], es=tuple(es), types=types, weights=weights, grad_scale=grad_scale,
                logit=logit, Y=Y, loss=want[0], loss_t=want[1], n_t=want[2], pred=want[3], dlogit=want[4], f32=f32,
                z_seen=es_labels(Y, *es)[1])


def es_label_columns(g, B, share_nan_click=0.05, share_nan_conv=0.2):
    """(click [B], conversion [B]): 30 % clicks, a few click labels unobserved; the conversion label is NaN on every
    non-click and on a share of the clicks, otherwise 1 with probability 0.4."""
    click = (torch.rand(B, generator=g) < 0.3).double()
    conv = (torch.rand(B, generator=g) < 0.4).double()
    conv[(click == 0) | (torch.rand(B, generator=g) < share_nan_conv)] = NAN
    click[torch.rand(B, generator=g) < share_nan_click] = NAN
    return click, conv


@C.memo
def es_case(T, B, es=(0, 1), seed=0):
    """A seeded entire-space loss case in float64 (made once, never changed): logits ~ 2 N(0,1); the pair's tasks are
    classification, the others alternate regression and classification with about 30 % of their labels NaN; weights
    0.5 + 0.25 t; grad_scale 0.5.  With the float64 outputs and the float32 CPU restatement's own measures."""
    g = torch.Generator().manual_seed(37000 + 101 * seed + 17 * T + B + 1000 * es[0] + 100 * es[1])
    rnd = C.rnd_stream(g)
    others = [t for t in range(T) if t not in es]
    types = ["classification"] * T
    for i, t in enumerate(others):
        types[t] = "regression" if i % 2 == 0 else "classification"
    weights = [0.5 + 0.25 * t for t in range(T)]
    logit = rnd(T, B, std=2.0)
    Y = torch.empty(B, T, dtype=torch.float64)
    Y[:, es[0]], Y[:, es[1]] = es_label_columns(g, B)
    for t in others:
        Y[:, t] = (torch.rand(B, generator=g) < 0.3).double() if types[t] == "classification" else rnd(B)
        Y[torch.rand(B, generator=g) < 0.3, t] = NAN
    return _es_case(logit, Y, types, weights, es, 0.5)


@C.memo
def saturation_case():
    """The logits of the pair on the grid SAT_GRID x SAT_GRID, each point with z = 0 and z = 1 (y_c = 1, y_v = z): T = 2,
    es = (0, 1), B = 162.  `q` and `one_minus_q` are the float64 product and its complement, the latter formed without
    cancellation; `clipped` marks the points in the clip region."""
    a, b, z = torch.meshgrid(torch.tensor(SAT_GRID, dtype=torch.float64), torch.tensor(SAT_GRID, dtype=torch.float64),
                             torch.tensor([0.0, 1.0], dtype=torch.float64), indexing="ij")
    logit = torch.stack([a.reshape(-1), b.reshape(-1)])
    Y = torch.stack([torch.ones_like(z.reshape(-1)), z.reshape(-1)], dim=1)
    out = _es_case(logit, Y, ["classification"] * 2, [1.0, 0.75], (0, 1), 1.0)
    q = torch.sigmoid(logit[0]) * torch.sigmoid(logit[1])
    r = torch.sigmoid(-logit[0]) + torch.sigmoid(logit[0]) * torch.sigmoid(-logit[1])
    out.update(q=q, one_minus_q=r, clipped=(q < TL.KERAS_EPS) | (r < TL.KERAS_EPS))
    return out


# ---------------------------------------------------------------------------------------------------- the model
def is_ple(hp):
    return not (hp.get("task_experts", 0) == 0 and hp.get("num_levels", 1) == 1)


def es_pair(hp):
    es = hp.get("entire_space")
    return (-1, -1) if es is None else tuple(list(hp["task_names"]).index(n) for n in es)


def ple_logits(p, spec, idx, dense, hp, mv=None, pres=None, E_in=None, level=-1):
    """-> (logit [T, B], the task gates' weights [B, T, S + C] of `level`).  pres: a list that receives every expert
    and tower pre-activation.  E_in: the embeddings [B, F, D] to use instead of the lookup (to take their gradient).
    Without task experts and levels this is mmoe_ref.mmoe_logits."""
    if not is_ple(hp):
        return R.mmoe_logits(p, spec, idx, dense, hp, mv, pres, E_in)
    names = hp["task_names"]
    T, S, C_, L, units = len(names), hp["task_experts"], hp["num_experts"], hp["num_levels"], list(hp["expert_hidden_units"])
    N, W, H = T * S + C_, S + C_, units[-1]
    act = TL.act_fn(hp.get("deep_activation", "relu"))
    x = TL.dnn_input(embeddings(p, spec, idx, hp, mv) if E_in is None else E_in, dense)
    B = x.shape[0]
    X, P_out = [x] * (T + 1), None
    for l in range(L):
        sg = l < L - 1
        W0, b0, Gw = (p[f"level_{l}_expert_layer_0_weights"], p[f"level_{l}_expert_layer_0_bias"],
                      p[f"level_{l}_gate_weights"])
        group = lambda s: (s * S * units[0], (s * S + (S if s < T else C_)) * units[0])  # noqa: E731
        pre = torch.cat([X[s] @ W0[:, group(s)[0]: group(s)[1]] + b0[group(s)[0]: group(s)[1]] for s in range(T + 1)],
                        dim=1)
        if pres is not None:
            pres.append(pre)
        h = act(pre)
        for k in range(1, len(units)):
            Wk, bk = p[f"level_{l}_expert_layer_{k}_weights"], p[f"level_{l}_expert_layer_{k}_bias"]
            pre = torch.einsum("bek,ekn->ben", h.reshape(B, N, units[k - 1]), Wk) + bk
            if pres is not None:
                pres.append(pre)
            h = act(pre).reshape(B, N * units[k])
        A = torch.cat([X[g] @ Gw[:, a0:a1] for g, (a0, a1, _) in enumerate(gates(T, S, C_, sg))], dim=1)
        M, P = cgc_fwd(h, A, T, S, C_, sg)
        X = [M[:, g * H: (g + 1) * H] for g in range(T + (1 if sg else 0))]
        if l == range(L)[level]:
            P_out = P[:, : T * W].reshape(B, T, W)
    n = len(hp["tower_hidden_units"])
    logits = []
    for t, name in enumerate(names):
        tv = tower_vars(p, name)
        y = X[t]
        if pres is not None:
            for i in range(n):
                pres.append(y @ tv[f"dnn_layer_{i}_weights"] + tv[f"dnn_layer_{i}_bias"])
                y = act(pres[-1])
        logits.append(TL.dnn(tv, X[t], n, hp.get("deep_activation", "relu")).reshape(-1))
    return torch.stack(logits), P_out


def ple_l2(p, spec, hp):
    if not is_ple(hp):
        return R.mmoe_l2(p, spec, hp)
    tl = spec.tl if hasattr(spec, "tl") else spec
    out = TL.embedding_l2(p, tl, hp.get("embedding_l2_reg", 0.0))
    reg = hp.get("deep_l2_reg", 0.0)
    ws = [v for n, v in p.items() if n.startswith("level_") and n.endswith("_weights")]
    for name in hp["task_names"]:
        tv = tower_vars(p, name)
        ws += [v for n, v in tv.items() if n.endswith("_weights") or n == "dnn_w"]
    return out + sum(reg * 0.5 * w.square().sum() for w in ws)


def model_loss(p, spec, idx, dense, Y, hp, mv=None, E_in=None):
    logit, _ = ple_logits(p, spec, idx, dense, hp, mv, E_in=E_in)
    loss, loss_t, n_t, pred = es_loss_head(logit, Y.to(logit.dtype), hp["task_types"], hp.get("task_weights"),
                                           es_pair(hp))
    return loss + ple_l2(p, spec, hp), logit, pred


def fwd_bwd(p, spec, idx, dense, Y, hp, mv=None):
    """One forward+backward: (loss, logit [T, B], pred [T, B], grads) - the twin of oracle.th_layers.fwd_bwd."""
    out, grads = C.backward(model_loss, p, spec, idx, dense, Y, hp, mv)
    return out + (grads,)


def d_rows(p, spec, idx, dense, Y, hp, mv=None):
    """dLoss/dE [B, F, D] of the data loss (no l2): what the engine's d_rows holds (mmoe_ref.d_rows)."""
    E = embeddings(p, spec, idx, hp, mv).detach().clone().requires_grad_(True)
    logit, _ = ple_logits(p, spec, idx, dense, hp, mv, E_in=E)
    es_loss_head(logit, Y.to(logit.dtype), hp["task_types"], hp.get("task_weights"), es_pair(hp))[0].backward()
    return E.grad


# model-level cases: (task_types, task_experts S, shared experts C, levels L, expert_hidden_units, tower_hidden_units, B,
# F, D, Dn, nan_share, entire_space, attempt).  `attempt` is the first stream of make_case whose every expert and tower
# ReLU pre-activation is at least KINK from 0 in float64 (tests/test_ple_host.py asserts it); towers of (8,) run the
# fused skinny-MLP kernels, (40,) and (64, 16) the layer-by-layer path.  S = 0: the MMoE engine (C experts).
C2 = ("classification", "classification")
C3 = ("classification", "classification", "classification")
MODEL_CASES = {
    "two_levels": (C2, 2, 2, 2, (32, 16), (8,), 70, 5, 8, 3, 0.0, None, 0),
    "cgc_no_dense": (C2, 1, 1, 1, (16,), (40,), 67, 3, 16, 0, 0.0, None, 0),
    "three_tasks_nan": (("classification", "regression", "classification"), 1, 3, 3, (24, 16), (64, 16), 71, 7, 8, 2,
                        0.6, None, 0),
    "one_task": (("classification",), 1, 1, 2, (16,), (8,), 66, 4, 8, 2, 0.0, None, 0),
    "entire_space_mmoe": (C2, 0, 3, 1, (32, 16), (8,), 70, 5, 8, 3, 0.0, ("ctr", "cvr"), 0),
    "entire_space_ple": (C3, 2, 2, 2, (16,), (40,), 69, 4, 8, 1, 0.3, ("ctr", "cvr"), 0),
}
SEQ_CASE = (C2, 1, 2, 2, (16, 8), (40,), 0)  # over tests/asp_ref.py's front (B = 37, D = 8, two dense features)


def _model_vars(rnd, p, K0, names, S, C_, L, units, towers):
    if S == 0:
        return R._model_vars(rnd, p, K0, names, C_, units, towers)
    T = len(names)
    N, H = T * S + C_, units[-1]
    for l in range(L):
        K, AW = (K0 if l == 0 else H), widths(T, S, C_, l < L - 1)[1]
        p[f"level_{l}_expert_layer_0_weights"] = C.glorot(rnd, (K, N * units[0]), K, units[0])
        p[f"level_{l}_expert_layer_0_bias"] = rnd(N * units[0], std=0.1)
        for k in range(1, len(units)):
            p[f"level_{l}_expert_layer_{k}_weights"] = C.glorot(rnd, (N, units[k - 1], units[k]), units[k - 1], units[k])
            p[f"level_{l}_expert_layer_{k}_bias"] = rnd(N, units[k], std=0.1)
        p[f"level_{l}_gate_weights"] = rnd(K, AW, std=0.3)  # (wide enough that the gates are not all near uniform)
    for name in names:
        C.draw_dnn(rnd, p, [H] + list(towers), prefix=f"{name}_")


def _hp(types, S, C_, L, units, towers, D, l2, es):
    hp = R._hp(types, C_, units, towers, D, l2)
    hp.update(task_experts=S, num_levels=L, entire_space=es)
    return hp


def _labels(g, rnd, B, types, nan_share, hp):
    Y = R._labels(g, rnd, B, types, nan_share)
    if hp["entire_space"] is not None:
        c, v = es_pair(hp)
        Y[:, c], Y[:, v] = es_label_columns(g, B)
    return Y


def min_abs_pre(p, spec, idx, dense, hp, mv=None):
    pres = []
    with torch.no_grad():
        ple_logits(p, spec, idx, dense, hp, mv, pres=pres)
    return C.min_abs(pres)


@C.memo
def make_case(types, S, C_, L, units, towers, B, F, D, Dn, nan_share, es, attempt, l2=1e-4):
    """A seeded model-level case in float64 (made once, never changed): spec, p (the contract's variable names, with
    the unused linear_w / linear_w0 of every state_dict), idx, dense, Y [B, T], hp.  Embeddings ~ N(0, 0.3^2), dense ~
    N(0,1); `min_abs_pre` is the distance of the closest expert or tower unit to its kink."""
    spec, sizes = C.plain_spec(F, Dn)
    hp = _hp(types, S, C_, L, units, towers, D, l2, es)
    g = torch.Generator().manual_seed(38000 + attempt)
    rnd = C.rnd_stream(g)
    p = {f"{name}_feat_embed": rnd(V, D, std=0.3) for name, V in zip(spec.sparse_names, sizes)}
    p["linear_w"] = torch.zeros(spec.lin_layout[2], 1, dtype=torch.float64)
    p["linear_w0"] = torch.zeros(1, dtype=torch.float64)
    _model_vars(rnd, p, F * D + Dn, hp["task_names"], S, C_, L, units, towers)
    idx, dense = C.draw_idx(g, sizes, B), rnd(B, Dn)
    Y = _labels(g, rnd, B, types, nan_share, hp)
    return dict(spec=spec, p=p, idx=idx, dense=dense, Y=Y, hp=hp, mv=None,
                min_abs_pre=min_abs_pre(p, spec, idx, dense, hp))


@C.memo
def make_seq_case(types=SEQ_CASE[0], S=SEQ_CASE[1], C_=SEQ_CASE[2], L=SEQ_CASE[3], units=SEQ_CASE[4],
                  towers=SEQ_CASE[5], attempt=SEQ_CASE[6], l2=1e-3):
    """PLE over the front of tests/asp_ref.py:make_model_case, as mmoe_ref.make_seq_case: the embedding tables, the
    unit's variables, ids, histories and dense values are that case's, the PLE variables and labels are drawn here."""
    u = asp_ref.make_model_case("din", B=37, D=8, Dn=2, seed=attempt, max_len=6)
    spec = u["spec"]
    p = {n: v for n, v in u["p"].items() if not n.startswith("dnn_")}
    hp = _hp(types, S, C_, L, units, towers, 8, l2, None)
    hp.update({n: u["hp"][n] for n in ("att_hidden_units", "att_activation", "att_weight_normalization")},
              seq_pooling="din")
    g = torch.Generator().manual_seed(39000 + attempt)
    rnd = C.rnd_stream(g)
    _model_vars(rnd, p, spec.F * 8 + 2, hp["task_names"], S, C_, L, units, towers)
    Y = R._labels(g, rnd, 37, types, 0.3)
    return dict(model="ple", spec=spec, p=p, idx=u["idx"], dense=u["dense"], Y=Y, hp=hp, mv=u["mv"],
                min_abs_pre=min_abs_pre(p, spec, u["idx"], u["dense"], hp, u["mv"]))
