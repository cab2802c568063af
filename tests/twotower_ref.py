"""CPU PyTorch restatement (dtype-generic) of two-tower retrieval: the in-batch softmax loss with its closed-form
backward, the row normalisation, and the model built on them.

TEST INFRASTRUCTURE.  Nothing in the reference implements a retrieval model, so the arithmetic is the project's contract
(include/recman_hip.h, engine.TwoTowerEngine).  U, V [B, H]:

    S_ij    = scale <U_i, V_j> - logq_j                       (logq None: 0; applied to the diagonal too)
    allowed = (j == i) or item_id None or item_id_j != item_id_i
    lse_i   = log sum_{j allowed} exp(S_ij);   l_i = lse_i - S_ii;   W = sum_i w_i;   loss = sum_i w_i l_i / W  (W = 0: 0)
    rank_i  = #{ j allowed, j != i : S_ij > S_ii }
    backward: P_ij = exp(S_ij - lse_i) for allowed j, else 0;  G_ij = grad_scale w_i / W (P_ij - [i == j])
              dU = scale G V;  dV = scale G^T U                                              (W = 0: both 0)
    rownorm:  Y = X / max(|X|_2, eps);  dX = (dY - Y <Y, dY>) / max(|X|_2, eps)
    model:    x = [E | dense]; u = tower_user(x's user columns), v = tower_item(its item columns): act(x W + b) per
              hidden layer, a last linear layer; rows normalised with hp["normalize"]; scale = 1 / temperature;
              logq = item_logq[item id]; the labels are the weights w; + the l2 terms

The embedding and l2 pieces are oracle.th_layers' public functions.  tests/test_twotower_host.py pins this file without a
GPU; the GPU tests compare the HIP kernels and the engine against it in float64, with the float32 run of the same code
as the yardstick of the tolerances:
    measure <= max(TOL_GRAD, 4 x the float32 CPU restatement's own measure on the case)      (tests/test_gpu_asp.py)
"""
import math

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK, glorot, grad_measure, to_f32  # noqa: F401  (part of this module's interface)

TOL_GRAD = 2e-5
EPS = 1e-12   # the row norm's floor (engine.TwoTowerEngine.EPS)
TIE = 1e-4    # |S_ij - S_ii| <= TIE max(1, |S_ii|) in float64 is a near tie: the float32 rank may differ there
TIE_SHARE = 0.25  # at most this share of a rank case's rows may have a near tie

# kernel-level GPU cases (B, H): the smallest shapes at which a tile edge, a k-step, a split or a mask can go wrong
CASES = [(1, 4), (15, 8), (16, 16), (17, 20), (64, 64), (65, 64), (130, 36), (200, 256)]
ROWNORM_CASES = [(1, 4), (33, 20), (77, 256)]


def bound(f32_measure):
    return max(TOL_GRAD, 4.0 * f32_measure)


# ------------------------------------------------------------------------------------------------------ the loss
def scores(U, V, scale, logq=None):
    S = scale * (U @ V.t())
    return S if logq is None else S - logq.to(S.dtype).unsqueeze(0)


def allowed(B, item_id=None):
    eye = torch.eye(B, dtype=torch.bool)
    if item_id is None:
        return torch.ones(B, B, dtype=torch.bool)
    return eye | (item_id.unsqueeze(0) != item_id.unsqueeze(1))


def fwd(U, V, scale, item_id=None, logq=None, w=None):
    """-> dict(S, ok, lse [B], row_loss [B], loss [], rank [B] int64, W)."""
    B = U.shape[0]
    S, ok = scores(U, V, scale, logq), allowed(B, item_id)
    lse = torch.logsumexp(S.masked_fill(~ok, -math.inf), dim=1)
    diag = S.diagonal()
    row_loss = lse - diag
    wt = torch.ones(B, dtype=S.dtype) if w is None else w.to(S.dtype)
    W = wt.sum()
    loss = (wt * row_loss).sum() / W if float(W) > 0 else S.new_zeros(())
    off = ok & ~torch.eye(B, dtype=torch.bool)
    rank = (off & (S > diag.unsqueeze(1))).sum(dim=1)
    return dict(S=S, ok=ok, lse=lse, row_loss=row_loss, loss=loss, rank=rank, W=W)


def bwd(U, V, scale, item_id=None, logq=None, w=None, grad_scale=1.0):
    """The closed-form backward of the contract (no autograd): -> (dU, dV)."""
    B = U.shape[0]
    f = fwd(U, V, scale, item_id, logq, w)
    if float(f["W"]) == 0:
        return torch.zeros_like(U), torch.zeros_like(V)
    P = torch.where(f["ok"], torch.exp(f["S"] - f["lse"].unsqueeze(1)), torch.zeros_like(f["S"]))
    wt = torch.ones(B, dtype=U.dtype) if w is None else w.to(U.dtype)
    G = (grad_scale * wt / f["W"]).unsqueeze(1) * (P - torch.eye(B, dtype=U.dtype))
    return scale * (G @ V), scale * (G.t() @ U)


def loss_autograd(U, V, scale, item_id=None, logq=None, w=None, grad_scale=1.0):
    """(loss, dU, dV) with the gradient of grad_scale * loss by autograd."""
    u, v = U.detach().clone().requires_grad_(True), V.detach().clone().requires_grad_(True)
    loss = fwd(u, v, scale, item_id, logq, w)["loss"]
    if loss.requires_grad:
        (grad_scale * loss).backward()
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)  # noqa: E731
    return loss.detach(), z(u), z(v)


def loops(U, V, scale, item_id=None, logq=None):
    """lse, row_loss and rank as explicit Python loops over floats (no tensor arithmetic)."""
    u, v = U.tolist(), V.tolist()
    B = len(u)
    ids = None if item_id is None else item_id.tolist()
    q = [0.0] * B if logq is None else logq.tolist()
    lse, rl, rank = [], [], []
    for i in range(B):
        s = [scale * sum(a * b for a, b in zip(u[i], v[j])) - q[j] for j in range(B)]
        ok = [j == i or ids is None or ids[j] != ids[i] for j in range(B)]
        mx = max(s[j] for j in range(B) if ok[j])
        l = mx + math.log(sum(math.exp(s[j] - mx) for j in range(B) if ok[j]))
        lse.append(l)
        rl.append(l - s[i])
        rank.append(sum(1 for j in range(B) if ok[j] and j != i and s[j] > s[i]))
    return lse, rl, rank


def near_ties(S, ok):
    """Per row the number of allowed j != i with |S_ij - S_ii| <= TIE max(1, |S_ii|) (float64 S)."""
    B = S.shape[0]
    d = S.diagonal().unsqueeze(1)
    off = ok & ~torch.eye(B, dtype=torch.bool)
    return (off & ((S - d).abs() <= TIE * torch.clamp(d.abs(), min=1.0))).sum(dim=1)


def check_ranks(rank, k, what=""):
    """The float32 ranks of a kernel against case k: equal on every row without a near tie, elsewhere off by at most
    the row's near ties; at most TIE_SHARE of the rows have one."""
    rank, want, ties = rank.cpu().long(), k["rank"], k["ties"]
    share = float((ties > 0).double().mean())
    assert share <= TIE_SHARE, f"{what}{share:.2f} of the rows have a near tie"
    diff = (rank - want).abs()
    assert torch.equal(rank[ties == 0], want[ties == 0]), f"{what}rank differs on rows without a near tie"
    assert bool((diff <= ties).all()), f"{what}rank off by more than the row's near ties"


def rownorm_fwd(X, eps=EPS):
    """-> (Y, inv_norm [B])."""
    inv = 1.0 / torch.clamp(torch.linalg.vector_norm(X, dim=1), min=eps)
    return X * inv.unsqueeze(1), inv


def rownorm_bwd(Y, inv, dY):
    return inv.unsqueeze(1) * (dY - Y * (Y * dY).sum(dim=1, keepdim=True))


@C.memo
def ibs_case(B, H, ids=True, logq=True, w=True, scale=20.0, normalised=True, seed=0, same_ids=False, zero_w=False):
    """A seeded kernel-level case in float64 (made once per key, never changed): U, V ~ N(0,1), rows normalised (in
    float64, then rounded to float32 values) when `normalised`; item ids from about B/3 values (real duplicates), logq
    in [-6, 0], about a quarter of w zero; grad_scale 0.5.  With the float64 outputs lse, row_loss, loss, rank, dU, dV,
    the near-tie counts `ties` and the float32 CPU restatement's own measures `f32`."""
    g = torch.Generator().manual_seed(41000 + 131 * seed + 7 * B + H)
    rnd = C.rnd_stream(g)
    U, V = rnd(B, H), rnd(B, H)
    if normalised:
        U, V = rownorm_fwd(U)[0].float().double(), rownorm_fwd(V)[0].float().double()
    item = torch.randint(0, max(1, B // 3), (B,), generator=g) + 5 if ids else None
    if same_ids:
        item = torch.full((B,), 9, dtype=torch.int64)
    lq = (-6.0 * torch.rand(B, generator=g, dtype=torch.float64)).float().double() if logq else None
    wt = (torch.rand(B, generator=g) >= 0.25).double() if w else None
    if zero_w:
        wt = torch.zeros(B, dtype=torch.float64)
    gs = 0.5
    f = fwd(U, V, scale, item, lq, wt)
    dU, dV = bwd(U, V, scale, item, lq, wt, gs)
    c32 = lambda t: None if t is None else t.float()  # noqa: E731
    f32r = fwd(U.float(), V.float(), scale, item, c32(lq), c32(wt))
    dU32, dV32 = bwd(U.float(), V.float(), scale, item, c32(lq), c32(wt), gs)
    f32 = dict(lse=grad_measure(f32r["lse"], f["lse"]), row_loss=grad_measure(f32r["row_loss"], f["row_loss"]),
               loss=grad_measure(f32r["loss"], f["loss"]), dU=grad_measure(dU32, dU), dV=grad_measure(dV32, dV))
    return dict(B=B, H=H, U=U, V=V, item=item, logq=lq, w=wt, scale=scale, grad_scale=gs, S=f["S"],
                lse=f["lse"], row_loss=f["row_loss"], loss=f["loss"], rank=f["rank"], dU=dU, dV=dV,
                ties=near_ties(f["S"], f["ok"]), f32=f32)


@C.memo
def rownorm_case(B, H, seed=0):
    rnd = C.rnd_stream(torch.Generator().manual_seed(42000 + 17 * seed + 3 * B + H))
    X, dY = rnd(B, H, std=2.0), rnd(B, H)
    Y, inv = rownorm_fwd(X)
    dX = rownorm_bwd(Y, inv, dY)
    Y32, inv32 = rownorm_fwd(X.float())
    f32 = dict(Y=grad_measure(Y32, Y), dX=grad_measure(rownorm_bwd(Y32, inv32, dY.float()), dX))
    return dict(B=B, H=H, X=X, dY=dY, Y=Y, inv=inv, dX=dX, f32=f32)


# ---------------------------------------------------------------------------------------------------- the model
def _cols(spec, names):
    return ([j for j, n in enumerate(spec.sparse_names) if n in names],
            [j for j, n in enumerate(spec.dense_names) if n in names])


def tower(p, side, x, n_layers, activation, pres=None):
    act = TL.act_fn(activation)
    for i in range(n_layers):
        x = x @ p[f"{side}_dnn_layer_{i}_weights"] + p[f"{side}_dnn_layer_{i}_bias"]
        if i < n_layers - 1:
            if pres is not None:
                pres.append(x)
            x = act(x)
    return x


def tower_out(p, spec, side, E, dense, hp, pres=None):
    """The embeddings [B, H] of one tower from E [B, F, D] and the dense columns."""
    fe, fd = _cols(spec, hp[f"{side}_features"])
    x = E[:, fe].reshape(E.shape[0], -1)
    if fd:
        x = torch.cat([x, dense[:, fd].to(x.dtype)], dim=1)
    out = tower(p, side, x, len(hp[f"{side}_hidden_units"]), hp.get("deep_activation", "relu"), pres)
    return rownorm_fwd(out)[0] if hp.get("normalize", True) else out


def embeddings(p, spec, idx, mv=None):
    return TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)[0]


def model_parts(p, spec, idx, dense, hp, mv=None, E_in=None, pres=None):
    """-> (u, v, item ids or None, logq or None, scale)."""
    E = embeddings(p, spec, idx, mv) if E_in is None else E_in
    u, v = tower_out(p, spec, "user", E, dense, hp, pres), tower_out(p, spec, "item", E, dense, hp, pres)
    col = idx[:, spec.sparse_names.index(hp["item_id_feature"])] if hp.get("item_id_feature") else None
    ids = col if hp.get("mask_accidental_hits", True) else None
    logq = p["item_logq"][col] if hp.get("logq_correction", False) else None
    return u, v, ids, logq, 1.0 / hp["temperature"]


def model_l2(p, spec, hp):
    out = TL.embedding_l2(p, spec, hp.get("embedding_l2_reg", 0.0))
    reg = hp.get("deep_l2_reg", 0.0)
    return out + sum(reg * 0.5 * v.square().sum() for n, v in p.items()
                     if n.endswith("_weights") and n.split("_")[0] in ("user", "item"))


def model_loss(p, spec, idx, dense, y, hp, mv=None, E_in=None):
    """(loss + l2, the forward's dict); y [B] weights or None."""
    u, v, ids, logq, scale = model_parts(p, spec, idx, dense, hp, mv, E_in)
    f = fwd(u, v, scale, ids, logq, y)
    return f["loss"] + model_l2(p, spec, hp), f


def fwd_bwd(p, spec, idx, dense, y, hp, mv=None):
    """One forward+backward: (loss, row_loss [B], rank [B], grads)."""
    def loss_fn(leaves):
        loss, f = model_loss(leaves, spec, idx, dense, y, hp, mv)
        return loss, f["row_loss"], f["rank"]

    out, grads = C.backward(loss_fn, p)
    return out + (grads,)


def d_rows(p, spec, idx, dense, y, hp, mv=None):
    """dLoss/dE [B, F, D] of the data loss (no l2): what the engine's d_rows holds."""
    E = embeddings(p, spec, idx, mv).detach().clone().requires_grad_(True)
    u, v, ids, logq, scale = model_parts(p, spec, idx, dense, hp, mv, E_in=E)
    loss = fwd(u, v, scale, ids, logq, y)["loss"]
    if loss.requires_grad:
        loss.backward()
    return E.grad if E.grad is not None else torch.zeros_like(E)


def sgd_steps(p, spec, idx, dense, y, hp, lr, steps, mv=None):
    """`steps` plain SGD steps on the same batch in float64 -> (per-step losses, final p).  item_logq is no trained
    variable; linear_w / linear_w0 have zero gradients."""
    p = {k: v.clone() for k, v in p.items()}
    losses = []
    for _ in range(steps):
        loss, _, _, g = fwd_bwd(p, spec, idx, dense, y, hp, mv)
        losses.append(float(loss))
        for k in p:
            if k != "item_logq":
                p[k] = p[k] - lr * g[k]
    return losses, p


USER, ITEM = ("U0", "U1", "Utags", "du"), ("item", "Icat", "di")
SIZES = dict(U0=7, U1=11, Utags=5, item=13, Icat=6)


def min_abs_pre(p, spec, idx, dense, hp, mv):
    pres = []
    with torch.no_grad():
        model_parts(p, spec, idx, dense, hp, mv, pres=pres)
    return C.min_abs(pres)


@C.memo
def make_case(normalize=True, masking=True, logq=False, labels=False, B=37, D=8, units=((16, 8), (12, 8)), l2=1e-4,
              attempt=0):
    """A seeded model-level case in float64 (made once, never changed): three user embedding features (Utags
    multi-valued) and two item ones, one dense feature per tower.  spec, p (the contract's variable names, with the
    unused linear_w / linear_w0 of every state_dict), idx, dense, y (weights or None), mv, hp.  Embeddings ~ N(0,
    0.3^2), dense ~ N(0,1).  The first stream from `attempt` on whose every hidden ReLU pre-activation is at least
    KINK from 0 in float64 is taken (`attempt` in the result says which)."""
    names = [n for n in USER + ITEM if n in SIZES]
    spec = TL.Spec(names, [SIZES[n] for n in names], ["du", "di"], multi_names=["Utags"])
    hp = dict(embedding_size=D, embedding_l2_reg=l2, deep_l2_reg=l2, user_features=USER, item_features=ITEM,
              item_id_feature="item", user_hidden_units=tuple(units[0]), item_hidden_units=tuple(units[1]),
              temperature=0.05 if normalize else 1.0, normalize=normalize, mask_accidental_hits=masking,
              logq_correction=logq, deep_activation="relu")
    # (its own loop and front: ten streams from `attempt` on, the last one kept whatever its gap; the linear term is
    # unused, so linear_w and linear_w0 are zeros and draw nothing; Utags' ids come as a CSR)
    for a in range(attempt, attempt + 10):
        g = torch.Generator().manual_seed(43000 + a)
        rnd = C.rnd_stream(g)
        p = {f"{n}_feat_embed": rnd(SIZES[n], D, std=0.3) for n in names}
        p["linear_w"] = torch.zeros(spec.lin_layout[2], 1, dtype=torch.float64)
        p["linear_w0"] = torch.zeros(1, dtype=torch.float64)
        for side, un, feats in (("user", units[0], USER), ("item", units[1], ITEM)):
            d_in = sum(D for n in feats if n in SIZES) + sum(1 for n in feats if n not in SIZES)
            C.draw_dnn(rnd, p, [d_in] + list(un), head=False, prefix=f"{side}_")
        p["item_logq"] = (-6.0 * torch.rand(SIZES["item"], generator=g, dtype=torch.float64)).float().double()
        idx = torch.stack([torch.randint(0, SIZES[n], (B,), generator=g) for n in names], 1)
        idx[:, names.index("Utags")] = 0  # (a multi-valued feature's idx column is a placeholder)
        n_tags = torch.randint(0, 4, (B,), generator=g)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(n_tags, 0)])
        mv = {"Utags": (offsets, torch.randint(0, SIZES["Utags"], (int(offsets[-1]),), generator=g))}
        dense = rnd(B, 2)
        y = (torch.rand(B, generator=g) >= 0.25).double() if labels else None
        gap = min_abs_pre(p, spec, idx, dense, hp, mv)
        if gap >= KINK:
            break
    return dict(spec=spec, p=p, idx=idx, dense=dense, y=y, mv=mv, hp=hp, min_abs_pre=gap, attempt=a)
