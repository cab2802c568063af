"""CPU PyTorch restatement (dtype-generic) of the field-pair weighted FM family - FwFM (arXiv 1806.03514), FvFM and
FmFM (arXiv 2102.12994) - and of the model built on it.

TEST INFRASTRUCTURE.  Nothing in the reference implements these models, so the arithmetic is the papers' as the
project's contract states it.  Per example, E [F,D], P = F(F-1)/2 pairs p = (i, j), 0 <= i < j < F, in
itertools.combinations order:

    pair_logit = sum_p E_i W_(p) E_j^T
      "matrix": W_(p) = M[p]        field_pair_w [P,D,D]   (FmFM; the LEFT field i on the rows)
      "vector": W_(p) = diag(w[p])  field_pair_w [P,D]     (FvFM)
      "scalar": W_(p) = r[p] I      field_pair_w [P]       (FwFM)
    logit = linear (use_linear) + pair_logit (+ DNN([E | dense]) with a non-empty deep_hidden_units)

    backward, g = dLoss/dpair_logit:  dE_i += g W_(p) E_j   dE_j += g W_(p)^T E_i   dM[p] = sum_b g_b E_i (x) E_j
      (vector: its diagonal; scalar: its trace)

Everything but the pair term is composed from the public functions of oracle.th_layers, imported and not modified.
tests/test_fmfm_host.py pins this file without a GPU; the GPU tests compare the HIP kernels and the engine against it in
float64.
"""
import itertools

import torch

from oracle import th_layers as TL

TYPES = ("matrix", "vector", "scalar")
# kernel-level GPU cases (B, F, D) of tests/test_gpu_fmfm.py, each for the three types (the grid-stride case is built
# there): one pair; an odd pair count at D = 8 (a lone last pair in the two-pairs-per-MFMA packing); B no multiple of
# 16 or of the tile; several tiles; F at the limit; every supported D
GPU_CASES = [(5, 2, 8), (33, 3, 8), (37, 5, 8), (130, 26, 16), (65, 10, 32), (9, 40, 32), (257, 26, 16), (6, 27, 16)]
# model-level cases: (type, hidden, B, F, D, Dn)
MODEL_CASES = {
    "scalar_no_dnn": ("scalar", (), 33, 5, 8, 3),
    "vector_dnn": ("vector", (16, 16), 257, 5, 8, 0),
    "matrix_criteo_like": ("matrix", (32, 32), 130, 26, 16, 13),
}
TOL_LOGIT, TOL_GRAD = 1e-5, 2e-5  # |logit - logit64| <= TOL_LOGIT max(1, |logit64|); the project's gradient measure
KINK = 1e-6  # a relu unit whose float64 pre-activation is this close to 0 may flip in fp32
WRONG = ("transposed", "with_diagonal", "both_orders", "matrix_by_left_field")


def pairs(F):
    return F * (F - 1) // 2


def pair_fields(F):
    """(left fields, right fields) of the P pairs in itertools.combinations order, as index tensors."""
    li, lj = zip(*itertools.combinations(range(F), 2))
    return torch.tensor(li), torch.tensor(lj)


def weight_shape(F, D, ftype):
    return {"matrix": (pairs(F), D, D), "vector": (pairs(F), D), "scalar": (pairs(F),)}[ftype]


def as_matrices(W, D, ftype):
    """field_pair_w of any type as [P,D,D] matrices."""
    if ftype == "matrix":
        return W
    eye = torch.eye(D, dtype=W.dtype)
    return W.unsqueeze(2) * eye if ftype == "vector" else W.view(-1, 1, 1) * eye


def wrong_applies(wrong, F, ftype):
    """Whether a deliberately wrong variant differs from the contract at all: a transposed diagonal matrix is itself;
    choosing the matrix by the left field alone is the contract itself while every left field leads one pair (F = 2)."""
    if wrong == "transposed":
        return ftype == "matrix"
    if wrong == "matrix_by_left_field":
        return F >= 3
    return True


def _first_pair_of_left(F):
    """For every pair, the index of the first pair with the same left field."""
    li, _ = pair_fields(F)
    first = {}
    for p, i in enumerate(li.tolist()):
        first.setdefault(i, p)
    return torch.tensor([first[i] for i in li.tolist()])


def pair_terms(E, W, ftype, wrong=None):
    """E [B,F,D] -> [B,P]: every pair's E_i W_(p) E_j^T (no sum over pairs yet)."""
    B, F, D = E.shape
    li, lj = pair_fields(F)
    Wm = as_matrices(W, D, ftype)
    if wrong == "matrix_by_left_field":
        Wm = Wm[_first_pair_of_left(F)]
    left, right = (E[:, lj], E[:, li]) if wrong == "transposed" else (E[:, li], E[:, lj])
    if ftype == "matrix" or wrong == "matrix_by_left_field":
        return (torch.einsum("bpk,pkd->bpd", left, Wm) * right).sum(dim=2)
    w = W if ftype == "vector" else W.unsqueeze(1)
    return (left * w * right).sum(dim=2)


def pair_logit(E, W, ftype, wrong=None):
    """E [B,F,D], field_pair_w -> [B].  wrong: one of WRONG, the deliberately wrong restatements that
    tests/test_fmfm_host.py shows the tolerances to catch.  Each pair is summed on its own, then the pairs."""
    out = pair_terms(E, W, ftype, wrong).sum(dim=1)
    if wrong in ("with_diagonal", "both_orders"):
        B, F, D = E.shape
        li, lj = pair_fields(F)
        Wm = as_matrices(W, D, ftype)
        if wrong == "both_orders":  # + E_j W_(p) E_i^T
            out = out + (torch.einsum("bpk,pkd->bpd", E[:, lj], Wm) * E[:, li]).sum(dim=(1, 2))
        else:  # + i = j, with the matrix of the first pair field i is part of
            first = [min(p for p in range(li.numel()) if f in (int(li[p]), int(lj[p]))) for f in range(F)]
            out = out + (torch.einsum("bfk,fkd->bfd", E, Wm[torch.tensor(first)]) * E).sum(dim=(1, 2))
    return out


def pair_logit_loops(E, W, ftype):
    """pair_logit as explicit Python loops over floats (no tensor arithmetic)."""
    El, Wl = E.tolist(), W.tolist()
    F, D = len(El[0]), len(El[0][0])
    out = []
    for e in El:
        total, p = 0.0, 0
        for i in range(F):
            for j in range(i + 1, F):
                if ftype == "matrix":
                    total += sum(e[i][k] * Wl[p][k][d] * e[j][d] for k in range(D) for d in range(D))
                elif ftype == "vector":
                    total += sum(e[i][d] * Wl[p][d] * e[j][d] for d in range(D))
                else:
                    total += Wl[p] * sum(e[i][d] * e[j][d] for d in range(D))
                p += 1
        out.append(total)
    return torch.tensor(out, dtype=E.dtype)


def pair_bwd(E, W, ftype, g):
    """The backward of the contract, written out (no autograd): g [B] -> (dE [B,F,D], dW like W)."""
    B, F, D = E.shape
    li, lj = pair_fields(F)
    Ei, Ej, gb = E[:, li], E[:, lj], g.view(B, 1, 1)
    dE = torch.zeros_like(E)
    if ftype == "matrix":
        dE.index_add_(1, li, gb * torch.einsum("pkd,bpd->bpk", W, Ej))
        dE.index_add_(1, lj, gb * torch.einsum("bpk,pkd->bpd", Ei, W))
        return dE, torch.einsum("b,bpk,bpd->pkd", g, Ei, Ej)
    w = W if ftype == "vector" else W.unsqueeze(1)
    dE.index_add_(1, li, gb * w * Ej)
    dE.index_add_(1, lj, gb * w * Ei)
    dw = torch.einsum("b,bpd->pd", g, Ei * Ej)
    return dE, dw if ftype == "vector" else dw.sum(dim=1)


def fm_second_order(E):
    """Plain FM: 0.5 (|sum_f E_f|^2 - sum_f |E_f|^2)."""
    return 0.5 * (E.sum(dim=1).square().sum(dim=1) - E.square().sum(dim=(1, 2)))


def init_weights(F, D, ftype, dtype=torch.float64):
    """The initial field_pair_w: identity matrices, all-ones vectors, all-ones scalars."""
    if ftype == "matrix":
        return torch.eye(D, dtype=dtype).expand(pairs(F), D, D).clone()
    return torch.ones(weight_shape(F, D, ftype), dtype=dtype)


def _rnd(g):
    def rnd(*shape, std=1.0):
        # (every value is a float32 number: the kernels, the float32 restatement and float64 see the same inputs)
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * std).float().double()
    return rnd


def glorot(rnd, shape, fan_in, fan_out):
    return rnd(*shape, std=(2.0 / (fan_in + fan_out)) ** 0.5)


SPECIAL_ROWS = {3: "E = 0", 4: "g = 0", 5: "E x 8"}
_KERNEL_CASES = {}


def kernel_case(B, F, D, ftype, seed=0):
    """A seeded kernel-level case in float64 (made once per shape, never changed): E ~ N(0, s^2) with s^2 = (P D)^(-1/2)
    (the logit, a sum of about P D products of two entries, is then O(1)), matrix weights I + 0.25 N(0,1) (not
    symmetric: a transposed matrix shows), vector and scalar weights N(0,1), g ~ N(0,1), dE_up ~ 0.1 N(0,1); with
    B > 8 the special rows 3: E = 0 (logit and dE exactly 0), 4: g = 0 (dE exactly 0), 5: E x 8.  With the float64
    outputs logit, dE (without dE_up) and dW."""
    key = (B, F, D, ftype, seed)
    if key not in _KERNEL_CASES:
        rnd = _rnd(torch.Generator().manual_seed(14000 + 16 * seed + TYPES.index(ftype)))
        E = rnd(B, F, D, std=(pairs(F) * D) ** -0.25)
        if ftype == "matrix":
            W = (torch.eye(D, dtype=torch.float64) + 0.25 * rnd(pairs(F), D, D)).float().double()
        else:
            W = rnd(*weight_shape(F, D, ftype))
        g, up = rnd(B), rnd(B, F, D, std=0.1)
        if B > 8:
            E[3] = 0.0
            g[4] = 0.0
            E[5] *= 8.0
        dE, dW = pair_bwd(E, W, ftype, g)
        _KERNEL_CASES[key] = dict(B=B, F=F, D=D, ftype=ftype, E=E, W=W, g=g, dE_up=up,
                                  logit=pair_logit(E, W, ftype), dE=dE, dW=dW)
    return _KERNEL_CASES[key]


def logit_error(got, want):
    """max |got - want| / max(1, |want|): the forward's measure."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float(((got - want).abs() / want.abs().clamp(min=1.0)).max()) if got.numel() else 0.0


def f32_errors(case):
    """The float32 CPU restatement's own errors on a kernel case, every pair summed on its own: (logit_error,
    measure of dE, measure of dW)."""
    E, W, g = (case[n].float() for n in ("E", "W", "g"))
    dE, dW = pair_bwd(E, W, case["ftype"], g)
    return (logit_error(pair_logit(E, W, case["ftype"]), case["logit"]), grad_measure(dE, case["dE"]),
            grad_measure(dW, case["dW"]))


# ---------------------------------------------------------------------------------------------------- the model
def fmfm_logit(p, spec, idx, dense, hp, training=True, masks=None, manual_weights=None, mv=None, return_pre=False):
    """logit = linear (use_linear) + pair (+ dnn([E | dense]) with a non-empty deep_hidden_units); no bias tables."""
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    logit = pair_logit(E, p["field_pair_w"], hp.get("field_interaction", "matrix")).reshape(-1, 1)
    if hp.get("use_linear", True):
        logit = logit + TL.linear_layer(p, spec, idx, dense, manual_weights, mv)
    n = len(hp.get("deep_hidden_units") or ())
    pres = []
    if n:
        keep = hp.get("deep_dropout") or [1] * (n + 1)
        keep = list(keep) if training else [1] * (n + 1)
        dm = (masks or {}).get("dnn")
        x = TL.dnn_input(E, dense)
        logit = logit + TL.dnn(p, x, n, hp.get("deep_activation", "relu"), keep, dm)
        if return_pre:
            dm = dm or [None] * (n + 1)
            y = TL.dropout(x, keep[0], dm[0])
            for i in range(n):
                pres.append(y @ p[f"dnn_layer_{i}_weights"] + p[f"dnn_layer_{i}_bias"])
                y = TL.dropout(torch.relu(pres[-1]), keep[i + 1], dm[i + 1])
    return (logit, pres) if return_pre else logit


def interaction_l2(p, l2_reg):
    return l2_reg * 0.5 * p["field_pair_w"].square().sum()


def fmfm_l2(p, spec, hp):
    out = TL.embedding_l2(p, spec, hp.get("embedding_l2_reg", 0.0))
    if hp.get("use_linear", True):
        out = out + TL.linear_l2(p, hp.get("linear_l2_reg", 0.0))
    n = len(hp.get("deep_hidden_units") or ())
    if n:
        out = out + TL.dnn_l2(p, n, hp.get("deep_l2_reg", 0.0))
    return out + interaction_l2(p, hp.get("interaction_l2_reg", 0.0))


def model_loss(p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None):
    logit = fmfm_logit(p, spec, idx, dense, hp, True, masks, mv=mv)
    pred = TL.prediction(logit, task)
    return TL.create_loss(y, pred, task) + fmfm_l2(p, spec, hp), logit, pred


def fwd_bwd(p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None):
    """One forward+backward: (loss, logit [B], pred [B], grads) - the twin of oracle.th_layers.fwd_bwd."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    loss, logit, pred = model_loss(leaves, spec, idx, dense, y, hp, task, masks, mv)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return loss.detach(), logit.detach().reshape(-1), pred.detach(), grads


_MODEL_CASES = {}


def make_case(ftype, hidden, B, F, D, Dn, seed=0, use_linear=True, l2=1e-4):
    """A seeded model-level case in float64 (made once, never changed): spec, p (the variable names of the contract),
    idx, dense, y, hp.  Embeddings ~ N(0, 0.15^2), dense ~ N(0,1), field_pair_w its initial value + 0.25 N(0,1) (so that
    it is neither plain FM nor symmetric); `min_abs_pre` is the distance of the closest DNN unit to its kink (inf
    without a DNN).  The first stream whose min_abs_pre is at least KINK is taken."""
    key = (ftype, tuple(hidden), B, F, D, Dn, seed, use_linear, l2)
    if key in _MODEL_CASES:
        return _MODEL_CASES[key]
    sizes = [7, 11, 5, 13, 3, 17, 4, 9, 6, 8][:F] if F <= 10 else [5 + (i * 7) % 23 for i in range(F)]
    spec = TL.Spec([f"C{i}" for i in range(F)], sizes, [f"I{j}" for j in range(Dn)])
    n = len(hidden)
    hp = dict(embedding_size=D, embedding_l2_reg=l2, linear_l2_reg=l2, deep_hidden_units=tuple(hidden),
              deep_dropout=(1,) * (n + 1), deep_l2_reg=l2 if n else 0.0, interaction_l2_reg=l2,
              field_interaction=ftype, use_linear=use_linear, deep_activation="relu")
    for attempt in range(64):
        g = torch.Generator().manual_seed(15000 + 64 * seed + attempt)
        rnd = _rnd(g)
        p = {}
        for name, V in zip(spec.sparse_names, sizes):
            p[f"{name}_feat_embed"] = rnd(V, D, std=0.15)
        p["linear_w"] = rnd(spec.lin_layout[2], 1, std=0.1)
        p["linear_w0"] = rnd(1, std=0.1)
        dims = [F * D + Dn] + list(hidden)
        for i in range(n):
            p[f"dnn_layer_{i}_weights"] = glorot(rnd, (dims[i], dims[i + 1]), dims[i], dims[i + 1])
            p[f"dnn_layer_{i}_bias"] = rnd(dims[i + 1], std=0.1)
        if n:
            p["dnn_w"] = glorot(rnd, (dims[-1], 1), dims[-1], 1)
            p["dnn_w0"] = rnd(1, std=0.1)
        p["field_pair_w"] = (init_weights(F, D, ftype) + 0.25 * rnd(*weight_shape(F, D, ftype))).float().double()
        idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in sizes], 1)
        dense = rnd(B, Dn)
        y = (torch.rand(B, generator=g) < 0.3).long()
        pres = fmfm_logit(p, spec, idx, dense, hp, return_pre=True)[1]
        min_abs_pre = min([float(t.abs().min()) for t in pres] + [float("inf")])
        if min_abs_pre >= KINK:
            break
    else:
        raise AssertionError("no stream met the case conditions")
    out = dict(spec=spec, p=p, idx=idx, dense=dense, y=y, hp=hp, min_abs_pre=min_abs_pre)
    _MODEL_CASES[key] = out
    return out


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
