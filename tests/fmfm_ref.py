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
from functools import partial

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK, glorot, grad_measure, pair_fields, pairs, to_f32  # noqa: F401  (its interface)

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
WRONG = ("transposed", "with_diagonal", "both_orders", "matrix_by_left_field")


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


SPECIAL_ROWS = {3: "E = 0", 4: "g = 0", 5: "E x 8"}


@C.memo
def kernel_case(B, F, D, ftype, seed=0):
    """A seeded kernel-level case in float64 (made once per shape, never changed): E ~ N(0, s^2) with s^2 = (P D)^(-1/2)
    (the logit, a sum of about P D products of two entries, is then O(1)), matrix weights I + 0.25 N(0,1) (not
    symmetric: a transposed matrix shows), vector and scalar weights N(0,1), g ~ N(0,1), dE_up ~ 0.1 N(0,1); with
    B > 8 the special rows 3: E = 0 (logit and dE exactly 0), 4: g = 0 (dE exactly 0), 5: E x 8.  With the float64
    outputs logit, dE (without dE_up) and dW."""
    rnd = C.rnd_stream(torch.Generator().manual_seed(14000 + 16 * seed + TYPES.index(ftype)))
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
    return dict(B=B, F=F, D=D, ftype=ftype, E=E, W=W, g=g, dE_up=up, logit=pair_logit(E, W, ftype), dE=dE, dW=dW)


logit_error = C.rel_error


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
        keep, dm = C.dnn_keep(hp, n, training), (masks or {}).get("dnn")
        x = TL.dnn_input(E, dense)
        logit = logit + TL.dnn(p, x, n, hp.get("deep_activation", "relu"), keep, dm)
        if return_pre:
            pres = C.dnn_pres(p, x, n, keep, dm)
    return (logit, pres) if return_pre else logit


interaction_l2 = partial(C.param_l2, ("field_pair_w",))  # (p, l2_reg)


def fmfm_l2(p, spec, hp):
    n = len(hp.get("deep_hidden_units") or ())
    return C.base_l2(p, spec, hp, n or None, hp.get("use_linear", True)) + interaction_l2(
        p, hp.get("interaction_l2_reg", 0.0))


# (p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None) -> (loss, logit [B,1], pred)
model_loss = partial(C.model_loss, fmfm_logit, fmfm_l2)
# ... -> (loss, logit [B], pred [B], grads): one forward+backward, the twin of oracle.th_layers.fwd_bwd
fwd_bwd = partial(C.fwd_bwd, model_loss)


@C.memo
def make_case(ftype, hidden, B, F, D, Dn, seed=0, use_linear=True, l2=1e-4):
    """A seeded model-level case in float64 (made once, never changed): spec, p (the variable names of the contract),
    idx, dense, y, hp.  Embeddings ~ N(0, 0.15^2), dense ~ N(0,1), field_pair_w its initial value + 0.25 N(0,1) (so that
    it is neither plain FM nor symmetric); `min_abs_pre` is the distance of the closest DNN unit to its kink (inf
    without a DNN).  The first stream whose min_abs_pre is at least KINK is taken."""
    spec, sizes = C.plain_spec(F, Dn)
    n = len(hidden)
    hp = dict(embedding_size=D, embedding_l2_reg=l2, linear_l2_reg=l2, deep_hidden_units=tuple(hidden),
              deep_dropout=(1,) * (n + 1), deep_l2_reg=l2 if n else 0.0, interaction_l2_reg=l2,
              field_interaction=ftype, use_linear=use_linear, deep_activation="relu")

    def build(g, rnd):
        p = C.draw_front(rnd, spec, D, std=0.15)
        C.draw_dnn(rnd, p, [F * D + Dn] + list(hidden), head=n > 0)
        p["field_pair_w"] = (init_weights(F, D, ftype) + 0.25 * rnd(*weight_shape(F, D, ftype))).float().double()
        idx, dense, y = C.draw_batch(g, rnd, sizes, B, Dn)
        min_abs_pre = C.min_abs(fmfm_logit(p, spec, idx, dense, hp, return_pre=True)[1])
        return dict(spec=spec, p=p, idx=idx, dense=dense, y=y, hp=hp, min_abs_pre=min_abs_pre)

    return C.first_stream(15000 + 64 * seed, build, lambda k: k["min_abs_pre"] >= KINK)[0]
