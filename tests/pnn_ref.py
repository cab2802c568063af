"""CPU PyTorch restatement (dtype-generic) of the product layer of the Product-based Neural Network (PNN,
arXiv 1611.00144) in its kernel form, and of the model built on it.

TEST INFRASTRUCTURE.  Nothing in the reference implements PNN, so the arithmetic is the kernel-form product layer of
the widely used open-source PNN (use_inner, use_outter, kernel_type mat / vec / num) as the project's contract states
it - not the paper's sum-pooled outer-product shortcut.  Per example, E [F,D], P = F(F-1)/2 pairs p = (i, j),
0 <= i < j < F, in itertools.combinations order:

    inner[p] = <E_i, E_j>
    outer[p] = E_i K_(p) E_j^T   "mat": K_(p) = K[p]        product_kernel [P,D,D]  (the LEFT field i on the rows)
                                 "vec": K_(p) = diag(K[p])  product_kernel [P,D]
                                 "num": K_(p) = K[p] I      product_kernel [P]
    X = [ E flattened (F D columns) | inner (P, with INNER) | outer (P, with OUTER) ]
    logit = DNN([X | dense]) (+ linear with use_linear)

    backward, G_in / G_out = the product column blocks of dX:
      dE_i += G_in[p] E_j + G_out[p] K_(p) E_j    dE_j += G_in[p] E_i + G_out[p] K_(p)^T E_i
      d_rows = dX[:, 0:FD] + dE                   dK[p] = sum_b G_out[b,p] E_bi (x) E_bj (vec: its diagonal; num: trace)

`products` is the bit set INNER = 1 | OUTER = 2.  The per-pair terms and the pair order are those of tests/fmfm_ref.py
(imported, not modified); everything but the product layer is composed from the public functions
of oracle.th_layers.  tests/test_pnn_host.py pins this file without a GPU; the GPU tests compare the HIP kernels and
the engine against it in float64.
"""
import itertools
from functools import partial

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.fmfm_ref import pair_terms
from tests.ref_common import KINK, glorot, grad_measure, pair_fields, pairs, to_f32  # noqa: F401  (its interface)

INNER, OUTER = 1, 2
KERNELS = ("mat", "vec", "num")
_FTYPE = {"mat": "matrix", "vec": "vector", "num": "scalar"}  # fmfm_ref's names of the same three weight forms
# the product selections every kernel-level shape runs: inner only, outer only for each kernel type, inner + mat
COMBOS = [(INNER, "mat"), (OUTER, "mat"), (OUTER, "vec"), (OUTER, "num"), (INNER | OUTER, "mat")]
# both products with the vector-ALU kernel types: G_in behind G_out in the dE kernel's LDS (read from dX at F = 40, D = 32)
EXTRA_COMBOS = [(INNER | OUTER, "vec"), (INNER | OUTER, "num")]
EXTRA_CASES = [(37, 5, 8), (9, 40, 32)]
# kernel-level GPU cases (B, F, D) of tests/test_gpu_pnn.py (the grid-stride cases are built there): one pair; an odd
# pair count at D = 8 (a lone last pair in the two-pairs-per-MFMA packing); B no multiple of 16 or of the tile; several
# tiles; F at the limit (with both products: G_in read from dX); every supported D
GPU_CASES = [(5, 2, 8), (33, 3, 8), (37, 5, 8), (130, 26, 16), (65, 10, 32), (9, 40, 32), (6, 27, 16)]
LDX_PADS = (0, 3)
# model-level cases: (products, kernel_type, use_linear, hidden, B, F, D, Dn)
MODEL_CASES = {
    "inner_only": (INNER, "mat", False, (16, 16), 33, 5, 8, 3),
    "outer_vec_linear": (OUTER, "vec", True, (16, 16), 257, 5, 8, 0),
    "inner_mat_criteo_like": (INNER | OUTER, "mat", False, (32, 32), 130, 26, 16, 13),
}
TOL_X, TOL_GRAD = 1e-5, 2e-5  # |X - X64| <= TOL_X max(1, |X64|) per element; the project's gradient measure
WRONG = ("transposed", "j_major", "blocks_swapped", "with_diagonal", "matrix_by_left_field")


def n_products(products):
    return bin(products).count("1")


def width(F, D, products):
    return F * D + n_products(products) * pairs(F)


def weight_shape(F, D, kernel_type):
    return {"mat": (pairs(F), D, D), "vec": (pairs(F), D), "num": (pairs(F),)}[kernel_type]


def wrong_applies(wrong, F, products, kernel_type):
    """Whether a deliberately wrong variant differs from the contract at all."""
    outer = bool(products & OUTER)
    if wrong == "transposed":  # (a transposed diagonal matrix is itself; the inner product is symmetric)
        return outer and kernel_type == "mat"
    if wrong == "j_major":  # (up to F = 3 both orders are (0,1), (0,2), (1,2))
        return F >= 4
    if wrong == "blocks_swapped":
        return products == (INNER | OUTER)
    if wrong == "matrix_by_left_field":  # (the contract itself while every left field leads one pair)
        return outer and F >= 3
    return True


def _wrong_pair_fields(F, wrong):
    if wrong == "j_major":  # pairs ordered by the right field first
        order = sorted(itertools.combinations(range(F), 2), key=lambda ij: (ij[1], ij[0]))
    else:  # "with_diagonal": the enumeration runs over i <= j; its first P entries
        order = list(itertools.combinations_with_replacement(range(F), 2))[: pairs(F)]
    li, lj = zip(*order)
    return torch.tensor(li), torch.tensor(lj)


def _terms(E, K, ftype, wrong):
    """[B,P] pair terms E_i K_(p) E_j^T; with a wrong pair enumeration pair p reads the wrong fields."""
    if wrong in ("j_major", "with_diagonal"):
        B, F, D = E.shape
        li, lj = _wrong_pair_fields(F, wrong)
        if ftype == "matrix":
            return (torch.einsum("bpk,pkd->bpd", E[:, li], K) * E[:, lj]).sum(dim=2)
        w = K if ftype == "vector" else K.unsqueeze(1)
        return (E[:, li] * w * E[:, lj]).sum(dim=2)
    return pair_terms(E, K, ftype, wrong if wrong in ("transposed", "matrix_by_left_field") else None)


def product_layer(E, K, products, kernel_type, wrong=None):
    """E [B,F,D], product_kernel (None without OUTER) -> X [B, F D + n P].  wrong: one of WRONG, the deliberately
    wrong restatements that tests/test_pnn_host.py shows the tolerances to catch."""
    B, F, D = E.shape
    blocks = []
    if products & INNER:
        blocks.append(_terms(E, torch.ones(pairs(F), dtype=E.dtype), "scalar", wrong))
    if products & OUTER:
        blocks.append(_terms(E, K, _FTYPE[kernel_type], wrong))
    if wrong == "blocks_swapped":
        blocks = blocks[::-1]
    return torch.cat([E.reshape(B, F * D)] + blocks, dim=1)


def product_layer_loops(E, K, products, kernel_type):
    """product_layer as explicit Python loops over floats (no tensor arithmetic)."""
    El = E.tolist()
    Kl = K.tolist() if K is not None else None
    F, D = len(El[0]), len(El[0][0])
    out = []
    for e in El:
        row = [v for f in range(F) for v in e[f]]
        inner, outer, p = [], [], 0
        for i in range(F):
            for j in range(i + 1, F):
                inner.append(sum(e[i][d] * e[j][d] for d in range(D)))
                if products & OUTER:
                    if kernel_type == "mat":
                        outer.append(sum(e[i][k] * Kl[p][k][d] * e[j][d] for k in range(D) for d in range(D)))
                    elif kernel_type == "vec":
                        outer.append(sum(e[i][d] * Kl[p][d] * e[j][d] for d in range(D)))
                    else:
                        outer.append(Kl[p] * sum(e[i][d] * e[j][d] for d in range(D)))
                p += 1
        out.append(row + (inner if products & INNER else []) + outer)
    return torch.tensor(out, dtype=E.dtype)


def product_bwd(E, K, products, kernel_type, dX):
    """The backward of the contract, written out (no autograd): dX [B, W] -> (d_rows [B,F,D], dK like K or None)."""
    B, F, D = E.shape
    P, FD = pairs(F), F * D
    li, lj = pair_fields(F)
    Ei, Ej = E[:, li], E[:, lj]
    d_rows = dX[:, :FD].reshape(B, F, D).clone()
    col = FD
    if products & INNER:
        g = dX[:, col:col + P].unsqueeze(2)
        d_rows.index_add_(1, li, g * Ej)
        d_rows.index_add_(1, lj, g * Ei)
        col += P
    if not products & OUTER:
        return d_rows, None
    G = dX[:, col:col + P]
    g = G.unsqueeze(2)
    if kernel_type == "mat":
        d_rows.index_add_(1, li, g * torch.einsum("pkd,bpd->bpk", K, Ej))
        d_rows.index_add_(1, lj, g * torch.einsum("bpk,pkd->bpd", Ei, K))
        return d_rows, torch.einsum("bp,bpk,bpd->pkd", G, Ei, Ej)
    w = K if kernel_type == "vec" else K.unsqueeze(1)
    d_rows.index_add_(1, li, g * w * Ej)
    d_rows.index_add_(1, lj, g * w * Ei)
    dk = torch.einsum("bp,bpd->pd", G, Ei * Ej)
    return d_rows, dk if kernel_type == "vec" else dk.sum(dim=1)


SPECIAL_ROWS = {3: "E = 0", 4: "dX = 0", 5: "E x 8"}
MAX_STREAMS = 128  # draws kernel_case may try for one case


def _draw_kernel_case(B, F, D, products, kernel_type, stream):
    gen = torch.Generator().manual_seed(16000 + 64 * stream + 8 * products + KERNELS.index(kernel_type))
    rnd = C.rnd_stream(gen)
    E = rnd(B, F, D, std=D ** -0.25)
    K = None
    if products & OUTER:
        if kernel_type == "mat":
            K = (torch.eye(D, dtype=torch.float64) + 0.25 * rnd(pairs(F), D, D)).float().double()
        else:
            K = rnd(*weight_shape(F, D, kernel_type))
    W = width(F, D, products)
    dX = rnd(B, W)
    if B > 8:
        E[3] = 0.0
        dX[4] = 0.0
        E[5] *= 8.0
    d_rows, dK = product_bwd(E, K, products, kernel_type, dX)
    return dict(B=B, F=F, D=D, products=products, kernel_type=kernel_type, W=W, E=E, K=K, dX=dX, stream=stream,
                X=product_layer(E, K, products, kernel_type), d_rows=d_rows, dK=dK)


def kernel_case(B, F, D, products, kernel_type, ldx_pad=0, seed=0):
    """A seeded kernel-level case in float64 (made once per key, never changed): E ~ N(0, s^2) with s^2 = D^(-1/2) (a
    product, a sum of D products of two entries, is then O(1)), mat kernels I + 0.25 N(0,1) (not symmetric: a
    transposed matrix shows), vec and num kernels N(0,1), dX ~ N(0,1) [B, W]; with B > 8 the special rows 3: E = 0 (the
    products are exactly 0 and d_rows is dX's row part), 4: dX = 0 (d_rows exactly 0), 5: E x 8.  ldx = W + ldx_pad is
    the row stride the GPU tests give X and dX (the pad columns hold no data of the case: both strides share it).  With
    the float64 outputs X, d_rows and dK (None without OUTER).

    A condition on the case: the float32 CPU restatement must itself stay inside TOL_X and TOL_GRAD.  Where a draw
    fails it the draw changes, nothing else: the first of MAX_STREAMS streams that meets the condition is taken
    (`stream` says which; 0 for all but a few).  It is the E x 8 row that makes this a matter of the draw at the widest
    shapes: a mat product of that row at D = 32 is a sum of 1024 terms of size 20, and the few of the row's P products
    that cancel to below 1 are held to 1e-5 absolute (tests/test_pnn_host.py lists the streams)."""
    case = _kernel_case(B, F, D, products, kernel_type, seed)
    return dict(case, ldx=case["W"] + ldx_pad)


@C.memo
def _kernel_case(B, F, D, products, kernel_type, seed):
    # (its own loop: MAX_STREAMS streams from MAX_STREAMS * seed on, each seeded by _draw_kernel_case)
    for stream in range(MAX_STREAMS * seed, MAX_STREAMS * (seed + 1)):
        case = _draw_kernel_case(B, F, D, products, kernel_type, stream)
        case["f32"] = f32_errors(case)
        if case["f32"][0] <= TOL_X and max(case["f32"][1:]) <= TOL_GRAD:
            return case
    raise AssertionError(f"no stream of {(B, F, D, products, kernel_type)} met the float32 condition")


x_error = C.rel_error


def f32_errors(case):
    """The float32 CPU restatement's own errors on a kernel case: (x_error, measure of d_rows, measure of dK)."""
    E, dX = case["E"].float(), case["dX"].float()
    K = case["K"].float() if case["K"] is not None else None
    d_rows, dK = product_bwd(E, K, case["products"], case["kernel_type"], dX)
    return (x_error(product_layer(E, K, case["products"], case["kernel_type"]), case["X"]),
            grad_measure(d_rows, case["d_rows"]), grad_measure(dK, case["dK"]) if dK is not None else 0.0)


# ---------------------------------------------------------------------------------------------------- the model
def pnn_logit(p, spec, idx, dense, hp, training=True, masks=None, manual_weights=None, mv=None, return_pre=False):
    """logit = dnn([X | dense]) (+ linear with use_linear); no bias tables."""
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    products = (INNER if hp.get("use_inner", True) else 0) | (OUTER if hp.get("use_outer", False) else 0)
    X = product_layer(E, p.get("product_kernel"), products, hp.get("kernel_type", "mat"))
    n = len(hp["deep_hidden_units"])
    keep, dm = C.dnn_keep(hp, n, training), (masks or {}).get("dnn")
    x = TL.dnn_input(X, dense)
    logit = TL.dnn(p, x, n, hp.get("deep_activation", "relu"), keep, dm)
    if hp.get("use_linear", False):
        logit = logit + TL.linear_layer(p, spec, idx, dense, manual_weights, mv)
    return (logit, C.dnn_pres(p, x, n, keep, dm)) if return_pre else logit


interaction_l2 = partial(C.param_l2, ("product_kernel",))  # (p, l2_reg); 0 without the outer product's kernel


def pnn_l2(p, spec, hp):
    return C.base_l2(p, spec, hp, len(hp["deep_hidden_units"]), hp.get("use_linear", False)) + interaction_l2(
        p, hp.get("interaction_l2_reg", 0.0))


# (p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None) -> (loss, logit [B,1], pred)
model_loss = partial(C.model_loss, pnn_logit, pnn_l2)
# ... -> (loss, logit [B], pred [B], grads): one forward+backward, the twin of oracle.th_layers.fwd_bwd
fwd_bwd = partial(C.fwd_bwd, model_loss)


@C.memo
def make_case(products, kernel_type, use_linear, hidden, B, F, D, Dn, seed=0, l2=1e-4):
    """A seeded model-level case in float64 (made once, never changed): spec, p (the variable names of the contract),
    idx, dense, y, hp.  Embeddings ~ N(0, 0.15^2), dense ~ N(0,1), product_kernel glorot (fan D / D) + for "mat" the
    identity (so that the outer products are neither tiny nor symmetric); `min_abs_pre` is the distance of the closest DNN unit to its kink.  The first stream whose min_abs_pre
    is at least KINK is taken."""
    spec, sizes = C.plain_spec(F, Dn)
    n = len(hidden)
    hp = dict(embedding_size=D, embedding_l2_reg=l2, linear_l2_reg=l2, deep_hidden_units=tuple(hidden),
              deep_dropout=(1,) * (n + 1), deep_l2_reg=l2, interaction_l2_reg=l2, use_inner=bool(products & INNER),
              use_outer=bool(products & OUTER), kernel_type=kernel_type, use_linear=use_linear, deep_activation="relu")

    def build(g, rnd):
        p = C.draw_front(rnd, spec, D, std=0.15)
        C.draw_dnn(rnd, p, [width(F, D, products) + Dn] + list(hidden))
        if products & OUTER:
            K = glorot(rnd, weight_shape(F, D, kernel_type), D, D)
            if kernel_type == "mat":
                K = (K + torch.eye(D, dtype=torch.float64)).float().double()
            p["product_kernel"] = K
        idx, dense, y = C.draw_batch(g, rnd, sizes, B, Dn)
        min_abs_pre = C.min_abs(pnn_logit(p, spec, idx, dense, hp, return_pre=True)[1])
        return dict(spec=spec, p=p, idx=idx, dense=dense, y=y, hp=hp, min_abs_pre=min_abs_pre)

    return C.first_stream(17000 + 64 * seed, build, lambda k: k["min_abs_pre"] >= KINK)[0]
