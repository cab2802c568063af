"""CPU PyTorch restatement (dtype-generic) of FiBiNET's interaction and of the model.

TEST INFRASTRUCTURE.  Nothing in the reference implements the model, so the arithmetic is the paper's (arXiv 1905.09433)
as the project's contract states it.  Per example, E [F,D], R = max(1, F // reduction_ratio), P = F(F-1)/2:

    z_f = (1/D) sum_d E[f,d]    s = relu(z W1)    a = relu(s W2)    V[f] = a_f E[f]         (W1 [F,R], W2 [R,F], no biases)
    pairs p = (i, j), 0 <= i < j < F, in itertools.combinations order
    bilinear(Y, W)[p, d] = (sum_k Y[i,k] W_(i)[k,d]) Y[j,d];  "all": W_(i) = W[0] (W [1,D,D]);  "each": W_(i) = W[i] (W [F-1,D,D])
    X = [ bilinear(E, bilinear_w) | bilinear(V, senet_bilinear_w) ]        width 2 P D, pair-major, d fastest
    logit = DNN([X | dense]) (+ linear with use_linear)

    backward (relu'(0) = 0), per branch:  dU_i[d] = sum_{j>i} dX[p,d] Y[j,d]   dY_j[d] += sum_{i<j} dX[p,d] U_i[d]
        dY_i += dU_i W_(i)^T   dW_(i) += Y_i^T dU_i;  V branch: dE_f += a_f dV_f, da_f = <dV_f, E_f>, back through the two
        relus, W2 and W1, dE[f,d] += dz_f / D

Everything but the interaction is composed from the public functions of oracle.th_layers, imported and not modified.
tests/test_fibinet_host.py pins this file without a GPU; the GPU tests compare the HIP kernels and the engine against it
in float64.
"""
from functools import partial

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK, glorot, grad_measure, pair_fields, pairs, to_f32  # noqa: F401  (its interface)
from tests.ref_common import rnd_stream as _rnd  # noqa: F401  (tests/test_gpu_fibinet_model.py draws with it)

# kernel-level GPU cases (B, F, D, R, type) of tests/test_gpu_fibinet.py (the grid-stride case is built there)
GPU_CASES = [(5, 2, 8, 1, "each"), (33, 3, 8, 1, "all"), (37, 5, 8, 2, "each"), (130, 26, 16, 8, "each"),
             (130, 26, 16, 8, "all"), (65, 10, 32, 3, "each"), (9, 40, 32, 13, "each"), (257, 26, 16, 8, "all"),
             (6, 27, 16, 20, "each")]  # (the last: the backward with the weights in LDS and the accumulators not)
# model-level cases (B, F, D, Dn, reduction_ratio, type)
MODEL_CASES = {
    "each_d8": (33, 5, 8, 3, 3, "each"),
    "all_no_dense": (257, 5, 8, 0, 2, "all"),
    "criteo_like": (130, 26, 16, 13, 3, "each"),
}
TOL_X, TOL_GRAD = 1e-5, 2e-5  # |X - X64| <= TOL_X max(1, |X64|); the project's gradient measure on gradients
PARAMS = ("senet_w1", "senet_w2", "bilinear_w", "senet_bilinear_w")
WRONG = ("sum_squeeze", "each_by_right", "no_second_relu", "branches_swapped", "v_uses_bilinear_w")


def reduction(F, ratio):
    return max(1, F // ratio)


def n_matrices(F, btype):
    return F - 1 if btype == "each" else 1


def one_pair_one_unit(F, R):
    """F = 2 with R = 1: both gates carry the sign of their senet_w2 entry wherever s > 0, so either both are open in
    every example or the only pair of the V branch is identically 0.  The cases take the first: no gate is ever closed
    by the second relu there."""
    return F == 2 and R == 1


def wrong_applies(wrong, F, R, btype):
    """Whether a deliberately wrong variant differs from the contract at all on this shape: indexing "each" by the
    right field is the contract itself with one shared matrix ("all") and with a single pair (F = 2); the second relu
    has nothing to close at F = 2, R = 1 (one_pair_one_unit)."""
    if wrong == "each_by_right":
        return btype == "each" and F >= 3
    if wrong == "no_second_relu":
        return not one_pair_one_unit(F, R)
    return True


def gate(E, W1, W2, wrong=None):
    """-> (z [B,F], hs [B,R], s, ha [B,F], a): the squeeze, both pre-activations and both relus."""
    z = E.sum(dim=2) if wrong == "sum_squeeze" else E.mean(dim=2)
    hs = z @ W1
    s = torch.relu(hs)
    ha = s @ W2
    a = ha if wrong == "no_second_relu" else torch.relu(ha)
    return z, hs, s, ha, a


def _pair_matrices(W, F, btype, by_right=False):
    """[P,D,D]: the matrix of every pair."""
    li, lj = pair_fields(F)
    if btype == "all":
        return W[0].expand(li.numel(), -1, -1)
    return W[lj - 1] if by_right else W[li]


def bilinear(Y, W, btype, wrong=None):
    """Y [B,F,D], W [1 | F-1, D, D] -> [B, P D]."""
    B, F, D = Y.shape
    li, lj = pair_fields(F)
    Wp = _pair_matrices(W, F, btype, by_right=wrong == "each_by_right")
    left = torch.einsum("bpk,pkd->bpd", Y[:, li], Wp)
    return (left * Y[:, lj]).reshape(B, -1)


def interact(E, W1, W2, Wb, Wsb, btype, wrong=None):
    """E [B,F,D] -> X [B, 2 P D].  wrong: one of WRONG, the deliberately wrong restatements that
    tests/test_fibinet_host.py shows the tolerances to catch."""
    a = gate(E, W1, W2, wrong)[4]
    V = a.unsqueeze(2) * E
    xe = bilinear(E, Wb, btype, wrong)
    xv = bilinear(V, Wb if wrong == "v_uses_bilinear_w" else Wsb, btype, wrong)
    return torch.cat([xv, xe] if wrong == "branches_swapped" else [xe, xv], dim=1)


def interact_loops(E, W1, W2, Wb, Wsb, btype):
    """interact as explicit Python loops over floats (no tensor arithmetic)."""
    El, W1l, W2l, Wbl, Wsbl = E.tolist(), W1.tolist(), W2.tolist(), Wb.tolist(), Wsb.tolist()
    F, D, R = len(El[0]), len(El[0][0]), len(W2l)
    out = []
    for e in El:
        z = [sum(e[f]) / D for f in range(F)]
        s = [max(0.0, sum(z[f] * W1l[f][r] for f in range(F))) for r in range(R)]
        a = [max(0.0, sum(s[r] * W2l[r][f] for r in range(R))) for f in range(F)]
        v = [[a[f] * e[f][d] for d in range(D)] for f in range(F)]
        row = []
        for y, W in ((e, Wbl), (v, Wsbl)):
            for i in range(F):
                M = W[i] if btype == "each" and i < F - 1 else W[0]
                u = [sum(y[i][k] * M[k][d] for k in range(D)) for d in range(D)]
                for j in range(i + 1, F):
                    row += [u[d] * y[j][d] for d in range(D)]
        out.append(row)
    return torch.tensor(out, dtype=E.dtype).reshape(len(El), -1)


def _bilinear_bwd(Y, W, btype, dXb):
    """One branch, written out: dXb [B,P,D] -> (dY [B,F,D], dW like W)."""
    B, F, D = Y.shape
    li, lj = pair_fields(F)
    Wp = _pair_matrices(W, F, btype)
    left = torch.einsum("bpk,pkd->bpd", Y[:, li], Wp)   # U_i of every pair
    dleft = dXb * Y[:, lj]                               # the pair's addend to dU_i
    dY = torch.zeros_like(Y)
    dY.index_add_(1, lj, dXb * left)
    dY.index_add_(1, li, torch.einsum("bpd,pkd->bpk", dleft, Wp))
    dWp = torch.einsum("bpk,bpd->pkd", Y[:, li], dleft)
    if btype == "all":
        return dY, dWp.sum(dim=0, keepdim=True)
    return dY, torch.zeros_like(W).index_add_(0, li, dWp)


def interact_bwd(E, W1, W2, Wb, Wsb, btype, dX):
    """The backward of the contract, written out (no autograd): -> (dE, dW1, dW2, dWb, dWsb)."""
    B, F, D = E.shape
    P = pairs(F)
    z, hs, s, ha, a = gate(E, W1, W2)
    V = a.unsqueeze(2) * E
    dYe, dWb = _bilinear_bwd(E, Wb, btype, dX[:, : P * D].reshape(B, P, D))
    dV, dWsb = _bilinear_bwd(V, Wsb, btype, dX[:, P * D: 2 * P * D].reshape(B, P, D))
    dE = dYe + a.unsqueeze(2) * dV
    dha = (dV * E).sum(dim=2) * (ha > 0).to(E.dtype)
    dW2 = s.t() @ dha
    dhs = (dha @ W2.t()) * (hs > 0).to(E.dtype)
    dW1 = z.t() @ dhs
    dE = dE + (dhs @ W1.t()).unsqueeze(2) / D
    return dE, dW1, dW2, dWb, dWsb


def gate_conditions(E, W1, W2):
    """(the smallest |pre-activation| of the gate, the share of gates a > 0, the most negative pre-activation of a) in
    float64.  The z W1 entries of an example whose rows are all zero and the s W2 entries of an example whose s is
    identically 0 are exact zeros in every precision (relu'(0) = 0 on both sides): they are left out of the minimum."""
    z, hs, s, ha, a = gate(E, W1, W2)
    live_e = E.abs().amax(dim=(1, 2)) > 0
    live_s = s.abs().amax(dim=1) > 0
    vals = [hs[live_e].abs().reshape(-1), ha[live_s].abs().reshape(-1)]
    vals = torch.cat([v for v in vals if v.numel()]) if any(v.numel() for v in vals) else torch.ones(1)
    return float(vals.min()), float((a > 0).double().mean()), float(ha.min())


SPECIAL_ROWS = {3: "E = 0", 4: "dX = 0", 5: "E x 8"}


@C.memo
def kernel_case(B, F, D, R, btype, seed=0):
    """A seeded kernel-level case in float64 (made once per shape, never changed): E ~ N(0,1), W1 and W2 ~ 2 glorot,
    the bilinear weights ~ N(0, 1/D), dX ~ N(0,1); with B > 8 the special rows 3: E = 0 (X and dE exactly 0),
    4: dX = 0 (dE exactly 0), 5: E x 8.  The first stream that meets the case conditions is taken: every gate
    pre-activation at least KINK from 0, a gate open and a gate closed by the second relu (none closed at F = 2,
    R = 1), and with B >= 33 a share of open gates in [0.2, 0.8]; tests/test_fibinet_host.py asserts them.  With the
    float64 outputs X, dE and the four parameter gradients."""
    nW, W = n_matrices(F, btype), 2 * pairs(F) * D

    def build(g, rnd):
        E, dX = rnd(B, F, D), rnd(B, W)
        W1, W2 = 2.0 * glorot(rnd, (F, R), F, R), 2.0 * glorot(rnd, (R, F), R, F)
        Wb, Wsb = rnd(nW, D, D, std=D ** -0.5), rnd(nW, D, D, std=D ** -0.5)
        if B > 8:
            E[3] = 0.0
            dX[4] = 0.0
            E[5] *= 8.0
        return E, dX, W1, W2, Wb, Wsb

    def ok(drawn):
        dist, share, most_negative = gate_conditions(drawn[0], drawn[2], drawn[3])
        # (some gate open and some closed by its relu, or the second relu would have nothing to do)
        closed = most_negative >= 0 if one_pair_one_unit(F, R) else most_negative < 0
        return dist >= KINK and share > 0 and closed and (B < 33 or 0.2 <= share <= 0.8)

    E, dX, W1, W2, Wb, Wsb = C.first_stream(11000 + 64 * seed, build, ok)[0]
    dE, dW1, dW2, dWb, dWsb = interact_bwd(E, W1, W2, Wb, Wsb, btype, dX)
    return dict(B=B, F=F, D=D, R=R, btype=btype, E=E, dX=dX, senet_w1=W1, senet_w2=W2, bilinear_w=Wb,
                senet_bilinear_w=Wsb, X=interact(E, W1, W2, Wb, Wsb, btype), dE=dE,
                d_senet_w1=dW1, d_senet_w2=dW2, d_bilinear_w=dWb, d_senet_bilinear_w=dWsb)


def case_weights(case, dtype=torch.float64):
    return tuple(case[n].to(dtype) for n in PARAMS)


x_error = C.rel_error


def f32_errors(case):
    """The float32 CPU restatement's own errors on a kernel case: (x_error of X, measure dE, then the measures of the
    four parameter gradients in PARAMS order)."""
    ws = case_weights(case, torch.float32)
    X = interact(case["E"].float(), *ws, case["btype"])
    got = interact_bwd(case["E"].float(), *ws, case["btype"], case["dX"].float())
    return (x_error(X, case["X"]), grad_measure(got[0], case["dE"])) + tuple(
        grad_measure(g, case["d_" + n]) for g, n in zip(got[1:], PARAMS))


# ---------------------------------------------------------------------------------------------------- the model
def fibinet_x(p, E, hp, wrong=None):
    return interact(E, p["senet_w1"], p["senet_w2"], p["bilinear_w"], p["senet_bilinear_w"],
                    hp.get("bilinear_type", "each"), wrong)


def fibinet_logit(p, spec, idx, dense, hp, training=True, masks=None, manual_weights=None, mv=None, return_pre=False):
    """logit = DNN([X | dense]) (+ linear with use_linear); no bias tables."""
    masks = masks or {}
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    x = fibinet_x(p, E, hp)
    if dense is not None and dense.shape[1]:
        x = torch.cat([x, dense], dim=1)
    n = len(hp["deep_hidden_units"])
    keep = C.dnn_keep(hp, n, training)
    logit = TL.dnn(p, x, n, hp.get("deep_activation", "relu"), keep, masks.get("dnn"))
    if hp.get("use_linear", True):
        logit = logit + TL.linear_layer(p, spec, idx, dense, manual_weights, mv)
    if return_pre:
        z, hs, s, ha, a = gate(E, p["senet_w1"], p["senet_w2"])
        return logit, [hs, ha[s.abs().amax(dim=1) > 0]] + C.dnn_pres(p, x, n, keep, masks.get("dnn"))
    return logit


interaction_l2 = partial(C.param_l2, PARAMS)  # (p, l2_reg)


def fibinet_l2(p, spec, hp):
    return C.base_l2(p, spec, hp, len(hp["deep_hidden_units"]), hp.get("use_linear", True)) + interaction_l2(
        p, hp.get("interaction_l2_reg", 0.0))


# (p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None) -> (loss, logit [B,1], pred)
model_loss = partial(C.model_loss, fibinet_logit, fibinet_l2)
# ... -> (loss, logit [B], pred [B], grads): one forward+backward, the twin of oracle.th_layers.fwd_bwd
fwd_bwd = partial(C.fwd_bwd, model_loss)


@C.memo
def make_case(B, F, D, Dn, ratio, btype, seed=0, hidden=(32, 32), use_linear=True, l2=1e-4):
    """A seeded model-level case in float64 (made once, never changed): spec, p (the variable names of the contract),
    idx, dense, y, hp.  Embeddings ~ N(0, 0.15^2), dense ~ N(0,1), the gate's matrices ~ 2 glorot, the bilinear ones
    glorot (N(0, 1/D)); `min_abs_pre` is the distance of the closest unit - the gate's and the DNN's - to its kink.  The
    first stream whose min_abs_pre is at least KINK is taken."""
    spec, sizes = C.plain_spec(F, Dn)
    R, nW = reduction(F, ratio), n_matrices(F, btype)
    hp = dict(embedding_size=D, embedding_l2_reg=l2, linear_l2_reg=l2, deep_hidden_units=tuple(hidden),
              deep_dropout=(1,) * (len(hidden) + 1), deep_l2_reg=l2, interaction_l2_reg=l2, bilinear_type=btype,
              reduction_ratio=ratio, use_linear=use_linear)

    def build(g, rnd):
        p = C.draw_front(rnd, spec, D, std=0.15)
        C.draw_dnn(rnd, p, [2 * pairs(F) * D + Dn] + list(hidden))
        p["senet_w1"] = 2.0 * glorot(rnd, (F, R), F, R)
        p["senet_w2"] = 2.0 * glorot(rnd, (R, F), R, F)
        p["bilinear_w"] = glorot(rnd, (nW, D, D), D, D)
        p["senet_bilinear_w"] = glorot(rnd, (nW, D, D), D, D)
        idx, dense, y = C.draw_batch(g, rnd, sizes, B, Dn)
        min_abs_pre = C.min_abs(fibinet_logit(p, spec, idx, dense, hp, return_pre=True)[1])
        return dict(spec=spec, p=p, idx=idx, dense=dense, y=y, hp=hp, min_abs_pre=min_abs_pre)

    return C.first_stream(12000 + 64 * seed, build, lambda k: k["min_abs_pre"] >= KINK)[0]
