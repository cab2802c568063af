"""CPU PyTorch restatement (dtype-generic) of MaskNet (arXiv 2102.07619) - its two normalise-and-mask kernel families
written out by hand, forward and backward, and the model built on them.

TEST INFRASTRUCTURE.  Nothing in the reference implements MaskNet, so the arithmetic is the paper's as the project's
contract states it.  Per example, E [F,D], x = [flatten(E) | dense] of width K:

    mask(x)  = relu(x Wa + ba) Wp + bp                         Wa [K,A], Wp [A,Wout], A = max(1, round(ratio * Wout))
    V[f,:]   = gamma[f,:] o (E[f,:] - mean_f) / sqrt(var_f + eps) + beta[f,:]     per field row, biased variance,
                                                                                   eps = 1e-5 inside the root
    embedding block: h = relu(LN_H((mask(x) o V) Wh))          Wh [F D, H], LN_H over the H columns (own gamma, beta)
    block on a block: h = relu(LN_H((mask(x) o h_prev) Wh))    Wh [H, H]; h_prev is NOT normalised again
    parallel: DNN([h_1 | .. | h_N | dense]);  serial: DNN([h_N | dense]);  logit = DNN (+ linear if use_linear)

Everything but the blocks is composed from the public functions of oracle.th_layers, imported and not modified.
tests/test_masknet_host.py pins this file without a GPU; the GPU tests compare the HIP kernels and the engine against it
in float64.
"""
from functools import partial

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK, glorot, grad_measure, to_f32  # noqa: F401  (part of this module's interface)
from tests.ref_common import rel_error as logit_error
from tests.ref_common import rnd_stream as _rnd  # noqa: F401  (tests/test_masknet_host.py draws with it)

EPS = 1e-5
TOL_Y, TOL_GRAD = 1e-5, 2e-5  # |Y - Y64| <= TOL_Y max(1, |Y64|); the project's gradient measure
# kernel-level row cases keep every pre-activation 2e-6 away from 0: v = gamma xhat + beta with xhat rounded once from
# float64 (6e-8 relative) and |gamma xhat| < 8 is within 1e-6 of its float64 value
ROW_KINK = 2e-6
# model-level cases keep every relu unit 1e-5 away from 0: a float32 pre-activation is a dot product of up to ~100 terms
# of size ~1, each rounded at 6e-8, behind a LayerNorm that divides by a deviation as small as 0.1 - several 1e-6 off
MODEL_KINK = 1e-5
# the deliberately wrong variants tests/test_masknet_host.py shows the tolerances to catch
WRONG_GROUP = ("flattened", "unbiased", "eps_outside", "mask_first")
WRONG_ROW = ("relu_first", "unbiased", "eps_outside")
# kernel-level GPU cases: group (B, F, D, N), row (B, H), plain (normalize = 0) (B, H)
GROUP_CASES = [(70, 3, 8, 2), (70, 5, 16, 3), (300, 26, 16, 3), (70, 4, 32, 1), (1, 1, 8, 1), (33, 40, 32, 8)]
ROW_CASES = [(70, 8), (70, 100), (300, 256), (33, 2048), (1, 12)]
PLAIN_CASES = [(70, 64), (1, 8)]
# the stream (attempt index) each seeded case settles on - pinned by tests/test_masknet_host.py, so that a change of
# torch's random streams that moves a case to other inputs shows as a failure there
ROW_ATTEMPTS = {(70, 8): 0, (70, 100): 0, (300, 256): 0, (33, 2048): 0, (1, 12): 0}
MODEL_ATTEMPTS = {"parallel3": 3, "parallel1_no_dense": 0, "serial3": 9, "serial1": 0, "serial3_no_dense": 2}
# fixed example indices of the special inputs (cases with B > 8)
EX_ZERO, EX_NO_GRAD, EX_SHIFT, EX_SMALL = 3, 4, 5, 6


# ------------------------------------------------------------------------------------------- LayerNorm by hand
def ln_stats(x, wrong=None):
    """x [.., n] -> (xhat, rstd [.., 1]) over the last dimension."""
    n = x.shape[-1]
    mean = x.mean(dim=-1, keepdim=True)
    c = x - mean
    var = c.square().sum(dim=-1, keepdim=True) / (n - 1 if wrong == "unbiased" else n)
    rstd = 1.0 / (var.sqrt() + EPS) if wrong == "eps_outside" else 1.0 / (var + EPS).sqrt()
    return c * rstd, rstd


def ln_bwd(dxhat, xhat, rstd):
    """The LayerNorm backward through the mean and the variance: dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat o
    xhat)) over the last dimension."""
    return rstd * (dxhat - dxhat.mean(dim=-1, keepdim=True) - xhat * (dxhat * xhat).mean(dim=-1, keepdim=True))


def ln_emb(E, gamma, beta, wrong=None):
    """V [B,F,D]: every field row normalised on its own."""
    if wrong == "flattened":
        B, F, D = E.shape
        xh, _ = ln_stats(E.reshape(B, F * D))
        return gamma * xh.view(B, F, D) + beta
    xh, _ = ln_stats(E, wrong)
    return gamma * xh + beta


def group_fwd(E, gamma, beta, Ms, wrong=None):
    """E [B,F,D], gamma / beta [F,D], Ms: N masks [B,FD] -> [Y_n = M_n o V]."""
    B, F, D = E.shape
    if wrong == "mask_first":
        return [ln_emb(M.view(B, F, D) * E, gamma, beta).reshape(B, F * D) for M in Ms]
    V = ln_emb(E, gamma, beta, wrong).reshape(B, F * D)
    return [M * V for M in Ms]


def group_bwd(E, gamma, beta, Ms, dYs):
    """The backward written out (no autograd) -> (dMs, dE [B,F,D], dgamma, dbeta [F,D])."""
    B, F, D = E.shape
    xh, rstd = ln_stats(E)
    V = (gamma * xh + beta).reshape(B, F * D)
    dMs = [dY * V for dY in dYs]
    dV = sum(dY * M for dY, M in zip(dYs, Ms)).view(B, F, D)
    return dMs, ln_bwd(dV * gamma, xh, rstd), (dV * xh).sum(dim=0), dV.sum(dim=0)


def plain_fwd(X, M):
    """normalize = 0: Y = M o h_prev."""
    return M * X


def plain_bwd(X, M, dY):
    """-> (dM, dX)."""
    return dY * X, dY * M


def row_fwd(Z, gamma, beta, wrong=None, return_pre=False):
    """h = relu(gamma o LN(Z) + beta) over the H columns of a row."""
    if wrong == "relu_first":
        xh, _ = ln_stats(torch.relu(Z))
        return gamma * xh + beta
    xh, _ = ln_stats(Z, wrong)
    pre = gamma * xh + beta
    return (torch.relu(pre), pre) if return_pre else torch.relu(pre)


def row_bwd(Z, gamma, beta, dh):
    """relu'(0) = 0 -> (dZ, dgamma, dbeta [H])."""
    xh, rstd = ln_stats(Z)
    dy = dh * (gamma * xh + beta > 0).to(Z.dtype)
    return ln_bwd(dy * gamma, xh, rstd), (dy * xh).sum(dim=0), dy.sum(dim=0)


# ------------------------------------------------------------------------------------------------ kernel cases
def _special(X, B, scale_small=1e-3):
    """The special examples of a case with B > 8, on X [B, rows, n]: an all-zero example, a row shifted by +50 with a
    spread of 0.05 (its mean far above its spread), a row scaled by 1e-3 (its spread near sqrt(eps))."""
    if B > 8:
        X[EX_ZERO] = 0.0
        X[EX_SHIFT, 0] = (X[EX_SHIFT, 0] * 0.05 + 50.0).float().double()
        X[EX_SMALL, -1] = (X[EX_SMALL, -1] * scale_small).float().double()


@C.memo
def kernel_case(B, F, D, N, seed=0):
    """A seeded group-kernel case in float64 (made once per shape, never changed): E ~ N(0,1), gains 1 + 0.5 N(0,1),
    biases 0.3 N(0,1), masks and upstream gradients N(0,1), dE_up 0.1 N(0,1); with B > 8 example 3 is all zero, example
    4 has zero upstream gradient, row 0 of example 5 is shifted by +50 (spread 0.05) and the last row of example 6 is
    scaled by 1e-3.  With the float64 outputs Y, dM, dE (without dE_up), dgamma, dbeta."""
    rnd = C.rnd_stream(torch.Generator().manual_seed(16000 + seed))
    E = rnd(B, F, D)
    _special(E, B)
    gamma, beta = (1.0 + rnd(F, D, std=0.5)).float().double(), rnd(F, D, std=0.3)
    Ms, dYs = [rnd(B, F * D) for _ in range(N)], [rnd(B, F * D) for _ in range(N)]
    if B > 8:
        for dY in dYs:
            dY[EX_NO_GRAD] = 0.0
    dMs, dE, dg, db = group_bwd(E, gamma, beta, Ms, dYs)
    return dict(B=B, F=F, D=D, N=N, E=E, gamma=gamma, beta=beta, M=Ms, dY=dYs, dE_up=rnd(B, F, D, std=0.1),
                Y=group_fwd(E, gamma, beta, Ms), dM=dMs, dE=dE, dgamma=dg, dbeta=db)


@C.memo
def plain_case(B, H, seed=0):
    """normalize = 0: X = h_prev >= 0 like a block's output, one mask."""
    rnd = C.rnd_stream(torch.Generator().manual_seed(16500 + seed))
    X, M, dY = torch.relu(rnd(B, H)), rnd(B, H), rnd(B, H)
    dM, dX = plain_bwd(X, M, dY)
    return dict(B=B, H=H, X=X, M=M, dY=dY, dE_up=rnd(B, H, std=0.1), Y=plain_fwd(X, M), dM=dM, dX=dX)


@C.memo
def row_case(B, H, seed=0):
    """A seeded row-kernel case: Z ~ N(0,1) with the special examples of kernel_case (the whole row is the group),
    the first stream whose pre-activations all stay ROW_KINK away from 0."""
    def build(g, rnd):
        Z = rnd(B, 1, H)
        _special(Z, B)
        Z = Z.view(B, H)
        gamma, beta, dh = (1.0 + rnd(H, std=0.5)).float().double(), rnd(H, std=0.3), rnd(B, H)
        if B > 8:
            dh[EX_NO_GRAD] = 0.0
        return (Z, gamma, beta, dh) + row_fwd(Z, gamma, beta, return_pre=True)

    (Z, gamma, beta, dh, h, pre), attempt = C.first_stream(17000 + 64 * seed, build,
                                                           lambda k: float(k[5].abs().min()) >= ROW_KINK)
    dZ, dg, db = row_bwd(Z, gamma, beta, dh)
    return dict(B=B, H=H, attempt=attempt, Z=Z, gamma=gamma, beta=beta, dh=dh, h=h, pre=pre, dZ=dZ, dgamma=dg, dbeta=db)


def group_errors(case, Y, dM, dE, dg, db):
    """(worst forward error, worst gradient measure) of a group kernel's outputs against the case's float64."""
    fwd = max(logit_error(a, b) for a, b in zip(Y, case["Y"]))
    bwd = max([grad_measure(a, b) for a, b in zip(dM, case["dM"])]
              + [grad_measure(dE, case["dE"]), grad_measure(dg, case["dgamma"]), grad_measure(db, case["dbeta"])])
    return fwd, bwd


def f32_stats_group(case):
    """The group kernel emulated with float32 statistics (mean and centred squares summed in float32), float32
    elementwise work and float32 batch sums -> (Y, dM, dE, dgamma, dbeta)."""
    E, gamma, beta = case["E"].float(), case["gamma"].float(), case["beta"].float()
    Ms, dYs = [m.float() for m in case["M"]], [d.float() for d in case["dY"]]
    return (group_fwd(E, gamma, beta, Ms),) + group_bwd(E, gamma, beta, Ms, dYs)


def f64_stats_group(case):
    """... and with the kernels' numerics: statistics and xhat in float64, rounded once, float32 behind them."""
    B, F, D = case["E"].shape
    xh64, rstd64 = ln_stats(case["E"])
    xh, rstd = xh64.float(), rstd64.float()
    gamma, beta = case["gamma"].float(), case["beta"].float()
    Ms, dYs = [m.float() for m in case["M"]], [d.float() for d in case["dY"]]
    V = (gamma * xh + beta).reshape(B, F * D)
    dV = sum(dY * M for dY, M in zip(dYs, Ms)).view(B, F, D)
    return ([M * V for M in Ms], [dY * V for dY in dYs], ln_bwd(dV * gamma, xh, rstd), (dV * xh).sum(dim=0),
            dV.sum(dim=0))


# ---------------------------------------------------------------------------------------------------- the model
def agg_units(ratio, wout):
    return max(1, round(ratio * wout))


def block_widths(hp, FD):
    """[Wout of block 1..N]."""
    N, H = hp.get("num_blocks", 3), hp.get("block_hidden_units", 64)
    par = hp.get("block_order", "parallel") == "parallel"
    return [FD if (par or n == 1) else H for n in range(1, N + 1)]


def mask_block(p, n, x, inp, pres=None, wrong=None):
    """Block n (1-based) on `inp` [B,Wout] (already normalised where it is the embedding)."""
    pre_a = x @ p[f"block{n}_agg_weights"] + p[f"block{n}_agg_bias"]
    M = torch.relu(pre_a) @ p[f"block{n}_proj_weights"] + p[f"block{n}_proj_bias"]
    Z = (M * inp) @ p[f"block{n}_hidden_weights"]
    h, pre_h = row_fwd(Z, p[f"block{n}_ln_gamma"], p[f"block{n}_ln_beta"], return_pre=True)
    if pres is not None:
        pres += [pre_a, pre_h]
    return h


def blocks(p, E, dense, hp, pres=None, wrong=None):
    """E [B,F,D], dense -> the DNN's input without the dense columns: [h_1 | .. | h_N] or h_N."""
    B, F, D = E.shape
    x = TL.dnn_input(E, dense)
    V = ln_emb(E, p["ln_emb_gamma"], p["ln_emb_beta"]).reshape(B, F * D)
    N = hp.get("num_blocks", 3)
    if hp.get("block_order", "parallel") == "parallel":
        return torch.cat([mask_block(p, n, x, V, pres) for n in range(1, N + 1)], dim=1)
    h = mask_block(p, 1, x, V, pres)
    for n in range(2, N + 1):
        if wrong == "renormalised":  # serial blocks re-normalising h_prev
            h = ln_stats(h)[0]
        h = mask_block(p, n, x, h, pres)
    return h


def masknet_logit(p, spec, idx, dense, hp, training=True, masks=None, manual_weights=None, mv=None, return_pre=False,
                  wrong=None):
    """logit = DNN([blocks | dense]) (+ linear with use_linear); no bias tables, no FM term."""
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    pres = []
    X = TL.dnn_input(blocks(p, E, dense, hp, pres, wrong), dense)
    n = len(hp["deep_hidden_units"])
    keep, dm = C.dnn_keep(hp, n, training), (masks or {}).get("dnn")
    logit = TL.dnn(p, X, n, hp.get("deep_activation", "relu"), keep, dm)
    if hp.get("use_linear", True):
        logit = logit + TL.linear_layer(p, spec, idx, dense, manual_weights, mv)
    return (logit, pres + C.dnn_pres(p, X, n, keep, dm)) if return_pre else logit


def masknet_l2(p, spec, hp):
    out = C.base_l2(p, spec, hp, len(hp["deep_hidden_units"]), hp.get("use_linear", True))
    reg = hp.get("deep_l2_reg", 0.0)
    for n in range(1, hp.get("num_blocks", 3) + 1):
        out = out + sum(reg * 0.5 * p[f"block{n}_{w}_weights"].square().sum() for w in ("agg", "proj", "hidden"))
    return out


# (p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None) -> (loss, logit [B,1], pred)
model_loss = partial(C.model_loss, masknet_logit, masknet_l2)
# ... -> (loss, logit [B], pred [B], grads): one forward+backward, the twin of oracle.th_layers.fwd_bwd
fwd_bwd = partial(C.fwd_bwd, model_loss)


def min_abs_pre(p, spec, idx, dense, hp, masks=None, mv=None):
    """The distance of the closest relu unit (mask aggregation layers, LN_H outputs, DNN layers) to its kink."""
    pres = masknet_logit(p, spec, idx, dense, hp, masks=masks, mv=mv, return_pre=True)[1]
    return min(float(t.abs().min()) for t in pres)


def block_params(rnd, hp, F, D, Dn):
    """The blocks' and the DNN's variables (names of the contract): glorot weights, gains 1 + 0.3 N(0,1), biases
    0.1 N(0,1) (0.2 for the LayerNorms)."""
    FD, K, H = F * D, F * D + Dn, hp["block_hidden_units"]
    p = {"ln_emb_gamma": (1.0 + rnd(F, D, std=0.3)).float().double(), "ln_emb_beta": rnd(F, D, std=0.2)}
    widths = block_widths(hp, FD)
    for n, wout in enumerate(widths, 1):
        A = agg_units(hp["reduction_ratio"], wout)
        p[f"block{n}_agg_weights"] = glorot(rnd, (K, A), K, A)
        p[f"block{n}_agg_bias"] = rnd(A, std=0.1)
        p[f"block{n}_proj_weights"] = glorot(rnd, (A, wout), A, wout)
        p[f"block{n}_proj_bias"] = rnd(wout, std=0.1)
        p[f"block{n}_hidden_weights"] = glorot(rnd, (wout, H), wout, H)
        p[f"block{n}_ln_gamma"] = (1.0 + rnd(H, std=0.3)).float().double()
        p[f"block{n}_ln_beta"] = rnd(H, std=0.2)
    d_in = (len(widths) if hp["block_order"] == "parallel" else 1) * H + Dn
    C.draw_dnn(rnd, p, [d_in] + list(hp["deep_hidden_units"]))
    return p


# model-level cases (all B <= 256, F <= 6, H <= 32): order, num_blocks, H, ratio, hidden, B, F, D, Dn
MODEL_CASES = {
    "parallel3": ("parallel", 3, 32, 2.0, (32, 16), 130, 5, 8, 3),
    "parallel1_no_dense": ("parallel", 1, 16, 0.5, (16,), 64, 6, 16, 0),
    "serial3": ("serial", 3, 32, 2.0, (32, 16), 130, 5, 8, 3),
    "serial1": ("serial", 1, 8, 1.3, (16,), 33, 3, 32, 2),
    "serial3_no_dense": ("serial", 3, 32, 1.0, (16, 16), 256, 4, 16, 0),
}


@C.memo
def make_case(order, N, H, ratio, hidden, B, F, D, Dn, seed=0, use_linear=True, l2=1e-4):
    """A seeded model-level case in float64 (made once, never changed): spec, p, idx, dense, y, hp.  Embeddings ~
    N(0, 0.15^2), dense ~ N(0,1).  The first stream in which every relu unit is at least MODEL_KINK from its kink."""
    spec, sizes = C.plain_spec(F, Dn)
    hp = dict(embedding_size=D, embedding_l2_reg=l2, linear_l2_reg=l2, deep_hidden_units=tuple(hidden),
              deep_dropout=(1,) * (len(hidden) + 1), deep_l2_reg=l2, block_order=order, num_blocks=N,
              block_hidden_units=H, reduction_ratio=ratio, use_linear=use_linear, deep_activation="relu")

    def build(g, rnd):
        p = C.draw_front(rnd, spec, D, std=0.15)
        p.update(block_params(rnd, hp, F, D, Dn))
        idx, dense, y = C.draw_batch(g, rnd, sizes, B, Dn)
        return dict(spec=spec, p=p, idx=idx, dense=dense, y=y, hp=hp, min_abs_pre=min_abs_pre(p, spec, idx, dense, hp))

    k, attempt = C.first_stream(18000 + 64 * seed, build, lambda k: k["min_abs_pre"] >= MODEL_KINK)
    return dict(k, attempt=attempt)
