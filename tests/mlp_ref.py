"""Plain float64 references and error bounds for the skinny-MLP kernels (csrc/mlp.hip: rm_mlp_fwd, rm_embed_mlp_fwd,
rm_mlp_bwd and the fused training head rm_mlp_tail).  Test infrastructure, like tests/front_refs.py, whose bound
helpers and loss functions it reuses: tests/test_mlp_host.py checks it on the CPU, tests/test_gpu_mlp_kernels.py uses
it on the GPU.

Every function restates ONE stage of the contract in include/recman_hip.h in torch, in float64, on whatever device
its inputs live on, from the SAME fp32 tensors the kernel gets (widened, never re-rounded).  Nothing here is derived
from the kernels: no tiles, no lane maps, no launch arithmetic.  Hidden tensors (h_l, dh_l) may be passed as the
kernel stores them, [B, 32] with zero columns past H_l: only the first H_l columns are read.

A function that sums returns, next to the value, the float64 sum of the |terms| of every output element; the
comparison is front_refs.sum_bound(n, sum|terms|) with the n stated in the docstring (and again at every call).

Activation.  relu and identity are 1-Lipschitz and exact in fp32, so act(fp32 sum) is as close to act(exact sum) as
the sums are to each other - whichever side of the kink each lands on.  leaky_relu multiplies by fp32(0.2) on the
negative side: one more rounding, inside the bound's slack of 2.  The SLOPE of the backward is read off the
post-activation value the kernel stored (act' = 1 where it is > 0), as rm_act_bwd's contract does: fp32 and float64
can then never take different branches, and no element has to be left out of a comparison.
"""
import torch

from tests import front_refs as R

F64 = torch.float64
LEAK32 = float(torch.tensor(0.2, dtype=torch.float32))  # the slope as the fp32 kernels hold it


def _act(z, act):
    if act == "relu":
        return z.clamp(min=0)
    if act == "leaky_relu":
        return torch.where(z > 0, z, LEAK32 * z)
    assert act == "identity", act
    return z


def _slope(a, act):
    """act' read off the post-activation value a (float64 of what the kernel stored)."""
    if act == "relu":
        return (a > 0).to(F64)
    if act == "leaky_relu":
        return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, LEAK32))
    assert act == "identity", act
    return torch.ones_like(a)


def _cols(t, n):
    return t[:, :n].to(F64)


# ----------------------------------------------------------------------------------------------------- forward
def layer_ref(h_prev, W, b, act):
    """One hidden layer: act(h_prev W + b).  h_prev [B, >= K_l] (its first K_l = W.shape[0] columns are the input).
    Returns (h [B, H_l], sum|terms| of the pre-activation).  n = K_l + 1."""
    x, W64, b64 = _cols(h_prev, W.shape[0]), W.to(F64), b.to(F64)
    return _act(x @ W64 + b64, act), x.abs() @ W64.abs() + b64.abs()


def logit_ref(h_last, w_out, w0):
    """The output projection h_last w_out + w0: (logit [B], sum|terms|).  n = H + 1."""
    h, w = _cols(h_last, w_out.shape[0]), w_out.to(F64)
    w0 = torch.zeros((), dtype=F64, device=h.device) if w0 is None else w0.to(F64).reshape(())
    return h @ w + w0, h.abs() @ w.abs() + w0.abs()


def head_ref(dnn, branches, coef_mlp, y, task, grad_scale=1.0, pred=None):
    """rm_mlp_tail: final logit = coef_a a + coef_b b + coef_mlp dnn (branches: up to two (tensor, coefficient) pairs,
    summed BEFORE the MLP's logit), PredictionLayer + create_loss per example (front_refs.loss_point_ref; pred = the
    fp32 probabilities the kernel wrote, as that function documents), dlogit = dz / B * grad_scale, the per-example
    loss terms and their mean.  Returns a dict: logit + logit_abs (n = 3), pred, dlogit, terms, loss [1].
    dlogit is dLoss/d(final logit).  The backward takes it as dLoss/d(the MLP's logit), which it is only for
    coef_mlp = 1: the contract admits no other value in a tail (rm_mlp_tail refuses it), and the stage references
    downstream are called with g = dlogit on that ground.  coef_mlp stays a parameter of the branch sum."""
    z, zab = R.logit_sum_ref(list(branches) + [(dnn, coef_mlp)])
    B = z.shape[0]
    p, dz, terms = R.loss_point_ref(z, y, task, pred=pred)
    return dict(logit=z, logit_abs=zab, pred=p, dlogit=dz / B * R._f32(grad_scale), terms=terms,
                loss=terms.mean().reshape(1))


# ----------------------------------------------------------------------------------------------------- backward
def dh_last_ref(g, w_out, h_last, act):
    """dLoss/d(pre-activation of the last layer) = g w_out act'(h_last): (dh [B, H], sum|terms| = |dh|).  n = H + 1
    (one product of three factors per element; the n of the chain's other links, for one rule)."""
    H = w_out.shape[0]
    v = g.to(F64)[:, None] * w_out.to(F64)[None, :] * _slope(_cols(h_last, H), act)
    return v, v.abs()


def dh_prev_ref(dh_l, W_l, h_prev, act):
    """dh_{l-1} = (dh_l W_l^T) act'(h_{l-1}), W_l [H_{l-1}, H_l]: (dh [B, H_{l-1}], sum|terms|).  n = H_l + 1."""
    Hp, Hl = W_l.shape
    d, W64, s = _cols(dh_l, Hl), W_l.to(F64), _slope(_cols(h_prev, Hp), act)
    return (d @ W64.T) * s, (d.abs() @ W64.abs().T) * s


def d_rows_ref(dh0, W0, FD, g=None, S=None, E=None):
    """dLoss/dxe = dh0 W0[:FD]^T (+ g (S - E), the FM second-order term, when S [B, D] and E = xe [B, FD] are given;
    column k of xe belongs to embedding column k mod D).  Returns (d_rows [B, FD], sum|terms|).  n = H0 + 2."""
    H0 = W0.shape[1]
    d, W64 = _cols(dh0, H0), W0[:FD].to(F64)
    v, ab = d @ W64.T, d.abs() @ W64.abs().T
    if S is not None:
        B, D = S.shape
        g64 = g.to(F64)[:, None]
        s = S.to(F64).repeat(1, FD // D)
        e = E.to(F64).reshape(B, FD)
        v, ab = v + g64 * (s - e), ab + (g64 * s).abs() + (g64 * e).abs()
    return v, ab


def dW0_ref(x, dh0):
    """dW0 = x^T dh0 with x = [xe | xd] [B, K]: (dW0 [K, width of dh0], sum|terms|) - slice [:, :H0] of a padded dh0.
    n = B."""
    x64, d = x.to(F64), dh0.to(F64)
    return x64.T @ d, x64.abs().T @ d.abs()


def dW_ref(h_prev, dh_l):
    """dW_l = h_{l-1}^T dh_l for l >= 1: (dW, sum|terms|), as wide as its inputs - slice [:H_{l-1}, :H_l] of padded
    ones.  n = B."""
    h, d = h_prev.to(F64), dh_l.to(F64)
    return h.T @ d, h.abs().T @ d.abs()


def db_ref(dh_l):
    """db_l = column sums of dh_l: (db, sum|terms|) - slice [:H_l].  n = B."""
    d = dh_l.to(F64)
    return d.sum(0), d.abs().sum(0)


def d_w_out_ref(h_last, g):
    """d w_out = h_last^T g: (d_w_out, sum|terms|) - slice [:H_last].  n = B."""
    t = h_last.to(F64) * g.to(F64)[:, None]
    return t.sum(0), t.abs().sum(0)


def sum_g_ref(g):
    """sum_b g[b], the gradient of w0_out (d_w0_out) and of the linear term's bias (d_g_sum): ([1], sum|terms|).
    n = B."""
    g64 = g.to(F64)
    return g64.sum().reshape(1), g64.abs().sum().reshape(1)


def d_xd_wsum_ref(xd, g):
    """d_xd_wsum = sum_b g[b] xd[b, :], the gradient of the linear term's dense weights: ([Dn], sum|terms|).
    n = B."""
    t = xd.to(F64) * g.to(F64)[:, None]
    return t.sum(0), t.abs().sum(0)


# -------------------------------------------------------------------------------------- the whole thing, autograd
def mlp_autograd_ref(xe, xd, Ws, bs, w_out, w0, act, y, task, *, D=0, lin_w=None, lin_w0=None, extra=None,
                     coef_extra=1.0, grad_scale=1.0):
    """The forward, the head and the FM term in float64 through torch autograd - written as a MODEL, not as stages;
    it exists to check the stage functions above (tests/test_mlp_host.py).
        dnn   = MLP([xe | xd])                 final logit z = dnn + fm2 + lin + coef_extra * extra
        fm2   = 0.5 sum_k ((sum_f E)^2 - sum_f E^2),  E = xe as [B, FD / D, D]     (D > 0)
        lin   = xd lin_w + lin_w0                                                  (lin_w given)
        loss  = grad_scale * mean_b term(z_b, y_b)   (front_refs.loss_point_ref's term: Keras BCE on clipped
                probabilities, the clip passing no gradient outside, or MSE)
    Returns a dict of float64 values (h list, dnn, z, pred, loss) and gradients (g = dloss/dz, xe, W list, b list,
    w_out, w0, lin_w, lin_w0)."""
    leaf = lambda t: None if t is None else t.detach().to(F64).clone().requires_grad_(True)
    xe_, Ws_, bs_, wo_, w0_ = leaf(xe), [leaf(W) for W in Ws], [leaf(b) for b in bs], leaf(w_out), leaf(w0)
    lw_, l0_ = leaf(lin_w), leaf(lin_w0)
    xd64 = None if xd is None else xd.detach().to(F64)
    x = xe_ if xd64 is None or xd64.shape[1] == 0 else torch.cat([xe_, xd64], 1)
    hs, hcur = [], x
    for W, b in zip(Ws_, bs_):
        hcur = _act(hcur @ W + b, act)
        hs.append(hcur)
    dnn = hcur @ wo_ + w0_.reshape(())
    z = dnn
    if D:
        Bn, FD = xe_.shape
        E = xe_.reshape(Bn, FD // D, D)
        z = z + 0.5 * (E.sum(1).square() - E.square().sum(1)).sum(1)
    if lw_ is not None:
        z = z + xd64 @ lw_ + l0_.reshape(())
    if extra is not None:
        z = z + R._f32(coef_extra) * extra.detach().to(F64)
    z.retain_grad()
    t = y.to(F64)
    if task == "classification":
        p = torch.sigmoid(z)
        inside = ((p >= R.KERAS_EPS32) & (p <= R.KERAS_HI32)).detach()
        pc = torch.where(inside, p, p.detach().clamp(R.KERAS_EPS32, R.KERAS_HI32))  # clip: no gradient outside
        terms = -(t * torch.log(pc + R.KERAS_EPS32) + (1 - t) * torch.log(1 - pc + R.KERAS_EPS32))
    else:
        p = z
        terms = (z - t).square()
    loss = R._f32(grad_scale) * terms.mean()
    loss.backward()
    gr = lambda v: None if v is None else v.grad
    return dict(h=[h.detach() for h in hs], dnn=dnn.detach(), z=z.detach(), pred=p.detach(),
                loss=terms.mean().detach().reshape(1), g=z.grad, xe=xe_.grad, W=[W.grad for W in Ws_],
                b=[b.grad for b in bs_], w_out=wo_.grad, w0=w0_.grad, lin_w=gr(lw_), lin_w0=gr(l0_))

