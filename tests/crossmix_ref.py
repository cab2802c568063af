"""CPU PyTorch restatement (dtype-generic) of the DCN-Mix cross network and of DCN with cross_type="mix".

TEST INFRASTRUCTURE.  Nothing in the reference implements a cross layer, so the arithmetic is the paper's (DCN-V2,
arXiv 2008.13535 eq. 4-5) as the project's contract states it.  With E experts of rank r, expert i owning columns
[i r, i r + r), for layer l from x_0 = x0 [B,d]:

    t = x_l V_l   s = x_l G_l   a_i = tanh(t_i)   c_i = tanh(a_i C_{l,i})   p = softmax_i(s)   m = [p_1 c_1 | .. | p_E c_E]
    x_{l+1} = x0 o (m U_l^T + b_l) + x_l          cross_logit = x_L w_out

    core backward (a, c, p recomputed):  dc_i = p_i dm_i   dp_i = <dm_i, c_i>   ds_i = p_i (dp_i - sum_j p_j dp_j)
        dh_i = dc_i o (1 - c_i^2)   dC_i = sum_b a_i^T dh_i   da_i = dh_i C_i^T   dt_i = da_i o (1 - a_i^2)

The gate is per layer.  Everything but the cross network is composed from the public functions of oracle.th_layers,
imported and not modified.  tests/test_crossmix_host.py pins this file without a GPU; the GPU tests compare the HIP
kernels and the engine against it in float64.
"""
from functools import partial

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK, glorot, grad_measure, to_f32  # noqa: F401  (part of this module's interface)

# kernel-level GPU cases (B, E, r) of tests/test_gpu_cross_mix.py (the grid-stride case is built there)
GPU_CASES = [(5, 1, 8), (37, 1, 8), (33, 3, 8), (9, 5, 16), (64, 4, 32), (130, 4, 16), (65, 2, 64), (257, 8, 32)]
# model-level cases (B, F, D, Dn, L, E, r)
MODEL_CASES = {
    "e1_r8": (33, 5, 8, 3, 2, 1, 8),
    "e4_r16": (257, 5, 8, 3, 3, 4, 16),
    "criteo_like": (130, 26, 16, 13, 3, 4, 32),
    "no_dense_r64": (65, 7, 8, 0, 4, 2, 64),
}
TOL_M, TOL_GRAD = 1e-5, 2e-5  # the project's own: absolute on M and the logits, the gradient measure on gradients


def tanh_exp(x):
    """The kernels' form of tanh: 1 - 2 / (exp(2x) + 1)."""
    return 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0)


def _parts(t, s, C, tanh):
    """-> a [B,E,r], c [B,E,r], p [B,E]."""
    E, r = C.shape[0], C.shape[1]
    a = tanh(t.reshape(t.shape[0], E, r))
    c = tanh(torch.einsum("bij,ijk->bik", a, C))
    p = torch.softmax(s, dim=1)
    return a, c, p


def core_fwd(t, s, C, tanh=torch.tanh, wrong=None):
    """t [B, E r], s [B, E], C [E,r,r] -> m [B, E r].  wrong: one of the deliberately wrong restatements that
    tests/test_crossmix_host.py shows the tolerances to catch."""
    B, E, r = t.shape[0], C.shape[0], C.shape[1]
    if wrong == "c_transposed":
        C = C.transpose(1, 2)
    a = tanh(t.reshape(B, E, r))
    h = torch.einsum("bij,ijk->bik", a, C)
    c = h if wrong == "no_second_tanh" else tanh(h)
    p = torch.softmax(s, dim=1)
    m = c if wrong == "no_p" else p.unsqueeze(2) * c
    if wrong == "blocks_swapped":
        m = torch.cat([m[:, 1:2], m[:, 0:1], m[:, 2:]], dim=1)
    return m.reshape(B, E * r)


def core_bwd(t, s, C, dm, tanh=torch.tanh, wrong=None):
    """The backward of the contract, written out (no autograd): -> (dt [B, E r], ds [B, E], dC [E,r,r])."""
    B, E, r = t.shape[0], C.shape[0], C.shape[1]
    a, c, p = _parts(t, s, C, tanh)
    dm = dm.reshape(B, E, r)
    dc = p.unsqueeze(2) * dm
    dp = (dm * c).sum(dim=2)
    mean = torch.zeros_like(dp) if wrong == "ds_without_mean" else (p * dp).sum(dim=1, keepdim=True)
    ds = p * (dp - mean)
    dh = dc * (1.0 - c * c)
    dC = torch.einsum("bij,bik->ijk", a, dh)
    da = torch.einsum("bik,ijk->bij", dh, C)
    dt = da * (1.0 - a * a)
    return dt.reshape(B, E * r), ds, dC


def core_loops(t, s, C):
    """core_fwd as explicit Python loops over floats (no tensor arithmetic)."""
    import math

    E, r = C.shape[0], C.shape[1]
    tl, sl, Cl = t.tolist(), s.tolist(), C.tolist()
    out = []
    for b in range(len(tl)):
        mx = max(sl[b])
        e = [math.exp(v - mx) for v in sl[b]]
        p = [v / sum(e) for v in e]
        row = []
        for i in range(E):
            a = [math.tanh(v) for v in tl[b][i * r:(i + 1) * r]]
            row += [p[i] * math.tanh(sum(a[j] * Cl[i][j][k] for j in range(r))) for k in range(r)]
        out.append(row)
    return torch.tensor(out, dtype=t.dtype).reshape(len(tl), E * r)


SPECIAL_ROWS = {3: "t x 8", 4: "t = 0", 5: "s x 60", 6: "s = 0", 7: "dm = 0"}


@C.memo
def kernel_case(B, E, r, seed=0):
    """A seeded kernel-level case in float64 (made once per shape, never changed): t ~ N(0,1), s ~ 2 N(0,1),
    C ~ 1.5 glorot(r, r), dm ~ N(0,1); with B > 8 the special rows 3: t x 8 (saturated tanh), 4: t = 0 (m exactly 0),
    5: s x 60 (needs the max-subtraction), 6: s = 0 (p = 1/E), 7: dm = 0 (dt, ds exactly 0).  With the float64 outputs
    m, dt, ds, dC."""
    def build(g, rnd):
        t, s, dm = rnd(B, E * r), rnd(B, E, std=2.0), rnd(B, E * r)
        Cm = (1.5 * glorot(rnd, (E, r, r), r, r)).float().double()
        if B > 8:
            t[3] *= 8.0
            t[4] = 0.0
            s[5] *= 60.0
            s[6] = 0.0
            dm[7] = 0.0
        return t, s, dm, Cm

    def ok(drawn):  # the special rows are what they claim: row 3 holds a tanh that rounds to 1 in float32; row 5 has a
        t, s = drawn[:2]  # score whose float32 exp overflows without the max-subtraction
        return B <= 8 or (float(t[3].abs().max()) > 9.1 and (E == 1 or float(s[5].max()) > 100.0))

    t, s, dm, Cm = C.first_stream(9000 + 64 * seed, build, ok)[0]
    dt, ds, dC = core_bwd(t, s, Cm, dm)
    return dict(B=B, E=E, r=r, t=t, s=s, C=Cm, dm=dm, m=core_fwd(t, s, Cm), dt=dt, ds=ds, dC=dC)


def f32_errors(case, tanh=torch.tanh):
    """The float32 CPU restatement's own errors on a kernel case: (max |m - m64|, measure dt, measure ds, measure dC)."""
    f = lambda n: case[n].float()  # noqa: E731
    m = core_fwd(f("t"), f("s"), f("C"), tanh)
    dt, ds, dC = core_bwd(f("t"), f("s"), f("C"), f("dm"), tanh)
    return (float((m.double() - case["m"]).abs().max()), grad_measure(dt, case["dt"]), grad_measure(ds, case["ds"]),
            grad_measure(dC, case["dC"]))


# ---------------------------------------------------------------------------------------------------- the model
def mix_dims(p):
    """(L, E, r) of a parameter set."""
    return p["cross_c"].shape[0], p["cross_c"].shape[1], p["cross_c"].shape[2]


def cross_mix_net(p, x0, tanh=torch.tanh):
    """The cross stack: x0 [B,d] -> cross_logit [B,1]."""
    L = p["cross_c"].shape[0]
    x = x0
    for l in range(L):
        m = core_fwd(x @ p["cross_v"][l], x @ p["cross_gate"][l], p["cross_c"][l], tanh)
        x = x0 * (m @ p["cross_u"][l].t() + p["cross_b"][l]) + x
    return x @ p["cross_w_out"]


CROSS_L2_NAMES = ("cross_v", "cross_gate", "cross_c", "cross_u", "cross_w_out")


cross_mix_l2 = partial(C.param_l2, CROSS_L2_NAMES)  # (p, l2_reg)


def dcn_mix_logit(p, spec, idx, dense, hp, training=True, masks=None, manual_weights=None, mv=None, tanh=torch.tanh,
                  return_pre=False):
    """DCN's composition (oracle.th_layers.dcn_logit) with the mix cross network: dnn + cross (+ dnn under
    strict_reference) (+ linear with use_linear)."""
    masks = masks or {}
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    x = TL.dnn_input(E, dense)
    n = len(hp["deep_hidden_units"])
    keep = hp.get("deep_dropout", [1] * (n + 1)) if training else [1] * (n + 1)
    dnn_logit = TL.dnn(p, x, n, hp.get("deep_activation", "relu"), keep, masks.get("dnn"))
    logit = dnn_logit + cross_mix_net(p, x, tanh)
    if hp.get("strict_reference", False):
        logit = logit + dnn_logit
    if hp.get("use_linear", True):
        logit = logit + TL.linear_layer(p, spec, idx, dense, manual_weights, mv)
    return (logit, C.dnn_pres(p, x, n)) if return_pre else logit  # (the pre-activations without dropout)


def dcn_mix_l2(p, spec, hp):
    return C.base_l2(p, spec, hp, len(hp["deep_hidden_units"]), hp.get("use_linear", True)) + cross_mix_l2(
        p, hp.get("cross_layer_l2_reg", 0.0))


# (p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None, tanh=torch.tanh) -> (loss, logit [B,1], pred)
model_loss = partial(C.model_loss, dcn_mix_logit, dcn_mix_l2)
# ... -> (loss, logit [B], pred [B], grads): one forward+backward, the twin of oracle.th_layers.fwd_bwd
fwd_bwd = partial(C.fwd_bwd, model_loss)


def cross_params(rnd, d, L, E, r):
    """The variables of the mix cross network: glorot with the contract's fans, cross_b ~ 0.1 N(0,1)."""
    return {
        "cross_v": glorot(rnd, (L, d, E * r), d, r),
        "cross_gate": glorot(rnd, (L, d, E), d, E),
        "cross_c": glorot(rnd, (L, E, r, r), r, r),
        "cross_u": glorot(rnd, (L, d, E * r), r, d),
        "cross_b": rnd(L, d, std=0.1),
        "cross_w_out": glorot(rnd, (d, 1), d, 1),
    }


@C.memo
def make_case(B, F, D, Dn, L, E, r, seed=0, hidden=(32, 32), use_linear=True, l2=1e-4):
    """A seeded model-level case in float64 (made once, never changed): spec, p (the variable names of the contract),
    idx, dense, y, hp.  Embeddings ~ N(0, 0.15^2), dense ~ N(0,1), cross_b ~ N(0, 0.1^2); `min_abs_pre` is the distance
    of the DNN's closest unit to its kink."""
    spec, sizes = C.plain_spec(F, Dn)
    g = torch.Generator().manual_seed(8000 + seed)
    rnd = C.rnd_stream(g)
    d = F * D + Dn
    p = C.draw_front(rnd, spec, D, std=0.15)
    C.draw_dnn(rnd, p, [d] + list(hidden))
    p.update(cross_params(rnd, d, L, E, r))
    idx, dense, y = C.draw_batch(g, rnd, sizes, B, Dn)
    hp = dict(embedding_size=D, embedding_l2_reg=l2, linear_l2_reg=l2, deep_hidden_units=tuple(hidden),
              deep_dropout=(1,) * (len(hidden) + 1), deep_l2_reg=l2, cross_layer_l2_reg=l2, cross_layer_num=L,
              cross_type="mix", cross_experts=E, cross_low_rank=r, use_linear=use_linear)
    return dict(spec=spec, p=p, idx=idx, dense=dense, y=y, hp=hp,
                min_abs_pre=C.min_abs(dcn_mix_logit(p, spec, idx, dense, hp, return_pre=True)[1]))
