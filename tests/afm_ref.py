"""CPU PyTorch restatement (dtype-generic, autograd) of the AFM attention layer and of the AFM model.

TEST INFRASTRUCTURE.  The reference has no code for the layer (recman/tf/core/AFM.py:7 comments the import out), so
the arithmetic is the paper's (arXiv 1708.04617 eq. (4)-(6)) as the project's contract states it:

    P_ij = E_i * E_j  (i < j, row-major over the upper triangle),  z_ij = W^T P_ij + b,  s_ij = h . relu(z_ij),
    a = softmax_ij(s),  v = sum_ij a_ij P_ij,  afm_logit = p . (m * v)

The model (AFM.py:111-126) is composed from the public functions of oracle.th_layers, imported and not modified.
tests/test_afm_host.py pins this file without a GPU; the GPU tests compare the HIP kernels against it in float64.
"""
from functools import partial

import torch

from oracle import th_layers as TL
from tests import ref_common as C
from tests.ref_common import KINK, glorot, grad_measure  # noqa: F401  (part of this module's interface)

# kernel-level GPU cases (B, F, D, T) of tests/test_gpu_afm.py; tests/test_afm_host.py asserts the kink guard's cap on
# every one of them (each with h_scale 1; the two softmax-range cases again with 400)
GPU_CASES = [(37, 5, 8, 8), (64, 26, 16, 8), (130, 26, 16, 32), (9, 39, 64, 64), (300, 40, 32, 16), (33, 2, 8, 4),
             (1, 6, 8, 8), (2, 6, 8, 8), (3, 6, 8, 8), (4100, 26, 16, 8), (2000, 26, 16, 64)]
# seed of make_afm_case per case (0 unless listed): with B = 9 one example is 11 % of the batch, and the seed is one
# under which the guard zeroes one example, not two
CASE_SEEDS = {(9, 39, 64, 64): 3}
RANGE_CASES = [(64, 26, 16, 8), (130, 26, 16, 32)]
RANGE_H_SCALE = 400.0
KINK_CAP = 0.20    # largest share of examples the guard may zero

# model-level GPU cases of tests/test_gpu_afm_model.py: keyword arguments of make_afm_case.  Their g comes from
# the labels and cannot be zeroed, so the seeds are such that no hidden unit lies within KINK of 0 (asserted on the
# CPU in tests/test_afm_host.py)
MODEL_CASES = {
    "d8": dict(B=37, F=5, D=8, Dn=2, T=8, seed=0),
    "d16": dict(B=37, F=5, D=16, Dn=2, T=8, seed=0),
    "d32": dict(B=37, F=5, D=32, Dn=2, T=4, seed=0),
    "d64": dict(B=21, F=7, D=64, Dn=2, T=16, seed=0),
    "criteo_like": dict(B=150, F=26, D=16, Dn=13, T=8, seed=1),
    "no_dense": dict(B=37, F=5, D=8, Dn=0, T=8, seed=0),
    "odd_factor": dict(B=45, F=9, D=16, Dn=1, T=5, seed=0),
}


def pair_index(F):
    """(i, j) index vectors of the F(F-1)/2 pairs, i < j, row-major over the upper triangle."""
    i, j = torch.triu_indices(F, F, 1)
    return i, j


def afm_hidden(E, W, b):
    """(P [B,P,D], z [B,P,T]): the pair products and the attention net's pre-activations."""
    i, j = pair_index(E.shape[1])
    P = E[:, i, :] * E[:, j, :]
    return P, P @ W + b


def afm_layer(E, W, b, h, p, mask=None):
    """E [B,F,D], W [D,T], b [T], h [T], p [D], mask [B,D] (dropout multiplier, 0 or 1/keep) -> afm_logit [B]."""
    P, z = afm_hidden(E, W, b)
    s = torch.relu(z) @ h.reshape(-1)
    a = torch.softmax(s, dim=1)  # max-subtracted
    v = (a.unsqueeze(-1) * P).sum(dim=1)
    u = v if mask is None else v * mask
    return u @ p.reshape(-1)


def afm_layer_bwd(E, W, b, h, p, mask, g, dE_up=None):
    """The backward of the contract, written out (no autograd): -> (dE, dW, db, dh, dp)."""
    B, F, D = E.shape
    i, j = pair_index(F)
    h, p = h.reshape(-1), p.reshape(-1)
    P, z = afm_hidden(E, W, b)
    r = torch.relu(z)
    a = torch.softmax(r @ h, dim=1)
    v = (a.unsqueeze(-1) * P).sum(dim=1)
    m = torch.ones_like(v) if mask is None else mask
    u = m * v
    logit = u @ p
    c = g.unsqueeze(1) * (m * p)                            # dLoss/dv
    q = (P * c.unsqueeze(1)).sum(dim=2)
    ds = a * (q - (g * logit).unsqueeze(1))
    dz = ds.unsqueeze(-1) * h * (z > 0).to(E.dtype)
    dP = a.unsqueeze(-1) * c.unsqueeze(1) + dz @ W.t()
    dE = torch.zeros_like(E) if dE_up is None else dE_up.clone()
    dE.index_add_(1, i, dP * E[:, j, :])
    dE.index_add_(1, j, dP * E[:, i, :])
    dW = torch.einsum("bpd,bpt->dt", P, dz)
    return dE, dW, dz.sum(dim=(0, 1)), (ds.unsqueeze(-1) * r).sum(dim=(0, 1)), (g.unsqueeze(1) * u).sum(dim=0)


# ---------------------------------------------------------------------------------------------------- the model
AFM_NAMES = ("afm_attention_w", "afm_attention_b", "afm_attention_h", "afm_projection_p")


def afm_logit(p, spec, idx, dense, hp, training=True, masks=None, manual_weights=None, mv=None):
    """AFM._init_graph (AFM.py:98-126): logit = linear + afm; the bias tables AFM.py:102-109 gathers are unused."""
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False, mv=mv)
    logit = TL.linear_layer(p, spec, idx, dense, manual_weights, mv)
    mask = (masks or {}).get("afm") if (training and hp.get("att_dropout", 1) < 1) else None
    afm = afm_layer(E, p["afm_attention_w"], p["afm_attention_b"], p["afm_attention_h"], p["afm_projection_p"],
                    mask)
    return logit + afm.reshape(-1, 1)


def afm_l2(p, spec, hp):
    """AFM.py:132-143: embeddings + linear + the attention layer's l2 (the attention matrix only, as in the paper)."""
    return C.base_l2(p, spec, hp, None, True) + hp.get("att_l2_reg", 0.0) * 0.5 * p["afm_attention_w"].square().sum()


# (p, spec, idx, dense, y, hp, task="classification", masks=None, mv=None) -> (loss, logit [B,1], pred)
model_loss = partial(C.model_loss, afm_logit, afm_l2)
# ... -> (loss, logit [B], pred [B], grads): one forward+backward, the twin of oracle.th_layers.fwd_bwd
fwd_bwd = partial(C.fwd_bwd, model_loss)


# -------------------------------------------------------------------------------------------------------- cases
def make_afm_case(B, F, D, Dn, T, seed=0, h_scale=1.0, dtype=torch.float64, att_dropout=1.0):
    """A seeded AFM case, model level and layer level at once.  Scales: table rows ~ 0.3 N(0,1) (so E is),
    glorot W / h / p (h times h_scale), b ~ 0.1 N(0,1).  Returns a dict:
      model level: spec, p (reference variable names), idx, dense, y, hp
      layer level: E ~ 0.3 N(0,1), W, b, h, p_vec, mask (multiplier for keep 0.8), g, dE_up - g is ZERO for every
        example that has a hidden unit with |z| < KINK in float64 (`near` marks them, `zeroed` = their share);
      `model_min_abs_z`: the model-level case's hidden unit closest to its kink."""
    spec, sizes = C.plain_spec(F, Dn)
    g = torch.Generator().manual_seed(1000 + seed)
    rnd = C.rnd_stream(g)
    p = C.draw_front(rnd, spec, D, std=0.3)
    p["afm_attention_w"] = glorot(rnd, (D, T), D, T)
    p["afm_attention_b"] = rnd(T, std=0.1)
    p["afm_attention_h"] = (glorot(rnd, (T, 1), T, 1) * h_scale).float().double()
    p["afm_projection_p"] = glorot(rnd, (D, 1), D, 1)
    idx, dense, y = C.draw_batch(g, rnd, sizes, B, Dn)
    mask = (torch.rand(B, D, generator=g) < 0.8).to(torch.float64) / 0.8
    gl = rnd(B)
    dE_up = rnd(B, F, D, std=0.1)
    hp = dict(embedding_size=D, embedding_l2_reg=1e-3, linear_l2_reg=1e-3, att_factor=T, att_l2_reg=1e-3,
              att_dropout=att_dropout)
    E_model, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False)
    _, z_model = afm_hidden(E_model, p["afm_attention_w"], p["afm_attention_b"])
    E = rnd(B, F, D, std=0.3)  # the layer-level rows are drawn on their own: every example differs
    _, z = afm_hidden(E, p["afm_attention_w"], p["afm_attention_b"])
    near = (z.abs() < KINK).flatten(1).any(dim=1)
    gl = torch.where(near, torch.zeros_like(gl), gl)
    c = lambda t: t.to(dtype) if t.is_floating_point() else t  # noqa: E731
    return dict(spec=spec, p={k: c(v) for k, v in p.items()}, idx=idx, dense=c(dense), y=y, hp=hp,
                E=c(E), W=c(p["afm_attention_w"]), b=c(p["afm_attention_b"]), h=c(p["afm_attention_h"].reshape(-1)),
                p_vec=c(p["afm_projection_p"].reshape(-1)), mask=c(mask), g=c(gl), dE_up=c(dE_up),
                zeroed=float(near.double().mean()), near=near, model_min_abs_z=float(z_model.abs().min()))


def gpu_case(c, h_scale=1.0):
    """make_afm_case for a kernel-level (B, F, D, T) of GPU_CASES / RANGE_CASES."""
    B, F, D, T = c
    return make_afm_case(B, F, D, 0, T, seed=CASE_SEEDS.get(tuple(c), 0), h_scale=h_scale)


def layer_reference(case, use_mask, use_up, dtype=torch.float64):
    """afm_layer + autograd on a case's layer-level tensors in `dtype`: (logit, dE, dW, db, dh, dp) as float64."""
    E, W, b, h, p = (case[k].to(dtype).clone().requires_grad_(True) for k in ("E", "W", "b", "h", "p_vec"))
    mask = case["mask"].to(dtype) if use_mask else None
    y = afm_layer(E, W, b, h, p, mask)
    (y * case["g"].to(dtype)).sum().backward()
    dE = E.grad + (case["dE_up"].to(dtype) if use_up else 0)
    return tuple(t.detach().double() for t in (y, dE, W.grad, b.grad, h.grad, p.grad))
