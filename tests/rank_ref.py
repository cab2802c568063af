"""Float64 twin of the grouped ranking objectives (include/recman_hip_rank.h, csrc/rank.hip) on tests/ref_common.py: the
pairwise (RankNet / BPR) and listwise (ListNet softmax) terms, their closed-form gradients, the combination with the
pointwise head, and the seeded cases the kernel is held to.

Every function takes the logit `s` in the dtype it is to compute in: float64 is the reference, float32 the CPU
restatement whose own error sets the kernel's bound (tests/test_gpu_rank.py).  A group is SCORED when it holds both
classes (GAUC's rule, tests/gauc_ref.py); c_g is formed from Python integers in double."""
import math

import torch

from tests import ref_common as C

KINDS, NORMS = ("pairwise", "listwise"), ("pairs", "group")


def softplus_neg(d):
    """softplus(-d) = max(-d, 0) + log1p(exp(-|d|))."""
    return torch.clamp(-d, min=0) + torch.log1p(torch.exp(-d.abs()))


def step_neg(d):
    """The 0/1 loss the softplus smooths: [d < 0] + 0.5 [d = 0], d = s_pos - s_neg."""
    return (d < 0).to(d.dtype) + 0.5 * (d == 0).to(d.dtype)


def split(y, groups):
    """[(index tensor of the group's positives, of its negatives)] in ascending id order; groups None: one group."""
    y = y.reshape(-1)
    g = torch.zeros_like(y) if groups is None else groups.reshape(-1)
    out = []
    for gid in torch.unique(g).tolist():
        idx = (g == gid).nonzero().reshape(-1)
        out.append((idx[y[idx] == 1], idx[y[idx] != 1]))
    return out


def counts(y, groups):
    """dict(groups, scored_groups, pairs Q, pos P, weight W) as Python ints."""
    parts = split(y, groups)
    sc = [(len(p), len(n)) for p, n in parts if len(p) and len(n)]
    return dict(groups=len(parts), scored_groups=len(sc), pairs=sum(p * n for p, n in sc), pos=sum(p for p, _ in sc),
                weight=sum(p + n for p, n in sc))


def coef(kind, norm, P, N, tot):
    """c_g of a scored group with P positives and N negatives."""
    if norm == "pairs":
        return 1.0 / (tot["pairs"] if kind == "pairwise" else tot["pos"])
    return (P + N) / (tot["weight"] * P * (N if kind == "pairwise" else 1))


def rank_term(s, y, groups, kind, norm, pair_fn=softplus_neg):
    """L, differentiable in s (0 with no scored group)."""
    assert kind in KINDS and norm in NORMS
    s, tot = s.reshape(-1), counts(y, groups)
    L = s.sum() * 0
    for pos, neg in split(y, groups):
        P, N = len(pos), len(neg)
        if not (P and N):
            continue
        c = coef(kind, norm, P, N, tot)
        if kind == "pairwise":
            L = L + c * pair_fn(s[pos][:, None] - s[neg][None, :]).sum()
        else:
            L = L + c * (P * torch.logsumexp(s[torch.cat([pos, neg])], 0) - s[pos].sum())
    return L


def rank_grad(s, y, groups, kind, norm):
    """dL/ds in closed form; exactly +0.0 outside the scored groups."""
    s, tot = s.reshape(-1), counts(y, groups)
    g = torch.zeros_like(s)
    for pos, neg in split(y, groups):
        P, N = len(pos), len(neg)
        if not (P and N):
            continue
        c = coef(kind, norm, P, N, tot)
        if kind == "pairwise":
            sg = torch.sigmoid(-(s[pos][:, None] - s[neg][None, :]))
            g[pos] = -c * sg.sum(1)
            g[neg] = c * sg.sum(0)
        else:
            idx = torch.cat([pos, neg])
            g[idx] = c * P * torch.softmax(s[idx], 0)
            g[pos] = g[pos] - c
    return g


def combine(s, y, groups, kind, norm, alpha, grad_scale=1.0, dlogit_in=None, loss_in=None):
    """(loss, dlogit, L) of the contract: loss = (1 - alpha) loss_in + alpha L, dlogit = grad_scale ((1 - alpha)
    dlogit_in + alpha dL/ds), the pointwise parts taken as given (None: absent)."""
    L, g = rank_term(s, y, groups, kind, norm).detach(), rank_grad(s, y, groups, kind, norm)
    loss, d = alpha * L, alpha * g
    if loss_in is not None:
        loss = loss + (1 - alpha) * loss_in.to(s.dtype).reshape(())
    if dlogit_in is not None:
        d = d + (1 - alpha) * dlogit_in.to(s.dtype)
    return loss, grad_scale * d, L


def bce(s, y):
    """(mean log loss, its gradient) of the pointwise head (oracle.th_layers: Keras binary_crossentropy on the
    probability), at the logits s."""
    from oracle import th_layers as TL

    z = s.detach().clone().requires_grad_(True)
    loss = TL.create_loss(y.to(s.dtype).reshape(-1), TL.prediction(z.reshape(-1, 1), "classification"),
                          "classification")
    loss.backward()
    return loss.detach(), z.grad


def model_fwd_bwd(model, p, spec, idx, dense, y, hp):
    """Autograd (in p's precision) of an oracle model with the loss swapped for the combined one that hp configures
    (rank_loss, rank_group_by, rank_loss_weight, rank_norm): (loss, logit [B], pred [B], grads) like
    oracle.th_layers.fwd_bwd."""
    from oracle import th_layers as TL

    logit_fn, l2_fn = TL.MODELS[model]
    alpha, by = hp.get("rank_loss_weight", 0.5), hp.get("rank_group_by")
    groups = None if by is None else idx[:, list(spec.sparse_names).index(by)]

    def loss_fn(leaves):
        logit = logit_fn(leaves, spec, idx, dense, hp, True, None, mv=None)
        pred = TL.prediction(logit, "classification")
        data = (1 - alpha) * TL.create_loss(y, pred, "classification") + \
            alpha * rank_term(logit.reshape(-1), y, groups, hp["rank_loss"], hp.get("rank_norm", "group"))
        return data + l2_fn(leaves, spec, hp), logit, pred

    return C.fwd_bwd(loss_fn, p)


# ------------------------------------------------------------------------------------------------------- the cases
MAX_ID = 2 ** 32 - 1


def _layout(g, blocks):
    """blocks: [(number of groups, group size or (lo, hi))] laid out in ascending id order -> (ids [B], sizes)."""
    ids, sizes, nxt = [], [], 3
    for count, size in blocks:
        for _ in range(count):
            n = size if isinstance(size, int) else int(torch.randint(size[0], size[1] + 1, (1,), generator=g))
            ids += [nxt] * n
            sizes.append(n)
            nxt += 1 + int(torch.randint(0, 1 << 20, (1,), generator=g))
    return torch.tensor(ids, dtype=torch.int64), sizes


@C.memo
def make_case(name):
    """dict(s float64 [B] of float32 values, y int64, groups int64 or None, dlogit_in, loss_in) of a named case; the
    examples are in random order in the batch (the sorted layout is what the name describes)."""
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    rnd = C.rnd_stream(g)
    kind = CASES[name]
    scale, p_pos, groups = 1.0, 0.4, None
    if kind == "b1":
        groups = torch.tensor([7])
    elif kind == "b2":
        groups = torch.tensor([5, 5])
    elif kind == "single_class":
        groups, _ = _layout(g, [(60, (1, 9))])
    elif kind == "small":  # sizes 1..5 at B = 1000
        groups, sizes = _layout(g, [(400, (1, 5))])
        groups = groups[:1000]
    elif kind == "edge300":  # pairs up to sorted position 3900, then 300 across position 4096, then pairs
        groups, _ = _layout(g, [(1950, 2), (1, 300), (50, 2)])
    elif kind == "long700":  # sorted positions 400 .. 1100: its runs span more than two tiles of 256
        groups, _ = _layout(g, [(400, 1), (1, 700), (400, 1)])
    elif kind == "null777":
        groups = None
    elif kind == "extreme_ids":
        groups = torch.tensor([0] * 31 + [MAX_ID] * 33)
    elif kind == "saturated":
        groups, _ = _layout(g, [(40, (2, 20))])
        scale = 60.0
    elif kind == "ties":
        groups, _ = _layout(g, [(40, (1, 9))])
    B = 777 if groups is None else int(groups.shape[0])
    if groups is not None and B > 2:
        groups = groups[torch.randperm(B, generator=g)]
    s = (rnd(B) * scale).float().double()
    y = C.draw_labels(g, B, p_pos)
    if kind == "b2":
        y = torch.tensor([1, 0])
    if kind == "single_class":
        y = (groups % 2 == 1).long()
    if kind == "ties":
        s = torch.full((B,), 0.25, dtype=torch.float64)
    if kind == "extreme_ids":
        y[0], y[1], y[-1], y[-2] = 1, 0, 1, 0
    return dict(s=s, y=y, groups=groups, dlogit_in=rnd(B, std=1.0 / B), loss_in=(rnd(1).abs() + 0.3).float().double())


CASES = {"b1": "b1", "b2_one_pair": "b2", "single_class_groups": "single_class", "sizes_1_to_5_b1000": "small",
         "group_300_across_a_tile_edge": "edge300", "group_700_among_singletons": "long700", "no_ids_b777": "null777",
         "ids_0_and_max": "extreme_ids", "logits_x60": "saturated", "tied_logits": "ties"}
LN2 = math.log(2.0)
