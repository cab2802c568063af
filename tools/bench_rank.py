#!/usr/bin/env python
"""Times rm_rank_loss (hipEvents, warm clocks, 50 timed calls, min / median / mean) at B = 65536 beside
  - the comparator: the same arithmetic composed from torch ops in fp32 - a sort-free segment form (torch.unique,
    bincount, scatter_reduce, index_add) for the listwise term, and for the pairwise term the examples of every group
    padded to [groups, max positives] and [groups, max negatives] and one masked pair block [groups, max positives, max
    negatives], forward + autograd backward.  Where that block has more than 2^28 entries the comparator runs at
    B = 8192 and the record says so (`composed_B`);
and Engine.fwd_bwd of DeepFM and DCN with a ranking term beside the same engines without one: the plain step (for
DeepFM the one-kernel step) and DeepFM on the multi-kernel path with rm_logit_loss (step_fusion and the fused head
off) - the path the ranking term runs on.  With rank_loss unset no new code runs, so the plain steps are the parent
commit's.  All contenders of a setting alternate in one process.
    python tools/bench_rank.py [--json out.json] [--kernels-only | --step-only]
Inputs: about 3 % and 50 % positives; ids: none (one group of B), Zipf (exponent 1) and uniform over 8192 ids.  Pair
evaluations are 2 P_g N_g per group (every pair is evaluated from both sides).
`--kernels-only` launches nothing but rm_rank_loss, `--step-only` nothing but the engines' steps."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recman_amd import engine as eng
from recman_amd import ops
from tools._bench import alternate, main

B, IDS = 65536, 8192
COMPOSED_MAX = 1 << 28  # entries of the comparator's pair block (1 GiB per fp32 temporary)


def draw_ids(kind, n, g):
    if kind == "none":
        return None
    if kind == "uniform":
        return torch.randint(0, IDS, (n,), generator=g)
    w = 1.0 / torch.arange(1, IDS + 1, dtype=torch.float64)  # Zipf, exponent 1
    return torch.multinomial(w, n, replacement=True, generator=g)


def composed(s, y, groups, kind, norm):
    """(L, dL/ds) as a user would compose them from torch ops."""
    sl = s.detach().clone().requires_grad_(True)
    inv = torch.zeros_like(y) if groups is None else torch.unique(groups, return_inverse=True)[1]
    ng = int(inv.max()) + 1
    n_g = torch.bincount(inv, minlength=ng)
    P_g = torch.bincount(inv, weights=y.double(), minlength=ng).long()
    N_g = n_g - P_g
    scored = (P_g > 0) & (N_g > 0)
    pairs = kind == "pairwise"
    if norm == "pairs":
        c = torch.full((ng,), 1.0 / float(((P_g * N_g) if pairs else P_g)[scored].sum()), device=s.device)
    else:
        c = (n_g.double() / (float(n_g[scored].sum()) * P_g.double() * (N_g.double() if pairs else 1.0))).float()
    c = torch.where(scored, c, torch.zeros_like(c))
    if not pairs:
        mx = torch.zeros(ng, device=s.device).scatter_reduce(0, inv, sl.detach(), "amax", include_self=False)
        lse = mx + torch.log(torch.zeros(ng, device=s.device).index_add(0, inv, torch.exp(sl - mx[inv])))
        L = (c[inv] * y * (lse[inv] - sl)).sum()
    else:
        order = torch.argsort(inv * 2 + y, stable=True)  # a group's negatives, then its positives
        si, yi, gi = sl[order], y[order], inv[order]
        start = torch.cumsum(n_g, 0) - n_g
        at = torch.arange(s.shape[0], device=s.device) - start[gi]
        Ln, Lp = int(N_g.max()), int(P_g.max())
        at_n, at_p = (gi[yi == 0], at[yi == 0]), (gi[yi == 1], (at - N_g[gi])[yi == 1])
        neg = torch.zeros(ng, max(Ln, 1), device=s.device).index_put(at_n, si[yi == 0])
        pos = torch.zeros(ng, max(Lp, 1), device=s.device).index_put(at_p, si[yi == 1])
        one = torch.ones(1, device=s.device)
        m_n = torch.zeros_like(neg).index_put(at_n, one)
        m_p = torch.zeros_like(pos).index_put(at_p, one)
        d = pos[:, :, None] - neg[:, None, :]
        term = (torch.clamp(-d, min=0) + torch.log1p(torch.exp(-d.abs()))) * (m_p[:, :, None] * m_n[:, None, :])
        L = (c * term.sum((1, 2))).sum()
    L.backward()
    return L.detach(), sl.grad


def block_entries(y, groups):
    inv = torch.zeros_like(y) if groups is None else torch.unique(groups, return_inverse=True)[1]
    n_g = torch.bincount(inv)
    P_g = torch.bincount(inv, weights=y.double()).long()
    return int(n_g.shape[0]) * int(P_g.max()) * int((n_g - P_g).max())


def kernel_record(share, ids, kind, comparator):
    g = torch.Generator().manual_seed(0)
    s = torch.randn(B, generator=g).cuda()
    y = (torch.rand(B, generator=g) < share).long().cuda()
    gr = draw_ids(ids, B, g)
    gr = None if gr is None else gr.cuda()
    d_in, loss = torch.randn(B, generator=g).cuda() / B, torch.ones(1, device="cuda")
    d, out = torch.empty(B, device="cuda"), torch.zeros(7, dtype=torch.int64, device="cuda")
    ws = torch.empty(ops.rank_loss_workspace(B), dtype=torch.uint8, device="cuda")
    run = lambda: ops.rank_loss(s, y, gr, kind, "group", 0.5, d, dlogit_in=d_in, loss_in=loss, loss_out=None,  # noqa: E731
                                out=out, workspace=ws)
    fns, names = [run], ["ms"]
    rec = dict(B=B, positives=share, ids=ids, kind=kind)
    if comparator:
        n = B if kind == "listwise" or block_entries(y, gr) <= COMPOSED_MAX else 8192
        sc, yc, gc = s[:n].contiguous(), y[:n].contiguous(), None if gr is None else gr[:n].contiguous()
        if kind == "pairwise" and block_entries(yc, gc) > COMPOSED_MAX:
            n = 0
        if n:
            fns.append(lambda: composed(sc, yc, gc, kind, "group"))
            names.append("composed_ms")
            rec["composed_B"] = n
    rec.update(zip(names, alternate(fns)))
    run()
    torch.cuda.synchronize()
    value, groups, scored, pairs, pos, weight, flags = ops.read_rank_loss(out)
    rec.update(groups=groups, scored_groups=scored, pairs=pairs, pair_evaluations=2 * pairs, flags=flags)
    if kind == "pairwise" and pairs:
        rec["pair_evaluations_per_s"] = round(2 * pairs / (rec["ms"]["median"] * 1e-3), 0)
    if comparator and rec.get("composed_B") == B:
        L, grad = composed(s, y, gr, kind, "group")
        only = torch.empty(B, device="cuda")
        ops.rank_loss(s, y, gr, kind, "group", 1.0, only, workspace=ws)
        rec["max_rel_grad_diff_vs_composed"] = float((only - grad).abs().max() / grad.abs().max())
        rec["rel_loss_diff_vs_composed"] = abs(value - float(L)) / abs(float(L))
    return rec


def kernels(comparator=True):
    return [kernel_record(share, ids, kind, comparator) for kind in ("pairwise", "listwise")
            for share in (0.03, 0.5) for ids in ("none", "zipf", "uniform")]


def steps():
    g = torch.Generator().manual_seed(0)
    F, Dn = 26, 13
    sizes = [IDS] + [40000] * (F - 1)  # C0: the group feature, uniform over 8192 ids
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in sizes], 1).cuda()
    dense = torch.randn(B, Dn, generator=g).cuda()
    y = (torch.rand(B, generator=g) < 0.3).long().cuda()
    spec = eng.FeatureSpec([f"C{i}" for i in range(F)], sizes, [f"I{j}" for j in range(Dn)])
    base = dict(embedding_size=16, deep_hidden_units=(32, 32), deep_activation="relu")
    rank = lambda kind: dict(rank_loss=kind, rank_group_by="C0", rank_loss_weight=0.5)  # noqa: E731

    def engine(model, hp, fuse_head=True):
        e = eng.ENGINES[model](spec, 16, dict(base, **hp))
        eng.init_reference(e, 2019)
        e.fuse_head = fuse_head
        return lambda: e.fwd_bwd(idx, dense, y)

    res = {"shape": dict(B=B, F=F, D=16, Dn=Dn, hidden=(32, 32), group_ids=IDS, positives=0.3)}
    names = ["plain", "multi_kernel", "pairwise", "listwise"]
    fns = [engine("deepfm", dict(step_fusion=True)), engine("deepfm", dict(step_fusion=False, front_fusion=False), False),
           engine("deepfm", dict(step_fusion=True, **rank("pairwise"))),
           engine("deepfm", dict(step_fusion=True, **rank("listwise")))]
    res["deepfm_ms"] = dict(zip(names, alternate(fns)))
    dcn = dict(cross_layer_num=3)
    fns = [engine("dcn", dcn), engine("dcn", dcn, False), engine("dcn", dict(dcn, **rank("pairwise"))),
           engine("dcn", dict(dcn, **rank("listwise")))]
    res["dcn_ms"] = dict(zip(["plain", "unfused_head", "pairwise", "listwise"], alternate(fns)))
    for m in ("deepfm_ms", "dcn_ms"):
        t = res[m]
        res[m.replace("_ms", "_pairwise_over_plain")] = round(t["pairwise"]["median"] / t["plain"]["median"], 2)
    return res


if __name__ == "__main__":
    main(kernels, steps)
