"""CPU PyTorch restatement (dtype-generic) of the optimizer steps of csrc/optim.hip, and the seeded cases the tests
run them on.

TEST INFRASTRUCTURE.  The lazy row-wise step (rm_sparse_optimizer_step / rm_sparse_optimizer_step_rows), per step:

    G[r]  = sum over the occurrences o of row r of [dE_o | g_bias_o | g_lin_o * mask_f]        (D + 2 columns)
    G[r] += l2_emb * row[r] on the embedding columns, l2_lin * lin[r] on the linear entry      (once per touched row;
                                                                                                no l2 on the bias entry)
    Adam     m = b1 m + (1 - b1) G, v = b2 v + (1 - b2) G^2, p -= lr_t m / (sqrt(v) + eps)     (eps OUTSIDE the sqrt)
    Adagrad  v += G^2, p -= lr G / (sqrt(v) + eps)                                              (v starts at 0.1)
    SGD      p -= lr G

for the rows a step touches; every other row keeps parameters and state.  Skipped occurrences (id < 0, row >= R, or an
id beyond its field when the ids are sorted per field) contribute nothing.  `reset` rebuilds the state of the touched
rows first (Adam: m = v = 0 and lr_t of t = 1; Adagrad: v = 0.1).

Every hyper-parameter crosses the C ABI as a float, so reference() computes with the float32-ROUNDED values in
`dtype` (1 - beta is then exact in float32 as well, by Sterbenz); lr_t is formed in double from the rounded betas
and rounded to float32, as opt_args does.  f32_hyper=False keeps the literal values (recman_amd.optim.Optimizer's).

reference(case, torch.float32) is the yardstick of the bounds: the same restatement in float32, every run summed
sequentially in occurrence order (what the kernel's inline path does).  `mutate` restates it deliberately wrong;
tests/test_optim_host.py asserts that compare()'s bounds catch every such mutation and pass the plain restatement.
"""
import math
import os
import re

import numpy as np
import torch

from tests.ref_common import grad_measure_or_empty as grad_measure

KINDS = ("adam", "adagrad", "sgd")
ENTRIES = ("fields", "pairs", "rows")
WIDTHS = (8, 12, 16, 24, 32, 48, 64)

# the kernels' compile-time limits (csrc/optim.hip), restated: the GPU test asserts its launch arithmetic from them
K_LONG, K_SEG, K_POS, K_FLIGHT = 16, 128, 2, 8
K_BLOCK, DENSE_GRID_CAP = 256, 256 * 4   # rm_dense_optimizer_step: min(ceil(n / 256), 1024) blocks of 256

# run lengths that step 1 of every full case must hold (why: the table in tests/test_gpu_optim_kernels.py)
RUN_LENGTHS = (1, 2, 3, 16, 17, 18, 33, 127, 128, 129, 130, 256, 257, 512, 513, 641, 897, 1025)
# rows 0.. of field 0: 1, 2, 17 and 129 twice, starting once at an even and once at an odd sorted position
HEAD = (1, 1, 2, 3, 2, 17, 17, 129, 129)
F_FULL, B_FULL, B_STEP2 = 3, 2048, 151
SENTINEL = -7777.25                    # row columns D+6 .., and the m halves of Adagrad's moment array

MUTATIONS = ("drop_last", "segment_twice", "no_l2", "neighbour_v")


def f32(x):
    return float(np.float32(x))


def cdiv(a, b):
    return -(-a // b)


def kernel_constants():
    """The limits above as the source text of csrc/optim.hip states them today: a change there makes the tests say
    so instead of silently testing other paths than they name.  kLong and kPos are the DEFAULTS of RM_OPT_LONG and
    RM_OPT_POS, which sit inside #ifndef: a library built with -DRM_OPT_LONG / -DRM_OPT_POS (an experiment build;
    recman_amd.build passes neither) runs other paths than these numbers say, and this helper cannot see that."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recman_amd", "csrc",
                           "optim.hip")) as f:
        src = f.read()

    def one(pattern):
        found = re.findall(pattern, src)
        assert len(found) == 1, (pattern, found)
        return found[0]

    cap = one(r"dense_opt_kernel, dim3\(rm_grid_cap\(\(n \+ kBlock - 1\) / kBlock, (\d+) \* (\d+)\)\)")
    return dict(kLong=int(one(r"#define RM_OPT_LONG (\d+)")), kPos=int(one(r"#define RM_OPT_POS (\d+)")),
                kSeg=int(one(r"constexpr int kSeg = (\d+);")), kBlock=int(one(r"constexpr int kBlock = (\d+);")),
                kLongFlight=int(one(r"constexpr int kLongFlight = (\d+);")), dense_grid_cap=int(cap[0]) * int(cap[1]))


def group_lanes(D):
    """(G, GE, NG) of sparse_step's dispatch: GE float4 slices, G = the power of two >= GE + 2, NG groups a wave."""
    GE = D // 4
    G = 2
    while G < GE + 2:
        G <<= 1
    return G, GE, 64 // G


# ------------------------------------------------------------------------------------------- the moment layout
def interleave(m, v):
    """m, v [R, D] -> the kernel's moment row [m4 v4 | m4 v4 | ..] [R, 2 D]."""
    R, D = m.shape
    return torch.stack([m.reshape(R, D // 4, 4), v.reshape(R, D // 4, 4)], dim=2).reshape(R, 2 * D).contiguous()


def deinterleave(mom, D):
    R = mom.shape[0]
    q = mom.reshape(R, D // 4, 2, 4)
    return q[:, :, 0, :].reshape(R, D), q[:, :, 1, :].reshape(R, D)


def state_of(rows, mom, D, kind):
    """Kernel layout -> (p, m, v), each [R, D + 2] float64 on the CPU (m / v None where the kind has none)."""
    rows = rows.detach().cpu().double()
    p = rows[:, : D + 2].clone()
    if kind == "sgd":
        return p, None, None
    me, ve = deinterleave(mom.detach().cpu().double(), D)
    v = torch.cat([ve, rows[:, D + 4: D + 6]], dim=1)
    m = torch.cat([me, rows[:, D + 2: D + 4]], dim=1) if kind == "adam" else None
    return p, m, v


# ----------------------------------------------------------------------------------------------- the case builder
_LAYOUTS = {}   # (tail, skip_share, seed, run lengths) -> ids: the ids depend on nothing else (not on D, kind, entry)


def _layout(tail, skip_share, seed=0, run_lengths=RUN_LENGTHS):
    """Local ids of the three steps of a full case, [B, F] int64 with -1 for a skipped occurrence, and the field
    sizes.  Step 1: a run of every length in run_lengths - HEAD first in field 0, the others dealt to the emptiest
    field, longest first, and shuffled among filler runs of 1..12 and a few rows no occurrence names; row R - 1 holds
    the longest run (tail "long") or one of K_LONG (tail "inline").  Step 2: other ids, no run beyond K_LONG, every
    third row of a field left out.  Step 3: step 1's ids."""
    key = (tail, skip_share, seed, tuple(run_lengths))
    if key in _LAYOUTS:
        return _LAYOUTS[key]
    g = torch.Generator().manual_seed(1234 + seed)
    nskip = int(round(skip_share * B_FULL))
    assert set(HEAD) <= set(run_lengths) and max(run_lengths) > K_LONG
    last_run = max(run_lengths) if tail == "long" else K_LONG
    rest = sorted(set(run_lengths) - set(HEAD) - ({last_run} if tail == "long" else set()), reverse=True)
    dealt, load = [[] for _ in range(F_FULL)], [sum(HEAD)] + [0] * (F_FULL - 2) + [last_run]
    for L in rest:
        f = load.index(min(load))
        dealt[f].append(L)
        load[f] += L
    cols, sizes = [], []
    for f in range(F_FULL):
        fixed = dealt[f]
        last = [last_run] if f == F_FULL - 1 else []
        head = list(HEAD) if f == 0 else []
        room = B_FULL - nskip - sum(head) - sum(fixed) - sum(last)
        assert room >= 0
        fill = []
        while room > 0:
            c = min(room, int(torch.randint(1, 13, (1,), generator=g)))
            fill.append(c)
            room -= c
        mid = fixed + fill + [0] * 3   # (0: a row no step-1 occurrence names)
        mid = [mid[i] for i in torch.randperm(len(mid), generator=g).tolist()]
        lens = head + mid + last
        ids = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
        ids = torch.cat([ids, torch.full((nskip,), -1, dtype=torch.int64)])
        assert ids.numel() == B_FULL
        cols.append(ids[torch.randperm(B_FULL, generator=g)])
        sizes.append(len(lens))
    step1 = torch.stack(cols, 1)
    cols = []
    skip2 = 10 if nskip else 0
    for f in range(F_FULL):
        allowed = [r for r in range(sizes[f]) if r % 3 != 0]
        allowed = [allowed[i] for i in torch.randperm(len(allowed), generator=g).tolist()]
        want, ids = B_STEP2 - skip2, []
        for j, r in enumerate(allowed):
            c = K_LONG if j == 0 else int(torch.randint(1, K_LONG + 1, (1,), generator=g))
            c = min(c, want - len(ids))
            ids += [r] * c
            if len(ids) == want:
                break
        assert len(ids) == want, "step 2 needs more rows"
        ids = torch.tensor(ids + [-1] * skip2, dtype=torch.int64)
        cols.append(ids[torch.randperm(B_STEP2, generator=g)])
    step2 = torch.stack(cols, 1)
    _LAYOUTS[key] = ([step1, step2, step1.clone()], sizes)
    return _LAYOUTS[key]


def _encode_skips(local, sizes, entry):
    """The entry's own spelling of a skipped occurrence: negative ids, and ids at or beyond the limit the entry
    checks (the field's size; R - field_off[f]; R for "rows", whose skipped ids are taken as they are)."""
    B, F = local.shape
    R = int(sum(sizes))
    foff = torch.tensor([0] + list(np.cumsum(sizes)[:-1]), dtype=torch.int64)
    limit = {"fields": torch.tensor(sizes, dtype=torch.int64), "pairs": R - foff,
             "rows": torch.full((F,), R, dtype=torch.int64)}[entry]
    out = local.clone()
    pos = (local < 0).nonzero()
    for j, (b, f) in enumerate(pos.tolist()):
        out[b, f] = (-1, int(limit[f]), -5, int(limit[f]) + 7, 1 << 33)[j % 5]
    return out, foff


def assemble(D, kind, entry, sizes, id_steps, seed=0, ld=None, gw=None, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-7,
             l2_emb=0.0, l2_lin=0.0, lin_mask=None, no_bias=False, no_lin=False, step0=1, reset_at=(),
             prepared_at=(2,), name=None):
    """A case from explicit local ids (one [B, F] int64 tensor per step, -1 = skipped).  Every float is a float32
    number.  rows0 [R, ld]: unit-normal parameters, the state columns D+2..D+5 at their initial values (SENTINEL where
    the kind has no such state: all four under SGD, m_b and m_l under Adagrad), SENTINEL beyond; mom0 [R, 2 D]
    (Adagrad: the m halves hold SENTINEL)."""
    assert kind in KINDS and entry in ENTRIES
    R, F = int(sum(sizes)), len(sizes)
    ld = 2 * D if ld is None else ld
    gw = D + 4 if gw is None else gw
    g = torch.Generator().manual_seed(4321 + 17 * D + seed)
    rows0 = torch.randn(R, ld, generator=g)
    rows0[:, D + 6:] = SENTINEL
    rows0[:, D + 2: D + 6] = 0.0
    mom0 = None
    if kind == "adagrad":
        rows0[:, D + 2: D + 4] = SENTINEL   # m_b, m_l: Adagrad has no first moment, the kernel must not write them
        rows0[:, D + 4: D + 6] = 0.1
        mom0 = interleave(torch.full((R, D), SENTINEL), torch.full((R, D), 0.1))
    elif kind == "adam":
        mom0 = torch.zeros(R, 2 * D)
    else:
        rows0[:, D + 2: D + 6] = SENTINEL
    steps = []
    for local in id_steps:
        B = local.shape[0]
        idx, foff = _encode_skips(local, sizes, entry)
        st = dict(B=B, d_rows=torch.randn(B, F, D, generator=g), g_bias=torch.randn(B, generator=g),
                  g_lin=torch.randn(B, generator=g))
        if entry == "rows":
            ok = local >= 0
            st["ids"] = torch.where(ok, idx + foff, idx).reshape(-1).contiguous()
            packed = torch.full((B * F, gw), SENTINEL)   # (columns D+2.. are padding the kernel must not read)
            packed[:, :D] = st["d_rows"].reshape(-1, D)
            packed[:, D] = 0.0 if no_bias else st["g_bias"].repeat_interleave(F)
            lm = torch.ones(F) if lin_mask is None else torch.tensor(lin_mask, dtype=torch.float32)
            packed[:, D + 1] = 0.0 if no_lin else (st["g_lin"][:, None] * lm[None, :]).reshape(-1)
            st["packed"] = packed
        else:
            st["idx"] = idx
        steps.append(st)
    return dict(name=name, D=D, kind=kind, entry=entry, sizes=list(sizes), R=R, F=F, ld=ld, gw=gw, foff=foff,
                max_field_rows=max(sizes) if entry == "fields" else 0, rows0=rows0, mom0=mom0, steps=steps,
                lr=lr, beta1=beta1, beta2=beta2, eps=eps, l2_emb=l2_emb, l2_lin=l2_lin, lin_mask=lin_mask,
                no_bias=no_bias, no_lin=no_lin, step0=step0, reset_at=tuple(reset_at), prepared_at=tuple(prepared_at),
                # what the occurrences' rows and gradients depend on (not the kind, not the entry)
                data_key=(D, seed, ld, tuple(hash(x.numpy().tobytes()) for x in id_steps)))


def make_case(D, kind, entry, tail="long", skip_share=0.06, seed=0, run_lengths=RUN_LENGTHS, **opts):
    """A full case: three steps over a few hundred rows in three fields, 6,144 occurrences in step 1 (shuffled, so
    occurrence order is not row order).  Same (D, seed): the same occurrences and gradients for every kind and entry."""
    id_steps, sizes = _layout(tail, skip_share, seed, run_lengths)
    return assemble(D, kind, entry, sizes, id_steps, seed=seed, **opts)


def small_case(which, D, kind, entry):
    """The smallest occurrence lists: one step each."""
    t = lambda x: torch.tensor(x, dtype=torch.int64)  # noqa: E731
    sizes, ids = {
        "n1": ([5], t([[3]])),
        "n2_same_row": ([5], t([[2], [2]])),
        "n_odd": ([4, 3], None),
        "all_skipped": ([4, 3], t([[-1, -1]] * 9)),
        "empty": ([4, 3], torch.zeros(0, 2, dtype=torch.int64)),
    }[which]
    if which == "n_odd":   # n = 7 x 1 would do for "rows"; [B, F] batches need an odd B and an odd F
        sizes, ids = [4, 3, 6], t([[0, 2, 5], [3, 2, -1], [0, 0, 5], [1, 2, 0], [3, -1, 5]])
    return assemble(D, kind, entry, sizes, [ids], seed=99, prepared_at=(), name=which)


# ------------------------------------------------------------------------------------ what the kernels are handed
def occurrence_rows(case, s):
    """Global table row of every occurrence of step s, -1 for a skipped one: the entry's own rule."""
    st, R = case["steps"][s], case["R"]
    if case["entry"] == "rows":
        ids = st["ids"]
        return torch.where((ids >= 0) & (ids < R), ids, torch.full_like(ids, -1))
    idx, foff = st["idx"], case["foff"]
    if case["entry"] == "fields":
        ok = (idx >= 0) & (idx < torch.tensor(case["sizes"])[None, :])
    else:
        ok = (idx >= 0) & (idx + foff[None, :] < R)
    return torch.where(ok, idx + foff[None, :], torch.full_like(idx, -1)).reshape(-1)


def occurrence_grads(case, s):
    """[n, D + 2] float32: [dE | g_bias | g_lin * mask] of every occurrence of step s."""
    st, D, F = case["steps"][s], case["D"], case["F"]
    if case["entry"] == "rows":
        return st["packed"][:, : D + 2].clone()
    B = st["B"]
    gb = torch.zeros(B) if case["no_bias"] else st["g_bias"]
    gl = torch.zeros(B) if case["no_lin"] else st["g_lin"]
    lm = torch.ones(F) if case["lin_mask"] is None else torch.tensor(case["lin_mask"], dtype=torch.float32)
    return torch.cat([st["d_rows"].reshape(B * F, D), gb.repeat_interleave(F)[:, None],
                      (gl[:, None] * lm[None, :]).reshape(-1, 1)], dim=1)


def sorted_keys(case, s):
    """The sorted key list as the apply kernels read it (R = skipped): all rows ascending, then the skipped
    ("pairs", "rows"); field f at [f B, (f + 1) B) with its skipped ids at the end of its block ("fields")."""
    keys = occurrence_rows(case, s)
    keys = torch.where(keys < 0, torch.full_like(keys, case["R"]), keys)
    if case["entry"] != "fields":
        return keys[torch.argsort(keys, stable=True)]
    k = keys.reshape(-1, case["F"])
    return torch.cat([k[:, f][torch.argsort(k[:, f], stable=True)] for f in range(case["F"])])


def runs_of(keys, R):
    """[(start, length, row)] of the runs of equal keys < R in a sorted list."""
    k = keys.tolist()
    out, i = [], 0
    while i < len(k):
        j = i
        while j < len(k) and k[j] == k[i]:
            j += 1
        if k[i] < R:
            out.append((i, j - i, k[i]))
        i = j
    return out


# -------------------------------------------------------------------------------------------------- the restatement
# run_sums' results by what the occurrences' rows and gradients depend on.  The kind and the entry are NOT in the key:
# the three entries spell the same occurrences (tests/test_optim_host.py::test_entries_hold_the_same_occurrences, at
# every width), so their cases share the float32 sums - the only slow part of a reference.
_SUMS = {}


def run_sums(case, s, dtype, mutate=None):
    """G [R, D + 2] and the touched mask.  float64: index_add.  float32: each run summed sequentially in occurrence
    order.  mutate "drop_last": runs longer than K_LONG lose their last member; "segment_twice": runs longer than
    K_SEG get their second segment (members K_SEG .. 2 K_SEG - 1) added twice."""
    mutate = mutate if mutate in ("drop_last", "segment_twice") else None
    key = (case["data_key"], case["lin_mask"] and tuple(case["lin_mask"]), case["no_bias"], case["no_lin"], s, dtype,
           mutate)
    if key in _SUMS:
        return _SUMS[key]
    R, D = case["R"], case["D"]
    rows = occurrence_rows(case, s)
    keep = (rows >= 0).nonzero().reshape(-1)
    rows, g = rows[keep], occurrence_grads(case, s)[keep].to(dtype)
    touched = torch.zeros(R, dtype=torch.bool)
    touched[rows] = True
    order = torch.argsort(rows, stable=True)           # by row, occurrence order inside a run
    rows, g = rows[order], g[order]
    n = rows.numel()
    start = torch.zeros(n, dtype=torch.int64)
    if n:
        head = torch.ones(n, dtype=torch.bool)
        head[1:] = rows[1:] != rows[:-1]
        first = head.nonzero().reshape(-1)
        start = first[torch.cumsum(head.long(), 0) - 1]
    rank = torch.arange(n) - start
    length = torch.zeros(R, dtype=torch.int64).index_add_(0, rows, torch.ones(n, dtype=torch.int64))[rows]
    if mutate == "drop_last":
        sel = ~((length > K_LONG) & (rank == length - 1))
        rows, g, rank = rows[sel], g[sel], rank[sel]
    elif mutate == "segment_twice":
        twice = (length > K_SEG) & (rank >= K_SEG) & (rank < 2 * K_SEG)
        rows, g = torch.cat([rows, rows[twice]]), torch.cat([g, g[twice]])
        rank = torch.cat([rank, rank[twice] + (1 << 20)])
    G = torch.zeros(R, D + 2, dtype=dtype)
    if dtype == torch.float64:
        G.index_add_(0, rows, g)
    else:
        by_rank = torch.argsort(rank, stable=True)
        rows, g, rank = rows[by_rank], g[by_rank], rank[by_rank]
        cuts = (torch.nonzero(rank[1:] != rank[:-1]).reshape(-1) + 1).tolist() if rank.numel() else []
        for a, b in zip([0] + cuts, cuts + [rank.numel()]):
            G[rows[a:b]] += g[a:b]                      # (one member of every run still open: distinct rows)
    _SUMS[key] = (G, touched)
    return _SUMS[key]


def lr_t_of(case, t, f32_hyper=True):
    r = f32 if f32_hyper else float
    v = r(case["lr"]) * math.sqrt(1.0 - r(case["beta2"]) ** t) / (1.0 - r(case["beta1"]) ** t)
    return r(v)


def update(kind, p, m, v, G, dtype, lr, lr_t, b1, b2, eps, reset):
    """The Keras rule of opt_update on whole arrays: new (p, m, v)."""
    if kind == "adam":
        if reset:
            m, v = torch.zeros_like(m), torch.zeros_like(v)
        m = b1 * m + (1.0 - b1) * G
        v = b2 * v + (1.0 - b2) * G * G
        p = p - lr_t * m / (v.sqrt() + eps)
    elif kind == "adagrad":
        if reset:
            v = torch.full_like(v, f32(0.1))
        v = v + G * G
        p = p - lr * G / (v.sqrt() + eps)
    else:
        p = p - lr * G
    return p, m, v


def reference(case, dtype=torch.float64, mutate=None, f32_hyper=True):
    """[(p, m, v) after step s, s = 0, 1, ..], each [R, D + 2] as float64 (m / v None where the kind has none)."""
    D, kind = case["D"], case["kind"]
    r = f32 if f32_hyper else float
    p0, m0, v0 = state_of(case["rows0"], case["mom0"], D, kind)
    p = p0.to(dtype)
    m = torch.zeros_like(p) if m0 is None else m0.to(dtype)
    v = torch.zeros_like(p) if v0 is None else v0.to(dtype)
    l2e, l2l = (0.0, 0.0) if mutate == "no_l2" else (r(case["l2_emb"]), r(case["l2_lin"]))
    out = []
    for s in range(len(case["steps"])):
        G, touched = run_sums(case, s, dtype, mutate)
        G = G.clone()
        G[:, :D] += l2e * p[:, :D]
        G[:, D + 1] += l2l * p[:, D + 1]
        reset = s in case["reset_at"]
        v_in = v
        if mutate == "neighbour_v":   # the side entries read the v of the last embedding slice
            v_in = v.clone()
            v_in[:, D: D + 2] = v[:, D - 4: D - 2]
        pn, mn, vn = update(kind, p, m, v_in, G, dtype, r(case["lr"]),
                            lr_t_of(case, 1 if reset else case["step0"] + s, f32_hyper), r(case["beta1"]),
                            r(case["beta2"]), r(case["eps"]), reset)
        tm = touched[:, None]
        p, m, v = torch.where(tm, pn, p), torch.where(tm, mn, m), torch.where(tm, vn, v)
        out.append((p.double(), m.double() if kind == "adam" else None, v.double() if kind != "sgd" else None))
    return out


def dense_reference(p0, grads, kind, dtype=torch.float64, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-7, reset_at=()):
    """rm_dense_optimizer_step restated: [(p, m, v) after every step], step s at t = s + 1."""
    case = dict(lr=lr, beta1=beta1, beta2=beta2)
    p = p0.to(dtype)
    m, v = torch.zeros_like(p), torch.full_like(p, f32(0.1) if kind == "adagrad" else 0.0)
    out = []
    for s, g in enumerate(grads):
        reset = s in reset_at
        p, m, v = update(kind, p, m, v, g.to(dtype), dtype, f32(lr), lr_t_of(case, 1 if reset else s + 1),
                         f32(beta1), f32(beta2), f32(eps), reset)
        out.append((p.double(), m.double() if kind == "adam" else None, v.double() if kind != "sgd" else None))
    return out


# ------------------------------------------------------------------------------------------------------ the bounds
def compare(got, want, ref32, D, tag="", show=True):
    """The bounds of tests/test_gpu_optim_kernels.py on one state (p, m, v) against float64 `want`, with the float32
    restatement `ref32` as the yardstick.  Parameters: max abs error <= max(5e-6 max(1, max|want|), 4 x the
    restatement's); moments (embedding and side entries apart): grad_measure <= max(2e-5, 4 x the restatement's).
    Returns [(quantity, value, restatement's value, bound)] of what FAILS."""
    bad, lines = [], []
    # (D None: a flat buffer, one part)
    parts = (("", slice(None)),) if D is None else (("_emb", slice(0, D)), ("_side", slice(D, D + 2)))
    e, e32 = float((got[0] - want[0]).abs().max()), float((ref32[0] - want[0]).abs().max())
    bound = max(5e-6 * max(1.0, float(want[0].abs().max())), 4 * e32)
    lines.append(("p", e, e32, bound))
    for name, i in (("m", 1), ("v", 2)):
        if want[i] is None:
            continue
        for part, sl in parts:
            x, x32 = grad_measure(got[i][:, sl], want[i][:, sl]), grad_measure(ref32[i][:, sl], want[i][:, sl])
            lines.append((name + part, x, x32, max(2e-5, 4 * x32)))
    for q in lines:
        if show:
            print(f"{tag}: {q[0]} {q[1]:.2e}, float32 restatement {q[2]:.2e}, bound {q[3]:.2e}")
        if not q[1] <= q[3]:
            bad.append(q)
    return bad


# -------------------------------------------------------------------------- the cases of the GPU file, by their names
SPARSE_CASES = {f"d{D}_{kind}_{entry}": dict(D=D, kind=kind, entry=entry)
                for D in WIDTHS for kind in KINDS for entry in ENTRIES}
# the sorted list ENDS with a run (no skipped id anywhere): a handed-over one, an inline one
END_CASES = {f"d{D}_{kind}_{entry}_ends_{tail}": dict(D=D, kind=kind, entry=entry, tail=tail, skip_share=0.0)
             for D, kind in ((8, "adam"), (24, "sgd"), (64, "adagrad")) for entry in ENTRIES
             for tail in ("long", "inline")}
OPTION_CASES = {}
for _D in (12, 32, 64):
    _o = {
        "reset_adam": dict(kind="adam", entry="fields", reset_at=(2,)),
        "reset_adagrad": dict(kind="adagrad", entry="pairs", reset_at=(2,)),
        "reset_adam_rows": dict(kind="adam", entry="rows", reset_at=(2,)),
        "l2_adam": dict(kind="adam", entry="fields", l2_emb=3e-2, l2_lin=2e-2),
        "l2_adagrad": dict(kind="adagrad", entry="rows", l2_emb=3e-2, l2_lin=2e-2),
        "l2_sgd": dict(kind="sgd", entry="pairs", l2_emb=3e-2, l2_lin=2e-2),
        "lin_mask_adam": dict(kind="adam", entry="fields", lin_mask=(1.0, 0.0, 1.0), l2_lin=2e-2),
        "lin_mask_sgd": dict(kind="sgd", entry="pairs", lin_mask=(1.0, 0.0, 1.0), l2_lin=2e-2),
        "no_bias_adam": dict(kind="adam", entry="fields", no_bias=True),
        "no_lin_adagrad": dict(kind="adagrad", entry="pairs", no_lin=True),
        "no_bias_no_lin_adam": dict(kind="adam", entry="pairs", no_bias=True, no_lin=True),
        "no_bias_no_lin_sgd": dict(kind="sgd", entry="fields", no_bias=True, no_lin=True),
        "ld_d8_adam": dict(kind="adam", entry="fields", ld=_D + 8),
        "ld_d12_adagrad": dict(kind="adagrad", entry="rows", ld=_D + 12),
        "ld_d12_sgd": dict(kind="sgd", entry="pairs", ld=_D + 12),
        "hyper_adam": dict(kind="adam", entry="rows", lr=0.037, beta1=0.8, beta2=0.95, eps=1e-5),
        "hyper_adagrad": dict(kind="adagrad", entry="fields", lr=0.2, eps=1e-3),
        "step1000_adam": dict(kind="adam", entry="pairs", step0=1000),
        "gw_d8_adam": dict(kind="adam", entry="rows", gw=_D + 8),
        "gw_d8_sgd": dict(kind="sgd", entry="rows", gw=_D + 8),
    }
    for _k, _v in _o.items():
        OPTION_CASES[f"d{_D}_{_k}"] = dict(D=_D, **_v)
ALL_CASES = {**SPARSE_CASES, **END_CASES, **OPTION_CASES}
