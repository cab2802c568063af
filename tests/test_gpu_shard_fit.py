"""GPU: the layer users call on a row-sharded table - DeepModel.fit(), fit_on_batch(), predict() and
_fit_sharded_batch (recman_amd/th/DeepModel.py) - held against BOTH

  * tests/shard_fit_ref.py, the float64 restatement of the sharded training loop, and
  * a one-GPU twin of the same class with table_sharding="none" and sparse_optimizer=True (the same row-wise rule),

on the ml-100k golden slice: D = 16, batch 96, one epoch of at most 12 steps, dropout off, Adam at 0.01.  The twin is
built first and loads a seeded start (tests/test_shard_fit_host.host_params); the sharded model takes the twin's
initial rows (ShardedTable.load_global) and dense variables, and so does the float64 loop.  Compared: the shard's rows (local row i is global row i * world + rank), every dense
variable, the per-step losses, predict() on the frame.

Every case proves whether a fixed-capacity batch overflowed: on the host before the run (ShardedTable.capacity against
the occurrences of every batch; recman_amd.dist.route_torch on two ranks) and through the engine's flag path during it
- e.fwd_bwd is wrapped, so a batch that was redone shows two calls, the second with exact split sizes.

Bounds.  Against float64: 4 x the deviation of the float32 CPU restatement from the float64 one, measured per case by
tests/test_shard_fit_host.py (TWIN_DRIFT below; the GPU sums in another order than the CPU twin); losses 2e-5.
Against the twin: 4 x the worst difference measured over the epoch on the first green run (VS_TWIN below), and never
below one float32 ulp at the scale max(1, |w|) - no bound under the format's resolution can hold across two
summation orders; tests/test_gpu_dist.py applies 1e-6 max(1, |w|) and 2e-5 on losses after three steps.
profiles/shard_fit.md has every number.
"""
import datetime
import os
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import shard_fit_ref as R
from tests.test_shard_fit_host import (BATCH, D, LAZY_L2, NO_L2, SEED, SKEW_PART, TWO_RANK, encode, host_params, make_model,
                                       ml_case, oracle_model, skew_batches, skew_steps)

pytestmark = pytest.mark.gpu
L2 = {"no_l2": NO_L2, "lazy_l2": LAZY_L2}
ULP = 2.0 ** -23
LOSS_F64 = 2e-5
MODELS = ("deepfm", "dcn", "xdeepfm", "deepfm_genres")

# float32 CPU restatement against the float64 one, (parameters as |d| / max(1, max|w|), predictions as |d|) after the
# case's run: printed by tests/test_shard_fit_host.py (test_float32_twin_drift_*) from the very start the models load
TWIN_DRIFT = {
    ("deepfm", "no_l2"): (3.21e-07, 1.01e-07), ("deepfm", "lazy_l2"): (3.03e-07, 1.06e-07),
    ("dcn", "no_l2"): (2.45e-07, 8.34e-08), ("dcn", "lazy_l2"): (2.50e-07, 8.88e-08),
    ("xdeepfm", "no_l2"): (2.07e-07, 8.59e-08), ("xdeepfm", "lazy_l2"): (1.78e-07, 9.79e-08),
    ("deepfm_genres", "no_l2"): (8.11e-07, 9.78e-08), ("deepfm_genres", "lazy_l2"): (7.07e-07, 8.71e-08),
    ("deepfm_genres", "964"): (5.45e-07, 1.38e-07),
    "xdeepfm_fit_ragged_fixed_micro2": (2.31e-07, 8.12e-08), "deepfm_genres_fit_dynamic": (4.51e-07, 1.01e-07),
    "deepfm_one_rank_overflows": (1.08e-07, 9.49e-08), "deepfm_genres_one_rank_overflows_micro2": (7.92e-07, 1.16e-07),
}
# sharded model against the one-GPU twin, (parameters, losses, predictions): the worst difference over the run as
# measured on the first green run (0.0: bit for bit - the exact-split sharded step at world size 1 IS the twin's
# arithmetic; with the lazy l2 the sharded loss leaves out the l2 value of the linear term's dense weights, up to
# 1.8e-07 of the loss here); two ranks: the worse rank.  A case without an entry would get the three-step bounds of
# tests/test_gpu_dist.py
VS_TWIN = {
    "deepfm-dynamic": (0.00e+00, 0.00e+00, 0.00e+00),
    "deepfm-fixed_micro2": (4.92e-07, 1.19e-07, 1.19e-07),
    "deepfm-lazy_l2": (0.00e+00, 5.96e-08, 0.00e+00),
    "dcn-dynamic": (0.00e+00, 0.00e+00, 0.00e+00),
    "dcn-fixed_micro2": (1.30e-07, 5.96e-08, 5.96e-08),
    "dcn-lazy_l2": (0.00e+00, 1.79e-07, 0.00e+00),
    "xdeepfm-dynamic": (0.00e+00, 0.00e+00, 0.00e+00),
    "xdeepfm-fixed_micro2": (1.19e-07, 5.96e-08, 1.19e-07),
    "xdeepfm-lazy_l2": (0.00e+00, 1.79e-07, 0.00e+00),
    "deepfm_genres-dynamic": (0.00e+00, 0.00e+00, 0.00e+00),
    "deepfm_genres-fixed_micro2": (1.49e-07, 1.19e-07, 1.19e-07),
    "deepfm_genres-lazy_l2": (0.00e+00, 1.19e-07, 0.00e+00),
    "deepfm-overflow": (0.00e+00, 0.00e+00, 0.00e+00),
    "deepfm_genres-overflow_micro2": (1.49e-08, 0.00e+00, 1.19e-07),
    "xdeepfm_fit_ragged_fixed_micro2": (1.97e-07, 5.96e-08, 1.19e-07),
    "deepfm_genres_fit_dynamic": (1.19e-07, 4.22e-08, 1.19e-07),
    "deepfm_one_rank_overflows": (2.61e-08, 5.96e-08, 5.96e-08),
    "deepfm_genres_one_rank_overflows_micro2": (2.91e-07, 2.98e-08, 1.19e-07),
}


def twin_bounds(name):
    got = VS_TWIN.get(name)
    if got is None:
        return 1e-6, 2e-5, 2e-5
    return tuple(max(4.0 * x, ULP) for x in got)


# ------------------------------------------------------------------------------------------------- running a model
class Spy:
    """Wraps the engine's fwd_bwd and the model's _fit_sharded_batch: per training step its loss, this rank's weight,
    what the step left behind (capacity factor, micro-batches, sticky overflow flag) and its fwd_bwd calls - the
    layout and micro-batch count each ran with and the bucket capacity of its last exchange (0: exact split sizes)."""

    def __init__(self, m):
        self.calls, self.steps = [], []
        e = m._engine
        inner, batch = e.fwd_bwd, m._fit_sharded_batch

        def fwd_bwd(*a, **k):
            rec = dict(factor=e.st.capacity_factor, micro=e.micro_batches)
            self.calls.append(rec)
            out = inner(*a, **k)
            rec["cap"] = int(e.ex.cap)
            return out

        def fit_batch(*a, **k):
            at = len(self.calls)
            loss = batch(*a, **k)
            flag = getattr(e.st.route_fn, "overflow", None)
            self.steps.append(dict(loss=float(loss), weight=m._w, calls=self.calls[at:], factor=e.st.capacity_factor,
                                   micro=e.micro_batches, flag=0 if flag is None else int(flag.item()),
                                   cap_occurrences=getattr(e.st, "cap_occurrences", None)))
            return loss

        e.fwd_bwd, m._fit_sharded_batch = fwd_bwd, fit_batch


def redone(steps):
    return [len(s["calls"]) > 1 for s in steps]


def seed_shard(es, init):
    rows = init["rows"]
    es.st.load_global(rows[:, :D], bias=rows[:, D], lin=rows[:, D + 1])
    names = [k for k in es.params if k != "table_shard"]
    assert sorted(names) == sorted(init["dense"]), (names, sorted(init["dense"]))
    for k in names:
        es.params[k].copy_(init["dense"][k].to(es.params[k].device))


def collect(m, df, steps):
    e = m._engine
    return dict(rows=e.st.shard[:, : D + 2].detach().cpu().double(), steps=steps,
                dense={k: v.detach().cpu().double() for k, v in e.params.items() if k != "table_shard"},
                pred=torch.from_numpy(m.predict(df)).double())


def build_twin(case, fd, spec, l2):
    """The one-GPU twin with the row-wise rule, started at tests/test_shard_fit_host.host_params' seeded values (the
    start TWIN_DRIFT was measured from); returns (model, its initial rows and dense variables as the engine holds
    them, its losses - filled while it trains)."""
    m = make_model(case, fd, L2[l2], dict(table_sharding="none", sparse_optimizer=True))
    e = m._build()
    assert m._shard is None and m._sparse_opt is not None
    e.load_params(host_params(case, spec, m.hparams))
    n = e.spec.rows
    init = dict(rows=e.rows[:n, : D + 2].detach().cpu().clone(),
                dense={k: e.params[k].detach().cpu().clone() for k in sorted(e.grads)})
    losses, inner = [], e.fwd_bwd

    def fwd_bwd(*a, **k):
        out = inner(*a, **k)
        losses.append(float(out))
        return out

    e.fwd_bwd = fwd_bwd
    return m, init, losses


def twin_result(m, df, losses):
    e = m._engine
    n = e.spec.rows
    return dict(rows=e.rows[:n, : D + 2].detach().cpu().double(), losses=list(losses),
                dense={k: e.params[k].detach().cpu().double() for k in sorted(e.grads)},
                pred=torch.from_numpy(m.predict(df)).double())


def f64_result(case, spec, data, hp, init, world=1, batches=None):
    st = R.make_state(oracle_model(case), spec, D, init["rows"], init["dense"])
    if batches is None:
        losses = R.fit(st, data, hp, BATCH, 1, SEED, world)
    else:
        losses = [R.step(st, b, hp, world) for b in batches]
    return dict(rows=st["rows"], dense=st["dense"], losses=losses, pred=R.predict(st, data, hp))


_BASE = {}


def base_run(case, n, l2):
    """(frame pieces, initial values, the twin's result, the float64 result) of one fit() epoch, once per frame."""
    key = (case, n, l2)
    if key not in _BASE:
        df, fd, spec, data = ml_case(case, n)
        twin, init, losses = build_twin(case, fd, spec, l2)
        twin.fit(df, df["label"].values, random_seed_for_mini_batch=False)
        tw = twin_result(twin, df, losses)
        _BASE[key] = ((df, fd, spec, data), init, tw, f64_result(case, spec, data, dict(twin.hparams), init))
    return _BASE[key]


def shard_fit(case, frame, l2, init, extra, before=None):
    """One fit() epoch of the row-sharded model at world size 1, in process; before(model, engine): host checks on
    the built model."""
    df, fd, spec, data = frame
    m = make_model(case, fd, L2[l2], dict(table_sharding="row", **extra))
    es = m._build()
    assert m._shard == (0, 1) and es.st.shard.shape[0] == es.st.R == init["rows"].shape[0]
    seed_shard(es, init)
    if before is not None:
        before(m, es)
    spy = Spy(m)
    m.fit(df, df["label"].values, random_seed_for_mini_batch=False)
    return m, es, collect(m, df, spy.steps)


# ------------------------------------------------------------------------------------------------------ comparing
def rel(got, want):
    return float((got - want.double()).abs().max()) / max(1.0, float(want.abs().max()))


def measure(got, ref, rank=0, world=1, losses=None):
    """(parameters, losses, predictions, where): worst difference of a sharded result to a reference result, and
    the variable that holds the worst parameter (rows: with the global row and the column)."""
    want_rows = ref["rows"][rank::world].double()
    d = (got["rows"] - want_rows).abs()
    at = int(d.argmax())
    p = float(d.max()) / max(1.0, float(want_rows.abs().max()))
    where = f"rows[{(at // d.shape[1]) * world + rank}, {at % d.shape[1]}]"
    for k, v in ref["dense"].items():
        x = rel(got["dense"][k], v)
        if x > p:
            p, where = x, k
    losses = [s["loss"] for s in got["steps"]] if losses is None else losses
    want = [x for x in ref["losses"] if x is not None]
    assert len(losses) == len(want), (len(losses), len(want))
    return (p, max(abs(a - b) for a, b in zip(losses, want)),
            float((got["pred"] - ref["pred"]).abs().max()), where)


def check(name, drift_key, got, tw, f64, rank=0, world=1, losses=None):
    """Prints every figure, then asserts the bounds of the module docstring."""
    vt = measure(got, tw, rank, world, losses)
    vf = measure(got, f64, rank, world, losses)
    bt, drift = twin_bounds(name), TWIN_DRIFT[drift_key]
    print(f"SHARDFIT {name} rank {rank}: vs twin parameters {vt[0]:.2e} losses {vt[1]:.2e} predictions {vt[2]:.2e} "
          f"(bounds {bt[0]:.2e} {bt[1]:.2e} {bt[2]:.2e}); vs float64 parameters {vf[0]:.2e} at {vf[3]} losses "
          f"{vf[1]:.2e} predictions {vf[2]:.2e} (float32 twin {drift[0]:.2e} {drift[1]:.2e})")
    bad = [(q, x, b) for q, x, b in zip(("twin parameters", "twin losses", "twin predictions"), vt, bt) if not x <= b]
    bad += [(q, x, b) for q, x, b in (("float64 parameters at " + vf[3], vf[0], 4 * drift[0]),
                                      ("float64 losses", vf[1], LOSS_F64),
                                      ("float64 predictions", vf[2], 4 * drift[1])) if not x <= b]
    assert not bad, (name, bad)
    return vt, vf


def occurrences(spec, batch):
    return int(R.global_rows(spec, batch).numel())


def micro_parts(spec, batch, M):
    """The (micro-)batches a part runs as: M equal ones when its rows divide, the whole part otherwise."""
    B = batch["idx"].shape[0]
    M = M if B % M == 0 else 1
    return [R.cut(spec, batch, c * (B // M), (c + 1) * (B // M)) for c in range(M)]


def host_overflow_plan(es, spec, data, Fx, M):
    """Per fit() batch at world size 1: does a bucket overflow?  There a bucket overflows exactly when the
    occurrences of a (micro-)batch exceed ShardedTable.capacity of the part (the model sizes every micro-batch's
    buckets for the whole part: cap_occurrences)."""
    _, batches = R.epoch_batches(spec, data, BATCH, SEED)
    plan = []
    for b in batches:
        cap = es.st.capacity(b["idx"].shape[0] * Fx)
        plan.append(any(occurrences(spec, mb) > cap for mb in micro_parts(spec, b, M)))
    return plan


# ------------------------------------------------------------------------------- world size 1, in process: fit()
FIXED = dict(exchange_capacity_factor=2.0, micro_batches=2)
VARIANTS = {"dynamic": ("no_l2", {}), "fixed_micro2": ("no_l2", FIXED), "lazy_l2": ("lazy_l2", {})}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", MODELS)
def test_sharded_fit_at_world_size_one(hip_lib, case, variant):
    """One fit() epoch over 996 rows (ten batches of 96 and one of 36): exact split sizes; fixed-capacity buckets
    with two micro-batches; the reference's default l2 on the table, applied lazily by the owner-side step."""
    l2, extra = VARIANTS[variant]
    frame, init, tw, f64 = base_run(case, 996, l2)
    spec, data = frame[2], frame[3]
    Fx = len(spec.sparse_names) - len(spec.multi_names) + sum(
        int((data["mv"][n][0][1:] - data["mv"][n][0][:-1]).max()) for n in spec.multi_names)

    def before(m, es):
        if extra:
            assert es.st.capacity_factor == 2.0 and es.micro_batches == 2
            assert not any(host_overflow_plan(es, spec, data, Fx, 2))   # no batch overflows: proven on the host
        else:
            assert es.st.capacity_factor is None and es.micro_batches == 1

    m, es, got = shard_fit(case, frame, l2, init, extra, before)
    steps = got["steps"]
    assert len(steps) == 11 and not any(redone(steps)) and all(s["flag"] == 0 for s in steps)
    if extra:
        assert es.exchange_columns() == Fx
        assert all(s["calls"][0]["cap"] > 0 and s["calls"][0]["micro"] == 2 for s in steps)
        assert all(s["factor"] == 2.0 and s["micro"] == 2 and s["cap_occurrences"] is None for s in steps)
    else:
        assert all(s["calls"][0]["cap"] == 0 for s in steps)
    if variant == "lazy_l2":
        assert m._shard_opt.l2_embedding == 1e-5 and m._shard_opt.l2_linear == 1e-5
    check(f"{case}-{variant}", (case, l2), got, tw, f64)


OVERFLOW = {
    # 996 rows, F = 5, factor 0.9: a full batch has 480 occurrences and capacity 448, the last one 180 and 192
    "deepfm-overflow": ("deepfm", 996, dict(exchange_capacity_factor=0.9), ("deepfm", "no_l2")),
    # with `genres` and two micro-batches: every micro-batch's buckets are sized for the whole part (96 rows of
    # 5 + 6 columns at factor 0.2: 256 slots) and a micro-batch of 48 rows brings 240 occurrences and its tags; the
    # last batch of 964 rows has 4 rows: 64 slots for micro-batches of some 14 occurrences
    "deepfm_genres-overflow_micro2": ("deepfm_genres", 964, dict(exchange_capacity_factor=0.2, micro_batches=2),
                                      ("deepfm_genres", "964")),
}


@pytest.mark.parametrize("name", list(OVERFLOW))
def test_sharded_fit_redoes_the_batches_that_overflow(hip_lib, name):
    """The overflow redo of _fit_sharded_batch through fit(): the ten full batches overflow their fixed-capacity
    buckets and are redone with exact split sizes, the last batch fits.  The trajectory is the dynamic layout's, the
    twin's and float64's; the layout is restored after every redo.  With a multi-valued feature the redo has to run
    without the micro-batch pipeline (exact split sizes have none for expanded tag lists): this raised ValueError
    ("micro-batching with multi-valued / value features needs their mv= entries") before the redo set
    micro_batches = 1 for engines with scratch-row features."""
    case, n, extra, drift_key = OVERFLOW[name]
    factor, M = extra["exchange_capacity_factor"], extra.get("micro_batches", 1)
    frame, init, tw, f64 = base_run(case, n, "no_l2")
    spec, data = frame[2], frame[3]
    Fx = 5 + (int((data["mv"]["genres"][0][1:] - data["mv"]["genres"][0][:-1]).max()) if data["mv"] else 0)
    want = [True] * 10 + [False]

    def before(m, es):
        assert es.st.capacity_factor == factor and es.micro_batches == M
        if case == "deepfm":   # the arithmetic of the worked example, from capacity() itself
            assert (es.st.capacity(480), es.st.capacity(180)) == (448, 192)
        assert host_overflow_plan(es, spec, data, Fx, M) == want

    m, es, got = shard_fit(case, frame, "no_l2", init, extra, before)
    steps = got["steps"]
    assert redone(steps) == want and sum(len(s["calls"]) for s in steps) == 21
    for s, over in zip(steps, want):
        first = s["calls"][0]
        assert first["factor"] == factor and first["cap"] > 0 and first["micro"] == M   # ran fixed-capacity first
        if over:
            again = s["calls"][1]
            assert again["factor"] is None and again["cap"] == 0
            assert again["micro"] == (1 if case.endswith("genres") else M)
        # the layout is back, and no sticky flag is left for the next batch
        assert s["factor"] == factor and s["micro"] == M and s["flag"] == 0 and s["cap_occurrences"] is None
    assert es.st.capacity_factor == factor and es.micro_batches == M and es.exchange_columns() == Fx
    # (so the batch after an overflowed one ran fixed-capacity, from its own exchange: calls[0]["cap"] is e.ex.cap)
    check(name, drift_key, got, tw, f64)
    # ... and the dynamic layout's trajectory
    _, _, dyn = shard_fit(case, frame, "no_l2", init, {})
    assert not any(redone(dyn["steps"]))
    vd = measure(got, dict(dyn, losses=[s["loss"] for s in dyn["steps"]]))
    bt = twin_bounds(name)
    print(f"SHARDFIT {name}: vs the dynamic layout parameters {vd[0]:.2e} losses {vd[1]:.2e} predictions {vd[2]:.2e}")
    assert vd[0] <= bt[0] and vd[1] <= bt[1] and vd[2] <= bt[2], vd


# ------------------------------------------------------------------------------------------------------ two ranks
TWO_RANK_EXTRA = {
    "xdeepfm_fit_ragged_fixed_micro2": dict(exchange_capacity_factor=1.5, micro_batches=2),
    "deepfm_genres_fit_dynamic": {},
    # factor 1.0: 48 rows of 5 columns over two owners -> 192 slots a bucket; rank 1 sends 240 occurrences to owner 0
    "deepfm_one_rank_overflows": dict(exchange_capacity_factor=1.0),
    # 48 rows of 5 + 6 columns at factor 0.3 -> 192 slots for every micro-batch of 24 rows; rank 1's bring
    # 24 x (5 + 4 tags) = 216 occurrences for owner 0 (at factor 1.0 there would be 384 slots: no overflow)
    "deepfm_genres_one_rank_overflows_micro2": dict(exchange_capacity_factor=0.3, micro_batches=2),
}


def _worker(rank, world, port, name, init, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.pop("RECMAN_FORCE_COLLECTIVES", None)
    # (a finite timeout: ranks that disagree on a collective fail instead of waiting)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        import sys

        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        case, n, what = TWO_RANK[name]
        df, fd, spec, data = ml_case(case, n)
        m = make_model(case, fd, NO_L2, TWO_RANK_EXTRA[name])
        es = m._build()
        assert m._shard == (rank, world) and es.st.shard.shape[0] < es.st.R
        seed_shard(es, init)
        spy = Spy(m)
        if what == "fit":
            m.fit(df, df["label"].values, random_seed_for_mini_batch=False)
        else:
            for parts in skew_steps(case, df, fd, spec, data):
                m.fit_on_batch(parts[rank], parts[rank]["label"].values)
        out = collect(m, df, spy.steps)
        out["exchange_columns"] = es.exchange_columns()
        torch.save(out, f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


def wide_matrix(spec, batch, T):
    """The occurrence matrix the fixed-capacity exchange carries: the plain columns, then T padded tag columns."""
    idx = batch["idx"][:, :5]
    if not T:
        return idx
    o, ids = batch["mv"]["genres"]
    n = o[1:] - o[:-1]
    w = torch.full((idx.shape[0], T), -1, dtype=torch.int64)
    seg = torch.repeat_interleave(torch.arange(idx.shape[0]), n)
    w[seg, torch.arange(ids.numel()) - o[seg]] = ids
    return torch.cat([idx, w], 1)


def host_route_plan(spec, parts_of_steps, factor, M, genres, world=2):
    """Per step and rank: does a bucket of that rank's part overflow?  recman_amd.dist.route_torch at the capacity
    ShardedTable.capacity gives the largest part (the formula is restated here: there is no table on the host); the
    tag columns are as wide as the widest list seen so far on any rank, as fit_on_batch agrees on them."""
    from recman_amd.dist import ShardedTable, route_torch

    offs = torch.tensor(np.concatenate([[0], np.cumsum(spec.feat_sizes)[:-1]]))
    st = SimpleNamespace(capacity_factor=factor, world=world, cap_occurrences=None)   # what capacity() reads
    T, plan, caps = 0, [], []
    for parts in parts_of_steps:
        if genres:
            T = max([T] + [int((p["mv"]["genres"][0][1:] - p["mv"]["genres"][0][:-1]).max()) for p in parts])
        foff = torch.cat([offs[:5], offs[5:6].repeat(T)]) if genres else offs[:5]
        hi = max(p["idx"].shape[0] for p in parts)
        lo = min(p["idx"].shape[0] for p in parts)
        cap = ShardedTable.capacity(st, hi * (5 + T))
        m = M if (lo == hi and lo % M == 0) else 1
        plan.append([any(int(route_torch(wide_matrix(spec, mb, T), foff, world, cap)[3]) for mb in micro_parts(spec, p, m))
                     for p in parts])
        caps.append(cap)
    return plan, caps


def run_two_ranks(tmp_path, name, want_plan=None, want_caps=None):
    case, n, what = TWO_RANK[name]
    df, fd, spec, data = ml_case(case, n)
    twin, init, losses = build_twin(case, fd, spec, "no_l2")
    extra = TWO_RANK_EXTRA[name]
    factor, M = extra.get("exchange_capacity_factor"), extra.get("micro_batches", 1)
    genres = case.endswith("genres")
    # host: which rank's part overflows at which step
    if what == "fit":
        _, batches = R.epoch_batches(spec, data, BATCH, SEED)
        parts_of_steps = [[R.cut(spec, b, a, z) for a, z, _ in R.split(b["idx"].shape[0], 2)] for b in batches]
        frames = None
    else:
        frames = skew_steps(case, df, fd, spec, data)
        parts_of_steps = [[encode(fd, p)[1] for p in parts] for parts in frames]
        batches = skew_batches(fd, spec, frames)
    plan, caps = host_route_plan(spec, parts_of_steps, factor, M, genres) if factor else (None, None)
    if want_plan is not None:    # before anything is spawned: the overflow the case is about happens, and only it
        assert plan == want_plan and (want_caps is None or caps == want_caps), (plan, caps)
    if what == "steps":
        rows = R.global_rows(spec, parts_of_steps[1][1])
        assert bool((rows % 2 == 0).all()) and parts_of_steps[1][1]["idx"].shape[0] == SKEW_PART
    out = str(tmp_path / "r")
    port = 29200 + list(TWO_RANK).index(name)
    mp.spawn(_worker, args=(2, port, name, init, out), nprocs=2, join=True)
    res = [torch.load(f"{out}.{r}", weights_only=True) for r in range(2)]
    # the twin and the float64 loop on the global batches
    if what == "fit":
        twin.fit(df, df["label"].values, random_seed_for_mini_batch=False)
        f64 = f64_result(case, spec, data, dict(twin.hparams), init, world=2)
    else:
        for parts in frames:
            both = pd.concat(list(parts), ignore_index=True)
            twin.fit_on_batch(both, both["label"].values)
        f64 = f64_result(case, spec, data, dict(twin.hparams), init, world=2, batches=batches)
    tw = twin_result(twin, df, losses)
    # the global loss of a step: the parts' losses by their weights (None: 1 / world, fit_on_batch)
    steps = [res[r]["steps"] for r in range(2)]
    assert len(steps[0]) == len(steps[1]) == len(batches)
    glob = [sum((0.5 if s[t]["weight"] is None else s[t]["weight"]) * s[t]["loss"] for s in steps)
            for t in range(len(batches))]
    for r in range(2):
        check(name, name, res[r], tw, f64, rank=r, world=2, losses=glob)
    assert torch.equal(res[0]["pred"], res[1]["pred"])
    return res, steps, plan, parts_of_steps


@pytest.mark.parametrize("name", ["xdeepfm_fit_ragged_fixed_micro2", "deepfm_genres_fit_dynamic"])
def test_two_rank_fit_follows_the_twin_and_float64(hip_lib, tmp_path, name):
    """fit() on two ranks over 1001 rows - ten batches of 48 + 48 and one of 41 rows split 21 + 20: each rank's rows
    rank::2 and every dense variable against the twin and float64.  xDeepFM: fixed capacity 1.5 with two
    micro-batches (the ragged batch runs without the pipeline, both ranks with the buckets of the larger part);
    DeepFM with `genres`: exact split sizes."""
    res, steps, plan, parts = run_two_ranks(tmp_path, name)
    assert [p[0]["idx"].shape[0] for p in parts][-1] == 21 and [p[1]["idx"].shape[0] for p in parts][-1] == 20
    for r in range(2):
        assert not any(redone(steps[r])) and all(s["flag"] == 0 for s in steps[r])
        assert [s["weight"] for s in steps[r]] == [0.5] * 10 + [(21 - r) / 41]
    if plan is not None:
        assert not any(any(p) for p in plan)                 # no part overflows: proven on the host
        for r in range(2):
            assert [s["calls"][0]["micro"] for s in steps[r]] == [2] * 10 + [1]
            assert all(s["calls"][0]["cap"] > 0 and s["factor"] == 1.5 and s["micro"] == 2 for s in steps[r])
    else:
        assert all(s["calls"][0]["cap"] == 0 for r in range(2) for s in steps[r])


@pytest.mark.parametrize("name", ["deepfm_one_rank_overflows", "deepfm_genres_one_rank_overflows_micro2"])
def test_two_rank_step_is_redone_on_both_ranks_when_one_overflows(hip_lib, tmp_path, name):
    """Three fit_on_batch steps on two ranks; in the second, rank 1's part is 48 copies of one example whose global
    rows are all even: every occurrence goes to owner 0 and overflows rank 1's bucket, rank 0's part fits.  BOTH
    ranks redo the step (_any_rank: otherwise their collectives would mismatch and the job would time out); the
    result is the twin's and float64's on the concatenated 96-row batches; the third step runs fixed-capacity again
    without overflow."""
    extra = TWO_RANK_EXTRA[name]
    factor, M = extra["exchange_capacity_factor"], extra.get("micro_batches", 1)
    # on the host: rank 1 alone overflows, in step 2 alone, at 192 slots a bucket
    res, steps, plan, parts = run_two_ranks(tmp_path, name, [[False, False], [False, True], [False, False]], [192] * 3)
    for r in range(2):
        assert redone(steps[r]) == [False, True, False]
        again = steps[r][1]["calls"][1]
        assert again["factor"] is None and again["cap"] == 0
        assert again["micro"] == (1 if name.startswith("deepfm_genres") else M)
        for s in steps[r]:
            assert s["calls"][0]["factor"] == factor and s["calls"][0]["cap"] > 0 and s["calls"][0]["micro"] == M
            assert s["factor"] == factor and s["micro"] == M and s["flag"] == 0 and s["cap_occurrences"] is None
    if name.startswith("deepfm_genres"):
        assert res[0]["exchange_columns"] == res[1]["exchange_columns"] == 11

