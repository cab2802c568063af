"""CPU (no GPU): tests/shard_fit_ref.py, the float64 restatement of a row-sharded training loop, pinned itself -
against the oracle's own gradients at world size 1, against itself across world sizes, and against two deliberately
wrong variants; and the float32 twin's drift from float64, the yardstick of tests/test_gpu_shard_fit.py's bounds.
The cases and the frame builders below are shared with that file."""
import numpy as np
import pytest
import torch

from oracle import th_layers as T
from tests import shard_fit_ref as R

D, BATCH, LR, SEED = 16, 96, 0.01, 2019
NO_L2 = dict(embedding_l2_reg=0.0, linear_l2_reg=0.0, deep_l2_reg=1e-4)
# the reference's default coefficients on the table (hparams/xDeepFM.py:22-23): the lazy path
LAZY_L2 = dict(embedding_l2_reg=1e-5, linear_l2_reg=1e-5, deep_l2_reg=1e-4)
MODELS = ("deepfm", "dcn", "xdeepfm", "deepfm_genres")


def make_model(case, fd, l2=NO_L2, extra=None, epoch=1):
    """The model class of `case` on the feature dictionary fd: D = 16, batch 96, dropout off, Adam at 0.01.  extra:
    more hyper-parameters (table_sharding, exchange_capacity_factor, micro_batches, sparse_optimizer)."""
    import recman_amd.th as th

    common = dict(epoch=epoch, batch_size=BATCH, random_seed=SEED)
    if case in ("deepfm", "deepfm_genres"):
        m = th.DeepFM(fd, embedding_size=D, deep_dropout=(1, 1, 1), learning_rate=LR, **l2, **common)
    elif case == "dcn":
        m = th.DCN(fd, embedding_size=D, deep_dropout=(1, 1, 1), learning_rate=LR, cross_layer_num=2, **l2, **common)
    else:
        hp = dict(embedding_size=D, deep_dropout=(1, 1, 1), cin_cross_layer_units=[16, 16], cin_dropout=[1, 1, 1],
                  learning_rate=LR, cin_l2_reg=0.0, **l2)
        m = th.xDeepFM(fd, hp, **common)
    m.hparams.update(extra or {})  # (the gen-1 signatures are the reference's: the exchange knobs are hparams)
    return m


def oracle_model(case):
    return "deepfm" if case.startswith("deepfm") else case


def ml_case(case, n):
    """The first n rows of the ml-100k golden slice for `case`: (frame, feature dictionary, oracle Spec, the encoded
    frame as shard_fit_ref's data dict)."""
    import recman_amd.th as th
    from tests.test_gpu_models import GOLD, ml_features, ml_frame

    df = ml_frame().iloc[:n].copy()
    genres = case.endswith("genres")
    if genres:
        df["genres"] = GOLD["raw_genres"][:n].astype(object)
    fd = ml_features(df)
    if genres:
        fd["genres"] = th.MultiValCsvFeat(name="genres", tags=tuple(GOLD["genre_tags"].tolist()))
    return (df, fd) + encode(fd, df)


def encode(fd, df):
    """(oracle Spec, data dict) of a frame under an initialised feature dictionary."""
    import recman_amd.th as th

    inp = th.DataInputs().load(fd, df, df["label"].values)
    multi = [f.name for f in fd.multi_val_csv_feats]
    spec = T.Spec([f.name for f in fd.embedding_feats], [f.feat_size for f in fd.embedding_feats],
                  [f.name for f in fd.dense_feats], multi)
    mv = {k: (torch.from_numpy(c.offsets), torch.from_numpy(c.ids)) for k, c in inp.mv.items()}
    data = dict(idx=torch.from_numpy(np.ascontiguousarray(inp.idx)), dense=torch.from_numpy(np.ascontiguousarray(inp.dense)),
                y=torch.from_numpy(np.asarray(inp.y).astype(np.int64)), mv=mv or None)
    return spec, data


def host_params(case, spec, hp, seed=0):
    """A seeded start under the reference's variable names (float32 values): uniform on +-0.1 sqrt(3), that is std
    0.1, about the reference initialiser's scale at these shapes (glorot: 0.06 .. 0.29); the variables the reference
    starts at zero - bias tables, linear weights, biases - are non-zero too, so every term of the step is exercised.
    Uniform because it is the same on every machine, bit for bit (24 random bits scaled; a truncated normal goes
    through erfinv, whose last bit differs between CPUs - and Adam's first steps amplify that, see
    profiles/shard_fit.md).  The GPU file loads the same values into its models: the float32 twin's drift measured
    here is the drift of ITS cases."""
    model = oracle_model(case)
    p = T.make_params(spec, model, D, hidden=tuple(hp["deep_hidden_units"]),
                      cin_units=tuple(hp.get("cin_cross_layer_units", ())) if model == "xdeepfm" else (),
                      cross_layers=hp.get("cross_layer_num", 0) if model == "dcn" else 0,
                      use_bias=(model == "deepfm"), seed=SEED, dtype=torch.float32, scale=0.1)   # names and shapes
    g = torch.Generator().manual_seed(SEED + seed)
    a = float(np.float32(0.1 * 3 ** 0.5))
    return {k: (torch.rand(v.shape, generator=g, dtype=torch.float32) * 2 - 1) * a for k, v in p.items()}


def host_state(case, spec, hp, dtype=torch.float64, seed=0):
    """shard_fit_ref's state at host_params' values."""
    model = oracle_model(case)
    p = host_params(case, spec, hp, seed)
    offs, dense_offs, _ = spec.lin_layout
    blocks = []
    for f, (name, V) in enumerate(zip(spec.sparse_names, spec.feat_sizes)):
        bias = p[f"{name}_feat_bias"] if model == "deepfm" else torch.zeros(V, 1)
        blocks.append(torch.cat([p[f"{name}_feat_embed"], bias, p["linear_w"][offs[f]: offs[f] + V]], dim=1))
    dense = {k: v for k, v in p.items() if "_feat_" not in k and k != "linear_w"}
    dense["linear_w_dense"] = torch.stack([p["linear_w"][o, 0] for o in dense_offs])
    return R.make_state(model, spec, D, torch.cat(blocks), dense, dtype=dtype)


def state_error(a, b, keys=("rows", "m_rows", "v_rows")):
    """Worst |a - b| / max(1, max|b|) over the rows, their moments and every dense variable with its moments."""
    worst = 0.0
    for k in keys:
        worst = max(worst, float((a[k].double() - b[k].double()).abs().max()) / max(1.0, float(b[k].abs().max())))
    for grp in ("dense", "m_dense", "v_dense"):
        for k, v in b[grp].items():
            worst = max(worst, float((a[grp][k].double() - v.double()).abs().max()) / max(1.0, float(v.abs().max())))
    return worst


def hand_batches(spec, data):
    """Global batches of 96, 96, 41 (21 + 20 on two ranks), 1 (skipped by more than one rank), 96 and 7 rows."""
    out, at = [], 0
    for n in (96, 96, 41, 1, 96, 7):
        out.append(R.cut(spec, data, at, at + n))
        at += n
    return out


def run_batches(case, spec, data, hp, world, mutate=None, dtype=torch.float64):
    st = host_state(case, spec, hp, dtype)
    losses = [R.step(st, b, hp, world, mutate) for b in hand_batches(spec, data)
              if not (world == 1 and b["idx"].shape[0] == 1)]  # (one rank would train on the batch the others skip)
    return st, losses


@pytest.fixture(scope="module")
def frames():
    out = {}
    for case in MODELS:
        df, fd, spec, data = ml_case(case, 1001)
        out[case] = (spec, data, dict(make_model(case, fd, LAZY_L2).hparams))
    return out


@pytest.fixture(scope="module")
def world1(frames):
    """The float64 trajectory at world size 1 over hand_batches, computed once per case."""
    return {case: run_batches(case, *frames[case], 1) for case in MODELS}


def test_the_split_rule():
    assert R.split(41, 2) == [(0, 21, 21 / 41), (21, 41, 20 / 41)]
    assert R.split(7, 3) == [(0, 3, 3 / 7), (3, 5, 2 / 7), (5, 7, 2 / 7)]
    assert R.split(1, 2) is None and R.split(2, 3) is None and R.split(1, 1) == [(0, 1, 1.0)]
    for n in range(1, 60):
        for w in (1, 2, 3, 4):
            p = R.split(n, w)
            if p is None:
                assert n < w
                continue
            assert p[0][0] == 0 and p[-1][1] == n and all(a[1] == b[0] for a, b in zip(p, p[1:]))
            assert abs(sum(x[2] for x in p) - 1.0) < 1e-15 and max(b - a for a, b, _ in p) - min(b - a for a, b, _ in p) <= 1


def test_take_cut_and_concat_keep_every_example(frames):
    spec, data, _ = frames["deepfm_genres"]
    perm = np.random.RandomState(3).permutation(data["idx"].shape[0])
    sh = R.take(spec, data, perm)
    offsets, ids = data["mv"]["genres"]
    for j in (0, 17, 1000):
        b = R.cut(spec, sh, j, j + 1)
        src = int(perm[j])
        assert torch.equal(b["idx"][0], data["idx"][src]) and int(b["y"][0]) == int(data["y"][src])
        assert torch.equal(b["mv"]["genres"][1], ids[int(offsets[src]): int(offsets[src + 1])])
    whole = R.concat(spec, [R.cut(spec, sh, 0, 40), R.cut(spec, sh, 40, 41), R.cut(spec, sh, 41, 1001)])
    assert torch.equal(whole["idx"], sh["idx"]) and torch.equal(whole["mv"]["genres"][0], sh["mv"]["genres"][0])
    assert torch.equal(whole["mv"]["genres"][1], sh["mv"]["genres"][1])
    _, batches = R.epoch_batches(spec, data, BATCH, SEED)
    assert [b["idx"].shape[0] for b in batches] == [96] * 10 + [41]
    _, batches = R.epoch_batches(spec, R.cut(spec, data, 0, 960), BATCH, SEED)
    assert [b["idx"].shape[0] for b in batches] == [96] * 10  # the empty trailing batch is skipped


@pytest.mark.parametrize("case", MODELS)
def test_world_one_gradients_equal_the_oracle_step_by_step(frames, case):
    """Along the world-1 trajectory, every step's gradients on identical parameters equal oracle.th_layers.fwd_bwd's,
    called as tests/test_gpu_models.oracle_fit calls it (one batch, the full hyper-parameters): on the rows the batch
    touches with the l2 term in, the dense variables everywhere; on every other row the oracle has the dense l2 term
    reg * row alone, which the lazy rule leaves out."""
    spec, data, hp = frames[case]
    st = host_state(case, spec, hp)
    model = st["model"]
    worst = [0.0]

    def check(st, batch):
        gr = R.gradients(st, batch, hp, 1)
        p = R.reference_params(st)
        idx, dense, y, mv = R._to(batch, torch.float64)
        _, _, _, g = T.fwd_bwd(model, p, spec, idx, dense, y, hp, mv=mv)
        G, gd = R._split_grads(st, g)
        t = gr["touched"]
        assert 0 < int(t.sum()) < t.numel()
        for name, got, want in [("rows", gr["G"][t], G[t])] + [(k, gr["dense"][k], gd[k]) for k in gd]:
            err = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
            worst[0] = max(worst[0], err)
            assert err <= 1e-12, (name, err)
        assert float(gr["G"][~t].abs().max()) == 0.0
        lazy_out = G[~t].clone()
        lazy_out[:, :D] -= hp["embedding_l2_reg"] * st["rows"][~t][:, :D]
        lazy_out[:, D + 1] -= hp["linear_l2_reg"] * st["rows"][~t][:, D + 1]
        assert float(lazy_out.abs().max()) <= 1e-15

    losses = R.fit(st, data, hp, BATCH, seed=SEED, on_step=check)
    assert len(losses) == 11 and st["t"] == 11 and losses[-1] < losses[0]
    print(f"{case}: worst gradient difference to the oracle {worst[0]:.2e}")


def test_world_one_first_step_equals_oracle_fit(frames):
    """oracle_fit itself (float32 data, Keras Adam over whole variables, the literal hyper-parameters) for one step
    over one batch: from zero moments, Adam leaves a row with a zero gradient where it is, so with no l2 on the table
    the dense rule and the row-wise rule coincide at the first step.  The bound is not float64's rounding but the
    hyper-parameters' float32 rounding, which the restatement has and oracle_fit has not: 1 - beta2 is off by 1.3e-5
    relative, sqrt(v) by half of that, and where |g| is of eps' order this no longer cancels against lr_t - at most
    6.5e-6 of a step of lr = 0.01, 6.5e-8."""
    from tests.test_gpu_models import oracle_fit

    spec, data, hp = frames["deepfm"]
    hp = dict(hp, embedding_l2_reg=0.0, linear_l2_reg=0.0)
    part = R.cut(spec, data, 0, 96)
    st = host_state("deepfm", spec, hp)
    p0 = {k: v.clone() for k, v in R.reference_params(st).items()}
    p1 = oracle_fit("deepfm", p0, spec, part["idx"].numpy(), part["dense"].double().numpy(), part["y"].numpy(), hp, 96,
                    1, SEED, LR)
    sh, _ = R.epoch_batches(spec, part, 96, SEED)   # (oracle_fit shuffles inside the batch: the same examples)
    R.step(st, sh, hp, 1)
    got = R.reference_params(st)
    for k, v in p1.items():
        assert float((got[k] - v).abs().max()) <= 1e-7, k
    assert float((got["linear_w"] - p0["linear_w"]).abs().max()) > 1e-3   # it stepped


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", MODELS)
def test_every_world_size_gives_the_world_one_trajectory(frames, world1, case, world):
    """The weighted parts add up to the global mean: 41 rows as 21 + 20, 7 rows as 3 + 2 + 2; the 1-row batch is
    skipped without advancing t."""
    spec, data, hp = frames[case]
    st1, losses1 = world1[case]
    st, losses = run_batches(case, spec, data, hp, world)
    assert losses[3] is None and st["t"] == st1["t"] == 5
    got = [x for x in losses if x is not None]
    assert max(abs(a - b) for a, b in zip(got, losses1)) <= 1e-12
    err = state_error(st, st1)
    print(f"{case} world {world}: {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("mutate", R.MUTATIONS)
@pytest.mark.parametrize("case", MODELS)
def test_a_wrong_restatement_is_caught(frames, world1, case, mutate):
    """Equal weights 1 / world on the ragged 21 + 20 split, and the dense l2 term once per rank: both leave the
    world-1 trajectory by far more than float64 rounding - and by more than the 1e-6 the GPU file allows the product
    against its one-GPU twin."""
    spec, data, hp = frames[case]
    st1, _ = world1[case]
    st, _ = run_batches(case, spec, data, hp, 2, mutate)
    err = state_error(st, st1, keys=("rows",))
    print(f"{case} {mutate}: {err:.2e}")
    assert err > 1e-6
    assert err > 1e6 * 1e-12   # the bound of test_every_world_size_gives_the_world_one_trajectory, a million times


# ------------------------------------------------------------------------------------------- the float32 twin's drift
def twin_drift(case, spec, data, hp, world=1, epochs=1, batches=None):
    """(parameters, predictions): the float32 restatement's worst deviation from the float64 one after the run - on
    rows and dense variables as |d| / max(1, max|w|), on predict() over the frame as |d|."""
    out = {}
    for dtype in (torch.float64, torch.float32):
        st = host_state(case, spec, hp, dtype)
        if batches is None:
            R.fit(st, data, hp, BATCH, epochs, SEED, world)
        else:
            for b in batches:
                R.step(st, b, hp, world)
        out[dtype] = (st, R.predict(st, data, hp))
    (s64, p64), (s32, p32) = out[torch.float64], out[torch.float32]
    return state_error(s32, s64, keys=("rows",)), float((p32 - p64).abs().max())


@pytest.mark.parametrize("l2", ["no_l2", "lazy_l2"])
@pytest.mark.parametrize("case", MODELS)
def test_float32_twin_drift_over_one_epoch(case, l2):
    """One fit() epoch (11 steps) of every in-process case of tests/test_gpu_shard_fit.py: the float32 twin stays
    within 2e-4 of float64 on predictions (the bound test_fit_predict_matches_oracle_training_loop uses), so no case
    needs a shorter run.  The printed numbers are that file's TWIN_DRIFT constants."""
    df, fd, spec, data = ml_case(case, 996)
    hp = dict(make_model(case, fd, NO_L2 if l2 == "no_l2" else LAZY_L2).hparams)
    dp, dy = twin_drift(case, spec, data, hp)
    print(f"TWIN_DRIFT {case} {l2}: parameters {dp:.2e}, predictions {dy:.2e}")
    assert 0 < dy < 2e-4 and 0 < dp < 2e-4


# ------------------------------------------------------------------------- the two-rank cases of the GPU file
COLS = ("user_id", "item_id", "gender", "occupation", "zip")
SKEW_ROWS, SKEW_PART = 1000, 48


def skew_steps(case, df, fd, spec, data):
    """Three global batches of 48 + 48 rows for fit_on_batch on two ranks, as [(rank 0's frame, rank 1's frame)]: the
    second batch gives rank 1 48 copies of ONE example put together from column values of the frame so that its five
    global rows (field offset + encoded id) are all even - every occurrence goes to owner 0; with `genres`, the
    longest genre list of the frame whose tag rows are all even as well.  Every other part is ordinary rows."""
    import pandas as pd

    offs = np.concatenate([[0], np.cumsum(spec.feat_sizes)[:-1]])
    g = (data["idx"][:, :5] + torch.tensor(offs[:5])).numpy()
    one = df.iloc[[0]].copy()
    for f, c in enumerate(COLS):
        one[c] = [df[c].values[int(np.nonzero(g[:, f] % 2 == 0)[0][0])]]
    if case.endswith("genres"):
        o, ids = data["mv"]["genres"]
        best = None
        for j in range(len(df)):
            t = ids[int(o[j]): int(o[j + 1])] + int(offs[5])
            if bool((t % 2 == 0).all()) and (best is None or len(t) > best[1]):
                best = (j, len(t))
        one["genres"] = [df["genres"].values[best[0]]]
    skew = pd.concat([one] * SKEW_PART, ignore_index=True)
    order = np.random.RandomState(7).permutation(len(df))
    cut = lambda k: df.iloc[order[k * SKEW_PART: (k + 1) * SKEW_PART]]  # noqa: E731
    return [(cut(0), cut(1)), (cut(2), skew), (cut(3), cut(4))]


def skew_batches(fd, spec, steps):
    """The global 96-row batches of skew_steps, encoded (rank 0's rows first: the split rule gives them back)."""
    return [R.concat(spec, [encode(fd, part)[1] for part in parts]) for parts in steps]


TWO_RANK = {  # name -> (case, rows of the frame, what runs)
    "xdeepfm_fit_ragged_fixed_micro2": ("xdeepfm", 1001, "fit"),
    "deepfm_genres_fit_dynamic": ("deepfm_genres", 1001, "fit"),
    "deepfm_one_rank_overflows": ("deepfm", SKEW_ROWS, "steps"),
    "deepfm_genres_one_rank_overflows_micro2": ("deepfm_genres", SKEW_ROWS, "steps"),
}


@pytest.mark.parametrize("name", list(TWO_RANK))
def test_float32_twin_drift_of_the_two_rank_cases(name):
    case, n, what = TWO_RANK[name]
    df, fd, spec, data = ml_case(case, n)
    hp = dict(make_model(case, fd, NO_L2).hparams)
    batches = skew_batches(fd, spec, skew_steps(case, df, fd, spec, data)) if what == "steps" else None
    if batches is not None:
        assert [b["idx"].shape[0] for b in batches] == [96, 96, 96]
        rows = R.global_rows(spec, R.cut(spec, batches[1], 48, 96))
        assert bool((rows % 2 == 0).all()) and rows.numel() >= 240
    dp, dy = twin_drift(case, spec, data, hp, world=2, batches=batches)
    print(f"TWIN_DRIFT {name}: parameters {dp:.2e}, predictions {dy:.2e}")
    assert 0 < dy < 2e-4 and 0 < dp < 2e-4


def test_float32_twin_drift_of_the_overflow_frame_with_genres():
    """964 rows: ten full batches and one of 4 rows (tests/test_gpu_shard_fit.py says why)."""
    df, fd, spec, data = ml_case("deepfm_genres", 964)
    dp, dy = twin_drift("deepfm_genres", spec, data, dict(make_model("deepfm_genres", fd, NO_L2).hparams))
    print(f"TWIN_DRIFT deepfm_genres 964 rows: parameters {dp:.2e}, predictions {dy:.2e}")
    assert 0 < dy < 2e-4 and 0 < dp < 2e-4
