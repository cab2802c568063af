"""CPU: the top-k twin (tests/topk_ref.py), its cases, the C ABI and ledger of include/recman_hip_topk.h, the limits of
rm_topk_ip and the retrieval errors of th.TwoTower - all without a GPU."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from tests import topk_ref as R
from tests import twotower_ref as TT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recman_hip_topk.h")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(rm_[a-z0-9_]+)\s*\(", _header_text())))


def _stream_entry_points():
    return {m.group(1) for m in re.finditer(r"\b(rm_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", _header_text(), flags=re.S)
            if re.search(r"\brm_stream_t\s+stream\b", m.group(2))}


# ------------------------------------------------------------------------------------------------------ the twin
def _tricky_scores():
    """Ties, -0.0 against +0.0, NaN (two of them), -inf, a row that appears in no top."""
    S = torch.tensor([[1.0, 2.0, 2.0, -0.0, 0.0, float("nan"), -1.0, float("nan"), 2.0, -math.inf],
                      [0.5, 0.5, 0.5, 0.5, float("nan"), 0.5, -0.0, 3.0, -2.0, 0.0]], dtype=torch.float64)
    return torch.cat([S, torch.randint(-3, 4, (5, 10), generator=torch.Generator().manual_seed(1)).double() / 2])


@pytest.mark.parametrize("k", [1, 3, 8, 10, 13])
def test_twin_agrees_with_python_loops(k):
    S = _tricky_scores()
    ex = [[2, 2, -1, 99], [], [0, 1, 2, 3, 4, 5, 6, 7], [9], [], [3, 3], [1, 8, 0]]
    for exclude in (None, ex):
        rows, sc = R.topk(S, k, exclude)
        lr, ls = R.loops(S, k, exclude)
        assert rows.tolist() == lr
        got, want = sc.tolist(), ls
        for a, b in zip(got, want):
            for x, y in zip(a, b):
                assert (math.isnan(x) and math.isnan(y)) or (x == y and math.copysign(1, x) == math.copysign(1, y))
    rows, sc = R.topk(S, 10)
    assert rows[0].tolist() == [1, 2, 8, 0, 3, 4, 6, 9, 5, 7]  # ties by row, -0.0 == +0.0, -inf, then NaN by row
    assert math.copysign(1.0, float(sc[0, 4])) == 1.0  # -0.0 comes back as +0.0
    rows, sc = R.topk(S, 13, ex)
    assert sorted(rows[2].tolist()[:2]) == [8, 9] and rows[2, 2:].eq(-1).all() and sc[2, 2:].eq(-math.inf).all()


def test_exact_cases_meet_the_exact_arithmetic_precondition():
    for Nq, N, H, k, _ in R.EXACT_CASES:
        case = R.exact_case(Nq, N, H, k)
        for t in (case["Q"], case["C"]):
            assert bool((t * 8 == (t * 8).round()).all()) and float(t.abs().max()) <= 1.0
        m = R.exact_precondition(case)
        print(f"exact {Nq}x{N} H={H}: largest |partial sum| x 64 = {m:.0f}")
        assert m < 2 ** 24
        assert torch.equal(case["S"].float().double(), case["S"])  # every score is an fp32 number
        if N > 7:
            assert int((case["C"][1:] == case["C"][:-1]).all(1).sum()) > 0  # repeated rows: ties
    for Nq, N, H, k, _ in R.RISING_CASES:
        case = R.rising_case(Nq, N, H, k)
        assert R.exact_precondition(case, R.RISING_QUANTUM) < 2 ** 24
        assert bool((case["Q"] / R.RISING_QUANTUM * 8192 / 8).frac().eq(0).all())
        assert bool((case["S"][:, 1:] > case["S"][:, :-1]).all())  # strictly rising: every row beats the threshold
        assert torch.equal(case["S"].float().double(), case["S"])


def test_near_tie_cap_holds_on_every_random_case():
    for Nq, N, H, k in R.RANDOM_CASES:
        share = R.tie_share(R.random_case(Nq, N, H, k))
        print(f"random {Nq}x{N} H={H} k={k}: boundary near-tie share {share:.3f}")
        assert share <= TT.TIE_SHARE


# ------------------------------------------------------------------------------------------- the ABI and the ledger
def test_the_header_is_bound_in_its_own_table(hip_lib):
    from recman_amd import _lib

    syms = _declared()
    assert syms == sorted(["rm_topk_ip_supported", "rm_topk_ip_tile", "rm_topk_ip_workspace", "rm_topk_ip"])
    for name in syms:
        assert hasattr(hip_lib, name), f"{name} declared in recman_hip_topk.h but not exported"
    assert set(_lib.SIGNATURES_TOPK) == set(syms), set(_lib.SIGNATURES_TOPK) ^ set(syms)
    assert not set(_lib.SIGNATURES_TOPK) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_I64))
    assert hip_lib.rm_topk_ip_workspace.restype is ctypes.c_int64 and hip_lib.rm_topk_ip.restype is ctypes.c_int
    # recman_hip.h itself declares none of them
    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    assert "rm_topk" not in text


def test_ledger_covers_every_entry_point_with_a_stream():
    from tests import test_gpu_topk as T

    entries = _stream_entry_points()
    assert entries == {"rm_topk_ip"}
    assert set(T.COVERED) == entries
    for entry, test in T.COVERED.items():
        fn = getattr(T, test)
        assert "lds_pattern" in inspect.signature(fn).parameters, f"{test} does not run under lds_pattern"


# ------------------------------------------------------------------------------------------------------ the limits
def _call(hip_lib, k=5, H=8, ldq=8, ldc=8, Nq=3, N=10, splits=0, ldo=None):
    """rm_topk_ip with stand-in operand pointers and NULL outputs and workspace: nothing can be launched."""
    rc = hip_lib.rm_topk_ip(4096, ldq, 8192, ldc, Nq, N, H, 1.0, k, None, None, splits, None, None,
                            k if ldo is None else ldo, None, None)
    return rc, hip_lib.rm_last_error().decode()


@pytest.mark.parametrize("kw,match", [
    (dict(k=0), r"k=0 out of range .*k in 1\.\.1024"),
    (dict(k=1025), r"k=1025 out of range .*k in 1\.\.1024"),
    (dict(H=2, ldq=4, ldc=4), r"H=2 unsupported .*H a multiple of 4 in 4\.\.256"),
    (dict(H=260, ldq=260, ldc=260), r"H=260 unsupported .*H a multiple of 4 in 4\.\.256"),
    (dict(ldc=10), r"ldc=10 .*ldq and ldc multiples of 4"),
    (dict(ldq=4), r"ldq=4 < H=8"),
    (dict(splits=65), r"item_splits=65 out of range .*item_splits 0\.\.64"),
    (dict(Nq=-1), r"bad Nq=-1"),
])
def test_every_limit_raises_without_a_gpu(hip_lib, kw, match):
    rc, msg = _call(hip_lib, **kw)
    assert rc == -1, (rc, msg)  # RM_EINVAL
    assert re.search(match, msg), msg


def test_size_queries_and_the_empty_call(hip_lib):
    from recman_amd import ops

    assert ops.topk_ip_supported(4, 1) and ops.topk_ip_supported(256, 1024)
    assert not ops.topk_ip_supported(2, 10) and not ops.topk_ip_supported(8, 0) and not ops.topk_ip_supported(8, 1025)
    assert ops.topk_ip_tile(64) == 64 and ops.topk_ip_tile(256, "cols") == 32 and ops.topk_ip_tile(8, "max_splits") == 64
    with pytest.raises(ValueError, match="unsupported"):
        ops.topk_ip_tile(6)
    with pytest.raises(ValueError, match="unsupported"):
        ops.topk_ip_workspace(4, 10, 8, 2000)
    # linear in Nq; it covers 64 splits of 2 x 128 keys (2 floats each) per query when the catalogue has 64 tiles
    w1 = ops.topk_ip_workspace(1, 100000, 64, 100)
    assert ops.topk_ip_workspace(7, 100000, 64, 100) == 7 * w1 and w1 >= 64 * 2 * 256
    assert ops.topk_ip_workspace(1, 64, 64, 100) < w1  # one tile: one split
    assert ops.topk_ip_workspace(0, 10, 8, 5) == 0
    assert _call(hip_lib, Nq=0)[0] == 0  # Nq = 0: RM_OK before the pointers are looked at


# --------------------------------------------------------------------------------------------------- th.TwoTower
def _model(**kw):
    import recman_amd.th as th

    fd = th.FeatureDictionary()
    for n, v in (("u0", 3), ("u1", 4), ("it", 5), ("cat", 2)):
        fd[n] = th.SparseFeat(n, v)
    fd["du"], fd["di"] = th.DenseFeat("du"), th.DenseFeat("di")
    args = dict(user_features=("u0", "u1", "du"), item_features=("it", "cat", "di"), item_id_feature="it",
                user_hidden_units=(16, 8), item_hidden_units=(8,))
    args.update(kw)
    return th.TwoTower(fd, **args)


def test_twotower_retrieval_errors_before_any_gpu_work():
    import pandas as pd

    m = _model(recall_at=(1, 5))
    assert m.catalogue_metric_names == ["catalogue_recall@1", "catalogue_recall@5"]
    df = pd.DataFrame(dict(u0=[1, 2], u1=[1, 1], du=[0.5, 1.0], it=[1, 2], cat=[1, 1], di=[0.0, 1.0]))
    with pytest.raises(RuntimeError, match="index_items"):
        m.retrieve(df, 10)
    with pytest.raises(RuntimeError, match="index_items"):
        m.evaluate_catalogue(df)
    with pytest.raises(KeyError, match="item_id_feature"):
        m.index_items(df.drop(columns=["it"]))
    m2 = _model(item_id_feature=None, mask_accidental_hits=False)
    with pytest.raises(ValueError, match="item_id_feature"):
        m2.evaluate_catalogue(df)
    m._index = dict(emb=None, item_id=None)  # past the index check: the arguments are checked next
    with pytest.raises(ValueError, match="1..1024"):
        m.retrieve(df, 0)
    with pytest.raises(ValueError, match="1..1024"):
        m.retrieve(df, 1025)
    with pytest.raises(ValueError, match="exclude"):
        m.retrieve(df, 3, exclude=[[1]])
    assert m._engine is None and m2._engine is None  # nothing was built on the GPU
    assert "brute-force" not in " ".join(type(m).__doc__.split())
