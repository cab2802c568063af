"""GPU: rm_dot_interact_fwd / rm_dot_interact_bwd through the C ABI (recman_amd.ops) against the float64 restatement
(tests/dlrm_ref.py, pinned on the CPU by tests/test_dlrm_host.py).

Bounds (tests/dlrm_ref.py:fwd_bound / bwd_bound): |X - X64| <= D 2^-23 sum_k |v_ik v_jk| and
|dV - dV64| <= (T+1) 2^-23 sum_j |G_ij| |v_jk| elementwise (dz: with its pass-through addend in the sum) - the textbook
n 2^-24 sum |a b| of a sum of n products in ANY order, which an fmaf chain also meets, doubled for the neglected
second-order term.  A wrong index or a missing term exceeds them by orders of magnitude (shown on the CPU).  X[:, :D] is
z bit for bit, the columns from D + P up to the row stride are +0.0, every output is finite.  The observed maxima are
printed as a fraction of the bound.

Every case runs at three row strides: D + P (rows unaligned whenever D + P is odd), that rounded up to a multiple of 4,
and 4 more.  X, d_rows, dz and dX's columns >= D + P are NaN before each launch.

Grid-stride loop: the kernels take G = min(16, 16 KB / LDS bytes per example) examples per block and at most 2048
blocks, so the loop runs a second time from B > 2048 G; at (70001, 3, 8) G = 16 and B > 32768."""
import pytest
import torch

from tests import dlrm_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
_ids = lambda c: "x".join(map(str, c))  # noqa: E731
NAN = float("nan")


def _dev(t):
    return t.to(F32).cuda().contiguous()


def _strides(F, D):
    from recman_amd import ops

    W, W4 = ops.dot_interact_width(F, D)
    assert W == D + R.pairs(F) and W4 % 4 == 0 and 0 <= W4 - W < 4
    return W, (W, W4, W4 + 4)


def _run(case, ldx, whole=False):
    """The kernels on a case's tensors with X / dX rows ldx floats apart: (the whole X buffer [B, ldx], d_rows, dz).
    whole: the ops get the [B, ldx] buffers themselves, otherwise their [B, D+P] views."""
    from recman_amd import ops

    B, F, D = case["B"], case["F"], case["D"]
    W = D + R.pairs(F)
    E, z = _dev(case["E"]), _dev(case["z"])
    Xb = torch.full((B, ldx), NAN, device="cuda")
    dXb = torch.full((B, ldx), NAN, device="cuda")
    dXb[:, :W] = _dev(case["dX"])
    d_rows, dz = torch.full((B, F, D), NAN, device="cuda"), torch.full((B, D), NAN, device="cuda")
    ops.dot_interact_fwd(E, z, Xb if whole else Xb[:, :W])
    ops.dot_interact_bwd(E, z, dXb if whole else dXb[:, :W], d_rows, dz)
    torch.cuda.synchronize()
    return Xb, d_rows, dz


@pytest.mark.parametrize("c", R.GPU_CASES, ids=_ids)
def test_dot_interact_matches_float64(hip_lib, c):
    case = R.kernel_case(*c)
    W, strides = _strides(c[1], c[2])
    first = None
    for n, ldx in enumerate(strides):
        X, d_rows, dz = _run(case, ldx, whole=(n == 2))
        tag = f"{c} ldx={ldx}: "
        rx = R.check_fwd(X, case, tag)
        rr, rz = R.check_bwd(d_rows, dz, case, tag)
        print(f"{tag}err / bound: X {rx:.3f}, d_rows {rr:.3f}, dz {rz:.3f}")
        # the same bits at every row stride, and on a second run
        if first is None:
            first = (X[:, :W].clone(), d_rows, dz)
            again = _run(case, ldx)
            assert torch.equal(again[0], X) and torch.equal(again[1], d_rows) and torch.equal(again[2], dz)
        else:
            assert torch.equal(X[:, :W], first[0]) and torch.equal(d_rows, first[1]) and torch.equal(dz, first[2])


def test_supported_range(hip_lib):
    from recman_amd import ops

    for F in (1, 2, 26, 40):
        for D in (8, 16, 32, 64):
            assert ops.dot_interact_supported(F, D)
    for F, D in ((0, 16), (41, 16), (-1, 16), (5, 12), (5, 4), (5, 128), (5, 0), (5, 24)):
        assert not ops.dot_interact_supported(F, D)
    assert ops.dot_interact_width(26, 16) == (367, 368) and ops.dot_interact_width(7, 16) == (44, 44)
    assert ops.dot_interact_width(1, 8) == (9, 12)


@pytest.mark.parametrize("F,D", [(5, 12), (0, 16), (41, 16)])
def test_unsupported_shapes_raise_and_launch_nothing(hip_lib, F, D):
    from recman_amd import _lib, ops

    B, W = 4, D + R.pairs(F)
    E, z = torch.randn(B, F, D, device="cuda"), torch.randn(B, D, device="cuda")
    X, dX = torch.full((B, W + 3), NAN, device="cuda"), torch.randn(B, W + 3, device="cuda")
    d_rows, dz = torch.full((B, F, D), NAN, device="cuda"), torch.full((B, D), NAN, device="cuda")
    with pytest.raises(ValueError, match="unsupported"):
        ops.dot_interact_fwd(E, z, X)
    with pytest.raises(ValueError, match="unsupported"):
        ops.dot_interact_bwd(E, z, dX, d_rows, dz)
    # ... and the C entry points themselves refuse before any launch
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        _lib.call("rm_dot_interact_fwd", E.data_ptr(), z.data_ptr(), B, F, D, X.data_ptr(), W + 3, st)
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        _lib.call("rm_dot_interact_bwd", E.data_ptr(), z.data_ptr(), dX.data_ptr(), W + 3, B, F, D,
                  d_rows.data_ptr(), dz.data_ptr(), st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(X).all()) and bool(torch.isnan(dz).all())
    assert d_rows.numel() == 0 or bool(torch.isnan(d_rows).all())


def test_argument_checks_and_an_empty_batch(hip_lib):
    from recman_amd import _lib, ops

    F, D = 3, 8
    W = D + R.pairs(F)
    E, z = torch.randn(4, F, D, device="cuda"), torch.randn(4, D, device="cuda")
    with pytest.raises(ValueError):
        ops.dot_interact_fwd(E, z, torch.empty(4, W - 1, device="cuda"))  # too narrow
    with pytest.raises(ValueError):
        ops.dot_interact_fwd(E, z, torch.empty(3, W, device="cuda"))  # rows
    with pytest.raises(ValueError):
        ops.dot_interact_fwd(E, z[:, :4].contiguous(), torch.empty(4, W, device="cuda"))
    with pytest.raises(TypeError):
        ops.dot_interact_fwd(E.double(), z, torch.empty(4, W, device="cuda"))
    with pytest.raises(ValueError):
        ops.dot_interact_fwd(E, z, torch.empty(W, 4, device="cuda").t())  # column stride
    with pytest.raises(_lib.RecmanHipError, match="ldx"):
        _lib.call("rm_dot_interact_fwd", E.data_ptr(), z.data_ptr(), 4, F, D, E.data_ptr(), W - 1,
                  torch.cuda.current_stream().cuda_stream)
    # B = 0 is accepted
    E0, z0 = torch.empty(0, F, D, device="cuda"), torch.empty(0, D, device="cuda")
    ops.dot_interact_fwd(E0, z0, torch.empty(0, W, device="cuda"))
    ops.dot_interact_bwd(E0, z0, torch.empty(0, W, device="cuda"), torch.empty(0, F, D, device="cuda"),
                         torch.empty(0, D, device="cuda"))
    torch.cuda.synchronize()
