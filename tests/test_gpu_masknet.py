"""GPU: the MaskNet kernels (csrc/masknet.hip) through recman_amd.ops against the float64 restatement
(tests/masknet_ref.py): |Y - Y64| <= 1e-5 max(1, |Y64|), every gradient at the project's gradient measure 2e-5, outputs
pre-filled with NaN, every case twice with all bits equal."""
import ctypes

import pytest
import torch

from tests import masknet_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
EPS32 = 2.0 ** -23


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device="cuda")


def _dev(t):
    return t.to(F32).cuda()


def _in_rows(t, pad, col0=0):
    """t [B,W] as columns [col0, col0 + W) of a NaN-filled buffer whose rows are W + pad floats."""
    B, W = t.shape
    buf = _nan(B, W + pad)
    view = buf[:, col0: col0 + W]
    view.copy_(t)
    return view


def _out_rows(B, W, pad, col0=0):
    return _nan(B, W + pad)[:, col0: col0 + W]


def _one_ulp(got, want):
    return bool(((got - want).abs() <= EPS32 * want.abs()).all())


def _group_run(c, pad, one_buffer=False, in_place=False, dE_up=None, alias=False):
    """-> (Y list, dM list, d_rows, dgamma, dbeta) of one forward + backward."""
    from recman_amd import ops

    B, F, D, N = c["B"], c["F"], c["D"], c["N"]
    W = F * D
    E, gamma, beta = _dev(c["E"]), _dev(c["gamma"]), _dev(c["beta"])
    M = [_in_rows(_dev(m), pad) for m in c["M"]]
    if one_buffer:  # the N outputs side by side in one buffer, as the engine could lay them out
        big = _nan(B, N * W + pad)
        Y = [big[:, n * W: (n + 1) * W] for n in range(N)]
    else:
        Y = [_out_rows(B, W, pad) for _ in range(N)]
    ops.masknet_group_fwd(E, gamma, beta, M, Y)
    dY = [_in_rows(_dev(d), pad) for d in c["dY"]]
    dM = dY if in_place else [_out_rows(B, W, pad) for _ in range(N)]
    d_rows, dg, db = _nan(B, F, D), _nan(F, D), _nan(F, D)
    if alias:  # d_rows is dE_up itself
        d_rows = dE_up = dE_up.clone()
    ws = _nan(max(4, ops.masknet_group_bwd_workspace(B, F, D)))
    ops.masknet_group_bwd(E, gamma, beta, M, dY, dM, d_rows, dg, db, ws, dE_up=dE_up)
    torch.cuda.synchronize()
    return [y.clone() for y in Y], [d.clone() for d in dM], d_rows, dg, db


def _check_group(c, out, what):
    Y, dM, d_rows, dg, db = out
    for t in Y + dM + [d_rows, dg, db]:
        assert bool(torch.isfinite(t).all()), f"{what}: an output was not written"
    fwd, bwd = R.group_errors(c, Y, dM, d_rows, dg, db)
    print(f"{what}: Y {fwd:.2e} gradients {bwd:.2e}")
    assert fwd <= R.TOL_Y, (what, fwd)
    for name, got, want in [(f"dM{n}", a, b) for n, (a, b) in enumerate(zip(dM, c["dM"]))] + [
            ("dE", d_rows, c["dE"]), ("dgamma", dg, c["dgamma"]), ("dbeta", db, c["dbeta"])]:
        m = R.grad_measure(got, want)
        assert m <= R.TOL_GRAD, (what, name, m)


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0] + a[1] + list(a[2:]), b[0] + b[1] + list(b[2:])))


@pytest.mark.parametrize("shape", R.GROUP_CASES, ids=lambda s: "B%d_F%d_D%d_N%d" % s)
def test_group_kernels_match_float64(hip_lib, shape):
    c = R.kernel_case(*shape)
    B, F, D, N = shape
    first = _group_run(c, pad=4, one_buffer=(shape == (70, 5, 16, 3)))
    _check_group(c, first, f"group {shape}")
    assert _same_bits(first, _group_run(c, pad=4)), "two runs differ"
    if B > 8:
        # the all-zero example: xhat = 0, Y = M o beta, not NaN; zero upstream gradient: dE = 0
        beta = _dev(c["beta"]).reshape(-1)
        for y, m in zip(first[0], c["M"]):
            assert torch.equal(y[R.EX_ZERO], _dev(m)[R.EX_ZERO] * beta)
        assert float(first[2][R.EX_NO_GRAD].abs().max()) == 0.0
    # dM written over dY: the same bits
    assert _same_bits(first, _group_run(c, pad=4, in_place=True)), "dM over dY differs"
    # a third run with dE_up adds it to one ulp (d_rows may be dE_up itself)
    up = _dev(c["dE_up"])
    third = _group_run(c, pad=4, dE_up=up)
    assert _one_ulp(third[2], up + first[2])
    assert _same_bits(first[:2] + first[3:], third[:2] + third[3:])
    assert _same_bits(third, _group_run(c, pad=4, dE_up=up, alias=True)), "d_rows as dE_up itself differs"


def test_group_kernels_with_rows_of_any_stride(hip_lib):
    """Row strides that are no multiple of 4 floats (and so no 16-byte rows) take per-element accesses: the same
    bits."""
    c = R.kernel_case(70, 5, 16, 3)
    odd = _group_run(c, pad=3)
    _check_group(c, odd, "odd strides")
    assert _same_bits(odd, _group_run(c, pad=4))
    assert _same_bits(odd, _group_run(c, pad=0))


def _plain_run(c, pad, dE_up=None):
    from recman_amd import ops

    B, H = c["B"], c["H"]
    X, M = _dev(c["X"]), [_in_rows(_dev(c["M"]), pad)]
    Y = [_out_rows(B, H, pad)]
    ops.masknet_group_fwd(X, None, None, M, Y, normalize=False)
    dY = [_in_rows(_dev(c["dY"]), pad)]
    dM, dX = [_out_rows(B, H, pad)], _nan(B, H)
    ops.masknet_group_bwd(X, None, None, M, dY, dM, dX, dE_up=dE_up, normalize=False)
    torch.cuda.synchronize()
    return Y[0].clone(), dM[0].clone(), dX


def _check_plain(c, out, what):
    Y, dM, dX = out
    assert all(bool(torch.isfinite(t).all()) for t in out)
    assert R.logit_error(Y, c["Y"]) <= R.TOL_Y, what
    assert R.grad_measure(dM, c["dM"]) <= R.TOL_GRAD and R.grad_measure(dX, c["dX"]) <= R.TOL_GRAD, what


@pytest.mark.parametrize("shape", R.PLAIN_CASES, ids=lambda s: "B%d_H%d" % s)
def test_group_kernels_without_normalisation(hip_lib, shape):
    c = R.plain_case(*shape)
    first = _plain_run(c, pad=4)
    _check_plain(c, first, f"plain {shape}")
    assert all(torch.equal(a, b) for a, b in zip(first, _plain_run(c, pad=4)))
    up = _dev(c["dE_up"])
    third = _plain_run(c, pad=4, dE_up=up)
    assert _one_ulp(third[2], up + first[2]) and torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])


def _row_run(c, out_mul=3):
    """h lands in columns [H, 2H) of a buffer of row stride out_mul H, dh comes from such a buffer too."""
    from recman_amd import ops

    B, H = c["B"], c["H"]
    Z, gamma, beta = _dev(c["Z"]), _dev(c["gamma"]), _dev(c["beta"])
    col0 = H if out_mul > 1 else 0
    h = _out_rows(B, H, (out_mul - 1) * H, col0)
    ops.masknet_row_fwd(Z, gamma, beta, h)
    dh = _in_rows(_dev(c["dh"]), (out_mul - 1) * H, col0)
    dZ, dg, db = _nan(B, H), _nan(H), _nan(H)
    ops.masknet_row_bwd(Z, gamma, beta, dh, dZ, dg, db, _nan(max(4, ops.masknet_row_bwd_workspace(B, H))))
    torch.cuda.synchronize()
    return h.clone(), dZ, dg, db


def _check_row(c, out, what):
    h, dZ, dg, db = out
    assert all(bool(torch.isfinite(t).all()) for t in out), f"{what}: an output was not written"
    fwd = R.logit_error(h, c["h"])
    ms = [R.grad_measure(a, c[n]) for a, n in ((dZ, "dZ"), (dg, "dgamma"), (db, "dbeta"))]
    print(f"{what}: h {fwd:.2e} dZ {ms[0]:.2e} dgamma {ms[1]:.2e} dbeta {ms[2]:.2e}")
    assert fwd <= R.TOL_Y and max(ms) <= R.TOL_GRAD, (what, fwd, ms)
    assert bool(((h > 0).cpu() == (c["pre"] > 0)).all())  # no unit crossed its kink


@pytest.mark.parametrize("shape", R.ROW_CASES, ids=lambda s: "B%d_H%d" % s)
def test_row_kernels_match_float64(hip_lib, shape):
    c = R.row_case(*shape)
    first = _row_run(c)
    _check_row(c, first, f"row {shape}")
    assert all(torch.equal(a, b) for a, b in zip(first, _row_run(c))), "two runs differ"
    assert all(torch.equal(a, b) for a, b in zip(first, _row_run(c, out_mul=1))), "the output stride changes bits"
    if shape[0] > 8:
        # the all-zero row: xhat = 0, h = relu(beta); zero upstream gradient: dZ = 0
        assert torch.equal(first[0][R.EX_ZERO], torch.relu(_dev(c["beta"])))
        assert float(first[1][R.EX_NO_GRAD].abs().max()) == 0.0


def test_grid_stride_paths(hip_lib):
    """The smallest batch at which a block's loop runs twice, with a partial last tile: cap x tile + 1 examples."""
    from recman_amd import ops

    F, D = 3, 8
    tile, cap = ops.masknet_group_tile(F, D, "tile"), ops.masknet_group_tile(F, D, "cap")
    assert tile == 256 // (F * D // 4) and cap == 512
    c = R.kernel_case(cap * tile + 1, F, D, 2)
    first = _group_run(c, pad=4)
    _check_group(c, first, "group grid stride")
    assert _same_bits(first, _group_run(c, pad=4))
    assert ops.masknet_group_bwd_workspace(c["B"], F, D) == cap * tile * 2 * F * D
    H = 8
    tile, cap = ops.masknet_row_tile(H, "tile"), ops.masknet_row_tile(H, "cap")
    assert (tile, cap) == (128, 512)
    c = R.row_case(cap * tile + 1, H)
    first = _row_run(c)
    _check_row(c, first, "row grid stride")
    assert all(torch.equal(a, b) for a, b in zip(first, _row_run(c)))
    tile, cap = ops.masknet_group_tile(1, H, "tile", normalize=False), ops.masknet_group_tile(1, H, "cap", normalize=False)
    assert (tile, cap) == (128, 512)
    c = R.plain_case(cap * tile + 1, H)
    _check_plain(c, _plain_run(c, pad=4), "plain grid stride")


def test_supported_range_matches_the_query(hip_lib):
    from recman_amd import ops

    for F in (0, 1, 2, 26, 40, 41):
        for D in (4, 8, 12, 16, 32, 64):
            for N in (0, 1, 3, 8, 9):
                want = D in (8, 16, 32) and 1 <= F <= 40 and 1 <= N <= 8
                assert ops.masknet_group_supported(F, D, N) == want, (F, D, N)
                assert (hip_lib.rm_masknet_group_bwd_workspace(4, F, D) >= 0) == (D in (8, 16, 32) and 1 <= F <= 40)
    for H in (0, 4, 8, 10, 12, 100, 256, 2044, 2048, 2052, 4096):
        want = H % 4 == 0 and 8 <= H <= 2048
        assert ops.masknet_row_supported(H) == want, H
        assert ops.masknet_group_supported(1, H, 1, normalize=False) == want, H
        assert (hip_lib.rm_masknet_row_tile(H, 0) > 0) == want and (hip_lib.rm_masknet_row_bwd_workspace(4, H) > 0) == want
    assert not ops.masknet_group_supported(2, 8, 1, normalize=False)  # one [B,H] input
    assert not ops.masknet_group_supported(1, 8, 2, normalize=False)  # one mask
    assert hip_lib.rm_masknet_group_supported(3, 8, 1, 2) == 0 and hip_lib.rm_masknet_group_tile(3, 8, 1, 2) == -1
    # a thread owns one float4: 256 // (F D / 4) examples per pass, one example in two chunks past 256 float4
    assert ops.masknet_group_tile(26, 16, "tile") == 2 and ops.masknet_group_tile(40, 32, "tile") == 1
    assert ops.masknet_group_tile(1, 8, "tile") == 128
    assert [ops.masknet_row_tile(H, "tile") for H in (8, 12, 100, 256, 2048)] == [128, 64, 8, 4, 4]
    # the widest rows get fewer blocks: 16 MB of partial sets at most
    assert ops.masknet_row_tile(2048, "cap") == 256 and ops.masknet_row_tile(256, "cap") == 512
    assert ops.masknet_row_bwd_workspace(0, 256) == 0 and ops.masknet_group_bwd_workspace(0, 26, 16) == 0
    assert hip_lib.rm_masknet_row_bwd_workspace(-1, 256) == -1 and hip_lib.rm_masknet_group_bwd_workspace(-1, 3, 8) == -1
    with pytest.raises(ValueError, match="unsupported"):
        ops.masknet_row_tile(10, "tile")
    with pytest.raises(ValueError, match="unsupported"):
        ops.masknet_group_tile(3, 12, "cap")


def test_unsupported_shapes_and_bad_arguments_raise_and_launch_nothing(hip_lib):
    from recman_amd import ops

    for F, D in ((41, 8), (3, 12), (3, 64)):
        g = _nan(F, D)
        with pytest.raises(ValueError, match="unsupported"):
            ops.masknet_group_fwd(_nan(4, F, D), g, g, [_nan(4, F * D)], [_nan(4, F * D)])
        with pytest.raises(ValueError, match="unsupported"):
            ops.masknet_group_bwd(_nan(4, F, D), g, g, [_nan(4, F * D)], [_nan(4, F * D)], [_nan(4, F * D)],
                                  _nan(4, F, D), g.clone(), g.clone(), _nan(4096))
        with pytest.raises(ValueError, match="unsupported"):
            ops.masknet_group_bwd_workspace(4, F, D)
    E, g, M = _nan(4, 3, 8), _nan(3, 8), [_nan(4, 24) for _ in range(9)]
    with pytest.raises(ValueError, match="unsupported"):
        ops.masknet_group_fwd(E, g, g, M, [m.clone() for m in M])  # nine masks
    with pytest.raises(ValueError, match="unsupported"):
        ops.masknet_group_fwd(E, g, g, [], [])
    with pytest.raises(ValueError, match="unsupported"):
        ops.masknet_group_fwd(_nan(4, 10), None, None, [_nan(4, 10)], [_nan(4, 10)], normalize=False)
    for H in (4, 10, 2052):
        with pytest.raises(ValueError, match="unsupported"):
            ops.masknet_row_fwd(_nan(4, H), _nan(H), _nan(H), _nan(4, H))
        with pytest.raises(ValueError, match="unsupported"):
            ops.masknet_row_bwd(_nan(4, H), _nan(H), _nan(H), _nan(4, H), _nan(4, H), _nan(H), _nan(H), _nan(4096))
    # short or mixed row strides, strides the row kernels cannot take
    short = torch.as_strided(_nan(4 * 24), (4, 24), (20, 1))
    with pytest.raises(ValueError, match="unsupported row stride"):
        ops.masknet_group_fwd(E, g, g, [short], [_nan(4, 24)])
    with pytest.raises(ValueError, match="unsupported mix"):
        ops.masknet_group_fwd(E, g, g, [_nan(4, 24), _nan(4, 28)[:, :24]], [_nan(4, 24), _nan(4, 24)])
    with pytest.raises(ValueError, match="unsupported row stride"):
        ops.masknet_row_fwd(_nan(4, 8), _nan(8), _nan(8), _nan(4, 10)[:, :8])
    with pytest.raises(ValueError, match="unsupported row stride"):
        ops.masknet_row_fwd(_nan(4, 8), _nan(8), _nan(8), _nan(4, 12)[:, 1:9])  # rows off 16 bytes
    # the C entry points themselves: an unsupported shape, a short stride, a NULL pointer
    Mb, Yb, dg, db, d_rows, wsp = _nan(4, 24), _nan(4, 24), _nan(3, 8), _nan(3, 8), _nan(4, 3, 8), _nan(4096)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    arr = lambda *ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    null1 = (ctypes.c_void_p * 1)(None)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = [P(E), P(g), P(g), 1, arr(Mb), 24, 1, 4, 3, 8, arr(Yb), 24, st]
    for pos, val, msg in ((8, 41, "F=41"), (9, 12, "D=12"), (6, 9, "N=9"), (6, 0, "N=0"), (3, 2, "normalize=2"),
                          (7, -1, "batch"), (5, 23, "ldm=23"), (11, 20, "ldy=20"), (0, None, "NULL"),
                          (1, None, "NULL"), (4, None, "NULL"), (4, null1, "NULL mask"), (10, null1, "NULL mask")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_masknet_group_fwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    ok = [P(E), P(g), P(g), 1, arr(Mb), 24, arr(Yb), 24, arr(Yb), 24, 1, None, 4, 3, 8, P(d_rows), P(dg), P(db),
          P(wsp), st]
    for pos, val, msg in ((13, 0, "F=0"), (14, 64, "D=64"), (10, 9, "N=9"), (12, -1, "batch"), (7, 23, "lddy=23"),
                          (9, 25, "lddm = lddy"), (8, arr(Mb), "may overlap"), (0, None, "NULL"), (15, None, "NULL"), (16, None, "NULL"),
                          (18, None, "NULL"), (6, null1, "NULL mask")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_masknet_group_bwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    Z, g8, h, dZ = _nan(4, 8), _nan(8), _nan(4, 8), _nan(4, 8)
    ok = [P(Z), P(g8), P(g8), 4, 8, P(h), 8, st]
    for pos, val, msg in ((4, 10, "H=10"), (4, 4, "H=4"), (3, -1, "batch"), (6, 4, "ldh=4"), (6, 10, "ldh=10"),
                          (0, None, "NULL"), (5, None, "NULL")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_masknet_row_fwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    ok = [P(Z), P(g8), P(g8), P(h), 8, 4, 8, P(dZ), P(dg), P(db), P(wsp), st]
    for pos, val, msg in ((6, 2052, "H=2052"), (5, -1, "batch"), (4, 6, "lddh=6"), (3, None, "NULL"),
                          (7, None, "NULL"), (7, P(Z), "dZ must not be Z"), (7, P(h), "dZ must not be dh"),
                          (10, None, "NULL")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_masknet_row_bwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    torch.cuda.synchronize()
    for t in (Yb, dg, db, d_rows, wsp, h, dZ):
        assert bool(torch.isnan(t).all()), "a refused call launched something"
    with pytest.raises(ValueError, match="workspace too small"):
        ops.masknet_group_bwd(E, g, g, [Mb], [Yb], [Yb], d_rows, dg, db, _nan(3))
    with pytest.raises(ValueError, match="workspace too small"):
        ops.masknet_row_bwd(Z, g8, g8, h, dZ, _nan(8), _nan(8), _nan(3))
    with pytest.raises(ValueError, match="expected shape"):
        ops.masknet_group_fwd(E, _nan(3, 4), g, [Mb], [Yb])
    with pytest.raises(ValueError, match="takes no gamma"):
        ops.masknet_group_fwd(_nan(4, 8), g8, g8, [_nan(4, 8)], [_nan(4, 8)], normalize=False)
    with pytest.raises(ValueError, match="differ in length"):
        ops.masknet_group_fwd(E, g, g, [Mb], [Yb, Yb])


def test_empty_batch_touches_nothing(hip_lib):
    from recman_amd import ops

    E, g = torch.zeros(0, 3, 8, dtype=F32, device="cuda"), torch.ones(3, 8, dtype=F32, device="cuda")
    M = [torch.zeros(0, 24, dtype=F32, device="cuda")]
    ops.masknet_group_fwd(E, g, g, M, [M[0].clone()])
    dg, db, wsp = _nan(3, 8), _nan(3, 8), _nan(16)
    ops.masknet_group_bwd(E, g, g, M, [M[0].clone()], [M[0].clone()], E.clone(), dg, db, wsp)
    Z, g8 = torch.zeros(0, 8, dtype=F32, device="cuda"), torch.ones(8, dtype=F32, device="cuda")
    ops.masknet_row_fwd(Z, g8, g8, Z.clone())
    dg8, db8 = _nan(8), _nan(8)
    ops.masknet_row_bwd(Z, g8, g8, Z.clone(), Z.clone(), dg8, db8, wsp)
    ops.masknet_group_fwd(Z, None, None, [Z.clone()], [Z.clone()], normalize=False)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dg, db, wsp, dg8, db8))
