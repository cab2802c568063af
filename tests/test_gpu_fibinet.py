"""GPU: FiBiNET's interaction kernels (csrc/fibinet.hip) through recman_amd.ops against the float64 restatement
(tests/fibinet_ref.py).  Tolerances: |X - X64| <= 1e-5 max(1, |X64|) (with N(0,1) rows |X| reaches about 28 at F = 26,
so the project's plain 1e-5 absolute does not fit), dE the project's gradient measure at 2e-5, the four batch-summed
parameter gradients the measure against max(2e-5, 4 x the float32 CPU restatement's own error on the case).  Every case
runs at three layouts - contiguous, ldx = 2PD + 4, and ldx rounded up to 8 plus 4, the padded ones in NaN-filled
buffers whose pad columns must still be NaN afterwards - and twice: all bits must agree.  A fourth layout, ldx = 2PD + 1,
has rows that are not 16-byte aligned (the kernels' narrow loads)."""
import ctypes

import pytest
import torch

from tests import fibinet_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")
GRADS = ("dE",) + tuple("d_" + n for n in R.PARAMS)


def _grid_stride_B():
    """The smallest B at which BOTH kernels' block loops run a second time at F = 3, D = 8, R = 1, type "all": both
    tiles hold 16 examples (the cap: the LDS budget would allow more) and both grids are capped at 512 blocks, so
    B = 512 * 16 + 1 = 8193."""
    from recman_amd import ops

    return max(ops.FIBINET_FWD_BLOCKS * ops.fibinet_tile(3, 8, 1, "all"),
               ops.FIBINET_BWD_BLOCKS * ops.fibinet_tile(3, 8, 1, "all", backward=True)) + 1


def _ld(W, which):
    return {0: W, 1: W + 4, 2: (W + 7) // 8 * 8 + 4, 3: W + 1}[which]


def _run(case, which):
    """One forward + backward at a layout: -> dict of output tensors (contiguous copies)."""
    from recman_amd import ops

    B, F, D, Rr, btype = (case[n] for n in ("B", "F", "D", "R", "btype"))
    W = 2 * R.pairs(F) * D
    ld = _ld(W, which)
    E = case["E"].to(F32).cuda()
    ws = [w.cuda() for w in R.case_weights(case, F32)]
    Xbuf = torch.full((B, ld), NAN, dtype=F32, device="cuda")
    dXbuf = torch.full((B, ld), NAN, dtype=F32, device="cuda")
    X, dX = Xbuf[:, :W], dXbuf[:, :W]
    dX.copy_(case["dX"].to(F32))
    ops.fibinet_fwd(E, *ws, btype, X)
    dE = torch.full((B, F, D), NAN, dtype=F32, device="cuda")
    dws = [torch.full(tuple(w.shape), NAN, dtype=F32, device="cuda") for w in ws]
    wsp = torch.full((max(1, ops.fibinet_bwd_workspace(B, F, D, Rr, btype)),), NAN, dtype=F32, device="cuda")
    ops.fibinet_bwd(E, *ws, btype, dX, dE, *dws, wsp)
    torch.cuda.synchronize()
    if ld > W:  # the pad columns are untouched
        assert bool(torch.isnan(Xbuf[:, W:]).all()), "X's buffer: columns past 2PD were written"
        assert bool(torch.isnan(dXbuf[:, W:]).all())
    out = dict(X=X.contiguous(), dE=dE)
    out.update({"d_" + n: g for n, g in zip(R.PARAMS, dws)})
    return out


def _check(case, what):
    B = case["B"]
    first = _run(case, 0)
    for n, v in first.items():
        assert bool(torch.isfinite(v).all()), f"{what}{n} is not finite"
    for which in (0, 1, 2, 3):
        again = _run(case, which)
        for n in first:
            assert torch.equal(first[n], again[n]), f"{what}{n}: layout {which} differs in its bits"
    err_x = R.x_error(first["X"], case["X"])
    ms = {n: R.grad_measure(first[n], case[n]) for n in GRADS}
    f32 = R.f32_errors(case)
    bounds = {n: max(R.TOL_GRAD, 4 * e) for n, e in zip(GRADS[1:], f32[2:])}
    print(f"{what}X err {err_x:.2e} (float32 CPU {f32[0]:.2e}); measures dE {ms['dE']:.2e} ({f32[1]:.2e}) "
          + " ".join(f"{n} {ms[n]:.2e} ({e:.2e}, bound {bounds[n]:.2e})" for n, e in zip(GRADS[1:], f32[2:])))
    assert err_x <= R.TOL_X, f"{what}|X - X64| / max(1, |X64|) = {err_x:.3g}"
    assert ms["dE"] <= R.TOL_GRAD, f"{what}dE measure {ms['dE']:.3g}"
    for n in GRADS[1:]:
        assert ms[n] <= bounds[n], f"{what}{n} measure {ms[n]:.3g} > {bounds[n]:.3g}"
    if B > 8:
        assert float(first["X"][3].abs().max()) == 0.0 and float(first["dE"][3].abs().max()) == 0.0, "E = 0 row"
        assert float(first["dE"][4].abs().max()) == 0.0, "dX = 0 row"


@pytest.mark.parametrize("shape", R.GPU_CASES, ids=lambda s: "B%d_F%d_D%d_R%d_%s" % s)
def test_fibinet_kernels_match_float64(hip_lib, shape):
    _check(R.kernel_case(*shape), "(B, F, D, R, type) = %s: " % (shape,))


def test_fibinet_grid_stride(hip_lib):
    """F = 3, D = 8, R = 1 at the smallest B that makes both kernels' block loops run a second time (8193)."""
    from recman_amd import ops

    B = _grid_stride_B()
    G = ops.fibinet_tile(3, 8, 1, "all", backward=True)
    assert ops.fibinet_tile(3, 8, 1, "all") == 16 and G == 16
    assert B == 8193 and B < 300000
    # the backward's grid is capped: its workspace holds fewer partial gradients than the batch has tiles
    N = 2 * 64 + 2 * 3
    assert ops.fibinet_bwd_workspace(B, 3, 8, 1, "all") == ops.FIBINET_BWD_BLOCKS * N
    assert ops.fibinet_bwd_workspace(B - 1, 3, 8, 1, "all") == ops.FIBINET_BWD_BLOCKS * N
    assert ops.fibinet_bwd_workspace(B - 1 - G, 3, 8, 1, "all") == (ops.FIBINET_BWD_BLOCKS - 1) * N
    assert ops.fibinet_bwd_workspace(G * 7 + 1, 3, 8, 1, "all") == 8 * N
    assert ops.fibinet_bwd_workspace(B, 3, 8, 1, "each") == ops.FIBINET_BWD_BLOCKS * (2 * 2 * 64 + 2 * 3)
    # the largest weight sets get fewer blocks: 32 MB of partials at most, but never fewer than 128 blocks
    assert ops.fibinet_bwd_workspace(1 << 20, 26, 16, 8, "each") == 512 * (2 * 25 * 256 + 2 * 26 * 8)
    assert ops.fibinet_bwd_workspace(1 << 20, 40, 16, 13, "each") == ((8 << 20) // 21008) * 21008 == 399 * 21008
    assert ops.fibinet_bwd_workspace(1 << 20, 40, 32, 13, "each") == 128 * (2 * 39 * 1024 + 2 * 40 * 13)
    _check(R.kernel_case(B, 3, 8, 1, "all"), "grid stride: ")


def test_supported_range(hip_lib):
    from recman_amd import ops

    for F in (0, 1, 2, 3, 26, 40, 41):
        for D in (0, 4, 8, 12, 16, 32, 64):
            for Rr in (0, 1, 2, F, F + 1):
                for btype in ("all", "each", "interaction"):
                    want = D in (8, 16, 32) and 2 <= F <= 40 and 1 <= Rr <= F and btype in ("all", "each")
                    assert ops.fibinet_supported(F, D, Rr, btype) == want, (F, D, Rr, btype)
    assert hip_lib.rm_fibinet_supported(26, 16, 8, 2) == 0 and hip_lib.rm_fibinet_supported(26, 16, 8, -1) == 0
    assert ops.fibinet_width(26, 16) == (10400, 10400) and ops.fibinet_width(2, 8) == (16, 16)
    # the tiles: what the LDS budget leaves, at least one example
    for F, D, Rr, btype in ((2, 8, 1, "each"), (26, 16, 8, "each"), (26, 16, 8, "all"), (40, 32, 13, "each"),
                            (40, 32, 40, "all")):
        assert 1 <= ops.fibinet_tile(F, D, Rr, btype) <= 16 and 1 <= ops.fibinet_tile(F, D, Rr, btype, True) <= 16


def test_unsupported_shapes_and_bad_arguments_raise_and_launch_nothing(hip_lib):
    from recman_amd import ops

    z = lambda *s: torch.full(s, NAN, dtype=F32, device="cuda")  # noqa: E731
    for F, D, Rr in ((1, 8, 1), (41, 8, 2), (3, 12, 1), (3, 64, 1), (3, 8, 4)):
        W = max(F * (F - 1) * D, 1)
        with pytest.raises(ValueError, match="unsupported"):
            ops.fibinet_fwd(z(4, F, D), z(F, Rr), z(Rr, F), z(1, D, D), z(1, D, D), "all", z(4, W))
        with pytest.raises(ValueError, match="unsupported"):
            ops.fibinet_bwd(z(4, F, D), z(F, Rr), z(Rr, F), z(1, D, D), z(1, D, D), "all", z(4, W), z(4, F, D),
                            z(F, Rr), z(Rr, F), z(1, D, D), z(1, D, D), z(8))
        with pytest.raises(ValueError, match="unsupported"):
            ops.fibinet_bwd_workspace(4, F, D, Rr, "all")
        assert hip_lib.rm_fibinet_bwd_workspace(4, F, D, Rr, 0) == -1
    with pytest.raises(ValueError, match="unsupported"):
        ops.fibinet_fwd(z(4, 3, 8), z(3, 1), z(1, 3), z(3, 8, 8), z(3, 8, 8), "interaction", z(4, 48))
    assert hip_lib.rm_fibinet_bwd_workspace(-1, 3, 8, 1, 0) == -1 and hip_lib.rm_fibinet_bwd_workspace(0, 3, 8, 1, 0) == 0
    # the C entry points themselves: an unsupported shape, a NULL pointer, a stride below the width
    E, W1, W2, Wb, Wsb, X = z(4, 3, 8), z(3, 1), z(1, 3), z(2, 8, 8), z(2, 8, 8), z(4, 48)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = [P(E), P(W1), P(W2), P(Wb), P(Wsb), 4, 3, 8, 1, 1, P(X), 48, st]
    assert len(ok) == 13
    for pos, val, msg in ((6, 1, "F=1"), (6, 41, "F=41"), (7, 12, "D=12"), (7, 64, "D=64"), (8, 0, "R=0"), (8, 4, "R=4"),
                          (9, 2, "type=2"), (5, -1, "batch"), (0, None, "E is NULL"), (1, None, "W1 is NULL"),
                          (2, None, "W2 is NULL"), (3, None, "Wb is NULL"), (4, None, "Wsb is NULL"),
                          (10, None, "X is NULL"), (11, 47, "ldx")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_fibinet_fwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    dE, dW1, dW2, dWb, dWsb, wsp = z(4, 3, 8), z(3, 1), z(1, 3), z(2, 8, 8), z(2, 8, 8), z(1024)
    ok = [P(E), P(W1), P(W2), P(Wb), P(Wsb), P(X), 48, 4, 3, 8, 1, 1, P(dE), P(dW1), P(dW2), P(dWb), P(dWsb), P(wsp), st]
    for pos, val, msg in ((8, 1, "F=1"), (9, 12, "D=12"), (10, 4, "R=4"), (11, 2, "type=2"), (7, -1, "batch"),
                          (0, None, "E is NULL"), (1, None, "W1 is NULL"), (4, None, "Wsb is NULL"),
                          (5, None, "dX is NULL"), (12, None, "dE is NULL"), (13, None, "dW1 is NULL"),
                          (14, None, "dW2 is NULL"), (15, None, "dWb is NULL"), (16, None, "dWsb is NULL"),
                          (17, None, "workspace is NULL"), (6, 47, "lddx")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_fibinet_bwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    torch.cuda.synchronize()
    for t in (X, dE, dW1, dW2, dWb, dWsb, wsp):
        assert bool(torch.isnan(t).all()), "a refused call launched something"
    # ops' own argument checks
    E, W1, W2, Wb, X = (torch.zeros(s, dtype=F32, device="cuda") for s in ((4, 3, 8), (3, 1), (1, 3), (2, 8, 8), (4, 48)))
    with pytest.raises(ValueError, match=r"expected \[B,F,D\]"):
        ops.fibinet_fwd(E[0], W1, W2, Wb, Wb, "each", X)
    with pytest.raises(ValueError, match="expected shape"):
        ops.fibinet_fwd(E, W1, W2, Wb[:1], Wb, "each", X)  # "each" needs F - 1 matrices
    with pytest.raises(ValueError, match="expected shape"):
        ops.fibinet_fwd(E, W1, W2[:, :2].contiguous(), Wb, Wb, "each", X)
    with pytest.raises(ValueError, match="must be"):
        ops.fibinet_fwd(E, W1, W2, Wb, Wb, "each", X[:, :40])
    with pytest.raises(ValueError, match="must be"):
        ops.fibinet_fwd(E, W1, W2, Wb, Wb, "each", X[:3])
    with pytest.raises(ValueError, match="unit column stride"):
        ops.fibinet_fwd(E, W1, W2, Wb, Wb, "each", torch.zeros(4, 96, dtype=F32, device="cuda")[:, ::2])
    with pytest.raises(ValueError, match="float32"):
        ops.fibinet_fwd(E, W1, W2, Wb, Wb, "each", X.double())
    with pytest.raises(ValueError, match="device"):
        ops.fibinet_fwd(E, W1, W2, Wb, Wb, "each", X.cpu())
    with pytest.raises(TypeError):
        ops.fibinet_fwd(E.double(), W1, W2, Wb, Wb, "each", X)
    with pytest.raises(ValueError, match="GPU"):
        ops.fibinet_fwd(E, W1.cpu(), W2, Wb, Wb, "each", X)
    with pytest.raises(ValueError, match="workspace too small"):
        ops.fibinet_bwd(E, W1, W2, Wb, Wb, "each", X, E.clone(), W1.clone(), W2.clone(), Wb.clone(), Wb.clone(),
                        torch.zeros(3, dtype=F32, device="cuda"))
    with pytest.raises(ValueError, match="expected shape"):
        ops.fibinet_bwd(E, W1, W2, Wb, Wb, "each", X, E[:3].clone(), W1.clone(), W2.clone(), Wb.clone(), Wb.clone(),
                        torch.zeros(1024, dtype=F32, device="cuda"))


def test_empty_batch(hip_lib):
    from recman_amd import ops

    W1, W2, Wb = (torch.randn(s, device="cuda") for s in ((3, 1), (1, 3), (2, 8, 8)))
    E, X = torch.zeros(0, 3, 8, dtype=F32, device="cuda"), torch.zeros(0, 48, dtype=F32, device="cuda")
    ops.fibinet_fwd(E, W1, W2, Wb, Wb, "each", X)
    assert ops.fibinet_bwd_workspace(0, 3, 8, 1, "each") == 0
    dws = [torch.full(tuple(w.shape), NAN, dtype=F32, device="cuda") for w in (W1, W2, Wb, Wb)]
    ops.fibinet_bwd(E, W1, W2, Wb, Wb, "each", X, E.clone(), *dws, torch.zeros(1, dtype=F32, device="cuda"))
    torch.cuda.synchronize()
    for g in dws:
        assert float(g.abs().max()) == 0.0  # the sums over an empty batch
