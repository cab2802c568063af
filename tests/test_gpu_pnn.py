"""GPU: the PNN product-layer kernels (csrc/pnn.hip) through recman_amd.ops against the float64 restatement
(tests/pnn_ref.py).  Tolerances, the project's own (tests/test_gpu_parity.py): every X element within 1e-5 max(1,
|X64|), d_rows and dK the gradient measure at 2e-5.  Every output buffer is pre-filled with NaN, the pad columns of dX
hold NaN (they are never read), and every case runs twice (all bits must agree)."""
import ctypes

import pytest
import torch

from tests import pnn_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")


def _nan(*shape):
    return torch.full(shape, NAN, dtype=F32, device="cuda")


def _run(case):
    from recman_amd import ops

    B, F, D, pr, kt, W, ldx = (case[n] for n in ("B", "F", "D", "products", "kernel_type", "W", "ldx"))
    E = case["E"].to(F32).cuda()
    K = case["K"].to(F32).cuda() if case["K"] is not None else None
    Xb, dXb = _nan(B, ldx), _nan(B, ldx)
    dXb[:, :W] = case["dX"].to(F32).cuda()
    d_rows = _nan(B, F, D)
    dK = _nan(*K.shape) if K is not None else None
    ws = _nan(max(1, ops.pnn_bwd_workspace(B, F, D, pr, kt))) if K is not None else None
    ops.pnn_fwd(E, K, pr, kt, Xb[:, :W])
    ops.pnn_bwd(E, K, pr, kt, dXb[:, :W], d_rows, dK, ws)
    torch.cuda.synchronize()
    return dict(X=Xb, d_rows=d_rows, dK=dK)


def _check(case, what):
    B, F, D, W, ldx = (case[n] for n in ("B", "F", "D", "W", "ldx"))
    first, again = _run(case), _run(case)
    for n, v in first.items():
        if v is None:
            continue
        assert bool(torch.isfinite(v).all()), f"{what}{n} is not finite (an element was not written)"
        assert torch.equal(v, again[n]), f"{what}{n} differs between two runs"
    X, pad = first["X"][:, :W], first["X"][:, W:]
    assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any()), f"{what}pad columns are not +0.0"
    assert torch.equal(X[:, : F * D], case["E"].to(F32).cuda().view(B, F * D)), f"{what}the row copy changed bits"
    err = R.x_error(X, case["X"])
    m_rows = R.grad_measure(first["d_rows"], case["d_rows"])
    m_k = R.grad_measure(first["dK"], case["dK"]) if case["dK"] is not None else 0.0
    f32 = case["f32"]
    print(f"{what}X err {err:.2e} (float32 CPU {f32[0]:.2e}); measures d_rows {m_rows:.2e} ({f32[1]:.2e}) "
          f"dK {m_k:.2e} ({f32[2]:.2e})")
    assert err <= R.TOL_X, f"{what}|X - X64| / max(1, |X64|) = {err:.3g}"
    assert m_rows <= R.TOL_GRAD, f"{what}d_rows measure {m_rows:.3g}"
    assert m_k <= R.TOL_GRAD, f"{what}dK measure {m_k:.3g}"
    if B > 8:
        assert float(X[3].abs().max()) == 0.0, "E = 0 row: X"
        assert torch.equal(first["d_rows"][3].view(-1), case["dX"][3, : F * D].to(F32).cuda()), "E = 0 row: d_rows"
        assert float(first["d_rows"][4].abs().max()) == 0.0, "dX = 0 row"


@pytest.mark.parametrize("ldx_pad", R.LDX_PADS)
@pytest.mark.parametrize("combo", R.COMBOS, ids=lambda c: "p%d_%s" % c)
@pytest.mark.parametrize("shape", R.GPU_CASES, ids=lambda s: "B%d_F%d_D%d" % s)
def test_pnn_kernels_match_float64(hip_lib, shape, combo, ldx_pad):
    _check(R.kernel_case(*shape, *combo, ldx_pad), f"(B, F, D) = {shape} {combo} pad {ldx_pad}: ")


@pytest.mark.parametrize("ldx_pad", R.LDX_PADS)
@pytest.mark.parametrize("combo", R.EXTRA_COMBOS, ids=lambda c: "p%d_%s" % c)
@pytest.mark.parametrize("shape", R.EXTRA_CASES, ids=lambda s: "B%d_F%d_D%d" % s)
def test_pnn_both_products_on_the_vector_alu(hip_lib, shape, combo, ldx_pad):
    """Inner + vec / num: the dE kernel keeps G_in behind G_out in LDS, and reads it from dX at F = 40, D = 32."""
    _check(R.kernel_case(*shape, *combo, ldx_pad), f"(B, F, D) = {shape} {combo} pad {ldx_pad}: ")


@pytest.mark.parametrize("combo", [(R.OUTER, "mat"), (R.OUTER, "vec"), (R.OUTER, "num")], ids=lambda c: c[1])
def test_pnn_grid_stride(hip_lib, combo):
    """F = 3, D = 8 at the smallest B that makes every kernel's block loop run a second time, with a partial last
    tile: one more example than (grid cap) x (tile) of the forward, dE and dK kernels."""
    from recman_amd import ops

    pr, kt = combo
    tile = {k: ops.pnn_tile(3, 8, pr, kt, k) for k in ops.PNN_TILE}
    assert all(16 <= tile[k] <= 64 for k in ("fwd", "de", "dk")) and all(tile[k] >= 1 for k in tile)
    B = max(tile["fwd"] * tile["fwd_cap"], tile["de"] * tile["de_cap"], tile["dk"] * tile["dk_cap"]) + 1
    assert B < 300000
    # the dK workspace holds at most dk_cap sets of partials
    N = {"mat": 3 * 64, "vec": 3 * 8, "num": 3}[kt]
    assert ops.pnn_bwd_workspace(B, 3, 8, pr, kt) == tile["dk_cap"] * N
    assert ops.pnn_bwd_workspace(tile["dk"] * 7 + 1, 3, 8, pr, kt) == 8 * N
    assert ops.pnn_bwd_workspace(B, 3, 8, R.INNER, kt) == 0
    _check(R.kernel_case(B, 3, 8, pr, kt, 3), f"grid stride B={B} {kt}: ")


def test_supported_range_and_tiles(hip_lib):
    from recman_amd import ops

    for F in (0, 1, 2, 3, 26, 40, 41):
        for D in (0, 4, 8, 12, 16, 32, 64):
            for pr in (0, 1, 2, 3, 4):
                for kt in ("mat", "vec", "num", "ten"):
                    want = D in (8, 16, 32) and 2 <= F <= 40 and pr in (1, 2, 3) and kt in R.KERNELS
                    assert ops.pnn_supported(F, D, pr, kt) == want, (F, D, pr, kt)
    assert hip_lib.rm_pnn_supported(26, 16, 3, 3) == 0 and hip_lib.rm_pnn_supported(26, 16, 3, -1) == 0
    assert hip_lib.rm_pnn_supported(26, 16, 0, 0) == 0 and hip_lib.rm_pnn_supported(26, 16, 4, 0) == 0
    assert hip_lib.rm_pnn_tile(26, 16, 3, 0, 6) == -1 and hip_lib.rm_pnn_tile(41, 16, 3, 0, 0) == -1
    for F, D in ((2, 8), (26, 16), (40, 32)):
        for pr, kt in R.COMBOS:
            for k in ("fwd", "de"):
                assert ops.pnn_tile(F, D, pr, kt, k) in (16, 32, 48, 64)
            assert ops.pnn_tile(F, D, pr, kt, "dk") in ((16, 32, 48, 64) if pr & R.OUTER else (0,))
    # the largest kernel set gets fewer batch slices: 32 MB of partials at most
    assert ops.pnn_tile(40, 32, 2, "mat", "dk_cap") == (8 << 20) // (780 * 1024) == 10
    assert ops.pnn_tile(26, 16, 3, "mat", "dk_cap") == 64 and ops.pnn_tile(26, 16, 1, "mat", "dk_cap") == 0


def test_unsupported_shapes_and_bad_arguments_raise_and_launch_nothing(hip_lib):
    from recman_amd import ops

    for F, D in ((1, 8), (41, 8), (3, 12), (3, 64)):
        for pr, kt in R.COMBOS:
            K = _nan(*R.weight_shape(max(F, 2), D, kt))
            W = F * D + 2 * F * F
            with pytest.raises(ValueError, match="unsupported"):
                ops.pnn_fwd(_nan(4, F, D), K, pr, kt, _nan(4, W))
            with pytest.raises(ValueError, match="unsupported"):
                ops.pnn_bwd(_nan(4, F, D), K, pr, kt, _nan(4, W), _nan(4, F, D), K.clone(), _nan(8))
            with pytest.raises(ValueError, match="unsupported"):
                ops.pnn_bwd_workspace(4, F, D, pr, kt)
            assert hip_lib.rm_pnn_bwd_workspace(4, F, D, pr, ops.PNN_KERNELS[kt]) == -1
    with pytest.raises(ValueError, match="unsupported"):
        ops.pnn_fwd(_nan(4, 3, 8), _nan(3, 8, 8), 3, "ten", _nan(4, 30))
    with pytest.raises(ValueError, match="unsupported"):
        ops.pnn_fwd(_nan(4, 3, 8), _nan(3, 8, 8), 0, "mat", _nan(4, 30))
    assert hip_lib.rm_pnn_bwd_workspace(-1, 3, 8, 3, 0) == -1 and hip_lib.rm_pnn_bwd_workspace(0, 3, 8, 3, 0) == 0
    # the C entry points themselves: an unsupported shape, a NULL pointer, a stride below W = 24 + 2 * 3
    E, K, X, dX, d_rows, dK, wsp = (_nan(4, 3, 8), _nan(3, 8, 8), _nan(4, 32), _nan(4, 32), _nan(4, 3, 8),
                                    _nan(3, 8, 8), _nan(1024))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = [P(E), P(K), 3, 0, 4, 3, 8, P(X), 32, st]
    for pos, val, msg in ((5, 1, "F=1"), (5, 41, "F=41"), (6, 12, "D=12"), (6, 64, "D=64"), (3, 3, "kernel_type=3"),
                          (2, 0, "products=0"), (2, 4, "products=4"), (4, -1, "batch"), (0, None, "E is NULL"),
                          (1, None, "K is NULL"), (7, None, "X is NULL"), (8, 29, "ldx=29")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_pnn_fwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    ok = [P(E), P(K), 3, 0, P(dX), 32, 4, 3, 8, P(d_rows), P(dK), P(wsp), st]
    for pos, val, msg in ((7, 1, "F=1"), (8, 12, "D=12"), (3, -1, "kernel_type=-1"), (2, 0, "products=0"),
                          (6, -1, "batch"), (0, None, "E is NULL"), (1, None, "K is NULL"), (4, None, "dX is NULL"),
                          (9, None, "d_rows is NULL"), (10, None, "dK is NULL"), (11, None, "workspace is NULL"),
                          (5, 29, "lddx=29")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_pnn_bwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    torch.cuda.synchronize()
    for t in (X, d_rows, dK, wsp):
        assert bool(torch.isnan(t).all()), "a refused call launched something"
    # without OUTER the kernel, its gradient and the workspace may be NULL; the stride is then checked against 24 + 3
    assert hip_lib.rm_pnn_fwd(P(E), None, 1, 0, 4, 3, 8, P(X), 26, st) != 0
    assert "ldx=26" in hip_lib.rm_last_error().decode()
    Ez = torch.zeros(4, 3, 8, dtype=F32, device="cuda")
    assert hip_lib.rm_pnn_fwd(P(Ez), None, 1, 0, 4, 3, 8, P(X), 32, st) == 0
    dXz = torch.zeros(4, 32, dtype=F32, device="cuda")
    assert hip_lib.rm_pnn_bwd(P(Ez), None, 1, 0, P(dXz), 32, 4, 3, 8, P(d_rows), None, None, st) == 0
    torch.cuda.synchronize()
    assert bool((X == 0).all()) and bool((d_rows == 0).all())
    # ops' own argument checks
    E, K, X = (torch.zeros(s, dtype=F32, device="cuda") for s in ((4, 3, 8), (3, 8, 8), (4, 30)))
    with pytest.raises(ValueError, match=r"expected \[B,F,D\]"):
        ops.pnn_fwd(E[0], K, 3, "mat", X)
    with pytest.raises(ValueError, match="expected shape"):
        ops.pnn_fwd(E, K, 3, "vec", X)  # "vec" needs [P, D]
    with pytest.raises(ValueError, match="expected shape"):
        ops.pnn_fwd(E, K[:2], 3, "mat", X)
    with pytest.raises(ValueError, match="must be"):
        ops.pnn_fwd(E, K, 3, "mat", X[:, :29])
    with pytest.raises(ValueError, match="must be"):
        ops.pnn_fwd(E, K, 3, "mat", X[:3])
    with pytest.raises(ValueError, match="must not be None"):
        ops.pnn_fwd(E, None, 3, "mat", X)
    with pytest.raises(ValueError, match="contiguous"):
        ops.pnn_fwd(torch.zeros(4, 3, 16, dtype=F32, device="cuda")[:, :, ::2], K, 3, "mat", X)
    with pytest.raises(TypeError):
        ops.pnn_fwd(E.double(), K, 3, "mat", X)
    with pytest.raises(ValueError, match="GPU"):
        ops.pnn_fwd(E, K.cpu(), 3, "mat", X)
    with pytest.raises(ValueError, match="workspace too small"):
        ops.pnn_bwd(E, K, 3, "mat", X, E.clone(), K.clone(), torch.zeros(3, dtype=F32, device="cuda"))
    with pytest.raises(ValueError, match="expected shape"):
        ops.pnn_bwd(E, K, 3, "mat", X, E[:3].clone(), K.clone(), torch.zeros(1024, dtype=F32, device="cuda"))
    with pytest.raises(ValueError, match="expected shape"):
        ops.pnn_bwd(E, K, 3, "mat", X, E.clone(), K[:2].clone(), torch.zeros(1024, dtype=F32, device="cuda"))
    assert ops.pnn_width(3, 8, 3) == (30, 32) and ops.pnn_width(3, 8, 1) == (27, 28)
    assert ops.pnn_products(True, False) == 1 and ops.pnn_products(True, True) == 3 and ops.pnn_products(False, False) == 0


@pytest.mark.parametrize("combo", R.COMBOS, ids=lambda c: "p%d_%s" % c)
def test_empty_batch_touches_nothing(hip_lib, combo):
    from recman_amd import ops

    pr, kt = combo
    K = torch.randn(R.weight_shape(3, 8, kt), device="cuda") if pr & R.OUTER else None
    E = torch.zeros(0, 3, 8, dtype=F32, device="cuda")
    X = torch.zeros(0, R.width(3, 8, pr), dtype=F32, device="cuda")
    ops.pnn_fwd(E, K, pr, kt, X)
    assert ops.pnn_bwd_workspace(0, 3, 8, pr, kt) == 0
    dK, wsp = (_nan(*K.shape), _nan(16)) if K is not None else (None, None)
    ops.pnn_bwd(E, K, pr, kt, X, E.clone(), dK, wsp)
    torch.cuda.synchronize()
    if K is not None:
        assert bool(torch.isnan(dK).all()) and bool(torch.isnan(wsp).all())
