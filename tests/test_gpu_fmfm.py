"""GPU: the field-pair weighted FM kernels (csrc/fmfm.hip) through recman_amd.ops against the float64 restatement
(tests/fmfm_ref.py).  Tolerances, the project's own (tests/test_gpu_parity.py): |logit - logit64| <= 1e-5 max(1,
|logit64|), d_rows and dW the gradient measure at 2e-5.  Every output buffer is pre-filled with NaN; every case runs
twice (all bits must agree) and a third time with dE_up, which must be added exactly."""
import ctypes

import pytest
import torch

from tests import fmfm_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")


def _nan(*shape):
    return torch.full(shape, NAN, dtype=F32, device="cuda")


def _run(case, with_up=False):
    from recman_amd import ops

    B, F, D, ftype = (case[n] for n in ("B", "F", "D", "ftype"))
    E, W, g = (case[n].to(F32).cuda() for n in ("E", "W", "g"))
    logit, d_rows, dW = _nan(B), _nan(B, F, D), _nan(*W.shape)
    ws = _nan(max(1, ops.fmfm_bwd_workspace(B, F, D, ftype)))
    ops.fmfm_fwd(E, W, ftype, logit)
    ops.fmfm_bwd(E, W, ftype, g, d_rows, dW, ws, dE_up=case["dE_up"].to(F32).cuda() if with_up else None)
    torch.cuda.synchronize()
    return dict(logit=logit, d_rows=d_rows, dW=dW)


def _check(case, what):
    B = case["B"]
    first, again, up = _run(case), _run(case), _run(case, with_up=True)
    for n, v in first.items():
        assert bool(torch.isfinite(v).all()), f"{what}{n} is not finite (an element was not written)"
        assert torch.equal(v, again[n]), f"{what}{n} differs between two runs"
    err = R.logit_error(first["logit"], case["logit"])
    m_rows, m_w = R.grad_measure(first["d_rows"], case["dE"]), R.grad_measure(first["dW"], case["dW"])
    f32 = R.f32_errors(case)
    print(f"{what}logit err {err:.2e} (float32 CPU {f32[0]:.2e}); measures d_rows {m_rows:.2e} ({f32[1]:.2e}) "
          f"dW {m_w:.2e} ({f32[2]:.2e})")
    assert err <= R.TOL_LOGIT, f"{what}|logit - logit64| / max(1, |logit64|) = {err:.3g}"
    assert m_rows <= R.TOL_GRAD, f"{what}d_rows measure {m_rows:.3g}"
    assert m_w <= R.TOL_GRAD, f"{what}dW measure {m_w:.3g}"
    if B > 8:
        assert float(first["logit"][3]) == 0.0 and float(first["d_rows"][3].abs().max()) == 0.0, "E = 0 row"
        assert float(first["d_rows"][4].abs().max()) == 0.0, "g = 0 row"
    # dE_up is added exactly: to one ulp of the sum
    want = first["d_rows"] + case["dE_up"].to(F32).cuda()
    ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
    assert bool(((up["d_rows"] - want).abs() <= ulp).all()), f"{what}dE_up is not added exactly"
    assert torch.equal(up["logit"], first["logit"]) and torch.equal(up["dW"], first["dW"])


@pytest.mark.parametrize("ftype", R.TYPES)
@pytest.mark.parametrize("shape", R.GPU_CASES, ids=lambda s: "B%d_F%d_D%d" % s)
def test_fmfm_kernels_match_float64(hip_lib, shape, ftype):
    _check(R.kernel_case(*shape, ftype), f"(B, F, D) = {shape} {ftype}: ")


@pytest.mark.parametrize("ftype", R.TYPES)
def test_fmfm_grid_stride(hip_lib, ftype):
    """F = 3, D = 8 at the smallest B that makes every kernel's block loop run a second time, with a partial last
    tile: one more example than (grid cap) x (tile) of the forward, dE and dW kernels."""
    from recman_amd import ops

    tile = {k: ops.fmfm_tile(3, 8, ftype, k) for k in ops.FMFM_TILE}
    assert all(16 <= tile[k] <= 64 for k in ("fwd", "de", "dw")) and all(tile[k] >= 1 for k in tile)
    B = max(tile["fwd"] * tile["fwd_cap"], tile["de"] * tile["de_cap"], tile["dw"] * tile["dw_cap"]) + 1
    assert B < 300000
    # the dW workspace holds at most dw_cap sets of partials
    N = {"matrix": 3 * 64, "vector": 3 * 8, "scalar": 3}[ftype]
    assert ops.fmfm_bwd_workspace(B, 3, 8, ftype) == tile["dw_cap"] * N
    assert ops.fmfm_bwd_workspace(tile["dw"] * 7 + 1, 3, 8, ftype) == 8 * N
    _check(R.kernel_case(B, 3, 8, ftype), f"grid stride B={B} {ftype}: ")


def test_supported_range_and_tiles(hip_lib):
    from recman_amd import ops

    for F in (0, 1, 2, 3, 26, 40, 41):
        for D in (0, 4, 8, 12, 16, 32, 64):
            for ftype in ("matrix", "vector", "scalar", "tensor"):
                want = D in (8, 16, 32) and 2 <= F <= 40 and ftype in R.TYPES
                assert ops.fmfm_supported(F, D, ftype) == want, (F, D, ftype)
    assert hip_lib.rm_fmfm_supported(26, 16, 3) == 0 and hip_lib.rm_fmfm_supported(26, 16, -1) == 0
    assert hip_lib.rm_fmfm_tile(26, 16, 0, 6) == -1 and hip_lib.rm_fmfm_tile(41, 16, 0, 0) == -1
    assert ops.fmfm_weight_shape(26, 16, "matrix") == (325, 16, 16)
    assert ops.fmfm_weight_shape(26, 16, "vector") == (325, 16) and ops.fmfm_weight_shape(26, 16, "scalar") == (325,)
    for F, D in ((2, 8), (26, 16), (40, 32)):
        for ftype in R.TYPES:
            for k in ("fwd", "de", "dw"):
                assert ops.fmfm_tile(F, D, ftype, k) in (16, 32, 48, 64)
    # the largest weight set gets fewer batch slices: 32 MB of partials at most
    assert ops.fmfm_tile(40, 32, "matrix", "dw_cap") == (8 << 20) // (780 * 1024) == 10
    assert ops.fmfm_tile(26, 16, "matrix", "dw_cap") == 64


def test_unsupported_shapes_and_bad_arguments_raise_and_launch_nothing(hip_lib):
    from recman_amd import ops

    for F, D in ((1, 8), (41, 8), (3, 12), (3, 64)):
        for ftype in R.TYPES:
            W = _nan(*R.weight_shape(max(F, 2), D, ftype))
            with pytest.raises(ValueError, match="unsupported"):
                ops.fmfm_fwd(_nan(4, F, D), W, ftype, _nan(4))
            with pytest.raises(ValueError, match="unsupported"):
                ops.fmfm_bwd(_nan(4, F, D), W, ftype, _nan(4), _nan(4, F, D), W.clone(), _nan(8))
            with pytest.raises(ValueError, match="unsupported"):
                ops.fmfm_bwd_workspace(4, F, D, ftype)
            assert hip_lib.rm_fmfm_bwd_workspace(4, F, D, ops.FMFM_TYPES[ftype]) == -1
    with pytest.raises(ValueError, match="unsupported"):
        ops.fmfm_fwd(_nan(4, 3, 8), _nan(3, 8, 8), "tensor", _nan(4))
    assert hip_lib.rm_fmfm_bwd_workspace(-1, 3, 8, 0) == -1 and hip_lib.rm_fmfm_bwd_workspace(0, 3, 8, 0) == 0
    # the C entry points themselves: an unsupported shape, a NULL pointer
    E, W, g, logit, d_rows, dW, wsp = _nan(4, 3, 8), _nan(3, 8, 8), _nan(4), _nan(4), _nan(4, 3, 8), _nan(3, 8, 8), _nan(1024)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = [P(E), P(W), 0, 4, 3, 8, P(logit), st]
    for pos, val, msg in ((4, 1, "F=1"), (4, 41, "F=41"), (5, 12, "D=12"), (5, 64, "D=64"), (2, 3, "type=3"),
                          (3, -1, "batch"), (0, None, "E is NULL"), (1, None, "W is NULL"), (6, None, "logit is NULL")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_fmfm_fwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    ok = [P(E), P(W), 0, P(g), None, 4, 3, 8, P(d_rows), P(dW), P(wsp), st]
    for pos, val, msg in ((6, 1, "F=1"), (7, 12, "D=12"), (2, -1, "type=-1"), (5, -1, "batch"), (0, None, "E is NULL"),
                          (1, None, "W is NULL"), (3, None, "g is NULL"), (8, None, "d_rows is NULL"),
                          (9, None, "dW is NULL"), (10, None, "workspace is NULL")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_fmfm_bwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    torch.cuda.synchronize()
    for t in (logit, d_rows, dW, wsp):
        assert bool(torch.isnan(t).all()), "a refused call launched something"
    # ops' own argument checks
    E, W, v = (torch.zeros(s, dtype=F32, device="cuda") for s in ((4, 3, 8), (3, 8, 8), (4,)))
    with pytest.raises(ValueError, match=r"expected \[B,F,D\]"):
        ops.fmfm_fwd(E[0], W, "matrix", v)
    with pytest.raises(ValueError, match="expected shape"):
        ops.fmfm_fwd(E, W, "vector", v)  # "vector" needs [P, D]
    with pytest.raises(ValueError, match="expected shape"):
        ops.fmfm_fwd(E, W[:2], "matrix", v)
    with pytest.raises(ValueError, match="expected shape"):
        ops.fmfm_fwd(E, W, "matrix", v[:3])
    with pytest.raises(ValueError, match="contiguous"):
        ops.fmfm_fwd(torch.zeros(4, 3, 16, dtype=F32, device="cuda")[:, :, ::2], W, "matrix", v)
    with pytest.raises(TypeError):
        ops.fmfm_fwd(E.double(), W, "matrix", v)
    with pytest.raises(ValueError, match="GPU"):
        ops.fmfm_fwd(E, W.cpu(), "matrix", v)
    with pytest.raises(ValueError, match="workspace too small"):
        ops.fmfm_bwd(E, W, "matrix", v, E.clone(), W.clone(), torch.zeros(3, dtype=F32, device="cuda"))
    with pytest.raises(ValueError, match="expected shape"):
        ops.fmfm_bwd(E, W, "matrix", v, E[:3].clone(), W.clone(), torch.zeros(1024, dtype=F32, device="cuda"))
    with pytest.raises(ValueError, match="expected shape"):
        ops.fmfm_bwd(E, W, "matrix", v, E.clone(), W.clone(), torch.zeros(1024, dtype=F32, device="cuda"),
                     dE_up=E[:3].clone())


@pytest.mark.parametrize("ftype", R.TYPES)
def test_empty_batch_touches_nothing(hip_lib, ftype):
    from recman_amd import ops

    W = torch.randn(R.weight_shape(3, 8, ftype), device="cuda")
    E, v = torch.zeros(0, 3, 8, dtype=F32, device="cuda"), torch.zeros(0, dtype=F32, device="cuda")
    ops.fmfm_fwd(E, W, ftype, v)
    assert ops.fmfm_bwd_workspace(0, 3, 8, ftype) == 0
    dW, wsp = _nan(*W.shape), _nan(16)
    ops.fmfm_bwd(E, W, ftype, v, E.clone(), dW, wsp)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dW).all()) and bool(torch.isnan(wsp).all())
