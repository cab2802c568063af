"""GPU: the DCN-Mix core kernels (csrc/cross_mix.hip) through recman_amd.ops against the float64 restatement
(tests/crossmix_ref.py), with the project's own tolerances (tests/test_gpu_autoint.py): M 1e-5 absolute, dT and dS the
gradient measure at 2e-5, the batch-summed dC the measure against max(2e-5, 4 x the float32 CPU restatement's own error
on the case).  Every case runs at three layouts - separate contiguous arrays, T | S (and dT | dS) as column ranges of
one buffer of row stride exactly E r + E, and that stride rounded up to 4 plus 4 - and twice: all bits must agree."""
import ctypes

import pytest
import torch

from tests import crossmix_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")


def _grid_stride_B():
    """The smallest B at which BOTH kernels' block loops run a second time at E = 3, r = 8: a tile holds
    min(4096 // 24, 64) // 4 * 4 = 64 examples, the forward's grid is capped at 2048 blocks and the backward's at 512,
    so B = 2048 * 64 + 1 = 131073."""
    from recman_amd import ops

    return max(ops.CROSS_MIX_FWD_BLOCKS, ops.CROSS_MIX_BWD_BLOCKS) * ops.cross_mix_tile(3, 8) + 1


def _layout(B, E, r, which):
    """-> (row stride, make): make(width, col0) gives a [B, width] view at columns col0.. of a NaN-filled buffer (a
    fresh contiguous array when which == 0) and the buffer."""
    W = E * r
    ld = {0: None, 1: W + E, 2: (W + E + 3) // 4 * 4 + 4}[which]

    def make(width, col0):
        if ld is None:
            buf = torch.full((B, width), NAN, dtype=F32, device="cuda")
            return buf, buf
        buf = torch.full((B, ld), NAN, dtype=F32, device="cuda")
        return buf[:, col0: col0 + width], buf
    return ld, make


def _run(case, which):
    """One forward + backward at a layout: -> dict of output tensors (contiguous copies)."""
    from recman_amd import ops

    B, E, r = case["B"], case["E"], case["r"]
    W = E * r
    ld, make = _layout(B, E, r, which)
    # inputs: T | S in one buffer (layouts 1, 2), dM in a buffer of its own
    if ld is None:
        T, S = case["t"].to(F32).cuda(), case["s"].to(F32).cuda()
        dM = case["dm"].to(F32).cuda()
    else:
        ts = torch.full((B, ld), NAN, dtype=F32, device="cuda")
        ts[:, :W], ts[:, W: W + E] = case["t"].to(F32).cuda(), case["s"].to(F32).cuda()
        T, S = ts[:, :W], ts[:, W: W + E]
        dmb = torch.full((B, ld), NAN, dtype=F32, device="cuda")
        dmb[:, :W] = case["dm"].to(F32).cuda()
        dM = dmb[:, :W]
    C = case["C"].to(F32).cuda()
    M, Mbuf = make(W, 0)
    ops.cross_mix_fwd(T, S, C, M)
    if ld is None:
        dT, dTbuf = make(W, 0)
        dS, dSbuf = make(E, 0)
    else:
        dT, dTbuf = make(W, 0)
        dS, dSbuf = dTbuf[:, W: W + E], dTbuf
    dC = torch.full((E, r, r), NAN, dtype=F32, device="cuda")
    ws = torch.full((max(1, ops.cross_mix_bwd_workspace(B, E, r)),), NAN, dtype=F32, device="cuda")
    ops.cross_mix_bwd(T, S, C, dM, dT, dS, dC, ws)
    torch.cuda.synchronize()
    if ld is not None:
        # the pad columns of the shared buffers are untouched
        assert bool(torch.isnan(Mbuf[:, W:]).all()), "M's buffer: columns past E r were written"
        assert bool(torch.isnan(dTbuf[:, W + E:]).all()), "dT | dS buffer: pad columns were written"
        assert bool(torch.isnan(ts[:, W + E:]).all()) and bool(torch.isnan(dmb[:, W:]).all())
    return dict(m=M.contiguous(), dt=dT.contiguous(), ds=dS.contiguous(), dC=dC)


def _check(case, what):
    B, E = case["B"], case["E"]
    first = _run(case, 0)
    for n, v in first.items():
        assert bool(torch.isfinite(v).all()), f"{what}{n} is not finite"
    for which in (0, 1, 2):
        again = _run(case, which)
        for n in first:
            assert torch.equal(first[n], again[n]), f"{what}{n}: layout {which} differs in its bits"
    err_m = float((first["m"].cpu().double() - case["m"]).abs().max())
    ms = {n: R.grad_measure(first[n], case[n]) for n in ("dt", "ds", "dC")}
    f32 = R.f32_errors(case)
    bound_dc = max(R.TOL_GRAD, 4 * f32[3])
    print(f"{what}M err {err_m:.2e} (float32 CPU {f32[0]:.2e}); measures dT {ms['dt']:.2e} ({f32[1]:.2e}) "
          f"dS {ms['ds']:.2e} ({f32[2]:.2e}) dC {ms['dC']:.2e} ({f32[3]:.2e}, bound {bound_dc:.2e})")
    assert err_m <= R.TOL_M, f"{what}|M - M64| = {err_m:.3g}"
    assert ms["dt"] <= R.TOL_GRAD, f"{what}dT measure {ms['dt']:.3g}"
    assert ms["ds"] <= R.TOL_GRAD, f"{what}dS measure {ms['ds']:.3g}"
    assert ms["dC"] <= bound_dc, f"{what}dC measure {ms['dC']:.3g} > {bound_dc:.3g}"
    if B > 8:
        assert float(first["m"][4].abs().max()) == 0.0, "t = 0 must give m = 0 exactly"
        assert float(first["dt"][7].abs().max()) == 0.0 and float(first["ds"][7].abs().max()) == 0.0, "dm = 0 row"
        p6 = R.core_fwd(case["t"][6:7], case["s"][6:7], case["C"])  # p = 1/E on the s = 0 row
        assert float((first["m"][6:7].cpu().double() - p6).abs().max()) <= R.TOL_M
    if E == 1:
        assert float(first["ds"].abs().max()) == 0.0 and not bool(torch.signbit(first["ds"]).any()), "E = 1: ds = +0.0"


@pytest.mark.parametrize("shape", R.GPU_CASES, ids=lambda s: "B%d_E%d_r%d" % s)
def test_cross_mix_kernels_match_float64(hip_lib, shape):
    _check(R.kernel_case(*shape), "(B, E, r) = %s: " % (shape,))


def test_cross_mix_grid_stride(hip_lib):
    """E = 3, r = 8 at the smallest B that makes both kernels' block loops run a second time (_grid_stride_B: 131073)."""
    from recman_amd import ops

    B = _grid_stride_B()
    G = ops.cross_mix_tile(3, 8)
    assert B == 131073 and B < 300000
    # the backward's grid is capped: its workspace holds fewer partial dC than the batch has tiles
    assert ops.cross_mix_bwd_workspace(B, 3, 8) == ops.CROSS_MIX_BWD_BLOCKS * 3 * 64
    assert ops.cross_mix_bwd_workspace(B - 1, 3, 8) == ops.CROSS_MIX_BWD_BLOCKS * 3 * 64
    assert ops.cross_mix_bwd_workspace(G * 7 + 1, 3, 8) == 8 * 3 * 64
    _check(R.kernel_case(B, 3, 8), "grid stride: ")


def test_supported_range(hip_lib):
    from recman_amd import ops

    for E in range(0, 11):
        for r in (0, 4, 8, 12, 16, 32, 48, 64, 128):
            want = 1 <= E <= 8 and r in (8, 16, 32, 64) and E * r <= 256
            assert ops.cross_mix_supported(E, r) == want, (E, r)
    assert ops.cross_mix_supported(8, 32) and not ops.cross_mix_supported(5, 64)


def test_unsupported_shapes_and_bad_arguments_raise_and_launch_nothing(hip_lib):
    from recman_amd import ops

    z = lambda *s: torch.full(s, NAN, dtype=F32, device="cuda")  # noqa: E731
    for E, r in ((9, 8), (2, 12), (5, 64), (1, 128)):
        with pytest.raises(ValueError, match="unsupported"):
            ops.cross_mix_fwd(z(4, E * r), z(4, E), z(E, r, r), z(4, E * r))
        with pytest.raises(ValueError, match="unsupported"):
            ops.cross_mix_bwd(z(4, E * r), z(4, E), z(E, r, r), z(4, E * r), z(4, E * r), z(4, E), z(E, r, r), z(8))
        with pytest.raises(ValueError, match="unsupported"):
            ops.cross_mix_bwd_workspace(4, E, r)
        assert hip_lib.rm_cross_mix_bwd_workspace(4, E, r) == -1
    # the C entry points themselves: an unsupported shape, a NULL pointer, a stride below the width
    T, S, C, M = z(4, 16), z(4, 2), z(2, 8, 8), z(4, 16)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = [((P(T), 16, P(S), 2, P(C), 9, 8, 4, P(M), 72, st), "E=9"),
           ((P(T), 24, P(S), 2, P(C), 2, 12, 4, P(M), 24, st), "r=12"),
           ((P(T), 16, P(S), 2, P(C), 2, 8, -1, P(M), 16, st), "batch"),
           ((None, 16, P(S), 2, P(C), 2, 8, 4, P(M), 16, st), "T is NULL"),
           ((P(T), 16, None, 2, P(C), 2, 8, 4, P(M), 16, st), "S is NULL"),
           ((P(T), 16, P(S), 2, None, 2, 8, 4, P(M), 16, st), "C is NULL"),
           ((P(T), 16, P(S), 2, P(C), 2, 8, 4, None, 16, st), "M is NULL"),
           ((P(T), 15, P(S), 2, P(C), 2, 8, 4, P(M), 16, st), "ldt"),
           ((P(T), 16, P(S), 1, P(C), 2, 8, 4, P(M), 16, st), "lds"),
           ((P(T), 16, P(S), 2, P(C), 2, 8, 4, P(M), 8, st), "ldm")]
    for args, msg in bad:
        assert hip_lib.rm_cross_mix_fwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    dT, dS, dC, ws = z(4, 16), z(4, 2), z(2, 8, 8), z(256)
    ok = [P(T), 16, P(S), 2, P(C), 2, 8, 4, P(M), 16, P(dT), 16, P(dS), 2, P(dC), P(ws), st]
    for pos, val, msg in ((5, 9, "E=9"), (6, 12, "r=12"), (0, None, "T is NULL"), (8, None, "dM is NULL"),
                          (10, None, "dT is NULL"), (12, None, "dS is NULL"), (14, None, "dC is NULL"),
                          (15, None, "workspace is NULL"), (9, 15, "lddm"), (11, 15, "lddt"), (13, 1, "ldds")):
        args = list(ok)
        args[pos] = val
        assert hip_lib.rm_cross_mix_bwd(*args) != 0, msg
        assert msg in hip_lib.rm_last_error().decode(), (msg, hip_lib.rm_last_error())
    torch.cuda.synchronize()
    for t in (M, dT, dS, dC, ws):
        assert bool(torch.isnan(t).all()), "a refused call launched something"
    # ops' own argument checks
    T, S, C, M = (torch.zeros(s, dtype=F32, device="cuda") for s in ((4, 16), (4, 2), (2, 8, 8), (4, 16)))
    with pytest.raises(ValueError, match=r"expected \[E,r,r\]"):
        ops.cross_mix_fwd(T, S, C[0], M)
    with pytest.raises(ValueError, match="must be"):
        ops.cross_mix_fwd(T, S[:, :1], C, M)
    with pytest.raises(ValueError, match="must be"):
        ops.cross_mix_fwd(T[:3], S, C, M)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.cross_mix_fwd(torch.zeros(4, 32, dtype=F32, device="cuda")[:, ::2], S, C, M)
    with pytest.raises(ValueError, match="float32"):
        ops.cross_mix_fwd(T.double(), S, C, M)
    with pytest.raises(ValueError, match="device"):
        ops.cross_mix_fwd(T.cpu(), S, C, M)
    with pytest.raises(TypeError):
        ops.cross_mix_fwd(T, S, C.double(), M)
    with pytest.raises(ValueError, match="workspace too small"):
        ops.cross_mix_bwd(T, S, C, M, T.clone(), S.clone(), C.clone(), torch.zeros(3, dtype=F32, device="cuda"))


def test_empty_batch(hip_lib):
    from recman_amd import ops

    e = lambda w: torch.zeros(0, w, dtype=F32, device="cuda")  # noqa: E731
    C = torch.randn(2, 8, 8, device="cuda")
    ops.cross_mix_fwd(e(16), e(2), C, e(16))
    assert ops.cross_mix_bwd_workspace(0, 2, 8) == 0
    dC = torch.full((2, 8, 8), NAN, dtype=F32, device="cuda")
    ops.cross_mix_bwd(e(16), e(2), C, e(16), e(16), e(2), dC, torch.zeros(1, dtype=F32, device="cuda"))
    torch.cuda.synchronize()
    assert float(dC.abs().max()) == 0.0  # the sum over an empty batch
