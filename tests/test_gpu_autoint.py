"""GPU: rm_autoint_layer_fwd / _bwd and rm_autoint_head_fwd / _bwd through the C ABI (recman_amd.ops) against the
float64 restatement + autograd (tests/autoint_ref.py, pinned on the CPU by tests/test_autoint_host.py).

Tolerances (the project's own, tests/test_gpu_afm.py): Y 1e-5 absolute; dX with the gradient measure at 2e-5; the
batch-summed dWq, dWk, dWv, dWr and the head's dw, dw0 with the same measure and the bound max(2e-5, 4 x the float32
CPU restatement's own error on the case) - 4 x because the kernel's reduction tree differs from the CPU's.  Both numbers
are printed.

Kink guard: dY is zero for every example with a pre-activation within 1e-6 of 0 in float64 (same dY for kernel and
reference; the cap of 20 % per case is asserted on the CPU) - those examples' dX must be exactly dX_up or 0."""
import pytest
import torch

from tests import autoint_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAMES = ("Y", "dX", "dWq", "dWk", "dWv", "dWr")
_ids = lambda c: "x".join(map(str, c))  # noqa: E731


def _dev(t):
    return t.to(F32).cuda().contiguous()


def _run(case, use_res, use_up, scaling, stats=True, alias=False):
    """The kernels on a case's tensors: (Y, dX, dWq, dWk, dWv[, dWr])."""
    from recman_amd import ops

    X, Wq, Wk, Wv, dY = (_dev(case[k]) for k in ("X", "Wq", "Wk", "Wv", "dY"))
    Wr = _dev(case["Wr"]) if use_res else None
    B, F, Din = X.shape
    H, dk, HD = case["H"], case["dk"], Wq.shape[1]
    scale = R.att_scale(dk, scaling)
    Y = torch.full((B, F, HD), float("nan"), device="cuda")
    st = torch.empty(B, H, F, 2, device="cuda") if stats else None
    assert st is None or st.numel() == ops.autoint_stats_floats(B, F, H)
    ops.autoint_layer_fwd(X, Wq, Wk, Wv, Wr, H, scale, Y, stats=st)
    if not stats:
        return (Y,)
    dX = torch.full((B, F, Din), float("nan"), device="cuda")
    up = _dev(case["dX_up"]) if use_up else None
    if alias and use_up:
        dX.copy_(up)
        up = dX
    dW = [torch.full((Din, HD), float("nan"), device="cuda") for _ in range(4 if use_res else 3)]
    ws = torch.empty(ops.autoint_layer_bwd_workspace(B, F, Din, H, dk), device="cuda")
    ops.autoint_layer_bwd(X, Wq, Wk, Wv, Wr, Y, st, dY, H, scale, dX, *dW, *(() if use_res else (None,)), ws,
                          dX_up=up)
    torch.cuda.synchronize()
    return (Y, dX, *dW)


def _check(case, c, use_res, use_up, scaling):
    want = R.layer_reference(case, use_res, use_up, scaling)
    cpu32 = R.layer_reference(case, use_res, use_up, scaling, dtype=F32)
    got = [t.cpu().double() for t in _run(case, use_res, use_up, scaling)]
    tag = f"{c} res={use_res} dX_up={use_up} scaling={scaling}"
    err = float((got[0] - want[0]).abs().max())
    print(f"{tag}: Y err {err:.2e}")
    assert err <= 1e-5, f"{tag}: Y err {err:.3e}"
    m = R.grad_measure(got[1], want[1])
    print(f"{tag}: dX measure {m:.2e} (float32 CPU {R.grad_measure(cpu32[1], want[1]):.2e})")
    assert m <= 2e-5, f"{tag}: dX measure {m:.3e}"
    # examples the kink guard zeroed: exactly dX_up, or exactly 0
    near = case["near"]
    if bool(near.any()):
        rest = case["dX_up"].float().double()[near] if use_up else torch.zeros_like(got[1][near])
        assert torch.equal(got[1][near], rest), f"{tag}: a zeroed example's dX is not dX_up / 0"
    for name, a, w, c32 in zip(NAMES[2:], got[2:], want[2:], cpu32[2:]):
        m, m32 = R.grad_measure(a, w), R.grad_measure(c32, w)
        bound = max(2e-5, 4 * m32)
        print(f"{tag}: {name} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        assert m <= bound, f"{tag}: {name} measure {m:.3e} > {bound:.3e} (float32 CPU {m32:.3e})"
    return got


@pytest.mark.parametrize("c", R.GPU_CASES, ids=_ids)
def test_autoint_layer_kernels_match_float64(hip_lib, c):
    case = R.gpu_case(c)
    for use_res in (True, False):
        for use_up in (False, True):
            for scaling in (False, True):
                got = _check(case, c, use_res, use_up, scaling)
                if c[1] == 1:  # a single field: the weight is 1 whatever Q and K are
                    assert float(got[2].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0, (
                        "dWq and dWk must be exactly zero with a single field")


@pytest.mark.parametrize("c", [(64, 26, 16, 2, 8), (33, 2, 8, 1, 8), (9, 39, 64, 4, 16), (3, 6, 8, 2, 4),
                               (150, 1, 16, 2, 8)], ids=_ids)
def test_inference_output_is_the_training_output_bit_for_bit(hip_lib, c):
    case = R.gpu_case(c)
    for use_res in (False, True):
        assert torch.equal(_run(case, use_res, False, False, stats=False)[0], _run(case, use_res, False, False)[0])


def test_upstream_gradient_may_alias_the_output(hip_lib):
    case = R.gpu_case((130, 26, 16, 2, 16))
    a, b = _run(case, True, True, False), _run(case, True, True, False, alias=True)
    for x, y, name in zip(a, b, NAMES):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("c", R.RANGE_CASES, ids=_ids)
def test_softmax_range_scores_in_the_hundreds(hip_lib, c):
    case = R.gpu_case(c, q_scale=R.RANGE_Q_SCALE)
    s = R.interacting_parts(case["X"], case["Wq"], case["Wk"], case["Wv"], case["Wr"], case["H"])[3]
    assert float(s.max()) > 89.0 and float(s.min()) < -89.0  # exp(s) itself is not finite in fp32
    for use_res in (False, True):
        want = R.layer_reference(case, use_res, False, False)[0]
        e32 = float((R.layer_reference(case, use_res, False, False, dtype=F32)[0] - want).abs().max())
        got = _run(case, use_res, False, False)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        err = float((got[0].cpu().double() - want).abs().max())
        bound = max(1e-5, 4 * e32)
        print(f"{c} Wq x {R.RANGE_Q_SCALE}: scores {float(s.min()):.0f} .. {float(s.max()):.0f}, Y err {err:.2e}, "
              f"float32 CPU {e32:.2e}, bound {bound:.2e}")
        assert err <= bound


@pytest.mark.parametrize("c", [(4100, 26, 16, 2, 8), (300, 40, 32, 1, 16), (130, 26, 16, 2, 16), (37, 5, 8, 2, 4)],
                         ids=_ids)
def test_two_runs_are_bit_equal(hip_lib, c):
    case = R.gpu_case(c)
    a, b = _run(case, True, True, False), _run(case, True, True, False)
    for x, y, name in zip(a, b, NAMES):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("F,Din,H,dk", [(0, 16, 2, 8), (41, 16, 2, 8), (26, 12, 2, 8), (26, 16, 3, 8), (26, 16, 2, 64),
                                        (26, 16, 2, 2), (26, 16, 3, 4)])
def test_unsupported_shapes_are_rejected(hip_lib, F, Din, H, dk):
    """F = 0 or 41; Din = 12; HD = 24 or 128; dk = 2; H = 3."""
    from recman_amd import _lib, ops

    assert not ops.autoint_supported(F, Din, H, dk)
    B, HD = 4, H * dk
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        ops.autoint_layer_fwd(z(B, F, Din), z(Din, HD), z(Din, HD), z(Din, HD), z(Din, HD), H, 1.0, z(B, F, HD))
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        ops.autoint_layer_bwd(z(B, F, Din), z(Din, HD), z(Din, HD), z(Din, HD), z(Din, HD), z(B, F, HD),
                              z(B, H, F, 2), z(B, F, HD), H, 1.0, z(B, F, Din), z(Din, HD), z(Din, HD), z(Din, HD),
                              z(Din, HD), z(16))
    assert ops.autoint_supported(26, 16, 2, 8) and ops.autoint_supported(1, 8, 1, 8)
    assert ops.autoint_supported(40, 64, 8, 8)


def _run_head(case, Y):
    from recman_amd import ops

    Yd, w, w0, g = (_dev(t) for t in (Y, case["w"], case["w0"], case["g"]))
    B, K = Yd.shape[0], w.numel()
    logit = torch.full((B,), float("nan"), device="cuda")
    ops.autoint_head_fwd(Yd, w, w0, logit)
    dY, dw, dw0 = torch.full_like(Yd, float("nan")), torch.full((K,), float("nan"), device="cuda"), torch.full(
        (1,), float("nan"), device="cuda")
    ws = torch.empty(ops.autoint_head_bwd_workspace(B, K), device="cuda")
    ops.autoint_head_bwd(Yd, w, g, dY, dw, dw0, ws)
    torch.cuda.synchronize()
    return logit, dY, dw, dw0


@pytest.mark.parametrize("c", R.GPU_CASES, ids=_ids)
def test_head_kernels_match_float64_and_two_runs_are_bit_equal(hip_lib, c):
    case = R.gpu_case(c)
    Y = R.layer_reference(case, True, False, False)[0].float().double()  # K = F HD, every value a float32 number
    want, cpu32 = R.head_reference(case, Y), R.head_reference(case, Y, dtype=F32)
    a, b = _run_head(case, Y), _run_head(case, Y)
    for x, y, name in zip(a, b, ("logit", "dY", "dw", "dw0")):
        assert torch.equal(x, y), name
    got = [t.cpu().double() for t in a]
    err = float((got[0] - want[0]).abs().max())
    print(f"{c}: K = {c[1] * c[3] * c[4]}, logit err {err:.2e}")
    assert err <= 1e-5
    m = R.grad_measure(got[1], want[1])
    assert m <= 2e-5, f"dY measure {m:.3e}"
    for name, x, w, c32 in zip(("dw", "dw0"), got[2:], want[2:], cpu32[2:]):
        m, m32 = R.grad_measure(x, w), R.grad_measure(c32, w)
        bound = max(2e-5, 4 * m32)
        print(f"{c}: {name} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        assert m <= bound, f"{name} measure {m:.3e} > {bound:.3e}"
