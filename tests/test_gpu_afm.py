"""GPU: rm_afm_fwd / rm_afm_bwd through the C ABI (recman_amd.ops) against the float64 restatement + autograd
(tests/afm_ref.py, pinned on the CPU by tests/test_afm_host.py).

Tolerances: forward logit 1e-5 absolute (the model-level bound of tests/test_gpu_parity.py); d_rows with that file's
gradient measure at 2e-5.  The batch-summed dW, db, dh, dp use the same measure with the bound
max(2e-5, 4 x the float32 CPU restatement's own error on the case): dh is a sum over B * P terms that cancel, and the
float32 CPU restatement itself sits near 2e-5 on the larger cases - a fixed bound would test summation order; 4 x
because the kernel's reduction tree differs from the CPU's.  Both numbers are printed.

Kink guard: g is zero for every example with a hidden unit within 1e-6 of its ReLU kink in float64 (same g for kernel
and reference; the cap of 20 % per case is asserted on the CPU) - those examples' d_rows must be exactly dE_up or 0."""
import pytest
import torch

from tests import afm_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _dev(t):
    return t.to(F32).cuda().contiguous()


def _run(case, use_mask, use_up, stats=True, alias=False):
    """The kernels on a case's layer-level tensors: (logit, d_rows, dW, db, dh, dp)."""
    from recman_amd import ops

    E, W, b, h, p, g = (_dev(case[k]) for k in ("E", "W", "b", "h", "p_vec", "g"))
    B, F, D = E.shape
    T = W.shape[1]
    mask = _dev(case["mask"]) if use_mask else None
    logit = torch.empty(B, device="cuda")
    st = torch.empty(B, ops.afm_stats_width(D), device="cuda") if stats else None
    ops.afm_fwd(E, W, b, h, p, logit, mask=mask, stats=st)
    if not stats:
        return (logit,)
    d_rows = torch.full((B, F, D), float("nan"), device="cuda")
    up = _dev(case["dE_up"]) if use_up else None
    if alias and use_up:
        d_rows.copy_(up)
        up = d_rows
    dW, db, dh, dp = (torch.full(s, float("nan"), device="cuda") for s in ((D, T), (T,), (T,), (D,)))
    ws = torch.empty(ops.afm_bwd_workspace(B, F, D, T), device="cuda")
    ops.afm_bwd(E, W, b, h, p, g, logit, st, d_rows, dW, db, dh, dp, ws, mask=mask, dE_up=up)
    torch.cuda.synchronize()
    return logit, d_rows, dW, db, dh, dp


def _check(case, c, use_mask, use_up):
    want = R.layer_reference(case, use_mask, use_up)
    cpu32 = R.layer_reference(case, use_mask, use_up, dtype=F32)
    got = [t.cpu().double() for t in _run(case, use_mask, use_up)]
    tag = f"{c} mask={use_mask} dE_up={use_up}"
    err = float((got[0] - want[0]).abs().max())
    print(f"{tag}: logit err {err:.2e}")
    assert err <= 1e-5, f"{tag}: logit err {err:.3e}"
    m = R.grad_measure(got[1], want[1])
    print(f"{tag}: d_rows measure {m:.2e} (float32 CPU {R.grad_measure(cpu32[1], want[1]):.2e})")
    assert m <= 2e-5, f"{tag}: d_rows measure {m:.3e}"
    # examples the kink guard zeroed: exactly dE_up, or exactly 0
    near = case["near"]
    if bool(near.any()):
        rest = case["dE_up"].float().double()[near] if use_up else torch.zeros_like(got[1][near])
        assert torch.equal(got[1][near], rest), f"{tag}: a zeroed example's d_rows is not dE_up / 0"
    for name, a, w, c32 in zip(("dW", "db", "dh", "dp"), got[2:], want[2:], cpu32[2:]):
        m, m32 = R.grad_measure(a, w), R.grad_measure(c32, w)
        bound = max(2e-5, 4 * m32)
        print(f"{tag}: {name} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        assert m <= bound, f"{tag}: {name} measure {m:.3e} > {bound:.3e} (float32 CPU {m32:.3e})"
    return got


@pytest.mark.parametrize("c", R.GPU_CASES, ids=lambda c: "x".join(map(str, c)))
def test_afm_kernels_match_float64(hip_lib, c):
    case = R.gpu_case(c)
    for use_mask in (False, True):
        for use_up in (False, True):
            got = _check(case, c, use_mask, use_up)
            if c[1] == 2:  # one pair: a = 1 whatever W, b, h are
                for t in got[2:5]:
                    assert float(t.abs().max()) == 0.0, "dW, db, dh must be exactly zero with a single pair"


@pytest.mark.parametrize("c", [(64, 26, 16, 8), (33, 2, 8, 4), (9, 39, 64, 64), (3, 6, 8, 8)],
                         ids=lambda c: "x".join(map(str, c)))
def test_inference_logits_are_the_training_logits_bit_for_bit(hip_lib, c):
    case = R.gpu_case(c)
    for use_mask in (False, True):
        assert torch.equal(_run(case, use_mask, False, stats=False)[0], _run(case, use_mask, False)[0])


def test_upstream_gradient_may_alias_the_output(hip_lib):
    case = R.gpu_case((130, 26, 16, 32))
    a, b = _run(case, True, True), _run(case, True, True, alias=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("c", R.RANGE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_softmax_range_scores_in_the_hundreds(hip_lib, c):
    case = R.gpu_case(c, h_scale=R.RANGE_H_SCALE)
    P, z = R.afm_hidden(case["E"], case["W"], case["b"])
    s = torch.relu(z) @ case["h"]
    assert float(s.max()) > 89.0 and float(s.min()) < -89.0  # exp(s) itself is not finite in fp32
    for use_mask in (False, True):
        want = R.layer_reference(case, use_mask, False)[0]
        got = _run(case, use_mask, False)
        assert bool(torch.isfinite(got[0]).all()) and all(bool(torch.isfinite(t).all()) for t in got[1:])
        err = float((got[0].cpu().double() - want).abs().max())
        print(f"{c} h x {R.RANGE_H_SCALE}: scores {float(s.min()):.0f} .. {float(s.max()):.0f}, logit err {err:.2e}")
        assert err <= 1e-5


@pytest.mark.parametrize("c", [(4100, 26, 16, 8), (300, 40, 32, 16), (130, 26, 16, 32), (37, 5, 8, 8)],
                         ids=lambda c: "x".join(map(str, c)))
def test_two_runs_are_bit_equal(hip_lib, c):
    case = R.gpu_case(c)
    a, b = _run(case, True, True), _run(case, True, True)
    for x, y, name in zip(a, b, ("logit", "d_rows", "dW", "db", "dh", "dp")):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("F,D,T", [(26, 12, 8), (1, 16, 8), (41, 16, 8), (26, 16, 65), (26, 16, 0)])
def test_unsupported_shapes_are_rejected(hip_lib, F, D, T):
    from recman_amd import _lib, ops

    assert not ops.afm_supported(F, D, T)
    B = 4
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        ops.afm_fwd(z(B, F, D), z(D, T), z(T), z(T), z(D), z(B))
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        ops.afm_bwd(z(B, F, D), z(D, T), z(T), z(T), z(D), z(B), z(B), z(B, D + 2), z(B, F, D), z(D, T), z(T), z(T),
                    z(D), z(16))
    assert ops.afm_supported(26, 16, 8) and ops.afm_supported(2, 8, 1) and ops.afm_supported(40, 64, 64)
