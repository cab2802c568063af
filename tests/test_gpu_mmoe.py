"""GPU: the MMoE mixture kernels (rm_mmoe_mix_fwd / rm_mmoe_mix_bwd) and the loss head for several labels
(rm_multitask_loss) against the float64 restatement (tests/mmoe_ref.py, pinned without a GPU in
tests/test_mmoe_host.py).  Tolerance, the convention of tests/test_gpu_asp.py: for every output the project's gradient
measure against float64 must be <= max(2e-5, 4 x the float32 CPU restatement's own measure on the case); both numbers
are printed."""
import pytest
import torch

from tests import mmoe_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")


def _check(what, got, want, f32):
    m = R.grad_measure(got, want)
    print(f"{what}: measure {m:.2e}, float32 CPU {f32:.2e}, bound {R.bound(f32):.2e}")
    assert m <= R.bound(f32), f"{what}: {m:.3e} > {R.bound(f32):.3e}"


def _out(B, W, pad):
    """[B, W] as a column range (from column 4 on) of a wider NaN-filled buffer whose row stride is a multiple of 4
    floats and no multiple of 32; pad = 0: rows of W floats rounded up to whole float4s.  -> (view, buffer, first column)."""
    if not pad:
        buf = torch.full((B, (W + 3) // 4 * 4), NAN, dtype=F32, device="cuda")
        return buf[:, :W], buf, 0
    ld = (4 + W + pad + 3) // 4 * 4
    ld += 4 if ld % 32 == 0 else 0
    buf = torch.full((B, ld), NAN, dtype=F32, device="cuda")
    return buf[:, 4: 4 + W], buf, 4


def _view(t, pad):
    """A device copy of t [B, W] laid out by _out."""
    view, buf, lead = _out(t.shape[0], t.shape[1], pad)
    view.copy_(t.to(F32))
    return view, buf, lead


def _canaries_intact(buf, lead, W):
    return bool(torch.isnan(buf[:, :lead]).all()) and bool(torch.isnan(buf[:, lead + W:]).all())


def _run(c, pad=0, want_p=False):
    """Forward and backward of a mix case; every operand a column range at stride width + 4 + pad when pad is set."""
    from recman_amd import ops

    B, E, T, H = c["B"], c["E"], c["T"], c["H"]
    Z, zb, zl = _view(c["Z"], pad)
    A, ab, al = _view(c["A"], pad)
    dM, db, dl = _view(c["dM"], pad)
    M, mb, ml = _out(B, T * H, pad)
    P, pb, pl = _out(B, T * E, pad) if want_p else (None, None, 0)
    dZ, dzb, dzl = _out(B, E * H, pad)
    dA, dab, dal = _out(B, T * E, pad)
    ops.mmoe_mix_fwd(Z, A, E, T, M, P=P)
    ops.mmoe_mix_bwd(Z, A, E, T, dM, dZ, dA)
    torch.cuda.synchronize()
    bufs = dict(M=(mb, ml, T * H), dZ=(dzb, dzl, E * H), dA=(dab, dal, T * E))
    if want_p:
        bufs["P"] = (pb, pl, T * E)
    return dict(M=M, P=P, dZ=dZ, dA=dA), bufs


@pytest.mark.parametrize("shape", R.MIX_CASES)
def test_mixture_matches_float64(hip_lib, shape):
    B, E, T, H = shape
    c = R.mix_case(*shape)
    out, _ = _run(c)
    for n in ("M", "dZ", "dA"):
        _check(f"{shape} {n}", out[n], c[n], c["f32"][n])
    assert bool(torch.isfinite(out["M"]).all())
    if E == 1:  # p = 1: M is Z's bits, dZ is dM's, dA exactly 0
        assert torch.equal(out["M"].cpu(), c["Z"].float()) and torch.equal(out["dZ"].cpu(), c["dM"].float())
        assert float(out["dA"].abs().max()) == 0.0


@pytest.mark.parametrize("shape,pad", [((77, 8, 2, 128), 8), ((33, 16, 8, 36), 12), ((70, 3, 2, 512), 20),
                                       ((5, 3, 2, 8), 4)])
def test_column_ranges_of_wider_buffers(hip_lib, shape, pad):
    """Every operand is a column range of a NaN-filled buffer; the strides are multiples of 4 and not of 32."""
    B, E, T, H = shape
    c = R.mix_case(*shape)
    out, bufs = _run(c, pad=pad, want_p=True)
    for n, (buf, lead, W) in bufs.items():
        assert buf.stride(0) % 4 == 0 and buf.stride(0) % 32 != 0, (n, buf.stride(0))
        assert _canaries_intact(buf, lead, W), f"{n}: a column outside its range was written"
    for n in ("M", "dZ", "dA"):
        _check(f"{shape} strided {n}", out[n], c[n], c["f32"][n])
    # the same bits as from contiguous operands
    plain, _ = _run(c)
    for n in ("M", "dZ", "dA"):
        assert torch.equal(out[n], plain[n]), n
    assert float((out["P"].cpu().double().reshape(B, T, E) - c["P"]).abs().max()) <= 1e-6


def test_gate_logit_range(hip_lib):
    from recman_amd import ops

    # logits x 60: the softmax is one-hot and only the subtracted maximum keeps it finite
    c = R.mix_case(33, 4, 2, 8, logit_scale=60.0)
    out, _ = _run(c, want_p=True)
    assert bool(torch.isfinite(out["M"]).all()) and bool(torch.isfinite(out["dA"]).all())
    f32 = c["f32"]
    for n in ("M", "dZ", "dA"):
        _check(f"x60 {n}", out[n], c[n], f32[n])
    # equal logits: p = 1 / E exactly for E a power of two
    for E in (1, 2, 8, 16):
        T, H, B = 3, 16, 19
        Z = torch.randn(B, E * H, device="cuda")
        A, P = _out(B, T * E, 0)[0], _out(B, T * E, 0)[0]  # (rows of whole float4s: T E = 3 at E = 1)
        A.fill_(-3.25)
        M = torch.empty(B, T * H, device="cuda")
        ops.mmoe_mix_fwd(Z, A, E, T, M, P=P)
        assert bool((P == 1.0 / E).all()), E
        want = Z.double().reshape(B, E, H).mean(dim=1)
        assert float((M.double().reshape(B, T, H) - want.unsqueeze(1)).abs().max()) <= 1e-6


def test_grid_stride_walk(hip_lib):
    """B from the kernel's own tile and grid cap: every block walks three whole tiles, the first blocks a fourth, and
    the last tile is partial."""
    from recman_amd import ops

    E, T, H = 2, 2, 8
    tile, cap = ops.mmoe_mix_tile(E, T, H), ops.mmoe_mix_tile(E, T, H, "cap")
    assert (tile, cap) == (128, 1024) and ops.mmoe_mix_tile(E, T, H, backward=True) == tile
    B = 3 * tile * cap + 5 * tile + 77
    assert B // (tile * cap) == 3 and B % tile not in (0, tile)
    g = torch.Generator(device="cuda").manual_seed(5)
    Z = torch.randn(B, E * H, device="cuda", generator=g)
    A = torch.randn(B, T * E, device="cuda", generator=g)
    dM = torch.randn(B, T * H, device="cuda", generator=g)
    M, dZ, dA = torch.empty(B, T * H, device="cuda"), torch.empty(B, E * H, device="cuda"), torch.empty(
        B, T * E, device="cuda")
    ops.mmoe_mix_fwd(Z, A, E, T, M)
    ops.mmoe_mix_bwd(Z, A, E, T, dM, dZ, dA)
    torch.cuda.synchronize()
    # float64 on the device (the restatement's own functions): the whole batch, first to last example
    M64, _ = R.mix_fwd(Z.double(), A.double(), E, T)
    dZ64, dA64 = R.mix_bwd(Z.double(), A.double(), E, T, dM.double())
    M32, _ = R.mix_fwd(Z, A, E, T)
    dZ32, dA32 = R.mix_bwd(Z, A, E, T, dM)
    for n, got, want, twin in (("M", M, M64, M32), ("dZ", dZ, dZ64, dZ32), ("dA", dA, dA64, dA32)):
        _check(f"grid-stride {n}", got, want, R.grad_measure(twin, want))
        last = slice(B - 77, B)
        assert R.grad_measure(got[last], want[last]) <= R.bound(R.grad_measure(twin[last], want[last])), n


@pytest.mark.parametrize("shape", [(77, 8, 2, 128), (33, 16, 8, 36), (70, 3, 2, 512)])
def test_two_runs_are_bit_equal_and_p_changes_nothing(hip_lib, shape):
    B, E, T, H = shape
    c = R.mix_case(*shape)
    a, _ = _run(c)
    b, _ = _run(c, want_p=True)
    for n in ("M", "dZ", "dA"):
        assert torch.equal(a[n], b[n]), f"{n} differs between two runs"
    again, _ = _run(c, want_p=True)
    assert torch.equal(b["P"], again["P"])
    rows = b["P"].double().reshape(B, T, E).sum(dim=2)
    assert float((rows - 1).abs().max()) <= 1e-6


def test_refusals_name_the_limits(hip_lib):
    from recman_amd import ops
    from recman_amd._lib import RecmanHipError

    def call(E, T, H, B=4, ldz=None):
        Z = torch.zeros(B, ldz or E * H, device="cuda")[:, : E * H]
        A = torch.zeros(B, (T * E + 3) // 4 * 4, device="cuda")[:, : T * E]
        ops.mmoe_mix_fwd(Z, A, E, T, torch.zeros(B, T * H, device="cuda"))

    for E, T, H in ((17, 1, 8), (2, 9, 8), (2, 2, 516), (2, 2, 6)):
        with pytest.raises(RecmanHipError, match=r"1 <= E <= 16.*1 <= T <= 8.*multiple of 4 in 4\.\.512"):
            call(E, T, H)
    with pytest.raises(RecmanHipError, match=r"row stride.*multiple of 4 floats.*1 <= E <= 16"):
        call(2, 2, 8, ldz=18)  # a stride that is no multiple of 4
    Z = torch.zeros(4, 16, device="cuda")
    A = torch.zeros(4, 4, device="cuda")
    with pytest.raises(RecmanHipError, match="multiple of 4 floats"):
        ops.mmoe_mix_bwd(Z, A, 2, 2, Z.clone(), torch.zeros(4, 18, device="cuda")[:, :16], A.clone())
    with pytest.raises(ValueError, match=r"\[B, T E\]"):
        ops.mmoe_mix_fwd(Z, torch.zeros(4, 6, device="cuda"), 2, 2, Z.clone())
    call(2, 2, 8, B=0)  # an empty batch is fine


# ----------------------------------------------------------------------------------------------- the loss head
def _loss_run(c):
    from recman_amd import ops

    T, B = c["T"], c["B"]
    dev = "cuda"
    logit, Y = c["logit"].to(F32).to(dev), c["Y"].to(F32).to(dev)
    out = dict(pred=torch.empty(T, B, device=dev), dlogit=torch.full((T, B), NAN, device=dev),
               n_t=torch.full((T,), -1, dtype=torch.int64, device=dev), loss_t=torch.full((T,), NAN, device=dev),
               loss=torch.full((1,), NAN, device=dev))
    ws = torch.empty(ops.multitask_loss_workspace(B, T), device=dev)
    ops.multitask_loss(logit, c["types"], out["pred"], Y=Y, task_weights=c["weights"], grad_scale=c["grad_scale"],
                       dlogit=out["dlogit"], n_t=out["n_t"], loss_t=out["loss_t"], loss=out["loss"], workspace=ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", R.LOSS_B)
@pytest.mark.parametrize("T", R.LOSS_T)
def test_loss_head_matches_float64(hip_lib, T, B):
    c = R.loss_case(T, B)
    out = _loss_run(c)
    what = f"T={T} B={B}"
    assert torch.equal(out["n_t"].cpu(), c["n_t"])
    for n in ("pred", "dlogit", "loss_t"):
        _check(f"{what} {n}", out[n], c[n], c["f32"][n])
    _check(f"{what} loss", out["loss"], c["loss"].reshape(1), c["f32"]["loss_t"])
    seen = ~torch.isnan(c["Y"]).t()
    assert float(out["dlogit"].cpu()[~seen].abs().sum()) == 0.0  # +0.0 wherever the label is unobserved
    assert bool(torch.isfinite(out["pred"]).all())  # written for unobserved labels too
    if T > 2:  # the task without a label: loss 0, a zero gradient
        assert float(out["loss_t"][T - 1]) == 0.0 and float(out["dlogit"][T - 1].abs().max()) == 0.0
    again = _loss_run(c)
    for n in out:
        assert torch.equal(out[n], again[n]), f"{n} differs between two runs"


def test_loss_head_inference_without_labels_through_both_entry_points(hip_lib):
    """Y = None and no training output: pred alone, the same bits from rm_multitask_loss and from
    rm_multitask_loss_es without a pair."""
    from recman_amd import ops

    T, B = 3, 257
    c = R.loss_case(T, B)
    logit = c["logit"].to(F32).cuda()
    pred, pred_es = torch.full((T, B), NAN, device="cuda"), torch.full((T, B), NAN, device="cuda")
    ops.multitask_loss(logit, c["types"], pred)
    ops.multitask_loss_es(logit, c["types"], pred_es, es=(-1, -1))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pred).all()) and torch.equal(pred, pred_es)
    _check(f"inference T={T} B={B} pred", pred, c["pred"], c["f32"]["pred"])


@pytest.mark.parametrize("B", [1, 77, 4099])
@pytest.mark.parametrize("kind", ["classification", "regression"])
def test_one_task_without_missing_labels_is_logit_loss(hip_lib, kind, B):
    from recman_amd import ops

    g = torch.Generator().manual_seed(B)
    logit = (torch.randn(1, B, generator=g) * 3).cuda()
    y = ((torch.rand(B, generator=g) < 0.3).float() if kind == "classification" else torch.randn(B, generator=g)).cuda()
    pred, dlogit = torch.empty(1, B, device="cuda"), torch.empty(1, B, device="cuda")
    loss = torch.empty(1, device="cuda")
    ws = torch.empty(ops.multitask_loss_workspace(B, 1), device="cuda")
    ops.multitask_loss(logit, [kind], pred, Y=y.reshape(B, 1).contiguous(), dlogit=dlogit, loss=loss, workspace=ws)
    pred1, dlogit1, loss1 = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
    ops.logit_loss([(logit[0], 1.0)], y_f=y, task=kind, pred=pred1, dlogit=dlogit1, loss=loss1,
                   workspace=torch.empty(1024, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(pred[0], pred1)
    assert float((dlogit[0] - dlogit1).abs().max()) <= 1e-6 * float(dlogit1.abs().max())
    assert abs(float(loss) - float(loss1)) <= 1e-5 * max(1.0, abs(float(loss1)))
    # inference: pred alone, the same bits
    pred_i = torch.empty(1, B, device="cuda")
    ops.multitask_loss(logit, [kind], pred_i)
    assert torch.equal(pred_i, pred)
