"""GPU: the in-batch softmax and row-norm kernels (csrc/inbatch.hip) through ops against the float64 restatement
(tests/twotower_ref.py).  Tolerance, the project's convention: grad_measure(got, float64) <= max(2e-5, 4 x the float32
CPU restatement's own measure) for lse, row_loss, loss, dU and dV; ranks by the near-tie rule of R.check_ranks."""
import pytest
import torch

from tests import twotower_ref as R
from tests.test_twotower_host import VARIANTS

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")
NAMES = ("lse", "row_loss", "loss", "dU", "dV")


def _check(what, got, want, f32):
    m = R.grad_measure(got, want)
    print(f"{what}: measure {m:.2e}, float32 CPU {f32:.2e}, bound {R.bound(f32):.2e}")
    assert m <= R.bound(f32), f"{what}: {m:.3e} > {R.bound(f32):.3e}"


def _out(B, W, pad):
    """[B, W] as a column range (from column 4 on) of a wider NaN-filled buffer whose row stride is a multiple of 4
    floats and no multiple of 32; pad = 0: contiguous.  -> (view, buffer, first column)."""
    if not pad:
        buf = torch.full((B, W), NAN, dtype=F32, device="cuda")
        return buf, buf, 0
    ld = (4 + W + pad + 3) // 4 * 4
    ld += 4 if ld % 32 == 0 else 0
    buf = torch.full((B, ld), NAN, dtype=F32, device="cuda")
    return buf[:, 4: 4 + W], buf, 4


def _view(t, pad):
    view, buf, lead = _out(t.shape[0], t.shape[1], pad)
    view.copy_(t.to(F32))
    return view, buf, lead


def _canaries_intact(buf, lead, W):
    return bool(torch.isnan(buf[:, :lead]).all()) and bool(torch.isnan(buf[:, lead + W:]).all())


def _dev(t, dtype=F32):
    return None if t is None else t.to(dtype).cuda().contiguous()


def _run(k, splits=0, pad=0):
    """Forward + backward of case k through ops -> (outputs, {name: (buffer, first column, width)})."""
    from recman_amd import ops

    B, H = k["B"], k["H"]
    bufs = {}
    U, bufs["U"], lu = _view(k["U"], pad)
    V, bufs["V"], lv = _view(k["V"], pad)
    dU, bufs["dU"], ldu = _out(B, H, pad + 4 if pad else 0)
    dV, bufs["dV"], ldv = _out(B, H, pad)
    bufs = {n: (b, l, H) for (n, b), l in zip(bufs.items(), (lu, lv, ldu, ldv))}
    lse, row_loss = torch.full((B,), NAN, device="cuda"), torch.full((B,), NAN, device="cuda")
    rank = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    loss = torch.full((1,), NAN, device="cuda")
    ws = torch.full((ops.inbatch_softmax_workspace(B, H),), NAN, device="cuda")
    kw = dict(item_id=_dev(k["item"], torch.int64), logq=_dev(k["logq"]), w=_dev(k["w"]), col_splits=splits)
    ops.inbatch_softmax_fwd(U, V, k["scale"], lse, row_loss, loss, ws, rank=rank, **kw)
    ops.inbatch_softmax_bwd(U, V, k["scale"], lse, dU, dV, ws, grad_scale=k["grad_scale"], **kw)
    torch.cuda.synchronize()
    return dict(lse=lse, row_loss=row_loss, loss=loss, rank=rank, dU=dU, dV=dV), bufs


def _check_all(what, out, k):
    for n in NAMES:
        _check(f"{what} {n}", out[n], k[n].reshape(out[n].shape), k["f32"][n])
    assert all(bool(torch.isfinite(out[n]).all()) for n in NAMES), what


@pytest.mark.parametrize("B,H", R.CASES)
@pytest.mark.parametrize("ids,logq,w", VARIANTS)
def test_matches_float64(hip_lib, B, H, ids, logq, w):
    k = R.ibs_case(B, H, ids, logq, w)
    out, _ = _run(k)
    what = f"B={B} H={H} ids={ids} logq={logq} w={w}"
    _check_all(what, out, k)
    R.check_ranks(out["rank"], k, what=what + ": ")
    if w:  # a row with w_i = 0 has dU_i = 0 exactly while its item still is a negative
        dead = (k["w"] == 0)
        assert float(out["dU"].cpu()[dead].abs().sum()) == 0.0
        if B > 1 and bool(dead.any()) and not bool(dead.all()):
            assert float(out["dV"].cpu()[dead].abs().sum()) > 0.0


def _tile(H):
    from recman_amd import ops

    return tuple(ops.inbatch_softmax_tile(H, w) for w in ("rows", "cols", "max_splits"))


def test_tile_edges(hip_lib):
    rows, cols, _ = _tile(16)
    for B in (3 * rows + 5, 2 * cols + 1):
        k = R.ibs_case(B, 16)
        out, _ = _run(k)
        _check_all(f"B={B} H=16", out, k)
        R.check_ranks(out["rank"], k, what=f"B={B}: ")


def test_col_splits(hip_lib):
    """1, 2 and the maximum: each within the tolerance, the same value twice bit-equal; at B = 130 the maximum is above
    the number of column tiles."""
    rows, cols, smax = _tile(16)
    from recman_amd import ops

    for B, H in ((130, 36), (5 * cols + 7, 16)):
        k = R.ibs_case(B, H)
        assert smax > (130 + ops.inbatch_softmax_tile(36, "cols") - 1) // ops.inbatch_softmax_tile(36, "cols")
        for s in (1, 2, smax):
            a, _ = _run(k, splits=s)
            b, _ = _run(k, splits=s)
            what = f"B={B} H={H} splits={s}"
            _check_all(what, a, k)
            R.check_ranks(a["rank"], k, what=what + ": ")
            for n in NAMES + ("rank",):
                assert torch.equal(a[n], b[n]), f"{what}: {n} differs between two runs"


@pytest.mark.parametrize("scale,normalised", [(200.0, True), (12.0, False)])
def test_large_scores_stay_finite(hip_lib, scale, normalised):
    k = R.ibs_case(65, 64, scale=scale, normalised=normalised)
    top = float(k["S"].abs().max())
    print(f"scale {scale}: |S| reaches {top:.0f}")
    assert top > 80  # expf of such a score overflows float32: only the subtracted maximum keeps the sums finite
    for s in (0, 2):
        out, _ = _run(k, splits=s)
        _check_all(f"scale={scale} splits={s}", out, k)


def test_exact_facts(hip_lib):
    out, _ = _run(R.ibs_case(1, 4))
    assert float(out["loss"]) == 0.0 and float(out["row_loss"]) == 0.0 and int(out["rank"]) == 0
    assert float(out["dU"].abs().max()) == 0.0 and float(out["dV"].abs().max()) == 0.0
    for s in (0, 2):
        k = R.ibs_case(70, 20, same_ids=True)
        out, _ = _run(k, splits=s)
        # only the diagonal is allowed: lse_i has the bits of S_ii (= lse_i - l_i with l_i = 0)
        assert float(out["row_loss"].abs().max()) == 0.0 and float(out["loss"]) == 0.0
        _check("same ids lse", out["lse"], k["lse"], k["f32"]["lse"])
        assert int(out["rank"].abs().max()) == 0
        assert float(out["dU"].abs().max()) == 0.0 and float(out["dV"].abs().max()) == 0.0
        out, _ = _run(R.ibs_case(70, 20, zero_w=True), splits=s)
        assert float(out["loss"]) == 0.0
        assert float(out["dU"].abs().max()) == 0.0 and float(out["dV"].abs().max()) == 0.0


@pytest.mark.parametrize("B,H,pad", [(65, 64, 4), (130, 36, 12), (17, 20, 8)])
def test_column_ranges_of_wider_buffers(hip_lib, B, H, pad):
    k = R.ibs_case(B, H)
    for s in (0, 2):
        out, bufs = _run(k, splits=s, pad=pad)
        for n, (buf, lead, W) in bufs.items():
            assert buf.stride(0) % 4 == 0 and buf.stride(0) % 32 != 0, (n, buf.stride(0))
            assert _canaries_intact(buf, lead, W), f"{n}: a column outside its range was written"
        _check_all(f"B={B} H={H} strided", out, k)
        flat, _ = _run(k, splits=s)
        for n in NAMES + ("rank",):
            assert torch.equal(out[n], flat[n]), f"{n}: strided and contiguous operands differ"


# --------------------------------------------------------------------------------------------------------- rownorm
@pytest.mark.parametrize("B,H", R.ROWNORM_CASES)
def test_rownorm_matches_float64(hip_lib, B, H):
    from recman_amd import ops

    k = R.rownorm_case(B, H)
    X, _, _ = _view(k["X"], 8)
    Y, ybuf, lead = _out(B, H, 4)
    inv = torch.full((B,), NAN, device="cuda")
    ops.rownorm_fwd(X, Y, inv, R.EPS)
    _check(f"rownorm B={B} H={H} Y", Y, k["Y"], k["f32"]["Y"])
    _check(f"rownorm B={B} H={H} inv", inv, k["inv"], k["f32"]["Y"])
    assert _canaries_intact(ybuf, lead, H)
    dY, dbuf, dlead = _view(k["dY"], 4)
    dX = torch.full((B, H), NAN, device="cuda")
    ops.rownorm_bwd(Y, inv, dY, dX)
    _check(f"rownorm B={B} H={H} dX", dX, k["dX"], k["f32"]["dX"])
    ops.rownorm_bwd(Y, inv, dY, dY)  # in place
    assert torch.equal(dY, dX) and _canaries_intact(dbuf, dlead, H)


def test_rownorm_zero_row(hip_lib):
    from recman_amd import ops

    X = torch.zeros(3, 8, device="cuda")
    X[1] = 1.0
    Y, inv, dY = torch.empty_like(X), torch.empty(3, device="cuda"), torch.full((3, 8), 0.5, device="cuda")
    ops.rownorm_fwd(X, Y, inv, 1e-6)
    assert float(Y[0].abs().max()) == 0.0 and float(Y[2].abs().max()) == 0.0
    dX = torch.empty_like(X)
    ops.rownorm_bwd(Y, inv, dY, dX)
    want = dY[0].double() / 1e-6
    assert float(((dX[0].double() - want).abs() / want).max()) <= 1e-6


# ------------------------------------------------------------------------------------------------- argument errors
def _raw(fn, **over):
    """A raw call of rm_inbatch_softmax_fwd / _bwd with valid arguments for B = 8, H = 8, then `over` -> (rc, message)."""
    from recman_amd import _lib

    lib = _lib.lib()
    B, H = 8, 8
    t = {n: torch.zeros(B, H, device="cuda") for n in ("U", "V", "dU", "dV")}
    v = {n: torch.zeros(B, device="cuda") for n in ("lse", "row_loss", "loss")}
    ws = torch.zeros(int(lib.rm_inbatch_softmax_workspace(B, H)), device="cuda")
    a = dict(U=t["U"].data_ptr(), ldu=H, V=t["V"].data_ptr(), ldv=H, B=B, H=H, splits=0, lse=v["lse"].data_ptr(),
             dU=t["dU"].data_ptr(), lddu=H, dV=t["dV"].data_ptr(), lddv=H, ws=ws.data_ptr())
    a.update(over)
    if fn == "fwd":
        rc = lib.rm_inbatch_softmax_fwd(a["U"], a["ldu"], a["V"], a["ldv"], None, None, None, 1.0, a["B"], a["H"],
                                        a["splits"], a["lse"], v["row_loss"].data_ptr(), None, v["loss"].data_ptr(),
                                        a["ws"], None)
    else:
        rc = lib.rm_inbatch_softmax_bwd(a["U"], a["ldu"], a["V"], a["ldv"], None, None, None, 1.0, 1.0, a["B"], a["H"],
                                        a["splits"], a["lse"], a["dU"], a["lddu"], a["dV"], a["lddv"], a["ws"], None)
    torch.cuda.synchronize()
    return rc, lib.rm_last_error().decode()


def test_argument_errors(hip_lib):
    from recman_amd import ops

    assert _raw("fwd")[0] == 0 and _raw("bwd")[0] == 0
    assert _raw("fwd", B=0, U=None, V=None)[0] == 0 and _raw("bwd", B=0, U=None, dU=None)[0] == 0  # B = 0 is RM_OK
    smax = ops.inbatch_softmax_tile(8, "max_splits")
    base = torch.zeros(8, 8, device="cuda").data_ptr()
    for fn in ("fwd", "bwd"):
        for over, word in ((dict(H=6), "H=6"), (dict(H=260), "H=260"), (dict(H=0), "H=0"),
                           (dict(U=None), "U is NULL"), (dict(V=None), "V is NULL"), (dict(ws=None), "workspace"),
                           (dict(U=base + 4), "16-byte"), (dict(ldu=6), "row stride of U"), (dict(ldv=10), "V must be"),
                           (dict(splits=smax + 1), "col_splits"), (dict(splits=-1), "col_splits"),
                           (dict(lse=None), "lse")):
            rc, msg = _raw(fn, **over)
            assert rc == -1 and word in msg and f"rm_inbatch_softmax_{fn}" in msg, (fn, over, rc, msg)
    for over, word in ((dict(dU=None), "dU is NULL"), (dict(lddv=4), "row stride of dV"), (dict(lddu=9), "dU must be")):
        rc, msg = _raw("bwd", **over)
        assert rc == -1 and word in msg, (over, rc, msg)
    assert not ops.inbatch_softmax_supported(6) and ops.inbatch_softmax_supported(256)
    assert not ops.inbatch_softmax_supported(260) and ops.inbatch_softmax_supported(4)
    with pytest.raises(ValueError, match="unsupported"):
        ops.inbatch_softmax_tile(6)
    # the wrappers refuse what the library would: shapes, dtypes, a short workspace
    U = torch.zeros(8, 8, device="cuda")
    v = torch.zeros(8, device="cuda")
    with pytest.raises(ValueError, match="workspace too small"):
        ops.inbatch_softmax_fwd(U, U, 1.0, v, v.clone(), torch.zeros(1, device="cuda"), torch.zeros(8, device="cuda"))
    with pytest.raises(ValueError, match=r"\[B, H\]"):
        ops.inbatch_softmax_fwd(U, U[:4], 1.0, v, v, v[:1], v)
    from recman_amd._lib import RecmanHipError

    with pytest.raises(RecmanHipError, match="H=260"):
        ops.rownorm_fwd(torch.zeros(2, 260, device="cuda"), torch.zeros(2, 260, device="cuda"),
                        torch.zeros(2, device="cuda"))
    with pytest.raises(RecmanHipError, match="eps"):
        ops.rownorm_fwd(U, U.clone(), v, eps=0.0)
