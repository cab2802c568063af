"""GPU: the grouped gate mixture of PLE / CGC (rm_cgc_mix_fwd / rm_cgc_mix_bwd) and the entire-space loss head
(rm_multitask_loss_es) against the float64 restatement (tests/ple_ref.py, pinned without a GPU in
tests/test_ple_host.py).  Tolerance, the convention of tests/test_gpu_asp.py: for every output the project's gradient
measure against float64 must be <= max(2e-5, 4 x the float32 CPU restatement's own measure on the case); both numbers
are printed."""
import pytest
import torch

from tests import ple_ref as R
from tests import stale_state as SS
from tests.stale_state import lds_pattern  # noqa: F401  (the fixture)
from tests.test_gpu_mmoe import _canaries_intact, _out, _view

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")

# the ledger (tests/test_ple_host.py): entry point of include/recman_hip_multitask.h with a stream -> its test under
# lds_pattern
COVERED = {
    "rm_cgc_mix_fwd": "test_mixture_forward_ignores_stale_lds",
    "rm_cgc_mix_bwd": "test_mixture_backward_ignores_stale_lds",
    "rm_multitask_loss_es": "test_entire_space_loss_ignores_stale_lds_and_keeps_to_its_workspace",
}


def _check(what, got, want, f32):
    m = R.grad_measure(got, want)
    print(f"{what}: measure {m:.2e}, float32 CPU {f32:.2e}, bound {R.bound(f32):.2e}")
    assert m <= R.bound(f32), f"{what}: {m:.3e} > {R.bound(f32):.3e}"


def _run(c, pad=0, want_p=False):
    """Forward and backward of a mix case; every operand a column range at stride width + 4 + pad when pad is set."""
    from recman_amd import ops

    B, T, S, C, H, sg, N, AW, G = (c[n] for n in ("B", "T", "S", "C", "H", "sg", "N", "AW", "G"))
    Z, zb, zl = _view(c["Z"], pad)
    A, ab, al = _view(c["A"], pad)
    dM, db, dl = _view(c["dM"], pad)
    M_, mb, ml = _out(B, G * H, pad)
    P, pb, pl = _out(B, AW, pad) if want_p else (None, None, 0)
    dZ, dzb, dzl = _out(B, N * H, pad)
    dA, dab, dal = _out(B, AW, pad)
    ops.cgc_mix_fwd(Z, A, T, S, C, sg, M_, P=P)
    ops.cgc_mix_bwd(Z, A, T, S, C, sg, dM, dZ, dA)
    torch.cuda.synchronize()
    bufs = dict(M=(mb, ml, G * H), dZ=(dzb, dzl, N * H), dA=(dab, dal, AW))
    if want_p:
        bufs["P"] = (pb, pl, AW)
    return dict(M=M_, P=P, dZ=dZ, dA=dA), bufs


@pytest.mark.parametrize("shape", R.MIX_CASES)
def test_mixture_matches_float64(hip_lib, shape):
    B, T, S, C, H, sg = shape
    c = R.mix_case(*shape)
    out, _ = _run(c)
    for n in ("M", "dZ", "dA"):
        _check(f"{shape} {n}", out[n], c[n], c["f32"][n])
        assert bool(torch.isfinite(out[n]).all())


def test_degenerate_gates(hip_lib):
    from recman_amd import ops

    # S = 1, C = 1 with logits x 60: every softmax is one-hot and only the subtracted maximum keeps it finite
    for sg in (0, 1):
        c = R.mix_case(33, 3, 1, 1, 8, sg, logit_scale=60.0)
        out, _ = _run(c, want_p=True)
        for n in ("M", "dZ", "dA", "P"):
            assert bool(torch.isfinite(out[n]).all()), n
        for n in ("M", "dZ", "dA"):
            _check(f"x60 shared_gate={sg} {n}", out[n], c[n], c["f32"][n])
    # equal logits: p = 1 / W exactly for W a power of two (the shared gate: 1 / N)
    for T, S, C in ((2, 1, 1), (3, 2, 2), (2, 4, 4), (1, 1, 1)):
        H, B = 16, 19
        N, AW, G = R.widths(T, S, C, 1)
        Z = torch.randn(B, N * H, device="cuda")
        A, P = _out(B, AW, 0)[0], _out(B, AW, 0)[0]
        A.fill_(-3.25)
        M_ = torch.empty(B, G * H, device="cuda")
        ops.cgc_mix_fwd(Z, A, T, S, C, 1, M_, P=P)
        W = S + C
        assert bool((P[:, : T * W] == 1.0 / W).all()), (T, S, C)
        if N & (N - 1) == 0:
            assert bool((P[:, T * W:] == 1.0 / N).all()), (T, S, C)
        want, _ = R.cgc_fwd(Z.double(), A.double(), T, S, C, 1)
        assert float((M_.double() - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("shape,pad", [((77, 2, 2, 2, 128, 1), 8), ((33, 8, 3, 8, 36, 1), 12),
                                       ((70, 3, 1, 1, 512, 1), 20), ((5, 2, 1, 2, 8, 0), 4)])
def test_column_ranges_of_wider_buffers(hip_lib, shape, pad):
    """Every operand is a column range of a NaN-filled buffer; the strides are multiples of 4 and not of 32."""
    B, T, S, C, H, sg = shape
    c = R.mix_case(*shape)
    out, bufs = _run(c, pad=pad, want_p=True)
    for n, (buf, lead, W) in bufs.items():
        assert buf.stride(0) % 4 == 0 and buf.stride(0) % 32 != 0, (n, buf.stride(0))
        assert _canaries_intact(buf, lead, W), f"{n}: a column outside its range was written"
    for n in ("M", "dZ", "dA"):
        _check(f"{shape} strided {n}", out[n], c[n], c["f32"][n])
    plain, _ = _run(c)  # the same bits as from contiguous operands
    for n in ("M", "dZ", "dA"):
        assert torch.equal(out[n], plain[n]), n
    assert float((out["P"].cpu().double() - c["P"]).abs().max()) <= 1e-6
    for a0, a1, _ in R.gates(T, S, C, sg):
        assert float((out["P"][:, a0:a1].double().sum(dim=1) - 1).abs().max()) <= 1e-6


def test_grid_stride_walk(hip_lib):
    """B from the kernel's own tile and grid cap: every block walks three whole tiles, the first blocks a fourth, and
    the last tile is partial."""
    from recman_amd import ops

    T, S, C, H, sg = 2, 1, 1, 8, 1
    tile, cap = ops.cgc_mix_tile(T, S, C, H, sg), ops.cgc_mix_tile(T, S, C, H, sg, "cap")
    assert (tile, cap) == (128, 1024) and ops.cgc_mix_tile(T, S, C, H, sg, backward=True) == tile
    B = 3 * tile * cap + 5 * tile + 77
    assert B // (tile * cap) == 3 and B % tile not in (0, tile)
    N, AW, G = R.widths(T, S, C, sg)
    g = torch.Generator(device="cuda").manual_seed(5)
    Z = torch.randn(B, N * H, device="cuda", generator=g)
    A = torch.randn(B, (AW + 3) // 4 * 4, device="cuda", generator=g)[:, :AW]  # (rows of whole float4s: AW = 7)
    dM = torch.randn(B, G * H, device="cuda", generator=g)
    M_, dZ, dA = (torch.empty(B, G * H, device="cuda"), torch.empty(B, N * H, device="cuda"),
                  torch.empty(B, (AW + 3) // 4 * 4, device="cuda")[:, :AW])
    ops.cgc_mix_fwd(Z, A, T, S, C, sg, M_)
    ops.cgc_mix_bwd(Z, A, T, S, C, sg, dM, dZ, dA)
    torch.cuda.synchronize()
    # float64 on the device (the restatement's own functions): the whole batch, first to last example
    M64, _ = R.cgc_fwd(Z.double(), A.double(), T, S, C, sg)
    dZ64, dA64 = R.cgc_bwd(Z.double(), A.double(), T, S, C, sg, dM.double())
    M32, _ = R.cgc_fwd(Z, A, T, S, C, sg)
    dZ32, dA32 = R.cgc_bwd(Z, A, T, S, C, sg, dM)
    for n, got, want, twin in (("M", M_, M64, M32), ("dZ", dZ, dZ64, dZ32), ("dA", dA, dA64, dA32)):
        _check(f"grid-stride {n}", got, want, R.grad_measure(twin, want))
        last = slice(B - 77, B)
        assert R.grad_measure(got[last], want[last]) <= R.bound(R.grad_measure(twin[last], want[last])), n


@pytest.mark.parametrize("shape", [(77, 2, 2, 2, 128, 1), (33, 8, 3, 8, 36, 1), (70, 3, 1, 1, 512, 1)])
def test_two_runs_are_bit_equal_and_p_changes_nothing(hip_lib, shape):
    c = R.mix_case(*shape)
    a, _ = _run(c)
    b, _ = _run(c, want_p=True)
    for n in ("M", "dZ", "dA"):
        assert torch.equal(a[n], b[n]), f"{n} differs between two runs"
    again, _ = _run(c, want_p=True)
    assert torch.equal(b["P"], again["P"])


@pytest.mark.parametrize("B,S,C,H,pad", [(33, 1, 1, 8, 0), (37, 2, 3, 36, 4), (5, 4, 8, 260, 0)])
def test_one_task_without_the_shared_gate_is_the_mmoe_mixture(hip_lib, B, S, C, H, pad):
    """T = 1, shared_gate = 0: the one gate sees its S own experts, then the C shared ones - all E = S + C experts in
    Z's order, as rm_mmoe_mix_fwd/bwd(E, T = 1) do.  The same bits from both entry points.  (A ragged tile; a lane
    group that H / 4 does not fill, on column ranges; two column vectors per lane.)"""
    from tests.test_gpu_mmoe import _run as mmoe_run

    c = R.mix_case(B, 1, S, C, H, 0)
    assert (c["N"], c["AW"], c["G"]) == (S + C, S + C, 1)
    cgc, _ = _run(c, pad=pad, want_p=True)
    mmoe, _ = mmoe_run(dict(B=B, E=S + C, T=1, H=H, Z=c["Z"], A=c["A"], dM=c["dM"]), pad=pad, want_p=True)
    for n in ("M", "P", "dZ", "dA"):
        assert bool(torch.isfinite(cgc[n]).all()), n
        assert torch.equal(cgc[n], mmoe[n]), f"{n}: rm_cgc_mix and rm_mmoe_mix differ"


def test_refusals_name_the_limits(hip_lib):
    from recman_amd import ops
    from recman_amd._lib import RecmanHipError

    def call(T, S, C, H, sg=1, B=4, ldz=None):
        N, AW, G = R.widths(T, S, C, sg)
        Z = torch.zeros(B, ldz or N * H, device="cuda")[:, : N * H]
        A = torch.zeros(B, (AW + 3) // 4 * 4, device="cuda")[:, :AW]
        ops.cgc_mix_fwd(Z, A, T, S, C, sg, torch.zeros(B, G * H, device="cuda"))

    limits = r"1 <= T <= 8.*1 <= S <= 4.*1 <= C <= 8.*N = T S \+ C <= 32.*multiple of 4 in 4\.\.512"
    for T, S, C, H in ((2, 5, 2, 8), (2, 2, 9, 8), (8, 4, 1, 8), (9, 1, 1, 8), (2, 2, 2, 6), (2, 2, 2, 516)):
        with pytest.raises(RecmanHipError, match=limits):
            call(T, S, C, H)
    with pytest.raises(RecmanHipError, match=r"row stride.*multiple of 4 floats.*1 <= T <= 8"):
        call(2, 2, 2, 8, ldz=50)  # a stride that is no multiple of 4
    Z, A = torch.zeros(4, 48, device="cuda"), torch.zeros(4, 16, device="cuda")[:, :14]
    with pytest.raises(RecmanHipError, match="multiple of 4 floats"):
        ops.cgc_mix_bwd(Z, A, 2, 2, 2, 1, torch.zeros(4, 24, device="cuda"),
                        torch.zeros(4, 50, device="cuda")[:, :48], A.clone())
    with pytest.raises(ValueError, match=r"\[B, T \(S \+ C\) \+ shared_gate N\]"):
        ops.cgc_mix_fwd(Z, torch.zeros(4, 8, device="cuda"), 2, 2, 2, 1, torch.zeros(4, 24, device="cuda"))
    call(2, 2, 2, 8, B=0)  # an empty batch is fine


# ------------------------------------------------------------------------------------------ the entire-space loss
def _loss_run(c, es=None, ws=None, plain=False):
    from recman_amd import ops

    T, B = c["T"], c["B"]
    dev = "cuda"
    logit, Y = c["logit"].to(F32).to(dev), c["Y"].to(F32).to(dev)
    out = dict(pred=SS.poisoned(T, B), dlogit=SS.poisoned(T, B),
               n_t=torch.full((T,), -1, dtype=torch.int64, device=dev), loss_t=SS.poisoned(T), loss=SS.poisoned(1))
    kw = dict(Y=Y, task_weights=c["weights"], grad_scale=c["grad_scale"], dlogit=out["dlogit"], n_t=out["n_t"],
              loss_t=out["loss_t"], loss=out["loss"])
    if plain:
        ops.multitask_loss(logit, c["types"], out["pred"], workspace=torch.empty(
            ops.multitask_loss_workspace(B, T), device=dev), **kw)
    else:
        ws = torch.empty(ops.multitask_loss_es_workspace(B, T), device=dev) if ws is None else ws
        ops.multitask_loss_es(logit, c["types"], out["pred"], es=c["es"] if es is None else es, workspace=ws, **kw)
    torch.cuda.synchronize()
    return out


def _check_loss(what, out, c):
    assert torch.equal(out["n_t"].cpu(), c["n_t"]), what  # exact
    for n in ("pred", "dlogit", "loss_t"):
        _check(f"{what} {n}", out[n], c[n], c["f32"][n])
    _check(f"{what} loss", out["loss"], c["loss"].reshape(1), c["f32"]["loss_t"])


@pytest.mark.parametrize("T,B,es", R.LOSS_CASES)
def test_entire_space_loss_matches_float64(hip_lib, T, B, es):
    from recman_amd import ops

    c = R.es_case(T, B, es)
    out = _loss_run(c)
    _check_loss(f"T={T} B={B} es={es}", out, c)
    v = es[1]
    unseen = ~c["z_seen"]
    g = out["dlogit"].cpu()
    # +0.0 exactly where z is unobserved (bit pattern 0, not -0.0)
    assert bool((g[v][unseen].view(torch.int32) == 0).all())
    for t in range(T):
        if t != v and t != es[0]:
            assert bool((g[t][torch.isnan(c["Y"][:, t])].view(torch.int32) == 0).all())
    assert bool(torch.isfinite(out["pred"]).all())  # written for every row; pred[v] stays pCVR
    assert R.grad_measure(out["pred"][v], torch.sigmoid(c["logit"][v])) <= R.bound(c["f32"]["pred"])
    again = _loss_run(c)
    for n in out:
        assert torch.equal(out[n], again[n]), f"{n} differs between two runs"
    # es = (-1, -1): rm_multitask_loss's bits
    a, b = _loss_run(c, es=(-1, -1)), _loss_run(c, plain=True)
    for n in a:
        assert torch.equal(a[n], b[n]), f"es = (-1, -1): {n} differs from multitask_loss"
    # inference (labels and every training output NULL): the same pred bits
    pred_i = SS.poisoned(T, B)
    ops.multitask_loss_es(c["logit"].to(F32).cuda(), c["types"], pred_i, es=es)
    assert torch.equal(pred_i, out["pred"])


def test_entire_space_loss_saturation(hip_lib):
    c = R.saturation_case()
    out = _loss_run(c)
    for n in ("pred", "dlogit", "loss_t", "loss"):
        assert bool(torch.isfinite(out[n]).all()), n
    g = out["dlogit"].cpu()
    assert bool((g[1][c["clipped"]].view(torch.int32) == 0).all())  # exactly +0.0 inside the clip region
    assert float(g[1][~c["clipped"]].abs().min()) > 0.0
    _check_loss("saturation grid", out, c)
    # outside the clip region alone (the rows of v that carry a gradient)
    keep = ~c["clipped"]
    m = R.grad_measure(g[1][keep], c["dlogit"][1][keep])
    print(f"saturation grid, coupled gradient outside the clip region: measure {m:.2e}")
    assert m <= R.bound(c["f32"]["dlogit"])


def test_ops_refuse_a_bad_pair(hip_lib):
    from recman_amd import ops

    logit, pred = torch.zeros(3, 5, device="cuda"), torch.zeros(3, 5, device="cuda")
    types = ["classification", "regression", "classification"]
    for es in ((0, 0), (0, 3), (-1, 0), (0, 1)):
        with pytest.raises(ValueError, match="two distinct classification tasks"):
            ops.multitask_loss_es(logit, types, pred, es=es)
    ops.multitask_loss_es(logit, types, pred, es=(2, 0))


# ------------------------------------------------------------------------------------------------------ stale state
def _mix_checked(c, names):
    def check(res):
        for n in names:
            assert bool(torch.isfinite(res[n]).all()), n
            _check(f"stale LDS {n}", res[n], c[n], c["f32"][n])
    return check


@pytest.mark.parametrize("shape", [(77, 2, 2, 2, 128, 1), (33, 8, 3, 8, 36, 1), (5, 1, 1, 1, 4, 0)])
def test_mixture_forward_ignores_stale_lds(lds_pattern, shape):  # noqa: F811
    from recman_amd import ops

    B, T, S, C, H, sg = shape
    c = R.mix_case(*shape)
    Z, A = c["Z"].to(F32).cuda(), _view(c["A"], 0)[0]

    def run():
        M_, P = SS.poisoned(B, c["G"] * H), _out(B, c["AW"], 0)[0]
        ops.cgc_mix_fwd(Z, A, T, S, C, sg, M_, P=P)
        return dict(M=M_, P=P)

    SS.run_patterns(run, _mix_checked(c, ("M",)), what=f"cgc_mix_fwd {shape}: ")
    assert "rm_cgc_mix_fwd" in lds_pattern["seen"] and lds_pattern["fills"] >= 4


@pytest.mark.parametrize("shape", [(77, 2, 2, 2, 128, 1), (33, 8, 3, 8, 36, 1), (5, 1, 1, 1, 4, 0)])
def test_mixture_backward_ignores_stale_lds(lds_pattern, shape):  # noqa: F811
    from recman_amd import ops

    B, T, S, C, H, sg = shape
    c = R.mix_case(*shape)
    Z, A, dM = c["Z"].to(F32).cuda(), _view(c["A"], 0)[0], c["dM"].to(F32).cuda()

    def run():
        dZ, dA = SS.poisoned(B, c["N"] * H), _out(B, c["AW"], 0)[0]
        ops.cgc_mix_bwd(Z, A, T, S, C, sg, dM, dZ, dA)
        return dict(dZ=dZ, dA=dA)

    SS.run_patterns(run, _mix_checked(c, ("dZ", "dA")), what=f"cgc_mix_bwd {shape}: ")
    assert "rm_cgc_mix_bwd" in lds_pattern["seen"] and lds_pattern["fills"] >= 4


@pytest.mark.parametrize("T,B,es", [(3, 77, (0, 1)), (8, 4099, (0, 1)), (3, 77, (2, 0))])
def test_entire_space_loss_ignores_stale_lds_and_keeps_to_its_workspace(lds_pattern, T, B, es):  # noqa: F811
    from recman_amd import ops

    c = R.es_case(T, B, es)
    ws, buf = SS.guarded(ops.multitask_loss_es_workspace(B, T))

    def run():
        ws.fill_(NAN)
        return _loss_run(c, ws=ws)

    SS.run_patterns(run, lambda res: _check_loss(f"stale LDS T={T} B={B}", res, c), what="multitask_loss_es: ")
    SS.assert_guards_intact(buf, "rm_multitask_loss_es")
    assert "rm_multitask_loss_es" in lds_pattern["seen"] and "rm_multitask_loss" not in lds_pattern["seen"]


def test_ledger_is_the_fixture_s_view(lds_pattern):  # noqa: F811
    """The three tests above saw, through the fixture, exactly the entry points COVERED claims."""
    from recman_amd import ops

    c = R.mix_case(5, 1, 1, 1, 4, 0)
    Z, A, dM = c["Z"].to(F32).cuda(), _view(c["A"], 0)[0], c["dM"].to(F32).cuda()
    ops.cgc_mix_fwd(Z, A, 1, 1, 1, 0, SS.poisoned(5, 4))
    ops.cgc_mix_bwd(Z, A, 1, 1, 1, 0, dM, SS.poisoned(5, 8), _out(5, c["AW"], 0)[0])
    _loss_run(R.es_case(2, 1))
    assert lds_pattern["seen"] == set(COVERED)
