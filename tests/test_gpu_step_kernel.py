"""GPU: rm_deepfm_step (csrc/step.hip), the one-kernel DeepFM training step, called directly through
recman_amd.ops.deepfm_step and held to the float64 restatement of tests/step_ref.py (pinned against the model oracle
by tests/test_step_host.py), at the shapes the engines never show it.  Tolerances are the ones tests/test_gpu_step.py
and tests/test_gpu_steady_state.py hold this kernel to: logit / pred 1e-5 absolute, loss _close's defaults, dlogit,
d_rows and every parameter gradient _close_grad's 2e-5.  Every test prints the largest errors it saw.

Buffers.  Every output is a 16-byte-aligned view into a larger buffer with 64 floats of a sentinel bit pattern on
either side, pre-filled with NaN (the packed form's send buffer: with the sentinel); the workspace is NaN.  After
every call the sentinels are intact and every output is finite: a store past an output shows in a guard band, an
element that was not written shows as NaN.  Table columns past the 18 the kernel reads are NaN.

What each section reaches (line numbers of csrc/step.hip):
 a. slot map - slot_field (:119-121) spreads 27 slots over 7 workers and skips worker 3 in round 3; sv / sx (:196-197)
    decide from it which slots hold an embedding field, the dense pseudo-field (slot field == F, Dn > 0) or nothing.
    Every F in 1..26 puts the dense slot at every (worker, round) it can take, F = 26 with Dn = 0 leaves slot 26
    empty; Dn = 0..16 covers the head's column masks of the dense row (:651-652, :668) and of lin_w_dense (:451-452).
    B = 37: three tiles on three blocks, the last ragged (rows_t = 5, :308-314).
 b. hidden widths - `uf < H0` / `ux < H0` mask the workers' two W0 operand layouts (:205-211), `u < H0 && v < H1`
    the head's W1 image (:441-443), `lane < H0` / `lane < H1` b0, b1 and w_out (:447-450); the finishing launch
    stores `k < K && u < H0` (csrc/mlp.hip mlp_dw0_reduce_body).  (H0, H1) = (H, 33 - H) for H in 1..32.
 c. row stride - a.row_bytes = table_ld * 4 (:778) enters the row address only (:337): strides 20, 24, 32, 36.
 d. bounds - the guard bands of every call above; B = 0 returns before anything is touched (:765).
 e. packed form - deepfm_step_kernel<NT, false, true> (:797-798): the register pipeline rp[4][kSlots] (:236-304)
    carries an occurrence's position from the segment that requests tile s + 1 (:303) to the one that stores the
    gradient of tile s - 2 (:321); it is in its steady state once a block runs T >= 2 tiles (:719), which needs
    more than 256 tiles (:775-776).  B = 8 200: T = 2 (3 in block 0), fill and drain overlap; B = 17 609: T = 4 or
    5, the 3-slot row ring wraps in every block and the last tile has 9 examples (ex_ok, :314, and the dropped
    store at 0x7ffffff0, :321-324).  lin_field_mask (:243) at None, ones and 0/1.
 f. rows past 4 GiB - the row address (int64_t)rid[j] * a.row_bytes (:337) with rid a u32: a 4.3 GB table whose
    last rows lie past byte offset 2^32.
"""
import functools
import os
import struct

import pytest
import torch

from tests import step_ref as SR
from tests.test_gpu_parity import _close, _close_grad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32, I64 = torch.float32, torch.int32, torch.int64
NAN = float("nan")
SENT = -777.25
SENT_BITS = struct.unpack("<i", struct.pack("<f", SENT))[0]
G = 64  # guard floats on either side of every output: 256 bytes, so the view keeps the buffer's alignment


def cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def _src():
    with open(os.path.join(ROOT, "recman_amd", "csrc", "step.hip")) as f:
        return " ".join(f.read().split())


def _cite(snippet):
    """The code a case relies on, as it stands in csrc/step.hip (whitespace-insensitive)."""
    assert " ".join(snippet.split()) in _src(), f"csrc/step.hip no longer contains `{snippet}`: re-derive this case"


def _bits(t):
    return t.contiguous().view(I32)


class Guarded:
    """A tensor of `shape` inside a buffer with G sentinel floats before and behind it."""

    def __init__(self, shape, fill=NAN):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * G,), SENT, dtype=F32, device="cuda")
        self.t = self.buf[G: G + n].view(*shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()

    def check(self, what):
        b = _bits(self.buf)
        ok = bool((b[:G] == SENT_BITS).all()) and bool((b[b.numel() - G:] == SENT_BITS).all())
        assert ok, f"{what}: the sentinels around the output were overwritten"


SMALL = ("logit", "pred", "dlogit", "loss") + SR.PARAM_GRADS


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _run(c, what, rows=None, idx=None, field_off=None, packed_rows=0, mask=None, grad_scale=1.0):
    """One call of ops.deepfm_step on case c (rows / idx / field_off: another table of the same rows).  Returns
    name -> Guarded of every output, d_rows [B,F,16] - or the send buffer [packed_rows, 20] - among them."""
    from recman_amd import ops

    rows = _dev(c.rows if rows is None else rows)
    idx = _dev(c.idx if idx is None else idx)
    field_off = _dev(c.field_off if field_off is None else field_off)
    B, F = idx.shape
    K = SR.D * F + c.Dn
    shapes = dict(logit=(B,), pred=(B,), dlogit=(B,), loss=(1,), dW0=(K, c.H0), db0=(c.H0,), dW1=(c.H0, c.H1),
                  db1=(c.H1,), d_w_out=(c.H1,), d_w0_out=(1,), d_lin_w0=(1,))
    if c.Dn:
        shapes["d_lin_w_dense"] = (c.Dn,)
    o = {k: Guarded(s) for k, s in shapes.items()}
    o["d_rows"] = Guarded((packed_rows, SR.D + 4), fill=SENT) if packed_rows else Guarded((B, F, SR.D))
    t = lambda k: o[k].t if k in o else None
    ws = torch.full((ops.deepfm_step_workspace(F, c.Dn),), NAN, dtype=F32, device="cuda")
    ops.deepfm_step(idx, rows, field_off, SR.D, rows.shape[1], _dev(c.dense), _dev(c.y),
                    [_dev(c.W0), _dev(c.W1)], [_dev(c.b0), _dev(c.b1)], _dev(c.w_out), _dev(c.w0_out),
                    _dev(c.lin_w_dense), _dev(c.lin_w0), c.act, c.task, t("d_rows"), t("logit"), t("pred"),
                    t("dlogit"), t("loss"), [t("dW0"), t("dW1")], [t("db0"), t("db1")], t("d_w_out"), t("d_w0_out"),
                    t("d_lin_w_dense"), t("d_lin_w0"), ws, grad_scale=grad_scale, packed_rows=packed_rows,
                    lin_field_mask=_dev(mask))
    torch.cuda.synchronize()
    for k, g in o.items():  # d. bounds
        g.check(f"{what}: {k}")
        if not (packed_rows and k == "d_rows"):
            assert bool(torch.isfinite(g.t).all()), f"{what}: {k} holds a NaN or an infinity (an element not written?)"
    return o


def _err(got, want):
    return float((got.detach().cpu().double() - want).abs().max())


def _rel_err(got, want):
    """The largest error in units of _close_grad's per-element scale (its tolerance is 2e-5 of that)."""
    got, want = got.detach().cpu().double(), want.double()
    scale = float(want.abs().max())
    if scale == 0.0:
        return float(got.abs().max())
    return float(((got - want).abs() / torch.clamp(want.abs(), min=0.1 * scale)).max())


def _check_small(o, ref, what):
    """logit, pred, dlogit, loss and the parameter gradients against float64."""
    seen = dict(logit=_err(o["logit"].t, ref["logit"]), pred=_err(o["pred"].t, ref["pred"]),
                loss=_err(o["loss"].t, ref["loss"]))
    grads = ("dlogit",) + SR.PARAM_GRADS
    seen.update({k: _rel_err(o[k].t, ref[k]) for k in grads if ref[k] is not None})
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in seen.items()))
    _close(o["logit"].t, ref["logit"], rtol=0, atol=1e-5, what=f"{what}: logit vs float64")
    _close(o["pred"].t, ref["pred"], rtol=0, atol=1e-5, what=f"{what}: pred vs float64")
    _close(o["loss"].t, ref["loss"], what=f"{what}: loss vs float64")
    for k in grads:
        if ref[k] is None:
            assert k not in o
        else:
            _close_grad(o[k].t, ref[k], what=f"{what}: {k} vs float64")


def _check_plain(o, ref, what):
    _check_small(o, ref, what)
    print(f"{what}: d_rows {_rel_err(o['d_rows'].t, ref['d_rows']):.2e}")
    _close_grad(o["d_rows"].t, ref["d_rows"], what=f"{what}: d_rows vs float64")


def _assert_same_bits(a, b, what, keys=None):
    for k in keys or a:
        assert torch.equal(_bits(a[k].buf), _bits(b[k].buf)), f"{what}: {k} differs"


@functools.lru_cache(maxsize=4)
def _case_ref(key):
    """(case, float64 reference), built once per case and shared: read-only."""
    c = SR.make_step_case(**dict(key))
    return c, SR.ref_of(c)


def _key(kw):
    return tuple(sorted(kw.items()))


def _id(kw):
    return "B{B}F{F}Dn{Dn}H{H0}x{H1}-{act}-{task}".format(**kw)


# ------------------------------------------------------------------------------------------------------ a. slot map
def slot_field(w, j):
    _cite("return j < 3 ? 7 * j + w : (w < 3 ? 21 + w : (w > 3 ? 20 + w : -1));")
    return 7 * j + w if j < 3 else (21 + w if w < 3 else (20 + w if w > 3 else -1))


def test_slot_sweep_puts_the_dense_slot_everywhere_it_can_sit():
    slots = {(w, j): slot_field(w, j) for w in range(7) for j in range(4)}
    assert sorted(f for f in slots.values() if f >= 0) == list(range(27)) and slots[(3, 3)] == -1
    at = {f: wj for wj, f in slots.items()}
    # the dense pseudo-field is slot field F: every slot but field 0's, as F runs through 1..26
    seen = {at[k["F"]] for k in SR.SLOT_CASES if k["Dn"] > 0}
    assert seen == set(slots) - {(0, 0), (3, 3)}
    assert {at[F] for F in (22, 23, 24, 25)} == {(1, 3), (2, 3), (4, 3), (5, 3)}   # the last round, around worker 3
    assert {at[F] for F in (6, 13, 20)} == {(6, 0), (6, 1), (6, 2)}                # worker 6's slots of rounds 0..2
    assert any(k["F"] == 26 and k["Dn"] == 0 for k in SR.SLOT_CASES)               # slot 26 empty
    assert any(k["F"] == 26 and k["Dn"] == 16 for k in SR.SLOT_CASES)
    assert {k["Dn"] for k in SR.SLOT_CASES} == set(range(17))
    assert all(k["B"] == 37 and (k["H0"], k["H1"]) == (32, 32) for k in SR.SLOT_CASES)


@pytest.mark.parametrize("kw", SR.SLOT_CASES, ids=_id)
def test_slot_map_sweep_matches_float64(hip_lib, kw):
    c, ref = _case_ref(_key(kw))
    assert cdiv(c.B, 16) == 3 and c.B % 16 == 5
    _check_plain(_run(c, _id(kw)), ref, _id(kw))


# ---------------------------------------------------------------------------------------------------- b. widths
@pytest.mark.parametrize("kw", SR.WIDTH_CASES, ids=_id)
def test_hidden_width_sweep_matches_float64(hip_lib, kw):
    assert kw["H0"] + kw["H1"] == 33
    c, ref = _case_ref(_key(kw))
    _check_plain(_run(c, _id(kw)), ref, _id(kw))


# ------------------------------------------------------------------------------------------------ c. row stride
def test_row_strides_match_float64_and_each_other_bit_for_bit(hip_lib):
    from recman_amd import ops

    _cite("a.row_bytes = table_ld * 4;")
    c, ref = _case_ref(_key(SR.STRIDE_CASE))
    assert (c.B, c.F, c.Dn) == (53, 9, 4)
    first = None
    for ld in SR.STRIDES:
        w = SR.with_stride(c, ld)
        assert ops.deepfm_step_supported(w.F, SR.D, ld, w.Dn, (w.H0, w.H1))
        assert w.rows.shape[1] == ld and bool(torch.isnan(w.rows[:, SR.COLS:]).all())
        o = _run(w, f"table_ld {ld}")
        _check_plain(o, ref, f"table_ld {ld}")
        first = first or o
        _assert_same_bits(o, first, f"table_ld {ld} against {SR.STRIDES[0]}")


def test_grad_scale_multiplies_every_gradient_and_not_the_loss(hip_lib):
    """grad_scale (a micro-batch's share of the step) enters at dlogit (`gb *= a.grad_scale`)."""
    _cite("gb *= a.grad_scale;")
    c, ref1 = _case_ref(_key(SR.STRIDE_CASE))
    ref = SR.ref_of(c, grad_scale=0.25)
    assert torch.equal(ref["loss"], ref1["loss"]) and not torch.equal(ref["dlogit"], ref1["dlogit"])
    _check_plain(_run(c, "grad_scale 0.25", grad_scale=0.25), ref, "grad_scale 0.25")


# ----------------------------------------------------------------------------------------------------- d. B = 0
def test_empty_batch_touches_nothing(hip_lib):
    from recman_amd import ops

    _cite("if (B == 0) return RM_OK;")
    c, _ = _case_ref(_key(SR.STRIDE_CASE))
    K = SR.D * c.F + c.Dn
    shapes = dict(d_rows=(16, c.F, SR.D), logit=(0,), pred=(0,), dlogit=(0,), loss=(1,), dW0=(K, c.H0), db0=(c.H0,),
                  dW1=(c.H0, c.H1), db1=(c.H1,), d_w_out=(c.H1,), d_w0_out=(1,), d_lin_w_dense=(c.Dn,), d_lin_w0=(1,))
    o = {k: Guarded(s) for k, s in shapes.items()}
    before = {k: g.buf.clone() for k, g in o.items()}
    ws = torch.full((ops.deepfm_step_workspace(c.F, c.Dn),), NAN, dtype=F32, device="cuda")
    t = lambda k: o[k].t
    ops.deepfm_step(torch.zeros(0, c.F, dtype=I64, device="cuda"), _dev(c.rows), _dev(c.field_off), SR.D, c.table_ld,
                    torch.zeros(0, c.Dn, device="cuda"), torch.zeros(0, dtype=I64, device="cuda"),
                    [_dev(c.W0), _dev(c.W1)], [_dev(c.b0), _dev(c.b1)], _dev(c.w_out), _dev(c.w0_out),
                    _dev(c.lin_w_dense), _dev(c.lin_w0), c.act, c.task, t("d_rows"), t("logit"), t("pred"),
                    t("dlogit"), t("loss"), [t("dW0"), t("dW1")], [t("db0"), t("db1")], t("d_w_out"), t("d_w0_out"),
                    t("d_lin_w_dense"), t("d_lin_w0"), ws)
    torch.cuda.synchronize()
    for k, g in o.items():
        assert torch.equal(_bits(g.buf), _bits(before[k])), f"B = 0 wrote to {k}"
    assert bool(torch.isnan(ws).all()), "B = 0 wrote to the workspace"


# -------------------------------------------------------------------------------------------------- e. packed form
def _packed_launch(B):
    """(tiles, blocks, tiles per block) of a batch, from rm_deepfm_step's launch arithmetic."""
    _cite("const int64_t ntiles = (B + 15) / 16;")
    _cite("const int nblk = rm_grid_cap(ntiles, 256);")
    _cite("const int T = (int)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x);")
    ntiles = cdiv(B, 16)
    nblk = min(ntiles, 256)
    return ntiles, nblk, [cdiv(ntiles - b, nblk) for b in range(nblk)]


def _assert_packed_launch(B):
    ntiles, nblk, T = _packed_launch(B)
    want = {1: 1, 16: 1, 17: 2, 37: 3, 8200: 513, 17609: 1101}
    assert ntiles == want[B]
    if B <= 37:
        assert nblk == ntiles and set(T) == {1}
    elif B == 8200:
        # two tiles per block and three in block 0: the pipeline requests a tile's rows while the positions of
        # the tile before are still on their way to the store (fill and drain overlap)
        assert nblk == 256 and T[0] == 3 and set(T[1:]) == {2} and B % 16 == 8
    else:
        # every block at least 4 tiles: the 3-slot ring wraps in each; the last tile is ragged and not a first tile
        assert nblk == 256 and min(T) == 4 and max(T) == 5 and B % 16 == 9


@pytest.mark.parametrize("mask", ["none", "ones", "mixed"])
@pytest.mark.parametrize("B,F", list(SR.PACKED_CASES), ids=lambda v: str(v))
def test_packed_form_matches_float64_and_the_plain_form_plus_pack_grad_rows(hip_lib, B, F, mask):
    """The packed form against float64 (the send buffer against step_ref.pack_ref), then bit for bit against the
    plain form followed by ops.pack_grad_rows - PACKED changes only where the row gradients are stored (:311, :321)
    and multiplies dlogit by a 0/1 or absent mask exactly as rm_pack_grad_rows does - and against a second run."""
    from recman_amd import ops

    kw = SR.PACKED_CASES[(B, F)]
    what = f"packed B{B} F{F} mask {mask}"
    _assert_packed_launch(B)
    _cite("const int base = (ok && ex_ok) ? (int)rp[3][i] * a.out_row_bytes : 0x7ffffff0 - 64;")
    _cite("lmask[j] = (PACKED && a.lin_mask != nullptr && sx[j]) ? a.lin_mask[fld[j]] : 1.f;")
    c, ref = _case_ref(_key(kw))
    assert (c.table_ld, c.F, c.B) == (20, F, B)
    n = B * F + SR.PACKED_SPARE
    pos = SR.packed_positions(B, F, n, seed=kw["seed"])
    m = SR.lin_masks(F)[mask]
    if mask == "mixed":
        assert set(m.tolist()) == {0.0, 1.0}
    used = torch.zeros(n, dtype=torch.bool)
    used[pos.reshape(-1)] = True
    assert int(used.sum()) == B * F
    recv = torch.full((n, 20), NAN)
    recv[pos.reshape(-1)] = c.rows[(c.idx + c.field_off).reshape(-1)]
    zoff = torch.zeros(F, dtype=I64)

    o = _run(c, what, rows=recv, idx=pos, field_off=zoff, packed_rows=n, mask=m)
    _check_small(o, ref, what)
    send = o["d_rows"].t.cpu()
    want = SR.pack_ref(ref["d_rows"], ref["dlogit"], pos, n, m)
    got_rows, got_gb, got_gl, got_pad = SR.unpack_ref(send, pos)
    want_rows, want_gb, want_gl, _ = SR.unpack_ref(want, pos)
    assert bool(torch.isfinite(send[used]).all()), f"{what}: an addressed row of the send buffer was not written"
    print(f"{what}: d_rows {_rel_err(got_rows, want_rows):.2e} g_bias {_rel_err(got_gb, want_gb):.2e} "
          f"g_lin {_rel_err(got_gl, want_gl):.2e}")
    _close_grad(got_rows, want_rows, what=f"{what}: row gradients vs float64")
    _close_grad(got_gb, want_gb, what=f"{what}: column 16 (dlogit) vs float64")
    _close_grad(got_gl, want_gl, what=f"{what}: column 17 (dlogit * lin_field_mask) vs float64")
    assert bool((_bits(got_pad) == 0).all()), f"{what}: columns 18 / 19 of an addressed row are not +0.0"
    assert bool((_bits(send[~used]) == SENT_BITS).all()), f"{what}: a row nobody addresses was written"
    # the kernel's own dlogit is what it packs
    assert torch.equal(got_gb, o["dlogit"].t.cpu().reshape(B, 1).expand(B, F)), f"{what}: column 16 is not dlogit"

    # the plain form on the table itself + rm_pack_grad_rows
    p = _run(c, what + " (plain)")
    out = Guarded((n, SR.D + 4), fill=SENT)
    ops.pack_grad_rows(p["d_rows"].t, p["dlogit"].t, p["dlogit"].t, _dev(pos.reshape(-1)), out.t,
                       lin_field_mask=_dev(m))
    torch.cuda.synchronize()
    out.check(what + ": pack_grad_rows")
    _assert_same_bits(o, p, what + ": packed against plain", keys=[k for k in SMALL if k in o])
    assert torch.equal(_bits(o["d_rows"].buf), _bits(out.buf)), \
        f"{what}: the send buffer differs from the plain form's d_rows packed by rm_pack_grad_rows"
    # two runs
    _assert_same_bits(_run(c, what, rows=recv, idx=pos, field_off=zoff, packed_rows=n, mask=m), o, what + ": second run")


# -------------------------------------------------------------------------------------------- f. rows past 4 GiB
def test_rows_past_4_gib(hip_lib):
    """A table of 2^25 + 2^12 rows of 128 bytes (4.3 GB, allocated uninitialised: only the rows in use are written)
    with every field's ids drawn from its two ends.  Skips when the device has less than 6 GB free."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6e9:
        pytest.skip(f"needs 6 GB of free device memory for the 4.3 GB table, {free / 1e9:.1f} GB are free")
    _cite("(int64_t)rid[j] * a.row_bytes")
    kw = SR.BIG_CASE
    c, _ = _case_ref(_key(kw))
    R, END, ld = SR.BIG_ROWS, SR.BIG_END, c.table_ld
    assert (c.B, c.F, c.Dn, ld) == (37, 26, 13, 32) and R * ld * 4 > 2 ** 32 and R < 2 ** 32
    # every row of the small table gets a home among the first / last 2^11 rows of the big one
    Rs = c.rows.shape[0]
    assert Rs <= 2 * END
    ends = torch.cat([torch.arange(END), torch.arange(R - END, R)])
    home = ends[torch.randperm(2 * END, generator=torch.Generator().manual_seed(kw["seed"]))[:Rs]]
    idx = home[c.idx + c.field_off]
    assert int(idx.min()) < END and int(idx.max()) >= R - END                  # both ends are used
    assert int(idx.max()) * ld * 4 > 2 ** 32                                   # the highest byte offset
    big = torch.empty(R, ld, dtype=F32, device="cuda")
    big[home.cuda()] = c.rows.cuda()
    zoff = torch.zeros(c.F, dtype=I64)
    ref = SR.step_ref(big, idx, zoff, c.dense, c.y, c.W0, c.b0, c.W1, c.b1, c.w_out, c.w0_out, c.lin_w_dense,
                      c.lin_w0, c.act, c.task)   # (gathers the rows in use on the host)
    o = _run(c, "4 GiB table", rows=big, idx=idx, field_off=zoff)
    del big
    torch.cuda.empty_cache()
    _check_plain(o, ref, "4 GiB table")
