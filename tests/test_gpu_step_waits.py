"""GPU: rm_deepfm_step (csrc/step.hip) at the shapes where one of its hand-counted memory waits can be wrong.

The tile loop's barrier waits for LDS only; what keeps a consumer from data still in flight is a counted
`s_waitcnt vmcnt(N)`: the workers' kYounger (rows of the tile, in front of the forward) and kYoungerE (bias / linear
entries), the head's two waits for its prefetch registers.  The counts are derived in csrc/step.hip for a sequence of
vector-memory operations that is the same in every segment; the places where a derivation can go wrong are the
segments in which part of the sequence is a dummy - the fill and the drain - and the first steady segment.  So:

 * tiles per block T = 1, 2, 3, 4 (the grid is capped at 256 blocks): B = 16 k for k = 5 (T = 1, five blocks),
   256 * 2, 256 * 3 + 7 (T = 4 in seven blocks, 3 in the others) and 256 * 4, and B = 16 * 256 * 3 + 5 (a ragged
   last tile, T = 4 in block 0 alone);
 * F = 26, 7, 1: a full slot map, empty slots in every worker's later rounds, workers with no field at all;
 * Dn = 13, 0: with and without the dense pseudo-field (and the head's dense columns reading w_out[0] instead);
 * both row-load policies and both d_rows store policies (stream_rows / stream_d_rows: four kernel instantiations)
   and the packed form (packed_rows > 0, two stores per slot: other counts), driven as tests/test_gpu_dist.py and
   tests/test_gpu_step_kernel.py drive it;
 * about 1,000 rows per field, so that a tile's rows are not all the same few cache lines - and, in a second test,
   a table larger than the last-level cache (4,200,000 rows of 80 bytes = 336 MB against 256 MB) with ids drawn over
   each field's whole range, so that a tile's rows come from HBM and not from a cache that a read issued too early
   would still find its data in.  (Nobody has measured the miss rate of these shapes: the argument is the table's
   size against the cache's.)  The packed form's receive and send buffers have the table's size there.

Every case is held to the float64 reference of tests/step_ref.py with the tolerances of tests/test_gpu_step_kernel.py
(logit / pred 1e-5 absolute, loss _close's defaults, dlogit, d_rows and every parameter gradient _close_grad's 2e-5),
and every variant is run twice and must repeat itself bit for bit - outputs and guard bands: a wait that is too short
shows as a difference between runs long before it shows as a tolerance failure.  The cache policies change no
arithmetic, so the four plain variants must agree bit for bit with each other as well.

Every case runs ONCE per suite run and a failure may not be rerun to learn more, so a failure is a full report
(tests/step_report.py): over ALL outputs of the run, which elements are not finite, outside the tolerance or different
between two runs, and for each the block, the tile within the block (one of the first three = a ring buffer nothing
has written before), the lane, and for row gradients the worker and slot of the field.
"""
import functools
import types

import pytest
import torch

from tests import step_ref as SR
from tests import step_report as RP
from tests.cases import make_case
from tests.test_gpu_parity import _close_grad
from tests.test_gpu_step_kernel import (F32, G, I64, NAN, SENT, SENT_BITS, Guarded, _assert_same_bits, _bits,
                                        _check_plain, _check_small, _dev, _rel_err, cdiv)

pytestmark = pytest.mark.gpu

VOCAB = 1000
TILES = (5, 256 * 2, 256 * 3 + 7, 256 * 4)
BATCHES = tuple(16 * k for k in TILES) + (16 * 256 * 3 + 5,)
FIELDS = (26, 7, 1)
DENSE = (13, 0)
POLICIES = [(False, False), (True, False), (False, True), (True, True)]  # (stream_rows, stream_d_rows)
PACKED_SPARE = 1000
# tests/step_ref.py:default_scale uses 0.3 up to 10 fields at B = 37; among thousands of examples that scale puts
# logits past +-12, where fp32 cannot give dlogit to 2e-5: dlogit ~ (p - y) / B, and 1 - p carries an absolute error
# of fp32's 6e-8 next to 1, so its relative error stays under 2e-5 only while 1 - p > 3e-3, |logit| < 5.8.  Hence the
# scale of that file's F = 26 cases for every F, and the bound is asserted on the float64 logits of every case.
SCALE = 0.05
LOGIT_MAX = 5.8
# the table of the HBM cases: larger than the 256 MB last-level cache at the 80-byte rows of this file
LLC_BYTES = 256 * 2 ** 20
HBM_ROWS = 4_200_000
HBM_BATCHES = (16 * 256 * 3 + 5, 80)
HBM_FIELDS = (7, 26)


def _tiles_per_block(B):
    ntiles = cdiv(B, 16)
    nblk = min(ntiles, 256)
    return [cdiv(ntiles - b, nblk) for b in range(nblk)]


def test_the_batches_give_one_to_four_tiles_per_block_and_a_ragged_tile():
    T = {B: _tiles_per_block(B) for B in BATCHES}
    assert set(T[80]) == {1} and len(T[80]) == 5
    assert set(T[16 * 512]) == {2} and len(T[16 * 512]) == 256
    assert T[16 * 775][:7] == [4] * 7 and set(T[16 * 775][7:]) == {3}
    assert set(T[16 * 1024]) == {4}
    assert BATCHES[-1] % 16 == 5 and T[BATCHES[-1]][0] == 4 and set(T[BATCHES[-1]][1:]) == {3}
    assert HBM_BATCHES[0] == BATCHES[-1] and HBM_ROWS * 80 > LLC_BYTES


def _finish_case(B, F, Dn, seed, rows, idx, field_off, dense, y, p, lin_w_dense, **extra):
    """The B kink-clear examples among the candidates (tests/step_ref.py:make_step_case's rule) and their float64
    reference; rows / idx / field_off are what the reference gathers from, on the host."""
    n = idx.shape[0]
    Ws = [p[f"dnn_layer_{i}_weights"] for i in range(2)]
    bs = [p[f"dnn_layer_{i}_bias"] for i in range(2)]
    a = SR._gather(rows, idx, field_off)[..., :SR.D].reshape(n, F * SR.D)
    if Dn:
        a = torch.cat([a, dense.to(SR.F64)], 1)
    clear = torch.ones(n, dtype=torch.bool)
    for W, b in zip(Ws, bs):
        W, b = W.to(SR.F64), b.to(SR.F64)
        z = a @ W + b
        clear &= SR.kink_clear(z, a.abs() @ W.abs() + b.abs(), W.shape[0])
        a = SR._act(z, "relu")
    sel = clear.nonzero().reshape(-1)[:B]
    assert sel.numel() == B, f"only {sel.numel()} of {B} examples clear of the kink"
    c = types.SimpleNamespace(
        B=B, F=F, Dn=Dn, H0=32, H1=32, table_ld=20, act="relu", task="classification", seed=seed,
        rows=rows, idx=idx[sel].contiguous(), field_off=field_off, dense=dense[sel].contiguous() if Dn else None,
        y=y[sel].contiguous(), W0=Ws[0], b0=bs[0], W1=Ws[1], b1=bs[1], w_out=p["dnn_w"].reshape(-1).clone(),
        w0_out=p["dnn_w0"], lin_w_dense=lin_w_dense if Dn else None, lin_w0=p["linear_w0"],
        **{k: v[sel].contiguous() for k, v in extra.items()})
    ref = SR.ref_of(c)
    assert float(ref["logit"].abs().max()) < LOGIT_MAX
    return c, ref


@functools.lru_cache(maxsize=2)
def _case_ref(B, F, Dn):
    """tests/step_ref.py:make_step_case with VOCAB rows per field (its generators, scales and kink rule), and the
    float64 reference: built once per shape and shared by the variants, read-only."""
    n = B + B // 2
    seed = 600 + 7 * F + Dn
    spec, p, idx, dense, y, _ = make_case("deepfm", B=n, F=F, D=SR.D, Dn=Dn, sizes=[VOCAB] * F, hidden=(32, 32),
                                          seed=seed, scale=SCALE)
    rows, field_off, lin_w_dense = SR.fuse_rows(p, spec, 20)
    return _finish_case(B, F, Dn, seed, rows, idx, field_off, dense, y, p, lin_w_dense)


def _cpu(o):
    return {k: g.t.detach().cpu() for k, g in o.items()}


def _run(c, what, dev, stream_rows=False, stream_d_rows=False, packed=None):
    """One call of ops.deepfm_step on the device tensors `dev` of case c; packed = (rows, positions, field_off, n,
    mask), all on the device.  Outputs in guard bands, pre-filled with NaN (the send buffer: with the sentinel), as in
    test_gpu_step_kernel.  Everything that is wrong with the outputs is collected before anything raises."""
    from recman_amd import ops

    B, F = c.B, c.F
    K = SR.D * F + c.Dn
    shapes = dict(logit=(B,), pred=(B,), dlogit=(B,), loss=(1,), dW0=(K, c.H0), db0=(c.H0,), dW1=(c.H0, c.H1),
                  db1=(c.H1,), d_w_out=(c.H1,), d_w0_out=(1,), d_lin_w0=(1,))
    if c.Dn:
        shapes["d_lin_w_dense"] = (c.Dn,)
    o = {k: Guarded(s) for k, s in shapes.items()}
    rows, idx, field_off, n, mask = packed if packed else (dev["rows"], dev["idx"], dev["field_off"], 0, None)
    o["d_rows"] = Guarded((n, SR.D + 4), fill=SENT) if n else Guarded((B, F, SR.D))
    t = lambda k: o[k].t if k in o else None
    ws = torch.full((ops.deepfm_step_workspace(F, c.Dn),), NAN, dtype=F32, device="cuda")
    ops.deepfm_step(idx, rows, field_off, SR.D, rows.shape[1], dev["dense"], dev["y"], [dev["W0"], dev["W1"]],
                    [dev["b0"], dev["b1"]], dev["w_out"], dev["w0_out"], dev["lin_w_dense"], dev["lin_w0"], c.act,
                    c.task, t("d_rows"), t("logit"), t("pred"), t("dlogit"), t("loss"), [t("dW0"), t("dW1")],
                    [t("db0"), t("db1")], t("d_w_out"), t("d_w0_out"), t("d_lin_w_dense"), t("d_lin_w0"), ws,
                    stream_rows=stream_rows, stream_d_rows=stream_d_rows, packed_rows=n, lin_field_mask=mask)
    torch.cuda.synchronize()
    # ---- the report: every output, before the assertions below stop at the first
    fnd = RP.Findings(what, B, F, c.Dn, pos=idx.cpu() if n else None)
    for k, g in o.items():
        b = _bits(g.buf)
        for side, band in (("in front of", b[:G]), ("behind", b[b.numel() - G:])):
            hit = (band != SENT_BITS).nonzero().reshape(-1)
            if hit.numel():
                fnd.note(f"[guard band] {k}: {hit.numel()} of the {G} sentinels {side} the output were overwritten, "
                         f"first at float {int(hit[0])} of the band")
        bad = ~torch.isfinite(g.t)
        if n and k == "d_rows":  # the send buffer: rows nobody addresses keep the sentinel, addressed ones are written
            used = torch.zeros(n, dtype=torch.bool, device="cuda")
            used[idx.reshape(-1)] = True
            bad &= used.reshape(n, 1)
        fnd.add("NaN or infinity (an element not written?)", k, bad, values=[g.t])
    fnd.raise_if_any()
    for k, g in o.items():
        g.check(f"{what}: {k}")
        if not (n and k == "d_rows"):
            assert bool(torch.isfinite(g.t).all()), f"{what}: {k} holds a NaN or an infinity (an element not written?)"
    return o


def _reported(c, what, check, o, ref, pos=None):
    """check() holds o to float64 and raises at the first output that misses; the failure then names every output
    and element outside the tolerances (tests/step_report.py:tolerance_masks restates them) and where it came from."""
    try:
        check()
    except AssertionError as e:
        fnd = RP.Findings(what, c.B, c.F, c.Dn, pos=pos)
        fnd.note(f"[first assertion] {e}")
        got = _cpu(o)
        for k, m in RP.tolerance_masks(got, ref, pos).items():
            same_shape = ref[k].numel() == got[k].numel()
            fnd.add("outside the float64 tolerance (got / want)", k, m,
                    values=[got[k], ref[k].reshape(got[k].shape)] if same_shape else [got[k]])
        raise AssertionError(fnd.text()) from e


def _same_bits(c, a, b, what, keys=None, pos=None):
    """_assert_same_bits, and on a difference the place of every differing element of every output, both values."""
    try:
        _assert_same_bits(a, b, what, keys=keys)
    except AssertionError as e:
        fnd = RP.Findings(what, c.B, c.F, c.Dn, pos=pos)
        fnd.note(f"[first assertion] {e}")
        for k in keys or a:
            fnd.add("the two runs differ bit for bit (first / second)", k, _bits(a[k].t) != _bits(b[k].t),
                    values=[a[k].t, b[k].t])
            if not torch.equal(_bits(a[k].buf[:G]), _bits(b[k].buf[:G])) or \
                    not torch.equal(_bits(a[k].buf[-G:]), _bits(b[k].buf[-G:])):
                fnd.note(f"[guard band] {k}: the guard bands of the two runs differ")
        raise AssertionError(fnd.text()) from e


def _all_variants(c, ref, dev, name, recv, pos, n):
    """The four plain instantiations and the packed form (both row-load policies) of one case: float64, a second run,
    each other.  recv [n, 20] (device): the rows as a receive buffer in exchange order, pos [B, F] (host) their
    positions = the packed form's ids."""
    B, F = c.B, c.F
    first = None
    for sr, sd in POLICIES:
        what = f"{name} stream_rows {int(sr)} stream_d_rows {int(sd)}"
        o = _run(c, what, dev, sr, sd)
        _reported(c, what, lambda: _check_plain(o, ref, what), o, ref)
        _same_bits(c, _run(c, what, dev, sr, sd), o, what + ": second run")
        first = first or o
        _same_bits(c, o, first, what + ": against the default policies")
    # ---- the packed form
    m = SR.lin_masks(F)["mixed"] if F > 1 else None
    pos_dev = _dev(pos)
    used = torch.zeros(n, dtype=torch.bool, device="cuda")
    used[pos_dev.reshape(-1)] = True
    # step_ref.pack_ref's send buffer, of the addressed rows alone (in occurrence order)
    own = torch.arange(B * F).reshape(B, F)
    want_rows, want_gb, want_gl, _ = SR.unpack_ref(SR.pack_ref(ref["d_rows"], ref["dlogit"], own, B * F, m), own)
    packed = (recv, pos_dev, _dev(torch.zeros(F, dtype=I64)), n, _dev(m))
    for sr in (False, True):
        what = f"{name} packed stream_rows {int(sr)}"
        o = _run(c, what, dev, sr, False, packed)
        _reported(c, what, lambda: _check_small(o, ref, what), o, ref, pos)
        send = o["d_rows"].t
        got_rows, got_gb, got_gl, got_pad = SR.unpack_ref(send[pos_dev.reshape(-1)].cpu(), own)
        print(f"{what}: d_rows {_rel_err(got_rows, want_rows):.2e} g_bias {_rel_err(got_gb, want_gb):.2e} "
              f"g_lin {_rel_err(got_gl, want_gl):.2e}")

        def check_send():
            assert bool(torch.isfinite(got_rows).all() and torch.isfinite(got_gb).all() and
                        torch.isfinite(got_gl).all() and torch.isfinite(got_pad).all()), \
                f"{what}: an addressed row of the send buffer was not written"
            _close_grad(got_rows, want_rows, what=f"{what}: row gradients vs float64")
            _close_grad(got_gb, want_gb, what=f"{what}: column 16 (dlogit) vs float64")
            _close_grad(got_gl, want_gl, what=f"{what}: column 17 (dlogit * lin_field_mask) vs float64")
        _reported(c, what, check_send, o, ref, pos)
        assert bool((_bits(got_pad) == 0).all()), f"{what}: columns 18 / 19 of an addressed row are not +0.0"
        assert bool((_bits(send[~used]) == SENT_BITS).all()), f"{what}: a row nobody addresses was written"
        _same_bits(c, _run(c, what, dev, sr, False, packed), o, what + ": second run", pos=pos)
        _same_bits(c, o, first, what + ": against the plain form", keys=[k for k in o if k != "d_rows"])


DEV_KEYS = ("rows", "idx", "field_off", "dense", "y", "W0", "W1", "b0", "b1", "w_out", "w0_out", "lin_w_dense",
            "lin_w0")


@pytest.mark.parametrize("Dn", DENSE, ids=lambda v: f"Dn{v}")
@pytest.mark.parametrize("F", FIELDS, ids=lambda v: f"F{v}")
@pytest.mark.parametrize("B", BATCHES, ids=lambda v: f"B{v}")
def test_counted_waits_match_float64_and_repeat_bit_for_bit(hip_lib, B, F, Dn):
    c, ref = _case_ref(B, F, Dn)
    dev = {k: _dev(getattr(c, k)) for k in DEV_KEYS}
    name = f"B{B} F{F} Dn{Dn} T{min(_tiles_per_block(B))}..{max(_tiles_per_block(B))}"
    n = B * F + PACKED_SPARE
    pos = SR.packed_positions(B, F, n, seed=c.seed)
    recv = torch.full((n, 20), NAN)
    recv[pos.reshape(-1)] = c.rows[(c.idx + c.field_off).reshape(-1)]
    _all_variants(c, ref, dev, name, _dev(recv), pos, n)


# ------------------------------------------------------------------------------------------- rows that come from HBM
@pytest.fixture(scope="module")
def hbm_table(hip_lib):
    """HBM_ROWS fused rows of 20 floats, generated on the device (seeded): N(0, SCALE) cut at two sigma as
    oracle/th_layers.py:make_params draws, columns 18 / 19 poisoned with NaN as tests/step_ref.py:fuse_rows does.
    Built once for the module and released behind its last test."""
    g = torch.Generator(device="cuda").manual_seed(20240)
    t = torch.empty(HBM_ROWS, 20, dtype=F32, device="cuda")
    t.normal_(0.0, SCALE, generator=g).clamp_(-2 * SCALE, 2 * SCALE)
    t[:, SR.COLS:] = NAN
    assert t.numel() * 4 > LLC_BYTES
    yield t
    _hbm_case_ref.cache_clear()
    del t
    torch.cuda.empty_cache()


_HBM = {}  # the fixture's table, for the cached case builder below


@functools.lru_cache(maxsize=2)
def _hbm_case_ref(B, F, Dn):
    """A case whose ids are drawn uniformly over each field's whole share (HBM_ROWS // F rows) of the device table.
    The float64 reference is built from the device's own bits: the touched rows alone are copied to the host as a
    compacted table, the ids renumbered into it.  c.idx / c.field_off address the compacted host table, c.idx_table /
    field_off_table the device table."""
    table = _HBM["table"]
    n = B + B // 2
    seed = 900 + 7 * F + Dn
    per = HBM_ROWS // F
    spec, p, _, dense, y, _ = make_case("deepfm", B=n, F=F, D=SR.D, Dn=Dn, sizes=[1] * F, hidden=(32, 32),
                                        seed=seed, scale=SCALE)
    lin_w_dense = SR.fuse_rows(p, spec, 20)[2]
    idx = torch.randint(0, per, (n, F), generator=torch.Generator().manual_seed(seed))
    field_off = torch.arange(F, dtype=I64) * per
    assert int(field_off[-1]) + per <= HBM_ROWS and per * F * 80 > LLC_BYTES
    assert int(idx.max()) > 0.9 * per and int(idx.min()) < 0.1 * per  # the whole range (n >= 120 draws per field)
    uniq, inv = torch.unique((idx + field_off).reshape(-1), return_inverse=True)
    rows = table[uniq.cuda()].cpu()
    c, ref = _finish_case(B, F, Dn, seed, rows, inv.reshape(n, F), torch.zeros(F, dtype=I64), dense, y, p, lin_w_dense,
                          idx_table=idx)
    c.field_off_table = field_off
    return c, ref


@pytest.mark.parametrize("Dn", DENSE, ids=lambda v: f"Dn{v}")
@pytest.mark.parametrize("F", HBM_FIELDS, ids=lambda v: f"F{v}")
@pytest.mark.parametrize("B", HBM_BATCHES, ids=lambda v: f"B{v}")
def test_counted_waits_with_rows_from_hbm(hbm_table, B, F, Dn):
    """The same kernel, references, tolerances, bit-for-bit rules and variants as above on a table (and, packed, on
    exchange buffers) of 336 MB: B = 12,293 is three or four tiles per block with a ragged last tile, B = 80 one tile
    per block - a fill and a drain only."""
    _HBM["table"] = hbm_table
    c, ref = _hbm_case_ref(B, F, Dn)
    T = _tiles_per_block(B)
    assert (min(T), max(T)) == ((3, 4) if B > 80 else (1, 1))
    dev = {k: _dev(getattr(c, k)) for k in DEV_KEYS if k not in ("rows", "idx", "field_off")}
    dev.update(rows=hbm_table, idx=_dev(c.idx_table), field_off=_dev(c.field_off_table))
    name = f"HBM B{B} F{F} Dn{Dn} T{min(T)}..{max(T)}"
    # the packed form: a receive buffer of the table's size, the occurrences' rows spread all over it
    n = HBM_ROWS
    pos = SR.packed_positions(B, F, n, seed=c.seed)
    recv = torch.full((n, 20), NAN, device="cuda")
    recv[_dev(pos.reshape(-1))] = hbm_table[_dev((c.idx_table + c.field_off_table).reshape(-1))]
    _all_variants(c, ref, dev, name, recv, pos, n)
