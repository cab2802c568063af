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
 * about 1,000 rows per field, so that a tile's rows are not all the same few cache lines.

Every case is held to the float64 reference of tests/step_ref.py with the tolerances of tests/test_gpu_step_kernel.py
(logit / pred 1e-5 absolute, loss _close's defaults, dlogit, d_rows and every parameter gradient _close_grad's 2e-5),
and every variant is run twice and must repeat itself bit for bit - outputs and guard bands: a wait that is too short
shows as a difference between runs long before it shows as a tolerance failure.  The cache policies change no
arithmetic, so the four plain variants must agree bit for bit with each other as well.
"""
import functools
import types

import pytest
import torch

from tests import step_ref as SR
from tests.cases import make_case
from tests.test_gpu_parity import _close_grad
from tests.test_gpu_step_kernel import (F32, I64, NAN, SENT, SENT_BITS, Guarded, _assert_same_bits, _bits,
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


@functools.lru_cache(maxsize=2)
def _case_ref(B, F, Dn):
    """tests/step_ref.py:make_step_case with VOCAB rows per field (its generators, scales and kink rule), and the
    float64 reference: built once per shape and shared by the variants, read-only."""
    n = B + B // 2
    seed = 600 + 7 * F + Dn
    spec, p, idx, dense, y, _ = make_case("deepfm", B=n, F=F, D=SR.D, Dn=Dn, sizes=[VOCAB] * F, hidden=(32, 32),
                                          seed=seed, scale=SCALE)
    rows, field_off, lin_w_dense = SR.fuse_rows(p, spec, 20)
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
        w0_out=p["dnn_w0"], lin_w_dense=lin_w_dense if Dn else None, lin_w0=p["linear_w0"])
    ref = SR.ref_of(c)
    assert float(ref["logit"].abs().max()) < LOGIT_MAX
    return c, ref


def _run(c, what, dev, stream_rows=False, stream_d_rows=False, packed=None):
    """One call of ops.deepfm_step on the device tensors `dev` of case c; packed = (rows, idx, field_off, n, mask).
    Outputs in guard bands, pre-filled with NaN (the send buffer: with the sentinel), as in test_gpu_step_kernel."""
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
    for k, g in o.items():
        g.check(f"{what}: {k}")
        if not (n and k == "d_rows"):
            assert bool(torch.isfinite(g.t).all()), f"{what}: {k} holds a NaN or an infinity (an element not written?)"
    return o


@pytest.mark.parametrize("Dn", DENSE, ids=lambda v: f"Dn{v}")
@pytest.mark.parametrize("F", FIELDS, ids=lambda v: f"F{v}")
@pytest.mark.parametrize("B", BATCHES, ids=lambda v: f"B{v}")
def test_counted_waits_match_float64_and_repeat_bit_for_bit(hip_lib, B, F, Dn):
    c, ref = _case_ref(B, F, Dn)
    dev = {k: _dev(getattr(c, k)) for k in ("rows", "idx", "field_off", "dense", "y", "W0", "W1", "b0", "b1", "w_out",
                                            "w0_out", "lin_w_dense", "lin_w0")}
    name = f"B{B} F{F} Dn{Dn} T{min(_tiles_per_block(B))}..{max(_tiles_per_block(B))}"
    # ---- the four plain instantiations: float64, a second run, each other
    first = None
    for sr, sd in POLICIES:
        what = f"{name} stream_rows {int(sr)} stream_d_rows {int(sd)}"
        o = _run(c, what, dev, sr, sd)
        _check_plain(o, ref, what)
        _assert_same_bits(_run(c, what, dev, sr, sd), o, what + ": second run")
        first = first or o
        _assert_same_bits(o, first, what + ": against the default policies")
    # ---- the packed form (both row-load policies): the rows as a receive buffer in exchange order, ids = positions
    n = B * F + PACKED_SPARE
    pos = SR.packed_positions(B, F, n, seed=c.seed)
    m = SR.lin_masks(F)["mixed"] if F > 1 else None
    recv = torch.full((n, 20), NAN)
    recv[pos.reshape(-1)] = c.rows[(c.idx + c.field_off).reshape(-1)]
    used = torch.zeros(n, dtype=torch.bool)
    used[pos.reshape(-1)] = True
    want = SR.pack_ref(ref["d_rows"], ref["dlogit"], pos, n, m)
    want_rows, want_gb, want_gl, _ = SR.unpack_ref(want, pos)
    packed = (_dev(recv), _dev(pos), _dev(torch.zeros(F, dtype=I64)), n, _dev(m))
    for sr in (False, True):
        what = f"{name} packed stream_rows {int(sr)}"
        o = _run(c, what, dev, sr, False, packed)
        _check_small(o, ref, what)
        send = o["d_rows"].t.cpu()
        got_rows, got_gb, got_gl, got_pad = SR.unpack_ref(send, pos)
        print(f"{what}: d_rows {_rel_err(got_rows, want_rows):.2e} g_bias {_rel_err(got_gb, want_gb):.2e} "
              f"g_lin {_rel_err(got_gl, want_gl):.2e}")
        assert bool(torch.isfinite(send[used]).all()), f"{what}: an addressed row of the send buffer was not written"
        _close_grad(got_rows, want_rows, what=f"{what}: row gradients vs float64")
        _close_grad(got_gb, want_gb, what=f"{what}: column 16 (dlogit) vs float64")
        _close_grad(got_gl, want_gl, what=f"{what}: column 17 (dlogit * lin_field_mask) vs float64")
        assert bool((_bits(got_pad) == 0).all()), f"{what}: columns 18 / 19 of an addressed row are not +0.0"
        assert bool((_bits(send[~used]) == SENT_BITS).all()), f"{what}: a row nobody addresses was written"
        _assert_same_bits(_run(c, what, dev, sr, False, packed), o, what + ": second run")
        _assert_same_bits(o, first, what + ": against the plain form", keys=[k for k in o if k != "d_rows"])
