"""GPU: rm_deepfm_step (csrc/step.hip) must not depend on what an earlier kernel left in LDS.

The step reads LDS images that it fills itself - by row DMAs behind counted waits, by the head's ds_writes, by the
workers' zero image.  A read that runs ahead of its fill sees whatever the CU's LDS held before the launch; the
kernel's one known race of that kind showed as a flicker, because that content changes from run to run.  Here it is
made ONE known pattern first: rm_debug_lds_fill writes every word of every CU's LDS (as far as the step allocates
it) right in front of the step, once with a quiet NaN (0x7fc00000: any use of a stale word poisons an output) and once
with zero.  Each of the two runs is held to the float64 reference and the tolerances of
tests/test_gpu_step_waits.py (its case builders, its runner, tests/step_report.py's report), and the two must agree
bit for bit: a stale word that happens to stay inside the tolerance still differs between NaN and zero.

Shapes (about 1,000 rows per field): B = 80 (five blocks of one tile: fill and drain only), 16 * 256 * 3 + 5 (the
fill and a ragged tile) and 16 * 256 * 7 - seven tiles per block, the smallest length at which every ring buffer is
overwritten twice by a DMA that stands behind a counted LDS wait (lds_load's comment in csrc/step.hip); F = 26, 7, 1
and Dn = 13, 0 as in tests/test_gpu_step_waits.py; the unpacked default policies and the packed form.
"""
import pytest
import torch

from tests import step_ref as SR
from tests.test_gpu_parity import _close_grad
from tests.test_gpu_step_kernel import I64, NAN, SENT_BITS, _bits, _check_plain, _check_small, _dev
from tests.test_gpu_step_waits import (DEV_KEYS, DENSE, FIELDS, PACKED_SPARE, _case_ref, _reported, _run, _same_bits,
                                       _tiles_per_block)

pytestmark = pytest.mark.gpu

QNAN, ZERO = 0x7FC00000, 0
BATCHES = (80, 16 * 256 * 3 + 5, 16 * 256 * 7)


def test_the_batches_are_a_fill_a_ragged_tile_and_a_ring_that_wraps_twice():
    T = {B: _tiles_per_block(B) for B in BATCHES}
    assert set(T[80]) == {1} and len(T[80]) == 5
    assert BATCHES[1] % 16 == 5 and T[BATCHES[1]][0] == 4 and set(T[BATCHES[1]][1:]) == {3}
    assert set(T[BATCHES[2]]) == {7} and len(T[BATCHES[2]]) == 256
    # tile t lands in ring buffer t % 3, and tiles t >= 3 are requested in a segment that runs a backward, i.e. by a
    # DMA behind a counted LDS wait that has reads to wait for: buffer 0 gets tiles 0 3 6, buffer 1 1 4, buffer 2 2 5
    assert [[t for t in range(7) if t % 3 == r] for r in range(3)] == [[0, 3, 6], [1, 4], [2, 5]]


@pytest.fixture
def filled_step(monkeypatch, hip_lib):
    """ops.deepfm_step with the LDS fill enqueued directly in front of it (same stream); the pattern is set by the
    test between runs."""
    from recman_amd import ops

    state = {"pattern": None, "fills": 0}
    step = ops.deepfm_step

    def filled(*a, **k):
        ops.debug_lds_fill(state["pattern"])
        state["fills"] += 1
        return step(*a, **k)

    monkeypatch.setattr(ops, "deepfm_step", filled)
    return state


def _check_send(c, ref, o, what, pos, pos_dev, n, m):
    """The packed form's send buffer against float64, as tests/test_gpu_step_waits.py:_all_variants holds it."""
    B, F = c.B, c.F
    own = torch.arange(B * F).reshape(B, F)
    want_rows, want_gb, want_gl, _ = SR.unpack_ref(SR.pack_ref(ref["d_rows"], ref["dlogit"], own, B * F, m), own)
    send = o["d_rows"].t
    got_rows, got_gb, got_gl, got_pad = SR.unpack_ref(send[pos_dev.reshape(-1)].cpu(), own)

    def check():
        assert bool(torch.isfinite(got_rows).all() and torch.isfinite(got_gb).all() and
                    torch.isfinite(got_gl).all() and torch.isfinite(got_pad).all()), \
            f"{what}: an addressed row of the send buffer was not written"
        _close_grad(got_rows, want_rows, what=f"{what}: row gradients vs float64")
        _close_grad(got_gb, want_gb, what=f"{what}: column 16 (dlogit) vs float64")
        _close_grad(got_gl, want_gl, what=f"{what}: column 17 (dlogit * lin_field_mask) vs float64")
    _reported(c, what, check, o, ref, pos)
    assert bool((_bits(got_pad) == 0).all()), f"{what}: columns 18 / 19 of an addressed row are not +0.0"
    used = torch.zeros(n, dtype=torch.bool, device="cuda")
    used[pos_dev.reshape(-1)] = True
    assert bool((_bits(send[~used]) == SENT_BITS).all()), f"{what}: a row nobody addresses was written"


@pytest.mark.parametrize("Dn", DENSE, ids=lambda v: f"Dn{v}")
@pytest.mark.parametrize("F", FIELDS, ids=lambda v: f"F{v}")
@pytest.mark.parametrize("B", BATCHES, ids=lambda v: f"B{v}")
def test_step_does_not_depend_on_what_lds_held(filled_step, B, F, Dn):
    c, ref = _case_ref(B, F, Dn)
    dev = {k: _dev(getattr(c, k)) for k in DEV_KEYS}
    T = _tiles_per_block(B)
    name = f"stale LDS B{B} F{F} Dn{Dn} T{min(T)}..{max(T)}"
    # ---- the unpacked form, default policies
    runs = {}
    for pattern in (QNAN, ZERO):
        filled_step["pattern"] = pattern
        what = f"{name} LDS filled with {pattern:#010x}"
        o = runs[pattern] = _run(c, what, dev)
        _reported(c, what, lambda: _check_plain(o, ref, what), o, ref)
    _same_bits(c, runs[QNAN], runs[ZERO], f"{name}: LDS filled with a quiet NaN against LDS filled with zero")
    # ---- the packed form
    n = B * F + PACKED_SPARE
    pos = SR.packed_positions(B, F, n, seed=c.seed)
    recv = torch.full((n, 20), NAN)
    recv[pos.reshape(-1)] = c.rows[(c.idx + c.field_off).reshape(-1)]
    m = SR.lin_masks(F)["mixed"] if F > 1 else None
    pos_dev = _dev(pos)
    packed = (_dev(recv), pos_dev, _dev(torch.zeros(F, dtype=I64)), n, _dev(m))
    runs = {}
    for pattern in (QNAN, ZERO):
        filled_step["pattern"] = pattern
        what = f"{name} packed, LDS filled with {pattern:#010x}"
        o = runs[pattern] = _run(c, what, dev, False, False, packed)
        _reported(c, what, lambda: _check_small(o, ref, what), o, ref, pos)
        _check_send(c, ref, o, what, pos, pos_dev, n, m)
    _same_bits(c, runs[QNAN], runs[ZERO], f"{name} packed: LDS filled with a quiet NaN against LDS filled with zero",
               pos=pos)
    assert filled_step["fills"] == 4
