"""CPU: tests/graph_replay.py - the ledger of which entry points a captured step is known to contain, and the batch
permutation."""
import glob
import os

import torch

from tests.graph_replay import CASES, NOT_IN_A_STEP, PENDING, permuted_batch, permuted_csr
from tests.test_gpu_stale_lds import _stream_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_stream_entry_points():
    """Every entry point declared with an rm_stream_t stream argument, in every header under include/."""
    headers = sorted(os.path.basename(h) for h in glob.glob(os.path.join(ROOT, "include", "recman_hip*.h")))
    assert len(headers) >= 4 and "recman_hip.h" in headers
    per_header = {h: _stream_entry_points(h) for h in headers}
    assert all(per_header.values()), "a header declares no entry point with a stream"
    return set().union(*per_header.values())


def test_every_engine_has_a_case():
    from recman_amd import engine

    assert {row.engine for row in CASES.values()} == set(engine.ENGINES)
    assert all(len(row.case) > 10 for row in CASES.values())


def test_every_stream_entry_point_is_claimed_explained_or_pending():
    entries = _all_stream_entry_points()
    assert _stream_entry_points() < entries  # the later headers declare streams too
    claimed = set().union(*(row.claims for row in CASES.values() if row.claims is not None))
    groups = {"claimed by a case": claimed, "NOT_IN_A_STEP": set(NOT_IN_A_STEP), "PENDING": set(PENDING)}
    names = sorted(groups)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not groups[a] & groups[b], f"both {a} and {b}: {sorted(groups[a] & groups[b])}"
    union = claimed | set(NOT_IN_A_STEP) | set(PENDING)
    assert union == entries, sorted(union ^ entries)
    assert all(len(why) > 20 for why in NOT_IN_A_STEP.values())
    # a pending entry names rows that exist and whose capture has not been observed
    for entry, rows in PENDING.items():
        assert rows and all(r in CASES and CASES[r].claims is None for r in rows), entry
    # ... and every unobserved row is named by one
    unobserved = {n for n, row in CASES.items() if row.claims is None}
    assert unobserved == {r for rows in PENDING.values() for r in rows}
    # the route flags of the three DeepFM rows
    assert "rm_embed_mlp_fwd" in CASES["deepfm_front"].claims and "rm_embed_fwd" not in CASES["deepfm_front"].claims
    assert {"rm_embed_fwd", "rm_mlp_fwd"} <= CASES["deepfm_chain"].claims
    assert "rm_embed_mlp_fwd" not in CASES["deepfm_chain"].claims
    assert "rm_rank_loss" in CASES["deepfm_rank_pairwise"].claims


def _csr_example():
    """Five examples: an empty history, one item, a full-length one (max_len 4), two items, empty again."""
    lengths = [0, 1, 4, 2, 0]
    offsets = torch.tensor([0, 0, 1, 5, 7, 7])
    ids = torch.tensor([10, 20, 21, 22, 23, 30, 31])
    vals = ids.float() / 10
    return lengths, offsets, ids, vals


def test_permuted_csr_keeps_every_example_whole():
    lengths, offsets, ids, vals = _csr_example()
    off2, ids2, vals2 = permuted_csr(offsets, ids, vals)
    assert off2.shape == offsets.shape and off2.dtype == offsets.dtype and ids2.shape == ids.shape
    assert (off2[1:] - off2[:-1]).tolist() == lengths[::-1]            # the lengths are reversed
    assert int(off2[0]) == 0 and int(off2[-1]) == int(offsets[-1]) == 7   # the total nnz is unchanged
    B = len(lengths)
    for b in range(B):                                                   # the ids of every example are intact
        old = ids[offsets[b]: offsets[b + 1]].tolist()
        new = ids2[off2[B - 1 - b]: off2[B - b]].tolist()
        assert new == old, (b, old, new)
    assert torch.equal(vals2, ids2.float() / 10)                         # values travel with their ids
    assert ids2.tolist() == [30, 31, 20, 21, 22, 23, 10]
    # twice is the identity
    off3, ids3 = permuted_csr(off2, ids2)
    assert torch.equal(off3, offsets) and torch.equal(ids3, ids)


def test_permuted_batch_flips_every_input_and_draws_nothing():
    lengths, offsets, ids, vals = _csr_example()
    B = len(lengths)
    idx = torch.arange(B * 3).view(B, 3)
    dense = torch.arange(B * 2, dtype=torch.float32).view(B, 2)
    Y = torch.arange(B * 2, dtype=torch.float32).view(B, 2)
    masks = {"dnn": [torch.arange(B * 4).view(B, 4).float(), None], "fm": (None, torch.arange(B).float())}
    mv = {"hist": (offsets, ids), "val": (torch.arange(B + 1), torch.arange(B) + 100, torch.arange(B).float())}
    state = torch.get_rng_state()
    idx2, dense2, Y2, masks2, mv2 = permuted_batch(idx, dense, Y, masks, mv)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(idx2, idx.flip(0)) and torch.equal(dense2, dense.flip(0)) and torch.equal(Y2, Y.flip(0))
    assert torch.equal(masks2["dnn"][0], masks["dnn"][0].flip(0)) and masks2["dnn"][1] is None
    assert isinstance(masks2["fm"], tuple) and torch.equal(masks2["fm"][1], masks["fm"][1].flip(0))
    assert (mv2["hist"][0][1:] - mv2["hist"][0][:-1]).tolist() == lengths[::-1]
    assert torch.equal(mv2["val"][0], torch.arange(B + 1))               # one id per example: the offsets stay
    assert torch.equal(mv2["val"][1], (torch.arange(B) + 100).flip(0))
    assert torch.equal(mv2["val"][2], torch.arange(B).float().flip(0))
    assert all(t.is_contiguous() for t in (idx2, dense2, Y2))
    # nothing of the original was changed, and absent inputs stay absent
    assert torch.equal(idx, torch.arange(B * 3).view(B, 3)) and torch.equal(ids, _csr_example()[2])
    assert permuted_batch(idx, dense, None)[2:] == (None, None, None)
