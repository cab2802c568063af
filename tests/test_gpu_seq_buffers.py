"""GPU: the engine's one buffer policy for the sequence pooling units (Engine._seq_fwd / _seq_bwd).  One engine takes
four batches in a row - a small one, one whose histories are all at max_len (more occurrences: the field's buffers are
reallocated), a single example, and one without any history (nnz = 0) - and after each of them everything the unit
produced equals, bit for bit, what a FRESH engine with the same parameters produces for that batch alone: buffers that
are reused or regrown and the remembered CSR leak nothing from one batch into the next.  (Correctness against float64:
tests/test_gpu_din_model.py, test_gpu_bst_model.py, test_gpu_dien_model.py.)"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64

D, MAX_LEN, SEED = 8, 6, 11
NAMES, SIZES, DENSE = ["C0", "item", "hist", "C2"], [7, 11, 0, 5], ["I0", "I1"]
F_HIST = NAMES.index("hist")
HP = dict(deep_hidden_units=(8, 8), att_hidden_units=(8,), att_head_num=2, att_ffn_units=8)
PREFIX = {"din": "hist_asp_", "transformer": "hist_bst_", "dien": "hist_dien_"}
LENGTHS = ([0, 1, 2, 3, 1], [MAX_LEN] * 5, [1], [0, 0, 0])


@functools.lru_cache(maxsize=None)
def _batches():
    """(idx, dense, y, mv) per entry of LENGTHS, on the host: computed once, shared and left unchanged."""
    g = torch.Generator().manual_seed(SEED)
    out = []
    for lens in LENGTHS:
        B = len(lens)
        idx = torch.stack([torch.randint(0, v, (B,), generator=g) if v else torch.zeros(B, dtype=I64) for v in SIZES], 1)
        offsets = torch.tensor([0] + lens, dtype=I64).cumsum(0)
        ids = torch.randint(0, SIZES[1], (sum(lens),), generator=g)
        dense = torch.randn(B, len(DENSE), generator=g)
        y = torch.randint(0, 2, (B,), generator=g)
        out.append((idx, dense, y, {"hist": (offsets, ids)}))
    return out


def _engine(kind):
    from recman_amd import engine as eng

    spec = eng.FeatureSpec(NAMES, SIZES, DENSE, seq_query={"hist": "item"}, seq_max_len={"hist": MAX_LEN})
    e = eng.DINEngine(spec, D, dict(HP, seq_pooling=kind))
    eng.init_reference(e, SEED)
    return e


def _step(e, batch):
    """One fwd_bwd -> {name: a copy of everything the comparison covers}."""
    idx, dense, y, mv = batch
    loss = e.fwd_bwd(idx.cuda(), dense.cuda(), y.cuda(), mv={n: (o.cuda(), i.cuda()) for n, (o, i) in mv.items()})
    torch.cuda.synchronize()
    fq, ids, d_keys = e.seq_key_grads(F_HIST)
    assert fq == NAMES.index("item") and torch.equal(ids.cpu(), mv["hist"][1])
    assert d_keys.shape == (int(mv["hist"][1].shape[0]), D)
    got = {"loss": loss, "d_rows": e.d_rows, "d_keys": d_keys}
    got.update({n: t for n, t in e.grads.items() if n.startswith("hist_")})
    return {n: t.detach().clone() for n, t in got.items()}


@pytest.mark.parametrize("kind", sorted(PREFIX))
def test_reused_and_regrown_buffers_leak_nothing_between_batches(hip_lib, kind):
    e = _engine(kind)
    unit_vars = sorted(n for n in e.grads if n.startswith("hist_"))
    assert unit_vars and all(n.startswith(PREFIX[kind]) for n in unit_vars)
    caps = []
    for k, batch in enumerate(_batches()):
        got = _step(e, batch)
        caps.append(e._seq_buf[F_HIST]["cap"])
        fresh = _engine(kind)
        for n in e.params:
            assert torch.equal(e.params[n], fresh.params[n]), n  # the same parameters
        want = _step(fresh, batch)
        assert set(got) == set(want) == {"loss", "d_rows", "d_keys", *unit_vars}
        for n in sorted(want):
            assert got[n].shape == want[n].shape and bool(torch.isfinite(got[n]).all()), (kind, k, n)
            assert torch.equal(got[n].view(torch.int32), want[n].view(torch.int32)), (kind, k, n)
    # the second batch outgrew the first one's buffers; the smaller ones after it reused them
    assert caps == [sum(LENGTHS[0]), 5 * MAX_LEN, 5 * MAX_LEN, 5 * MAX_LEN]
