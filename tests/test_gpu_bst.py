"""GPU: rm_bst_fwd / rm_bst_bwd through the C ABI (recman_amd.ops) against the float64 restatement + autograd
(tests/bst_ref.py, pinned on the CPU by tests/test_bst_host.py).

Tolerance, the convention of tests/test_gpu_asp.py: for every output (pooled rows, key gradients, query gradient, each
of the 17 parameter gradients) the gradient measure of tests/test_gpu_parity.py must be <= max(2e-5, 4 x the float32
CPU restatement's own measure on the case); both numbers are printed.  The yardstick is the float32 restatement, never
the kernel.

d_bk is analytically zero (the key bias shifts every score of a query alike, and the softmax removes the shift): float64
itself returns a 1e-17 residue, so a relative measure against it means nothing.  There the measure is, per column,
|d_bk| / the sum over the tokens of |dLoss/dK_token| - the terms whose sum cancels, the scale dw0 is judged against in
tests/test_gpu_asp.py - under the same bound: max(2e-5, 4 x the float32 CPU restatement's own ratio).  (With wq x 4000
a score of 1e4 carries an absolute rounding error of 1e-3, so a softmax weight and with it the residue is only good to
that: the float32 CPU restatement leaves 2.8e-4 of the scale on d8_h2_f128_short.)

Kink guard: the pooled rows' gradient is zero for every example with an FFN unit within 1e-6 of its kink in float64
(same gradient for kernel and reference; the cap of 20 % per case is asserted on the CPU)."""
import functools

import pytest
import torch

from tests import bst_ref as R

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64
ROW0 = 5  # the key block starts behind a few foreign rows of the table


@functools.lru_cache(maxsize=None)
def _case(name, wq_scale=1.0):
    """(case, float64 reference, float32 CPU reference): computed once, shared and left unchanged."""
    case = R.make_bst_case(**R.GPU_CASES[name], wq_scale=wq_scale)
    return case, R.layer_reference(case), R.layer_reference(case, dtype=F32)


def _dev(t):
    return t.to(F32).cuda().contiguous()


def _table(case):
    """The fused table on the GPU: ROW0 rows of another feature, then the case's block."""
    g = torch.Generator().manual_seed(3)
    junk = torch.randn(ROW0, case["table"].shape[1], generator=g)
    return torch.cat([junk, case["table"].float()]).cuda().contiguous()


def _run(case, backward=True):
    """The kernels on a case: (out [B, LD], d_keys, d_query, {name: gradient})."""
    from recman_amd import ops

    B, D, heads, Hf, ML = case["B"], case["D"], case["heads"], case["Hf"], case["max_len"]
    rows = _table(case)
    LD = rows.shape[1]
    offsets, ids = case["offsets"].cuda(), case["ids"].cuda()
    qrow = (case["qidx"] + ROW0).cuda()
    nnz = int(ids.shape[0])
    p = {n: _dev(v) for n, v in case["p"].items()}
    out = torch.full((B, LD), float("nan"), device="cuda")
    ws = torch.empty(max(4, ops.bst_workspace(D, heads, Hf, ML, B, True)), device="cuda")
    ops.bst_fwd(rows, ROW0, D, offsets, ids, qrow, p, heads, ML, out, ws)
    if not backward:
        torch.cuda.synchronize()
        return (out,)
    # the pooled rows' gradient and the query gradient are columns of a wider [B, F, D] buffer, as in the engine
    wide = torch.zeros(B, 3, D, device="cuda")
    wide[:, 2, :] = _dev(case["g"])
    wide[:, 0, :] = _dev(case["dq_up"])
    d_keys = torch.full((nnz, D), float("nan"), device="cuda")
    grads = {n: torch.full_like(v, float("nan")) for n, v in p.items()}
    ops.bst_bwd(rows, ROW0, D, offsets, ids, qrow, p, heads, ML, wide[:, 2, :], d_keys, wide[:, 0, :], grads, ws)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, 2, :], _dev(case["g"])) and float(wide[:, 1, :].abs().max()) == 0.0
    return out, d_keys, wide[:, 0, :].clone(), grads


def _flat(res):
    """(name, tensor) pairs of a result tuple of _run / layer_reference."""
    out, d_keys, d_query, grads = res
    return [("out", out), ("d_keys", d_keys), ("d_query", d_query)] + [("d_" + n, grads[n]) for n in R.NAMES]


def _check(case, want, cpu32, tag):
    res = _run(case)
    D = case["D"]
    assert float(res[0][:, D:].abs().max()) == 0.0, f"{tag}: the pooled row must be zero behind column D"
    got = _flat((res[0][:, :D],) + res[1:])
    bad = []
    for (name, a), (_, wnt), (_, c32) in zip(got, _flat(want), _flat(cpu32)):
        assert bool(torch.isfinite(a).all()), f"{tag}: {name} is not finite"
        if name == "d_bk":
            scale = R.key_grad_abs_sum(case)
            r, r32 = float((a.cpu().double().abs() / scale).max()), float((c32.abs() / scale).max())
            bound = max(2e-5, 4 * r32)
            print(f"{tag}: d_bk / sum |dK| {r:.2e}, float32 CPU {r32:.2e}, bound {bound:.2e}")
            if not r <= bound:
                bad.append(f"d_bk {r:.3e} of sum |dK| > {bound:.3e} (float32 CPU {r32:.3e})")
            continue
        m, m32 = R.grad_measure(a, wnt.reshape(a.shape)), R.grad_measure(c32, wnt)
        bound = max(2e-5, 4 * m32)
        print(f"{tag}: {name} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        if not m <= bound:
            bad.append(f"{name} measure {m:.3e} > {bound:.3e} (float32 CPU {m32:.3e})")
    assert not bad, f"{tag}: " + "; ".join(bad)
    return res


@pytest.mark.parametrize("name", sorted(R.GPU_CASES))
def test_bst_kernels_match_float64(hip_lib, name):
    case, want, cpu32 = _case(name)
    n = case["offsets"][1:] - case["offsets"][:-1]
    assert int(n[0]) == 0 and int(n[1]) == 1 and int(n[2]) == case["max_len"] and case["B"] % 32 != 0
    ids = case["ids"][int(case["offsets"][2]): int(case["offsets"][3])]
    assert case["max_len"] < 2 or int(ids[0]) == int(ids[1])  # a repeated id in the longest history
    res = _check(case, want, cpu32, name)
    # an example without history is ONE token: Z_0 of the candidate, not zero
    assert float(res[0][0, : case["D"]].abs().max()) > 0


@pytest.mark.parametrize("name", R.RANGE_CASES)
def test_large_scores_under_the_softmax(hip_lib, name):
    case, want, cpu32 = _case(name, R.RANGE_SCALE)
    _check(case, want, cpu32, name + " wq x" + str(R.RANGE_SCALE))


@pytest.mark.parametrize("name", ["d16_grid_stride", "d32_h8_f128", "d16_h4_f20", "d8_h2_f128_short"])
def test_two_runs_are_bit_equal(hip_lib, name):
    case = _case(name)[0]
    a, b = _flat(_run(case)), _flat(_run(case))
    for (nm, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), nm


@pytest.mark.parametrize("name", ["d16_h2_f64", "d8_h1_f32_full", "d32_h8_f128"])
def test_inference_rows_are_the_training_rows_bit_for_bit(hip_lib, name):
    case = _case(name)[0]
    assert torch.equal(_run(case, backward=False)[0], _run(case)[0])


def test_query_gradient_is_added_onto_what_the_buffer_holds(hip_lib):
    case = _case("d16_h2_f64")[0]
    zero = dict(case, dq_up=torch.zeros_like(case["dq_up"]))
    with_up, plain = _run(case)[2], _run(zero)[2]
    assert float(plain.abs().max()) > 0
    want = plain.cpu().double() + case["dq_up"]
    assert float((with_up.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert float((with_up - plain).abs().max()) > 1e-3


def test_all_examples_without_history(hip_lib):
    case = _case("d8_h2_f128_short")[0]
    B, D = case["B"], case["D"]
    case = dict(case, offsets=torch.zeros(B + 1, dtype=I64), ids=torch.zeros(0, dtype=I64))
    want, cpu32 = R.layer_reference(case), R.layer_reference(case, dtype=F32)
    out, d_keys, d_query, grads = _run(case)
    assert d_keys.shape == (0, D)
    got = _flat((out[:, :D], d_keys, d_query, grads))
    for (name, a), (_, wnt), (_, c32) in zip(got, _flat(want), _flat(cpu32)):
        assert bool(torch.isfinite(a).all()), name
        # (one token per example: its softmax weight is 1, so d_wq, d_wk, d_bq and d_bk are exactly zero on both sides)
        m, m32 = R.grad_measure(a, wnt.reshape(a.shape)), R.grad_measure(c32, wnt)
        print(f"no history: {name} measure {m:.2e}, float32 CPU {m32:.2e}")
        assert m <= max(2e-5, 4 * m32), (name, m, m32)
    assert float(out[:, :D].abs().max()) > 0  # every T = 1: Z_0, not zero
    # only P[0] is ever used
    assert float(grads["pos"][1:].abs().max()) == 0.0 and float(grads["pos"][0].abs().max()) > 0


def test_a_history_longer_than_max_len_keeps_its_last_items_and_zeroes_the_rest(hip_lib):
    """A caller error made safe: example 2 (the longest) gets 3 more items in FRONT; the kernels use its last max_len
    items, so every output equals the unchanged case's, and the d_keys rows of the 3 cut occurrences are zero."""
    case = _case("d16_h2_f64")[0]
    s = int(case["offsets"][2])
    extra = torch.tensor([1, 2, 3])
    long = dict(case, ids=torch.cat([case["ids"][:s], extra, case["ids"][s:]]),
                offsets=torch.cat([case["offsets"][:3], case["offsets"][3:] + 3]))
    a, b = _run(case), _run(long)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    keep = torch.ones(long["ids"].shape[0], dtype=torch.bool)
    keep[s: s + 3] = False
    assert torch.equal(b[1][keep.cuda()], a[1]) and float(b[1][~keep.cuda()].abs().max()) == 0.0
    for n in R.NAMES:
        assert torch.equal(a[3][n], b[3][n]), n


def test_an_empty_batch_gives_zero_parameter_gradients(hip_lib):
    from recman_amd import ops

    D, heads, Hf, ML = 16, 2, 64, 10
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    p = {n: z(*s) for n, s in ops.bst_param_shapes(D, Hf, ML).items()}
    grads = {n: torch.full_like(v, float("nan")) for n, v in p.items()}
    e64 = torch.zeros(0, dtype=I64, device="cuda")
    ws = torch.empty(max(4, ops.bst_workspace(D, heads, Hf, ML, 0, True)), device="cuda")
    ops.bst_bwd(z(6, 2 * D), 0, D, torch.zeros(1, dtype=I64, device="cuda"), e64, e64, p, heads, ML, z(0, D), z(0, D),
                z(0, D), grads, ws)
    torch.cuda.synchronize()
    for n, t in grads.items():
        assert float(t.abs().max()) == 0.0, n


@pytest.mark.parametrize("D,heads,Hf,ML", [(12, 2, 64, 10), (64, 2, 64, 10), (16, 3, 64, 10), (8, 4, 32, 10),
                                           (16, 2, 130, 10), (16, 2, 6, 10), (16, 2, 64, 64), (16, 2, 64, 0)])
def test_unsupported_shapes_are_rejected(hip_lib, D, heads, Hf, ML):
    from recman_amd import _lib, ops

    assert not ops.bst_supported(D, heads, Hf, ML)
    assert ops.bst_supported(16, 2, 64, 63) and ops.bst_supported(8, 2, 4, 1) and ops.bst_supported(32, 8, 128, 63)
    assert ops.bst_workspace(D, heads, Hf, ML, 4, True) == 0
    B, nnz = 4, 8
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    p = {n: z(*s) for n, s in ops.bst_param_shapes(D, Hf, ML).items()}
    offsets = torch.arange(0, nnz + 1, 2, device="cuda")
    ids, qrow = torch.zeros(nnz, dtype=I64, device="cuda"), torch.zeros(B, dtype=I64, device="cuda")
    out = torch.full((B, 2 * D), 7.0, device="cuda")
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        ops.bst_fwd(z(6, 2 * D), 0, D, offsets, ids, qrow, p, heads, ML, out, z(1 << 16))
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        ops.bst_bwd(z(6, 2 * D), 0, D, offsets, ids, qrow, p, heads, ML, z(B, D), z(nnz, D), z(B, D),
                    {n: z(*v.shape) for n, v in p.items()}, z(1 << 16))
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0  # rejected before any launch


def test_cpu_tensors_are_refused(hip_lib):
    from recman_amd import ops

    case = _case("d16_h2_f64")[0]
    p = {n: v.float() for n, v in case["p"].items()}
    with pytest.raises(ValueError, match="GPU"):
        ops.bst_fwd(case["table"].float(), 0, 16, case["offsets"], case["ids"], case["qidx"], p, 2, 10,
                    torch.zeros(case["B"], 32), torch.zeros(1 << 16))


def test_engine_turns_an_unsupported_shape_into_a_value_error(hip_lib):
    from recman_amd import engine as eng

    hp = dict(deep_hidden_units=(8, 8), seq_pooling="transformer")
    long = eng.FeatureSpec(["item", "hist"], [9, 0], seq_query={"hist": "item"}, seq_max_len={"hist": 64})
    with pytest.raises(ValueError, match="max_len 1..63"):
        eng.DINEngine(long, 16, hp)
    ok = eng.FeatureSpec(["item", "hist"], [9, 0], seq_query={"hist": "item"}, seq_max_len={"hist": 30})
    with pytest.raises(ValueError, match="att_head_num 1/2/4/8"):
        eng.BSTEngine(ok, 16, dict(hp, att_head_num=3))
    with pytest.raises(ValueError, match="att_ffn_units"):
        eng.BSTEngine(ok, 16, dict(hp, att_ffn_units=130))
    with pytest.raises(ValueError, match="embedding_size 8/16/32"):
        eng.BSTEngine(ok, 64, hp)
    with pytest.raises(NotImplementedError, match="att_dropout"):
        eng.DCNEngine(ok, 16, dict(hp, att_dropout=(1, 0.5, 1)))
    with pytest.raises(ValueError, match="seq_pooling"):
        eng.DINEngine(ok, 16, dict(hp, seq_pooling="gru"))
    with pytest.raises(ValueError, match="seq_pooling"):  # also without a sequence feature
        eng.DINEngine(eng.FeatureSpec(["item"], [9]), 16, dict(hp, seq_pooling="gru"))
    e = eng.BSTEngine(ok, 16, dict(deep_hidden_units=(8, 8)))  # forced to "transformer"
    assert "hist_bst_pos" in e.params and not any("_asp_" in n for n in e.params)
    assert tuple(e.params["hist_bst_pos"].shape) == (31, 16) and tuple(e.params["hist_bst_ffn_w1"].shape) == (16, 64)
