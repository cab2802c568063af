"""GPU: rm_dien_fwd / rm_dien_bwd through the C ABI (recman_amd.ops) against the float64 restatement + autograd
(tests/dien_ref.py, pinned on the CPU by tests/test_dien_host.py).

Tolerance, the convention of tests/test_gpu_asp.py and tests/test_gpu_bst.py: for every output (pooled rows, key
gradients, query gradient, each of the 7 parameter gradients) the gradient measure of tests/test_gpu_parity.py must be
<= max(2e-5, 4 x the float32 CPU restatement's own measure on the case); both numbers are printed.  The yardstick is the
float32 restatement, never the kernel.  The unit has no kink (sigmoid, tanh, softmax): no guard, every example counts."""
import functools

import pytest
import torch

from tests import dien_ref as R

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64
ROW0 = 5  # the key block starts behind a few foreign rows of the table


@functools.lru_cache(maxsize=None)
def _case(name, rng=False):
    """(case, float64 reference, float32 CPU reference): computed once, shared and left unchanged."""
    if rng:
        case = R.make_dien_case(**R.RANGE_CASES[name], att_scale=R.RANGE_SCALE, big_bias=True)
    else:
        case = R.make_dien_case(**R.GPU_CASES[name])
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

    B, D, ML = case["B"], case["D"], case["max_len"]
    rows = _table(case)
    LD = rows.shape[1]
    offsets, ids = case["offsets"].cuda(), case["ids"].cuda()
    qrow = (case["qidx"] + ROW0).cuda()
    nnz = int(ids.shape[0])
    p = {n: _dev(v) for n, v in case["p"].items()}
    out = torch.full((B, LD), float("nan"), device="cuda")
    ws = torch.full((max(4, ops.dien_workspace(D, ML, B, nnz, backward)),), float("nan"), device="cuda")
    ops.dien_fwd(rows, ROW0, D, offsets, ids, qrow, p, ML, backward, out, ws)
    if not backward:
        torch.cuda.synchronize()
        return (out,)
    # the pooled rows' gradient and the query gradient are columns of a wider [B, F, D] buffer, as in the engine
    wide = torch.zeros(B, 3, D, device="cuda")
    wide[:, 2, :] = _dev(case["g"])
    wide[:, 0, :] = _dev(case["dq_up"])
    d_keys = torch.full((nnz, D), float("nan"), device="cuda")
    grads = {n: torch.full_like(v, float("nan")) for n, v in p.items()}
    ops.dien_bwd(rows, ROW0, D, offsets, ids, qrow, p, ML, wide[:, 2, :], d_keys, wide[:, 0, :], grads, ws)
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
        m, m32 = R.grad_measure(a, wnt.reshape(a.shape)), R.grad_measure(c32, wnt)
        bound = max(2e-5, 4 * m32)
        print(f"{tag}: {name} measure {m:.2e}, float32 CPU {m32:.2e}, bound {bound:.2e}")
        if not m <= bound:
            bad.append(f"{name} measure {m:.3e} > {bound:.3e} (float32 CPU {m32:.3e})")
    assert not bad, f"{tag}: " + "; ".join(bad)
    return res


@pytest.mark.parametrize("name", sorted(R.GPU_CASES))
def test_dien_kernels_match_float64(hip_lib, name):
    case, want, cpu32 = _case(name)
    n = case["offsets"][1:] - case["offsets"][:-1]
    assert int(n[0]) == 0 and int(n[1]) == 1 and int(n[2]) == case["max_len"]
    assert all(case["B"] % k for k in (16, 32, 64))
    ids = case["ids"][int(case["offsets"][2]): int(case["offsets"][3])]
    assert case["max_len"] < 2 or int(ids[0]) == int(ids[1])  # a repeated id in the longest history
    res = _check(case, want, cpu32, name)
    # an example without history: a zero row
    assert float(res[0][0].abs().max()) == 0.0 and float(res[0][1, : case["D"]].abs().max()) > 0


@pytest.mark.parametrize("name", sorted(R.RANGE_CASES))
def test_large_scores_and_saturated_gates(hip_lib, name):
    """att_w x 4000 and every second bias +-100.  On `d8_len30` the longest example's two top scores lie 0.123 apart at
    1062 (softmax weights 0.47 / 0.53, every other below 1e-12): |att_w q| multiplies the error of h_t into the
    score, and the score's error is the relative error of everything behind the softmax.  A float32 extractor measured
    d_keys 5.98e-4 here against the bound of 4.11e-4; with h_t and s_t formed in float64 the kernel measures 2.5e-5."""
    case, want, cpu32 = _case(name, True)
    _check(case, want, cpu32, f"{name} att_w x{R.RANGE_SCALE}, biases +-{R.BIG_BIAS}")


def test_two_runs_are_bit_equal(hip_lib):
    case = _case("d16_grid_stride")[0]
    a, b = _flat(_run(case)), _flat(_run(case))
    for (nm, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), nm


@pytest.mark.parametrize("name", ["d16", "d8_long", "d32"])
def test_out_is_bit_equal_with_and_without_save(hip_lib, name):
    case = _case(name)[0]
    assert torch.equal(_run(case, backward=False)[0], _run(case)[0])


def test_query_gradient_is_added_onto_what_the_buffer_holds(hip_lib):
    case = _case("d16")[0]
    zero = dict(case, dq_up=torch.zeros_like(case["dq_up"]))
    with_up, plain = _run(case)[2], _run(zero)[2]
    assert float(plain.abs().max()) > 0
    want = plain.cpu().double() + case["dq_up"]
    assert float((with_up.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert float((with_up - plain).abs().max()) > 1e-3


def test_all_examples_without_history(hip_lib):
    case = _case("d8_many")[0]
    B, D = case["B"], case["D"]
    case = dict(case, offsets=torch.zeros(B + 1, dtype=I64), ids=torch.zeros(0, dtype=I64))
    out, d_keys, d_query, grads = _run(case)
    assert d_keys.shape == (0, D)
    assert float(out.abs().max()) == 0.0
    assert torch.equal(d_query, _dev(case["dq_up"]))  # unchanged
    for n, t in grads.items():
        assert float(t.abs().max()) == 0.0, n


def test_a_history_longer_than_max_len_keeps_its_last_items_and_zeroes_the_rest(hip_lib):
    """A caller error made safe: example 2 (the longest) gets 3 more items in FRONT; the kernels use its last max_len
    items, so every output equals the unchanged case's, and the d_keys rows of the 3 cut occurrences are zero."""
    case = _case("d16")[0]
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

    D, ML = 16, 10
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    p = {n: z(*s) for n, s in ops.dien_param_shapes(D).items()}
    grads = {n: torch.full_like(v, float("nan")) for n, v in p.items()}
    e64 = torch.zeros(0, dtype=I64, device="cuda")
    ws = torch.empty(max(4, ops.dien_workspace(D, ML, 0, 0, True)), device="cuda")
    ops.dien_bwd(z(6, 2 * D), 0, D, torch.zeros(1, dtype=I64, device="cuda"), e64, e64, p, ML, z(0, D), z(0, D),
                 z(0, D), grads, ws)
    torch.cuda.synchronize()
    for n, t in grads.items():
        assert float(t.abs().max()) == 0.0, n


@pytest.mark.parametrize("D,ML", [(12, 10), (64, 10), (4, 10), (16, 0), (16, 257), (8, -1)])
def test_unsupported_shapes_are_rejected(hip_lib, D, ML):
    from recman_amd import _lib, ops

    assert not ops.dien_supported(D, ML)
    assert ops.dien_supported(16, 256) and ops.dien_supported(8, 1) and ops.dien_supported(32, 50)
    assert ops.dien_workspace(D, ML, 4, 8, True) == 0
    B, nnz = 4, 8
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    p = {n: z(*s) for n, s in ops.dien_param_shapes(D).items()}
    offsets = torch.arange(0, nnz + 1, 2, device="cuda")
    ids, qrow = torch.zeros(nnz, dtype=I64, device="cuda"), torch.zeros(B, dtype=I64, device="cuda")
    out = torch.full((B, 2 * D), 7.0, device="cuda")
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        ops.dien_fwd(z(6, 2 * D), 0, D, offsets, ids, qrow, p, ML, True, out, z(1 << 16))
    with pytest.raises(_lib.RecmanHipError, match="unsupported"):
        ops.dien_bwd(z(6, 2 * D), 0, D, offsets, ids, qrow, p, ML, z(B, D), z(nnz, D), z(B, D),
                     {n: z(*v.shape) for n, v in p.items()}, z(1 << 16))
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0  # rejected before any launch


def test_cpu_tensors_are_refused(hip_lib):
    from recman_amd import ops

    case = _case("d16")[0]
    p = {n: v.float() for n, v in case["p"].items()}
    with pytest.raises(ValueError, match="GPU"):
        ops.dien_fwd(case["table"].float(), 0, 16, case["offsets"], case["ids"], case["qidx"], p, 10, False,
                     torch.zeros(case["B"], 32), torch.zeros(1 << 16))


def test_engine_accepts_the_unit_and_refuses_what_it_cannot_do(hip_lib):
    from recman_amd import engine as eng

    hp = dict(deep_hidden_units=(8, 8), seq_pooling="dien")
    ok = eng.FeatureSpec(["item", "hist"], [9, 0], seq_query={"hist": "item"}, seq_max_len={"hist": 30})
    e = eng.DINEngine(ok, 16, hp)
    assert tuple(e.params["hist_dien_gru_w"].shape) == (16, 48) and tuple(e.params["hist_dien_att_w"].shape) == (16, 16)
    assert tuple(e.params["hist_dien_augru_b"].shape) == (48,) and float(e.params["hist_dien_gru_b"].abs().max()) == 0.0
    assert not any("_asp_" in n or "_bst_" in n for n in e.params)
    e = eng.DIENEngine(ok, 16, dict(deep_hidden_units=(8, 8)))  # forced to "dien"
    assert sorted(n for n in e.params if "_dien_" in n) == sorted(f"hist_dien_{v}" for v in R.NAMES)
    long = eng.FeatureSpec(["item", "hist"], [9, 0], seq_query={"hist": "item"}, seq_max_len={"hist": 257})
    with pytest.raises(ValueError, match="max_len 1..256"):
        eng.DINEngine(long, 16, hp)
    with pytest.raises(ValueError, match="embedding_size 8/16/32"):
        eng.DIENEngine(ok, 64, hp)
    with pytest.raises(NotImplementedError, match="att_dropout"):
        eng.DCNEngine(ok, 16, dict(hp, att_dropout=(1, 0.5, 1)))
    with pytest.raises(ValueError, match="seq_pooling"):
        eng.DINEngine(ok, 16, dict(hp, seq_pooling="gru"))
    with pytest.raises(ValueError, match="seq_pooling"):  # also without a sequence feature
        eng.DINEngine(eng.FeatureSpec(["item"], [9]), 16, dict(hp, seq_pooling="gru"))
