"""tests/ref_common.py - what every float64 twin shares - checked without a GPU: the measures on the inputs that
decide them, the stream search giving up, the streams' float32 values, and one frozen fingerprint per family of twins,
so that a change of a draw order fails here instead of shifting a tolerance unnoticed."""
import hashlib

import pytest
import torch

from tests import (afm_ref, asp_ref, autoint_ref, bst_ref, crossmix_ref, dien_ref, dlrm_ref, fibinet_ref, fmfm_ref,
                   masknet_ref, mmoe_ref, pnn_ref, seq_models_ref, twotower_ref)
from tests import ref_common as C

F64 = torch.float64


def test_grad_measure():
    zero = torch.zeros(3, dtype=F64)
    assert C.grad_measure(torch.zeros(3), zero) == 0.0
    assert C.grad_measure(torch.tensor([0.0, 1e-30, 0.0]), zero) == float("inf")
    # |got - want| = (0.5, 0.5, 0.01) over max(|want|, 0.1 * 10) = (10, 1, 1): the small entries are held to the floor
    want, got = torch.tensor([10.0, 1.0, 0.0], dtype=F64), torch.tensor([10.5, 0.5, 0.01], dtype=F64)
    assert C.grad_measure(got, want) == pytest.approx(0.5, rel=1e-12)
    assert C.grad_measure(want.float(), want) == 0.0
    # an empty gradient: the plain measure has nothing to take a maximum of, the sequence units' measure says 0
    empty = torch.zeros(0, 4, dtype=F64)
    with pytest.raises(RuntimeError):
        C.grad_measure(empty, empty)
    assert C.grad_measure_or_empty(empty, empty) == 0.0
    assert C.grad_measure_or_empty(got, want) == C.grad_measure(got, want)


def test_rel_error():
    want, got = torch.tensor([100.0, 0.5], dtype=F64), torch.tensor([101.0, 0.25], dtype=F64)
    assert C.rel_error(got, want) == pytest.approx(0.25, rel=1e-12)  # (1 / 100, 0.25 / max(1, 0.5))
    assert C.rel_error(torch.zeros(0), torch.zeros(0)) == 0.0


def test_first_stream_gives_up_after_its_attempts():
    seen = []
    with pytest.raises(AssertionError, match="no stream met"):
        C.first_stream(100, lambda g, rnd: seen.append(g.initial_seed()), lambda k: False, attempts=5)
    assert seen == [100, 101, 102, 103, 104]
    out, attempt = C.first_stream(100, lambda g, rnd: g.initial_seed(), lambda seed: seed == 102)
    assert (out, attempt) == (102, 2)


def test_rnd_stream_draws_float32_values_in_the_generators_order():
    a, b = C.rnd_stream(torch.Generator().manual_seed(7)), torch.Generator().manual_seed(7)
    x, y = a(5, 3, std=0.3), a(4)
    assert x.dtype == F64 and x.shape == (5, 3) and torch.equal(x, x.float().double())
    assert torch.equal(x, (torch.randn(5, 3, generator=b, dtype=F64) * 0.3).float().double())
    assert torch.equal(y, torch.randn(4, generator=b, dtype=F64).float().double())
    w = C.glorot(C.rnd_stream(torch.Generator().manual_seed(7)), (200, 300), 200, 300)
    assert float(w.std()) == pytest.approx((2.0 / 500) ** 0.5, rel=0.02)


def test_memo_makes_a_case_once_however_it_is_asked_for():
    calls = []

    @C.memo
    def make(a, hidden=(4,), **kw):
        calls.append(a)
        return dict(a=a)

    assert make(1) is make(1, (4,)) is make(a=1, hidden=[4]) and calls == [1]
    assert make(1, (5,)) is not make(1) and make(1, x=2) is make(1, x=2) and calls == [1, 1, 1]


def fingerprint(k):
    h = hashlib.sha256()
    for n, t in list(k["p"].items()) + [(n, k[n]) for n in ("idx", "dense", "y", "Y") if k.get(n) is not None]:
        h.update(f"{n} {t.dtype} {tuple(t.shape)} ".encode())
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


# family -> (the smallest model-level case its tests use, SHA-256 over the names, types, shapes and bytes of p (in the
# order drawn), idx, dense and the labels).  The digests were computed before the twins shared any scaffolding.
FAMILY_CASES = {
    "afm": (lambda: afm_ref.make_afm_case(**afm_ref.MODEL_CASES["d8"]),
            "1fe0f29df397e26f69a8b861439327390a056392f3e4d569725f628f7ea836fc"),
    "asp": (lambda: asp_ref.make_model_case(**asp_ref.MODEL_CASES["din_d8"]),
            "c5e2abfcfa682fd4747e1ad6dcff78661e5a16bfa484017fa10226be39720c4f"),
    "autoint": (lambda: autoint_ref.make_case(**autoint_ref.MODEL_CASES["d8"]),
                "d88021a05c1b2cede60893a2cf72669a0df290e60d6398fdb6a18bafe03750cf"),
    "bst": (lambda: bst_ref.make_model_case(**bst_ref.MODEL_CASES["bst_d8"]),
            "6dad287ca88817c0bc2ba3f574257360f6a3b70f2841b856abde26d6b7cbafc1"),
    "crossmix": (lambda: crossmix_ref.make_case(*crossmix_ref.MODEL_CASES["e1_r8"]),
                 "1534793ddb242a1c01d4aa1f54dbb17530946d9392f58105c309920f5686b1fa"),
    "dien": (lambda: dien_ref.make_model_case(**dien_ref.MODEL_CASES["dien_d8"]),
             "99b4367c3077bd143d5ef55fc5ca8803f43d862a75b45f852ee7a39a1d406554"),
    "dlrm": (lambda: dlrm_ref.make_case(**dlrm_ref.MODEL_CASES["d8"]),
             "bcdc340123d22b55e3d271157a3f3ef7c119d7d5344345aad8d1ce4e2d05bf1e"),
    "fibinet": (lambda: fibinet_ref.make_case(*fibinet_ref.MODEL_CASES["each_d8"]),
                "8c966648a0d352980fc301e3fa05c96c78bea55baf387c80e5659195d97968b2"),
    "fmfm": (lambda: fmfm_ref.make_case(*fmfm_ref.MODEL_CASES["scalar_no_dnn"]),
             "a94164fd61cd8a010227fa6f3de3b9077bd63a5cd1775c8f75b721dbe59622e3"),
    "masknet": (lambda: masknet_ref.make_case(*masknet_ref.MODEL_CASES["serial1"]),
                "da2575d083984d066aea1a8d016a27428fd1872e35044f24886fc81aec3e9750"),
    "mmoe": (lambda: mmoe_ref.make_case(*mmoe_ref.MODEL_CASES["one_task"]),
             "a99b00d439eda3f2d4579da2aa6fec4364314c5ab92ed6212c2c9881df98c81f"),
    "pnn": (lambda: pnn_ref.make_case(*pnn_ref.MODEL_CASES["inner_only"]),
            "7a316eef53b7f91f7828ffc3769bf5f8bc2b41a6e2a9d795dce341dc41dfc84c"),
    # (AFM, not DeepFM: DeepFM's variables come from oracle.th_layers.make_params, whose float32 draws differ in the last
    # bit between CPUs of different vector widths; everything fingerprinted here is a float64 stream)
    "seq_models": (lambda: seq_models_ref.make_case("afm", "din"),
                   "26ceaa9d1d75c4388978a70745cdfaab339944e05349a64dea04698aadc97db2"),
    "seq_models_mixed": (lambda: seq_models_ref.make_mixed_case("din"),
                         "6e32944272ee015e6074b07a035a749c92b0accdfddc8d0431ecd644ab453078"),
    "twotower": (lambda: twotower_ref.make_case(),
                 "d4e86abf544d564d4c4b415697fd8f51493a527ab8ccaa5d5c4985f5b5f4a1f3"),
}


@pytest.mark.parametrize("family", sorted(FAMILY_CASES))
def test_the_familys_case_is_the_one_its_tolerances_were_measured_on(family):
    make, want = FAMILY_CASES[family]
    assert fingerprint(make()) == want, f"{family}: the case's draws changed"
