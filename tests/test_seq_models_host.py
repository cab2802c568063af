"""tests/seq_models_ref.py - the float64 restatement of any model over any front - checked without a GPU: pinned bit
for bit to the restatements that are already pinned, its autograd against central differences, no unit of any case
near its kink, its own float32 twin inside half the GPU bound, and the comparison the GPU tests call
(seq_models_ref.check_grads) shown to catch each wrong hand-off between a pooling unit and a model."""
import pytest
import torch

from oracle import th_layers as TL
from tests import asp_ref, bst_ref, dien_ref
from tests import seq_models_ref as R

F64 = torch.float64
PAIRS = [(m, kind) for m in R.MODELS for kind in R.KINDS]
MIXED = [(m, kind) for m in ("deepfm", "dcn") for kind in R.KINDS]


def _case(model_id, kind):
    return R.make_case(model_id, kind)


def _all_cases():
    for m, kind in PAIRS:
        yield f"{m}-{kind}", R.make_case(m, kind)
    for m, kind in MIXED:
        yield f"mixed-{m}-{kind}", R.make_mixed_case(kind, model=m)


# ------------------------------------------------------------------------------------ pinned to what is pinned
@pytest.mark.parametrize("mod,name",
                         [(mod, n) for mod in (asp_ref, bst_ref, dien_ref) for n in sorted(mod.MODEL_CASES)],
                         ids=lambda v: v if isinstance(v, str) else v.__name__.split(".")[-1])
def test_fwd_bwd_equals_the_units_own_model_restatement(mod, name):
    k = mod.make_model_case(**mod.MODEL_CASES[name])
    a = (k["model"], k["p"], k["spec"], k["idx"], k["dense"], k["y"], k["hp"], k["mv"])
    want, got = mod.fwd_bwd(*a), R.fwd_bwd(*a)
    for w, g in zip(want[:3], got[:3]):
        assert torch.equal(w, g)
    assert set(want[3]) == set(got[3])
    for n in want[3]:
        assert torch.equal(want[3][n], got[3][n]), n
    assert torch.equal(mod.embeddings(k["p"], k["spec"], k["idx"], k["mv"], k["hp"]),
                       R.embeddings(k["p"], k["spec"], k["idx"], k["mv"], k["hp"]))


@pytest.mark.parametrize("model_id", list(R.MODELS))
def test_logit_without_a_sequence_feature_equals_the_models_own(model_id):
    c = R.own_case(model_id, 8)
    tl = c["spec"]
    spec = R.Spec(tl.sparse_names, tl.feat_sizes, tl.dense_names, {})
    want = R.OWN_LOGIT[model_id](c["p"], tl, c["idx"], c["dense"], c["hp"])
    got = R.logit(R.MODELS[model_id], c["p"], spec, c["idx"], c["dense"], c["hp"])
    assert want.shape == got.shape and torch.equal(want, got)
    want = R.OWN_LOGIT[model_id](c["p"], tl, c["idx"], c["dense"], c["hp"], training=False)
    assert torch.equal(want, R.logit(R.MODELS[model_id], c["p"], spec, c["idx"], c["dense"], c["hp"], training=False))


def test_mixed_front_embeddings_equal_the_pieces():
    """Field by field: the multi-valued and the value feature's rows are oracle.th_layers', each history's row is its
    unit's on ITS csr and ITS variables, and a history ahead of its query reads the query's column."""
    for kind in R.KINDS:
        k = R.make_mixed_case(kind)
        p, spec, idx, mv, hp = k["p"], k["spec"], k["idx"], k["mv"], k["hp"]
        E = R.embeddings(p, spec, idx, mv, hp)
        want = TL.feat_embedding_layer(p, spec.tl, idx[:, spec.plain_cols], use_bias=False, mv=mv)[0]
        for j, f in enumerate(spec.plain_cols):
            assert torch.equal(E[:, f], want[:, j])
        T = p["item_feat_embed"]
        for n in ("hist2", "hist"):
            row = R.unit_row(kind, p, n, T[idx[:, 2]], T[mv[n][1]], mv[n][0], hp)
            assert torch.equal(E[:, spec.sparse_names.index(n)], row)
        assert not torch.equal(E[:, 0], E[:, 3])
        n2, n6 = (mv[n][0][1:] - mv[n][0][:-1] for n in ("hist2", "hist"))
        assert int(n2[0]) == 0 and int(n6[0]) == 0 and int(n2.max()) == 3 and int(n6.max()) == 6
        nt = mv["tags"][0][1:] - mv["tags"][0][:-1]
        assert int(nt.min()) == 0 and int(nt.max()) > 1
        assert len(R.shared_rows(k)["item"]) > 0


# ------------------------------------------------------------------------------------------- finite differences
@pytest.mark.parametrize("model_id,kind", [(m, R.KINDS[i % 3]) for i, m in enumerate(R.MODELS)] + [("mixed", "dien")])
def test_autograd_matches_central_differences(model_id, kind):
    k = R.make_mixed_case(kind) if model_id == "mixed" else _case(model_id, kind)
    a = lambda p: (k["model"], p, k["spec"], k["idx"], k["dense"], k["hp"], k["mv"])  # noqa: E731
    grads = R.reference(k)[0][3]
    g = torch.Generator().manual_seed(5)
    v = {n: torch.randn(t.shape, generator=g, dtype=F64) for n, t in k["p"].items()}
    want = sum(float((grads[n] * v[n]).sum()) for n in v)

    def loss(t):
        p = {n: k["p"][n] + t * v[n] for n in v}
        out = R.logit(*a(p))
        return float(TL.create_loss(k["y"], TL.prediction(out)) + R.l2(k["model"], p, k["spec"], k["hp"]))

    h = 1e-6
    got = (loss(h) - loss(-h)) / (2 * h)
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)


# ------------------------------------------------------------------------------------------------------ kinks
def test_no_unit_of_any_case_is_near_its_kink():
    """Nothing may be left out (the gradient comes from the labels): the stream is searched for (make_case), and the
    distance of the closest kinked unit - DNN, the model's own, the transformer's FFN - is asserted here."""
    for what, k in _all_cases():
        p, spec = k["p"], k["spec"]
        d = R.min_abs_pre(k["model"], p, spec, k["idx"], k["dense"], k["hp"], k["mv"])
        assert d == k["min_abs_pre"] and R.KINK <= d < float("inf"), (what, d, k["attempt"])
    # the din unit under relu is covered by the same search
    k = R.make_case("afm", "din", att_activation="relu", att_hidden_units=(16, 8))
    assert k["hp"]["att_activation"] == "relu" and R.KINK <= k["min_abs_pre"] < float("inf")
    T = k["p"]["item_feat_embed"]
    z = asp_ref.asp_hidden(T[k["idx"][:, 1]], T[k["mv"]["hist"][1]], k["mv"]["hist"][0],
                           *asp_ref.asp_vars(k["p"], "hist_", 2)[:2], "relu")
    assert k["min_abs_pre"] <= min(float(t.abs().min()) for t in z)


def test_case_conditions():
    for m, kind in PAIRS:
        k = _case(m, kind)
        spec, hp = k["spec"], k["hp"]
        assert spec.sparse_names == ["C0", "item", "hist", "C2"] and spec.feat_sizes == [7, 11, 0, 5]
        assert k["idx"].shape == (37, 4) and k["dense"].shape == (37, 2) and spec.seq_max_len == {"hist": 6}
        n = k["mv"]["hist"][0][1:] - k["mv"]["hist"][0][:-1]
        assert n[:3].tolist() == [0, 1, 6] and R.shared_rows(k)["item"]
        # (AutoInt is cast without a DNN: its deep_l2_reg covers no variable)
        assert all(v > 0 for key, v in hp.items()
                   if key.endswith("_l2_reg") and (key != "deep_l2_reg" or m != "autoint"))
        assert hp["seq_pooling"] == kind and hp.get("use_linear", True)
        for t in k["p"].values():  # every value is a float32 number
            assert t.dtype == F64 and torch.equal(t, t.float().double())
        assert any(n.startswith(f"hist_{R.UNIT_TAG[kind]}_") for n in k["p"])


# ---------------------------------------------------------------------------------------- the float32 CPU twin
def test_float32_twin_stays_inside_half_the_gpu_bound():
    """Every variable the GPU test holds to the plain 2e-5 has a float32 CPU measure of at most 1e-5 against float64:
    the yardstick alone stays inside the bound.  The analytically zero gradients are judged as on the GPU."""
    worst, zero = {}, set()
    for what, k in _all_cases():
        (_, _, _, want), g32, scales = R.reference(k)
        for n in want:
            rule = R.zero_rule(n, k["spec"], k["hp"])
            if rule:
                # (float64's own residue of the cancellation is far below anything the rules accept)
                assert float(want[n].abs().max()) < 1e-12, (what, n)
                zero.add((rule, n))
            if rule or R.is_loose(n, k["spec"]):
                continue
            m32 = R.grad_measure(g32[n], want[n])
            worst[what] = max(worst.get(what, 0.0), m32)
            assert m32 <= 1e-5, (what, n, m32)
        R.check_grads(k, g32, want, g32, scales, what=what + " ", show=lambda s: None)  # the twin itself passes
        R.check_grads(k, want, want, g32, scales, what=what + " ", show=lambda s: None)
    # both analytically zero gradients occur among the cases, on both histories of the mixed spec
    assert {("w0", "hist_asp_w0"), ("w0", "hist2_asp_w0"), ("bk", "hist_bst_bk"), ("bk", "hist2_bst_bk")} <= zero
    print({w: f"{m:.1e}" for w, m in worst.items()})


# -------------------------------------------------------------------------- the comparison catches a wrong hand-off
@pytest.mark.parametrize("wrong", R.WRONG)
def test_the_comparison_catches_each_wrong_variant_on_every_model(wrong):
    for what, k in _all_cases():
        (_, _, _, want), g32, scales = R.reference(k)
        got = R.fwd_bwd(k["model"], k["p"], k["spec"], k["idx"], k["dense"], k["y"], k["hp"], k["mv"], wrong=wrong)[3]
        with pytest.raises(AssertionError, match="grad "):
            R.check_grads(k, got, want, g32, scales, what=f"{what} {wrong}: ", show=lambda s: None)


def test_mixed_spec_item_rows_hold_three_gradients():
    """item_feat_embed of the mixed case is the sum of the field's own gradient, both histories' query gradients and
    both histories' key gradients: dropping any of them moves the shared rows far beyond the bound."""
    for kind in R.KINDS:
        k = R.make_mixed_case(kind, model="dcn")
        want = R.reference(k)[0][3]["item_feat_embed"]
        both = R.shared_rows(k)["item"]
        for wrong in ("no_query_grad", "no_key_grad", "query_grad_overwrites"):
            got = R.fwd_bwd(k["model"], k["p"], k["spec"], k["idx"], k["dense"], k["y"], k["hp"], k["mv"],
                            wrong=wrong)[3]["item_feat_embed"]
            assert R.grad_measure(got[both], want[both]) > 100 * R.TOL, (kind, wrong)
