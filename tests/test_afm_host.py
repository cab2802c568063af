"""CPU: pins the AFM restatement (tests/afm_ref.py) the GPU tests compare the kernels against, and the public surface
of the feature (th.AFM's constructor, the engine registry, the C ABI).  No GPU needed."""
import inspect
import os

import pytest
import torch

from oracle import th_layers as TL
from tests import afm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _small(B=4, F=5, D=3, T=4, seed=0, mask=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    E, W, b, h, p = r(B, F, D) * 0.7, r(D, T) * 0.6, r(T) * 0.2, r(T), r(D)
    m = (torch.rand(B, D, generator=g) < 0.7).to(F64) / 0.7 if mask else None
    return E, W, b, h, p, m


def _loops(E, W, b, h, p, mask):
    """The contract as a plain-Python double loop over the pairs (lists and floats, no tensor arithmetic)."""
    import math

    E, W, b, h, p = E.tolist(), W.tolist(), b.tolist(), h.tolist(), p.tolist()
    B, F, D, T = len(E), len(E[0]), len(p), len(b)
    out = []
    for n in range(B):
        prods, scores = [], []
        for i in range(F):
            for j in range(i + 1, F):
                P = [E[n][i][d] * E[n][j][d] for d in range(D)]
                s = 0.0
                for t in range(T):
                    z = b[t] + sum(P[d] * W[d][t] for d in range(D))
                    s += h[t] * max(z, 0.0)
                prods.append(P)
                scores.append(s)
        mx = max(scores)
        ex = [math.exp(s - mx) for s in scores]
        den = sum(ex)
        v = [sum(e / den * P[d] for e, P in zip(ex, prods)) for d in range(D)]
        out.append(sum(p[d] * v[d] * (mask[n][d] if mask is not None else 1.0) for d in range(D)))
    return torch.tensor(out, dtype=F64)


@pytest.mark.parametrize("mask", [False, True])
def test_restatement_equals_a_plain_double_loop(mask):
    E, W, b, h, p, m = _small(mask=mask)
    got = R.afm_layer(E, W, b, h, p, m)
    want = _loops(E, W, b, h, p, m.tolist() if m is not None else None)
    assert float((got - want).abs().max()) < 1e-12


def test_pairs_are_the_upper_triangle_row_major():
    i, j = R.pair_index(4)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def test_closed_form_two_fields():
    """F = 2: one pair, a = 1, afm_logit = p . (E_0 * E_1) whatever W, b, h are; dW = db = dh = 0 (here: to the
    rounding of q - g * logit, two sums of the same terms in different orders; the kernel gets an exact 0)."""
    E, W, b, h, p, _ = _small(F=2, mask=False)
    leaves = [t.clone().requires_grad_(True) for t in (E, W, b, h, p)]
    y = R.afm_layer(*leaves)
    assert float((y.detach() - (E[:, 0] * E[:, 1]) @ p).abs().max()) < 1e-14
    y.sum().backward()
    for t in leaves[1:4]:
        assert float(t.grad.abs().max()) < 1e-15
    dE, dW, db, dh, dp = R.afm_layer_bwd(E, W, b, h, p, None, torch.ones(E.shape[0], dtype=F64))
    assert max(float(dW.abs().max()), float(db.abs().max()), float(dh.abs().max())) < 1e-15
    assert float((dE[:, 0] - E[:, 1] * p).abs().max()) < 1e-14 and float((dp - (E[:, 0] * E[:, 1]).sum(0)).abs().max()) < 1e-14


def test_closed_form_uniform_attention_is_the_fm_term():
    """h = 0: attention is uniform, P * afm_logit = p . 1/2 (S^2 - sum_f E_f^2); with p = 1 that is the FM
    second-order term of oracle.th_layers.fm_layer (called with a zero bias)."""
    E, W, b, h, p, _ = _small(F=6, D=5, mask=False)
    npairs = 6 * 5 // 2
    y = R.afm_layer(E, W, b, torch.zeros_like(h), torch.ones_like(p))
    fm = TL.fm_layer(E, torch.zeros(E.shape[0], 6, 1, dtype=F64)).reshape(-1)
    assert float((y * npairs - fm).abs().max()) < 1e-12


def test_logit_is_invariant_under_a_permutation_of_the_fields():
    E, W, b, h, p, m = _small(F=7)
    perm = torch.tensor([3, 0, 6, 1, 5, 2, 4])
    a, c = R.afm_layer(E, W, b, h, p, m), R.afm_layer(E[:, perm], W, b, h, p, m)
    assert float((a - c).abs().max()) < 1e-13


def test_gradcheck_float64():
    E, W, b, h, p, m = _small(B=3, F=4, D=3, T=3, seed=3)
    leaves = [t.clone().requires_grad_(True) for t in (E, W, b, h, p)]
    assert torch.autograd.gradcheck(lambda *a: R.afm_layer(*a, m), leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("mask,up", [(False, False), (True, True)])
def test_written_out_backward_equals_autograd(mask, up):
    E, W, b, h, p, m = _small(B=6, F=6, D=4, T=5, seed=5, mask=mask)
    g0 = torch.Generator().manual_seed(9)
    g = torch.randn(6, generator=g0, dtype=F64)
    dE_up = torch.randn(6, 6, 4, generator=g0, dtype=F64) if up else None
    leaves = [t.clone().requires_grad_(True) for t in (E, W, b, h, p)]
    (R.afm_layer(*leaves, m) * g).sum().backward()
    got = R.afm_layer_bwd(E, W, b, h, p, m, g, dE_up)
    want = [t.grad for t in leaves]
    if up:
        want[0] = want[0] + dE_up
    for a, c, name in zip(got, want, ("dE", "dW", "db", "dh", "dp")):
        assert float((a - c).abs().max()) < 1e-12, name
    # sum_ij a_ij q_ij = g * afm_logit, the identity the backward leans on
    P, z = R.afm_hidden(E, W, b)
    a_ = torch.softmax(torch.relu(z) @ h, dim=1)
    mm = m if m is not None else torch.ones(6, 4, dtype=F64)
    q = (P * (g.unsqueeze(1) * mm * p).unsqueeze(1)).sum(dim=2)
    assert float(((a_ * q).sum(dim=1) - g * R.afm_layer(E, W, b, h, p, m)).abs().max()) < 1e-13


def test_softmax_is_max_subtracted():
    """Scores in the hundreds: a softmax without max subtraction is not finite, the restatement is, in both types."""
    k = R.gpu_case(R.RANGE_CASES[0], h_scale=R.RANGE_H_SCALE)
    P, z = R.afm_hidden(k["E"], k["W"], k["b"])
    s = torch.relu(z) @ k["h"]
    assert float(s.abs().max()) > 89.0  # exp overflows fp32 beyond 88.7
    y64 = R.afm_layer(k["E"], k["W"], k["b"], k["h"], k["p_vec"])
    y32 = R.afm_layer(*(k[n].float() for n in ("E", "W", "b", "h", "p_vec")))
    assert bool(torch.isfinite(y32).all()) and float((y32.double() - y64).abs().max()) < 1e-5


def test_model_composition_matches_its_parts():
    k = R.make_afm_case(B=12, F=5, D=8, Dn=2, T=4, seed=2)
    p, spec, idx, dense, y, hp = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp"))
    loss, logit, pred, grads = R.fwd_bwd(p, spec, idx, dense, y, hp)
    E, _ = TL.feat_embedding_layer(p, spec, idx, use_bias=False)
    want = TL.linear_layer(p, spec, idx, dense).reshape(-1) + R.afm_layer(
        E, p["afm_attention_w"], p["afm_attention_b"], p["afm_attention_h"], p["afm_projection_p"])
    assert float((logit - want).abs().max()) < 1e-13
    l2 = 1e-3 * 0.5 * (sum(p[f"{n}_feat_embed"].square().sum() for n in spec.sparse_names)
                       + p["linear_w"].square().sum() + p["afm_attention_w"].square().sum())
    assert abs(float(loss) - float(TL.create_loss(y, TL.prediction(want)) + l2)) < 1e-13
    assert set(grads) == set(p) and all(float(g.abs().max()) > 0 for g in grads.values())
    assert not any(n.endswith("_feat_bias") for n in p)
    # dropout: active in training only, through masks["afm"]
    hp2 = dict(hp, att_dropout=0.8)
    a = R.afm_logit(p, spec, idx, dense, hp2, training=True, masks={"afm": k["mask"]})
    c = R.afm_logit(p, spec, idx, dense, hp2, training=False, masks={"afm": k["mask"]})
    assert float((a - c).abs().max()) > 1e-6 and float((c.reshape(-1) - want).abs().max()) < 1e-13


# ------------------------------------------------------------------------------------------- the kink guard
@pytest.mark.parametrize("case", R.GPU_CASES + [c + ("range",) for c in R.RANGE_CASES])
def test_kink_guard_zeroes_at_most_a_fifth_of_every_gpu_case(case):
    h_scale = R.RANGE_H_SCALE if case[-1] == "range" else 1.0
    k = R.gpu_case(case[:4], h_scale=h_scale)
    assert k["zeroed"] <= R.KINK_CAP, k["zeroed"]
    assert bool((k["g"][k["near"]] == 0).all()) and bool((k["g"][~k["near"]] != 0).all())


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_cases_have_no_hidden_unit_at_its_kink(name):
    assert R.make_afm_case(**R.MODEL_CASES[name])["model_min_abs_z"] >= R.KINK


# ------------------------------------------------------------------------------------------------- surface
def test_constructor_has_the_reference_signature():
    from sklearn.metrics import log_loss, roc_auc_score

    import recman_amd.th as th

    params = list(inspect.signature(th.AFM.__init__).parameters.values())[1:]
    want = [("feat_dict", inspect.Parameter.empty), ("embedding_size", 8), ("embedding_l2_reg", 0.00001),
            ("linear_l2_reg", 0.00001), ("att_factor", 8), ("att_l2_reg", 0.00001), ("att_dropout", 1),
            ("epoch", 10), ("batch_size", 256), ("learning_rate", 0.001), ("optimizer", "adam"),
            ("random_seed", 2019), ("use_deep", True), ("loss_type", "logloss"),
            ("eval_metric", (roc_auc_score, log_loss)), ("l2_reg", 0.1), ("what_means_greater", None),
            ("use_interactive_session", True), ("log_dir", "./logs")]
    assert [(p.name, p.default) for p in params[:len(want)]] == want
    assert [p.name for p in params[len(want):]] == ["strict_reference", "device"]
    assert th.AFM.model == "afm" and "AFM" in th.__all__


def test_engine_is_registered_and_layer_is_exported():
    from recman_amd import engine
    from recman_amd.th import layers

    assert "afm" in engine.ENGINES and engine.ENGINES["afm"].model == "afm"
    assert engine.ENGINES["afm"].use_bias_tables is False
    assert "AFMLayer" in layers.__all__
    fwd, bwd = engine.AFMEngine.afm_flops(65536, 26, 16, 8)
    assert fwd == 65536 * 325 * (16 + 2 * 16 * 8 + 2 * 8 + 2 * 16) and bwd > 2 * fwd


def test_header_declares_and_library_exports_the_kernels(hip_lib):
    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    for name in ("rm_afm_supported", "rm_afm_fwd", "rm_afm_bwd", "rm_afm_bwd_workspace"):
        assert name + "(" in text and hasattr(hip_lib, name), name
    # the supported set, asked without a GPU
    assert hip_lib.rm_afm_supported(26, 16, 8) == 1 and hip_lib.rm_afm_supported(40, 64, 64) == 1
    for F, D, T in ((26, 12, 8), (1, 16, 8), (41, 16, 8), (26, 16, 65), (26, 16, 0)):
        assert hip_lib.rm_afm_supported(F, D, T) == 0
        assert hip_lib.rm_afm_bwd_workspace(64, F, D, T) == 0
    assert hip_lib.rm_afm_bwd_workspace(64, 26, 16, 8) > 0


def test_ops_reject_host_tensors_before_any_launch(hip_lib):
    from recman_amd import ops

    with pytest.raises(ValueError):
        ops.afm_fwd(torch.zeros(2, 3, 8), torch.zeros(8, 4), torch.zeros(4), torch.zeros(4), torch.zeros(8),
                    torch.zeros(2))
