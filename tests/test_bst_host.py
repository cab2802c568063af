"""CPU: the transformer-pooled sequence lookup without a GPU - the restatement of tests/bst_ref.py against
torch.nn.TransformerEncoderLayer, its autograd against finite differences, the kink guard's cap, the T = 1 and
position-by-recency semantics, and the host side of the public surface (th.BST, ENGINES, the header, ops' checks)."""
import inspect
import os

import pytest
import torch

from tests import bst_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _encoder_layer(p, heads):
    """torch.nn.TransformerEncoderLayer (double, dropout 0, post-norm) holding the case's parameters: its weights are
    [out, in], the project's [in, out]."""
    D, Hf = p["ffn_w1"].shape
    layer = torch.nn.TransformerEncoderLayer(D, heads, Hf, dropout=0.0, batch_first=True, norm_first=False).double()
    with torch.no_grad():
        layer.self_attn.in_proj_weight.copy_(torch.cat([p["wq"].T, p["wk"].T, p["wv"].T]))
        layer.self_attn.in_proj_bias.copy_(torch.cat([p["bq"], p["bk"], p["bv"]]))
        layer.self_attn.out_proj.weight.copy_(p["wo"].T)
        layer.self_attn.out_proj.bias.copy_(p["bo"])
        layer.linear1.weight.copy_(p["ffn_w1"].T)
        layer.linear1.bias.copy_(p["ffn_b1"])
        layer.linear2.weight.copy_(p["ffn_w2"].T)
        layer.linear2.bias.copy_(p["ffn_b2"])
        layer.norm1.weight.copy_(p["ln1_gamma"])
        layer.norm1.bias.copy_(p["ln1_beta"])
        layer.norm2.weight.copy_(p["ln2_gamma"])
        layer.norm2.bias.copy_(p["ln2_beta"])
    assert layer.norm1.eps == 1e-5 and layer.norm2.eps == 1e-5
    return layer.train()  # (dropout is 0; training mode keeps the layer on its plain, unfused path)


def _by_encoder_layer(case):
    """Per example: the tokens gathered and the position rows added by hand, the layer applied to the example's own T
    tokens (examples of one length share a call: no token of another example, no padding, no mask), the mean by hand."""
    D, p = case["D"], case["p"]
    T, off, ids, qidx = case["table"][:, :D], case["offsets"], case["ids"], case["qidx"]
    layer = _encoder_layer(p, case["heads"])
    n = (off[1:] - off[:-1]).tolist()
    out = torch.zeros(case["B"], D, dtype=F64)
    with torch.no_grad():
        for length in sorted(set(n)):
            bs = [b for b in range(case["B"]) if n[b] == length]
            toks = []
            for b in bs:
                rows = [T[ids[off[b] + i]] + p["pos"][length - i] for i in range(length)] + [T[qidx[b]] + p["pos"][0]]
                toks.append(torch.stack(rows))
            Z = layer(torch.stack(toks))                     # [examples, T, D]
            out[bs] = Z.sum(dim=1) / (length + 1)
    return out


@pytest.mark.parametrize("name", sorted(R.GPU_CASES))
def test_restatement_equals_torch_transformer_encoder_layer(name):
    case = R.make_bst_case(**R.GPU_CASES[name])
    got = R.layer_reference(case)[0]
    want = _by_encoder_layer(case)
    err = float((got - want).abs().max())
    print(f"{name}: restatement vs TransformerEncoderLayer {err:.2e}")
    assert err <= 1e-12, err


def test_an_example_without_history_gives_the_candidates_own_output_row():
    case = R.make_bst_case(**R.GPU_CASES["d16_h2_f64"])
    assert int(case["offsets"][1]) == 0
    out = R.layer_reference(case)[0]
    p, D = case["p"], case["D"]
    x = (case["table"][case["qidx"][0], :D] + p["pos"][0]).reshape(1, 1, D)
    with torch.no_grad():
        z0 = _encoder_layer(p, case["heads"])(x).reshape(D)
    assert float(z0.abs().max()) > 0.1 and float((out[0] - z0).abs().max()) <= 1e-12


def _small_case():
    return R.make_bst_case(B=5, D=8, heads=2, Hf=8, max_len=3, V=9, seed=5)


def test_autograd_of_the_restatement_matches_finite_differences():
    case = _small_case()
    assert case["zeroed"] == 0.0
    D = case["D"]
    _, d_keys, d_query, grads = R.layer_reference(case)
    d_query = d_query - case["dq_up"]
    Q0, K0 = case["table"][case["qidx"], :D].clone(), case["table"][case["ids"], :D].clone()

    def loss(Q, K, p):
        return float((R.bst_layer(Q, K, case["offsets"], p, case["heads"]) * case["g"]).sum())

    def fd(which, name=None):
        base = dict(Q=Q0, K=K0, p=dict(case["p"]))
        t = (base["p"][name] if which == "p" else base[which]).clone()
        g = torch.zeros_like(t)
        h = 1e-6
        for i in range(t.numel()):
            vals = []
            for sgn in (1.0, -1.0):
                u = t.clone()
                u.view(-1)[i] += sgn * h
                args = dict(base, p=dict(base["p"]))
                if which == "p":
                    args["p"][name] = u
                else:
                    args[which] = u
                vals.append(loss(args["Q"], args["K"], args["p"]))
            g.view(-1)[i] = (vals[0] - vals[1]) / (2 * h)
        return g

    checks = [("d_keys", d_keys, fd("K")), ("d_query", d_query, fd("Q"))]
    checks += [("d_" + n, grads[n], fd("p", n)) for n in ("wq", "ffn_w1", "pos", "ln1_gamma")]
    for name, a, b in checks:
        err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-3)
        print(f"{name}: autograd vs central differences {err:.2e}")
        assert float(b.abs().max()) > 0 and err <= 1e-6, (name, err)


def test_position_rows_are_indexed_by_distance_from_the_candidate():
    """One example, history of 3 of max_len 5: P[0..3] get gradient, P[4..5] none.  Dropping the OLDEST item (the
    history's start moves) leaves every remaining token its position row - and P[3] without gradient."""
    case = _small_case()
    D, p = case["D"], dict(case["p"])
    g = torch.Generator().manual_seed(1)
    p["pos"] = torch.randn(6, D, generator=g, dtype=F64)
    T = case["table"][:, :D]
    q, ids = T[:1], torch.tensor([4, 2, 7])

    def run(hist):
        P = p["pos"].clone().requires_grad_(True)
        off = torch.tensor([0, len(hist)])
        X, valid = R.bst_tokens(q, T[hist], off, P)
        R.bst_layer(q, T[hist], off, dict(p, pos=P), case["heads"]).sum().backward()
        return X.detach()[0], valid[0], P.grad.abs().sum(dim=1) > 0

    X3, v3, used3 = run(ids)
    assert used3.tolist() == [True, True, True, True, False, False] and v3.tolist() == [True] * 4 + [False] * 2
    X2, v2, used2 = run(ids[1:])
    assert used2.tolist() == [True, True, True, False, False, False] and v2.tolist() == [True] * 3 + [False] * 3
    assert torch.equal(X2[:3], X3[1:4])                      # aligned on recency, not on the history's start
    assert torch.equal(X3[3], q[0] + p["pos"][0]) and torch.equal(X3[0], T[4] + p["pos"][3])


@pytest.mark.parametrize("name", sorted(R.GPU_CASES))
def test_kink_guard_zeroes_at_most_a_fifth_of_every_gpu_case(name):
    case = R.make_bst_case(**R.GPU_CASES[name])
    n = case["offsets"][1:] - case["offsets"][:-1]
    assert n[:3].tolist() == [0, 1, case["max_len"]] and case["B"] % 32 != 0
    print(f"{name}: zeroed share {case['zeroed']:.4f}")
    assert case["zeroed"] <= R.KINK_CAP
    assert bool((case["g"][case["near"]] == 0).all()) and float(case["g"].abs().max()) > 0
    for t in [case["table"], case["g"], case["dq_up"]] + list(case["p"].values()):
        assert torch.equal(t, t.float().double())            # every input value is a float32 number
    for nme in ("bq", "bk", "bv", "bo", "ffn_b1", "ffn_b2", "ln1_beta", "ln2_beta", "pos"):
        assert float(case["p"][nme].abs().min()) > 0
    for nme in ("ln1_gamma", "ln2_gamma"):
        assert float((case["p"][nme] - 1).abs().min()) > 0


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_cases_have_no_ffn_unit_at_its_kink(name):
    k = R.make_model_case(**R.MODEL_CASES[name])
    print(f"{name}: closest FFN pre-activation {k['min_abs_z']:.2e}")
    assert k["min_abs_z"] > R.KINK
    assert {"hist_bst_" + n for n in R.NAMES} <= set(k["p"]) and "hist_feat_embed" not in k["p"]


@pytest.mark.parametrize("name", R.RANGE_CASES)
def test_large_scores_case_is_out_of_fp32_exp_range_and_float32_stays_finite(name):
    """wq x RANGE_SCALE: scores beyond 88.7, where an un-subtracted fp32 exp overflows; the float32 restatement is
    finite there, so RANGE_SCALE itself (and no smaller power of ten) is the scale of the GPU test."""
    case = R.make_bst_case(**R.GPU_CASES[name], wq_scale=R.RANGE_SCALE)
    D, p, h = case["D"], case["p"], case["heads"]
    X, valid = R.bst_tokens(case["table"][case["qidx"], :D], case["table"][case["ids"], :D], case["offsets"], p["pos"])
    q, k = X @ p["wq"] + p["bq"], X @ p["wk"] + p["bk"]
    B, Tm = X.shape[:2]
    split = lambda t: t.reshape(B, Tm, h, D // h).transpose(1, 2)  # noqa: E731
    s = (split(q) @ split(k).transpose(2, 3)) / (D // h) ** 0.5
    s = s[(valid[:, None, :, None] & valid[:, None, None, :]).expand_as(s)]
    print(f"{name}: largest score {float(s.max()):.1f}")
    assert float(s.max()) > 89.0
    res = R.layer_reference(case, dtype=torch.float32)
    for t in list(res[:3]) + list(res[3].values()):
        assert bool(torch.isfinite(t).all())
    assert case["zeroed"] <= R.KINK_CAP


# ------------------------------------------------------------------------------------------- the public surface
def _dict(max_len=4):
    import recman_amd.th as th

    fd = th.FeatureDictionary()
    fd["user"] = th.SparseFeat("user", 7)
    item = fd["item"] = th.SparseFeat("item", 20)
    fd["hist"] = th.SequenceFeat("hist", item, max_len=max_len)
    return th, fd


def test_bst_constructor_follows_din_and_returns_its_params():
    from sklearn.base import clone
    from sklearn.metrics import log_loss, roc_auc_score

    from recman_amd import engine

    th, fd = _dict()
    params = list(inspect.signature(th.BST.__init__).parameters.values())[1:]
    want = [("feat_dict", inspect.Parameter.empty), ("embedding_size", 8), ("att_head_num", 2), ("att_ffn_units", None),
            ("deep_hidden_units", (32, 32)), ("deep_dropout", (0.6, 0.6, 0.6)), ("deep_l2_reg", 0.0),
            ("deep_activation", "relu"), ("epoch", 10), ("batch_size", 256), ("learning_rate", 0.001),
            ("optimizer", "adam"), ("random_seed", 2019), ("loss_type", "logloss"),
            ("eval_metric", (roc_auc_score, log_loss)), ("l2_reg", 0.1), ("what_means_greater", None),
            ("use_interactive_session", True), ("log_dir", "./logs"), ("strict_reference", False), ("device", "cuda")]
    assert [(p.name, p.default) for p in params] == want
    assert "BST" in th.__all__ and th.BST.model == "bst"
    m = th.BST(fd, embedding_size=16, att_head_num=4, att_ffn_units=24)
    got = m.get_params()
    for k, _ in want[1:]:
        assert k in got, k
    assert got["embedding_size"] == 16 and got["att_head_num"] == 4 and got["att_ffn_units"] == 24
    c = clone(m)
    assert isinstance(c, th.BST) and c.get_params()["att_ffn_units"] == 24 and c._engine is None
    e = engine.ENGINES["bst"]
    assert e.model == "bst" and issubclass(e, engine.DINEngine) and not e.shardable and not e.use_bias_tables
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="[Ss]equence features"):
        m._build()


def test_header_declares_and_library_exports_the_kernels(hip_lib):
    from recman_amd import _lib

    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    for name in ("rm_bst_supported", "rm_bst_fwd", "rm_bst_bwd", "rm_bst_workspace"):
        assert name + "(" in text and hasattr(hip_lib, name), name
    assert "typedef struct rm_bst_params" in text
    for n in _lib.BST_PARAM_NAMES:
        assert f"*{n}" in text, n                            # the binding's member order is the header's
    assert tuple(_lib.BST_PARAM_NAMES) == R.NAMES
    for D in (8, 16, 32):
        for h in (1, 2, 4, 8):
            for Hf in (4, 20, 64, 128):
                for ml in (1, 20, 63):
                    assert hip_lib.rm_bst_supported(D, h, Hf, ml) == (1 if D // h >= 4 else 0), (D, h, Hf, ml)
    for D, h, Hf, ml in ((12, 2, 64, 10), (64, 2, 64, 10), (16, 3, 64, 10), (8, 4, 32, 10), (16, 2, 130, 10),
                         (16, 2, 6, 10), (16, 2, 0, 10), (16, 2, 132, 10), (16, 2, 64, 64), (16, 2, 64, 0)):
        assert hip_lib.rm_bst_supported(D, h, Hf, ml) == 0, (D, h, Hf, ml)
        assert hip_lib.rm_bst_workspace(D, h, Hf, ml, 100, 1) == 0
    assert 0 < hip_lib.rm_bst_workspace(16, 2, 64, 20, 1000, 0) < hip_lib.rm_bst_workspace(16, 2, 64, 20, 1000, 1)


def test_ops_reject_host_tensors_and_bad_parameter_sets_before_any_launch(hip_lib):
    from recman_amd import ops

    z = torch.zeros
    i64 = torch.int64
    p = {n: z(*s) for n, s in ops.bst_param_shapes(8, 16, 3).items()}
    assert list(p) == list(ops.BST_PARAM_NAMES) and p["pos"].shape == (4, 8) and p["ffn_w2"].shape == (16, 8)
    with pytest.raises(ValueError, match="GPU"):
        ops.bst_fwd(z(5, 16), 0, 8, z(3, dtype=i64), z(4, dtype=i64), z(2, dtype=i64), p, 2, 3, z(2, 16), z(1000))
    with pytest.raises(ValueError):
        ops.bst_bwd(z(5, 16), 0, 8, z(3, dtype=i64), z(4, dtype=i64), z(2, dtype=i64), p, 2, 3, z(2, 8), z(4, 8),
                    z(2, 8), p, z(1000))
    with pytest.raises(ValueError, match="ffn_w1"):
        ops.bst_fwd(z(5, 16), 0, 8, z(3, dtype=i64), z(4, dtype=i64), z(2, dtype=i64), {"wq": z(8, 8)}, 2, 3, z(2, 16),
                    z(1000))
