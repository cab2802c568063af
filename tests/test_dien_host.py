"""CPU: the interest-evolution sequence lookup without a GPU - the extractor of tests/dien_ref.py against torch.nn.GRU,
the restatement's autograd against central differences, the n = 0 / n = 1 and batch-independence semantics, the range
cases' reach, and the host side of the public surface (th.DIEN, ENGINES, the header, ops' checks)."""
import inspect
import os

import pytest
import torch

from tests import dien_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _torch_gru(p, D):
    """torch.nn.GRU (double) holding the extractor's parameters.  torch: h' = (1 - z) n + z h, so its z is 1 - u: the
    z-block is -Wu^T, -Uu^T, -bu; the r- and n-blocks are plain transposes ([out, in] against the project's [in, out]);
    torch's n = tanh(W x + b_in + r * (U h + b_hn)) has the project's single bias with bias_hh = 0.  Gate order r, z, n."""
    gru = torch.nn.GRU(D, D, batch_first=True).double()
    W, U, b = p["gru_w"], p["gru_u"], p["gru_b"]
    blk = lambda t, g: t[..., g * D:(g + 1) * D]  # noqa: E731
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.cat([blk(W, 1).T, -blk(W, 0).T, blk(W, 2).T]))
        gru.weight_hh_l0.copy_(torch.cat([blk(U, 1).T, -blk(U, 0).T, blk(U, 2).T]))
        gru.bias_ih_l0.copy_(torch.cat([blk(b, 1), -blk(b, 0), blk(b, 2)]))
        gru.bias_hh_l0.zero_()
    return gru


@pytest.mark.parametrize("name", ["d16", "d8_long", "d32", "d8_many"])
def test_extractor_equals_torch_gru(name):
    case = R.make_dien_case(**R.GPU_CASES[name])
    D, off = case["D"], case["offsets"]
    T = case["table"][:, :D]
    tr = R.dien_trace(T[case["qidx"]], T[case["ids"]], off, case["p"])
    gru = _torch_gru(case["p"], D)
    worst = 0.0
    with torch.no_grad():
        for b in range(min(case["B"], 12)):
            n = int(off[b + 1] - off[b])
            if n == 0:
                continue
            want = gru(T[case["ids"][off[b]: off[b + 1]]].unsqueeze(0))[0][0]
            worst = max(worst, float((tr["H"][b, :n] - want).abs().max()))
    print(f"{name}: extractor vs torch.nn.GRU {worst:.2e}")
    assert worst <= 1e-12


def test_one_history_item_gives_one_augru_step_with_weight_one():
    case = R.make_dien_case(**R.GPU_CASES["d16"])
    assert int(case["offsets"][2] - case["offsets"][1]) == 1
    D, p = case["D"], case["p"]
    k = case["table"][case["ids"][int(case["offsets"][1])], :D].unsqueeze(0)
    zero = torch.zeros(1, D, dtype=F64)
    h1 = R.cell(k, zero, p["gru_w"], p["gru_u"], p["gru_b"])
    want = R.cell(h1, zero, p["augru_w"], p["augru_u"], p["augru_b"], torch.ones(1, dtype=F64))
    out = R.layer_reference(case)[0]
    assert float(want.abs().max()) > 1e-3 and float((out[1] - want[0]).abs().max()) <= 1e-15
    # one position: the softmax weight is 1 whatever the query is, so the query gets no gradient there
    dq = R.layer_reference(case)[2] - case["dq_up"]
    assert float(dq[1].abs().max()) == 0.0 and float(dq[2].abs().max()) > 0


def test_no_history_gives_a_zero_row_and_no_gradient():
    case = R.make_dien_case(**R.GPU_CASES["d16"])
    assert int(case["offsets"][1]) == 0
    out, _, d_query, _ = R.layer_reference(case)
    assert float(out[0].abs().max()) == 0.0 and float((d_query - case["dq_up"])[0].abs().max()) == 0.0
    B, D = case["B"], case["D"]
    empty = dict(case, offsets=torch.zeros(B + 1, dtype=torch.int64), ids=torch.zeros(0, dtype=torch.int64))
    out, d_keys, d_query, grads = R.layer_reference(empty)
    assert float(out.abs().max()) == 0.0 and d_keys.shape == (0, D) and torch.equal(d_query, case["dq_up"])
    assert all(float(g.abs().max()) == 0.0 for g in grads.values())


def test_an_example_does_not_change_when_longer_examples_join_its_batch():
    case = R.make_dien_case(**R.GPU_CASES["d16"])
    D, off = case["D"], case["offsets"]
    T = case["table"][:, :D]
    full = R.dien_layer(T[case["qidx"]], T[case["ids"]], off, case["p"])
    n = off[1:] - off[:-1]
    b = next(i for i in range(3, case["B"]) if 1 < int(n[i]) < case["max_len"])
    alone = R.dien_layer(T[case["qidx"][b: b + 1]], T[case["ids"][off[b]: off[b + 1]]],
                         torch.tensor([0, int(n[b])]), case["p"])
    assert int(n.max()) > int(n[b]) and float((full[b] - alone[0]).abs().max()) <= 1e-15


def _small_case():
    return R.make_dien_case(B=5, D=8, max_len=3, V=9, seed=5)


def test_autograd_of_the_restatement_matches_finite_differences():
    case = _small_case()
    D = case["D"]
    _, d_keys, d_query, grads = R.layer_reference(case)
    d_query = d_query - case["dq_up"]
    Q0, K0 = case["table"][case["qidx"], :D].clone(), case["table"][case["ids"], :D].clone()

    def loss(Q, K, p):
        return float((R.dien_layer(Q, K, case["offsets"], p) * case["g"]).sum())

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
    checks += [("d_" + n, grads[n], fd("p", n)) for n in ("gru_u", "gru_b", "att_w", "augru_w", "augru_u", "augru_b")]
    for name, a, b in checks:
        err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-3)
        print(f"{name}: autograd vs central differences {err:.2e}")
        assert float(b.abs().max()) > 0 and err <= 1e-6, (name, err)


@pytest.mark.parametrize("name", sorted(R.GPU_CASES))
def test_gpu_cases_are_what_the_kernel_tests_assume(name):
    case = R.make_dien_case(**R.GPU_CASES[name])
    n = case["offsets"][1:] - case["offsets"][:-1]
    assert n[:3].tolist() == [0, 1, case["max_len"]] and all(case["B"] % k for k in (16, 32, 64))
    assert int(n.max()) <= case["max_len"]
    for t in [case["table"], case["g"], case["dq_up"]] + list(case["p"].values()):
        assert torch.equal(t, t.float().double())            # every input value is a float32 number
    assert all(float(v.abs().min()) > 0 for v in case["p"].values())
    assert float(case["table"][:, case["D"]:].abs().min()) > 0  # junk behind column D


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_cases_carry_the_units_variables(name):
    k = R.make_model_case(**R.MODEL_CASES[name])
    assert {"hist_dien_" + n for n in R.NAMES} <= set(k["p"]) and "hist_feat_embed" not in k["p"]
    assert k["hp"]["seq_pooling"] == "dien"


@pytest.mark.parametrize("name", sorted(R.RANGE_CASES))
def test_range_cases_leave_the_fp32_exp_range_and_float32_stays_finite(name):
    """att_w x RANGE_SCALE: score differences beyond 88.7 inside an example, where a softmax without the maximum
    subtracted overflows; biases of +-100: pre-activations where (e^2x - 1) / (e^2x + 1) is inf / inf."""
    case = R.make_dien_case(**R.RANGE_CASES[name], att_scale=R.RANGE_SCALE, big_bias=True)
    D, p = case["D"], case["p"]
    for g in ("gru_b", "augru_b"):
        assert p[g][0::4].tolist() == [R.BIG_BIAS] * (3 * D // 4) and p[g][2::4].tolist() == [-R.BIG_BIAS] * (3 * D // 4)
    T = case["table"][:, :D]
    tr = R.dien_trace(T[case["qidx"]], T[case["ids"]], case["offsets"], p)
    s = tr["s"]
    spread = (s.masked_fill(~tr["valid"], float("-inf")).amax(1) - s.masked_fill(~tr["valid"], float("inf")).amin(1))
    spread = spread[tr["valid"].sum(1) > 1]
    print(f"{name}: largest score difference inside an example {float(spread.max()):.1f}")
    assert float(spread.max()) > 89.0
    for pre in (tr["pre_gru"], tr["pre_augru"]):
        big = pre[tr["valid"]][:, 0::2]
        print(f"{name}: smallest |pre-activation| of a +-100 unit {float(big.abs().min()):.1f}")
        assert float(big.abs().min()) > 89.0
    res = R.layer_reference(case, dtype=torch.float32)
    for t in list(res[:3]) + list(res[3].values()):
        assert bool(torch.isfinite(t).all())
    assert float(R.layer_reference(case)[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------- the public surface
def _dict(max_len=4):
    import recman_amd.th as th

    fd = th.FeatureDictionary()
    fd["user"] = th.SparseFeat("user", 7)
    item = fd["item"] = th.SparseFeat("item", 20)
    fd["hist"] = th.SequenceFeat("hist", item, max_len=max_len)
    return th, fd


def test_dien_constructor_follows_bst_and_returns_its_params():
    from sklearn.base import clone
    from sklearn.metrics import log_loss, roc_auc_score

    from recman_amd import engine

    th, fd = _dict()
    params = list(inspect.signature(th.DIEN.__init__).parameters.values())[1:]
    want = [("feat_dict", inspect.Parameter.empty), ("embedding_size", 8),
            ("deep_hidden_units", (32, 32)), ("deep_dropout", (0.6, 0.6, 0.6)), ("deep_l2_reg", 0.0),
            ("deep_activation", "relu"), ("epoch", 10), ("batch_size", 256), ("learning_rate", 0.001),
            ("optimizer", "adam"), ("random_seed", 2019), ("loss_type", "logloss"),
            ("eval_metric", (roc_auc_score, log_loss)), ("l2_reg", 0.1), ("what_means_greater", None),
            ("use_interactive_session", True), ("log_dir", "./logs"), ("strict_reference", False), ("device", "cuda")]
    assert [(p.name, p.default) for p in params] == want
    bst = [p.name for p in list(inspect.signature(th.BST.__init__).parameters.values())[1:]]
    assert [n for n in bst if n not in ("att_head_num", "att_ffn_units")] == [n for n, _ in want]
    assert "DIEN" in th.__all__ and th.DIEN.model == "dien"
    m = th.DIEN(fd, embedding_size=16, deep_hidden_units=(24, 8))
    got = m.get_params()
    for k, _ in want[1:]:
        assert k in got, k
    assert got["embedding_size"] == 16 and got["deep_hidden_units"] == (24, 8)
    c = clone(m)
    assert isinstance(c, th.DIEN) and c.get_params()["deep_hidden_units"] == (24, 8) and c._engine is None
    e = engine.ENGINES["dien"]
    assert e.model == "dien" and issubclass(e, engine.DINEngine) and not e.shardable and not e.use_bias_tables
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="[Ss]equence features"):
        m._build()


def test_header_declares_and_library_exports_the_kernels(hip_lib):
    from recman_amd import _lib

    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    for name in ("rm_dien_supported", "rm_dien_fwd", "rm_dien_bwd", "rm_dien_workspace"):
        assert name + "(" in text and hasattr(hip_lib, name), name
    assert "typedef struct rm_dien_params" in text
    body = text[text.index("typedef struct rm_dien_params"): text.index("} rm_dien_params;")]
    where = [body.index(f"*{n}") for n in _lib.DIEN_PARAM_NAMES]
    assert where == sorted(where)                            # the binding's member order is the header's
    assert tuple(_lib.DIEN_PARAM_NAMES) == R.NAMES
    assert [n for n, _ in _lib.DienParams._fields_] == list(R.NAMES)
    for D in (8, 16, 32):
        for ml in (1, 2, 20, 63, 64, 255, 256):
            assert hip_lib.rm_dien_supported(D, ml) == 1, (D, ml)
    for D, ml in ((12, 10), (64, 10), (4, 10), (0, 10), (24, 10), (16, 0), (16, 257), (16, -3), (8, 1000)):
        assert hip_lib.rm_dien_supported(D, ml) == 0, (D, ml)
        assert hip_lib.rm_dien_workspace(D, ml, 100, 1000, 1) == 0
    assert 0 < hip_lib.rm_dien_workspace(16, 20, 1000, 9000, 0) < hip_lib.rm_dien_workspace(16, 20, 1000, 9000, 1)
    assert hip_lib.rm_dien_workspace(16, 20, 0, 0, 1) > 0


def test_ops_reject_host_tensors_and_bad_parameter_sets_before_any_launch(hip_lib):
    from recman_amd import ops

    z = torch.zeros
    i64 = torch.int64
    p = {n: z(*s) for n, s in ops.dien_param_shapes(8).items()}
    assert list(p) == list(ops.DIEN_PARAM_NAMES) and p["gru_u"].shape == (8, 24) and p["augru_b"].shape == (24,)
    assert p["att_w"].shape == (8, 8) and "256" in ops.DIEN_LIMITS
    with pytest.raises(ValueError, match="GPU"):
        ops.dien_fwd(z(5, 16), 0, 8, z(3, dtype=i64), z(4, dtype=i64), z(2, dtype=i64), p, 3, True, z(2, 16), z(1000))
    with pytest.raises(ValueError):
        ops.dien_bwd(z(5, 16), 0, 8, z(3, dtype=i64), z(4, dtype=i64), z(2, dtype=i64), p, 3, z(2, 8), z(4, 8),
                     z(2, 8), p, z(1000))
    with pytest.raises(ValueError, match="gru_w"):
        ops.dien_fwd(z(5, 16), 0, 8, z(3, dtype=i64), z(4, dtype=i64), z(2, dtype=i64), {"att_w": z(8, 8)}, 3, True,
                     z(2, 16), z(1000))
