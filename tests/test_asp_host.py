"""CPU: SequenceFeat encoding, the DIN surface, and tests/asp_ref.py (the float64 restatement of the attention-pooled
sequence lookup) pinned against an independent per-example numpy loop and against finite differences.  The kink
guard's cap is asserted here for every GPU case of tests/test_gpu_asp.py."""
import inspect
import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests import asp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ SequenceFeat
def _item_feat():
    import recman_amd.th as th

    item = th.SparseFeat("item", 5)
    item.initialize(np.array(["a", "b", "c", "d", "e"], dtype=object))  # a..e -> 1..5, unseen -> 0
    return th, item


def test_sequence_feat_encoding_truncation_padding_unknown_and_empty():
    th, item = _item_feat()
    seq = th.SequenceFeat("hist", item, max_len=3)
    assert seq.feat_size == 0 and seq.encoder is item.encoder and seq.get_shape(for_tf=False) == (-1, 3)
    col = pd.Series([["a", "b", "c", "d", "e"], ["b"], [], None, float("nan"), ["zz", "a"], ["e", "e", "e"]])
    arr = seq(col)
    assert arr.dtype == np.int64 and arr.shape == (7, 3)
    assert arr.tolist() == [[3, 4, 5],      # longer than max_len: the LAST max_len items
                            [2, 0, 0],      # zero-padded at the end
                            [0, 0, 0], [0, 0, 0], [0, 0, 0],   # [], None, NaN
                            [0, 1, 0],      # an unseen item encodes to 0 and stays in its place
                            [5, 5, 5]]
    csr = seq.encode(col)
    assert type(csr).__name__ == "CSR"
    assert csr.offsets.tolist() == [0, 3, 4, 4, 4, 4, 6, 9]      # true lengths min(len, max_len); empty cells 0
    assert csr.ids.tolist() == [3, 4, 5, 2, 0, 1, 5, 5, 5]        # the unknown item (0) is inside the true length
    n = np.diff(csr.offsets)
    for b in range(7):                                            # padded array versus CSR
        assert arr[b, : n[b]].tolist() == csr.ids[csr.offsets[b]: csr.offsets[b + 1]].tolist()
        assert not arr[b, n[b]:].any()
    assert csr.vals is None and len(csr) == 7
    # numeric ids go through the numeric branch of the shared encoder
    num = th.SparseFeat("n", 3)
    num.initialize(np.array([10, 20, 30]))
    assert th.SequenceFeat("h", num, max_len=4)(pd.Series([[30, 10, 99], []])).tolist() == [[3, 1, 0, 0], [0, 0, 0, 0]]


def test_data_inputs_carry_the_history_as_csr_and_check_its_range():
    th, item = _item_feat()
    fd = th.FeatureDictionary()
    fd["item"] = item
    fd["hist"] = th.SequenceFeat("hist", item, max_len=2)
    fd["x"] = th.DenseFeat("x")
    df = pd.DataFrame({"item": ["a", "e"], "hist": [["b", "c", "d"], []], "x": [0.5, 1.5]})
    fd["x"].initialize(df["x"])
    assert [f.name for f in fd.sequence_feats] == ["hist"] and fd["hist"] in fd.embedding_feats
    assert fd["hist"] not in fd.linear_feats and fd["hist"] not in fd.sparse_feats
    inp = th.DataInputs().load(fd, df)
    assert inp.idx.tolist() == [[1, 0], [5, 0]] and inp["hist"].tolist() == [[3, 4], [0, 0]]
    assert inp.mv["hist"].offsets.tolist() == [0, 2, 2] and inp.mv["hist"].ids.tolist() == [3, 4]
    perm = inp.mv["hist"].take(np.array([1, 0]))
    assert perm.offsets.tolist() == [0, 0, 2] and perm.ids.tolist() == [3, 4]
    small = th.SparseFeat("item", 2, encoder=item.encoder)   # declared smaller than the fitted vocabulary
    fd2 = th.FeatureDictionary()
    fd2["item"] = small
    fd2["hist"] = th.SequenceFeat("hist", small, max_len=2)
    with pytest.raises(ValueError, match="hist"):
        th.DataInputs().load(fd2, pd.DataFrame({"item": ["a"], "hist": [["e"]]}))


def test_check_supported_accepts_and_rejects():
    th, item = _item_feat()
    fd = th.FeatureDictionary()
    fd["item"] = item
    fd["hist"] = th.SequenceFeat("hist", item)
    fd.check_supported()
    other = th.SparseFeat("item", 5)                       # same name, but not the dictionary's feature
    fd["hist2"] = th.SequenceFeat("hist2", other)
    with pytest.raises(ValueError, match="hist2"):
        fd.check_supported()
    del fd["hist2"]
    fd["hist3"] = th.SequenceFeat("hist3", th.MultiValCsvFeat("tags", ("a", "b")))
    with pytest.raises(ValueError, match="hist3"):
        fd.check_supported()
    del fd["hist3"]

    class Foreign:
        name, feat_size = "q", 4

    fd["q"] = Foreign()
    with pytest.raises(NotImplementedError):
        fd.check_supported()


# ----------------------------------------------------------------------------------------------------- surface
def _din_dict():
    th, item = _item_feat()
    fd = th.FeatureDictionary()
    fd["item"] = item
    fd["hist"] = th.SequenceFeat("hist", item, max_len=4)
    return th, fd


def test_din_constructor_has_the_reference_signature_and_returns_its_params():
    from sklearn.metrics import log_loss, roc_auc_score

    th, fd = _din_dict()
    params = list(inspect.signature(th.DIN.__init__).parameters.values())[1:]
    want = [("feat_dict", inspect.Parameter.empty), ("embedding_size", 8), ("att_hidden_units", (80, 40)),
            ("att_activation", "sigmoid"), ("att_dropout", (1, 1, 1)), ("att_weight_normalization", False),
            ("deep_hidden_units", (32, 32)), ("deep_dropout", (0.6, 0.6, 0.6)), ("deep_l2_reg", 0.0),
            ("deep_activation", "relu"), ("epoch", 10), ("batch_size", 256), ("learning_rate", 0.001),
            ("optimizer", "adam"), ("random_seed", 2019), ("loss_type", "logloss"),
            ("eval_metric", (roc_auc_score, log_loss)), ("l2_reg", 0.1), ("what_means_greater", None),
            ("use_interactive_session", True), ("log_dir", "./logs"), ("strict_reference", False), ("device", "cuda")]
    assert [(p.name, p.default) for p in params] == want
    assert "DIN" in th.__all__ and "SequenceFeat" in th.__all__ and th.DIN.model == "din"
    m = th.DIN(fd, embedding_size=16, att_hidden_units=(36,), att_weight_normalization=True, l2_reg=0.3)
    got = m.get_params()
    for k, default in want[1:]:
        assert k in got, k
    assert got["embedding_size"] == 16 and got["att_hidden_units"] == (36,) and got["l2_reg"] == 0.3
    assert got["att_weight_normalization"] is True and got["deep_dropout"] == (0.6, 0.6, 0.6)
    from recman_amd import engine

    assert engine.ENGINES["din"].model == "din" and engine.ENGINES["din"].use_bias_tables is False


def test_din_rejects_dice_dropout_and_row_sharding():
    th, fd = _din_dict()
    with pytest.raises(NotImplementedError, match="activation.py"):
        th.DIN(fd, att_activation="dice")
    with pytest.raises(NotImplementedError, match="att_dropout"):
        th.DIN(fd, att_dropout=(1, 0.9, 1))
    m = th.DIN(fd)
    m.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="[Ss]equence features"):
        m._build()
    d = th.DCN(fd)
    d.hparams["table_sharding"] = "row"
    with pytest.raises(NotImplementedError, match="[Ss]equence features"):
        d._build()


def test_feature_spec_names_the_query_field_and_counts_sequences_as_scratch_rows():
    from recman_amd.engine import FeatureSpec

    s = FeatureSpec(["a", "item", "hist"], [4, 6, 0], ["x"], seq_query={"hist": "item"}, seq_max_len={"hist": 12})
    assert s.seq_names == ["hist"] and s.scratch_names == ["hist"] and s.seq_max_len == {"hist": 12}
    assert s.rows == 10 and s.offsets() == [0, 4, 10]
    assert FeatureSpec(["a"], [4]).seq_query == {} and FeatureSpec(["a"], [4]).scratch_names == []
    with pytest.raises(ValueError):
        FeatureSpec(["a", "hist"], [4, 3], seq_query={"hist": "a"})       # a sequence owns no rows
    with pytest.raises(ValueError):
        FeatureSpec(["a", "hist"], [4, 0], seq_query={"hist": "nope"})
    with pytest.raises(ValueError):
        FeatureSpec(["a", "h1", "h2"], [4, 0, 0], seq_query={"h1": "a", "h2": "h1"})


def test_header_declares_and_library_exports_the_kernels(hip_lib):
    import ctypes

    text = open(os.path.join(ROOT, "include", "recman_hip.h")).read()
    for name in ("rm_asp_supported", "rm_asp_fwd", "rm_asp_bwd", "rm_asp_workspace"):
        assert name + "(" in text and hasattr(hip_lib, name), name
    arr = lambda *h: (ctypes.c_int * len(h))(*h)  # noqa: E731
    for D in (8, 16, 32):
        for h in ((80, 40), (36,), (16, 8), (128, 128), (1,), (128,)):
            for max_len in (1, 10, 256):
                assert hip_lib.rm_asp_supported(D, len(h), arr(*h), max_len) == 1, (D, h, max_len)
    for D, h, max_len in ((12, (80, 40), 10), (64, (80, 40), 10), (16, (129,), 10), (16, (80, 0), 10),
                          (16, (80, 40), 257), (16, (80, 40), 0)):
        assert hip_lib.rm_asp_supported(D, len(h), arr(*h), max_len) == 0, (D, h, max_len)
    assert hip_lib.rm_asp_supported(16, 3, arr(8, 8, 8), 10) == 0 and hip_lib.rm_asp_supported(16, 0, arr(8), 10) == 0
    assert hip_lib.rm_asp_workspace(16, 2, arr(80, 40), 1000, 0) > 0
    assert hip_lib.rm_asp_workspace(16, 2, arr(80, 40), 1000, 1) > hip_lib.rm_asp_workspace(16, 2, arr(80, 40), 1000, 0)
    assert hip_lib.rm_asp_workspace(12, 2, arr(80, 40), 1000, 1) == 0


def test_ops_reject_host_tensors_before_any_launch(hip_lib):
    from recman_amd import ops

    z = torch.zeros
    with pytest.raises(ValueError):
        ops.asp_fwd(z(5, 16), 0, 8, z(3, dtype=torch.int64), z(4, dtype=torch.int64), z(2, dtype=torch.int64),
                    [z(32, 6)], [z(6)], z(6), z(1), "sigmoid", False, z(2, 16), z(4), z(1000))


# ------------------------------------------------------------------------- the restatement against a numpy loop
def _numpy_loop(case):
    """Per example, per position, with numpy only: nothing shared with asp_ref but the inputs."""
    D = case["D"]
    T = case["table"].numpy()[:, :D]
    Ws, bs = [W.numpy() for W in case["Ws"]], [b.numpy() for b in case["bs"]]
    w, w0 = case["w"].numpy().reshape(-1), float(case["w0"])
    off, ids, qidx = case["offsets"].numpy(), case["ids"].numpy(), case["qidx"].numpy()
    f = (lambda v: np.maximum(v, 0.0)) if case["act"] == "relu" else (lambda v: 1.0 / (1.0 + np.exp(-v)))
    out = np.zeros((case["B"], D))
    for b in range(case["B"]):
        q = T[qidx[b]]
        s, ks = [], []
        for t in range(off[b], off[b + 1]):
            k = T[ids[t]]
            h = np.concatenate([q, k, q - k, q * k])
            for W, bb in zip(Ws, bs):
                h = f(h @ W + bb)
            s.append(float(h @ w) + w0)
            ks.append(k)
        if not s:
            continue
        s = np.array(s)
        if case["norm"]:
            e = np.exp(s - s.max())
            s = e / e.sum()
        out[b] = (s[:, None] * np.array(ks)).sum(axis=0)
    return out


@pytest.mark.parametrize("name", ["d16_80x40_sigmoid", "d16_80x40_relu_norm", "d8_36_relu", "d8_36_sigmoid_norm",
                                  "d32_16x8_sigmoid_norm", "d32_128x64_sigmoid"])
def test_restatement_equals_a_per_example_numpy_loop(name):
    case = R.make_asp_case(**R.GPU_CASES[name])
    want = _numpy_loop(case)
    got = R.layer_reference(case)[0].numpy()
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    n = np.diff(case["offsets"].numpy())
    assert n[0] == 0 and n[1] == 1 and n[2] == case["max_len"] and not got[0].any()
    o2 = int(case["offsets"][2])
    assert int(case["ids"][o2]) == int(case["ids"][o2 + 1])  # the repeated id


def test_large_scores_case_is_out_of_fp32_exp_range_and_still_matches_the_loop():
    for name, kw in R.RANGE_CASES.items():
        case = R.make_asp_case(**kw, w_scale=R.RANGE_SCALE)
        D = case["D"]
        s = R.asp_scores(case["table"][case["qidx"], :D], case["table"][case["ids"], :D], case["offsets"], case["Ws"],
                         case["bs"], case["w"], case["w0"], case["act"])
        assert float(s.max() - s.min()) > 100.0, name   # exp of the raw scores' spread overflows fp32
        assert float(s.abs().max()) > 89.0, name
        want = _numpy_loop(case)
        assert np.abs(R.layer_reference(case)[0].numpy() - want).max() <= 1e-11 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("act,norm,hidden", [("sigmoid", False, (5, 3)), ("sigmoid", True, (5, 3)),
                                             ("relu", True, (6,)), ("relu", False, (5, 3))])
def test_autograd_of_the_restatement_matches_finite_differences(act, norm, hidden):
    case = R.make_asp_case(B=6, D=8, hidden=hidden, act=act, norm=norm, max_len=4, V=9, seed=5)
    assert case["zeroed"] == 0.0  # (relu: no unit near its kink, so central differences are valid)
    D = case["D"]
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    Q, K = leaf(case["table"][case["qidx"], :D]), leaf(case["table"][case["ids"], :D])
    Ws, bs, w, w0 = [leaf(W) for W in case["Ws"]], [leaf(b) for b in case["bs"]], leaf(case["w"]), leaf(case["w0"])
    m = len(Ws)

    def fn(Q, K, w, w0, *rest):
        return R.asp_layer(Q, K, case["offsets"], list(rest[:m]), list(rest[m:]), w, w0, act, norm)

    assert torch.autograd.gradcheck(fn, (Q, K, w, w0, *Ws, *bs), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_model_restatement_uses_the_query_features_rows_for_the_history():
    k = R.make_model_case(**R.MODEL_CASES["din_d8"])
    p, spec, idx, dense, y, hp, mv = (k[n] for n in ("p", "spec", "idx", "dense", "y", "hp", "mv"))
    assert "hist_feat_embed" not in p and spec.tl.sparse_names == ["C0", "item", "C2"]
    loss, logit, pred, grads = R.fwd_bwd("din", p, spec, idx, dense, y, hp, mv)
    assert set(grads) == set(p) and logit.shape == (idx.shape[0],)
    # a row that is a target in one example and a history item in another gets both gradients
    both = set(idx[:, 1].tolist()) & set(mv["hist"][1].tolist())
    assert both
    E = R.embeddings(p, spec, idx, mv, hp)
    n = mv["hist"][0][1:] - mv["hist"][0][:-1]
    assert bool((E[n == 0, 2] == 0).all()) and float(E[n > 0, 2].abs().max()) > 0
    # the history's placeholder column of idx plays no part
    idx2 = idx.clone()
    idx2[:, 2] = 3
    assert torch.equal(R.model_logit("din", p, spec, idx2, dense, hp, mv), R.model_logit("din", p, spec, idx, dense, hp, mv))


# ------------------------------------------------------------------------------------------- the kink guard
@pytest.mark.parametrize("name", sorted(R.GPU_CASES) + ["range:" + n for n in sorted(R.RANGE_CASES)])
def test_kink_guard_zeroes_at_most_a_fifth_of_every_gpu_case(name):
    if name.startswith("range:"):
        k = R.make_asp_case(**R.RANGE_CASES[name[6:]], w_scale=R.RANGE_SCALE)
    else:
        k = R.make_asp_case(**R.GPU_CASES[name])
    assert k["zeroed"] <= R.KINK_CAP, k["zeroed"]
    assert bool((k["g"][k["near"]] == 0).all()) and bool((k["g"][~k["near"]] != 0).all())
    if k["act"] != "relu":
        assert k["zeroed"] == 0.0


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_cases_have_no_attention_unit_at_its_kink(name):
    k = R.make_model_case(**R.MODEL_CASES[name])
    if k["hp"]["att_activation"] == "relu":
        assert k["min_abs_z"] >= R.KINK
