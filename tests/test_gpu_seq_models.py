"""GPU: sequence features in EVERY engine, under every pooling unit, against the float64 restatement of any model over
any front (tests/seq_models_ref.py, pinned without a GPU in tests/test_seq_models_host.py).  The pooling kernels are
pinned one by one elsewhere (tests/test_gpu_asp.py, test_gpu_bst.py, test_gpu_dien.py); here it is the hand-off: the
pooled row into a scratch row of the table (zero behind column D: no bias-table entry, no linear entry), its gradient
out of ONE column of d_rows after the model's own backward wrote it, the query gradient ADDED onto another, the key
gradients scattered into the query feature's block.

Tolerances are those of tests/test_gpu_parity.py and the models' own test_gpu_*_model.py: logit 1e-5, pred 1e-6, every
gradient 2e-5 in the project's measure - but a pooling unit's variables and AutoInt's attention matrices, which keep
max(2e-5, 4 x the float32 CPU restatement's measure), and the two analytically zero gradients (hist_asp_w0 under the
softmax, hist_bst_bk), judged against the terms that cancel.  seq_models_ref.check_grads is that rule; the host tests
show that it catches a gradient taken from the wrong field, a query gradient that overwrites, and missing query or key
gradients on every model.  Both measures are printed.

The one engine fault these cases found is pinned on its own at the end: the first CIN layer read LDS that nothing had
written (NaN logits of xdeepfm behind the transformer unit, in some runs)."""
import pytest
import torch

from tests import seq_models_ref as R
from tests.test_gpu_parity import _close

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _engine(k, hp=None):
    from recman_amd import engine as eng

    spec = k["spec"]
    hp = dict(k["hp"] if hp is None else hp)
    e = eng.ENGINES[k["model"]](eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names,
                                                multi_names=getattr(spec, "multi_names", ()),
                                                value_names=getattr(spec, "value_names", ()),
                                                seq_query=spec.seq_query, seq_max_len=spec.seq_max_len),
                                hp["embedding_size"], hp)
    e.load_params({n: v.to(F32) for n, v in k["p"].items()})
    return e


def _inputs(k):
    """The case on the device, mv in the engine's form: a value feature is (offsets, ids, vals), one id per example."""
    B, mv = k["idx"].shape[0], {}
    for n, ent in k["mv"].items():
        if n in getattr(k["spec"], "value_names", ()):
            mv[n] = (torch.arange(B + 1).cuda(), ent[0].cuda(), ent[1].to(F32).cuda())
        else:
            mv[n] = (ent[0].cuda(), ent[1].cuda())
    return k["idx"].cuda(), k["dense"].to(F32).cuda(), k["y"].cuda(), mv


def _check(k, what):
    """One fwd_bwd of the case's engine against float64; -> the engine and its device inputs."""
    (loss_o, logit_o, pred_o, grads_o), g32, scales = R.reference(k)
    p, spec = k["p"], k["spec"]
    e = _engine(k)
    assert set(e.state_dict()) == set(p), set(e.state_dict()) ^ set(p)
    _close(e.state_dict()["linear_w"], p["linear_w"], rtol=0, atol=0, what="linear_w round trip")
    idx_d, dense_d, y_d, mv_d = _inputs(k)
    loss = e.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
    torch.cuda.synchronize()
    print(f"{what}: logit err {float((e.logit.cpu().double() - logit_o).abs().max()):.2e}, "
          f"closest unit to its kink {k['min_abs_pre']:.1e}")
    _close(e.logit, logit_o, rtol=0, atol=1e-5, what="logit")
    _close(e.pred, pred_o, rtol=0, atol=1e-6, what="pred")
    _close(loss, loss_o.reshape(1), what="loss")
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) == set(grads_o), set(grads) ^ set(grads_o)
    R.check_grads(k, grads, grads_o, g32, scales, what=what + ": ")
    # the pooled scratch rows: the restatement's rows, exactly zero behind column D
    seq = [(j, f) for j, f in enumerate(e.mv_fields) if spec.sparse_names[f] in spec.seq_query]
    assert len(seq) == len(spec.seq_query)
    E_o = R.embeddings(p, spec, k["idx"], k["mv"], k["hp"])
    for j, f in seq:
        rows = e.mv_scratch[j]
        assert float(rows[:, e.D:].abs().max()) == 0.0, f"{what}: scratch row of field {f} is not zero behind column D"
        assert float((rows[:, : e.D].cpu().double() - E_o[:, f]).abs().max()) < 1e-5
        assert float(rows[:, : e.D].abs().max()) > 0
    # inference: the same logits, and the scratch rows of the inference pass are the training pass's bit for bit
    rows_train = e.mv_scratch.clone()
    e.mv_scratch.fill_(float("nan"))
    logit_i, _ = e.forward(idx_d, dense_d, training=False, mv=mv_d)
    _close(logit_i, logit_o, rtol=0, atol=1e-5, what="inference logit")
    assert torch.equal(e.mv_scratch, rows_train)
    with pytest.raises(ValueError, match="hist"):
        e.forward(idx_d, dense_d, training=False)  # the histories must be handed over
    return e, idx_d


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("model_id", list(R.MODELS))
def test_fwd_bwd_matches_float64(hip_lib, model_id, kind):
    _check(R.make_case(model_id, kind), f"{model_id}-{kind}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("model", ["deepfm", "dcn"])
def test_mixed_spec_matches_float64(hip_lib, model, kind):
    """Two histories of one query feature (one of them ahead of it), a multi-valued and a value feature in one spec:
    mv_fields, the scratch block index and the per-field buffers are keyed per field for exactly this."""
    k = R.make_mixed_case(kind, model=model)
    spec = k["spec"]
    e, idx_d = _check(k, f"mixed-{model}-{kind}")
    assert e.mv_fields == [0, 3, 4, 5] and e.use_bias_tables == (model == "deepfm")
    # (the candidate's own gradient, both histories' query gradients and both histories' key gradients all arrive in
    # item_feat_embed: check_grads compared it, and the rows that are candidate and item of both histories on their
    # own; tests/test_seq_models_host.py shows that dropping any of the three moves those rows by > 100 x the bound)
    assert len(R.shared_rows(k)["item"]) > 0
    for n in ("hist2", "hist"):
        fq, ids, d_keys = e.seq_key_grads(spec.sparse_names.index(n))
        assert fq == spec.sparse_names.index("item")
        assert torch.equal(ids.cpu(), k["mv"][n][1]) and d_keys.shape == (ids.shape[0], e.D)
        assert float(d_keys.abs().max()) > 0


@pytest.mark.parametrize("m", [2, 3, 4, 7])
def test_first_cin_layer_does_not_read_stale_lds(hip_lib, m):
    """xdeepfm-transformer above caught it: the first CIN layer (Xk IS X0: the symmetric k' ordering) walked the k'
    that pad the ordering to a multiple of 32 over rows PAST the staged Xk tile - for few fields, into the filter
    buffer that is not written yet - and multiplied what it found there by the zero row of X0: 0 x NaN = NaN wherever
    an earlier kernel (the transformer unit's masked softmax) had left a non-finite value in that LDS.  Here a GEMM on
    NaN operands runs first on every CU; the layer must still equal float64."""
    from recman_amd import ops

    B, N, D = 16384 + 5, 8, 8
    g = torch.Generator().manual_seed(m)
    X0 = torch.randn(B, m, D, generator=g)
    W = torch.randn(m * m, N, generator=g) * 0.2
    bias = torch.randn(N, generator=g) * 0.1
    Z = torch.einsum("bid,bjd->bdij", X0.double(), X0.double()).reshape(B, D, -1)
    want = (Z @ W.double() + bias.double()).transpose(1, 2)
    X0_d, W_d, bias_d = X0.cuda(), W.cuda(), bias.cuda()
    out = torch.empty(B, N, D, device="cuda")
    ws = torch.empty(ops.cin_filter_workspace(m, m, N), device="cuda")
    poison = torch.full((2048, 2048), float("nan"), device="cuda")
    for _ in range(3):
        torch.mm(poison, poison)
        ops.cin_layer_fwd(X0_d, X0_d, m, W_d, bias_d, "identity", out, ws)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), int((~torch.isfinite(out)).sum())
        err = float((out.cpu().double() - want).abs().max())
        assert err <= 2e-6 * max(1.0, float(want.abs().max())) * max(1.0, m / 4), err


def test_row_wise_step_equals_dense_step_on_the_mixed_spec(hip_lib):
    """Same gradients, one adam step from fresh optimizer state (tests/test_gpu_din_model.py's
    test_one_row_wise_step_equals_the_dense_path_step): the row-wise step - the item feature's own occurrences and the
    occurrences of BOTH histories as one occurrence list - and the dense-gradient step coincide."""
    from recman_amd.optim import Optimizer, SparseTableOptimizer

    for kind in R.KINDS:
        k = R.make_mixed_case(kind, model="dcn")
        hp = dict(k["hp"], embedding_l2_reg=0.0, linear_l2_reg=0.0, deep_l2_reg=0.0, cross_layer_l2_reg=0.0)
        e1, e2 = _engine(k, hp), _engine(k, hp)
        sopt = SparseTableOptimizer(e2, "adam", 0.01)
        idx_d, dense_d, y_d, mv_d = _inputs(k)
        e1.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
        before = e1.params["item_feat_embed"].clone()
        Optimizer("adam", 0.01).step(e1.params, e1.dense_grads(idx_d))
        e2.fwd_bwd(idx_d, dense_d, y_d, mv=mv_d)
        sopt.step(idx_d)
        Optimizer("adam", 0.01).step(e2.params, e2.grads)
        torch.cuda.synchronize()
        for n in e1.params:
            a, b = e1.params[n], e2.params[n]
            assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(a.abs().max())), (kind, n)
        moved = (e1.params["item_feat_embed"] - before).abs().sum(dim=1) > 0
        both = R.shared_rows(k)["item"]
        assert both and bool(moved[both].all())  # rows that are candidate and item of both histories
