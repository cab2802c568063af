"""GPU: the kernels' steady-state paths against float64.

Most hot kernels run a fixed-size grid (a persistent grid, a grid cap or an XCD-aware block map) and only take their
second code path when the batch is large: a block or a wave handles several tiles, ring buffers wrap, grid-stride
loops go round more than once, block maps reach their full-super-group and ragged-tail branches.  Every case here
runs a shape past one of those points, states which one, asserts it from the launch arithmetic of the C++ line it
cites, and compares the HIP result with a float64 reference of the same operation (the model oracle on .double()
parameters and inputs, or autograd in float64), to the tolerances of the module that tests the kernel at small sizes.
"""
import pytest
import torch

from oracle import th_layers as T
from tests import test_gpu_dense as TD
from tests.cases import make_case
from tests.stale_state import assert_guards_intact, guarded, poisoned
from tests.test_gpu_parity import _close, _close_grad, _engine

pytestmark = pytest.mark.gpu


def cdiv(a, b):
    return -(-a // b)


SIZES26 = [1000 + 137 * i for i in range(26)]  # vocabularies in the low thousands: rows repeat across the batch


def _kink_clear(z, terms, K):
    """Examples (dim 0) whose pre-activations z all lie outside 2 (K + 1) 2^-24 * terms of the kink at 0 (terms: the
    sum of the |terms| of each dot product of K inputs plus the bias)."""
    return (z.abs() > 2 * (K + 1) * 2.0 ** -24 * terms).flatten(1).all(1)


def _case(model, B, **kw):
    """make_case with B examples whose hidden pre-activations (DNN layers, and CIN layers for xDeepFM) all lie clear
    of the activation's kink at 0.  At an example within the fp32 rounding band of the kink, fp32 and float64 may
    take different branches of relu' / leaky_relu' and both be right, and one such example moves a batch-summed
    gradient by far more than rounding: at B = 70 001 one of 2.2 M pre-activations, 8e-9 from 0, flipped and put dW0
    44x over its tolerance.  The band is twice (K + 1) 2^-24, the worst-case fp32 error of one dot product of
    exact inputs, times the sum of its |terms|.  It is a margin, not a bound on the kernels' error: a layer's inputs
    carry rounding in from the layer before, and the split-operand kernels add six piece products per term.  A
    bound that propagates both would leave half (f32) to 1 % (split operands) of DCN's examples, whose two layers
    of 400 units give 800 pre-activations each.  The margin removes the examples near a kink; the seeds are fixed,
    so what remains is checked deterministically.  Examples are drawn beyond B and the first B clear ones kept."""
    spec, p, idx, dense, y, hp = make_case(model, B=B + B // 2, **kw)
    p64 = {k: v.double() for k, v in p.items()}
    E, _ = T.feat_embedding_layer(p64, spec, idx, use_bias=(model == "deepfm"))
    a = T.dnn_input(E, dense.double())
    clear = torch.ones(a.shape[0], dtype=torch.bool)
    for i in range(len(hp["deep_hidden_units"])):
        W, b = p64[f"dnn_layer_{i}_weights"], p64[f"dnn_layer_{i}_bias"]
        z = a @ W + b
        clear &= _kink_clear(z, a.abs() @ W.abs() + b.abs(), W.shape[0])
        a = T.act_fn(hp["deep_activation"])(z)
    units = hp.get("cin_cross_layer_units", ()) if model == "xdeepfm" else ()
    n, m, D = E.shape
    xk = E
    for i, N in enumerate(units):  # (T.cin's arithmetic: Z[b,d,i*H+j] = X0[b,i,d] Xk[b,j,d], maps = act(Z W + b))
        W, b = p64[f"cin_filter_{i}"][0], p64[f"cin_bias_{i}"]
        Z = torch.einsum("bid,bjd->bdij", E, xk).reshape(n, D, -1)
        z = Z @ W + b
        clear &= _kink_clear(z, Z.abs() @ W.abs() + b.abs(), W.shape[0])
        xk = T.act_fn(hp["cin_activation"])(z).transpose(1, 2)[:, : N // 2]
    sel = clear.nonzero().reshape(-1)[:B]
    assert sel.numel() == B, f"only {sel.numel()} of {B} examples clear of the kink"
    return spec, p, idx[sel].contiguous(), dense[sel].contiguous(), y[sel].contiguous(), hp


def _oracle64(model, p, spec, idx, dense, y, hp, task="classification"):
    """The model oracle in float64: (loss, logit, pred, grads)."""
    p64 = {k: v.double() for k, v in p.items()}
    yy = y.double() if y.is_floating_point() else y
    return T.fwd_bwd(model, p64, spec, idx, dense.double(), yy, hp, task=task)


def _check_against_oracle(e, idx_d, loss, want, p, pred_atol=1e-6):
    loss_o, logit_o, pred_o, grads_o = want
    _close(e.logit, logit_o, rtol=0, atol=1e-5, what="logit vs float64")
    _close(e.pred, pred_o, rtol=0, atol=pred_atol, what="pred vs float64")
    _close(loss, loss_o.reshape(1), what="loss vs float64")
    grads = e.dense_grads(idx_d, reference_names=True)
    assert set(grads) <= set(grads_o), set(grads) - set(grads_o)
    for k in grads_o:
        if k in grads:
            _close_grad(grads[k], grads_o[k], what=f"grad {k} vs float64")
        else:  # a variable the configuration does not use: its oracle gradient is the l2 term alone (as _check_model)
            assert float(grads_o[k].abs().max()) <= 1e-3 * 1.0001 * float(p[k].abs().max()), k


def _state(e):
    return [x.clone() for x in (e.logit, e.dlogit, e.d_rows, e.loss, *e.grads.values())]


def _assert_bit_equal(a, b, what):
    assert len(a) == len(b)
    for i, (x, z) in enumerate(zip(a, b)):
        assert torch.equal(x, z), f"{what}: tensor {i} of (logit, dlogit, d_rows, loss, grads...) differs"


# ---------------------------------------------------------------------------------------------------------------
# 1. the one-kernel DeepFM step (csrc/step.hip) in its steady state
STEP_B = 17_609


def _assert_step_steady_state(B):
    # rm_deepfm_step (csrc/step.hip:775-776): ntiles = (B + 15) / 16, nblk = rm_grid_cap(ntiles, 256);
    # deepfm_step_kernel (:719): block b runs the T = ceil((ntiles - b) / nblk) tiles b, b + nblk, ...; its t-th tile
    # goes to slot t % 3 of the worker's row ring (:226 and :263, (t + 6) % 3 and (td + 3) % 3)
    ntiles = cdiv(B, 16)
    nblk = min(ntiles, 256)
    assert (ntiles, nblk) == (1101, 256)
    tiles = [cdiv(ntiles - b, nblk) for b in range(nblk)]
    assert min(tiles) == 4 and max(tiles) == 5   # every block at least 4 tiles: the 3-slot ring wraps in each
    assert B % 16 == 9                           # the last tile is ragged (9 examples)


@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_one_kernel_step_steady_state_matches_float64(hip_lib, act):
    _assert_step_steady_state(STEP_B)
    spec, p, idx, dense, y, hp = _case("deepfm", STEP_B, F=26, D=16, Dn=13, hidden=(32, 32), sizes=SIZES26,
                                       scale=0.05, seed=3, hp_extra=dict(deep_activation=act))
    want = _oracle64("deepfm", p, spec, idx, dense, y, hp)
    e = _engine("deepfm", spec, 16, dict(hp, step_fusion=True), p)
    idx_d, dense_d, y_d = idx.cuda(), dense.cuda(), y.cuda()
    loss = e.fwd_bwd(idx_d, dense_d, y_d).clone()
    torch.cuda.synchronize()
    assert e._step_ok is True
    first = _state(e)
    _check_against_oracle(e, idx_d, loss, want, p, pred_atol=1e-5)  # (test_gpu_step's tolerances)
    # two runs: bit-identical
    e.fwd_bwd(idx_d, dense_d, y_d)
    _assert_bit_equal(_state(e), first, "second run")
    # the batch in slices of 4 096 examples, each run alone: one tile per block (the first tile of a block: ring slot
    # 0, dense slot 0).  In the full batch the same examples sat in tiles t = 0 .. 4 of their blocks: every slot of
    # the 3-slot row ring (t % 3) and of the 4-slot dense ring (:519, t & 3), wrapped.  Their logits are the same
    # bit for bit.
    starts = range(0, STEP_B, 4096)
    assert all(cdiv(min(4096, STEP_B - s0), 16) <= 256 for s0 in starts)
    t_full = {g // 256 for g in range(cdiv(STEP_B, 16))}   # tile counters of the full run (256 blocks)
    assert {t % 3 for t in t_full} == {0, 1, 2} and {t & 3 for t in t_full} == {0, 1, 2, 3}
    for s0 in starts:
        sl = slice(s0, min(s0 + 4096, STEP_B))
        e.fwd_bwd(idx_d[sl].contiguous(), dense_d[sl].contiguous(), y_d[sl].contiguous())
        assert torch.equal(e.logit, first[0][sl]), f"logits of examples {sl} depend on the rest of the batch"


def test_one_kernel_step_steady_state_non_temporal_variants_are_bit_equal(hip_lib):
    """deepfm_step_kernel<NT, NT_OUT, false> for all four (step_row_loads, d_rows_reuse): the load / store hints must
    not change the arithmetic."""
    _assert_step_steady_state(STEP_B)
    spec, p, idx, dense, y, hp = _case("deepfm", STEP_B, F=26, D=16, Dn=13, hidden=(32, 32), sizes=SIZES26,
                                       scale=0.05, seed=4)
    idx_d, dense_d, y_d = idx.cuda(), dense.cuda(), y.cuda()
    e = _engine("deepfm", spec, 16, dict(hp, step_fusion=True), p)
    e.fwd_bwd(idx_d, dense_d, y_d)
    base = _state(e)
    for rows in ("cache", "stream"):
        for d_rows in ("cache", "stream"):
            v = _engine("deepfm", spec, 16, dict(hp, step_fusion=True, step_row_loads=rows, d_rows_reuse=d_rows), p)
            v.fwd_bwd(idx_d, dense_d, y_d)
            assert v._step_ok is True
            _assert_bit_equal(_state(v), base, f"step_row_loads={rows}, d_rows_reuse={d_rows}")


def test_one_kernel_step_steady_state_regression_float_labels(hip_lib):
    from recman_amd import engine as eng

    _assert_step_steady_state(STEP_B)
    spec, p, idx, dense, _, hp = _case("deepfm", STEP_B, F=26, D=16, Dn=13, hidden=(32, 32), sizes=SIZES26,
                                       scale=0.05, seed=5)
    yf = torch.randn(STEP_B, generator=torch.Generator().manual_seed(11))
    want = _oracle64("deepfm", p, spec, idx, dense, yf, hp, task="regression")
    e = eng.DeepFMEngine(eng.FeatureSpec(spec.sparse_names, spec.feat_sizes, spec.dense_names), 16,
                         dict(hp, step_fusion=True), task="regression", device="cuda:0")
    e.load_params({k: v for k, v in p.items() if k in e.params or k == "linear_w"})
    idx_d = idx.cuda()
    loss = e.fwd_bwd(idx_d, dense.cuda(), yf.cuda())
    assert e._step_ok is True
    _check_against_oracle(e, idx_d, loss, want, p, pred_atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------
# 2. the two-kernel DeepFM path (csrc/mlp.hip) past every grid cap
MLP_B = 70_001


def _assert_past_every_mlp_grid_cap(B):
    ntiles = cdiv(B, 32)  # 32-example tiles / chunks in every MLP kernel
    # rm_mlp_fwd / rm_embed_mlp_fwd (csrc/mlp.hip:1534, :1598): grid = rm_grid_cap(ceil(ntiles / 8 waves), 256)
    assert cdiv(ntiles, 8) > 256
    # rm_mlp_bwd: nblk = rm_grid_cap(ntiles, 256) (csrc/mlp.hip:1654), one tile at a time: 8+ tiles per block
    assert ntiles >= 8 * 256
    # mlp_small_grads_mfma (csrc/mlp.hip:1688): sblk = rm_grid_cap(ceil(ntiles / 4), 512), one chunk per wave a round:
    # chunks past 512 x 4 go round again
    assert cdiv(ntiles, 4) > 512 and ntiles > 512 * 4
    assert B % 32 != 0


@pytest.mark.parametrize("D", [16, 8])
def test_two_kernel_path_past_the_grid_caps_matches_float64(hip_lib, D):
    """D = 16 with step_fusion=False: rm_embed_mlp_fwd + rm_mlp_bwd; D = 8 with the default step_fusion (the step and
    the fused front decline it on their own): the embedding kernel + rm_mlp_fwd + rm_mlp_bwd.
    d_rows_reuse="stream" (mlp_bwd_kernel<true>) is bit-equal."""
    from recman_amd import engine as eng
    from recman_amd import ops

    _assert_past_every_mlp_grid_cap(MLP_B)
    spec, p, idx, dense, y, hp = _case("deepfm", MLP_B, F=26, D=D, Dn=13, hidden=(32, 32), sizes=SIZES26,
                                       scale=0.05, seed=6)
    hp = dict(hp, step_fusion=False) if D == 16 else hp
    assert "step_fusion" in hp or eng.STEP_FUSION_DEFAULT is True
    want = _oracle64("deepfm", p, spec, idx, dense, y, hp)
    e = _engine("deepfm", spec, D, hp, p)
    assert ops.deepfm_step_supported(26, D, e.LD, 13, (32, 32)) is (D == 16)
    idx_d, dense_d, y_d = idx.cuda(), dense.cuda(), y.cuda()
    loss = e.fwd_bwd(idx_d, dense_d, y_d).clone()
    torch.cuda.synchronize()
    assert not getattr(e, "_step_ok", None)   # (D = 8: declined; D = 16: switched off)
    assert e._front_ok is (D == 16) and e.mlp.fused_ok
    base = _state(e)
    _check_against_oracle(e, idx_d, loss, want, p)
    s = _engine("deepfm", spec, D, dict(hp, d_rows_reuse="stream"), p)
    assert s.mlp.stream_d_rows
    s.fwd_bwd(idx_d, dense_d, y_d)
    _assert_bit_equal(_state(s), base, "d_rows_reuse=stream")


# ---------------------------------------------------------------------------------------------------------------
# 3. the CIN dM pass looping (csrc/cin.hip)
def _dm_blocks_wanted(B, D):
    # rm_cin_layer_bwd (csrc/cin.hip:1315-1318): epb = clamp(64 / D, 1, 8); nblk = rm_grid_cap(ceil(B / epb),
    # kDmBlocks = 2048), so blocks loop once ceil(B / epb) > 2048
    epb = min(max(64 // D, 1), 8)
    return cdiv(B, epb)


CIN_SHAPES = [  # B, m, H, N, D, act, first, last, six (csrc/cin6.hip takes the backward's dX / dW with split=True)
    # dM: ceil(8 203 / 4) = 2 051 blocks wanted against the cap of 2 048 - only 3 blocks go round a second time
    (8203, 4, 64, 128, 16, "leaky_relu", False, False, True),
    # D = 64: one example per dM block, 2 117 wanted (69 blocks loop); first layer: the symmetric f32 dX / dW kernels,
    # the split dX kernel with "first6"
    (2117, 4, 4, 128, 64, "relu", True, False, True),
    # N <= 64: the f32 dX / dW kernels whatever the split flag; 2 251 dM blocks wanted
    (9001, 5, 8, 48, 16, "leaky_relu", False, True, False),
]


@pytest.mark.parametrize("B,m,H,N,D,act,first,last,six", CIN_SHAPES)
@pytest.mark.parametrize("split", [False, True, "first6"], ids=["f32", "split", "split-first-layer-too"])
def test_cin_layer_bwd_dm_pass_looping(hip_lib, B, m, H, N, D, act, first, last, six, split):
    """rm_cin_layer_bwd against float64 autograd of the layer (as test_gpu_cin.test_cin_layer_bwd, same tolerance),
    with the reference built in chunks of 1 024 examples: W and bias gradients accumulate over the chunks in
    float64."""
    from recman_amd import ops

    assert _dm_blocks_wanted(B, D) > 2048
    # csrc/cin6.hip:518 / :774: the split dX / dW workspaces are 0 unless cin6_covers the layer (what
    # cin_filter_workspace6 reports) and N > 64
    assert (ops.cin_filter_workspace6(m, H, N, D) > 0 and N > 64) is six
    g_ = torch.Generator().manual_seed(B * 7 + N)
    X0 = torch.randn(B, m, D, generator=g_, dtype=torch.float64)
    Xk = X0 if first else torch.randn(B, H, D, generator=g_, dtype=torch.float64)
    W = (torch.randn(m * H, N, generator=g_, dtype=torch.float64) * 0.2).requires_grad_(True)
    bias = (torch.randn(N, generator=g_, dtype=torch.float64) * 0.1).requires_grad_(True)
    pool_from = 0 if last else N // 2
    cw = torch.randn(N - pool_from, generator=g_, dtype=torch.float64)
    gvec = torch.randn(B, generator=g_, dtype=torch.float64)
    dh = torch.randn(B, pool_from, D, generator=g_, dtype=torch.float64) if pool_from else None
    outs, gx0, gxk = [], [], []
    for s in range(0, B, 1024):
        x0 = X0[s:s + 1024].clone().requires_grad_(True)
        xk = x0 if first else Xk[s:s + 1024].clone().requires_grad_(True)
        n = x0.shape[0]
        Z = torch.einsum("bid,bjd->bdij", x0, xk).reshape(n, D, -1)
        out = T.act_fn(act)(Z @ W + bias).transpose(1, 2)  # [n,N,D]
        obj = (out[:, pool_from:].sum(-1) * cw * gvec[s:s + n, None]).sum()
        if pool_from:
            obj = obj + (out[:, :pool_from] * dh[s:s + n]).sum()
        obj.backward()
        outs.append(out.detach().float())
        gx0.append(x0.grad)
        if not first:
            gxk.append(xk.grad)
    out_d = torch.cat(outs).cuda().contiguous()
    want_dx0 = torch.cat(gx0)

    f = lambda t: t.detach().float().cuda().contiguous()
    dX0 = torch.full((B, m, D), 0.5, device="cuda")  # accumulate onto a known value
    dXk = None if first else poisoned(B, H, D)
    dW = poisoned(m * H, N)
    dbias = poisoned(N)
    ws, wsbuf = guarded(ops.cin_bwd_workspace(B, m, H, N, D))
    ops.cin_layer_bwd(f(X0), f(Xk), H, f(W), act, out_d, f(gvec), dX0, dW, dbias, ws,
                      xk_is_x0=first, d_hidden=f(dh) if pool_from else None, cin_w_direct=f(cw),
                      pool_from=pool_from, accumulate_dx0=True, dXk=dXk, split=bool(split), first6=split == "first6")
    torch.cuda.synchronize()

    def close(got, want, what):
        want = want.double()
        scale = max(1.0, float(want.abs().max()))
        err = float((got.cpu().double() - want).abs().max())
        assert err <= 2e-5 * scale, f"{what}: {err:.3e} (scale {scale:.3e})"

    close(dX0 - 0.5, want_dx0, "dX0")
    if not first:
        close(dXk, torch.cat(gxk), "dXk")
    close(dW, W.grad, "dW")
    close(dbias, bias.grad, "dbias")
    assert_guards_intact(wsbuf, "rm_cin_bwd_workspace")


@pytest.mark.parametrize("cin_gemm", ["bf16x6", "f32"])
def test_xdeepfm_past_the_dm_grid_cap_matches_float64(hip_lib, cin_gemm):
    B, D = 8300, 16
    assert _dm_blocks_wanted(B, D) > 2048
    spec, p, idx, dense, y, hp = _case("xdeepfm", B, F=10, D=D, cin_units=(32, 16), scale=0.2, seed=7,
                                       hp_extra=dict(cin_gemm=cin_gemm))
    want = _oracle64("xdeepfm", p, spec, idx, dense, y, hp)
    e = _engine("xdeepfm", spec, D, hp, p)
    idx_d = idx.cuda()
    loss = e.fwd_bwd(idx_d, dense.cuda(), y.cuda())
    torch.cuda.synchronize()
    assert (e.cin_fws6 is not None) == (cin_gemm == "bf16x6")
    _check_against_oracle(e, idx_d, loss, want, p)


# ---------------------------------------------------------------------------------------------------------------
# 4. the dense kernels past their block maps (csrc/gemm6.hip, csrc/gemm.hip)
DENSE_M = 9001


def _nn6_map(M):
    # dense_nn6_kernel (csrc/gemm6.hip:170-181): 128-row tiles (kRows6 = 32 x 4 waves); super-groups of 8 row tiles
    # x ngroups blocks take the XCD map while (sg + 1) * 8 <= ntiles, a ragged last one the plain map
    ntiles = cdiv(M, 128)
    return ntiles // 8, ntiles % 8


def _tn_slabs(K, N, M, allow_split):
    """Slabs of the f32 TN kernel's launch (csrc/gemm.hip tn_slabs / tn_plan), either form of the plan."""
    kts, nct = cdiv(K, 128), cdiv(cdiv(N, 32), 14)
    s = max(min(256 // (kts * nct), cdiv(M, 512)), 1)
    if s >= 8:
        s = s // 8 * 8
    live = cdiv(K - (kts - 1) * 128, 32)
    if allow_split and kts >= 2 and live <= 2:
        ratio = 0.667 if live == 2 else 0.41
        rb = 256 // nct
        sf = min(int(rb / (kts - 1 + ratio)), cdiv(M, 512))
        sr = min(rb - (kts - 1) * sf, int(ratio * sf + 0.999))
        if sf >= 4 and sr >= 1:
            s = sf
    return s


@pytest.mark.parametrize("K1,K2,N", [(416, 13, 400), (64, 0, 900)])
def test_dense_fwd6_full_super_groups_and_a_ragged_group(hip_lib, K1, K2, N):
    """Every check of test_gpu_dense's rm_dense_fwd6 test (all epilogues, the fused dot, <= 1.5x the f32 kernel's
    error, determinism) at 71 row tiles: 8 full super-groups and a ragged group of 7."""
    assert _nn6_map(DENSE_M) == (8, 7)
    TD.test_dense_fwd6_split_operands_match_float64_at_least_as_well_as_the_f32_kernel(hip_lib, DENSE_M, K1, K2, N)


@pytest.mark.parametrize("act", ["relu", "leaky_relu", "identity"])
def test_dense_fwd_f32_padded_second_round_and_stagger(hip_lib, act):
    # rm_dense_fwd (csrc/gemm.hip:1005-1021): span = min(ntiles, 256) row tiles per round, the grid padded to whole
    # rounds; groups = 2 * nct; the odd-group blocks of round 0 start late when ntiles * groups > 512
    M, K1, K2, N = 33_000, 416, 13, 400
    ntiles, nct = cdiv(M, 128), cdiv(cdiv(N, 32), 14)
    span, groups = min(ntiles, 256), 2 * nct
    assert ntiles > span and ntiles % span != 0   # a second round, padded with empty tiles
    assert ntiles * groups > 512                  # the stagger
    TD.test_dense_fwd_bias_act(hip_lib, M, K1, K2, N, act)
    if act == "relu":
        TD.test_dense_fwd_other_epilogues(hip_lib, M, K1, K2, N)


def test_dense_wgrad_f32_many_slabs(hip_lib):
    K1, K2, N = 416, 13, 400
    assert min(_tn_slabs(K1 + K2, N, DENSE_M, sp) for sp in (False, True)) >= 8
    TD.test_dense_wgrad(hip_lib, DENSE_M, K1, K2, N)


def test_dense_wgrad6_several_slabs_per_block_with_a_second_piece(hip_lib):
    # rm_dense_wgrad6 (csrc/gemm6.hip tn6_plan): 224 x 208 output tiles, per = ceil(nslab / want) 32-row slabs per
    # block with want = 256 / (nkh * nnh); M % 32 != 0: the ragged-batch kernel
    K, N, N2 = 429, 400, 7
    nkh, nnh, nslab = cdiv(K, 224), cdiv(N + N2, 208), cdiv(DENSE_M, 32)
    assert cdiv(nslab, min(256 // (nkh * nnh), nslab)) >= 2 and DENSE_M % 32 != 0
    TD.test_dense_wgrad6_split_operands(hip_lib, DENSE_M, 416, 13, N)


def test_dcn_past_the_block_maps_matches_float64(hip_lib):
    """dense_nn6 layer 0 with the dense-slab tail (K = 416 + 13) over full super-groups and a ragged one, the cross
    net's P folded into the first layer's weight-gradient pass (dcn_fold_cross_wgrad), cross kernels past one grid
    of blocks."""
    B = DENSE_M
    assert _nn6_map(B) == (8, 7)
    # cross_grid (csrc/cross.hip): rm_grid_cap(ceil(B / (4 waves x U = 2 rows)), 256 x 4 waves per SIMD)
    assert cdiv(B, 8) > 1024
    spec, p, idx, dense, y, hp = _case("dcn", B, F=26, D=16, Dn=13, hidden=(400, 400), cross_layers=6,
                                       sizes=SIZES26, scale=0.03, seed=8)
    want = _oracle64("dcn", p, spec, idx, dense, y, hp)
    e = _engine("dcn", spec, 16, hp, p)
    idx_d = idx.cuda()
    loss = e.fwd_bwd(idx_d, dense.cuda(), y.cuda())
    torch.cuda.synchronize()
    assert not e.matrix and e.mlp.can_defer_wgrad0()   # the folded cross wgrad ran
    _check_against_oracle(e, idx_d, loss, want, p)
