"""GPU: no kernel may depend on what an earlier kernel left in LDS.

tests/test_gpu_step_stale_lds.py holds rm_deepfm_step to this; this module holds every other kernel family to it.
Every test runs under tests/stale_state.py's `lds_pattern` fixture: ops.debug_lds_fill(pattern) - all 163,840 bytes of
every CU's LDS - is enqueued directly in front of every entry point, and `run_patterns` runs the case with the LDS
holding 0, 1, a quiet NaN and 1e38 in turn (0 and 1 first: a stale word used as an integer then fails on a bit
comparison while it is still a valid index).  Each run is held to the family's OWN float64 check - its runner, its
checker, its tolerances, imported from the family's test module, none restated - and the four runs must agree bit for
bit.

Cases: from each family's own case list the smallest cases with a ragged last tile (B = 33, 37, 65, 129: no multiple of
a 16-, 32- or 64-example tile), a width that the kernel pads to its MFMA or tile size (F = 5, 27, odd H, N = 40, 50, 70,
100, K1 = 40, 429 ...), B = 1 .. 5 (most of every tile is padding), and, where the kernel runs a ring or a double
buffer, one case whose blocks walk at least three tiles.  The core kernels' cases are the ones the issue behind this
module lists, through the runners of test_gpu_dense / _cin / _cross.

Engine-level cases run whole fwd_bwd passes, where kernels meet each other's leftovers: DeepFM (with and without the
one-kernel step), xDeepFM and DCN at B = 37 through test_gpu_parity._check_model, and the interaction engines' smallest
cases.  Loss, logits and predictions are compared bit for bit (the dense gradients of the embedding tables are made with
float atomics and are held to their float64 tolerance only).

Known limit: an entry point that launches several kernels is poisoned in front of the first one only.  The later
kernels see what the earlier ones left, as they do in production.

The ledger (checked without a GPU): COVERED names, per entry point, the test here that runs it under the fixture (each
test asserts that the fixture saw the entries it claims); EXEMPT holds the entry points none of whose kernels declares
static or dynamic __shared__ storage, with the kernels' names (checked against csrc).  Together they are exactly the
entry points include/recman_hip.h declares with an rm_stream_t stream argument.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests.stale_state import PATTERNS, lds_pattern, run_patterns  # noqa: F401  (lds_pattern: a fixture)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recman_amd", "csrc")

# ------------------------------------------------------------------------------------------------------ the ledger
_T = {  # test -> the entry points it runs under the fixture
    "test_the_fill_reaches_every_word_of_every_cu": ["rm_debug_lds_fill", "rm_debug_lds_probe"],
    "test_dense_fwd": ["rm_dense_fwd"],
    "test_dense_fwd6": ["rm_dense_fwd6"],
    "test_dense_wgrad": ["rm_dense_wgrad"],
    "test_dense_wgrad6": ["rm_dense_wgrad6"],
    "test_outer_actgrad_sums": ["rm_outer_actgrad_sums"],
    "test_cin_fwd": ["rm_cin_layer_fwd"],
    "test_cin_fwd6": ["rm_cin_layer_fwd6"],
    "test_cin_bwd": ["rm_cin_layer_bwd"],
    "test_cross": ["rm_cross_fwd", "rm_cross_bwd"],
    "test_mlp": ["rm_mlp_fwd", "rm_mlp_bwd"],
    "test_embed_mlp_fwd": ["rm_embed_mlp_fwd"],
    "test_linear_dense_bwd": ["rm_linear_dense_bwd"],
    "test_logit_loss": ["rm_logit_loss"],
    "test_shard_route": ["rm_shard_route", "rm_shard_route_padded"],
    "test_fibinet": ["rm_fibinet_fwd", "rm_fibinet_bwd"],
    "test_fmfm": ["rm_fmfm_fwd", "rm_fmfm_bwd"],
    "test_pnn": ["rm_pnn_fwd", "rm_pnn_bwd"],
    "test_masknet_group": ["rm_masknet_group_fwd", "rm_masknet_group_bwd"],
    "test_masknet_row": ["rm_masknet_row_fwd", "rm_masknet_row_bwd"],
    "test_afm": ["rm_afm_fwd", "rm_afm_bwd"],
    "test_autoint_layer": ["rm_autoint_layer_fwd", "rm_autoint_layer_bwd"],
    "test_autoint_head": ["rm_autoint_head_fwd", "rm_autoint_head_bwd"],
    "test_dot_interact": ["rm_dot_interact_fwd", "rm_dot_interact_bwd"],
    "test_cross_mix": ["rm_cross_mix_fwd", "rm_cross_mix_bwd"],
    "test_mmoe_mix": ["rm_mmoe_mix_fwd", "rm_mmoe_mix_bwd"],
    "test_multitask_loss": ["rm_multitask_loss"],
    "test_inbatch_softmax": ["rm_inbatch_softmax_fwd", "rm_inbatch_softmax_bwd"],
    "test_asp": ["rm_asp_fwd", "rm_asp_bwd"],
    "test_bst": ["rm_bst_fwd", "rm_bst_bwd"],
    "test_dien": ["rm_dien_fwd", "rm_dien_bwd"],
    "test_sparse_optimizer": ["rm_sparse_optimizer_prepare", "rm_sparse_optimizer_step_rules",
                              "rm_sparse_optimizer_step_rows_rules"],
    "test_sparse_optimizer_old_entries": ["rm_sparse_optimizer_step", "rm_sparse_optimizer_step_rows"],
    "test_metrics": ["rm_roc_auc", "rm_log_loss"],
    "test_group_auc": ["rm_group_auc"],
    "test_engines": ["rm_deepfm_step"],
}
COVERED = {e: t for t, es in _T.items() for e in es}

EXEMPT = {  # entry point -> (file, its kernels: none of them declares __shared__ storage), why it needs no LDS
    "rm_profile_marker": ("api.hip", ["rm_profile_marker_kernel"], "an empty kernel"),
    "rm_embed_fwd": ("embed.hip", ["embed_fwd_kernel", "embed_fwd_fused_kernel"],
                     "a lane group per example, registers only"),
    "rm_linear_fwd": ("embed.hip", ["linear_fwd_kernel"], "one thread per example"),
    "rm_embed_bwd": ("embed.hip", ["embed_bwd_kernel"], "an elementwise pass over float4s"),
    "rm_scatter_add_rows": ("embed.hip", ["scatter_add_rows_kernel"], "an elementwise pass of float atomics"),
    "rm_gather_rows": ("embed.hip", ["gather_rows_kernel"], "a row copy"),
    "rm_permute_rows": ("embed.hip", ["permute_rows_kernel"], "a row copy"),
    "rm_bias_act": ("loss.hip", ["bias_act_kernel"], "an elementwise pass"),
    "rm_act_bwd": ("loss.hip", ["act_bwd_kernel"], "an elementwise pass"),
    "rm_outer_actgrad": ("loss.hip", ["outer_actgrad_kernel"], "an elementwise pass"),
    "rm_rowdot": ("loss.hip", ["rowdot_kernel"], "a wave per row, registers only"),
    "rm_cross_param_grads": ("cross.hip", ["cross_param_grads_kernel"], "an elementwise pass over [L, d]"),
    "rm_pool_rows": ("pool.hip", ["pool_rows_kernel"], "a lane group per example, registers only"),
    "rm_pool_rows_bwd": ("pool.hip", ["pool_rows_bwd_kernel"], "a lane group per tag, registers only"),
    "rm_pool_rows_padded": ("pool.hip", ["pool_rows_padded_kernel"], "a lane group per example, registers only"),
    "rm_pack_pooled_grad_rows": ("pool.hip", ["pack_pooled_grad_rows_kernel"], "a row copy with a scale"),
    "rm_pack_grad_rows": ("route.hip", ["pack_grad_rows_kernel"], "a row copy"),
    "rm_dense_optimizer_step": ("optim.hip", ["dense_opt_kernel"], "an elementwise pass"),
    "rm_dense_optimizer_step_rule": ("optim.hip", ["dense_opt_kernel"], "an elementwise pass"),
    "rm_rownorm_fwd": ("inbatch.hip", ["rownorm_fwd_kernel"], "a wave per row, registers only"),
    "rm_rownorm_bwd": ("inbatch.hip", ["rownorm_bwd_kernel"], "a wave per row, registers only"),
}


def _stream_entry_points(header="recman_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(rm_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\brm_stream_t\s+stream\b", m.group(2))}


def test_ledger_is_every_entry_point_with_a_stream():
    entries = _stream_entry_points()
    assert len(entries) >= 79 and "rm_dense_fwd" in entries and "rm_version" not in entries
    assert not set(COVERED) & set(EXEMPT), sorted(set(COVERED) & set(EXEMPT))
    assert set(COVERED) | set(EXEMPT) == entries, sorted((set(COVERED) | set(EXEMPT)) ^ entries)
    assert len(EXEMPT) < len(COVERED) / 2
    for t in _T:
        assert callable(globals().get(t)), f"{t} is not a test of this module"


def _kernel_body(src, name):
    m = re.search(r"__global__[^;{]*?\bvoid\s+%s\s*\(" % re.escape(name), src)
    assert m, f"kernel {name} not found"
    end = src.find("\n}\n", m.end())
    assert end > 0
    return src[m.start():end]


def test_exempt_entry_points_launch_only_kernels_without_shared_storage():
    for entry, (fname, kernels, why) in EXEMPT.items():
        assert kernels and why, entry
        src = open(os.path.join(CSRC, fname)).read()
        assert re.search(r'extern "C" int %s\(' % entry, src), f"{entry} is not defined in {fname}"
        for k in kernels:
            assert "__shared__" not in _kernel_body(src, k), f"{entry}: {k} declares __shared__ storage"
        # nothing else of the file's kernels without the word can hide a helper with it: __shared__ appears in
        # __global__ functions only
        for m in re.finditer(r"__shared__", src):
            head = src.rfind("__global__", 0, m.start())
            assert head >= 0 and src.find("\n}\n", head) > m.start(), f"{fname}: __shared__ outside a kernel's body"
        # every kernel the entry point's file launches for it is named: the launches between the entry's definition
        # and the end of its body
        at = src.index('extern "C" int %s(' % entry)
        body = src[at:src.find("\n}\n", at)]
        launched = set(re.findall(r"hipLaunchKernelGGL\(\(?\s*([A-Za-z_0-9]+)", body))
        assert launched <= set(kernels), f"{entry} also launches {sorted(launched - set(kernels))}"


def _saw(state, test):
    claimed = set(_T[test])
    assert claimed <= state["seen"], f"{test}: the fixture did not see {sorted(claimed - state['seen'])}"
    assert state["fills"] > 0 and state["pattern"] is None


# ------------------------------------------------------------------------------------------------------- the aid
@gpu
def test_the_fill_reaches_every_word_of_every_cu(hip_lib):
    from recman_amd import ops

    cus = int(hip_lib.rm_device_cus())
    assert cus > 0
    n = 4 * cus
    for pattern in PATTERNS:
        ops.debug_lds_fill(pattern)
        counts = ops.debug_lds_probe(pattern, n)
        torch.cuda.synchronize()
        bad = counts.ne(0)
        assert not bool(bad.any()), (f"pattern {pattern:#010x}: {int(bad.sum())} of {n} probe blocks found words the "
                                     f"fill did not write, up to {int(counts.max())} of {163840 // 4}")
    # the probe does tell: behind a fill with another pattern every word differs
    ops.debug_lds_fill(PATTERNS[1])
    counts = ops.debug_lds_probe(PATTERNS[2], n)
    assert bool((counts == 163840 // 4).all())


# ------------------------------------------------------------------------------------------------ the core kernels
@gpu
@pytest.mark.parametrize("M,K1,K2,N", [(37, 40, 3, 50), (129, 400, 0, 400), (64, 429, 0, 429)])
def test_dense_fwd(lds_pattern, M, K1, K2, N):
    from tests import test_gpu_dense as TD

    run_patterns(lambda: (TD._fwd_bias_act_case(M, K1, K2, N, "relu"), TD._fwd_other_epilogues_case(M, K1, K2, N)),
                 what=f"dense fwd {(M, K1, K2, N)}: ")
    _saw(lds_pattern, "test_dense_fwd")


@gpu
def test_dense_fwd_unaligned_rows_and_the_k1_outer_product(lds_pattern):
    from tests import test_gpu_dense as TD

    run_patterns(TD._fwd_unaligned_rows_and_k1_case, what="dense fwd (77, 30, 0, 45) and K = 1: ")
    _saw(lds_pattern, "test_dense_fwd")


@gpu
@pytest.mark.parametrize("M,K1,K2,N", [(37, 40, 3, 50), (129, 400, 0, 400), (5, 8, 0, 8)])
def test_dense_fwd6(lds_pattern, M, K1, K2, N):
    from tests import test_gpu_dense as TD

    run_patterns(lambda: TD._fwd6_case(M, K1, K2, N), what=f"dense fwd6 {(M, K1, K2, N)}: ")
    _saw(lds_pattern, "test_dense_fwd6")


@gpu
@pytest.mark.parametrize("M,K1,K2,N", [(37, 40, 3, 50), (3, 8, 0, 8), (129, 32, 0, 1), (300, 30, 2, 5),
                                        (5000, 400, 0, 400)])
def test_dense_wgrad(lds_pattern, M, K1, K2, N):
    from tests import test_gpu_dense as TD

    run_patterns(lambda: TD._wgrad_case(M, K1, K2, N), what=f"dense wgrad {(M, K1, K2, N)}: ")
    _saw(lds_pattern, "test_dense_wgrad")


@gpu
@pytest.mark.parametrize("M,K1,K2,N", [(37, 40, 3, 50), (3, 8, 0, 8), (777, 230, 0, 210)])
def test_dense_wgrad6(lds_pattern, M, K1, K2, N):
    from tests import test_gpu_dense as TD

    run_patterns(lambda: TD._wgrad6_case(M, K1, K2, N), what=f"dense wgrad6 {(M, K1, K2, N)}: ")
    _saw(lds_pattern, "test_dense_wgrad6")


@gpu
@pytest.mark.parametrize("B,N,act", [(1, 64, "relu"), (257, 400, "relu"), (131, 68, "identity")])
def test_outer_actgrad_sums(lds_pattern, B, N, act):
    from tests import test_gpu_dense as TD

    run_patterns(lambda: TD._outer_actgrad_sums_case(B, N, act), what=f"outer_actgrad_sums {(B, N, act)}: ")
    _saw(lds_pattern, "test_outer_actgrad_sums")


@gpu
@pytest.mark.parametrize("B,m,H,N,D,act", [(17, 7, 3, 40, 16, "relu"), (5, 2, 2, 16, 4, "identity"),
                                            (9, 6, 25, 100, 32, "leaky_relu")])
def test_cin_fwd(lds_pattern, B, m, H, N, D, act):
    from tests import test_gpu_cin as TC

    run_patterns(lambda: TC._fwd_case(B, m, H, N, D, act), what=f"cin fwd {(B, m, H, N, D)}: ")
    _saw(lds_pattern, "test_cin_fwd")


@gpu
@pytest.mark.parametrize("B,m,N,D,act", [(9, 7, 100, 32, "leaky_relu"), (17, 5, 40, 16, "relu"), (3, 2, 16, 64, "identity")])
def test_cin_fwd_first_layer(lds_pattern, B, m, N, D, act):
    """Xk = X0: the symmetric ordering whose padding k' once read stale LDS (the comment at read_step in csrc/cin.hip)."""
    from tests import test_gpu_cin as TC

    run_patterns(lambda: TC._fwd_first_layer_case(B, m, N, D, act), what=f"cin first layer {(B, m, N, D)}: ")
    _saw(lds_pattern, "test_cin_fwd")


@gpu
@pytest.mark.parametrize("B,m,H,N,D,act", [(9, 5, 3, 40, 32, "relu"), (3, 3, 64, 100, 16, "identity"),
                                            (1, 1, 32, 16, 64, "leaky_relu")])
def test_cin_fwd6(lds_pattern, B, m, H, N, D, act):
    from tests import test_gpu_cin as TC

    run_patterns(lambda: TC._fwd6_case(B, m, H, N, D, act), what=f"cin fwd6 {(B, m, H, N, D)}: ")
    _saw(lds_pattern, "test_cin_fwd6")
    assert "rm_cin_layer_fwd" in lds_pattern["seen"]    # (the f32 kernel it is measured against)


@gpu
@pytest.mark.parametrize("split", [False, True, "first6"], ids=["f32", "split", "split-first-layer-too"])
@pytest.mark.parametrize("B,m,H,N,D,act,first,last", [
    (1, 2, 5, 128, 16, "relu", False, True), (3, 1, 1, 70, 64, "leaky_relu", False, False),
    (129, 4, 33, 128, 32, "identity", False, False), (17, 7, 3, 40, 16, "relu", False, False),
    (9, 7, 7, 100, 32, "leaky_relu", True, True)])
def test_cin_bwd(lds_pattern, B, m, H, N, D, act, first, last, split):
    from tests import test_gpu_cin as TC

    run_patterns(lambda: TC._bwd_case(B, m, H, N, D, act, first, last, split),
                 what=f"cin bwd {(B, m, H, N, D)} split={split}: ")
    _saw(lds_pattern, "test_cin_bwd")


@gpu
@pytest.mark.parametrize("B,FD,Dn,L", [(37, 40, 3, 3), (33, 24, 100, 1), (1, 8, 1, 4), (2, 8, 1, 4), (3, 8, 1, 4)])
def test_cross(lds_pattern, B, FD, Dn, L):
    from tests import test_gpu_cross as TX

    run_patterns(lambda: TX._fwd_bwd_case(B, FD, Dn, L), what=f"cross {(B, FD, Dn, L)}: ")
    _saw(lds_pattern, "test_cross")


# ----------------------------------------------------------------------------------- the skinny MLP and the front
@gpu
@pytest.mark.parametrize("FD,Dn,big", [(4, 0, False), (0, 37, False), (112, 3, False), (60, 4, True),
                                        (416, 13, False), (432, 16, True), (64, 1, True)])
def test_mlp(lds_pattern, FD, Dn, big):
    """Loader shapes of tests/mlp_cases.LOADER_SHAPES: a partial chunk, dense-only tiles, the straddling loader, the
    xe / xd boundary inside a float4, split14 with a ragged dense tile; at B = 33 (two tiles, the second with one
    example) or at the shape's batch of 255 .. 257 (eight or nine tiles of 32 examples: the tile-ahead prefetch of a
    block runs more than once)."""
    from tests import mlp_cases as MC
    from tests import test_gpu_mlp_kernels as TM

    case = [c for c in MC.loader_cases() if c[:2] == (FD, Dn) and (c[2] >= 255 if big else c[2] == 33)]
    assert len(case) == 1, "not a loader case"
    FD, Dn, B, hidden, act = case[0]

    def run():
        f, b = TM.fwd_bwd(TM.Case(FD, Dn, B, hidden, act))
        return f.hv(), f.logit.v, {k: a.v for k, a in b.outputs().items()}

    run_patterns(run, what=f"mlp FD={FD} Dn={Dn} B={B}: ")
    _saw(lds_pattern, "test_mlp")


@gpu
@pytest.mark.parametrize("i", [1, 4, 5, 9])
def test_embed_mlp_fwd(lds_pattern, i):
    """EMF_CASES: F = 1 with three ragged hidden widths, F = 4 with H = 1, F = 5 at B = 257, F = 27 (the largest K, a
    half chunk with one live field) at B = 33."""
    from tests import test_gpu_mlp_kernels as TM

    run_patterns(lambda: TM._embed_mlp_fwd_case(*TM.EMF_CASES[i]), what=f"embed_mlp_fwd {TM.EMF_CASES[i]}: ")
    _saw(lds_pattern, "test_embed_mlp_fwd")


@gpu
@pytest.mark.parametrize("B", [1, 257])
def test_linear_dense_bwd(lds_pattern, B):
    from tests import test_gpu_front_kernels as TF

    run_patterns(lambda: TF._linear_dense_bwd_case(B), what=f"linear_dense_bwd B={B}: ")
    _saw(lds_pattern, "test_linear_dense_bwd")


@gpu
@pytest.mark.parametrize("B", [1, 262_145])
def test_logit_loss(lds_pattern, B):
    """(Two sweeps of the capped grid with a ragged last block is the smallest batch the family's runner takes past
    B = 1.)"""
    from tests import test_gpu_front_kernels as TF

    for coefs, task, ydt in (TF.LOSS_CONFIGS[0], TF.LOSS_CONFIGS[-1]):
        run_patterns(lambda: TF._logit_loss_case(B, coefs, task, ydt), what=f"logit_loss B={B} {task}: ")
    _saw(lds_pattern, "test_logit_loss")


@gpu
@pytest.mark.parametrize("world", [1, 3, 16])
def test_shard_route(lds_pattern, world):
    """n = 257 (two blocks, the second with one occurrence) and 262 145 (1 024 blocks of two chunks: the running
    offsets in LDS are carried from chunk to chunk), with skipped ids; the padded form at a capacity that fits (with a
    slot too few, the clamped slot has several writers)."""
    from recman_amd import _lib
    from recman_amd.dist import route_torch
    from tests import test_gpu_front_kernels as TF

    ws = torch.empty(int(_lib.lib().rm_shard_route_workspace(world)), dtype=torch.int32, device="cuda")
    for n in (257, 262_145):
        idx, field_off = TF._route_inputs(n, TF._gen(world + n), 0.1)
        run_patterns(lambda: TF._shard_route_case(idx, field_off, world, ws, False, f"n={n}"),
                     what=f"shard_route world={world} n={n}: ")
        cap = int(route_torch(idx, field_off, world)[1].max())
        pos_t, counts_t, send_t, over_t = route_torch(idx, field_off, world, cap)
        over = torch.zeros(1, dtype=torch.int32, device="cuda")

        def check(out):
            pos, send, counts = out
            assert int(over) == 0 and int(over_t) == 0
            assert torch.equal(pos, pos_t) and torch.equal(send, send_t) and torch.equal(counts, counts_t)

        run_patterns(lambda: TF._shard_route_padded_run(idx, field_off, world, cap, over, ws), check,
                     what=f"shard_route_padded world={world} n={n}: ")
    _saw(lds_pattern, "test_shard_route")


# ------------------------------------------------------------------------------------------- the interaction kernels
def _family(state, test, run, check, what):
    run_patterns(run, check, what=what)
    _saw(state, test)


@gpu
@pytest.mark.parametrize("shape", [(5, 2, 8, 1, "each"), (33, 3, 8, 1, "all"), (37, 5, 8, 2, "each"),
                                   (6, 27, 16, 20, "each")], ids=lambda s: "B%d_F%d_D%d_R%d_%s" % s)
def test_fibinet(lds_pattern, shape):
    from tests import fibinet_ref as R
    from tests import test_gpu_fibinet as T

    case, what = R.kernel_case(*shape), f"fibinet {shape}: "
    _family(lds_pattern, "test_fibinet", lambda: T._run(case, 2), lambda out: T._check(case, what), what)


@gpu
@pytest.mark.parametrize("ftype", ["matrix", "vector", "scalar"])
@pytest.mark.parametrize("shape", [(5, 2, 8), (37, 5, 8), (6, 27, 16)], ids=lambda s: "B%d_F%d_D%d" % s)
def test_fmfm(lds_pattern, shape, ftype):
    from tests import fmfm_ref as R
    from tests import test_gpu_fmfm as T

    case, what = R.kernel_case(*shape, ftype), f"fmfm {shape} {ftype}: "
    _family(lds_pattern, "test_fmfm", lambda: T._run(case, with_up=True), lambda out: T._check(case, what), what)


@gpu
@pytest.mark.parametrize("shape,combo", [((37, 5, 8), c) for c in [(1, "mat"), (2, "mat"), (2, "vec"), (2, "num"),
                                                                  (3, "mat"), (3, "vec"), (3, "num")]]
                         + [((5, 2, 8), (3, "mat")), ((6, 27, 16), (3, "mat"))], ids=lambda v: str(v).replace(" ", ""))
def test_pnn(lds_pattern, shape, combo):
    from tests import pnn_ref as R
    from tests import test_gpu_pnn as T

    case, what = R.kernel_case(*shape, *combo, 3), f"pnn {shape} {combo}: "
    _family(lds_pattern, "test_pnn", lambda: T._run(case), lambda out: T._check(case, what), what)


@gpu
@pytest.mark.parametrize("shape", [(70, 3, 8, 2), (70, 5, 16, 3), (1, 1, 8, 1)], ids=lambda s: "B%d_F%d_D%d_N%d" % s)
def test_masknet_group(lds_pattern, shape):
    from tests import masknet_ref as R
    from tests import test_gpu_masknet as T

    c, what = R.kernel_case(*shape), f"masknet group {shape}"
    _family(lds_pattern, "test_masknet_group", lambda: T._group_run(c, pad=4), lambda out: T._check_group(c, out, what),
            what + ": ")
    p = R.plain_case(70, 64)
    run_patterns(lambda: T._plain_run(p, pad=4), lambda out: T._check_plain(p, out, "plain (70, 64)"),
                 what="masknet plain (70, 64): ")


@gpu
@pytest.mark.parametrize("shape", [(70, 8), (70, 100), (33, 2048), (1, 12)], ids=lambda s: "B%d_H%d" % s)
def test_masknet_row(lds_pattern, shape):
    from tests import masknet_ref as R
    from tests import test_gpu_masknet as T

    c, what = R.row_case(*shape), f"masknet row {shape}"
    _family(lds_pattern, "test_masknet_row", lambda: T._row_run(c), lambda out: T._check_row(c, out, what), what + ": ")


@gpu
@pytest.mark.parametrize("c", [(37, 5, 8, 8), (33, 2, 8, 4), (3, 6, 8, 8), (9, 39, 64, 64)],
                         ids=lambda c: "x".join(map(str, c)))
def test_afm(lds_pattern, c):
    from tests import afm_ref as R
    from tests import test_gpu_afm as T

    case = R.gpu_case(c)
    _family(lds_pattern, "test_afm", lambda: T._run(case, True, True),
            lambda out: [T._check(case, c, m, u) for m in (False, True) for u in (False, True)], f"afm {c}: ")


@gpu
@pytest.mark.parametrize("c", [(37, 5, 8, 2, 4), (33, 2, 8, 1, 8), (3, 6, 8, 2, 4), (9, 39, 64, 4, 16)],
                         ids=lambda c: "x".join(map(str, c)))
def test_autoint_layer(lds_pattern, c):
    from tests import autoint_ref as R
    from tests import test_gpu_autoint as T

    case = R.gpu_case(c)
    _family(lds_pattern, "test_autoint_layer", lambda: T._run(case, True, True, True),
            lambda out: [T._check(case, c, r, True, s) for r in (True, False) for s in (False, True)],
            f"autoint layer {c}: ")


@gpu
@pytest.mark.parametrize("c", [(37, 5, 8, 2, 4), (3, 6, 8, 2, 4), (9, 39, 64, 4, 16)],
                         ids=lambda c: "x".join(map(str, c)))
def test_autoint_head(lds_pattern, hip_lib, c):
    from tests import autoint_ref as R
    from tests import test_gpu_autoint as T

    case = R.gpu_case(c)
    Y = R.layer_reference(case, True, False, False)[0].float().double()
    _family(lds_pattern, "test_autoint_head", lambda: T._run_head(case, Y),
            lambda out: T.test_head_kernels_match_float64_and_two_runs_are_bit_equal(hip_lib, c), f"autoint head {c}: ")


@gpu
@pytest.mark.parametrize("c", [(3, 1, 8), (5, 2, 16), (6, 7, 16), (9, 31, 16), (4, 40, 64)],
                         ids=lambda c: "x".join(map(str, c)))
def test_dot_interact(lds_pattern, hip_lib, c):
    from tests import dlrm_ref as R
    from tests import test_gpu_dot_interact as T

    case = R.kernel_case(*c)
    ldx = T._strides(c[1], c[2])[1][1]
    _family(lds_pattern, "test_dot_interact", lambda: T._run(case, ldx),
            lambda out: T.test_dot_interact_matches_float64(hip_lib, c), f"dot_interact {c}: ")


@gpu
@pytest.mark.parametrize("shape", [(5, 1, 8), (33, 3, 8), (9, 5, 16), (65, 2, 64)], ids=lambda s: "B%d_E%d_r%d" % s)
def test_cross_mix(lds_pattern, shape):
    from tests import crossmix_ref as R
    from tests import test_gpu_cross_mix as T

    case, what = R.kernel_case(*shape), f"cross_mix {shape}: "
    _family(lds_pattern, "test_cross_mix", lambda: T._run(case, 2), lambda out: T._check(case, what), what)


@gpu
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (33, 16, 8, 36), (64, 4, 3, 8), (77, 8, 2, 128)],
                         ids=lambda s: "B%d_E%d_T%d_H%d" % s)
def test_mmoe_mix(lds_pattern, hip_lib, shape):
    from tests import mmoe_ref as R
    from tests import test_gpu_mmoe as T

    c = R.mix_case(*shape)
    _family(lds_pattern, "test_mmoe_mix", lambda: T._run(c, pad=4, want_p=True)[0],
            lambda out: T.test_mixture_matches_float64(hip_lib, shape), f"mmoe mix {shape}: ")


@gpu
@pytest.mark.parametrize("B", [1, 77])
@pytest.mark.parametrize("T_", [1, 2, 8])
def test_multitask_loss(lds_pattern, hip_lib, T_, B):
    from tests import mmoe_ref as R
    from tests import test_gpu_mmoe as T

    c = R.loss_case(T_, B)
    _family(lds_pattern, "test_multitask_loss", lambda: T._loss_run(c),
            lambda out: T.test_loss_head_matches_float64(hip_lib, T_, B), f"multitask loss T={T_} B={B}: ")


@gpu
@pytest.mark.parametrize("B,H,splits", [(1, 4, 0), (15, 8, 0), (17, 20, 0), (65, 64, 0), (130, 36, 0), (130, 36, 2)])
def test_inbatch_softmax(lds_pattern, B, H, splits):
    from tests import test_gpu_twotower as T
    from tests import twotower_ref as R

    k, what = R.ibs_case(B, H, True, True, True), f"inbatch softmax B={B} H={H} splits={splits}"

    def check(out):
        T._check_all(what, out, k)
        R.check_ranks(out["rank"], k, what=what + ": ")

    _family(lds_pattern, "test_inbatch_softmax", lambda: T._run(k, splits=splits, pad=4)[0], check, what + ": ")


# ------------------------------------------------------------------------------------------ the sequence units
@gpu
@pytest.mark.parametrize("name", ["d16_80x40_relu_norm", "d8_36_relu", "d32_16x8_sigmoid_norm", "d8_128_sigmoid_norm"])
def test_asp(lds_pattern, name):
    from tests import asp_ref as R
    from tests import test_gpu_asp as T

    case = R.make_asp_case(**R.GPU_CASES[name])
    _family(lds_pattern, "test_asp", lambda: T._run(case), lambda out: T._check(case, name), f"asp {name}: ")


@gpu
@pytest.mark.parametrize("name", ["d16_h2_f64", "d8_h2_f128_short", "d16_h4_f20", "d32_h8_f128"])
def test_bst(lds_pattern, name):
    from tests import test_gpu_bst as T

    case, want, cpu32 = T._case(name)
    _family(lds_pattern, "test_bst", lambda: T._run(case), lambda out: T._check(case, want, cpu32, name), f"bst {name}: ")


@gpu
@pytest.mark.parametrize("name", ["d16", "d16_len1", "d8_many", "d32"])
def test_dien(lds_pattern, name):
    from tests import test_gpu_dien as T

    case, want, cpu32 = T._case(name)
    _family(lds_pattern, "test_dien", lambda: T._run(case), lambda out: T._check(case, want, cpu32, name),
            f"dien {name}: ")


# ------------------------------------------------------------------------------------------------- the optimizers
@gpu
@pytest.mark.parametrize("name", ["d8_adam_fields", "d12_adagrad_pairs", "d32_adam_rows", "d64_sgd_rows",
                                  "d24_adam_pairs"])
def test_sparse_optimizer(lds_pattern, name):
    """Every entry (per-field ids, all pairs, packed rows), every rule, D = 8 .. 64 (4 .. 32 lanes per row); the cases'
    runs go from one occurrence to 1 025 (inline, handed over, nine segments), and their keys fill more than one block
    of the apply kernel."""
    from recman_amd import ops
    from tests import optim_ref as R
    from tests import test_gpu_optim_kernels as T

    case = R.make_case(**R.SPARSE_CASES[name])
    assert case["prepared_at"], "the case runs rm_sparse_optimizer_prepare"
    run_patterns(lambda: T._run(case, ops), lambda out: T._check_case(case, ops, name), what=f"optimizer {name}: ")
    for entry in R.ENTRIES:
        small = R.small_case("n_odd", 12, "adam", entry)
        run_patterns(lambda: T._run(small, ops), lambda out: T._check_case(small, ops, f"n_odd {entry}", full=False),
                     what=f"optimizer n_odd {entry}: ")
    _saw(lds_pattern, "test_sparse_optimizer")


@gpu
@pytest.mark.parametrize("name", ["d8_ftrl_fields", "d12_ftrl_pairs", "d64_ftrl_rows", "d8_adam_ftrl_fields",
                                  "d24_sgd_ftrl_rows"])
def test_sparse_optimizer_rules(lds_pattern, name):
    from recman_amd import ops
    from tests import optim_ftrl_ref as FR
    from tests import test_gpu_optim_ftrl as T

    case = FR.make_case(**{**FR.FTRL_CASES, **FR.SPLIT_CASES}[name])
    run_patterns(lambda: T._run(case, ops), lambda out: T._check_case(case, ops, name), what=f"optimizer {name}: ")
    other = FR.make_case(**FR.FTRL_CASES["d12_ftrl_rows" if case["entry"] != "rows" else "d12_ftrl_fields"])
    run_patterns(lambda: T._run(other, ops), what="optimizer, the other entry: ")
    assert {"rm_sparse_optimizer_step_rules", "rm_sparse_optimizer_step_rows_rules"} <= lds_pattern["seen"]
    assert lds_pattern["fills"] > 0


@gpu
@pytest.mark.parametrize("kind", ["adam", "adagrad", "sgd"])
def test_sparse_optimizer_old_entries(lds_pattern, kind):
    """The entry points that take the rule's constants as arguments (ops goes through the *_rules ones): the case and
    the assertion of test_gpu_optim_ftrl's comparison of the two."""
    from recman_amd import _lib, ops
    from tests import optim_ftrl_ref as FR
    from tests import optim_ref as R
    from tests import test_gpu_optim_ftrl as T

    for entry in ("fields", "rows"):
        case = FR.reseed(R.make_case(16, "adam", entry, prepared_at=()), kind)

        def check(old):
            new = T._run(case, ops)
            for s_ in range(3):
                assert torch.equal(new[s_][0], old[s_][0]), (kind, entry, s_)
                assert kind == "sgd" or torch.equal(new[s_][1], old[s_][1]), (kind, entry, s_)

        run_patterns(lambda: T._old_entry(case, _lib), check, what=f"optimizer, old entry {kind} {entry}: ")
    _saw(lds_pattern, "test_sparse_optimizer_old_entries")


# ---------------------------------------------------------------------------------------------------- the metrics
@gpu
@pytest.mark.parametrize("n", [2, 65, 4097, 2 ** 16 + 3])
def test_metrics(lds_pattern, hip_lib, n):
    """Below one tile, a tile and one element, several tiles with a ragged last one, several blocks."""
    from recman_amd.metrics import log_loss, roc_auc_score
    from tests import test_gpu_metrics as T

    for kind in ("general", "q8", "signed_zero"):
        rng = np.random.default_rng(n * 31 + T.KINDS.index(kind))
        y, s = T.scores_of(kind, n, rng)
        yt, st = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
        run_patterns(lambda: roc_auc_score(yt, st),
                     lambda out: T.test_auc_equals_the_exact_rational_and_sklearn(hip_lib, kind, n),
                     what=f"roc_auc {kind} n={n}: ")
    if n in (2, 65, 4097):
        rng = np.random.default_rng(n)
        y = (rng.random(n) < 0.3).astype(np.int64)
        y[0], y[1] = 1, 0   # both classes
        yl = torch.from_numpy(y).cuda()
        pl = torch.from_numpy(rng.random(n).astype(np.float32)).cuda()
        run_patterns(lambda: log_loss(yl, pl), lambda out: T.test_log_loss_against_sklearn(hip_lib, n, "int64"),
                     what=f"log_loss n={n}: ")
        _saw(lds_pattern, "test_metrics")
    assert "rm_roc_auc" in lds_pattern["seen"] and lds_pattern["fills"] > 0


@gpu
@pytest.mark.parametrize("n", [1, 65, 4097, 12_289])
@pytest.mark.parametrize("layout", ["pairs", "skewed", "zipf24", "gap"])
def test_group_auc(lds_pattern, hip_lib, layout, n):
    from tests import test_gpu_gauc as T

    rng = np.random.default_rng(2019 + 97 * T.SIZES.index(n) + T.LAYOUTS.index(layout))
    g = T.groups_of(layout, n, rng)
    y, s = T.scores_of("general", n, rng)

    def run():
        rec, rows = T.run(y, s, g, 0)
        return torch.tensor([float(v) for v in rec], dtype=torch.float64), torch.tensor(rows, dtype=torch.int64)

    _family(lds_pattern, "test_group_auc", run,
            lambda out: T.test_group_auc_equals_the_exact_reference(hip_lib, layout, n), f"gauc {layout} n={n}: ")


# ---------------------------------------------------------------------------------------------------- the engines
@gpu
@pytest.mark.parametrize("model,kw", [("deepfm", dict(D=16, hp_extra=dict(step_fusion=True))),
                                      ("deepfm", dict(D=16, hp_extra=dict(step_fusion=False))),
                                      ("xdeepfm", dict(D=16, cin_units=(32, 32, 16), scale=0.2)),
                                      ("dcn", dict(D=8, cross_layers=3, scale=0.15))],
                         ids=["deepfm-step", "deepfm", "xdeepfm", "dcn"])
def test_engines(lds_pattern, hip_lib, model, kw):
    """Whole fwd_bwd passes at B = 37: every kernel of the model behind known LDS contents, each after the others."""
    from tests import test_gpu_parity as TP

    def run():
        e = TP._check_model(model, hip_lib, B=37, **kw)
        return dict(loss=e.loss, logit=e.logit, pred=e.pred)

    run_patterns(run, what=f"{model} {kw}: ")
    fused = kw.get("hp_extra", {}).get("step_fusion")
    if fused is not None:
        assert ("rm_deepfm_step" in lds_pattern["seen"]) == fused
    assert lds_pattern["fills"] > 0


@gpu
@pytest.mark.parametrize("name", ["dlrm", "fibinet_each", "pnn_inner", "pnn_outer_vec"])
def test_interaction_engines(lds_pattern, hip_lib, name):
    from tests import test_gpu_interaction_engines as TI

    k, _, _ = TI._twin(name, True)
    idx, dense, y = k["idx"].cuda(), k["dense"].to(torch.float32).cuda(), k["y"].cuda()

    def run():
        e = TI.CASES[name][2](k)
        loss = e.fwd_bwd(idx, dense, y)
        return dict(loss=loss, logit=e.logit, pred=e.pred, d_rows=e.d_rows)

    run_patterns(run, lambda out: TI.test_pad_columns_and_the_float64_twin_across_batch_sizes(hip_lib, name, True),
                 what=f"{name}: ")
    assert lds_pattern["fills"] > 0
