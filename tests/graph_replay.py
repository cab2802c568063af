"""Test aids for replaying an engine's step from a hipGraph (a plain module like tests/stale_state.py, not a conftest),
as far as they need no GPU: the batch permutation, and the ledger of which entry points a captured step is known to
contain.  tests/test_graph_replay_host.py checks both.

A capture of engine.fwd_bwd requires (recman_amd/engine.py): the engine warmed at that batch size; the optimizers
built before it and their step() kept outside the graph (it takes the step count t by value); no call at another batch
size between capture and replay.

permuted_batch(...)  the same examples in reverse order: same shapes, same nnz, other contents at every position
CASES                one row per engine route: its engine, its case, the entry points its capture contains
NOT_IN_A_STEP        entry points no row's capture contains, with the reason
PENDING              entry points read off the engines' code that a row is expected to capture, not yet observed
"""
import types

import torch


def _flip(t):
    return None if t is None else torch.flip(t, dims=[0]).contiguous()


def _flip_nested(x):
    if x is None or torch.is_tensor(x):
        return _flip(x)
    if isinstance(x, dict):
        return {k: _flip_nested(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_flip_nested(v) for v in x)
    raise TypeError(f"masks: {type(x).__name__} is neither a tensor nor a container of them")


def permuted_csr(offsets, *per_item):
    """A CSR (offsets [B + 1], then tensors with one entry per item: ids, values) with the examples in reverse order:
    example b's slice moves to position B - 1 - b whole.  -> (offsets, *per_item) of the same lengths."""
    n = offsets[1:] - offsets[:-1]
    B = int(n.shape[0])
    new_off = torch.cat([offsets[:1] * 0, torch.cumsum(torch.flip(n, dims=[0]), 0)]).to(offsets.dtype)
    bounds = offsets.tolist()
    order = [i for b in range(B - 1, -1, -1) for i in range(bounds[b], bounds[b + 1])]
    order = torch.tensor(order, dtype=torch.int64, device=offsets.device)
    return (new_off,) + tuple(t[order].contiguous() for t in per_item)


def permuted_batch(idx, dense, y, masks=None, mv=None):
    """-> (idx, dense, y, masks, mv): the batch with its examples in reverse order.  idx, dense, y (or Y) and every
    given dropout mask are flipped along dim 0; every CSR input of mv (name -> (offsets, ids) or (offsets, ids, vals):
    multi-valued, value and sequence features) keeps each example's slice intact at its new position, so the offsets'
    contents change while their length, the ids' length and the total nnz do not.  No random draw."""
    mv_p = None
    if mv is not None:
        mv_p = {name: permuted_csr(ent[0], *ent[1:]) for name, ent in mv.items()}
    return _flip(idx), _flip(dense), _flip(y), _flip_nested(masks), mv_p


# ------------------------------------------------------------------------------------------------------ the ledger
def _row(engine, case, claims=None):
    """claims: the entry points seen through recman_amd._lib.call while the row's fwd_bwd was being captured on the
    MI355X (a set), or None: the row's capture has not been observed."""
    return types.SimpleNamespace(engine=engine, case=case, claims=None if claims is None else set(claims))


_STEP_CASE = 'tests/cases.py make_case("deepfm", D=16, B=37, F=5, Dn=3, hidden=(32, 32)), '
_HEAD = {"rm_embed_fwd", "rm_logit_loss", "rm_linear_dense_bwd"}  # gather + linear, the loss head, the linear term's dense gradient
_SKINNY = {"rm_mlp_fwd", "rm_mlp_bwd"}

# One row per engine route: each model's smallest existing case whose batch is no multiple of 32, from the model's own
# test module and twin (the xDeepFM and MMoE rows say why they take another).
CASES = {
    "deepfm_step": _row("deepfm", _STEP_CASE + "step_fusion=True"),
    "deepfm_front": _row("deepfm", _STEP_CASE + "step_fusion=False", {"rm_embed_mlp_fwd", "rm_mlp_bwd"}),
    "deepfm_chain": _row("deepfm", _STEP_CASE + "step_fusion=False, front_fusion=False", {"rm_embed_fwd"} | _SKINNY),
    "deepfm_rank_pairwise": _row("deepfm", "tests/test_gpu_rank_model.py _deepfm_case() (B=300), pairwise, group norm",
                                 {"rm_embed_mlp_fwd", "rm_logit_loss", "rm_rank_loss", "rm_mlp_bwd"}),
    "dcn_vector": _row("dcn", 'make_case("dcn", B=37, D=8, cross_layers=3, scale=0.15)',
                       _HEAD | _SKINNY | {"rm_cross_fwd", "rm_cross_bwd", "rm_cross_param_grads", "rm_dense_wgrad"}),
    "dcn_matrix": _row("dcn", "test_dcn_matrix_cross_fwd_bwd_matches_oracle at (B, L, use_linear) = (33, 2, True)",
                       _HEAD | _SKINNY | {"rm_dense_fwd", "rm_dense_wgrad", "rm_rowdot"}),
    "dcn_mix": _row("dcn", "crossmix_ref.MODEL_CASES['e1_r8'] (B=33)",
                    _HEAD | _SKINNY | {"rm_dense_fwd", "rm_dense_wgrad", "rm_rowdot", "rm_cross_mix_fwd",
                                       "rm_cross_mix_bwd"}),
    # the Criteo-like CIN: the smallest xDeepFM case whose layers the split-operand kernels take in the forward
    # (cin_filter_workspace6 > 0: D = 16, H <= 64, N <= 128) and in the backward (N > 64)
    "xdeepfm_bf16x6": _row("xdeepfm", 'make_case("xdeepfm", D=16, B=70, F=26, Dn=13, hidden=(32, 32), '
                                      'cin_units=(128, 128), scale=0.05)'),
    "xdeepfm_f32": _row("xdeepfm", 'make_case("xdeepfm", D=16, B=37, cin_units=(32, 32, 16), scale=0.2), '
                                   'cin_gemm="f32", dense_gemm="f32"'),
    "afm": _row("afm", "afm_ref.MODEL_CASES['d8'] (B=37)", _HEAD | {"rm_afm_fwd", "rm_afm_bwd"}),
    "afm_multi_valued_and_value": _row("afm", "test_afm_multi_valued_and_value_features' case (B=37)",
                                       _HEAD | {"rm_afm_fwd", "rm_afm_bwd", "rm_pool_rows"}),
    "autoint": _row("autoint", "autoint_ref.MODEL_CASES['d8'] (B=37)",
                    _HEAD | {"rm_autoint_layer_fwd", "rm_autoint_layer_bwd", "rm_autoint_head_fwd",
                             "rm_autoint_head_bwd"}),
    "dlrm": _row("dlrm", "dlrm_ref.MODEL_CASES['d8'] (B=37)"),
    "fibinet": _row("fibinet", "fibinet_ref.MODEL_CASES['each_d8'] (B=33)"),
    "fibinet_given_dropout_masks": _row("fibinet", "test_fibinet_deep_dropout_with_given_masks' case: the masks in "
                                                   "static buffers"),
    "fmfm": _row("fmfm", "fmfm_ref.MODEL_CASES['scalar_no_dnn'] (B=33)"),
    "pnn_inner": _row("pnn", "pnn_ref.MODEL_CASES['inner_only'] (B=33)"),
    "pnn_outer": _row("pnn", "pnn_ref.MODEL_CASES['outer_vec_linear'] (B=257)"),
    "masknet_serial": _row("masknet", "masknet_ref.MODEL_CASES['serial1'] (B=33)"),
    "masknet_parallel": _row("masknet", "masknet_ref.MODEL_CASES['parallel3'] (B=130)"),
    "din": _row("din", "asp_ref.MODEL_CASES['din_d8'] (B=37) with its history"),
    "bst": _row("bst", "bst_ref.MODEL_CASES['bst_d8'] (B=37) with its history",
                {"rm_embed_fwd", "rm_bst_fwd", "rm_bst_bwd"} | _SKINNY),
    "dien": _row("dien", "dien_ref.MODEL_CASES['dien_d8'] (B=37) with its history"),
    # (MMoE's cases have B = 66 .. 71: the one with unobserved labels, whose counts a capture could freeze)
    "mmoe": _row("mmoe", "mmoe_ref.MODEL_CASES['three_tasks_nan'] (B=71)"),
    "ple_entire_space": _row("ple", "ple_ref.MODEL_CASES['entire_space_ple'] (B=69)"),
    "twotower": _row("twotower", "twotower_ref.make_case(True, True, True, True) (B=37): normalised, accidental hits "
                                 "masked, logQ, row weights"),
}

_OPT = "an optimizer step takes the step count t by value: it runs outside the graph (recman_amd/optim.py)"
_METRIC = "a metric of evaluate() / fit()'s validation pass, not of a training step (recman_amd/metrics.py)"
_DIST = "routing / packing of the row-sharded engines (recman_amd/dist.py): tests/test_gpu_dist.py replays their segments"
_DEBUG = "a test aid (tests/stale_state.py), never part of a step"
_AFTER = "densifies the sparse gradients after the step (Engine.dense_grads): float atomics, outside fwd_bwd"
_LAYERS = "called by recman_amd/th/layers.py alone, by no engine's fwd_bwd"
NOT_IN_A_STEP = {
    "rm_dense_optimizer_step": "old ABI kept for compatibility; " + _OPT,
    "rm_dense_optimizer_step_rule": _OPT,
    "rm_sparse_optimizer_prepare": _OPT,
    "rm_sparse_optimizer_step": "old ABI kept for compatibility; " + _OPT,
    "rm_sparse_optimizer_step_rows": "old ABI kept for compatibility; " + _OPT,
    "rm_sparse_optimizer_step_rows_rules": _OPT,
    "rm_sparse_optimizer_step_rules": _OPT,
    "rm_roc_auc": _METRIC,
    "rm_log_loss": _METRIC,
    "rm_group_auc": _METRIC,
    "rm_group_gain": _METRIC,
    "rm_topk_ip": "retrieval over a catalogue (TwoTowerEngine.topk), not a training step",
    "rm_shard_route": _DIST,
    "rm_shard_route_padded": _DIST,
    "rm_gather_rows": _DIST + "; also the feeder's gather (recman_amd/th/feeder.py)",
    "rm_permute_rows": _DIST,
    "rm_pack_grad_rows": _DIST,
    "rm_pack_pooled_grad_rows": _DIST,
    "rm_pool_rows_padded": _DIST,
    "rm_debug_lds_fill": _DEBUG,
    "rm_debug_lds_probe": _DEBUG,
    "rm_profile_marker": "the profile marker of tools/, a named empty kernel",
    "rm_scatter_add_rows": _AFTER,
    "rm_pool_rows_bwd": _AFTER,
    "rm_linear_fwd": _LAYERS,
    "rm_bias_act": _LAYERS,
    "rm_embed_bwd": "in DeepFM's step only with FM dropout masks or use_deep=False, routes no row takes: not covered",
    "rm_outer_actgrad_sums": "in a wide DNN's backward only with a last hidden width >= 64, which no row has: not covered",
}

# entry point -> the rows whose engine code launches it (read off recman_amd/engine.py and ops.py), none of which has
# been observed yet.  An entry leaves this table when a row's observed claims hold it.
PENDING = {
    "rm_deepfm_step": ["deepfm_step"],
    "rm_cin_layer_fwd6": ["xdeepfm_bf16x6"],
    "rm_cin_layer_fwd": ["xdeepfm_f32"],
    "rm_cin_layer_bwd": ["xdeepfm_bf16x6", "xdeepfm_f32"],
    "rm_dot_interact_fwd": ["dlrm"],
    "rm_dot_interact_bwd": ["dlrm"],
    "rm_fibinet_fwd": ["fibinet", "fibinet_given_dropout_masks"],
    "rm_fibinet_bwd": ["fibinet", "fibinet_given_dropout_masks"],
    "rm_fmfm_fwd": ["fmfm"],
    "rm_fmfm_bwd": ["fmfm"],
    "rm_pnn_fwd": ["pnn_inner", "pnn_outer"],
    "rm_pnn_bwd": ["pnn_inner", "pnn_outer"],
    "rm_masknet_group_fwd": ["masknet_serial", "masknet_parallel"],
    "rm_masknet_group_bwd": ["masknet_serial", "masknet_parallel"],
    "rm_masknet_row_fwd": ["masknet_serial", "masknet_parallel"],
    "rm_masknet_row_bwd": ["masknet_serial", "masknet_parallel"],
    "rm_asp_fwd": ["din"],
    "rm_asp_bwd": ["din"],
    "rm_dien_fwd": ["dien"],
    "rm_dien_bwd": ["dien"],
    "rm_mmoe_mix_fwd": ["mmoe"],
    "rm_mmoe_mix_bwd": ["mmoe"],
    "rm_multitask_loss": ["mmoe"],
    "rm_cgc_mix_fwd": ["ple_entire_space"],
    "rm_cgc_mix_bwd": ["ple_entire_space"],
    "rm_multitask_loss_es": ["ple_entire_space"],
    "rm_inbatch_softmax_fwd": ["twotower"],
    "rm_inbatch_softmax_bwd": ["twotower"],
    "rm_rownorm_fwd": ["twotower"],
    "rm_rownorm_bwd": ["twotower"],
    "rm_act_bwd": ["mmoe", "ple_entire_space", "twotower", "fibinet_given_dropout_masks"],
    "rm_dense_fwd6": ["fibinet", "masknet_parallel", "mmoe", "ple_entire_space", "twotower"],
    "rm_dense_wgrad6": ["fibinet", "masknet_parallel", "mmoe", "ple_entire_space", "twotower"],
    "rm_outer_actgrad": ["fibinet", "masknet_parallel"],
}
