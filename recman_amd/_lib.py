"""ctypes binding of librecman_hip.so (the C ABI declared in include/recman_hip.h, include/recman_hip_topk.h,
include/recman_hip_multitask.h, include/recman_hip_rank.h and include/recman_hip_rankmetrics.h).

There is NO fallback: if the library is missing or a symbol does not resolve the
import raises, and every call that returns a non-zero code raises RecmanHipError
with the library's thread-local message.  The product path never computes on the CPU.
"""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# RECMAN_HIP_LIB: load another build of the same library (kernel experiments); default in-tree
LIB_PATH = os.environ.get("RECMAN_HIP_LIB") or os.path.join(_HERE, "csrc", "librecman_hip.so")


class RecmanHipError(RuntimeError):
    pass


P = c_void_p  # every device pointer and the stream travel as void*
I64 = c_int64

class MlpTail(ctypes.Structure):
    """rm_mlp_tail of include/recman_hip.h (the fused training head of the skinny MLP)."""
    _fields_ = [("logit_a", P), ("coef_a", c_float), ("logit_b", P), ("coef_b", c_float),
                ("coef_mlp", c_float), ("y", P), ("y_f", P), ("task", c_int), ("grad_scale", c_float),
                ("logit", P), ("pred", P), ("dlogit", P), ("loss_partial", P), ("loss", P),
                ("dh", P * 3)]


class OptRule(ctypes.Structure):
    """rm_opt_rule of include/recman_hip.h: one update rule (kind 0 Adam, 1 Adagrad, 2 SGD, 3 FTRL)."""
    _fields_ = [("kind", c_int), ("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float),
                ("l1", c_float), ("l2", c_float), ("beta", c_float)]


BST_PARAM_NAMES = ("wq", "wk", "wv", "wo", "bq", "bk", "bv", "bo", "ffn_w1", "ffn_b1", "ffn_w2", "ffn_b2", "ln1_gamma",
                   "ln1_beta", "ln2_gamma", "ln2_beta", "pos")


class BstParams(ctypes.Structure):
    """rm_bst_params of include/recman_hip.h: the 17 device pointers of the transformer unit (or of its gradients)."""
    _fields_ = [(n, P) for n in BST_PARAM_NAMES]


DIEN_PARAM_NAMES = ("gru_w", "gru_u", "gru_b", "att_w", "augru_w", "augru_u", "augru_b")


class DienParams(ctypes.Structure):
    """rm_dien_params of include/recman_hip.h: the 7 device pointers of the interest-evolution unit (or of its
    gradients)."""
    _fields_ = [(n, P) for n in DIEN_PARAM_NAMES]


# name -> argtypes, in the order of include/recman_hip.h
SIGNATURES = {
    "rm_version": [],
    "rm_device_cus": [],
    "rm_profile_marker": [c_int, P],
    "rm_embed_fwd": [P, P, I64, P, P, I64, P, I64, P, P, P, P, c_int, P, P, I64, c_int, c_int,
                     P, P, P, P, c_int, P],
    "rm_linear_fwd": [P, P, P, P, P, P, I64, c_int, c_int, P, P],
    "rm_embed_bwd": [P, P, P, P, P, P, I64, c_int, c_int, P, P, P],
    "rm_scatter_add_rows": [P, P, P, P, I64, c_int, c_int, I64, P, P],
    "rm_linear_dense_bwd": [P, P, I64, c_int, P, P, P, P],
    "rm_logit_loss": [P, c_float, P, c_float, P, c_float, P, c_float, P, P, c_int, I64, P, P, P,
                      P, P, P],
    "rm_mlp_supported": [c_int, c_int, c_int, P],
    "rm_mlp_fwd": [P, P, c_int, c_int, c_int, P, P, P, P, P, c_int, I64, P, P, P, P],
    "rm_embed_mlp_fwd_supported": [c_int, c_int, I64, c_int, c_int, P],
    "rm_embed_mlp_fwd": [P, P, I64, P, c_int, c_int, P, P, P, c_int, I64, c_int, c_int, P, P, P, P, c_int,
                         c_int, P, P, P, P, P, c_int, P, P, P, P],
    "rm_mlp_bwd": [P, P, c_int, c_int, c_int, P, P, P, c_int, I64, P, P, P, c_int, P, P, P, P, P, P,
                   P, P, P, P, c_int, P],
    "rm_deepfm_step_supported": [c_int, c_int, I64, c_int, c_int, P],
    "rm_deepfm_step": [P, P, I64, P, P, c_int, P, P, I64, c_int, c_int, c_int, P, P, P, P, P, P, P, c_int, c_int,
                       c_float, P, P, P, P, P, P, P, P, P, P, P, P, I64, P, c_int, P],
    "rm_debug_lds_fill": [ctypes.c_uint, P],
    "rm_debug_lds_probe": [ctypes.c_uint, P, c_int, P],
    "rm_bias_act": [P, P, I64, c_int, c_int, P],
    "rm_act_bwd": [P, P, I64, c_int, c_int, P],
    "rm_outer_actgrad": [P, P, P, I64, c_int, c_int, P, P],
    "rm_outer_actgrad_sums": [P, P, P, I64, c_int, c_int, P, P, P, P, P, P],
    "rm_rowdot": [P, P, P, I64, c_int, P, P],
    "rm_cross_fwd": [P, P, c_int, c_int, P, P, P, c_int, I64, P, P, c_int, P],
    "rm_cross_bwd": [c_int, c_int, P, P, P, c_int, I64, P, P, c_int, P, P, P, P],
    "rm_cross_param_grads": [P, P, P, P, P, c_int, c_int, P, P, P, P],
    "rm_afm_supported": [c_int, c_int, c_int],
    "rm_afm_fwd": [P, P, P, P, P, P, I64, c_int, c_int, c_int, P, P, P],
    "rm_afm_bwd": [P, P, P, P, P, P, P, P, P, P, I64, c_int, c_int, c_int, P, P, P, P, P, P, P],
    "rm_autoint_supported": [c_int, c_int, c_int, c_int],
    "rm_autoint_layer_fwd": [P, P, P, P, P, I64, c_int, c_int, c_int, c_int, c_float, P, P, P],
    "rm_autoint_layer_bwd": [P, P, P, P, P, P, P, P, I64, c_int, c_int, c_int, c_int, c_float, P, P, P, P, P, P, P,
                             P],
    "rm_autoint_head_fwd": [P, P, P, I64, c_int, P, P],
    "rm_autoint_head_bwd": [P, P, P, I64, c_int, P, P, P, P, P],
    "rm_dot_interact_supported": [c_int, c_int],
    "rm_dot_interact_fwd": [P, P, I64, c_int, c_int, P, I64, P],
    "rm_dot_interact_bwd": [P, P, P, I64, I64, c_int, c_int, P, P, P],
    "rm_cross_mix_supported": [c_int, c_int],
    "rm_cross_mix_fwd": [P, I64, P, I64, P, c_int, c_int, I64, P, I64, P],
    "rm_cross_mix_bwd": [P, I64, P, I64, P, c_int, c_int, I64, P, I64, P, I64, P, I64, P, P, P],
    "rm_fibinet_supported": [c_int, c_int, c_int, c_int],
    "rm_fibinet_tile": [c_int, c_int, c_int, c_int, c_int],
    "rm_fibinet_fwd": [P, P, P, P, P, I64, c_int, c_int, c_int, c_int, P, I64, P],
    "rm_fibinet_bwd": [P, P, P, P, P, P, I64, I64, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P],
    "rm_fmfm_supported": [c_int, c_int, c_int],
    "rm_fmfm_tile": [c_int, c_int, c_int, c_int],
    "rm_fmfm_fwd": [P, P, c_int, I64, c_int, c_int, P, P],
    "rm_fmfm_bwd": [P, P, c_int, P, P, I64, c_int, c_int, P, P, P, P],
    "rm_pnn_supported": [c_int, c_int, c_int, c_int],
    "rm_pnn_tile": [c_int, c_int, c_int, c_int, c_int],
    "rm_pnn_fwd": [P, P, c_int, c_int, I64, c_int, c_int, P, I64, P],
    "rm_pnn_bwd": [P, P, c_int, c_int, P, I64, I64, c_int, c_int, P, P, P, P],
    "rm_masknet_group_supported": [c_int, c_int, c_int, c_int],
    "rm_masknet_group_tile": [c_int, c_int, c_int, c_int],
    "rm_masknet_group_fwd": [P, P, P, c_int, P, I64, c_int, I64, c_int, c_int, P, I64, P],
    "rm_masknet_group_bwd": [P, P, P, c_int, P, I64, P, I64, P, I64, c_int, P, I64, c_int, c_int, P, P, P, P, P],
    "rm_masknet_row_supported": [c_int],
    "rm_masknet_row_tile": [c_int, c_int],
    "rm_masknet_row_fwd": [P, P, P, I64, c_int, P, I64, P],
    "rm_masknet_row_bwd": [P, P, P, P, I64, I64, c_int, P, P, P, P, P],
    "rm_asp_supported": [c_int, c_int, P, c_int],
    "rm_asp_fwd": [P, I64, c_int, I64, P, P, P, I64, I64, P, P, P, P, P, P, c_int, P, c_int, c_int, P, P, P, P],
    "rm_asp_bwd": [P, I64, c_int, I64, P, P, P, I64, I64, P, P, P, P, P, P, c_int, P, c_int, c_int, P, P, I64, P, P,
                   I64, P, P, P, P, P, P, P, P],
    "rm_bst_supported": [c_int, c_int, c_int, c_int],
    "rm_bst_fwd": [P, I64, c_int, I64, P, P, P, I64, I64, P, c_int, c_int, c_int, P, P, P],
    "rm_bst_bwd": [P, I64, c_int, I64, P, P, P, I64, I64, P, c_int, c_int, c_int, P, I64, P, P, I64, P, P, P],
    "rm_dien_supported": [c_int, c_int],
    "rm_dien_fwd": [P, I64, c_int, I64, P, P, P, I64, I64, P, c_int, c_int, P, P, P],
    "rm_dien_bwd": [P, I64, c_int, I64, P, P, P, I64, I64, P, c_int, P, I64, P, P, I64, P, P, P],
    "rm_cin_layer_fwd": [P, P, I64, P, P, c_int, I64, c_int, c_int, c_int, c_int, P, P, c_int, c_int,
                         c_int, P, P],
    "rm_cin_layer_fwd6": [P, P, I64, P, P, c_int, I64, c_int, c_int, c_int, c_int, P, P, c_int, c_int,
                         c_int, P, P],
    "rm_cin_layer_bwd": [P, P, I64, c_int, P, c_int, P, P, I64, P, P, c_int, I64, c_int, c_int, c_int,
                         c_int, P, c_int, P, I64, P, P, P, I64, P],
    "rm_pool_rows": [P, I64, c_int, c_int, P, P, P, I64, P, P],
    "rm_pool_rows_bwd": [P, I64, P, P, c_int, P, P, P, I64, I64, P, P, P, P],
    "rm_pool_rows_padded": [P, c_int, c_int, P, I64, P, I64, P, I64, I64, c_int, P, P],
    "rm_pack_pooled_grad_rows": [P, I64, P, P, c_int, P, I64, P, I64, P, I64, I64, c_int, c_int, P, P],
    "rm_sparse_optimizer_prepare": [P, P, P, I64, c_int, I64, I64, P, I64, P],
    "rm_sparse_optimizer_step": [P, P, P, P, P, I64, c_int, c_int, I64, P, I64, P, c_int, c_int,
                                 c_float, c_float, c_float, c_float, c_int, c_float, c_float, P, I64, c_int, P, I64, P],
    "rm_sparse_optimizer_step_rows": [P, P, I64, I64, c_int, I64, P, I64, P, c_int, c_int,
                                      c_float, c_float, c_float, c_float, c_int, c_float, c_float, c_int, P, I64, P],
    "rm_dense_optimizer_step": [P, P, P, P, I64, c_int, c_int, c_float, c_float, c_float, c_float, c_int, P],
    "rm_sparse_optimizer_step_rules": [P, P, P, P, P, I64, c_int, c_int, I64, P, I64, P, c_int, P, P, c_int,
                                       c_float, c_float, P, I64, c_int, P, I64, P],
    "rm_sparse_optimizer_step_rows_rules": [P, P, I64, I64, c_int, I64, P, I64, P, c_int, P, P, c_int,
                                            c_float, c_float, c_int, P, I64, P],
    "rm_dense_optimizer_step_rule": [P, P, P, P, I64, c_int, P, c_int, P],
    "rm_shard_route": [P, P, I64, c_int, c_int, P, P, P, P, P],
    "rm_shard_route_padded": [P, P, I64, c_int, c_int, I64, P, P, P, P, P, P],
    "rm_pack_grad_rows": [P, P, P, P, P, I64, c_int, c_int, c_int, P, P],
    "rm_gather_rows": [P, I64, P, I64, c_int, P, P],
    "rm_permute_rows": [P, P, I64, c_int, c_int, P, P],
    "rm_dense_fwd": [P, I64, c_int, P, I64, c_int, P, I64, c_int, c_int, P, c_int, c_int, P, I64, P, I64,
                     I64, P, I64, P, I64, P, P],
    "rm_dense_fwd6": [P, I64, c_int, P, I64, c_int, P, I64, c_int, c_int, P, c_int, c_int, P, I64, I64, P, I64,
                      P, P, P, P, P],
    "rm_dense_wgrad": [P, I64, c_int, P, I64, c_int, P, I64, c_int, I64, P, I64, c_int, P, P, I64, P],
    "rm_dense_wgrad6": [P, I64, c_int, P, I64, c_int, P, I64, c_int, P, I64, c_int, I64, P, I64, P, I64, c_int, P, P,
                        I64, P],
    "rm_roc_auc": [P, P, I64, P, P, P],
    "rm_log_loss": [P, P, I64, c_float, P, P, P],
    "rm_group_auc": [P, P, P, I64, c_int, P, P, P, P, P, P, P],
    "rm_mmoe_mix_supported": [c_int, c_int, c_int],
    "rm_mmoe_mix_tile": [c_int, c_int, c_int, c_int, c_int],
    "rm_mmoe_mix_fwd": [P, I64, P, I64, I64, c_int, c_int, c_int, P, I64, P, I64, P],
    "rm_mmoe_mix_bwd": [P, I64, P, I64, P, I64, I64, c_int, c_int, c_int, P, I64, P, I64, P],
    "rm_multitask_loss": [P, P, P, P, c_float, I64, c_int, P, P, P, P, P, P, P],
    "rm_inbatch_softmax_supported": [c_int],
    "rm_inbatch_softmax_tile": [c_int, c_int],
    "rm_inbatch_softmax_fwd": [P, I64, P, I64, P, P, P, c_float, I64, c_int, c_int, P, P, P, P, P, P],
    "rm_inbatch_softmax_bwd": [P, I64, P, I64, P, P, P, c_float, c_float, I64, c_int, c_int, P, P, I64, P, I64, P, P],
    "rm_rownorm_fwd": [P, I64, I64, c_int, c_float, P, I64, P, P],
    "rm_rownorm_bwd": [P, I64, P, P, I64, I64, c_int, P, I64, P],
}


# int64-returning size queries
SIGNATURES_I64 = {
    "rm_cin_filter_workspace": [c_int, c_int, c_int],
    "rm_cin_filter_workspace6": [c_int, c_int, c_int, c_int],
    "rm_cin_bwd_workspace": [I64, c_int, c_int, c_int, c_int],
    "rm_afm_bwd_workspace": [I64, c_int, c_int, c_int],
    "rm_autoint_stats_floats": [I64, c_int, c_int],
    "rm_autoint_layer_bwd_workspace": [I64, c_int, c_int, c_int, c_int],
    "rm_autoint_head_bwd_workspace": [I64, c_int],
    "rm_cross_mix_bwd_workspace": [I64, c_int, c_int],
    "rm_fibinet_bwd_workspace": [I64, c_int, c_int, c_int, c_int],
    "rm_fmfm_bwd_workspace": [I64, c_int, c_int, c_int],
    "rm_pnn_bwd_workspace": [I64, c_int, c_int, c_int, c_int],
    "rm_masknet_group_bwd_workspace": [I64, c_int, c_int],
    "rm_masknet_row_bwd_workspace": [I64, c_int],
    "rm_asp_workspace": [c_int, c_int, P, I64, c_int],
    "rm_bst_workspace": [c_int, c_int, c_int, c_int, I64, c_int],
    "rm_dien_workspace": [c_int, c_int, I64, I64, c_int],
    "rm_mlp_bwd_workspace": [c_int, c_int],
    "rm_deepfm_step_workspace": [c_int, c_int],
    "rm_outer_actgrad_sums_workspace": [I64, c_int],
    "rm_shard_route_workspace": [c_int],
    "rm_dense_filter_workspace": [c_int, c_int],
    "rm_dense6_workspace": [c_int, c_int, I64],
    "rm_dense_wgrad6_workspace": [c_int, c_int, I64],
    "rm_dense_wgrad_workspace": [c_int, c_int, I64],
    "rm_sparse_optimizer_workspace": [I64],
    "rm_metric_workspace": [I64],
    "rm_group_auc_workspace": [I64],
    "rm_multitask_loss_workspace": [I64, c_int],
    "rm_inbatch_softmax_workspace": [I64, c_int],
}


# name -> (restype, argtypes): the entry points of include/recman_hip_topk.h, in its order
SIGNATURES_TOPK = {
    "rm_topk_ip_supported": (c_int, [c_int, c_int]),
    "rm_topk_ip_tile": (c_int, [c_int, c_int]),
    "rm_topk_ip_workspace": (c_int64, [I64, I64, c_int, c_int]),
    "rm_topk_ip": (c_int, [P, I64, P, I64, I64, I64, c_int, c_float, c_int, P, P, c_int, P, P, I64, P, P]),
}


# name -> (restype, argtypes): the entry points of include/recman_hip_multitask.h, in its order
SIGNATURES_MULTITASK = {
    "rm_cgc_mix_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "rm_cgc_mix_tile": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "rm_cgc_mix_fwd": (c_int, [P, I64, P, I64, I64, c_int, c_int, c_int, c_int, c_int, P, I64, P, I64, P]),
    "rm_cgc_mix_bwd": (c_int, [P, I64, P, I64, P, I64, I64, c_int, c_int, c_int, c_int, c_int, P, I64, P, I64, P]),
    "rm_multitask_loss_es_workspace": (c_int64, [I64, c_int]),
    "rm_multitask_loss_es": (c_int, [P, P, P, P, c_float, I64, c_int, c_int, c_int, P, P, P, P, P, P, P]),
}


# name -> (restype, argtypes): the entry points of include/recman_hip_rank.h, in its order
SIGNATURES_RANK = {
    "rm_rank_loss_workspace": (c_int64, [I64]),
    "rm_rank_loss": (c_int, [P, P, P, I64, c_int, c_int, c_float, c_float, P, P, P, P, P, P, P]),
}


# name -> (restype, argtypes): the entry points of include/recman_hip_rankmetrics.h, in its order
SIGNATURES_RANKMETRICS = {
    "rm_group_gain_workspace": (c_int64, [I64]),
    "rm_group_gain": (c_int, [P, P, P, I64, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise RecmanHipError(
            f"{LIB_PATH} not found: build it with `python -m recman_amd.build` "
            "(hipcc --offload-arch=gfx950). recman_amd has no CPU fallback.")
    # torch first: it bundles its own libamdhip64; loading ours before it would bring
    # in a second HIP runtime (the system one) that does not share torch's context
    import torch  # noqa: F401

    lib = ctypes.CDLL(LIB_PATH)
    lib.rm_last_error.restype = c_char_p
    lib.rm_last_error.argtypes = []
    for name, argtypes in SIGNATURES_I64.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_int64
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: loud
        fn.argtypes = argtypes
        fn.restype = c_int
    for table in (SIGNATURES_TOPK, SIGNATURES_MULTITASK, SIGNATURES_RANK, SIGNATURES_RANKMETRICS):
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def call(name, *args):
    """Calls an int-returning entry point; raises RecmanHipError on a non-zero code."""
    l = lib()
    rc = getattr(l, name)(*args)
    if rc != 0:
        msg = l.rm_last_error().decode("utf-8", "replace")
        raise RecmanHipError(f"{name} failed ({rc}): {msg}")
    return rc
