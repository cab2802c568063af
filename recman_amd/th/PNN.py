"""PNN: the Product-based Neural Network (arXiv 1611.00144) - IPNN, OPNN and both.  Nothing in the reference
implements it; the constructor follows the pattern of the reference's other classes (recman/tf/core/AFM.py:27-48), the
product layer is the kernel form of the widely used open-source PNN, fused forward and backward in csrc/pnn.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel

KERNEL_TYPES = ("mat", "vec", "num")


class PNN(DeepModel):
    """final = DNN([E | inner | outer | dense]) (+ linear with use_linear=True; off by default) over every pair i < j of
    the F embedding rows (multi-valued, value and sequence features included): inner[(i,j)] = <E_i, E_j> (use_inner,
    IPNN), outer[(i,j)] = E_i K_(ij) E_j^T (use_outer, OPNN) with one kernel per pair - kernel_type "mat" a D x D
    matrix, "vec" a vector (K_(ij) = diag(k_ij)), "num" a scalar (K_(ij) = k_ij I).  This is the kernel-form product
    layer of the widely used open-source PNN, not the paper's sum-pooled outer-product shortcut.  The kernels are
    glorot; interaction_l2_reg covers them, deep_l2_reg the DNN.  deep_dropout holds KEEP probabilities
    (layers.py:461), None = no dropout.  Limits: one GPU, 2..40 embedding features, embedding_size 8/16/32, at least
    one of use_inner / use_outer, a non-empty deep_hidden_units.  The TF-only arguments are stored and used nowhere."""

    model = "pnn"

    def __init__(self, feat_dict, embedding_size=8, use_inner=True, use_outer=False, kernel_type="mat",
                 deep_hidden_units=(128, 128), deep_dropout=None, deep_l2_reg=0.0, interaction_l2_reg=0.0,
                 deep_activation="relu", use_linear=False, embedding_l2_reg=0.00001, linear_l2_reg=0.00001, epoch=10,
                 batch_size=256, learning_rate=0.001, optimizer="adam", random_seed=2019, loss_type="logloss",
                 eval_metric=(roc_auc_score, log_loss), what_means_greater=None, use_interactive_session=True,
                 log_dir="./logs", strict_reference=False, device="cuda"):
        if not (use_inner or use_outer):
            raise ValueError("PNN: neither use_inner nor use_outer is set: the product layer would be empty")
        if kernel_type not in KERNEL_TYPES:
            raise ValueError(f"PNN: kernel_type {kernel_type!r} is not one of 'mat', 'vec', 'num'")
        hidden = tuple(deep_hidden_units or ())
        if not hidden:
            raise ValueError("PNN: deep_hidden_units must name at least one layer of the DNN")
        keep = self._keep_probabilities(deep_dropout, hidden)
        hp = dict(embedding_size=embedding_size, use_inner=use_inner, use_outer=use_outer, kernel_type=kernel_type,
                  deep_hidden_units=hidden, deep_dropout=keep, deep_l2_reg=deep_l2_reg,
                  interaction_l2_reg=interaction_l2_reg, deep_activation=deep_activation, use_linear=use_linear,
                  embedding_l2_reg=embedding_l2_reg, linear_l2_reg=linear_l2_reg, learning_rate=learning_rate,
                  optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(deep_dropout=deep_dropout, deep_hidden_units=deep_hidden_units)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
