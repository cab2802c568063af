"""FiBiNET (arXiv 1905.09433).  Nothing in the reference implements the model; the constructor follows the pattern of
the reference's other classes (recman/tf/core/AFM.py:27-48), the model follows the paper, the SENET gate and the two
bilinear interactions are fused forward and backward in csrc/fibinet.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel


class FiBiNET(DeepModel):
    """final = DNN([bilinear(E) | bilinear(a o E) | dense]) (+ linear with use_linear=True, the default), where
    a = relu(relu(mean_d(E) senet_w1) senet_w2) re-weights the F embedding rows (multi-valued, value and sequence
    features included), senet_w1 is [F, max(1, F // reduction_ratio)], and bilinear(Y)[(i,j)] = (Y_i W_(i)) o Y_j over
    every field pair i < j: bilinear_type "all" shares one D x D matrix, "each" gives every left field its own.
    bilinear_type="interaction" (one matrix per pair) is not implemented and raises ValueError.  interaction_l2_reg
    covers the four interaction variables, deep_l2_reg the DNN.  deep_dropout holds KEEP probabilities (layers.py:461),
    None = no dropout.  Limits: one GPU, 2..40 embedding features, embedding_size 8/16/32.
    The TF-only arguments are stored and used nowhere."""

    model = "fibinet"

    def __init__(self, feat_dict, embedding_size=8, bilinear_type="each", reduction_ratio=3,
                 deep_hidden_units=(32, 32), deep_dropout=None, deep_l2_reg=0.0, interaction_l2_reg=0.0,
                 deep_activation="relu", use_linear=True, embedding_l2_reg=0.00001, linear_l2_reg=0.00001, epoch=10,
                 batch_size=256, learning_rate=0.001, optimizer="adam", random_seed=2019, loss_type="logloss",
                 eval_metric=(roc_auc_score, log_loss), what_means_greater=None, use_interactive_session=True,
                 log_dir="./logs", strict_reference=False, device="cuda"):
        if bilinear_type == "interaction":
            raise ValueError("FiBiNET: bilinear_type='interaction' (one matrix per field pair) is out of scope: "
                             "use 'all' or 'each'")
        if bilinear_type not in ("all", "each"):
            raise ValueError(f"FiBiNET: bilinear_type {bilinear_type!r} is not supported: 'all' or 'each'")
        hidden = tuple(deep_hidden_units or ())
        keep = self._keep_probabilities(deep_dropout, hidden)
        hp = dict(embedding_size=embedding_size, bilinear_type=bilinear_type, reduction_ratio=reduction_ratio,
                  deep_hidden_units=hidden, deep_dropout=keep, deep_l2_reg=deep_l2_reg,
                  interaction_l2_reg=interaction_l2_reg, deep_activation=deep_activation, use_linear=use_linear,
                  embedding_l2_reg=embedding_l2_reg, linear_l2_reg=linear_l2_reg, learning_rate=learning_rate,
                  optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(deep_dropout=deep_dropout, deep_hidden_units=deep_hidden_units)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
