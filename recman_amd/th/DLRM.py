"""DLRM (arXiv 1906.00091, the MLPerf recommendation model).  Nothing in the reference implements the model; the
constructor follows the pattern of the reference's other classes (recman/tf/core/AFM.py:27-48), the model follows the
paper, the dot interaction is fused forward and backward in csrc/dot_interact.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel


class DLRM(DeepModel):
    """final = DNN_top([z | <v_i, v_j> for 0 <= j < i <= F]) (+ linear with use_linear=True), where
    z = the bottom tower over the dense features, widths bottom_hidden_units + (embedding_size,) with the activation
    after every layer, v_0 = z and v_1..v_F are the embedding rows (multi-valued, value and sequence features
    included).  deep_activation applies to both towers, deep_l2_reg to every weight matrix of both and to top_dnn_w.
    deep_dropout holds KEEP probabilities of the top tower (layers.py:461), None = no dropout; the bottom tower has no
    dropout.  Limits: one GPU, at least one dense feature, 1..40 embedding features, embedding_size 8/16/32/64.
    The TF-only arguments are stored and used nowhere."""

    model = "dlrm"

    def __init__(self, feat_dict, embedding_size=8, bottom_hidden_units=(64, 32), deep_hidden_units=(32, 32),
                 deep_dropout=None, deep_l2_reg=0.0, deep_activation="relu", use_linear=False,
                 embedding_l2_reg=0.00001, linear_l2_reg=0.00001, epoch=10, batch_size=256, learning_rate=0.001,
                 optimizer="adam", random_seed=2019, loss_type="logloss", eval_metric=(roc_auc_score, log_loss),
                 what_means_greater=None, use_interactive_session=True, log_dir="./logs", strict_reference=False,
                 device="cuda"):
        hidden = tuple(deep_hidden_units or ())
        bottom = tuple(bottom_hidden_units or ())
        keep = self._keep_probabilities(deep_dropout, hidden)
        hp = dict(embedding_size=embedding_size, bottom_hidden_units=bottom, deep_hidden_units=hidden,
                  deep_dropout=keep, deep_l2_reg=deep_l2_reg, deep_activation=deep_activation, use_linear=use_linear,
                  embedding_l2_reg=embedding_l2_reg, linear_l2_reg=linear_l2_reg, learning_rate=learning_rate,
                  optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(deep_dropout=deep_dropout, bottom_hidden_units=bottom_hidden_units,
                     deep_hidden_units=deep_hidden_units)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
