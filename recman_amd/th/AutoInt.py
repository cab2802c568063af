"""AutoInt / AutoInt+ (arXiv 1810.11921).  Nothing in the reference implements the model; the constructor follows
the pattern of the reference's other classes (recman/tf/core/AFM.py:27-48), the interacting layers follow the paper,
forward and backward fused in csrc/autoint.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel


class AutoInt(DeepModel):
    """final = linear + autoint (+ DNN([E | dense]) with a non-empty deep_hidden_units: AutoInt+), where
    autoint = flatten(Y_L) . w + w0 and every interacting layer is multi-head self-attention over the F embedding rows,
    Y_m = relu(concat_h sum_k softmax_k(<Q^h_m, K^h_k> c) V^h_k + X_m Wr)  (att_res=False drops the residual,
    att_scaling=True sets c = 1/sqrt(att_embedding_size); the paper's c is 1).
    deep_dropout holds KEEP probabilities (layers.py:461), None = no dropout.  There is no dropout inside the
    attention and the dense features enter the linear term and the DNN only.  The TF-only arguments are stored and used
    nowhere."""

    model = "autoint"

    def __init__(self, feat_dict, embedding_size=8, att_layer_num=3, att_embedding_size=8, att_head_num=2,
                 att_res=True, att_scaling=False, att_l2_reg=0.0, deep_hidden_units=(), deep_dropout=None,
                 deep_l2_reg=0.0, deep_activation="relu", embedding_l2_reg=0.00001, linear_l2_reg=0.00001, epoch=10,
                 batch_size=256, learning_rate=0.001, optimizer="adam", random_seed=2019, loss_type="logloss",
                 eval_metric=(roc_auc_score, log_loss), what_means_greater=None, use_interactive_session=True,
                 log_dir="./logs", strict_reference=False, device="cuda"):
        hidden = tuple(deep_hidden_units or ())
        keep = self._keep_probabilities(deep_dropout, hidden)
        hp = dict(embedding_size=embedding_size, att_layer_num=att_layer_num, att_embedding_size=att_embedding_size,
                  att_head_num=att_head_num, att_res=att_res, att_scaling=att_scaling, att_l2_reg=att_l2_reg,
                  deep_hidden_units=hidden, deep_dropout=keep, deep_l2_reg=deep_l2_reg,
                  deep_activation=deep_activation, embedding_l2_reg=embedding_l2_reg, linear_l2_reg=linear_l2_reg,
                  learning_rate=learning_rate, optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(deep_dropout=deep_dropout)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
