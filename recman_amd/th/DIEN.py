"""DIEN (Deep Interest Evolution Network, arXiv 1809.03672): the recurrent successor of DIN.  The reference has no such
class; the constructor follows th.DIN / th.BST.  The interest-evolution pooling is fused, forward and backward, in
csrc/dien.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel


class DIEN(DeepModel):
    """https://arxiv.org/abs/1809.03672 : final = linear + DNN([E | dense]); E holds the plain features' embeddings and,
    per SequenceFeat, ONE row: a GRU reads the history (oldest first), the candidate attends over the GRU's states
    (softmax of h_t . att_w q), and a second GRU whose update gate is scaled by the attention weight (AUGRU) evolves
    the interest; the row is that GRU's last state.  An example without history gets a zero row.

    Not built: the auxiliary loss (it needs a negative-sample input), the AIGRU / AGRU variants, a hidden size other
    than embedding_size, dropout inside the unit.  Limits (rm_dien_supported): embedding_size 8/16/32, SequenceFeat
    max_len 1..256.  eval_metric is plain callables, as in the other classes here.  `l2_reg` and the TF-only arguments
    are stored and used nowhere."""

    model = "dien"

    def __init__(self, feat_dict, embedding_size=8, deep_hidden_units=(32, 32), deep_dropout=(0.6, 0.6, 0.6),
                 deep_l2_reg=0.0, deep_activation="relu", epoch=10, batch_size=256, learning_rate=0.001,
                 optimizer="adam", random_seed=2019, loss_type="logloss", eval_metric=(roc_auc_score, log_loss),
                 l2_reg=0.1, what_means_greater=None, use_interactive_session=True, log_dir="./logs",
                 strict_reference=False, device="cuda"):
        hp = dict(embedding_size=embedding_size, deep_hidden_units=tuple(deep_hidden_units),
                  deep_dropout=tuple(deep_dropout), deep_l2_reg=deep_l2_reg, deep_activation=deep_activation,
                  learning_rate=learning_rate, optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(l2_reg=l2_reg)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
