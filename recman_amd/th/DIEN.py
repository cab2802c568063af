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
        assert loss_type in ["logloss", "mse"], (
            "loss_type can be either 'logloss' for classification task or 'mse' for regression task")
        hp = dict(embedding_size=embedding_size, deep_hidden_units=tuple(deep_hidden_units),
                  deep_dropout=tuple(deep_dropout), deep_l2_reg=deep_l2_reg, deep_activation=deep_activation,
                  learning_rate=learning_rate, optimizer=optimizer)
        DeepModel.__init__(self, feat_dict, hp, metrics=eval_metric, epoch=epoch, batch_size=batch_size,
                           random_seed=random_seed,
                           task="classification" if loss_type == "logloss" else "regression",
                           strict_reference=strict_reference, device=device)
        # TF-only knobs and the unused argument are accepted and ignored
        self.what_means_greater, self.use_interactive_session, self.log_dir = (
            what_means_greater, use_interactive_session, log_dir)
        self.l2_reg = l2_reg
        self.loss_type, self.eval_metric = loss_type, eval_metric
        for k, v in hp.items():  # sklearn get_params()/clone() need the ctor arguments back
            setattr(self, k, v)
