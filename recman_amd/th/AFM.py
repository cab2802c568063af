"""AFM with the reference's constructor (recman/tf/core/AFM.py:27-48).  The reference's AFMLayer does not
exist (AFM.py:7 comments the import out, AFM.py:119-122 uses it); the attention layer here follows the paper the
class cites (arXiv 1708.04617), forward and backward fused in csrc/afm.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel


class AFM(DeepModel):
    """https://arxiv.org/abs/1708.04617 : final = linear + attention-pooled pair interactions (AFM.py:111-126).
    att_dropout is a KEEP probability (as every dropout of the reference, layers.py:461), active in training only.
    `l2_reg` and `use_deep` are stored and used nowhere, as in the reference."""

    model = "afm"

    def __init__(self, feat_dict, embedding_size=8, embedding_l2_reg=0.00001, linear_l2_reg=0.00001,
                 att_factor=8, att_l2_reg=0.00001, att_dropout=1, epoch=10, batch_size=256,
                 learning_rate=0.001, optimizer="adam", random_seed=2019, use_deep=True,
                 loss_type="logloss", eval_metric=(roc_auc_score, log_loss), l2_reg=0.1,
                 what_means_greater=None, use_interactive_session=True, log_dir="./logs",
                 strict_reference=False, device="cuda"):
        assert loss_type in ["logloss", "mse"], (
            "loss_type can be either 'logloss' for classification task or 'mse' for regression task")
        hp = dict(embedding_size=embedding_size, embedding_l2_reg=embedding_l2_reg,
                  linear_l2_reg=linear_l2_reg, att_factor=att_factor, att_l2_reg=att_l2_reg,
                  att_dropout=att_dropout, learning_rate=learning_rate, optimizer=optimizer)
        DeepModel.__init__(self, feat_dict, hp, metrics=eval_metric, epoch=epoch, batch_size=batch_size,
                           random_seed=random_seed,
                           task="classification" if loss_type == "logloss" else "regression",
                           strict_reference=strict_reference, device=device)
        # TF-only knobs and the two unused arguments are accepted and ignored
        self.what_means_greater, self.use_interactive_session, self.log_dir = (
            what_means_greater, use_interactive_session, log_dir)
        self.use_deep, self.l2_reg = use_deep, l2_reg
        self.loss_type, self.eval_metric = loss_type, eval_metric
        for k, v in hp.items():  # sklearn get_params()/clone() need the ctor arguments back
            setattr(self, k, v)
