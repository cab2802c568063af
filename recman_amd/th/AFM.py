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
        hp = dict(embedding_size=embedding_size, embedding_l2_reg=embedding_l2_reg,
                  linear_l2_reg=linear_l2_reg, att_factor=att_factor, att_l2_reg=att_l2_reg,
                  att_dropout=att_dropout, learning_rate=learning_rate, optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(use_deep=use_deep, l2_reg=l2_reg)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
