"""DeepFM with the reference's constructor (recman/tf/core/DeepFM.py:30-53) - the class
recman/th/DeepFM.py:12-13 leaves empty."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel


class DeepFM(DeepModel):
    """https://arxiv.org/abs/1703.04247 : final = linear + FM + DNN (DeepFM.py:107-158)."""

    model = "deepfm"

    def __init__(self, feat_dict, embedding_size=8, embedding_l2_reg=0.00001, linear_l2_reg=0.00001,
                 fm_dropout=(1.0, 1.0), deep_hidden_units=(32, 32), deep_dropout=(0.8, 0.8, 0.8),
                 deep_l2_reg=0.00001, deep_activation="relu", epoch=10, batch_size=64,
                 learning_rate=0.001, optimizer="adam", random_seed=2019, use_fm=True, use_deep=True,
                 loss_type="logloss", eval_metric=(roc_auc_score, log_loss), what_means_greater=None,
                 use_interactive_session=False, log_dir="./logs", strict_reference=False,
                 device="cuda"):
        assert use_fm or use_deep  # DeepFM.py:54
        hp = dict(embedding_size=embedding_size, embedding_l2_reg=embedding_l2_reg,
                  linear_l2_reg=linear_l2_reg, fm_dropout=tuple(fm_dropout),
                  deep_hidden_units=tuple(deep_hidden_units), deep_dropout=tuple(deep_dropout),
                  deep_l2_reg=deep_l2_reg, deep_activation=deep_activation, use_fm=use_fm,
                  use_deep=use_deep, learning_rate=learning_rate, optimizer=optimizer)
        self._init_front(feat_dict, hp, {}, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
