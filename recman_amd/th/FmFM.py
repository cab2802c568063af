"""FmFM, FvFM and FwFM: field-pair weighted factorization machines (FwFM: arXiv 1806.03514; FmFM and FvFM:
arXiv 2102.12994).  Nothing in the reference implements them; the constructor follows the pattern of the reference's
other classes (recman/tf/core/AFM.py:27-48), the models follow the papers, the pair term is fused forward and backward
in csrc/fmfm.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel

FIELD_INTERACTIONS = ("matrix", "vector", "scalar")


class FmFM(DeepModel):
    """final = linear (use_linear=True, the default) + sum_{i<j} E_i W_(ij) E_j^T (+ DNN([E | dense]) with a non-empty
    deep_hidden_units: DeepFwFM and its kin) over every pair of the F embedding rows (multi-valued, value and sequence
    features included).  field_interaction "matrix" (FmFM) gives every pair a D x D matrix, "vector" (FvFM) a vector
    (W_(ij) = diag(w_ij)), "scalar" (FwFM) a scalar (W_(ij) = r_ij I); the pair weights start at plain FM (identity /
    ones).  interaction_l2_reg covers them, deep_l2_reg the DNN.  deep_dropout holds KEEP probabilities
    (layers.py:461), None = no dropout.  Limits: one GPU, 2..40 embedding features, embedding_size 8/16/32.
    The TF-only arguments are stored and used nowhere."""

    model = "fmfm"

    def __init__(self, feat_dict, embedding_size=8, field_interaction="matrix", deep_hidden_units=(),
                 deep_dropout=None, deep_l2_reg=0.0, interaction_l2_reg=0.0, deep_activation="relu", use_linear=True,
                 embedding_l2_reg=0.00001, linear_l2_reg=0.00001, epoch=10, batch_size=256, learning_rate=0.001,
                 optimizer="adam", random_seed=2019, loss_type="logloss", eval_metric=(roc_auc_score, log_loss),
                 what_means_greater=None, use_interactive_session=True, log_dir="./logs", strict_reference=False,
                 device="cuda"):
        if field_interaction not in FIELD_INTERACTIONS:
            raise ValueError(f"{type(self).__name__}: field_interaction {field_interaction!r} is not one of 'matrix', "
                             "'vector', 'scalar'")
        hidden = tuple(deep_hidden_units or ())
        keep = self._keep_probabilities(deep_dropout, hidden)
        hp = dict(embedding_size=embedding_size, field_interaction=field_interaction, deep_hidden_units=hidden,
                  deep_dropout=keep, deep_l2_reg=deep_l2_reg, interaction_l2_reg=interaction_l2_reg,
                  deep_activation=deep_activation, use_linear=use_linear, embedding_l2_reg=embedding_l2_reg,
                  linear_l2_reg=linear_l2_reg, learning_rate=learning_rate, optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(deep_dropout=deep_dropout, deep_hidden_units=deep_hidden_units)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)


class FwFM(FmFM):
    """FmFM with field_interaction="scalar" as its default: one scalar r_ij per field pair (arXiv 1806.03514); with a
    non-empty deep_hidden_units, DeepFwFM."""

    def __init__(self, feat_dict, embedding_size=8, field_interaction="scalar", deep_hidden_units=(),
                 deep_dropout=None, deep_l2_reg=0.0, interaction_l2_reg=0.0, deep_activation="relu", use_linear=True,
                 embedding_l2_reg=0.00001, linear_l2_reg=0.00001, epoch=10, batch_size=256, learning_rate=0.001,
                 optimizer="adam", random_seed=2019, loss_type="logloss", eval_metric=(roc_auc_score, log_loss),
                 what_means_greater=None, use_interactive_session=True, log_dir="./logs", strict_reference=False,
                 device="cuda"):
        FmFM.__init__(self, feat_dict, embedding_size=embedding_size, field_interaction=field_interaction,
                      deep_hidden_units=deep_hidden_units, deep_dropout=deep_dropout, deep_l2_reg=deep_l2_reg,
                      interaction_l2_reg=interaction_l2_reg, deep_activation=deep_activation, use_linear=use_linear,
                      embedding_l2_reg=embedding_l2_reg, linear_l2_reg=linear_l2_reg, epoch=epoch,
                      batch_size=batch_size, learning_rate=learning_rate, optimizer=optimizer, random_seed=random_seed,
                      loss_type=loss_type, eval_metric=eval_metric, what_means_greater=what_means_greater,
                      use_interactive_session=use_interactive_session, log_dir=log_dir,
                      strict_reference=strict_reference, device=device)
