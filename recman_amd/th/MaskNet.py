"""MaskNet: feature-wise multiplication by instance-guided masks (arXiv 2102.07619).  Nothing in the reference
implements it; the constructor follows the pattern of the reference's other classes (recman/tf/core/AFM.py:27-48),
the model follows the paper, the normalise-and-mask passes are fused forward and backward in csrc/masknet.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .. import engine as eng
from .DeepModel import DeepModel


class MaskNet(DeepModel):
    """final = DNN logit (+ linear, use_linear=True, the default).  With x = [flatten(E) | dense] an instance-guided
    mask is relu(x Wa + ba) Wp + bp (aggregation width max(1, round(reduction_ratio * output width))); a MaskBlock is
    relu(LayerNorm((mask o input) Wh)) of width block_hidden_units, its input the per-field LayerNorm of the embedding
    rows (multi-valued, value and sequence features included) or the previous block's output.  block_order
    "parallel": num_blocks blocks on the embedding, the DNN reads [h_1 | .. | h_N | dense]; "serial": block 1 on the
    embedding, every later block on its predecessor, the DNN reads [h_N | dense].  deep_l2_reg covers every weight
    matrix, deep_dropout holds the DNN's KEEP probabilities (layers.py:461), None = no dropout.  Limits: one GPU, 1..40
    embedding features, embedding_size 8/16/32, block_hidden_units a multiple of 4 in 8..2048, num_blocks 1..8,
    reduction_ratio > 0, at least one DNN layer.  The TF-only arguments are stored and used nowhere."""

    model = "masknet"

    def __init__(self, feat_dict, embedding_size=8, block_order="parallel", num_blocks=3, block_hidden_units=64,
                 reduction_ratio=2.0, deep_hidden_units=(128, 128), deep_dropout=None, deep_l2_reg=0.0,
                 deep_activation="relu", use_linear=True, embedding_l2_reg=0.00001, linear_l2_reg=0.00001, epoch=10,
                 batch_size=256, learning_rate=0.001, optimizer="adam", random_seed=2019, loss_type="logloss",
                 eval_metric=(roc_auc_score, log_loss), what_means_greater=None, use_interactive_session=True,
                 log_dir="./logs", strict_reference=False, device="cuda"):
        _, _, _, _, hidden = eng.masknet_limits(
            dict(block_order=block_order, num_blocks=num_blocks, block_hidden_units=block_hidden_units,
                 reduction_ratio=reduction_ratio, deep_hidden_units=deep_hidden_units),
            len(feat_dict.embedding_feats), embedding_size)
        keep = self._keep_probabilities(deep_dropout, hidden)
        hp = dict(embedding_size=embedding_size, block_order=block_order, num_blocks=int(num_blocks),
                  block_hidden_units=int(block_hidden_units), reduction_ratio=float(reduction_ratio),
                  deep_hidden_units=hidden, deep_dropout=keep, deep_l2_reg=deep_l2_reg,
                  deep_activation=deep_activation, use_linear=use_linear, embedding_l2_reg=embedding_l2_reg,
                  linear_l2_reg=linear_l2_reg, learning_rate=learning_rate, optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(deep_dropout=deep_dropout, deep_hidden_units=deep_hidden_units, num_blocks=num_blocks,
                     block_hidden_units=block_hidden_units, reduction_ratio=reduction_ratio)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
