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
        assert loss_type in ["logloss", "mse"], (
            "loss_type can be either 'logloss' for classification task or 'mse' for regression task")
        _, _, _, _, hidden = eng.masknet_limits(
            dict(block_order=block_order, num_blocks=num_blocks, block_hidden_units=block_hidden_units,
                 reduction_ratio=reduction_ratio, deep_hidden_units=deep_hidden_units),
            len(feat_dict.embedding_feats), embedding_size)
        keep = tuple(deep_dropout) if deep_dropout is not None else (1,) * (len(hidden) + 1)
        if len(keep) != len(hidden) + 1:
            raise ValueError(f"deep_dropout needs {len(hidden) + 1} keep probabilities (input + every hidden layer), "
                             f"got {deep_dropout!r}")
        hp = dict(embedding_size=embedding_size, block_order=block_order, num_blocks=int(num_blocks),
                  block_hidden_units=int(block_hidden_units), reduction_ratio=float(reduction_ratio),
                  deep_hidden_units=hidden, deep_dropout=keep, deep_l2_reg=deep_l2_reg,
                  deep_activation=deep_activation, use_linear=use_linear, embedding_l2_reg=embedding_l2_reg,
                  linear_l2_reg=linear_l2_reg, learning_rate=learning_rate, optimizer=optimizer)
        DeepModel.__init__(self, feat_dict, hp, metrics=eval_metric, epoch=epoch, batch_size=batch_size,
                           random_seed=random_seed,
                           task="classification" if loss_type == "logloss" else "regression",
                           strict_reference=strict_reference, device=device)
        # TF-only knobs are accepted and ignored
        self.what_means_greater, self.use_interactive_session, self.log_dir = (
            what_means_greater, use_interactive_session, log_dir)
        self.loss_type, self.eval_metric = loss_type, eval_metric
        for k, v in hp.items():  # sklearn get_params()/clone() need the ctor arguments back
            setattr(self, k, v)
        # (as given: clone() compares the attributes with the arguments)
        self.deep_dropout, self.deep_hidden_units = deep_dropout, deep_hidden_units
        self.num_blocks, self.block_hidden_units, self.reduction_ratio = num_blocks, block_hidden_units, reduction_ratio
