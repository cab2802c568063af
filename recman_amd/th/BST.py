"""BST (Behavior Sequence Transformer, arXiv 1905.06874): the other standard successor of DIN.  The reference has no such
class; the constructor follows th.DIN.  The transformer pooling is fused, forward and backward, in csrc/bst.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel


class BST(DeepModel):
    """https://arxiv.org/abs/1905.06874 : final = linear + DNN([E | dense]); E holds the plain features' embeddings and,
    per SequenceFeat, ONE row: the history items and the candidate (last) plus a learned position row by distance from
    the candidate go through one post-norm transformer encoder block (att_head_num heads, a feed-forward layer of
    att_ffn_units, default 4 * embedding_size; no dropout inside the block), and the block's output rows are averaged.
    An example without history is the candidate's own output row.

    Limits (rm_bst_supported): embedding_size 8/16/32, att_head_num 1/2/4/8 with embedding_size / att_head_num >= 4,
    att_ffn_units a multiple of 4 in 4..128, SequenceFeat max_len 1..63.  eval_metric is plain callables, as in the
    other classes here.  `l2_reg` and the TF-only arguments are stored and used nowhere."""

    model = "bst"

    def __init__(self, feat_dict, embedding_size=8, att_head_num=2, att_ffn_units=None, deep_hidden_units=(32, 32),
                 deep_dropout=(0.6, 0.6, 0.6), deep_l2_reg=0.0, deep_activation="relu", epoch=10, batch_size=256,
                 learning_rate=0.001, optimizer="adam", random_seed=2019, loss_type="logloss",
                 eval_metric=(roc_auc_score, log_loss), l2_reg=0.1, what_means_greater=None,
                 use_interactive_session=True, log_dir="./logs", strict_reference=False, device="cuda"):
        hp = dict(embedding_size=embedding_size, att_head_num=att_head_num, att_ffn_units=att_ffn_units,
                  deep_hidden_units=tuple(deep_hidden_units), deep_dropout=tuple(deep_dropout),
                  deep_l2_reg=deep_l2_reg, deep_activation=deep_activation, learning_rate=learning_rate,
                  optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(l2_reg=l2_reg)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
