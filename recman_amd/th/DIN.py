"""DIN with the reference's constructor (recman/tf/core/DIN.py).  The reference's class cannot run: DIN.py:6 imports
ASPCombiner / ASPLayer, which exist nowhere, SequenceFeat.__init__ raises (inputs.py:443) and _init_graph stops after
the pooling layer.  The attention pooling here follows the paper the class cites (arXiv 1706.06978, the local
activation unit), forward and backward fused in csrc/asp.hip."""
from sklearn.metrics import log_loss, roc_auc_score

from .DeepModel import DeepModel


class DIN(DeepModel):
    """https://arxiv.org/abs/1706.06978 : final = linear + DNN([E | dense]); E holds the plain features' embeddings and,
    per SequenceFeat, ONE interest row: the history's rows summed with weights from the local activation unit
    a_l = MLP([q, k_l, q - k_l, q * k_l]) (q: the example's own row of the sequence's id_feat).

    Two defaults differ from the reference: att_activation is "sigmoid" (the reference's "dice" names a class,
    activation.py, that uses undefined names: asking for it raises NotImplementedError) and eval_metric is plain
    callables, as in the other classes here.  att_dropout holds KEEP probabilities and must be all ones.
    att_weight_normalization=True puts a softmax over the history's scores (off, as in the paper).
    `l2_reg` and the TF-only arguments are stored and used nowhere."""

    model = "din"

    def __init__(self, feat_dict, embedding_size=8, att_hidden_units=(80, 40), att_activation="sigmoid",
                 att_dropout=(1, 1, 1), att_weight_normalization=False, deep_hidden_units=(32, 32),
                 deep_dropout=(0.6, 0.6, 0.6), deep_l2_reg=0.0, deep_activation="relu", epoch=10, batch_size=256,
                 learning_rate=0.001, optimizer="adam", random_seed=2019, loss_type="logloss",
                 eval_metric=(roc_auc_score, log_loss), l2_reg=0.1, what_means_greater=None,
                 use_interactive_session=True, log_dir="./logs", strict_reference=False, device="cuda"):
        if isinstance(att_activation, str) and att_activation.lower() == "dice":
            raise NotImplementedError("att_activation='dice': the reference's Dice (activation.py) uses undefined names "
                                      "and has no arithmetic to follow; use 'sigmoid' or 'relu'")
        keep = att_dropout if isinstance(att_dropout, (list, tuple)) else (att_dropout,)
        if any(float(k) != 1.0 for k in keep):
            raise NotImplementedError(f"att_dropout={att_dropout!r}: the attention unit runs without dropout (every "
                                      "keep probability must be 1)")
        hp = dict(embedding_size=embedding_size, att_hidden_units=tuple(att_hidden_units),
                  att_activation=att_activation, att_dropout=att_dropout,
                  att_weight_normalization=att_weight_normalization, deep_hidden_units=tuple(deep_hidden_units),
                  deep_dropout=tuple(deep_dropout), deep_l2_reg=deep_l2_reg, deep_activation=deep_activation,
                  learning_rate=learning_rate, optimizer=optimizer)
        # (as given: clone() compares the attributes with the arguments)
        given = dict(l2_reg=l2_reg)
        self._init_front(feat_dict, hp, given, loss_type, eval_metric, epoch, batch_size, random_seed,
                         what_means_greater, use_interactive_session, log_dir, strict_reference, device)
