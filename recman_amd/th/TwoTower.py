"""TwoTower: the candidate-retrieval model (DSSM / YouTube-DNN; the sampling-bias-corrected in-batch softmax of Yi et
al., RecSys 2019) - a user tower and an item tower each produce an embedding, trained with a softmax over the other
items of the batch.  Nothing in the reference implements it (every model of it is a ranker that scores one (user, item)
row); the constructor follows the pattern of the reference's other classes (recman/tf/core/AFM.py:27-48), the in-batch
softmax loss and the row normalisation are fused HIP kernels (csrc/inbatch.hip)."""
import logging
from time import time

import numpy as np
import torch

from .. import engine as eng
from .DeepModel import DeepModel
from .inputs import CSR, DataInputs, DenseFeat, MultiValCsvFeat, SparseValueFeat

log = logging.getLogger(__name__)


def _spec_of(fd):
    return eng.FeatureSpec([f.name for f in fd.embedding_feats], [f.feat_size for f in fd.embedding_feats],
                           [f.name for f in fd.dense_feats], [f.name for f in fd.multi_val_csv_feats],
                           [f.name for f in fd.sparse_val_feats],
                           seq_query={f.name: f.id_feat.name for f in fd.sequence_feats},
                           seq_max_len={f.name: f.max_len for f in fd.sequence_feats})


class TwoTower(DeepModel):
    """u = user_tower(user features), v = item_tower(item features) - hidden layers with deep_activation and a final
    linear layer to H = the last unit of both towers, L2-normalised rows with normalize=True; score = <u, v> /
    temperature.  user_features and item_features partition the FeatureDictionary (embedding and dense features
    alike; multi-valued and value features included); each tower's embedding features, and its dense features, must be
    one contiguous run in dictionary order (engine.TwoTowerEngine has the arithmetic and the variable names).

    fit(X, y=None): every row is an observed (user, item) pair; the loss is the softmax of the row's own item against
    the items of the other rows of its batch.  y, when given, must be 0/1: a row with 0 contributes no loss term of
    its own, its item still serves as a negative.  mask_accidental_hits removes the other rows that carry the row's own
    item (item_id_feature) from its softmax; logq_correction subtracts log q(item) from the scores, with q estimated
    from the training frame by fit(): logq[id] = log((count[id] + 1) / (N + V)).
    predict(X) returns the [N] scores of the rows' own pairs (no logQ, no sigmoid); user_embeddings(X) /
    item_embeddings(X) return [N, H] from a frame that holds only that tower's columns - feed them to whatever
    nearest-neighbour index you use; evaluate(X, y=None) returns [in-batch loss, recall@k for k in recall_at] (named
    in `metric_names`).

    Out of scope: row sharding and multi-rank training, cross-device negatives, a learnable temperature, sampled or
    hard negatives beyond the batch, approximate or brute-force top-k search over an item catalogue, a bf16x6
    split-operand form of the score products, dropout inside the towers, sequence features (SequenceFeat raises: its
    query would cross the towers), strict_reference, feeder="pinned".  The TF-only arguments are stored and used
    nowhere."""

    model = "twotower"

    def __init__(self, feat_dict, user_features, item_features, item_id_feature=None, user_hidden_units=(256, 128),
                 item_hidden_units=(256, 128), embedding_size=8, temperature=0.05, normalize=True,
                 mask_accidental_hits=True, logq_correction=False, recall_at=(10,), deep_activation="relu",
                 deep_l2_reg=0.0, embedding_l2_reg=0.00001, epoch=10, batch_size=4096, learning_rate=0.001,
                 optimizer="adam", random_seed=2019, eval_metric=None, what_means_greater=None,
                 use_interactive_session=True, log_dir="./logs", strict_reference=False, device="cuda"):
        if strict_reference:
            raise ValueError("TwoTower: strict_reference reproduces quirks of the reference, which has no retrieval "
                             "model")
        hp = dict(user_features=user_features, item_features=item_features, item_id_feature=item_id_feature,
                  user_hidden_units=user_hidden_units, item_hidden_units=item_hidden_units,
                  embedding_size=embedding_size, temperature=temperature, normalize=normalize,
                  mask_accidental_hits=mask_accidental_hits, logq_correction=logq_correction,
                  deep_activation=deep_activation, deep_l2_reg=deep_l2_reg, embedding_l2_reg=embedding_l2_reg,
                  learning_rate=learning_rate, optimizer=optimizer)
        self.limits_ = eng.twotower_limits(hp, _spec_of(feat_dict))  # raises before any GPU work
        eng.act_name(deep_activation)
        self.recall_at = recall_at  # (kept as given: sklearn's clone() wants the constructor arguments back)
        self._recall_ks = tuple(int(k) for k in recall_at)
        if any(k < 1 for k in self._recall_ks):
            raise ValueError(f"TwoTower: recall_at={recall_at!r} must be positive integers")
        DeepModel.__init__(self, feat_dict, hp, metrics=[], epoch=epoch, batch_size=batch_size,
                           random_seed=random_seed, task="classification", strict_reference=False, device=device)
        self.metric_names = ["inbatch_loss"] + [f"recall@{k}" for k in self._recall_ks]
        # TF-only knobs are accepted and ignored
        self.eval_metric, self.what_means_greater, self.use_interactive_session, self.log_dir = (
            eval_metric, what_means_greater, use_interactive_session, log_dir)
        for k, v in hp.items():  # sklearn get_params()/clone() need the ctor arguments back
            setattr(self, k, v)

    # ------------------------------------------------------------------ inputs
    @staticmethod
    def _weights(y, n):
        """The labels as float32 row weights [N]: 0/1 only."""
        ya = np.asarray(y, dtype=np.float32).reshape(-1)
        if ya.shape[0] != n or not np.all((ya == 0) | (ya == 1)):
            raise ValueError("TwoTower: labels, when given, must be one 0 or 1 per row (1 = an observed pair that "
                             "contributes a loss term, 0 = its item serves as a negative only)")
        return np.ascontiguousarray(ya)

    def _encode(self, X, y=None, on_host=False):
        idx, dense, _ = DeepModel._encode(self, X, None, on_host)
        yt = None if y is None else torch.from_numpy(self._weights(y, idx.shape[0])).to(idx.device)
        return idx, dense, yt

    def _encode_side(self, X, side):
        """A frame with only one tower's columns -> (idx, dense, mv_host) of the whole dictionary: the other tower's
        ids are slot 0, its dense columns 0."""
        fd, n = self.feat_dict, len(X)
        own = set(self.hparams[f"{side}_features"])
        inp = DataInputs()
        cols, dense, mv = [], [], {}
        for f in fd.values():
            mine = f.name in own
            if isinstance(f, DenseFeat):
                dense.append(np.asarray(f(X[f.name]), dtype=np.float32).reshape(n, -1) if mine
                             else np.zeros((n, 1), np.float32))
                continue
            if isinstance(f, (MultiValCsvFeat, SparseValueFeat)):
                if mine:
                    mv[f.name] = f.encode(X[f.name])
                else:
                    mv[f.name] = CSR(np.arange(n + 1), np.zeros(n, np.int64),
                                     np.zeros(n, np.float32) if isinstance(f, SparseValueFeat) else None)
                cols.append(np.zeros((n, 1), np.int64))
                continue
            cols.append(np.asarray(f(X[f.name])).reshape(n, 1) if mine else np.zeros((n, 1), np.int64))
        inp.mv = mv
        inp.idx = np.concatenate(cols, axis=1).astype(np.int64)
        inp.dense = np.concatenate(dense, axis=1) if dense else np.zeros((n, 0), np.float32)
        inp.check_ranges(fd)
        dev = self._build().device
        return (torch.from_numpy(np.ascontiguousarray(inp.idx)).to(dev),
                torch.from_numpy(np.ascontiguousarray(inp.dense)).to(dev), mv)

    # ----------------------------------------------------------------- predict
    def _embeddings(self, X, side):
        e = self._build()
        own = set(self.hparams[f"{side}_features"])
        if all(f in X for f in self.feat_dict):
            idx, dense, _ = self._encode(X)
            mv_host = self._mv_host
        else:
            missing = [f for f in own if f not in X]
            if missing:
                raise KeyError(f"TwoTower.{side}_embeddings: the frame lacks the {side} features {missing}")
            idx, dense, mv_host = self._encode_side(X, side)
        n = idx.shape[0]
        out = np.empty((n, e.H), dtype=np.float32)
        for s in range(0, n, self.batch_size):
            t = min(s + self.batch_size, n)
            emb = e.embeddings(side, idx[s:t].contiguous(), dense[s:t].contiguous(), mv=self._mv_batch(mv_host, s, t))
            out[s:t] = emb.cpu().numpy()
        return out

    def user_embeddings(self, X):
        """The user tower's embeddings [N, H] float32 (normalised rows with normalize=True).  X needs the user
        features only; only the user tower runs."""
        return self._embeddings(X, "user")

    def item_embeddings(self, X):
        """The item tower's embeddings [N, H] float32.  X needs the item features only; only the item tower runs."""
        return self._embeddings(X, "item")

    def _evaluate_encoded(self, idx, dense, mv_host, w):
        """[in-batch loss, recall@k ..] over batches of batch_size in order; w: host float32 weights or None."""
        e = self._build()
        n = idx.shape[0]
        loss_sum = w_sum = 0.0
        hits = np.zeros(len(self._recall_ks), dtype=np.int64)
        for s in range(0, n, self.batch_size):
            t = min(s + self.batch_size, n)
            wb = None if w is None else w[s:t]
            if wb is not None and not isinstance(wb, torch.Tensor):
                wb = torch.from_numpy(np.ascontiguousarray(wb, dtype=np.float32))
            yb = None if wb is None else wb.to(e.device, torch.float32).contiguous()
            ib, db = idx[s:t].contiguous(), dense[s:t].contiguous()
            loss, _, rank = e.evaluate_batch(ib.to(e.device), db.to(e.device), yb, mv=self._mv_batch(mv_host, s, t))
            rk = rank.cpu().numpy()
            live = np.ones(t - s, dtype=bool) if yb is None else (yb.cpu().numpy() > 0)
            W = float(live.sum())  # (0/1 weights)
            loss_sum += float(loss.item()) * W
            w_sum += W
            hits += np.array([int((rk[live] < k).sum()) for k in self._recall_ks], dtype=np.int64)
        if w_sum == 0:
            return [0.0] + [0.0] * len(self._recall_ks)
        return [loss_sum / w_sum] + [float(h) / w_sum for h in hits]

    def evaluate(self, X, y=None, training=False, batch_number_to_show_progress=50):
        """[in-batch loss, recall@k for k in recall_at] (`metric_names`) over batches of batch_size in frame order, both
        from the forward kernel: the loss is the mean over the rows with w_i > 0 of logsumexp_j S_ij - S_ii, recall@k
        the mean of [rank_i < k], rank_i = the number of other rows of the batch whose item scores above the row's own.
        BOTH VALUES DEPEND ON THE BATCH COMPOSITION: the negatives are the other rows of the same batch, so another
        batch_size or row order gives other numbers; compare runs at the same batch_size and order only."""
        idx, dense, _ = self._encode(X)
        w = None if y is None else self._weights(y, idx.shape[0])
        return self._evaluate_encoded(idx, dense, self._mv_host, w)

    def _eval_at_epoch(self, enc_train, y_train, enc_valid=None, y_valid=None, start_time=None, epoch=0):
        tr = self._evaluate_encoded(enc_train[0], enc_train[1], enc_train[2], y_train)
        va = None
        if enc_valid is not None:
            va = self._evaluate_encoded(enc_valid[0], enc_valid[1], enc_valid[2], y_valid)
        log.info("[%d] train-result=%s%s [%.1f s]", epoch, [round(float(r), 4) for r in tr],
                 "" if va is None else ", valid-result=%s" % [round(float(r), 4) for r in va],
                 time() - (start_time or time()))
        return tr, va

    # --------------------------------------------------------------------- fit
    def _use_feeder(self, n):
        self._build()
        if self.hparams.get("feeder", "auto") == "pinned":
            raise NotImplementedError('TwoTower: feeder="pinned" is not available (the pinned-memory feeder carries '
                                      'integer labels); the encoded dataset stays on the GPU')
        return False

    def _set_logq(self, X):
        """logq[id] = log((count[id] + 1) / (N + V)) over the training frame's encoded item ids."""
        e = self._build()
        f = self.feat_dict[self.hparams["item_id_feature"]]
        ids = np.asarray(f(X[f.name])).reshape(-1).astype(np.int64)
        V = int(e.params["item_logq"].shape[0])
        count = np.bincount(ids, minlength=V).astype(np.float64)
        e.set_logq(np.log((count + 1.0) / (len(ids) + V)).astype(np.float32))

    def fit(self, X_train, y_train=None, X_valid=None, y_valid=None, **kw):
        n = len(X_train)
        y_train = np.ones(n, np.float32) if y_train is None else self._weights(y_train, n)
        if X_valid is not None:
            y_valid = np.ones(len(X_valid), np.float32) if y_valid is None else self._weights(y_valid, len(X_valid))
        if self.hparams["logq_correction"]:
            self._set_logq(X_train)
        return DeepModel.fit(self, X_train, y_train, X_valid, y_valid, **kw)

    def fit_on_batch(self, X, y=None):
        idx, dense, yt = self._encode(X, y)
        return self._fit_encoded(idx, dense, yt, self._mv_batch(self._mv_host, 0, idx.shape[0]))
