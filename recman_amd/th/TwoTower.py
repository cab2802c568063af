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
    item_embeddings(X) return [N, H] from a frame that holds only that tower's columns; evaluate(X, y=None) returns
    [in-batch loss, recall@k for k in recall_at] (named in `metric_names`).

    Retrieval: index_items(X_items) keeps the item tower's embeddings of a catalogue on the GPU; retrieve(X_users, k)
    returns the exact top-k catalogue rows and scores <u, v> / temperature of every user row (csrc/topk.hip);
    evaluate_catalogue(X, y=None) returns recall@k against the whole catalogue (named in `catalogue_metric_names`),
    which, unlike evaluate(), depends on neither batch_size nor row order.

    Out of scope: row sharding and multi-rank training, cross-device negatives, a learnable temperature, sampled or
    hard negatives beyond the batch, approximate top-k indexes (IVF, HNSW), quantised catalogues, a bf16x6
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
        self.catalogue_metric_names = [f"catalogue_recall@{k}" for k in self._recall_ks]
        self._index = None  # index_items(): the catalogue's embeddings [N, H] on the GPU and its item ids
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
    def _embeddings(self, X, side, on_device=False):
        """[N, H] float32 of one tower: host numpy, or with on_device a device tensor."""
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
        out = torch.empty((n, e.H), dtype=torch.float32, device=e.device) if on_device else \
            np.empty((n, e.H), dtype=np.float32)
        for s in range(0, n, self.batch_size):
            t = min(s + self.batch_size, n)
            emb = e.embeddings(side, idx[s:t].contiguous(), dense[s:t].contiguous(), mv=self._mv_batch(mv_host, s, t))
            if on_device:
                out[s:t].copy_(emb)
            else:
                out[s:t] = emb.cpu().numpy()
        return out

    def user_embeddings(self, X):
        """The user tower's embeddings [N, H] float32 (normalised rows with normalize=True).  X needs the user
        features only; only the user tower runs."""
        return self._embeddings(X, "user")

    def item_embeddings(self, X):
        """The item tower's embeddings [N, H] float32.  X needs the item features only; only the item tower runs."""
        return self._embeddings(X, "item")

    # --------------------------------------------------------------- retrieval
    def index_items(self, X_items):
        """Runs the item tower over the catalogue X_items (a frame with the item features; the item_id_feature
        column too when it is set) and keeps its embeddings [N, H] on the GPU, with the encoded item ids: the index
        retrieve() and evaluate_catalogue() search.  Catalogue row j is row j of X_items.  fit(), fit_on_batch() and
        restore() drop the index (its embeddings would be stale).  -> self."""
        idf = self.hparams.get("item_id_feature")
        ids = None
        if idf:
            if idf not in X_items:
                raise KeyError(f"TwoTower.index_items: the frame lacks the item_id_feature column {idf!r}")
            f = self.feat_dict[idf]
            ids = np.asarray(f(X_items[f.name])).reshape(-1).astype(np.int64)
        emb = self._embeddings(X_items, "item", on_device=True)
        self._index = dict(emb=emb, item_id=ids)
        return self

    def _need_index(self, what):
        if self._index is None:
            raise RuntimeError(f"TwoTower.{what}: no item index - call index_items(X_items) first (after fit() or "
                               "restore(), which drop it)")
        return self._index

    @staticmethod
    def _exclusions(exclude, s, t, dev):
        """Rows [s, t) of `exclude` (one iterable of catalogue rows per query row) as a device CSR."""
        lists = [np.asarray(list(r), dtype=np.int64).reshape(-1) for r in exclude[s:t]]
        offsets = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
        rows = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        return torch.from_numpy(offsets).to(dev), torch.from_numpy(rows.astype(np.int64)).to(dev)

    def _retrieve_rows(self, X_users, k, exclude, what):
        """Host (rows, scores) [n, k] of retrieve(); the argument errors raise before any GPU work."""
        index = self._need_index(what)
        k = int(k)
        if not 1 <= k <= 1024:
            raise ValueError(f"TwoTower.{what}: k={k} must be in 1..1024")
        if exclude is not None and len(exclude) != len(X_users):
            raise ValueError(f"TwoTower.{what}: exclude holds {len(exclude)} lists for {len(X_users)} rows")
        e = self._build()
        u = self._embeddings(X_users, "user", on_device=True)
        n = u.shape[0]
        rows, scores = np.empty((n, k), np.int64), np.empty((n, k), np.float32)
        for s in range(0, n, self.batch_size):
            t = min(s + self.batch_size, n)
            ex = None if exclude is None else self._exclusions(exclude, s, t, e.device)
            r, sc = e.topk(u[s:t], index["emb"], k, exclude=ex)
            rows[s:t], scores[s:t] = r.cpu().numpy(), sc.cpu().numpy()
        return rows, scores

    def retrieve(self, X_users, k, exclude=None):
        """The exact top-k of the indexed catalogue for every row of X_users (a frame with the user features):
        -> (rows int64 [n, k], scores float32 [n, k]), the catalogue rows sorted by score <u, v> / temperature (no
        logQ) descending, then by row; row -1 and score -inf past the available rows.  exclude: None or one iterable
        of catalogue rows per user row, rows that row must not get back.  Works in batches of batch_size; the
        result does not depend on it."""
        return self._retrieve_rows(X_users, k, exclude, "retrieve")

    def evaluate_catalogue(self, X, y=None, exclude=None):
        """[recall@k for k in recall_at] (`catalogue_metric_names`) against the whole indexed catalogue: row i of X
        (user features and the item_id_feature column) is a hit at k when one of its top-k catalogue rows carries the
        row's own item id; rows with y == 0 are not counted (0 when none is).  exclude as for retrieve().  Unlike
        evaluate(), the value depends on neither batch_size nor row order."""
        idf = self.hparams.get("item_id_feature")
        if not idf:
            raise ValueError("TwoTower.evaluate_catalogue: needs item_id_feature (a hit is a retrieved row with the "
                             "row's own item id)")
        index = self._need_index("evaluate_catalogue")
        if idf not in X:
            raise KeyError(f"TwoTower.evaluate_catalogue: the frame lacks the item_id_feature column {idf!r}")
        n = len(X)
        live = np.ones(n, dtype=bool) if y is None else self._weights(y, n) > 0
        f = self.feat_dict[idf]
        own = np.asarray(f(X[f.name])).reshape(-1).astype(np.int64)
        kmax = max(self._recall_ks)
        rows, _ = self._retrieve_rows(X, kmax, exclude, "evaluate_catalogue")
        ids = np.where(rows >= 0, index["item_id"][np.clip(rows, 0, None)], -1)
        hit = ids == own[:, None]
        W = int(live.sum())
        if W == 0:
            return [0.0] * len(self._recall_ks)
        return [float(hit[live, :k].any(axis=1).sum()) / W for k in self._recall_ks]

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

    def _fit_encoded(self, idx, dense, yt, mv=None):
        self._index = None  # the towers change: the catalogue's embeddings would be stale
        return DeepModel._fit_encoded(self, idx, dense, yt, mv)

    def restore(self, path="ckpt_model.pt"):
        self._index = None
        return DeepModel.restore(self, path)
