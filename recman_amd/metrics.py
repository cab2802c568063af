"""Evaluation metrics computed on the GPU: the counterpart of recman.metrics (recman/metrics/roc_auc.py:4-16,
logloss.py:4-19) and of the sklearn functions the models score with by default.

    from recman_amd.metrics import RocAucScore, LogLoss, GroupAuc, roc_auc_score, log_loss, group_auc
    from recman_amd.metrics import GroupNdcg, GroupRecall, GroupPrecision, group_ndcg, group_recall, group_precision

    model = DeepFM(feat_dict, hparams, metrics=(RocAucScore(), LogLoss()), epoch=3)
    model = DIN(feat_dict, eval_metric=(GroupAuc("user_id"), RocAucScore()))

| name                         | semantics                                                                   |
|------------------------------|-----------------------------------------------------------------------------|
| roc_auc_score(y_true, y_score) | sklearn 1.7.2's binary roc_auc_score with default arguments, exact:       |
|                              | the Mann-Whitney count in integers, ties one half (rm_roc_auc).  One class  |
|                              | present: UndefinedMetricWarning and nan, as sklearn.                        |
| log_loss(y_true, y_pred)     | sklearn 1.7.2's binary log_loss on float32 predictions: clip at FLT_EPSILON |
|                              | (rm_log_loss).  One class present: ValueError with sklearn's message.       |
| RocAucScore()                | callable, str / repr "roc_auc", higher_the_better = True                     |
| LogLoss(eps=1e-7)            | callable, str / repr "logloss", higher_the_better = False; clips at eps     |
|                              | (the reference class's intent; it passes eps= to sklearn, which 1.7.2 no   |
|                              | longer accepts)                                                             |
| group_auc(y_true, y_score,   | GAUC of the DIN paper (arXiv 1706.06978): the exact AUC inside each group,  |
|   groups, weight=...)        | averaged over the groups holding both classes, weighted by their examples   |
|                              | ("impressions", default) or positives ("clicks") (rm_group_auc).  Equal     |
|                              | scores in different groups never tie.  No group with both classes:          |
|                              | UndefinedMetricWarning and nan.  return_groups=True: (value, dict of the    |
|                              | device tensors ids, n, pos, two_u per group, ascending id)                  |
| GroupAuc(by, weight=...)     | callable metric(y_true, y_pred, groups=...), str / repr "gauc",              |
|                              | higher_the_better = True, group_by = by: DeepModel hands it the encoded id  |
|                              | column of the SparseFeat named `by` (unknown ids encode to 0: one group)    |
| group_ndcg / group_recall /  | NDCG@k (binary gains, discount 1 / log2(rank + 2)), recall@k and            |
|   group_precision(y_true,    | precision@k inside each group, averaged over the scored groups              |
|   y_score, groups, k=10,     | (rm_group_gain).  Ties: the expectation over the orders of equal scores,    |
|   scored=..., weight=...)    | sklearn's ndcg_score(ignore_ties=False); equal scores in different groups   |
|                              | never tie.  k: an int in 1..1024, or a tuple of up to 8 (a tuple back, one  |
|                              | sort).  groups=None: one list.  scored "both_classes" (default, GAUC's      |
|                              | rule) or "has_positive"; weight "groups" (default, the mean over queries),  |
|                              | "impressions" or "clicks".  No scored group: UndefinedMetricWarning and     |
|                              | nan.  return_groups=True: (value, dict of ids, n, pos, values per group)    |
| GroupNdcg / GroupRecall /    | callable metric(y_true, y_pred, groups=...), str / repr "ndcg@10",           |
|   GroupPrecision(by, k=10,   | "recall@10", "precision@10", higher_the_better = True, group_by = by as     |
|   scored=..., weight=...)    | GroupAuc; by=None: one list, called as metric(y_true, y_pred)               |

Inputs: torch tensors on the GPU are used in place; numpy arrays, lists and CPU tensors are copied to the GPU once.
Scores are compared and clipped as float32 (other float types are converted).  Labels are 0 / 1 as int64, int32,
bool or float; any other label value raises ValueError - a stated narrowing, sklearn accepts any two label values.
NaN or infinite scores and empty inputs raise ValueError, sklearn's keywords (sample_weight, max_fpr, labels, ...)
TypeError.  Every function returns a Python float: one device-to-host read per call.
Group ids are integers in [0, 2^32) of an integer dtype (label-encode anything else first): a float, bool or
string dtype and an id outside the range raise ValueError.

Each of the twelve carries `on_device = True`: DeepModel.fit() / evaluate() keep predictions and labels on the GPU
when every configured metric has it (recman_amd/th/DeepModel.py).
"""
import warnings

import numpy as np
import torch

from . import ops

__all__ = ["roc_auc_score", "log_loss", "group_auc", "group_ndcg", "group_recall", "group_precision", "RocAucScore",
           "LogLoss", "GroupAuc", "GroupNdcg", "GroupRecall", "GroupPrecision"]


def _no_extras(name, extra):
    if extra:
        raise TypeError(f"{name}: unsupported argument(s) {sorted(extra)} (binary and unweighted only)")


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _as_tensor(x):
    if isinstance(x, torch.Tensor):
        return x.detach()
    a = np.asarray(x)
    if a.dtype == object or a.dtype.kind in "USV":
        raise ValueError("recman_amd.metrics takes numeric inputs")
    return torch.from_numpy(np.ascontiguousarray(a))


def _inputs(y_true, y_score):
    dev = _device_of(y_score, y_true)
    s, y = _as_tensor(y_score), _as_tensor(y_true)
    if s.dim() != 1 or y.dim() != 1:
        raise ValueError(f"expected 1-D y_true and scores, got shapes {tuple(y.shape)} and {tuple(s.shape)}")
    if s.shape[0] != y.shape[0]:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{y.shape[0]}, {s.shape[0]}]")
    n = s.shape[0]
    if n == 0:
        raise ValueError("Found empty input: 0 samples")
    if n >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 samples, got {n}")
    if s.dtype == torch.bool or s.is_complex():
        raise ValueError(f"scores must be real numbers, got {s.dtype}")
    s = s.to(device=dev, dtype=torch.float32).contiguous()
    y = y.to(device=dev)
    if y.is_floating_point():
        # 0.0 / 1.0 -> 0 / 1; anything else (0.5, NaN, ...) -> 2, which the kernel flags
        y = (y == 1).to(torch.int64) + 2 * ((y != 0) & (y != 1)).to(torch.int64)
    elif y.dtype != torch.int64:
        if y.is_complex():
            raise ValueError(f"labels must be real numbers, got {y.dtype}")
        y = y.to(torch.int64)
    return s, y.contiguous()


def _check(rec, what):
    v, P, N, flags = ops.read_metric(rec)
    if flags & ops.METRIC_BAD_SCORE:
        raise ValueError(f"Input {what} contains NaN or infinity.")
    if flags & ops.METRIC_BAD_LABEL:
        raise ValueError("y_true must hold binary labels 0 / 1 (recman_amd.metrics scores 0/1 labels only)")
    return v, P, N, flags


def roc_auc_score(y_true, y_score, **unsupported):
    """Exact binary ROC AUC on the GPU (sklearn.metrics.roc_auc_score with default arguments)."""
    _no_extras("roc_auc_score", unsupported)
    s, y = _inputs(y_true, y_score)
    with torch.cuda.device(s.device):
        v, _, _, flags = _check(ops.roc_auc(s, y), "y_score")
    if flags & ops.METRIC_ONE_CLASS:
        from sklearn.exceptions import UndefinedMetricWarning

        warnings.warn("Only one class is present in y_true. ROC AUC score is not defined in that case.",
                      UndefinedMetricWarning, stacklevel=2)
        return float("nan")
    return v


def _log_loss(y_true, y_pred, eps):
    p, y = _inputs(y_true, y_pred)
    with torch.cuda.device(p.device):
        v, P, _, flags = _check(ops.log_loss(p, y, eps=float(np.float32(eps))), "y_pred")
    if flags & ops.METRIC_PROB_RANGE:
        raise ValueError("y_prob contains values outside [0, 1]")
    if flags & ops.METRIC_ONE_CLASS:
        raise ValueError("y_true contains only one label ({0}). Please provide the list of all expected class "
                         "labels explicitly through the labels argument.".format(1 if P else 0))
    return v


def log_loss(y_true, y_pred, **unsupported):
    """Binary log loss on the GPU (sklearn.metrics.log_loss on float32 predictions: clip at FLT_EPSILON)."""
    _no_extras("log_loss", unsupported)
    return _log_loss(y_true, y_pred, ops.FLT_EPSILON)


_WEIGHT_KINDS = {"impressions": 0, "clicks": 1}


def _group_ids(groups, n, dev):
    if isinstance(groups, torch.Tensor):
        g = groups.detach()
        if g.is_floating_point() or g.is_complex() or g.dtype == torch.bool:
            raise ValueError(f"groups must hold integer ids, got {g.dtype}")
    else:
        a = np.asarray(groups)
        if a.dtype.kind not in "iu":
            raise ValueError(f"groups must hold integer ids, got dtype {a.dtype} (label-encode them first)")
        if a.dtype == np.uint64:
            if a.size and int(a.max()) >= 2 ** 32:
                raise ValueError("group ids must lie in [0, 2^32)")
            a = a.astype(np.int64)
        elif a.dtype.kind == "u":
            a = a.astype(np.int64)  # (torch has no wide unsigned types)
        g = torch.from_numpy(np.ascontiguousarray(a))
    if g.dim() != 1:
        raise ValueError(f"expected 1-D groups, got shape {tuple(g.shape)}")
    if g.shape[0] != n:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{n}, {g.shape[0]}]")
    return g.to(device=dev, dtype=torch.int64).contiguous()


def group_auc(y_true, y_score, groups, weight="impressions", return_groups=False, **unsupported):
    """GAUC on the GPU: the exact AUC inside each group, averaged over the groups that hold both classes with
    the weights n_g ("impressions") or P_g ("clicks").  return_groups=True: (value, {"ids", "n", "pos",
    "two_u"}) - int64 device tensors, one entry per group in ascending id order (AUC_g = two_u / (2 pos (n -
    pos)); two_u holds uint64 bits)."""
    _no_extras("group_auc", unsupported)
    if weight not in _WEIGHT_KINDS:
        raise ValueError(f"weight must be one of {sorted(_WEIGHT_KINDS)}, got {weight!r}")
    s, y = _inputs(y_true, y_score)
    n = s.shape[0]
    g = _group_ids(groups, n, s.device)
    with torch.cuda.device(s.device):
        per = [torch.empty(n, dtype=torch.int64, device=s.device) for _ in range(4)] if return_groups else None
        rec = ops.group_auc(s, y, g, _WEIGHT_KINDS[weight], per_group=per)
        v, G, scored, _, _, flags = ops.read_group_auc(rec)
    if flags & ops.METRIC_BAD_SCORE:
        raise ValueError("Input y_score contains NaN or infinity.")
    if flags & ops.METRIC_BAD_LABEL:
        raise ValueError("y_true must hold binary labels 0 / 1 (recman_amd.metrics scores 0/1 labels only)")
    if flags & ops.METRIC_BAD_GROUP:
        raise ValueError("group ids must lie in [0, 2^32) (label-encode them first)")
    if flags & ops.METRIC_ONE_CLASS:
        from sklearn.exceptions import UndefinedMetricWarning

        warnings.warn("No group holds both classes. The grouped AUC is not defined in that case.",
                      UndefinedMetricWarning, stacklevel=2)
        v = float("nan")
    if return_groups:
        return v, dict(zip(("ids", "n", "pos", "two_u"), (t[:G] for t in per)))
    return v


_GAIN_KINDS = {"ndcg": ("log2", "ideal"), "recall": ("none", "positives"), "precision": ("none", "k")}


def _cutoffs(k):
    """(ascending tuple of the distinct cutoffs, whether k was a single int)."""
    single = isinstance(k, (int, np.integer)) and not isinstance(k, bool)
    ks = (k,) if single else tuple(k) if isinstance(k, (tuple, list)) else None
    if not ks or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in ks):
        raise ValueError(f"k must be an int or a tuple of ints, got {k!r}")
    ks = tuple(int(v) for v in ks)
    if len(ks) > ops.GAIN_MAX_CUTOFFS or len(set(ks)) != len(ks):
        raise ValueError(f"k: at most {ops.GAIN_MAX_CUTOFFS} distinct cutoffs, got {ks}")
    if any(not 1 <= v <= ops.GAIN_MAX_K for v in ks):
        raise ValueError(f"k must lie in [1, {ops.GAIN_MAX_K}], got {ks}")
    return ks, single


def _gain_options(scored, weight):
    if scored not in ops.GAIN_SCORED:
        raise ValueError(f"scored must be one of {sorted(ops.GAIN_SCORED)}, got {scored!r}")
    if weight not in ops.GAIN_WEIGHTS:
        raise ValueError(f"weight must be one of {sorted(ops.GAIN_WEIGHTS)}, got {weight!r}")


def _group_gain(name, y_true, y_score, groups, k, scored, weight, return_groups, unsupported):
    _no_extras(f"group_{name}", unsupported)
    ks, single = _cutoffs(k)
    _gain_options(scored, weight)
    disc_kind, norm = _GAIN_KINDS[name]
    s, y = _inputs(y_true, y_score)
    n = s.shape[0]
    g = None if groups is None else _group_ids(groups, n, s.device)
    order = sorted(ks)
    with torch.cuda.device(s.device):
        per = None
        if return_groups:
            per = [torch.empty(n, dtype=torch.int64, device=s.device) for _ in range(3)]
            per.append(torch.empty((n, len(ks)), dtype=torch.float64, device=s.device))
        rec = ops.group_gain(s, y, g, ops.gain_discounts(s.device, disc_kind, order[-1]), order,
                             ops.GAIN_NORMS[norm], ops.GAIN_SCORED[scored], ops.GAIN_WEIGHTS[weight], per_group=per)
        values, G, _, _, _, flags = ops.read_group_gain(rec, len(ks))
    if flags & ops.METRIC_BAD_SCORE:
        raise ValueError("Input y_score contains NaN or infinity.")
    if flags & ops.METRIC_BAD_LABEL:
        raise ValueError("y_true must hold binary labels 0 / 1 (recman_amd.metrics scores 0/1 labels only)")
    if flags & ops.METRIC_BAD_GROUP:
        raise ValueError("group ids must lie in [0, 2^32) (label-encode them first)")
    if flags & ops.METRIC_ONE_CLASS:
        from sklearn.exceptions import UndefinedMetricWarning

        what = "holds both classes" if scored == "both_classes" else "holds a positive"
        warnings.warn(f"No group {what}. {name}@k is not defined in that case.", UndefinedMetricWarning,
                      stacklevel=3)
        values = (float("nan"),) * len(ks)
    at = [order.index(v) for v in ks]  # the caller's order of cutoffs
    v = values[0] if single else tuple(values[i] for i in at)
    if return_groups:
        vals = per[3][:G]
        return v, {"ids": per[0][:G], "n": per[1][:G], "pos": per[2][:G],
                   "values": vals[:, 0] if single else vals[:, at]}
    return v


def group_ndcg(y_true, y_score, groups, k=10, scored="both_classes", weight="groups", return_groups=False,
               **unsupported):
    """NDCG@k with binary gains inside each group, on the GPU: DCG with the discount 1 / log2(rank + 2) over the
    ideal DCG, the expectation over the orders of tied scores (sklearn's ndcg_score(k=k) per group), averaged over
    the scored groups.  k: an int (returns a float) or a tuple of up to 8 distinct ints (returns a tuple, one sort).
    groups=None: one list.  return_groups=True: (value, {"ids", "n", "pos", "values"}) - device tensors, one entry
    per group in ascending id order, "values" float64 [groups] or [groups, len(k)]."""
    return _group_gain("ndcg", y_true, y_score, groups, k, scored, weight, return_groups, unsupported)


def group_recall(y_true, y_score, groups, k=10, scored="both_classes", weight="groups", return_groups=False,
                 **unsupported):
    """Recall@k inside each group, on the GPU: the share of the group's positives among its k highest scores (ties:
    the expectation over their orders), averaged over the scored groups.  Arguments as group_ndcg."""
    return _group_gain("recall", y_true, y_score, groups, k, scored, weight, return_groups, unsupported)


def group_precision(y_true, y_score, groups, k=10, scored="both_classes", weight="groups", return_groups=False,
                    **unsupported):
    """Precision@k inside each group, on the GPU: positives among the group's k highest scores over k (a group
    shorter than k still divides by k; ties: the expectation over their orders), averaged over the scored groups.
    Arguments as group_ndcg."""
    return _group_gain("precision", y_true, y_score, groups, k, scored, weight, return_groups, unsupported)


roc_auc_score.on_device = True
log_loss.on_device = True
group_auc.on_device = True
group_ndcg.on_device = True
group_recall.on_device = True
group_precision.on_device = True


class RocAucScore:
    """recman.metrics.RocAucScore on the GPU."""

    on_device = True
    higher_the_better = True

    def __call__(self, y_true, y_pred):
        return roc_auc_score(y_true, y_pred)

    def __str__(self):
        return "roc_auc"

    def __repr__(self):
        return "roc_auc"


class LogLoss:
    """recman.metrics.LogLoss on the GPU: clips at eps (rounded to float32)."""

    on_device = True
    higher_the_better = False

    def __init__(self, eps=1e-07):
        self.eps = eps

    def __call__(self, y_true, y_pred):
        return _log_loss(y_true, y_pred, self.eps)

    def __str__(self):
        return "logloss"

    def __repr__(self):
        return "logloss"


class GroupAuc:
    """GAUC (group_auc) grouped by the feature `by`: DeepModel.fit() / evaluate() call it with groups= the
    encoded id column of that SparseFeat.  Ids the encoder has not seen encode to 0 and form one group."""

    on_device = True
    higher_the_better = True

    def __init__(self, by, weight="impressions"):
        if weight not in _WEIGHT_KINDS:
            raise ValueError(f"weight must be one of {sorted(_WEIGHT_KINDS)}, got {weight!r}")
        self.by = self.group_by = by
        self.weight = weight

    def __call__(self, y_true, y_pred, groups=None):
        if groups is None:
            raise TypeError(f"GroupAuc needs groups=: the ids of {self.by!r}, one per example")
        return group_auc(y_true, y_pred, groups, weight=self.weight)

    def __str__(self):
        return "gauc"

    def __repr__(self):
        return "gauc"


class _GroupGain:
    """A grouped top-k metric grouped by the feature `by`: DeepModel.fit() / evaluate() call it with groups= the
    encoded id column of that SparseFeat.  by=None: all examples are one list and no groups= is taken."""

    on_device = True
    higher_the_better = True
    _name = None

    def __init__(self, by, k=10, scored="both_classes", weight="groups"):
        ks, single = _cutoffs(k)
        if not single:
            raise ValueError(f"{type(self).__name__} reports one number: k must be an int, got {k!r}")
        _gain_options(scored, weight)
        self.by = self.group_by = by
        self.k = ks[0]
        self.scored = scored
        self.weight = weight

    def __call__(self, y_true, y_pred, groups=None):
        if groups is None and self.by is not None:
            raise TypeError(f"{type(self).__name__} needs groups=: the ids of {self.by!r}, one per example")
        return _group_gain(self._name, y_true, y_pred, groups, self.k, self.scored, self.weight, False, {})

    def __str__(self):
        return f"{self._name}@{self.k}"

    def __repr__(self):
        return f"{self._name}@{self.k}"


class GroupNdcg(_GroupGain):
    """NDCG@k (group_ndcg) per group of the feature `by`, averaged over the scored groups."""

    _name = "ndcg"


class GroupRecall(_GroupGain):
    """Recall@k (group_recall) per group of the feature `by`, averaged over the scored groups."""

    _name = "recall"


class GroupPrecision(_GroupGain):
    """Precision@k (group_precision) per group of the feature `by`, averaged over the scored groups."""

    _name = "precision"
