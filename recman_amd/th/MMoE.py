"""MMoE: the Multi-gate Mixture-of-Experts multi-task model (Ma et al., KDD 2018) - several labels per example over one
set of embedding tables.  Nothing in the reference implements it (its DeepModel knows one label); the constructor
follows the pattern of the reference's other classes (recman/tf/core/AFM.py:27-48), the gate softmax + expert mixture
and the loss head for several labels are fused HIP kernels (csrc/multitask.hip).  The same class is PLE / CGC
(Progressive Layered Extraction, Tang et al., RecSys 2020: task_experts, num_levels; th.PLE) and carries ESMM's
entire-space loss (Ma et al., SIGIR 2018: entire_space), on the same kernels."""
import numpy as np
import torch
from sklearn.metrics import log_loss, roc_auc_score

from .. import engine as eng
from .DeepModel import DeepModel


class TaskMetric:
    """One metric of one task: called with the labels [N, T] and predictions [N, T] of all tasks (numpy arrays, or
    device tensors when the metric runs on the GPU), it scores column `task_index` on the rows whose label is
    observed (not NaN).  str() is "<task>/<metric>"; on_device, higher_the_better and group_by are the metric's own."""

    def __init__(self, metric, task_name, task_index):
        self.metric, self.task_name, self.task_index = metric, task_name, int(task_index)
        self.name = f"{task_name}/{getattr(metric, '__name__', None) or str(metric)}"
        self.on_device = bool(getattr(metric, "on_device", False))
        self.group_by = getattr(metric, "group_by", None)
        if hasattr(metric, "higher_the_better"):
            self.higher_the_better = metric.higher_the_better

    def __call__(self, y_true, y_pred, groups=None):
        t = self.task_index
        if isinstance(y_pred, torch.Tensor):
            y = torch.as_tensor(y_true).to(y_pred.device)[:, t]
            seen = ~torch.isnan(y) if y.is_floating_point() else torch.ones_like(y, dtype=torch.bool)
            y, p = y[seen].contiguous(), y_pred[:, t][seen].contiguous()
            if groups is not None:
                groups = torch.as_tensor(groups).to(y_pred.device)[seen].contiguous()
        else:
            y = np.asarray(y_true)[:, t]
            seen = ~np.isnan(y.astype(np.float64))
            y, p = y[seen], np.asarray(y_pred)[:, t][seen]
            if groups is not None:
                groups = np.asarray(groups)[seen]
        return self.metric(y, p) if self.group_by is None else self.metric(y, p, groups=groups)

    def __str__(self):
        return self.name

    __repr__ = __str__


def entire_space_labels(y_c, y_v):
    """ESMM's label of the product pCTR pCVR from the click and conversion labels (numpy arrays or tensors): 0 where
    there was no click (whatever the conversion label is), the conversion label where there was one; unobserved where
    the click label is NaN or a click's conversion label is.  -> (z, observed)."""
    if isinstance(y_c, torch.Tensor):
        z = torch.where(y_c == 0, torch.zeros_like(y_v), y_v)
        return z, (y_c == 0) | ((y_c == 1) & ~torch.isnan(y_v))
    y_c, y_v = np.asarray(y_c, dtype=np.float64), np.asarray(y_v, dtype=np.float64)
    return np.where(y_c == 0, 0.0, y_v), (y_c == 0) | ((y_c == 1) & ~np.isnan(y_v))


class EntireSpaceMetric(TaskMetric):
    """One metric of the entire-space product: pred[:, c] * pred[:, v] against entire_space_labels on the rows where
    that label is observed.  str() is "ctcvr/<metric>"."""

    def __init__(self, metric, c, v):
        TaskMetric.__init__(self, metric, "ctcvr", v)
        self.c, self.v = int(c), int(v)

    def __call__(self, y_true, y_pred, groups=None):
        c, v = self.c, self.v
        if isinstance(y_pred, torch.Tensor):
            y = torch.as_tensor(y_true).to(y_pred.device).to(torch.float32)
            z, seen = entire_space_labels(y[:, c], y[:, v])
            z, p = z[seen].contiguous(), (y_pred[:, c] * y_pred[:, v])[seen].contiguous()
            if groups is not None:
                groups = torch.as_tensor(groups).to(y_pred.device)[seen].contiguous()
        else:
            y = np.asarray(y_true)
            z, seen = entire_space_labels(y[:, c], y[:, v])
            z, p = z[seen], (np.asarray(y_pred)[:, c] * np.asarray(y_pred)[:, v])[seen]
            if groups is not None:
                groups = np.asarray(groups)[seen]
        return self.metric(z, p) if self.group_by is None else self.metric(z, p, groups=groups)


class MMoE(DeepModel):
    """logit_t = tower_t(sum_e softmax(x G_t)_e expert_e(x)) for every task t over x = [E | dense] (multi-valued, value
    and sequence features included): num_experts expert DNNs of expert_hidden_units, one bias-free linear gate per
    task, one tower DNN of tower_hidden_units per task (engine.MMoEEngine has the arithmetic and the variable names).
    num_experts=1 is the shared-bottom model.

    fit(X, Y) takes Y [N, T], one column per task in task_names order; NaN marks an unobserved label (CVR is defined
    on clicks only): loss = sum_t task_weights[t] * mean over the observed labels of task t (log loss for a
    "classification" task, squared error for a "regression" task).  predict(X) returns [N, T] (probabilities /
    values); evaluate(X, Y) a flat task-major list - every metric of task 0, then of task 1, ... - each scored on that
    task's observed rows, named in `metric_names` ("ctr/roc_auc_score", ...); gate_weights(X) the gate weights
    [N, T, num_experts].  Limits: one GPU (no row sharding, no multi-rank job), 1..8 tasks, num_experts 1..16,
    expert_hidden_units multiples of 4 with the last in 4..512, a non-empty tower_hidden_units, no dropout inside the
    model, no strict_reference, no feeder="pinned".  The TF-only arguments are stored and used nowhere.

    PLE / CGC: with task_experts = S > 0 (or num_levels > 1) the model is Progressive Layered Extraction
    (engine.PLEEngine; `model` is then "ple"): every task has S experts of its own beside the num_experts SHARED ones,
    task gate t mixes its own and the shared experts, and num_levels extraction levels are stacked (every level but
    the last has one more gate, over all experts, that feeds the next level's shared experts).  num_levels=1 is CGC.
    Limits: task_experts 1..4, num_experts 1..8, tasks x task_experts + num_experts <= 32, num_levels 1..4;
    num_levels > 1 needs task_experts >= 1.  gate_weights(X, level=-1) then returns the task gates' weights of a
    level, [N, T, task_experts + num_experts] (own experts first).

    entire_space=("ctr", "cvr") names the click and the conversion task (two distinct classification tasks): the
    conversion task is then trained as in ESMM, through pCTCVR = pCTR pCVR against click x conversion over ALL
    impressions - label 0 where there was no click (the conversion label of such a row is not read and may be NaN),
    the conversion label on clicks - which removes the sample-selection bias of a CVR head trained on clicks only.
    predict(X)[:, cvr] stays pCVR; predict_ctcvr(X) returns the product [N]; evaluate() appends one metric group
    "ctcvr/<metric>" after the tasks' groups.

    As in every front end here, hparams, the engine choice (`model`), the entire-space pair and the metric list are
    fixed by the constructor: set_params() changes the attributes only.  Use clone() with new arguments, or a new
    instance."""

    model = "mmoe"

    def __init__(self, feat_dict, task_names=("ctr", "cvr"), task_types=("classification", "classification"),
                 task_weights=None, num_experts=8, expert_hidden_units=(256, 128), tower_hidden_units=(64,),
                 embedding_size=8, deep_activation="relu", deep_l2_reg=0.0, embedding_l2_reg=0.00001, epoch=10,
                 batch_size=256, learning_rate=0.001, optimizer="adam", random_seed=2019,
                 eval_metric=(roc_auc_score, log_loss), what_means_greater=None, use_interactive_session=True,
                 log_dir="./logs", strict_reference=False, device="cuda", task_experts=0, num_levels=1,
                 entire_space=None):
        if strict_reference:
            raise ValueError("MMoE: strict_reference reproduces quirks of the reference, which has no multi-task model")
        hp = dict(task_names=task_names, task_types=task_types, task_weights=task_weights, num_experts=num_experts,
                  expert_hidden_units=expert_hidden_units, tower_hidden_units=tower_hidden_units,
                  embedding_size=embedding_size, deep_activation=deep_activation, deep_l2_reg=deep_l2_reg,
                  embedding_l2_reg=embedding_l2_reg, learning_rate=learning_rate, optimizer=optimizer,
                  task_experts=task_experts, num_levels=num_levels, entire_space=entire_space)
        # a ValueError naming the limit, before any GPU work
        if task_experts == 0 and num_levels == 1:
            names, types = eng.mmoe_limits(hp)[:2]
        else:
            names, types = eng.ple_limits(hp)[:2]
            self.model = "ple"  # (this instance's engine: ENGINES["ple"])
        self.es_ = eng.entire_space_pair(hp, names, types)
        eng.act_name(deep_activation)
        self.task_names_, self.task_types_ = names, types
        metrics = [TaskMetric(m, n, t) for t, n in enumerate(names) for m in (eval_metric or ())]
        if self.es_ != (-1, -1):
            metrics += [EntireSpaceMetric(m, *self.es_) for m in (eval_metric or ())]
        DeepModel.__init__(self, feat_dict, hp, metrics=metrics, epoch=epoch, batch_size=batch_size,
                           random_seed=random_seed,
                           # (the base class holds ONE task type; every use of it is overridden here)
                           task="classification" if "classification" in types else "regression",
                           strict_reference=False, device=device)
        self.metric_names = [str(m) for m in metrics]
        # TF-only knobs are accepted and ignored
        self.what_means_greater, self.use_interactive_session, self.log_dir = (
            what_means_greater, use_interactive_session, log_dir)
        self.eval_metric = eval_metric
        for k, v in hp.items():  # sklearn get_params()/clone() need the ctor arguments back
            setattr(self, k, v)

    # ------------------------------------------------------------------ labels
    def _labels(self, y):
        """Y [N, T] as float32, NaN = unobserved; a classification label that is neither 0, 1 nor NaN is refused."""
        ya = np.asarray(y, dtype=np.float32)
        T = len(self.task_names_)
        if ya.ndim == 1 and T == 1:
            ya = ya.reshape(-1, 1)
        if ya.ndim != 2 or ya.shape[1] != T:
            raise ValueError(f"MMoE: labels must be [N, {T}] - one column per task {self.task_names_} - got "
                             f"{ya.shape}")
        for t, (name, kind) in enumerate(zip(self.task_names_, self.task_types_)):
            col = ya[:, t]
            if kind == "classification" and not np.all((col == 0) | (col == 1) | np.isnan(col)):
                raise ValueError(f"MMoE: task {name!r} is a classification task: its labels must be 0, 1 or NaN "
                                 "(unobserved)")
            if kind == "regression" and np.isinf(col).any():
                raise ValueError(f"MMoE: task {name!r}: infinite labels")
        return np.ascontiguousarray(ya)

    def _encode(self, X, y=None, on_host=False):
        idx, dense, _ = DeepModel._encode(self, X, None, on_host)
        yt = None
        if y is not None:
            yt = torch.from_numpy(self._labels(y)).to(idx.device)
        return idx, dense, yt

    def _labels_on_device(self, y):
        if isinstance(y, torch.Tensor):
            return y.to(self._build().device)
        return torch.from_numpy(self._labels(y)).to(self._build().device)

    # ----------------------------------------------------------------- predict
    def _predict_encoded(self, idx, dense, training, mv_host=None):
        out = np.empty((idx.shape[0], len(self.task_names_)), dtype=np.float32)
        for s, t, pred in self._predict_batches(idx, dense, training, mv_host):
            out[s:t] = pred.t().cpu().numpy()
        return out

    def _predict_device(self, idx, dense, training, mv_host=None):
        e = self._build()
        out = torch.empty((idx.shape[0], len(self.task_names_)), dtype=torch.float32, device=e.device)
        for s, t, pred in self._predict_batches(idx, dense, training, mv_host):
            out[s:t].copy_(pred.t())
        return out

    def predict_ctcvr(self, X, training=False):
        """pCTCVR = pCTR pCVR of every example, [N] float32 (entire_space models only)."""
        if self.es_ == (-1, -1):
            raise ValueError("MMoE: predict_ctcvr needs entire_space=(the click task, the conversion task)")
        pred = self.predict(X, training)
        return pred[:, self.es_[0]] * pred[:, self.es_[1]]

    def gate_weights(self, X, level=-1):
        """The gate weights softmax(x G_t) of every example: [N, T, num_experts] float32, rows summing to 1.  PLE: the
        task gates of extraction level `level`, [N, T, task_experts + num_experts] (a task's own experts first)."""
        e = self._build()
        if self.model != "ple" and level not in (-1, 0):
            raise ValueError(f"MMoE: level={level!r}: the model has one level of gates")
        idx, dense, _ = self._encode(X)
        mv_host = self._mv_host
        n = idx.shape[0]
        out = np.empty((n, e.T, e.W), dtype=np.float32)
        for s in range(0, n, self.batch_size):
            t = min(s + self.batch_size, n)
            p = e.gate_weights(idx[s:t].contiguous(), dense[s:t].contiguous(), mv=self._mv_batch(mv_host, s, t),
                               level=level)
            out[s:t] = p.cpu().numpy()
        return out

    def evaluate(self, X, y, training=False, batch_number_to_show_progress=50):
        return DeepModel.evaluate(self, X, self._labels(y), training, batch_number_to_show_progress)

    # --------------------------------------------------------------------- fit
    def _use_feeder(self, n):
        self._build()
        if self.hparams.get("feeder", "auto") == "pinned":
            raise NotImplementedError('MMoE: feeder="pinned" is not available (the pinned-memory feeder carries one '
                                      'label per example); the encoded dataset stays on the GPU')
        return False

    def fit(self, X_train, y_train, X_valid=None, y_valid=None, **kw):
        y_train = self._labels(y_train)
        if y_valid is not None:
            y_valid = self._labels(y_valid)
        return DeepModel.fit(self, X_train, y_train, X_valid, y_valid, **kw)


def PLE(feat_dict, **kw):
    """Progressive Layered Extraction (Tang et al., RecSys 2020): th.MMoE with PLE's defaults - two shared and two
    task-specific experts per level, two extraction levels; every argument of th.MMoE may be given."""
    return MMoE(feat_dict, **{**dict(num_experts=2, task_experts=2, num_levels=2), **kw})
