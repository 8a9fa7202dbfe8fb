"""tf.estimator / tf.train look-alikes: the call surface the reference's model scripts drive
(algorithm/DeepFM/deepfm.py:231-343 and the same skeleton in every model).

  model_fn(features, labels, mode, params) -> EstimatorSpec     (unchanged contract)
  Estimator(model_fn, params, config).train / evaluate / predict, train_and_evaluate

Execution model (MI355X-first, not TF's): model_fn is run eagerly once per step on the
Estimator's VariableStore; its kernels are enqueued on one HIP stream.  For fixed-shape batches
the whole step (forward, backward, TF1-Adam) is captured once into a hipGraph and replayed
(`GraphedTrainStep`), so a step costs one graph launch instead of ~40 kernel launches.
"""
from __future__ import annotations

import os
import time
from typing import Callable, Dict, Iterable, Optional

import torch

from . import _lib, ops
from .variables import VariableStore, use_store


class ModeKeys:
    TRAIN = "train"
    EVAL = "eval"
    PREDICT = "infer"


class EstimatorSpec:
    def __init__(self, mode, predictions=None, loss=None, train_op=None, eval_metric_ops=None,
                 export_outputs=None, training_hooks=None, **_ignored):
        self.mode, self.predictions, self.loss, self.train_op = mode, predictions, loss, train_op
        self.eval_metric_ops = eval_metric_ops
        self.export_outputs, self.training_hooks = export_outputs, training_hooks


# --------------------------------------------------------------------------------------------
# the capacity of a padded Ragged (RunConfig(ragged_capacity=), ServingModel.compile(ragged_capacity=))
# --------------------------------------------------------------------------------------------
RAGGED_AUTO_MARGIN = (5, 4)      # "auto": 1.25 x the largest nnz seen ...
RAGGED_AUTO_ROUND = 1024         # ... rounded up to a multiple of this many values


def check_ragged_capacity(policy):
    """None | int >= 1 | {key: int >= 1} | "auto", or ValueError"""
    ok = policy is None or policy == "auto" or (isinstance(policy, int) and not isinstance(policy, bool) and policy >= 1) or \
        (isinstance(policy, dict) and all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in policy.values()))
    if not ok:
        raise ValueError(f"ragged_capacity = {policy!r}: expected None, an int >= 1 (values per example), a dict key -> int >= 1, "
                         "or 'auto'")
    return dict(policy) if isinstance(policy, dict) else policy


def ragged_auto_capacity(max_nnz: int) -> int:
    """ceil(1.25 * max_nnz / 1024) * 1024, in integers"""
    num, den = RAGGED_AUTO_MARGIN
    return (num * int(max_nnz) + den * RAGGED_AUTO_ROUND - 1) // (den * RAGGED_AUTO_ROUND) * RAGGED_AUTO_ROUND


def ragged_capacity_for(policy, key: str, rows: int, max_nnz: Optional[int] = None) -> Optional[int]:
    """The length of the padded `values` of `key` in a batch of `rows` examples, or None when the policy gives none (None; a
    dict without the key; "auto" before any batch was seen: max_nnz None)."""
    if isinstance(policy, dict):
        policy = policy.get(key)
    if policy is None:
        return None
    if policy == "auto":
        return None if max_nnz is None else ragged_auto_capacity(max_nnz)
    return int(policy) * int(rows)


def ragged_overflows(nnz: int, capacity: Optional[int]) -> bool:
    """A batch with more values than the capacity is never truncated: it takes the eager route."""
    return capacity is None or int(nnz) > int(capacity)


def dense_as_ragged(ids: torch.Tensor):
    """A [B] / [B, 1] id vector as the Ragged it stands for: B bags of one value each (an id of -1: a bag without a valid value,
    which looks up the same zero row)."""
    from .feature_column import Ragged
    ids = ids.reshape(-1)
    return Ragged(ids.contiguous(), torch.arange(ids.numel() + 1, dtype=torch.int64, device=ids.device))


GROUP_AUC_CAPACITY = 1 << 22    # rows of an evaluation's per-group AUC log, unless RunConfig(group_auc_capacity=) says otherwise


def check_group_auc_capacity(rows):
    """An int in 1 .. ops.GAUC_MAX_ROWS, or ValueError"""
    if not (isinstance(rows, int) and not isinstance(rows, bool) and 1 <= rows <= ops.GAUC_MAX_ROWS):
        raise ValueError(f"group_auc_capacity = {rows!r}: expected an int in 1 .. {ops.GAUC_MAX_ROWS} (rows of one evaluation)")
    return rows


class RunConfig:
    def __init__(self, model_dir=None, save_checkpoints_steps=None, device=None, seed=42,
                 use_hip_graph=True, device_metrics=True, ragged_capacity=None, group_auc_capacity=GROUP_AUC_CAPACITY,
                 **_ignored):
        self.model_dir, self.save_checkpoints_steps = model_dir, save_checkpoints_steps
        self.device, self.seed, self.use_hip_graph = device, seed, use_hip_graph
        # bags and histories (feature_column.Ragged) in buffers of fixed capacity, so that a step over them is captured:
        # None (the default): a ragged batch runs eagerly; an int: values per example, for every ragged key; a dict: key ->
        # values per example; "auto": per key, 1.25 x the largest nnz of the eager warm-up batches, rounded up to 1024 values.
        # A batch that does not fit is never truncated: it runs eagerly (Estimator.ragged_overflows)
        self.ragged_capacity = check_ragged_capacity(ragged_capacity)
        # evaluate(): the metrics and the loss sum are accumulated on the device, one launch per batch and one copy at the end
        # (EvalAccumulator); False: the host loop over Metric.update(), which also serves whatever the kernel does not
        self.device_metrics = device_metrics
        # the rows that the device log of a per-group AUC (GroupAUCMetric under device_metrics) holds for one evaluate() call: the
        # buffers are allocated once, before the first batch, so that the step stays captured; an evaluation with more rows than
        # this raises at its end and never reports a metric over part of the data
        self.group_auc_capacity = check_group_auc_capacity(group_auc_capacity)


class TrainSpec:
    def __init__(self, input_fn, max_steps=None, hooks=None):
        self.input_fn, self.max_steps, self.hooks = input_fn, max_steps, hooks


class EvalSpec:
    def __init__(self, input_fn, steps=None, throttle_secs=600, exporters=None, **_ignored):
        self.input_fn, self.steps, self.throttle_secs, self.exporters = input_fn, steps, throttle_secs, exporters


# --------------------------------------------------------------------------------------------
# tf.train.AdamOptimizer (a15)
# --------------------------------------------------------------------------------------------
class TrainOp:
    """optimizer.minimize(loss, var_list=...).  var_list None: every trainable variable (what every model but Wide&Deep asks
    for); else the variables `get_collection(GraphKeys.TRAINABLE_VARIABLES, scope=...)` returned."""

    def __init__(self, optimizer: "AdamOptimizer", loss: torch.Tensor, store: VariableStore, var_list=None):
        self.optimizer, self.loss, self.store = optimizer, loss, store
        self.var_list = None if var_list is None else list(var_list)

    def run(self):
        self.loss.backward()
        self.optimizer.apply_gradients(self.store)


class AdamOptimizer:
    """tf.train.AdamOptimizer(learning_rate, beta1, beta2, epsilon).minimize(loss):
    dense TF1 semantics for every variable, embedding tables included."""

    lazy_embeddings = False

    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.beta1, self.beta2, self.eps = float(learning_rate), beta1, beta2, epsilon

    def minimize(self, loss, global_step=None, var_list=None) -> TrainOp:
        """global_step is accepted and ignored: the Estimator counts its steps itself, once per step.  An Adam op over a
        var_list that leaves trainable variables out is only valid inside group() with the op that claims the rest (the
        fused launch sweeps the whole flat buffer: it is the identity exactly where g = m = v = 0)."""
        from .variables import current_store
        return TrainOp(self, loss, current_store(), var_list)

    def apply_gradients(self, store: VariableStore, grad_hook: Optional[Callable] = None,
                        before_update: Optional[Callable] = None):
        """before_update (group()): called once the step's gradients are complete (parked sums, all-reduce) and before the
        first Adam launch — another optimizer consumes and zeroes the gradients of ITS variables there."""
        st = store.ensure_opt_state()
        from . import nn, sparse
        arenas = [ar for ar in store.arenas.values() if ar.weight is not None and ar.trainable]
        # arenas on the owner-computes path (sparse.py): their optimizer step is fused with the row-gradient scatter
        # (recalgo_scatter_apply) — TF1 Adam with dense semantics evaluated lazily but exactly, or LazyAdam
        owned = [ar for ar in arenas if sparse.has_work(ar)]
        owned.sort(key=sparse.has_companions)     # (an arena whose lookups ride on another arena's plan comes after it)
        arenas = [ar for ar in arenas if not sparse.has_work(ar)]
        fused = all(ar.tracks_live_rows for ar in arenas) and len(arenas) <= 4 and store.device.type == "cuda"
        # The deferred sums INSIDE the optimizer launch (ops.adam_tf1_sum_step_) where nothing has to happen between the two:
        # no all-reduce of the summed gradients (grad_hook), no other optimizer consuming them (before_update), no parked
        # l2 term to add to them.  The launch advances the counter itself (arrival ticket: a device int beside the counter,
        # never created inside a graph capture — the capture's warm-up steps ran eagerly).
        if fused and ops.sum_step_enabled and grad_hook is None and before_update is None and not ops._parked_l2:
            if "ticket" not in st and not torch.cuda.is_current_stream_capturing():
                st["ticket"] = torch.zeros(ops.sum_step_ticket_ints(), dtype=torch.int32, device=store.device)
            if "ticket" in st:
                dense, colsums = ops.take_dense_splits()
                scans = [r for r in (sparse.plan_scan_record(ar, self.lazy_embeddings) for ar in owned[:4]) if r is not None]
                if not ops.adam_tf1_sum_step_(store.flat, store.flat_grad, store.flat_m, store.flat_v, arenas, st["step"],
                                              st["ticket"], self.lr, self.beta1, self.beta2, self.eps, dense, colsums,
                                              lazy=self.lazy_embeddings, plan_scans=scans):
                    ops._launch_dense_splits(dense, colsums, st["step"])         # refused: the two launches
                    ops.adam_tf1_step_(store.flat, store.flat_grad, store.flat_m, store.flat_v, arenas, st["step"], None,
                                       self.lr, self.beta1, self.beta2, self.eps, lazy=self.lazy_embeddings, plan_scans=scans)
                for ar in owned:
                    sparse.apply(ar, self.lazy_embeddings, st["step"], self.lr, self.beta1, self.beta2, self.eps)
                return
        # parked gradients: deferred weight-gradient split sums (+ the step counter, advanced by the same launch),
        # l2-regulariser contributions (PNN weight_regularizer)
        nn.apply_parked_grads(step_dev=st["step"] if fused else None)
        if grad_hook is not None:           # data-parallel all-reduce of the flat dense grads
            grad_hook(store)
        if before_update is not None:
            before_update()
        if fused:
            # one launch: dense TF1 Adam over the flat buffer + dense-semantics TF1 Adam over the rows a gradient has ever
            # reached (the update is the identity for all others); lr_t derived on the device from the step counter
            # (+ one workgroup per owner-computes plan: the prefix scan of its bucket totals, which `place` then reads)
            scans = [r for r in (sparse.plan_scan_record(ar, self.lazy_embeddings) for ar in owned[:4]) if r is not None]
            ops.adam_tf1_step_(store.flat, store.flat_grad, store.flat_m, store.flat_v, arenas, st["step"], None,
                               self.lr, self.beta1, self.beta2, self.eps, lazy=self.lazy_embeddings, plan_scans=scans)
            for ar in owned:
                sparse.apply(ar, self.lazy_embeddings, st["step"], self.lr, self.beta1, self.beta2, self.eps)
            return
        if self.lazy_embeddings and arenas:
            raise NotImplementedError("LazyAdamOptimizer needs the fused optimizer launch (HIP device, <= 4 arenas)")
        ops.adam_tf1_advance_(st["step"], st["lr_t"], self.lr, self.beta1, self.beta2)
        for ar in owned:
            sparse.apply(ar, self.lazy_embeddings, st["step"], self.lr, self.beta1, self.beta2, self.eps)
        kw = dict(step=-1, lr=self.lr, beta1=self.beta1, beta2=self.beta2, eps=self.eps,
                  zero_grad=True, lr_t_dev=st["lr_t"])
        if store.flat is not None and store.flat.numel():
            ops.adam_tf1_(store.flat, store.flat_grad, store.flat_m, store.flat_v, **kw)
        for ar in arenas:
            if ar.tracks_live_rows:
                ops.adam_tf1_list_(ar, st["lr_t"], self.beta1, self.beta2, self.eps)
            else:
                ops.adam_tf1_(ar.weight.view(-1), ar.grad.view(-1), ar.m.view(-1), ar.v.view(-1), **kw)


class LazyAdamOptimizer(AdamOptimizer):
    """tf.contrib.opt.LazyAdamOptimizer (the reference's DIEN, /root/reference algorithm/DIEN/dien.py:328): embedding rows
    without a gradient in a step keep their weights AND moments; dense variables update as in Adam.  The six hot-path
    models use tf.train.AdamOptimizer (dense semantics on the tables): selecting this class for them
    (params["lazy_adam"] = True / bench.py --lazy-adam) is a labelled DEVIATION that makes the optimizer cost
    proportional to the rows of the batch instead of the rows ever touched."""
    lazy_embeddings = True


def get_global_step():
    return None


# --------------------------------------------------------------------------------------------
# tf.train.FtrlOptimizer, tf.get_collection(TRAINABLE_VARIABLES, scope), tf.group (Wide&Deep, wide_and_deep.py:251-276)
# --------------------------------------------------------------------------------------------
class FtrlOptimizer:
    """tf.train.FtrlOptimizer(learning_rate) with TF's defaults (initial_accumulator_value 0.1, l1 = l2 = 0, lr_power -0.5):
    ApplyFtrl, restated in include/recalgo_wide.h (not checked against TensorFlow).  Slots: `<var>/Ftrl` (accum) and
    `<var>/Ftrl_1` (linear), TF's names.

    The reference's wide gradient is dense, so TF updates EVERY bucket of the wide kernel in every step.  Reproduced exactly
    by a sparse update: buckets the batch touched get the update (fused with the gradient sum, csrc/wide.hip); a bucket it
    did not touch has g = 0, for which the update (1) on the first step sets var = 0 (linear == 0): the glorot initial values
    survive only until the first training step — one hash_bucket_size-wide zeroing launch, once; (2) on every later step
    recomputes the same accum, linear and var: nothing to do.
    Serves the variables of nn.crossed_indicator_dense layers (kernel and bias); anything else raises."""

    def __init__(self, learning_rate, learning_rate_power=-0.5, initial_accumulator_value=0.1,
                 l1_regularization_strength=0.0, l2_regularization_strength=0.0):
        if float(learning_rate_power) != -0.5:
            raise NotImplementedError("FtrlOptimizer: learning_rate_power = -0.5 (TF's default) only")
        self.lr, self.init = float(learning_rate), float(initial_accumulator_value)
        self.l1, self.l2 = float(l1_regularization_strength), float(l2_regularization_strength)

    def minimize(self, loss, global_step=None, var_list=None) -> TrainOp:
        from . import wide
        from .variables import current_store
        store = current_store()
        if var_list is None:
            var_list = get_collection(GraphKeys.TRAINABLE_VARIABLES)
        op = TrainOp(self, loss, store, var_list)
        if not store.building:
            for st in self._states(store, op.var_list):
                st.ensure_slots(self.init)          # (before any capture: a slot is never allocated by a captured step)
        return op

    @staticmethod
    def _states(store, var_list):
        from . import wide
        found, names = [], {getattr(v, "name", None) for v in var_list}
        for v in var_list:
            st = wide.state_of(store, v)
            if st is None:
                raise NotImplementedError(f"FtrlOptimizer: {getattr(v, 'name', v)} is not a variable of a crossed wide layer "
                                          "(nn.crossed_indicator_dense)")
            if st not in found:
                found.append(st)
        for st in found:
            missing = [v.name for v in (st.kernel, st.bias) if v is not None and v.name not in names]
            if missing:
                raise NotImplementedError(f"FtrlOptimizer: var_list must hold both variables of a wide layer ({missing} left out)")
        return found

    def apply_var_list(self, store: VariableStore, var_list) -> None:
        """the gradients are complete (bias.grad in the flat gradient buffer): update, and leave g = 0 behind"""
        import struct
        f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]      # TF keeps the hyper-parameters as float32
        for st in self._states(store, var_list):
            st.apply_ftrl(f32(self.lr), f32(self.l1), f32(self.l2), f32(self.init))

    def apply_gradients(self, store: VariableStore, grad_hook: Optional[Callable] = None, var_list=None):
        from . import nn
        nn.apply_parked_grads()
        if grad_hook is not None:
            raise NotImplementedError("FtrlOptimizer: data parallelism is not supported")
        self.apply_var_list(store, get_collection(GraphKeys.TRAINABLE_VARIABLES, store=store) if var_list is None else var_list)


class GraphKeys:
    TRAINABLE_VARIABLES = "trainable_variables"


class TableRef:
    """An embedding table in a var_list (the tables live in arenas, not in Variables)."""

    def __init__(self, name: str):
        self.name = name

    def __repr__(self):
        return f"TableRef({self.name})"


def _trainable_names(store: VariableStore):
    names = [n for n in store.order if store.vars[n].trainable and n not in {b for b, _ in store._alias.values()}]
    names += [n for n, v in store.vars.items() if n in store._alias and v.trainable]
    for ar in store.arenas.values():
        if ar.trainable:
            names += list(ar.tables)
    return names


def get_collection(key, scope: Optional[str] = None, store: Optional[VariableStore] = None):
    """tf.get_collection(tf.GraphKeys.TRAINABLE_VARIABLES, scope=...): the trainable variables (and embedding tables, as
    TableRefs) whose name starts with `scope` (TF matches the scope as a prefix), in creation order."""
    from .variables import current_store
    if key != GraphKeys.TRAINABLE_VARIABLES:
        raise NotImplementedError(f"get_collection: only GraphKeys.TRAINABLE_VARIABLES (got {key!r})")
    store = store or current_store()
    names = [n for n in _trainable_names(store) if scope is None or n.startswith(scope)]
    return [store.vars[n] if n in store.vars else TableRef(n) for n in names]


class _Group:
    """The optimizers of group(op, op, ...): ONE backward pass has filled the gradients; each optimizer then updates its
    var_list.  FTRL ops run first, inside the Adam op's `before_update` (they consume and zero the gradients of their
    variables), then the one Adam launch sweeps everything — the identity on the variables it does not own."""

    def __init__(self, ops):
        self.ops = list(ops)
        store = self.ops[0].store
        self.adam = [op for op in self.ops if isinstance(op.optimizer, AdamOptimizer)]
        self.ftrl = [op for op in self.ops if isinstance(op.optimizer, FtrlOptimizer)]
        if len(self.adam) > 1 or len(self.adam) + len(self.ftrl) != len(self.ops):
            raise NotImplementedError("group: at most one Adam op, any number of FTRL ops")
        if any(op.loss is not self.ops[0].loss or op.store is not store for op in self.ops):
            raise NotImplementedError("group: every op must minimize the same loss (one backward pass)")
        if not store.building:
            claimed = [v.name for op in self.ops for v in (op.var_list if op.var_list is not None else get_collection(
                GraphKeys.TRAINABLE_VARIABLES, store=store))]
            if sorted(claimed) != sorted(_trainable_names(store)):
                raise NotImplementedError("group: the ops' var_lists must partition the trainable variables "
                                          f"({len(claimed)} claimed, {len(_trainable_names(store))} trainable)")

    def apply_gradients(self, store: VariableStore, grad_hook: Optional[Callable] = None):
        def ftrl_updates():
            for op in self.ftrl:
                op.optimizer.apply_var_list(store, op.var_list)
        if self.adam:
            self.adam[0].optimizer.apply_gradients(store, grad_hook, before_update=ftrl_updates)
        else:
            from . import nn
            nn.apply_parked_grads()
            ftrl_updates()


def group(*train_ops) -> TrainOp:
    """tf.group(wide_part_op, deep_part_op): one train op — one backward pass, every optimizer on its own var_list, the
    global step advanced once."""
    if not train_ops:
        raise ValueError("group: no ops")
    return TrainOp(_Group(train_ops), train_ops[0].loss, train_ops[0].store)


# --------------------------------------------------------------------------------------------
# tf.metrics.{accuracy, auc} (a14) — streaming accumulators
# --------------------------------------------------------------------------------------------
class Metric:
    def update(self):
        raise NotImplementedError

    def result(self) -> float:
        raise NotImplementedError


def _takes_part(mask):
    """mask (one value per row) -> bool [n]: the rows of a masked metric that take part, mask > 0.5 (a NaN takes no part);
    include/recalgo_maskmetrics.h makes the same comparison on the device"""
    return mask.detach().reshape(-1) > 0.5


class AccuracyMetric(Metric):
    """tf.metrics.accuracy; with `mask` (tf's 0/1 `weights=`) over the rows whose mask is > 0.5."""

    def __init__(self, labels, predictions, mask=None):
        self.labels, self.predictions, self.mask = labels, predictions, mask
        self.correct, self.total = 0.0, 0.0

    def merge(self, other):
        self.labels, self.predictions, self.mask = other.labels, other.predictions, other.mask

    def update(self):
        same = self.labels.reshape(-1) == self.predictions.reshape(-1)
        if self.mask is None:
            self.correct += float(same.sum())
            self.total += self.labels.numel()
        else:
            part = _takes_part(self.mask)
            self.correct += float((same & part).sum())
            self.total += float(part.sum())

    def result(self):
        return self.correct / max(self.total, 1.0)


class AUCMetric(Metric):
    """tf.metrics.auc defaults: 200 thresholds, trapezoidal ROC; with `mask` (tf's 0/1 `weights=`) over the rows
    whose mask is > 0.5."""

    def __init__(self, labels, predictions, num_thresholds=200, mask=None):
        self.labels, self.predictions, self.n, self.mask = labels, predictions, num_thresholds, mask
        eps = 1e-7
        th = [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)]
        self.th = torch.tensor([0.0 - eps] + th + [1.0 + eps], dtype=torch.float32)
        self.tp = torch.zeros(num_thresholds, dtype=torch.float64)
        self.fp = torch.zeros_like(self.tp)
        self.fn = torch.zeros_like(self.tp)
        self.tn = torch.zeros_like(self.tp)

    def merge(self, other):
        self.labels, self.predictions, self.mask = other.labels, other.predictions, other.mask

    def update(self):
        p = self.predictions.detach().reshape(1, -1).float().cpu()
        y = self.labels.detach().reshape(1, -1).cpu() > 0.5
        if self.mask is not None:
            part = _takes_part(self.mask).cpu()
            p, y = p[:, part], y[:, part]
        pred_pos = p > self.th.unsqueeze(1)
        self.tp += (pred_pos & y).sum(1)
        self.fp += (pred_pos & ~y).sum(1)
        self.fn += (~pred_pos & y).sum(1)
        self.tn += (~pred_pos & ~y).sum(1)

    def result(self):
        eps = 1e-7
        tpr = (self.tp + eps) / (self.tp + self.fn + eps)
        fpr = self.fp / (self.fp + self.tn + eps)
        return float(((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2).sum())


GROUP_AUC_WEIGHTINGS = ("uniform", "samples")


def group_auc_value(num2, pos, neg, weighting: str = "uniform"):
    """The one step from a task's integer counts per group (int64 arrays [G]) to (the metric, its valid groups), for the host
    loop and for the device path alike, so both return the same bits.  A group is valid when pos * neg > 0; its AUC is
    num2 / (2 pos neg) in float64; "uniform" (uAUC): the mean over the valid groups; "samples" (GAUC): the mean weighted by
    pos + neg; no valid group: 0.0."""
    import numpy as np
    if weighting not in GROUP_AUC_WEIGHTINGS:
        raise ValueError(f"group AUC weighting {weighting!r}: expected one of {GROUP_AUC_WEIGHTINGS}")
    num2, pos, neg = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (num2, pos, neg))
    valid = pos * neg > 0
    n = int(valid.sum())
    if n == 0:
        return 0.0, 0
    auc = num2[valid].astype(np.float64) / (2.0 * (pos[valid] * neg[valid]).astype(np.float64))
    if weighting == "uniform":
        return float(auc.sum() / n), n
    w = (pos[valid] + neg[valid]).astype(np.float64)
    return float((w * auc).sum() / w.sum()), n


def group_auc_counts(groups, y, p, num_groups: int):
    """include/recalgo_gauc.h's counts on the host: groups int64 [n], y bool [n], p float32 [n] -> (num2, pos, neg [G] int64,
    skipped), group by group with broadcast comparisons in float32 (the positives of a large group in slices)."""
    import numpy as np
    G = int(num_groups)
    num2, pos, neg = (np.zeros(G, np.int64) for _ in range(3))
    inside = (groups >= 0) & (groups < G)
    g, y, p = groups[inside], y[inside], p[inside].astype(np.float32, copy=False)
    order = np.argsort(g, kind="stable")
    g, y, p = g[order], y[order], p[order]
    ids, starts = np.unique(g, return_index=True)
    ends = np.append(starts[1:], g.size)
    for u, a, b in zip(ids.tolist(), starts.tolist(), ends.tolist()):
        pp, pn = p[a:b][y[a:b]], p[a:b][~y[a:b]]
        pos[u], neg[u] = pp.size, pn.size
        if pp.size and pn.size:
            step = max(1, (1 << 22) // pn.size)
            for k in range(0, pp.size, step):
                s = pp[k:k + step, None]
                num2[u] += 2 * int((s > pn[None, :]).sum()) + int((s == pn[None, :]).sum())
    return num2, pos, neg, int(groups.size - g.size)


class GroupAUCMetric(Metric):
    """The AUC of each group's own rows (a group: a user), averaged over the groups that have a positive and a negative row:
    uAUC (weighting="uniform") or, weighted by the group's rows, GAUC ("samples").  groups: the int64 id of each row, valid in
    0 .. num_groups - 1; any other id (-1: out of vocabulary) belongs to no group.  The definition is include/recalgo_gauc.h's,
    in integers; update() keeps host copies of the batch and result() counts group by group, so the host loop serves it without a
    kernel; under device_metrics the EvalAccumulator fills the same counts from the device (fill).  After result():
    .num2 / .pos / .neg (int64 [G]), .valid_groups, .skipped_rows."""

    def __init__(self, labels, predictions, groups, num_groups, weighting="uniform"):
        if weighting not in GROUP_AUC_WEIGHTINGS:
            raise ValueError(f"group_auc: weighting {weighting!r}, expected one of {GROUP_AUC_WEIGHTINGS}")
        if not (isinstance(num_groups, int) and not isinstance(num_groups, bool) and num_groups >= 1):
            raise ValueError(f"group_auc: num_groups = {num_groups!r}, expected an int >= 1")
        self.labels, self.predictions, self.groups = labels, predictions, groups
        self.num_groups, self.weighting = num_groups, weighting
        self._rows = []
        self.num2 = self.pos = self.neg = None
        self.valid_groups, self.skipped_rows = 0, 0

    def merge(self, other):
        self.labels, self.predictions, self.groups = other.labels, other.predictions, other.groups

    def update(self):
        self._rows.append((self.groups.detach().reshape(-1).cpu().numpy(), (self.labels.detach().reshape(-1).cpu() > 0.5).numpy(),
                           self.predictions.detach().reshape(-1).float().cpu().numpy()))
        self.num2 = None

    def fill(self, num2, pos, neg, skipped: int) -> None:
        """the counts as the device path found them, in place of update()"""
        self.num2, self.pos, self.neg, self.skipped_rows = num2, pos, neg, int(skipped)

    def result(self):
        import numpy as np
        if self.num2 is None:
            if self._rows:
                g, y, p = (np.concatenate(c) for c in zip(*self._rows))
            else:
                g, y, p = np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0, np.float32)
            self.num2, self.pos, self.neg, self.skipped_rows = group_auc_counts(g, y, p, self.num_groups)
        value, self.valid_groups = group_auc_value(self.num2, self.pos, self.neg, self.weighting)
        return value


class metrics:  # namespace mirror of tf.metrics
    @staticmethod
    def group_auc(labels, predictions, groups, num_groups, weighting="uniform"):
        m = GroupAUCMetric(labels, predictions, groups, num_groups, weighting)
        return (m, m)

    @staticmethod
    def accuracy(labels, predictions, mask=None):
        m = AccuracyMetric(labels, predictions, mask)
        return (m, m)

    @staticmethod
    def auc(labels, predictions, num_thresholds=200, mask=None):
        """mask, not tf's `weights`: only 0/1 keeps every count an integer"""
        m = AUCMetric(labels, predictions, num_thresholds, mask)
        return (m, m)


class EvalAccumulator:
    """The metrics of one evaluate() call, accumulated on the device: one recalgo_metrics_update launch per batch
    (ops.metrics_update: an integer histogram per AUC metric, two counters per accuracy metric, the loss sum), nothing read back
    until finish(), which makes ONE device-to-host copy of the state buffer and fills the first batch's Metric objects from the
    counts; their own result() then produces the values, so the trapezoid and the epsilons stay in AUCMetric.

    Exact: a prediction's bin is #{j : p > th[j]}, the very comparisons AUCMetric.update makes, so
    tp[j] = sum over bin > j of hist[1][bin] is the count update() would have added up, as an integer (float64 holds it exactly
    below 2**53); the loss sum is the same sequence of double additions as `loss_sum += float(spec.loss)`.

    Serves AUCMetric and AccuracyMetric over fp32 tensors on the HIP device with a fp32 scalar loss there (`of` returns None for
    any other spec: the caller keeps the host loop), and beside at least one of them up to 8 GroupAUCMetric over one tensor of
    int64 group ids: one recalgo_gauc_append launch per batch logs their rows on the device (ops.gauc_append), finish() groups the
    log and counts the pairs there (ops.gauc_finish), and the integer counts per group come back in the same copy.  A spec
    without a GroupAUCMetric makes exactly the launches, and owns exactly the state buffer, it did before they existed.

    An AUCMetric or AccuracyMetric may carry a mask (fp32 on the device, one value per row: the rows with mask > 0.5 take part).
    A spec with such a metric makes its one launch per batch through ops.maskmetrics_update, into the same state layout; a spec
    without one makes the launches it made before masks existed."""

    def __init__(self, spec: EstimatorSpec, device, group_auc_capacity: int = GROUP_AUC_CAPACITY):
        self.device = torch.device(device)
        self.keys, self.metrics, self._th, self._layout = [], {}, {}, None
        self.group_keys, self.gauc, self.group_auc_capacity = [], None, check_group_auc_capacity(group_auc_capacity)
        slots = self._slots(spec, first=True)
        _, self.first, words = ops.metrics_slot_table([s[:-1] for s in slots] if self.masked else slots)
        self.state = torch.zeros(words, dtype=torch.int64, device=spec.loss.device)
        if self.group_keys:              # the row log, its result and the finish's scratch: allocated here, never in add()
            self.gauc = ops.gauc_state(self.metrics[self.group_keys[0]].num_groups, len(self.group_keys), self.group_auc_capacity,
                                       spec.loss.device)

    @classmethod
    def of(cls, spec: EstimatorSpec, device, group_auc_capacity: int = GROUP_AUC_CAPACITY) -> Optional["EvalAccumulator"]:
        return cls(spec, device, group_auc_capacity) if cls.serves(spec, device) else None

    @staticmethod
    def serves(spec: EstimatorSpec, device) -> bool:
        def on_device(t):
            return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() > 0
                    and _same_device(t.device, device))
        metric_ops = spec.eval_metric_ops or {}
        grouped = [m for m, _ in metric_ops.values() if type(m) is GroupAUCMetric]
        if not (0 < len(metric_ops) - len(grouped) <= ops.METRICS_MAX_SLOTS) or not on_device(spec.loss) or spec.loss.numel() != 1:
            return False
        if grouped:                      # up to 8 of them, over ONE tensor of int64 ids on the device and one number of groups
            g = grouped[0].groups
            if len(grouped) > ops.GAUC_MAX_TASKS or not ops.gauc_shape_ok(grouped[0].num_groups, len(grouped), 1) \
                    or not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.int64 and _same_device(g.device, device)) \
                    or g.numel() != grouped[0].labels.numel() or ops.metrics_element_stride(g) is None \
                    or any(m.groups is not g or m.num_groups != grouped[0].num_groups for m in grouped):
                return False
        n = None
        for m, _ in metric_ops.values():
            if type(m) not in (AUCMetric, AccuracyMetric, GroupAUCMetric) or not (on_device(m.labels) and on_device(m.predictions)):
                return False
            n = m.labels.numel() if n is None else n
            if m.labels.numel() != n or m.predictions.numel() != n or ops.metrics_element_stride(m.labels) is None \
                    or ops.metrics_element_stride(m.predictions) is None:
                return False
            mask = getattr(m, "mask", None)          # of an AUC or accuracy metric: fp32 on the device, one value per row
            if mask is not None and not (on_device(mask) and mask.numel() == n and ops.metrics_element_stride(mask) is not None):
                return False
            if type(m) is AUCMetric and not (2 <= m.n <= ops.METRICS_MAX_THRESHOLDS and m.th.numel() == m.n):
                return False
        return True

    def _slots(self, spec: EstimatorSpec, first: bool = False):
        metric_ops = spec.eval_metric_ops or {}
        layout = [(k, type(m), getattr(m, "n", None), getattr(m, "mask", None) is not None) for k, (m, _) in metric_ops.items()]
        if first:
            self._layout = layout
            for k, (m, _) in metric_ops.items():
                self.metrics[k] = m
                if type(m) is GroupAUCMetric:  # (not a slot of the metrics launch: a task of the append launch)
                    self.group_keys.append(k)
                    continue
                self.keys.append(k)
                if type(m) is AUCMetric:       # the thresholds as the metric states them, on the device once
                    self._th[k] = m.th.to(device=m.predictions.device, dtype=torch.float32).contiguous()
        elif layout != self._layout or not self.serves(spec, self.device):
            raise ValueError("evaluate(device_metrics=True): a batch's eval_metric_ops differ from the first batch's "
                             f"({[k for k, *_ in layout]} against {list(self.metrics)}), or are not fp32 tensors on {self.device}")
        slots = [("auc", m.labels, m.predictions, self._th[k]) if type(m) is AUCMetric else ("accuracy", m.labels, m.predictions)
                 for k, (m, _) in metric_ops.items() if type(m) is not GroupAUCMetric]
        if first:
            self.masked = any(masked for *_, masked in layout)
        if self.masked:                        # every slot carries its mask (or None) behind it: ops.maskmetrics_update's tuples
            masks = [m.mask for m, _ in metric_ops.values() if type(m) is not GroupAUCMetric]
            slots = [(*slot, mask) for slot, mask in zip(slots, masks)]
        return slots

    def add(self, spec: EstimatorSpec) -> None:
        """One launch: the batch's metrics and loss into the state buffer (recalgo_metrics_update; when a metric of the spec
        carries a mask, recalgo_maskmetrics_update for all of them); with group metrics one more, for all of them together:
        the batch's rows into the log.  Capturable (no read-back, no allocation)."""
        update = ops.maskmetrics_update if self.masked else ops.metrics_update     # (one launch either way, for all slots)
        update(self._slots(spec), spec.loss.detach(), self.state)
        if self.gauc is not None:
            grouped = [spec.eval_metric_ops[k][0] for k in self.group_keys]
            ops.gauc_append(self.gauc, grouped[0].groups, [(m.labels, m.predictions) for m in grouped])

    @staticmethod
    def fill_auc(m: "AUCMetric", hist: torch.Tensor) -> None:
        """hist [2, N + 1] integer counts of (label > 0.5, #{j : p > th[j]}) -> m.tp / fp / fn / tn, as update() accumulates them"""
        hist = hist.to(torch.int64).reshape(2, m.n + 1)
        above = hist.flip(1).cumsum(1).flip(1)[:, 1:]             # above[y][j] = sum over bin > j of hist[y][bin]
        total = hist.sum(1, keepdim=True)
        m.fp, m.tp = above.to(torch.float64).unbind(0)
        m.tn, m.fn = (total - above).to(torch.float64).unbind(0)

    @staticmethod
    def fill_accuracy(m: "AccuracyMetric", correct: int, total: int) -> None:
        m.correct, m.total = float(correct), float(total)

    def finish(self):
        """-> ({key: filled Metric}, loss sum, batches) after ONE device-to-host copy (with group metrics: the finish launches
        first, and their result travels behind the state in that copy).  Rows that found no room in the log: RuntimeError."""
        if self.gauc is None:
            host = self.state.cpu()
        else:
            both = torch.cat([self.state, ops.gauc_finish(self.gauc)]).cpu()
            host, counts = both[:self.state.numel()], both[self.state.numel():]
            skipped, dropped, _, num2, pos, neg = ops.gauc_counts(counts, self.gauc.G, self.gauc.T)
            if dropped > 0:
                raise RuntimeError(f"evaluate(): group_auc_capacity = {self.group_auc_capacity} rows, and {dropped} more rows were "
                                   "dropped; a per-group AUC over part of the data is not reported: raise "
                                   "RunConfig(group_auc_capacity=) to the rows of one evaluation")
            for t, k in enumerate(self.group_keys):
                self.metrics[k].fill(num2[t].copy(), pos[t].copy(), neg[t].copy(), skipped)
        for k, first in zip(self.keys, self.first):
            m = self.metrics[k]
            if type(m) is AUCMetric:
                self.fill_auc(m, host[first:first + 2 * (m.n + 1)])
            else:
                self.fill_accuracy(m, int(host[first]), int(host[first + 1]))
        return self.metrics, float(host[:1].view(torch.float64)), int(host[1])


# --------------------------------------------------------------------------------------------
# hipGraph-captured training step
# --------------------------------------------------------------------------------------------
def _tree_tensors(obj, prefix=""):
    from .feature_column import Ragged
    if isinstance(obj, torch.Tensor):
        yield prefix, obj
    elif isinstance(obj, Ragged):
        yield prefix + ".values", obj.values
        yield prefix + ".offsets", obj.offsets
    elif isinstance(obj, dict):
        for k in sorted(obj):
            yield from _tree_tensors(obj[k], f"{prefix}/{k}")


def _byte_span(t: torch.Tensor):
    """[lo, hi) byte range of the storage that tensor t covers."""
    lo = t.storage_offset() * t.element_size()
    if t.numel() == 0:
        return lo, lo
    last = sum((d - 1) * st for d, st in zip(t.shape, t.stride()))
    return lo, lo + (last + 1) * t.element_size()


class DeviceBatch(dict):
    """features whose tensors (and the labels') are views of ONE device allocation laid out as `device_span[1]` describes:
    device_span = (uint8 tensor over the whole allocation, signature) — what Estimator._to_device_one_copy produces and
    GraphedTrainStep.load moves with one copy, without looking at the individual tensors."""
    device_span = None


def _clone_tree(obj):
    """Deep copy of a (features, labels) tree of tensors / Ragged / dicts that preserves storage sharing: tensors that
    are views of one allocation become views (same relative offsets / strides) of ONE cloned allocation — of the byte
    span the views cover, not of the whole storage (a batch that is a slice of a device-resident dataset must not
    duplicate the dataset)."""
    from .feature_column import Ragged
    spans = {}

    def scan(o):
        if isinstance(o, torch.Tensor):
            lo, hi = _byte_span(o)
            key = o.untyped_storage().data_ptr()
            a, b = spans.get(key, (lo, hi))
            spans[key] = (min(a, lo), max(b, hi))
        elif isinstance(o, Ragged):
            scan(o.values); scan(o.offsets)
        elif isinstance(o, dict):
            for v in o.values():
                scan(v)
        elif isinstance(o, (tuple, list)):
            for v in o:
                scan(v)
    scan(obj)
    storages = {}

    def cl(t):
        st = t.untyped_storage()
        key = st.data_ptr()
        lo, hi = spans[key]
        lo -= lo % 16                                           # keep every view's alignment
        if key not in storages:
            part = torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, lo, (max(hi - lo, 0),), (1,))
            storages[key] = part.clone().untyped_storage()
        off = t.storage_offset() - lo // t.element_size()
        return torch.empty(0, dtype=t.dtype, device=t.device).set_(storages[key], off, t.shape, t.stride())

    def walk(o):
        if isinstance(o, torch.Tensor):
            return cl(o)
        if isinstance(o, Ragged):
            return Ragged(cl(o.values), cl(o.offsets))
        if isinstance(o, dict):
            return {k: walk(v) for k, v in o.items()}
        if isinstance(o, (tuple, list)):
            return type(o)(walk(v) for v in o)
        return o
    return walk(obj)


# True: a captured step's first `prepare` launch is kept out of the graph and enqueued in front of every replay, where it also
# moves a one-span batch into the static input buffers (sparse.StepHead) — no copy launch.  False (read when a step is captured):
# everything inside the graph, the batch moved by a copy launch of its own (tests compare the two).
FEED_IN_PREPARE = True
HOUSEKEEPING_EVERY = 32      # steps between VariableStore.housekeeping() calls (live-row list ordering)
OVERFLOW_POLL_EVERY = 64     # steps between reads of the static row-exchange overflow flag (N > 1; one host sync)


def _quiesce_collectives() -> None:
    """Before a capture that contains RCCL collectives: let torch.distributed's watchdog thread retire the EAGER collectives
    issued so far.  It polls their completion events every 100 ms; HIP refuses an event query (hipErrorCapturedEvent:
    'operation not permitted on an event last recorded in a capturing stream') once the communicator's internal stream —
    on which those events were recorded — has joined a capture, and the watchdog then aborts the process (seen as a rare
    crash of the warm-up-then-capture sequence).  All eager work is complete here (the caller has synchronised), so one
    poll interval empties the watchdog's list."""
    try:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_backend() != "nccl":
            return
    except Exception:            # (custom collectives objects, e.g. the host-staged bring-up adapter: no watchdog)
        return
    import time
    torch.cuda.synchronize()
    time.sleep(0.5)


class BatchShapeMismatch(ValueError):
    """A batch whose structure / shapes are not those the step was captured on (the last partial batch of an epoch): the
    ONLY condition under which the training loop runs a step eagerly beside a captured graph — any other error of the
    replay path propagates."""


class GraphedTrainStep:
    """Capture `step_fn(features, labels)` (forward + backward + optimizer, everything enqueued
    on the current stream) into a hipGraph over static input buffers; `__call__` copies the new
    batch into the static buffers and replays.  Shapes must not change between calls."""

    # True (set by an Estimator with RunConfig(ragged_capacity=)): the static `values` of a Ragged is a buffer of fixed capacity,
    # and load() accepts the unpadded values of a device-resident batch that fit it
    pad_values = False
    # the step's head (sparse.StepHead; None: every launch is a node of the graph) and the one-span load left to its next launch
    _head = _feed = None
    head_launches = fused_feeds = 0                           # head launches in front of a replay; ... that carried the batch

    def __init__(self, step_fn: Callable, features, labels, warmup: int = 3):
        self.step_fn = step_fn
        # PRIVATE static input buffers: clones of the first batch (storage-preserving: the 26 id columns of one [B, F]
        # matrix stay views of one allocation).  Capturing on the caller's tensors would overwrite the user's batch on
        # every load() and replay stale data when that tensor comes round again.
        span = getattr(features, "device_span", None)
        features, labels = _clone_tree((features, labels))
        self.static_f, self.static_l = features, labels
        self._static = list(_tree_tensors(features, "f")) + list(_tree_tensors(labels, "l"))
        # a batch that is ONE allocation with a known layout (DeviceBatch): later batches of the same layout are loaded by one
        # copy of the whole span (the clone kept the layout: every static tensor sits at its source's offset)
        self._span_plan = None
        if span is not None and self._static:
            st0 = self._static[0][1].untyped_storage()
            if (st0.nbytes() >= span[0].numel() and all(t.untyped_storage().data_ptr() == st0.data_ptr() for _, t in self._static)
                    and all(a.storage_offset() == b.storage_offset() and a.stride() == b.stride() and a.shape == b.shape
                            for (_, a), (_, b) in zip(self._static, list(_tree_tensors(span[2][0], "f")) + list(_tree_tensors(span[2][1], "l"))))):
                dst = torch.empty(0, dtype=torch.uint8, device=span[0].device).set_(st0, 0, (span[0].numel(),), (1,))
                self._span_plan = (span[1], dst)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self.out = step_fn(features, labels)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        _quiesce_collectives()
        self.graph = torch.cuda.CUDAGraph()
        # the step's head (sparse.HeadRecorder): its first `prepare` launch, when its ids are views of a static input allocation
        from . import sparse
        rec = None
        if FEED_IN_PREPARE:
            storages = {t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for _, t in self._static if t.is_cuda}
            rec = sparse.HeadRecorder(storages.items())
        prev, sparse.head_recorder = sparse.head_recorder, rec
        try:
            # thread_local: HIP calls of OTHER threads (the RCCL watchdog of torch.distributed polls events)
            # must not be treated as capture violations while this thread captures
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self.out = step_fn(features, labels)
        finally:
            sparse.head_recorder = prev
        if rec is not None:
            self._head = rec.head
        self._feed_ok = {}
        self.warmup_steps = warmup
        owner = getattr(step_fn, "__self__", None)                # Estimator.train_step -> its VariableStore
        self._housekeeping = getattr(getattr(owner, "store", None), "housekeeping", None)
        self._calls = 0

    def load(self, features, labels):
        """Copy a new batch into the static input buffers.  Inputs that are views of one
        allocation with the same layout on both sides (the 26 id columns of one [B, F] matrix)
        are moved by a single whole-allocation copy — which a step with a head leaves to the head's launch in front of the
        next replay (_feed_through_head): until that __call__ the static buffers hold the previous batch."""
        span = getattr(features, "device_span", None)
        self._feed = None
        if span is not None and self._span_plan is not None and span[1] == self._span_plan[0]:
            dst = self._span_plan[1]
            if not self._feed_through_head(dst.data_ptr(), span[0], span[0].data_ptr(), dst.numel()):
                _device_copy(dst, span[0])
            return
        new = list(_tree_tensors(features, "f")) + list(_tree_tensors(labels, "l"))
        if len(new) != len(self._static):
            raise BatchShapeMismatch("graphed step: the input structure changed")
        spans = self._static_spans()
        groups = {}
        pads = []
        for i, ((k0, dst), (k1, src)) in enumerate(zip(self._static, new)):
            if k0 != k1 or dst.shape != src.shape:
                if (self.pad_values and k0 == k1 and k1.endswith(".values") and src.dim() == 1 and src.numel() <= dst.numel()
                        and src.dtype == dst.dtype == torch.int64 and src.device == dst.device and src.is_cuda):
                    pads.append((dst, src))      # (an unpadded device Ragged that fits the static buffer: see below)
                    continue
                raise BatchShapeMismatch(f"graphed step: input {k1} changed shape/structure")
            if dst.dtype == src.dtype and dst.stride() == src.stride() and src.device == dst.device:
                # (same shape, strides and dtype: the source covers a byte span of the same length as the destination's)
                groups.setdefault((spans[i][0], src.untyped_storage().data_ptr()), []).append((i, src.storage_offset() * spans[i][3]))
            else:
                dst.copy_(src, non_blocking=True)
        singles = []
        for items in groups.values():
            # views of one allocation on both sides with the same relative layout: ONE copy of the byte span they cover —
            # provided no OTHER static input lives inside that span (the copy overwrites the gaps between the views too)
            if len(items) > 1:
                d_lo = min(spans[i][1] for i, _ in items)
                d_hi = max(spans[i][2] for i, _ in items)
                s_lo = min(lo for _, lo in items)
                mine = {i for i, _ in items}
                st_ptr = spans[items[0][0]][0]
                alone = all(k in mine or sp[0] != st_ptr or sp[2] <= d_lo or sp[1] >= d_hi for k, sp in enumerate(spans))
                if alone and d_hi > d_lo and all(spans[i][1] - d_lo == lo - s_lo for i, lo in items):
                    d0, s0 = self._static[items[0][0]][1], new[items[0][0]][1]
                    dv = self._dst_views.get((spans[items[0][0]][0], d_lo, d_hi))
                    if dv is None:
                        dv = torch.empty(0, dtype=torch.uint8, device=d0.device).set_(d0.untyped_storage(), d_lo, (d_hi - d_lo,), (1,))
                        self._dst_views[(spans[items[0][0]][0], d_lo, d_hi)] = dv
                    sv = torch.empty(0, dtype=torch.uint8, device=s0.device).set_(s0.untyped_storage(), s_lo, (d_hi - d_lo,), (1,))
                    if not self._feed_through_head(dv.data_ptr(), sv, sv.data_ptr(), d_hi - d_lo):
                        _device_copy(dv, sv)
                    continue
            singles.extend(i for i, _ in items)
        for i in singles:                        # (after every span copy: a per-tensor copy is never overwritten by one)
            self._static[i][1].copy_(new[i][1], non_blocking=True)
        for dst, src in pads:
            # the values of a device-resident Ragged go into the static buffer of fixed capacity and the -1 tail is written
            # by the same launch (recalgo_ragged_pad)
            ops.ragged_pad(src.contiguous(), dst.numel(), out=dst)

    def _feed_through_head(self, dst: int, keep: torch.Tensor, src: int, nbytes: int) -> bool:
        """The one-copy load of static bytes [dst, dst + nbytes) from the caller's [src, ..): left to the step's head when the span
        covers the ids of every source of the head and recalgo_scatter_prepare_feed accepts it — the next __call__ launches the
        head on the caller's ids with the copy as workgroups of its grid (`keep` holds the caller's allocation until then)."""
        h = self._head
        if h is None or self._feed is not None or not (dst <= h.span_ptr + h.lo and h.span_ptr + h.hi <= dst + nbytes):
            return False
        ok = self._feed_ok.get((dst, src, nbytes))
        if ok is None:
            if len(self._feed_ok) >= 256:
                self._feed_ok.clear()
            ok = self._feed_ok[(dst, src, nbytes)] = (
                dst != src and keep.is_cuda and keep.device == h.arena.weight.device and keep.is_contiguous()
                and bool(_lib.load().recalgo_scatter_prepare_feed_supported(dst, src, nbytes)))
        if ok:
            self._feed = (dst, src, nbytes, keep)
        return ok

    def _static_spans(self):
        """Per static input: (storage pointer, first byte, end byte, element size) — computed once: the per-step path of a
        host-fed training loop is Python, and every tensor method call in it costs as much as a tenth of the GPU step."""
        sp = self.__dict__.get("_spans")
        if sp is None:
            sp = self._spans = [(t.untyped_storage().data_ptr(),) + _byte_span(t) + (t.element_size(),) for _, t in self._static]
            self._dst_views = {}
        return sp

    def __call__(self, features=None, labels=None):
        if features is not None:
            self.load(features, labels)
        if self._head is not None:
            feed, self._feed = self._feed, None
            self._head.launch(feed)
            self.head_launches += 1
            self.fused_feeds += feed is not None
        self.graph.replay()
        self._calls += 1
        if self._housekeeping is not None and self._calls % HOUSEKEEPING_EVERY == 0:
            self._housekeeping()       # enqueued between replays on the same stream; never waits for the GPU
        return self.out


# --------------------------------------------------------------------------------------------
# Estimator
# --------------------------------------------------------------------------------------------
def _device_copy(dst: torch.Tensor, src: torch.Tensor) -> None:
    """The batch -> static input buffer copy of a captured step.  Device to device on one GPU it is the library's own copy
    kernel (recalgo_copy_bytes: ~2 us for the 0.9 MB of a 4096-example batch; the runtime's copy kernel took 7.1 us of the
    230 us DCN step, profiles/r04zz_dcn_kernel_stats.md)."""
    if dst.is_cuda and src.is_cuda and dst.device == src.device and dst.is_contiguous() and src.is_contiguous():
        from . import ops
        ops.copy_bytes(dst, src)
    else:
        dst.copy_(src, non_blocking=True)


def _host_copy(dst: torch.Tensor, src: torch.Tensor) -> None:
    """dst.copy_(src) for host tensors on the training loop's thread.  Same dtype, both contiguous: ONE memmove — a batch's
    id matrix is ~1 MB, for which Tensor.copy_ starts an intra-op parallel region over every core of the host (128 threads
    on the GPU box); next to the reader's decode threads that costs milliseconds per call (measured: 1.6 ms against 0.08 ms),
    the whole difference between a host-fed loop at 0.5 M and at 8 M examples/s."""
    if (dst.dtype == src.dtype and dst.numel() == src.numel() and dst.is_contiguous() and src.is_contiguous()
            and dst.device.type == "cpu" and src.device.type == "cpu"):
        import ctypes
        ctypes.memmove(dst.data_ptr(), src.data_ptr(), dst.numel() * dst.element_size())
    else:
        dst.copy_(src)


class Estimator:
    def __init__(self, model_fn, params=None, config: Optional[RunConfig] = None, model_dir=None):
        self.model_fn, self.params = model_fn, params or {}
        self.config = config or RunConfig(model_dir=model_dir)
        dev = self.config.device
        if dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("recalgorithm_amd needs a HIP device (no CPU fallback)")
            dev = "cuda"
        self.device = torch.device(dev)
        self.store = VariableStore(self.device, seed=self.config.seed)
        self.global_step = 0
        self._built = False
        self._after_build = []           # callables run once at the end of the build (parallel.attach_data_parallel)
        self.grad_hook = None     # set by parallel wrappers (dense-grad all-reduce)
        self.loss_grad_scale = None   # 1/world under data parallelism (parallel.attach_data_parallel)
        self._seed_grad, self._seed_value = None, None
        self._pinned = {}                # (shape, dtype) -> ring of pinned staging buffers (_h2d)
        # RunConfig(ragged_capacity=): see _fit_ragged
        self.ragged_overflows = 0        # batches that did not fit their capacity and ran eagerly, unpadded
        self.capture_refused = None      # why no step of this model is captured over ragged inputs (store.data_dependent)
        self.graph_replays = 0           # steps (train and evaluate) that were one replay of a captured graph
        self._ragged_keys = set()        # keys that have arrived as a Ragged ...
        self._ragged_frozen = False      # ... before the first capture
        self._ragged_seen = {}           # key -> largest nnz of the eager warm-up batches ("auto")
        self._ragged_caps = {}           # key -> the capacity "auto" settled on when the warm-up ended

    # -- plumbing -------------------------------------------------------------------------
    _STAGING_RING = 8

    def _fit_ragged(self, features, warm: bool, loading: bool = False):
        """RunConfig(ragged_capacity=...): -> (features with every Ragged padded to its capacity, True), or (features as they
        came, False) for a batch that must run eagerly: one whose nnz exceeds the capacity of any key (never truncated;
        counted in ragged_overflows), or one with a ragged key the policy gives no capacity.
        A key that has arrived as a Ragged before and now comes as a dense [B] id vector (no row of the batch holds two values)
        is presented as B bags of one value.  Host values are padded while the pinned staging buffer is filled; device values
        by one launch — or, `loading` (the batch goes into a captured step's static buffers next), not at all: GraphedTrainStep.load
        pads them straight into the static buffer.  `warm`: the eager warm-up steps, which "auto" takes its capacity from."""
        from .feature_column import Ragged, pad_ragged
        policy = self.config.ragged_capacity
        if policy is None or self.capture_refused is not None or not isinstance(features, dict):
            return features, policy is None
        if not self._ragged_frozen:          # (until a step is captured: afterwards the padded keys are those of the capture)
            self._ragged_keys |= {k for k, v in features.items() if isinstance(v, Ragged)}
        if not self._ragged_keys and not any(isinstance(v, Ragged) for v in features.values()):
            return features, True
        out, fits = dict(features), True
        for k in sorted(set(self._ragged_keys) | {k for k, v in features.items() if isinstance(v, Ragged)}):
            v = features.get(k)
            if isinstance(v, torch.Tensor) and v.dtype == torch.int64 and (v.dim() == 1 or (v.dim() == 2 and v.shape[1] == 1)):
                v = dense_as_ragged(v)
            if not isinstance(v, Ragged):
                continue
            nnz, rows = int(v.values.numel()), int(v.offsets.numel()) - 1
            if policy == "auto":
                if warm and k not in self._ragged_caps:
                    self._ragged_seen[k] = max(self._ragged_seen.get(k, 0), nnz)
                    cap = ragged_auto_capacity(self._ragged_seen[k])
                else:
                    if k not in self._ragged_caps and k in self._ragged_seen:
                        self._ragged_caps[k] = ragged_auto_capacity(self._ragged_seen[k])
                    cap = self._ragged_caps.get(k)
            else:
                cap = ragged_capacity_for(policy, k, rows)
            if ragged_overflows(nnz, cap):
                fits = False
                continue
            if v.values.device.type == "cpu" and self.device.type == "cuda":
                def fill(buf, vals=v.values, n=nnz):
                    if n:
                        _host_copy(buf[:n], vals.contiguous())
                    buf[n:].fill_(-1)
                out[k] = Ragged(self._h2d(fill, (cap,), torch.int64), v.offsets)
            elif loading and v.values.is_cuda:
                out[k] = v
            else:
                out[k] = pad_ragged(v, cap)
        if not fits:
            self.ragged_overflows += 1
            return features, False
        return out, True

    def _capturable(self, features, fits: bool) -> bool:
        """May a step over this batch be captured (or replayed)?  Without a ragged capacity: a batch of dense tensors only."""
        if self.config.ragged_capacity is None:
            return _static_batch(features)
        if not fits:
            return False
        if self.capture_refused is None and getattr(self.store, "data_dependent", None):
            self.capture_refused = self.store.data_dependent
        from .feature_column import Ragged
        return self.capture_refused is None and all(isinstance(v, (torch.Tensor, Ragged)) for v in features.values())

    def _h2d(self, fill, shape, dtype, dst: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Host -> device through a small ring of PERSISTENT pinned staging buffers (one ring per dtype, buffers grow to
        the largest batch seen): `fill(view)` writes the batch into a view of a pinned buffer, the copy to the device is
        asynchronous.  (tensor.pin_memory() per batch allocates and frees page-locked memory every step — on this stack
        milliseconds per call, an order of magnitude more than the step; a pageable source makes the copy synchronous.)
        A buffer is reused only after the copy that read it last has completed (its event)."""
        shape = tuple(int(d) for d in shape)
        numel = 1
        for d in shape:
            numel *= d
        ring = self._pinned.get(dtype)
        if ring is None:
            ring = self._pinned[dtype] = {"bufs": [None] * self._STAGING_RING, "events": [None] * self._STAGING_RING, "i": 0}
        i = ring["i"]
        ring["i"] = (i + 1) % self._STAGING_RING
        if ring["events"][i] is not None:
            ring["events"][i].synchronize()
        buf = ring["bufs"][i]
        if buf is None or buf.numel() < numel:
            cap = 1 << max(int(numel - 1).bit_length(), 10)
            buf = ring["bufs"][i] = torch.empty(cap, dtype=dtype, pin_memory=True)
        view = buf[:numel].view(shape)
        fill(view)
        if dst is None:
            dev = view.to(self.device, non_blocking=True)
        else:                                # (an existing device buffer of this shape: no allocation, the same asynchronous copy)
            dev = dst
            dev.copy_(view, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        ring["events"][i] = ev
        return dev

    def _to_device(self, features, labels):
        from .feature_column import Ragged

        def mv(x):
            if isinstance(x, torch.Tensor):
                if x.device.type == "cpu" and self.device.type == "cuda" and x.numel() and not x.is_pinned():
                    return self._h2d(lambda buf: _host_copy(buf, x), x.shape, x.dtype)
                return x.to(self.device, non_blocking=True)
            if isinstance(x, Ragged):
                return Ragged(mv(x.values), mv(x.offsets))
            if isinstance(x, dict):
                return {k: mv(v) for k, v in x.items()}
            return x

        one = self._to_device_one_copy(features, labels)
        if one is not None:
            return one
        if isinstance(features, dict):
            features = self._pack_host_columns(features)
        return mv(features), mv(labels)

    def _to_device_one_copy(self, features, labels):
        """The batch of the native reader whose features are exactly the columns of ONE [B, F] id matrix (io/native.py
        PackedBatch) with [B, 1] float labels: matrix and labels go through ONE staging buffer and ONE host-to-device copy, and
        arrive as views of one device allocation (id matrix, then the labels) — the layout a captured step's input load moves
        with a single copy (GraphedTrainStep.load).  None: not that shape of batch."""
        pb = self._packed_host_batch(features, labels)
        if pb is None:
            return None
        mat, keys, labs, nid, total, sig, fill = pb
        B = mat.shape[0]
        dev = self._h2d(fill, (total,), torch.uint8)
        dmat = dev[:nid].view(torch.int64).view(mat.shape)
        feats = DeviceBatch()
        for j, k in enumerate(keys):
            feats[k] = dmat[:, j]
        out_l = {k: dev[nid + 4 * B * i:nid + 4 * B * (i + 1)].view(torch.float32).view(v.shape) for i, (k, v) in enumerate(labs)}
        feats.device_span = (dev, sig, (dict(feats), out_l))
        return feats, out_l

    def _packed_host_batch(self, features, labels):
        """-> (id matrix, keys, [(label key, tensor)], id bytes, total bytes, layout signature, fill(pinned uint8 view)) of a
        native-reader batch whose features are exactly the columns of ONE host [B, F] id matrix with [B, 1] float labels;
        None for any other batch."""
        packed = getattr(features, "packed_ids", None)
        if self.device.type != "cuda" or packed is None or not isinstance(labels, dict) or not labels:
            return None
        mat, keys = packed
        if len(keys) < 2 or set(features) != set(keys) or mat.dtype != torch.int64 or not mat.is_contiguous() or mat.device.type != "cpu":
            return None
        B = mat.shape[0]
        labs = list(labels.items())
        if not all(isinstance(v, torch.Tensor) and v.device.type == "cpu" and v.dtype == torch.float32 and v.numel() == B
                   for _, v in labs):
            return None
        nid = mat.numel() * 8
        total = nid + 4 * B * len(labs)
        sig = ("ids+labels", int(total), int(B), tuple(keys), tuple(k for k, _ in labs), tuple(tuple(v.shape) for _, v in labs))

        def fill(buf):
            _host_copy(buf[:nid].view(torch.int64).view(mat.shape), mat)
            for i, (_, v) in enumerate(labs):
                _host_copy(buf[nid + 4 * B * i:nid + 4 * B * (i + 1)].view(torch.float32), v.reshape(-1))
        return mat, keys, labs, nid, total, sig, fill

    def feed_step(self, graphed: "GraphedTrainStep", features, labels, pb=None):
        """One replay of a captured step on a HOST batch.  A native-reader batch with the layout the step was captured on goes
        from its pinned staging buffer STRAIGHT into the graph's static input span — one asynchronous copy; no intermediate
        device tensor, no per-column views, no device-to-device load (together they were 0.3 ms of host time per step, more
        than the GPU step).  Any other batch: `_to_device` + `graphed(features, labels)` as before."""
        plan = graphed._span_plan
        if plan is not None:
            pb = pb if pb is not None else self._packed_host_batch(features, labels)     # (the training loop passes its own)
            if pb is not None and pb[5] == plan[0] and plan[1].numel() == pb[4]:
                self._h2d(pb[6], (pb[4],), torch.uint8, dst=plan[1])
                graphed._feed = None             # (a load() left to the head would copy its batch over this one)
                return graphed()
        features, labels = self._to_device(features, labels)
        return graphed(features, labels)

    def _pack_host_columns(self, features: dict, force: bool = False) -> dict:
        """A decoded batch arrives as one host tensor per feature (26 id vectors + 16 dense columns for the
        WeChat-shaped data): moved one by one that is ~40 tiny host-to-device copies per step, more than the
        GPU step itself.  Host-resident single-valued id vectors ([B] int64) are packed into ONE [B, F] matrix
        (columns in sorted key order, the order fc.input_layer consumes them in) and the [B, 1] float columns
        into one [B, n] matrix; each is copied once and the features become column views of it — which is also
        the layout the gather kernels read in place (feature_column._as_matrix).  Device-resident inputs are
        left alone."""
        if self.device.type == "cpu" and not force:
            return features
        groups = {"ids": [], "dense": []}
        for k in sorted(features):
            v = features[k]
            if not isinstance(v, torch.Tensor) or v.device.type != "cpu":
                continue
            if v.dtype == torch.int64 and v.dim() == 1:
                groups["ids"].append(k)
            elif v.dtype == torch.float32 and v.dim() == 2 and v.shape[1] == 1:
                groups["dense"].append(k)
        out = dict(features)
        packed = getattr(features, "packed_ids", None)
        if packed is not None and len(packed[1]) >= 2 and packed[1] == groups["ids"] and all(
                features[k].data_ptr() == packed[0][:, j].data_ptr() and features[k].stride() == packed[0][:, j].stride()
                for j, k in enumerate(packed[1])):
            # the native reader already decoded the id features into ONE [B, F] matrix in this order (io/native.py
            # PackedBatch): one contiguous copy instead of re-stacking F strided column views
            mat = packed[0]
            dev = self._h2d(lambda buf: _host_copy(buf, mat), tuple(mat.shape), torch.int64) if self.device.type == "cuda" \
                else mat.to(self.device)
            for j, k in enumerate(packed[1]):
                out[k] = dev[:, j]
            groups["ids"] = []
        for kind, keys in groups.items():
            keys = [k for k in keys if features[k].shape[0] == features[keys[0]].shape[0]]
            if len(keys) < 2:
                continue
            cols_ = [features[k] for k in keys]
            B_ = cols_[0].shape[0]
            if self.device.type == "cuda":
                if kind == "ids":                                                          # [B, F]
                    dev = self._h2d(lambda buf: torch.stack(cols_, dim=1, out=buf), (B_, len(cols_)), torch.int64)
                else:                                                                      # [B, n]
                    dev = self._h2d(lambda buf: torch.cat(cols_, dim=1, out=buf), (B_, len(cols_)), torch.float32)
            else:
                host = torch.stack(cols_, dim=1) if kind == "ids" else torch.cat(cols_, dim=1)
                dev = host.to(self.device)
            for j, k in enumerate(keys):
                out[k] = dev[:, j] if kind == "ids" else dev[:, j:j + 1]
        return out

    def _call_model_fn(self, features, labels, mode) -> EstimatorSpec:
        with use_store(self.store):
            self.store.begin_call()
            self.store.call_features = features      # (model_tail reads the group ids of a per-group AUC from them)
            return self.model_fn(features, labels, mode, self.params)

    def _build(self, features, labels, mode):
        if self._built:
            return
        self.store.building = True
        with torch.no_grad():
            self._call_model_fn(features, labels, mode)
        self.store.finalize()
        self._built = True
        self._maybe_restore()
        for fn in self._after_build:
            fn()

    def build(self, features, labels=None, mode=ModeKeys.TRAIN):
        features, labels = self._to_device(features, labels)
        self._build(features, labels, mode)
        return self

    def train_step(self, features, labels):
        """One eager training step on device-resident inputs; returns the loss tensor."""
        from . import ops
        seed = 1.0 if self.loss_grad_scale is None else float(self.loss_grad_scale)
        with ops.loss_seed(seed):
            spec = self._call_model_fn(features, labels, ModeKeys.TRAIN)
        op = spec.train_op
        if self._seed_grad is None or float(self._seed_value) != seed or self._seed_grad.device != op.loss.device:
            self._seed_grad, self._seed_value = torch.full_like(op.loss.detach(), seed), seed   # made once, reused
        op.loss.backward(self._seed_grad)
        op.optimizer.apply_gradients(self.store, self.grad_hook)
        return spec.loss.detach()

    # -- public API -----------------------------------------------------------------------
    def train(self, input_fn, steps=None, max_steps=None, hooks=None, log_every=100):
        it = iter(input_fn())
        graphed = None
        t0 = time.time()
        n = 0
        while True:
            if max_steps is not None and self.global_step >= max_steps:
                break
            if steps is not None and n >= steps:
                break
            try:
                features, labels = next(it)
            except StopIteration:
                break
            loss = None
            pb = self._packed_host_batch(features, labels) if graphed is not None else None
            fits = True
            if pb is not None:
                host = (features, labels)
                try:
                    loss = self.feed_step(graphed, features, labels, pb)     # (host batch -> the graph's input span, one copy)
                    self.graph_replays += 1
                except BatchShapeMismatch:       # last partial batch: eager step
                    features, labels = self._to_device(*host)
                    loss = self.train_step(features, labels)
            else:
                # (ragged_capacity: every Ragged padded to its capacity, the eager warm-up steps included)
                features, fits = self._fit_ragged(features, warm=n < 2, loading=graphed is not None)
                features, labels = self._to_device(features, labels)
                self._build(features, labels, ModeKeys.TRAIN)
            # the first two steps run eagerly (they also warm the allocator and hipBLASLt);
            # from the third fixed-shape batch on, the step is one hipGraph replay
            if loss is not None:
                pass
            elif self.config.use_hip_graph and n >= 2 and self._capturable(features, fits):
                try:
                    if graphed is None:
                        graphed = GraphedTrainStep(self.train_step, features, labels, warmup=0)
                        graphed.pad_values = self.config.ragged_capacity is not None
                        self._ragged_frozen = True
                        loss = graphed()
                        if log_every and self._ragged_keys:
                            print(f"[recalgo] step {self.global_step + 1}: training step captured over ragged inputs of fixed "
                                  f"capacity ({', '.join(sorted(self._ragged_keys))})", flush=True)
                    else:
                        loss = graphed(features, labels)
                        self.graph_replays += 1
                except BatchShapeMismatch:       # last partial batch: eager step
                    loss = self.train_step(features, labels)
            else:
                loss = self.train_step(features, labels)
                if n % HOUSEKEEPING_EVERY == HOUSEKEEPING_EVERY - 1:
                    self.store.housekeeping()
            self.global_step += 1
            n += 1
            if log_every and self.global_step % log_every < 1:
                print(f"[recalgo] step {self.global_step} loss {float(loss):.6f} "
                      f"({n / max(time.time() - t0, 1e-9):.1f} steps/s)", flush=True)
            if self.global_step % OVERFLOW_POLL_EVERY == 0:
                self._check_exchange_overflow()
            sc = self.config.save_checkpoints_steps
            if sc and self.config.model_dir and self.global_step % sc == 0:
                self.save_checkpoint()
        self._check_exchange_overflow()
        if self.config.model_dir:
            self.save_checkpoint()
        return self

    @torch.no_grad()
    def evaluate(self, input_fn, steps=None) -> Dict[str, float]:
        """RunConfig(device_metrics=True) on a HIP device: metrics and loss are accumulated by one launch per batch and read
        once at the end (_evaluate_on_device); otherwise, and for a spec whose metrics that launch does not serve, the host
        loop over Metric.update()."""
        if getattr(self.config, "device_metrics", False) and self.device.type == "cuda":
            return self._evaluate_on_device(iter(input_fn()), steps)
        return self._evaluate_on_host(input_fn(), steps)

    def _evaluate_on_device(self, batches, steps) -> Dict[str, float]:
        """No host synchronisation inside the loop.  With config.use_hip_graph the EVAL step — model_fn under no_grad plus the
        metrics launch, one stream — is captured on the third fixed-shape batch and replayed from then on (GraphedTrainStep's
        static inputs and one-copy load); a batch of another shape (the last partial one) and, without config.ragged_capacity,
        every ragged batch run the same step eagerly into the same accumulator; with a capacity every Ragged is padded to it
        first (_fit_ragged) and only a batch that overflows runs eagerly.  The graph lives for this call only."""
        acc, graphed, n = None, None, 0

        def step(features, labels):
            spec = self._call_model_fn(features, labels, ModeKeys.EVAL)
            acc.add(spec)
            return spec.loss

        for i, (features, labels) in enumerate(batches):
            if steps is not None and i >= steps:
                break
            pb = self._packed_host_batch(features, labels) if graphed is not None else None
            fits = True
            if pb is not None:
                host = (features, labels)
                try:
                    self.feed_step(graphed, features, labels, pb)     # (host batch -> the graph's input span, one copy)
                    self.graph_replays += 1
                    n += 1
                    continue
                except BatchShapeMismatch:       # last partial batch: eager step
                    features, labels = self._to_device(*host)
            else:
                features, fits = self._fit_ragged(features, warm=n < 2, loading=graphed is not None)
                features, labels = self._to_device(features, labels)
                self._build(features, labels, ModeKeys.EVAL)
            if acc is None:
                spec = self._call_model_fn(features, labels, ModeKeys.EVAL)
                acc = EvalAccumulator.of(spec, self.device, getattr(self.config, "group_auc_capacity", GROUP_AUC_CAPACITY))
                if acc is None:                  # metrics the launch does not serve: the host loop, from this batch on
                    import itertools
                    return self._evaluate_on_host(itertools.chain([(features, labels)], batches), None if steps is None else steps - i)
                acc.add(spec)
            elif pb is None and self.config.use_hip_graph and n >= 2 and self._capturable(features, fits):
                try:
                    if graphed is None:
                        graphed = GraphedTrainStep(step, features, labels, warmup=0)
                        graphed.pad_values = self.config.ragged_capacity is not None
                        self._ragged_frozen = True
                        graphed()
                    else:
                        graphed(features, labels)
                        self.graph_replays += 1
                except BatchShapeMismatch:
                    step(features, labels)
            else:
                step(features, labels)
            n += 1
        del graphed
        if acc is None:
            return self._evaluate_on_host((), steps)
        agg, loss_sum, nb = acc.finish()
        out = {k: m.result() for k, m in agg.items()}
        out["loss"] = loss_sum / max(nb, 1)
        out["global_step"] = self.global_step
        return out

    def _evaluate_on_host(self, batches, steps) -> Dict[str, float]:
        agg: Dict[str, Metric] = {}
        loss_sum, nb = 0.0, 0
        for i, (features, labels) in enumerate(batches):
            if steps is not None and i >= steps:
                break
            features, labels = self._to_device(features, labels)
            self._build(features, labels, ModeKeys.EVAL)
            spec = self._call_model_fn(features, labels, ModeKeys.EVAL)
            for k, (m, _) in (spec.eval_metric_ops or {}).items():
                if k in agg:
                    agg[k].merge(m)
                else:
                    agg[k] = m
                agg[k].update()
            loss_sum += float(spec.loss)
            nb += 1
        out = {k: m.result() for k, m in agg.items()}
        out["loss"] = loss_sum / max(nb, 1)
        out["global_step"] = self.global_step
        return out

    @torch.no_grad()
    def predict(self, input_fn) -> Iterable[Dict[str, object]]:
        for features, labels in _with_labels(input_fn()):
            features, labels = self._to_device(features, labels)
            self._build(features, labels, ModeKeys.PREDICT)
            spec = self._call_model_fn(features, None, ModeKeys.PREDICT)
            preds = {k: v.detach().cpu().numpy() for k, v in spec.predictions.items()}
            B = len(next(iter(preds.values())))
            for b in range(B):
                yield {k: v[b] for k, v in preds.items()}

    # -- checkpoints (RunConfig(model_dir, save_checkpoints_steps)) -------------------------
    def _ckpt_path(self):
        return os.path.join(self.config.model_dir, "model.ckpt.pt")

    def save_checkpoint(self):
        """Every rank must call (collective when the arenas are row-sharded): the shards are gathered, rank 0 writes."""
        self._check_exchange_overflow()
        state, writer = collect_checkpoint_state(self.store, self.global_step)
        if writer:
            os.makedirs(self.config.model_dir, exist_ok=True)
            tmp = self._ckpt_path() + ".tmp"
            torch.save(state, tmp)
            os.replace(tmp, self._ckpt_path())
        sh = getattr(self, "shard_spec", None)
        if sh is not None and sh.world > 1:
            sh.dist.barrier(group=sh.group)            # nobody resumes from a half-written file

    # -- variables by their reference (TF) names --------------------------------
    # The mirror keeps every variable under the reference's TF name with the reference's shape, with one
    # exception: the (sum V, 1) first-order kernel of DeepFM / FwFM (`.../fm_first_order_dense/kernel`) is
    # stored as one slice per indicator column (`<kernel name>/<column key>`).  TF's input_layer lays the
    # indicator columns out sorted by column name (`<key>_indicator`), which fixes the row order.
    def _kernel_slices(self, arrays, name):
        subs = [k for k in arrays if k.startswith(name + "/")]
        return sorted(subs, key=lambda k: k[len(name) + 1:] + "_indicator")

    def export_variables(self) -> dict:
        """{reference TF variable name: numpy array} of the built model (per-column first-order slices are
        concatenated back into the reference's (sum V, 1) kernel)."""
        import numpy as np
        if not self._built:
            raise RuntimeError("export_variables: call build(features, labels) first")
        arrays = self.store.named_arrays()
        out, merged = {}, {}
        for k, v in arrays.items():
            base = k.rsplit("/", 1)[0]
            if base.endswith("/kernel") and base not in arrays:
                merged.setdefault(base, None)
            else:
                out[k] = v.detach().cpu().numpy().copy()
        for base in merged:
            out[base] = np.concatenate([arrays[k].detach().cpu().numpy() for k in self._kernel_slices(arrays, base)], 0)
        return out

    def load_variables(self, values, strict: bool = True):
        """Assign variables from {reference TF variable name: array} — e.g. the tensors of a TF-1.14
        checkpoint of the reference script dumped with `tf.train.load_checkpoint(dir).get_tensor(name)`
        (scripts/tf_ckpt_to_npz.py) — so that reference-trained weights run on these kernels.  Optimizer
        slots (`.../Adam`, `.../Adam_1`), `global_step` and `beta*_power` entries are ignored.  Returns the
        names assigned; with `strict`, a shape mismatch or a model variable without a value raises."""
        if not self._built:
            raise RuntimeError("load_variables: call build(features, labels) first")
        arrays = self.store.named_arrays()
        done = set()
        with torch.no_grad():
            for name, val in values.items():
                if name.endswith("/Adam") or name.endswith("/Adam_1") or name in ("global_step", "beta1_power", "beta2_power"):
                    continue
                if name.endswith("/Ftrl") or name.endswith("/Ftrl_1"):
                    # FTRL slots (TF's names): restored where the model has an FTRL-trained wide layer for them
                    from . import wide
                    for st in wide.states(self.store).values():
                        if name.rsplit("/", 1)[0] in [v.name for v in (st.kernel, st.bias) if v is not None]:
                            st.ensure_slots(0.1)
                            st.slots[name].copy_(torch.as_tensor(val).to(torch.float32).reshape(st.slots[name].shape))
                            st.ftrl_steps = max(st.ftrl_steps, 1)      # (slots of a trained model: the first-step zeroing is behind it)
                    continue
                t = torch.as_tensor(val).to(torch.float32)
                if name in arrays:
                    if tuple(arrays[name].shape) != tuple(t.shape):
                        if strict:
                            raise ValueError(f"load_variables: {name} has shape {tuple(t.shape)}, the model wants {tuple(arrays[name].shape)}")
                        continue
                    arrays[name].copy_(t)
                    done.add(name)
                    continue
                subs = self._kernel_slices(arrays, name)
                if subs and sum(arrays[k].shape[0] for k in subs) != t.shape[0]:
                    if strict:
                        raise ValueError(f"load_variables: {name} has {t.shape[0]} rows, the model's columns add up to "
                                         f"{sum(arrays[k].shape[0] for k in subs)}")
                    continue
                if subs:
                    row = 0
                    for k in subs:
                        n = arrays[k].shape[0]
                        arrays[k].copy_(t[row:row + n].reshape(arrays[k].shape))
                        row += n
                        done.add(k)
                elif strict and not name.endswith(("moving_mean", "moving_variance")):
                    raise KeyError(f"load_variables: the model has no variable {name}")
            blocks = {b for b, _ in self.store._alias.values()}     # fused blocks are covered by their named parts
            missing = [k for k in arrays if k not in done and k not in blocks]
            if strict and missing:
                raise KeyError(f"load_variables: no value for {missing[:5]}{' ...' if len(missing) > 5 else ''}")
        for a in self.store.arenas.values():
            a.live = None                    # liveness is rebuilt from the (unchanged) moments on next use
        return sorted(done)

    def load_tf_checkpoint(self, path: str, strict: bool = True):
        """Load the variables of a TensorFlow checkpoint written by the reference script — `path` is a model_dir (its
        `checkpoint` state file names the newest one) or a checkpoint prefix (`.../model.ckpt-10000`) — read natively
        (io/tf_checkpoint.py: no TensorFlow needed; format restated, see its header).  Returns the global step stored
        in the file (0 if none); optimizer slots are ignored, as in load_variables."""
        from .io import tf_checkpoint
        prefix = path
        if os.path.isdir(path):
            prefix = tf_checkpoint.latest_checkpoint(path)
            if prefix is None:
                raise FileNotFoundError(f"load_tf_checkpoint: no `checkpoint` state file in {path}")
        # optimizer slots (3x the embedding tables in host memory) are never read: load_variables ignores them anyway
        names = [n for n in tf_checkpoint.list_variables(prefix)
                 if not (n.endswith("/Adam") or n.endswith("/Adam_1") or n in ("beta1_power", "beta2_power"))]
        values = tf_checkpoint.read_checkpoint(prefix, names=names)
        self.load_variables(values, strict=strict)
        return int(values["global_step"]) if "global_step" in values else 0

    def save_tf_checkpoint(self, prefix: str) -> str:
        """Write the model's variables (reference names / shapes) + global_step as a TensorFlow V2 checkpoint
        (`<prefix>.index`, `<prefix>.data-00000-of-00001`, `checkpoint`): the hand-back to the reference's tooling."""
        import numpy as np
        from .io import tf_checkpoint
        arrays = dict(self.export_variables())
        from . import wide
        for st in wide.states(self.store).values():              # FTRL slots under TF's names: <var>/Ftrl, <var>/Ftrl_1
            for n, t in st.slots.items():
                arrays[n] = t.detach().cpu().numpy().copy()
        arrays["global_step"] = np.array(int(self.global_step), dtype=np.int64)
        tf_checkpoint.write_checkpoint(prefix, arrays)
        return prefix

    def _maybe_restore(self):
        md = self.config.model_dir
        if not md or not os.path.exists(self._ckpt_path()):
            return
        state = torch.load(self._ckpt_path(), map_location="cpu", weights_only=True)
        self.global_step = restore_checkpoint_state(self.store, state, self.device, where=self._ckpt_path())

    def _check_exchange_overflow(self):
        """Row-sharded arenas with the static (graph-capturable) exchange drop the requests that do not fit a bucket
        (the staged row reads as zeros, its gradient is discarded) and only raise a device flag: poll it."""
        if getattr(self, "shard_spec", None) is None:
            return
        from .parallel import exchange_overflowed
        if exchange_overflowed(self):
            raise RuntimeError(
                "row exchange bucket overflow: a (source, owner) bucket received more requests than its fixed capacity, "
                "so some embedding rows were read as zeros and their gradients dropped since the last check.  Re-attach "
                "with a larger capacity_factor (attach_data_parallel(..., capacity_factor=world) can never overflow) or "
                "with capacity_factor=None (exact, eager exchange).")


def collect_checkpoint_state(store: VariableStore, global_step: int):
    """-> (state dict, this rank writes it).  COLLECTIVE when arenas are row-sharded (parallel.attach_data_parallel): the
    weight / m / v shards are assembled into whole tables in the HOST memory of rank 0 only, through a bounded device
    window (parallel.gather_arena_to_host) — no rank ever holds a whole table on its GPU and the other ranks copy nothing
    to their hosts; the file is independent of the number of ranks (restore happens before re-sharding)."""
    from . import parallel, sparse
    sparse.sync_store(store)                                   # deferred Adam: every row reflects all completed steps
    sharded = {n: a for n, a in store.arenas.items() if getattr(a, "sharding", None) is not None}
    writer = all(a.sharding.sh.rank == 0 for a in sharded.values())
    variables = {n: v.data.detach().cpu() for n, v in store.vars.items()} if writer else {}
    arena_m, arena_v = {}, {}
    for n, a in store.arenas.items():
        if n in sharded:
            full = {what: parallel.gather_arena_to_host(a, what, 0) for what in ("weight", "m", "v")}
            if writer:
                for tn, (rb, vocab) in a.tables.items():
                    variables[tn] = a.shaped(tn, full["weight"][rb:rb + vocab])
                arena_m[n], arena_v[n] = full["m"], full["v"]
        else:
            if writer:
                for tn in a.tables:
                    variables[tn] = a.table_view(tn).detach().cpu()
                arena_m[n], arena_v[n] = a.m.cpu(), a.v.cpu()
    if not writer:
        return None, False
    state = {
        "global_step": int(global_step),
        "variables": variables,
        "flat_m": None if store.flat_m is None else store.flat_m.cpu(),
        "flat_v": None if store.flat_v is None else store.flat_v.cpu(),
        "arena_m": arena_m, "arena_v": arena_v,
        "opt_step": None if store.opt_state is None else int(store.opt_state["step"]),
    }
    from . import wide
    ftrl = {n: t.cpu() for st in wide.states(store).values() for n, t in st.slots.items()}
    if ftrl:                                 # FTRL slots under TF's names (<var>/Ftrl accum, <var>/Ftrl_1 linear)
        state["ftrl_slots"] = ftrl
        state["ftrl_steps"] = {k: st.ftrl_steps for k, st in wide.states(store).items()}
    return state, True


def _same_device(a, b) -> bool:
    """torch.device('cuda') and torch.device('cuda:0') name the same GPU when 0 is the current device."""
    a, b = torch.device(a), torch.device(b)
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return True
    cur = torch.cuda.current_device()
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


def restore_checkpoint_state(store: VariableStore, state: dict, device, where: str = "checkpoint") -> int:
    """Load `state` into a built store; returns the global step.  The file holds whole tables (it is independent of
    the number of ranks): a row-sharded arena takes its own rows r % world == rank from them.  A variable that is
    missing from the file or whose shape changed (another vocabulary, other hidden_units) makes the restore fail:
    resuming the step counter and Adam's bias correction on a partly re-initialised model is never what the caller
    wants."""
    saved = state["variables"]
    arrays = {n: v.data for n, v in store.vars.items()}
    table_shape = {}
    for a in store.arenas.values():
        for tn, (rb, vocab) in a.tables.items():
            table_shape[tn] = a.__dict__.get("view_shapes", {}).get(tn, (vocab, a.K))
    blocks = {b for b, _ in store._alias.values()}
    problems = []
    for k, shape in list((k, tuple(t.shape)) for k, t in arrays.items()) + list(table_shape.items()):
        if k in blocks:
            continue                                           # fused blocks are covered by their named parts
        if k not in saved:
            problems.append(f"{k}: not in the file")
        elif tuple(saved[k].shape) != tuple(shape):
            problems.append(f"{k}: file has {tuple(saved[k].shape)}, model wants {tuple(shape)}")
    for n, a in store.arenas.items():
        sd = getattr(a, "sharding", None)
        full = (sd.global_rows if sd is not None else a.m.shape[0], a.K)
        for slot in ("arena_m", "arena_v"):
            if n not in state.get(slot, {}) or tuple(state[slot][n].shape) != full:
                problems.append(f"{slot}[{n}]: missing or shape differs")
    if state.get("flat_m") is not None and store.flat_m is not None and state["flat_m"].shape != store.flat_m.shape:
        problems.append(f"dense Adam moments: file has {tuple(state['flat_m'].shape)}, model wants {tuple(store.flat_m.shape)}")
    if problems:
        raise RuntimeError(f"{where} does not match the model ({len(problems)} problem(s)): " + "; ".join(problems[:8])
                           + (" ..." if len(problems) > 8 else ""))
    unused = [k for k in saved if k not in arrays and k not in table_shape]
    if unused:
        import warnings
        warnings.warn(f"{where}: {len(unused)} saved variable(s) the model does not have were ignored: {unused[:5]}")
    with torch.no_grad():
        for k, t in arrays.items():
            if k not in blocks:
                t.copy_(saved[k])
        if state.get("flat_m") is not None and store.flat_m is not None:
            store.flat_m.copy_(state["flat_m"])
            store.flat_v.copy_(state["flat_v"])
        for n, a in store.arenas.items():
            sd = getattr(a, "sharding", None)
            rank, world = (0, 1) if sd is None else (sd.sh.rank, sd.sh.world)
            for tn, (rb, vocab) in a.tables.items():
                first = (rank - rb) % world                    # first row of the table this rank owns
                mine = saved[tn].reshape(vocab, a.K)[first::world]
                l0 = (rb + first) // world
                a.weight[l0:l0 + mine.shape[0]].copy_(mine)
            n_local = len(range(rank, state["arena_m"][n].shape[0], world))
            a.m[:n_local].copy_(state["arena_m"][n][rank::world])
            a.v[:n_local].copy_(state["arena_v"][n][rank::world])
            a.live = None            # rebuilt from the restored moments on next use
            from . import sparse
            sparse.reset(a)          # (deferred-Adam bookkeeping likewise)
    from . import wide
    for k, st in wide.states(store).items():
        saved_slots = state.get("ftrl_slots") or {}
        mine = [v.name + sfx for v in (st.kernel, st.bias) if v is not None for sfx in ("/Ftrl", "/Ftrl_1")]
        if all(n in saved_slots for n in mine):
            st.slots = {}
            st.ensure_slots(0.0)
            for n in mine:
                st.slots[n].copy_(saved_slots[n].reshape(st.slots[n].shape))
            st.ftrl_steps = int((state.get("ftrl_steps") or {}).get(k, 1))
    if state.get("opt_step") is not None:
        if store.opt_state is not None and _same_device(store.opt_state["step"].device, device):
            # in place: the captured step, and the arenas' deferred-Adam plans (sparse.sync_arena), hold THIS tensor
            store.opt_state["step"].fill_(int(state["opt_step"]))
        else:
            store.opt_state = {
                "step": torch.tensor([state["opt_step"]], dtype=torch.int64, device=device),
                "lr_t": torch.zeros(1, device=device)}
        from . import sparse
        for ar in store.arenas.values():       # (a plan made before the restore must not sync against a stale counter)
            plan = sparse.plan_of(ar)
            if plan is not None:
                plan.step_dev = store.opt_state["step"]
    return int(state["global_step"])


def _static_batch(features) -> bool:
    from .feature_column import Ragged
    return all(isinstance(v, torch.Tensor) for v in features.values()) and \
        not any(isinstance(v, Ragged) for v in features.values())


def _with_labels(it):
    for item in it:
        if isinstance(item, tuple) and len(item) == 2:
            yield item
        else:
            yield item, None


def train_and_evaluate(estimator: Estimator, train_spec: TrainSpec, eval_spec: EvalSpec):
    """tf.estimator.train_and_evaluate (deepfm.py:323): train to max_steps, evaluate, then hand the evaluation result to
    the EvalSpec's exporters (deepfm.py:309-321: BestExporter -> <model_dir>/export/<name>/<timestamp>)."""
    estimator.train(train_spec.input_fn, max_steps=train_spec.max_steps)
    result = estimator.evaluate(eval_spec.input_fn, steps=eval_spec.steps)
    exporters = eval_spec.exporters or []
    if not isinstance(exporters, (list, tuple)):
        exporters = [exporters]
    base = estimator.config.model_dir
    for ex in exporters:
        if base is None:
            raise ValueError("train_and_evaluate: exporters need RunConfig(model_dir=...)")
        ex.export(estimator, os.path.join(base, "export", ex.name), estimator._ckpt_path(), result, True)
    return result
