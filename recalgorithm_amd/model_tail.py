"""The prediction / loss / metric / train_op tail every reference model_fn repeats
(e.g. /root/reference algorithm/DeepFM/deepfm.py:214-273): sigmoid, mean sigmoid-CE
(fused HIP kernel, a14), tf.metrics accuracy@0.5 + 200-bucket AUC, Adam(lr, .9, .999, 1e-8); on request
(params["group_auc_key"], not a reference parameter) the per-user AUC of the evaluation beside them."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from . import ops
from .estimator import AdamOptimizer, EstimatorSpec, LazyAdamOptimizer, ModeKeys, metrics
from .variables import current_store


def sigmoid(logit: torch.Tensor) -> torch.Tensor:
    return torch.sigmoid(logit)


def group_auc_metric_ops(params, tasks) -> Dict[str, tuple]:
    """params["group_auc_key"] names the categorical feature whose encoded ids group the rows of a per-group AUC (the user id),
    params["group_auc_groups"] is its vocabulary size and params.get("group_auc_weighting") "uniform" (uAUC, the default) or
    "samples" (GAUC).  tasks: [(task name or None, labels, probabilities)] -> {"eval_[<task>_]uauc" | "eval_[<task>_]gauc":
    metrics.group_auc(..)}, every one over the same tensor of ids, as the model_fn received them (int64 [B] or [B, 1], an id < 0
    for out-of-vocabulary); {} without the key."""
    key = params.get("group_auc_key")
    if not key:
        return {}
    from .feature_column import Ragged
    weighting = params.get("group_auc_weighting") or "uniform"
    features = current_store().call_features
    if not isinstance(features, dict) or key not in features:
        raise ValueError(f"params['group_auc_key'] = {key!r}: the model_fn's features hold no such key")
    groups = features[key]
    if isinstance(groups, Ragged):
        raise ValueError(f"params['group_auc_key'] = {key!r}: a Ragged (a bag or a history) does not give each row one group")
    if not isinstance(groups, torch.Tensor) or groups.dtype != torch.int64 or groups.dim() > 2 or (groups.dim() == 2 and groups.shape[1] != 1):
        raise ValueError(f"params['group_auc_key'] = {key!r}: expected the feature's encoded ids, an int64 [B] or [B, 1] tensor")
    num_groups = params.get("group_auc_groups")
    if not (isinstance(num_groups, int) and not isinstance(num_groups, bool) and num_groups >= 1):
        raise ValueError(f"params['group_auc_groups'] = {num_groups!r}: expected the vocabulary size of {key!r}, an int >= 1")
    suffix = "gauc" if weighting == "samples" else "uauc"
    return {f"eval_{suffix}" if name is None else f"eval_{name}_{suffix}":
            metrics.group_auc(labels=y, predictions=p, groups=groups, num_groups=num_groups, weighting=weighting)
            for name, y, p in tasks}


def finish_model_fn(mode, logit: torch.Tensor, labels, params,
                    predictions: Optional[Callable[[torch.Tensor], Dict[str, torch.Tensor]]] = None,
                    extra_loss: Optional[Callable[[], torch.Tensor]] = None,
                    label_key: str = "read_comment",
                    train_op: Optional[Callable[[torch.Tensor], object]] = None) -> EstimatorSpec:
    """`train_op` (a model that trains with its own optimizers, wide_and_deep.py:251-276): loss -> the train op; default:
    Adam(params["learning_rate"]) on every variable."""
    from .nn import LazyLogit
    lazy = logit if isinstance(logit, LazyLogit) else None
    extra = None
    tail = lazy.tail() if (lazy is not None and mode == ModeKeys.TRAIN and not current_store().building) else None
    if tail is not None and extra_loss is not None:
        extra = extra_loss()
        if extra is not None and extra.requires_grad:
            tail = None
    if lazy is not None and tail is None:
        ok = mode == ModeKeys.TRAIN and lazy.fusable() and not current_store().building
        if ok and extra_loss is not None:
            # the fused tail delivers the loss VALUE through the step's deferred sums: an extra term can only join it as
            # a detached addend (DIN's regulariser value; its gradient rides on the first fcn layer)
            extra = extra_loss() if extra is None else extra
            ok = extra is None or not extra.requires_grad
        if not ok:
            logit, lazy = lazy.materialize(), None
    if mode == ModeKeys.PREDICT:
        prob = torch.sigmoid(logit)
        preds = predictions(prob) if predictions else {"probabilities": prob}
        return EstimatorSpec(mode, predictions=preds, export_outputs={"prediction": preds})

    y = labels[label_key]
    if tail is not None:
        # one launch: the last hidden layer + the one-unit head over [side, layer] + sigmoid-CE + the backward of all of it
        side, ld, side_first = tail
        head_kernel, head_bias, _ = lazy.heads[0]
        loss, prob, logit = ops.tail_dense_head(current_store(), y, head_kernel, head_bias, ld.kernel, ld.bias, ld.x, side,
                                                side_first, loss_addend=extra)
    elif lazy is not None:
        # one launch: one-unit head(s) + sigmoid-CE + the backward of both (the loss-gradient seed is known)
        heads = [(k, len(ps)) for k, _, ps in lazy.heads]
        bias = next((b for _, b, _ in lazy.heads if b is not None), None)
        parts = [t for _, _, ps in lazy.heads for t in ps]
        loss, prob, logit = ops.logit_loss(current_store(), y, heads, bias, parts, lazy.tensors, loss_addend=extra)
    elif current_store().building:          # variable-registration pass: nothing is launched
        loss, prob = logit.new_zeros(()), torch.zeros_like(logit)
    else:
        loss, prob = ops.sigmoid_cross_entropy(logit, y)
    if extra_loss is not None and lazy is None:
        if extra is None:
            extra = extra_loss()
        if extra is not None:
            loss = loss + extra
    if mode == ModeKeys.EVAL:
        acc = metrics.accuracy(labels=y, predictions=(prob >= 0.5).to(torch.float32))
        auc = metrics.auc(labels=y, predictions=prob)
        return EstimatorSpec(mode, loss=loss, eval_metric_ops={"eval_accuracy": acc, "eval_auc": auc,
                                                               **group_auc_metric_ops(params, [(None, y, prob)])})

    # TRAIN: the reference also builds the two metric ops here, but only to feed tf.summary /
    # LoggingTensorHook (deepfm.py:237-238,256-271); they are not part of the training step
    assert mode == ModeKeys.TRAIN
    if train_op is not None:
        return EstimatorSpec(mode, loss=loss, train_op=train_op(loss), predictions={"probabilities": prob})
    opt_cls = LazyAdamOptimizer if params.get("lazy_adam") else AdamOptimizer      # lazy_adam: labelled deviation (§8f-1)
    optimizer = opt_cls(learning_rate=params["learning_rate"], beta1=0.9, beta2=0.999, epsilon=1e-8)
    train_op = optimizer.minimize(loss=loss)
    return EstimatorSpec(mode, loss=loss, train_op=train_op, predictions={"probabilities": prob})


def finish_multitask_model_fn(mode, logits: Dict[str, torch.Tensor], labels, params) -> EstimatorSpec:
    """The tail of a multi-task model_fn (/root/reference algorithm/MMOE/mmoe.py:234-262): `logits` maps task name -> [B, 1]
    logit, in task order.  PREDICT: {"<task>_probabilities"}; EVAL: the summed loss and eval_<task>_accuracy / eval_<task>_auc;
    TRAIN: Adam on the sum of the tasks' mean sigmoid-CE (one loss launch: ops.multitask_sigmoid_cross_entropy).
    The single-logit fused tails (LazyLogit, ops.tail_dense_head, the riders) hold ONE head per step — one rider slot, one
    `_dlogit_partials` entry — so every tower logit is evaluated by its own head kernel (LazyLogit.materialize) here."""
    from .nn import LazyLogit
    names = list(logits)
    ts = [t.materialize() if isinstance(t, LazyLogit) else t for t in logits.values()]
    if mode == ModeKeys.PREDICT:
        preds = {f"{n}_probabilities": torch.sigmoid(t) for n, t in zip(names, ts)}
        return EstimatorSpec(mode, predictions=preds, export_outputs={"prediction": preds})

    ys = [labels[n] for n in names]
    if current_store().building:            # variable-registration pass: nothing is launched
        loss, probs = ts[0].new_zeros(()), [torch.zeros_like(t) for t in ts]
    else:
        loss, _, prob = ops.multitask_sigmoid_cross_entropy(ts, ys)
        probs = [prob[:, i:i + 1] for i in range(len(names))]
    if mode == ModeKeys.EVAL:
        acc = {f"eval_{n}_accuracy": metrics.accuracy(labels=y, predictions=(p >= 0.5).to(torch.float32))
               for n, y, p in zip(names, ys, probs)}
        auc = {f"eval_{n}_auc": metrics.auc(labels=y, predictions=p) for n, y, p in zip(names, ys, probs)}
        return EstimatorSpec(mode, loss=loss, eval_metric_ops={**acc, **auc, **group_auc_metric_ops(params, list(zip(names, ys, probs)))})

    assert mode == ModeKeys.TRAIN
    opt_cls = LazyAdamOptimizer if params.get("lazy_adam") else AdamOptimizer      # lazy_adam: labelled deviation (§8f-1)
    optimizer = opt_cls(learning_rate=params["learning_rate"], beta1=0.9, beta2=0.999, epsilon=1e-8)
    train_op = optimizer.minimize(loss=loss)
    return EstimatorSpec(mode, loss=loss, train_op=train_op,
                         predictions={f"{n}_probabilities": p for n, p in zip(names, probs)})


def finish_esmm_model_fn(mode, ctr_logit: torch.Tensor, cvr_logit: torch.Tensor, labels, params) -> EstimatorSpec:
    """The tail of ESMM (Ma et al., SIGIR 2018; no reference file): two [B, 1] logits over ALL impressions, the click label
    labels[params["ctr_task_name"]] and the conversion label labels[params["cvr_task_name"]].
    PREDICT: {"ctr_probabilities", "cvr_probabilities", "ctcvr_probabilities"} (pCTR, pCVR, their product).
    EVAL: loss = L_ctr + L_ctcvr; eval_ctr_{auc, accuracy} against the click, eval_ctcvr_{auc, accuracy} against click *
    conversion, and eval_cvr_{auc, accuracy}: the conversion against pCVR over the CLICKED impressions only (mask = the click:
    the space the CVR tower is defined on); with params["group_auc_key"] the per-user AUC of ctr and ctcvr.
    TRAIN: Adam on the total — one loss launch for both terms and both logit gradients (ops.esmm_loss).
    As in the multi-task tail, every tower logit is evaluated by its own head kernel (LazyLogit.materialize)."""
    from .nn import LazyLogit
    a, b = (t.materialize() if isinstance(t, LazyLogit) else t for t in (ctr_logit, cvr_logit))
    names = ("ctr_probabilities", "cvr_probabilities", "ctcvr_probabilities")
    if mode == ModeKeys.PREDICT:
        p_ctr, p_cvr = torch.sigmoid(a), torch.sigmoid(b)
        preds = dict(zip(names, (p_ctr, p_cvr, p_ctr * p_cvr)))
        return EstimatorSpec(mode, predictions=preds, export_outputs={"prediction": preds})

    y, c = labels[params["ctr_task_name"]], labels[params["cvr_task_name"]]
    if current_store().building:            # variable-registration pass: nothing is launched
        loss, probs = a.new_zeros(()), [torch.zeros_like(a) for _ in names]
    else:
        loss, _, prob = ops.esmm_loss(a, b, y, c)
        probs = [prob[:, i:i + 1] for i in range(3)]
    if mode == ModeKeys.EVAL:
        y = y.to(torch.float32).reshape(-1, 1)
        c = c.to(torch.float32).reshape(-1, 1)
        tasks = [("ctr", y, probs[0], None), ("ctcvr", y * c, probs[2], None), ("cvr", c, probs[1], y)]
        metric_ops = {}
        for n, lab, p, mask in tasks:
            metric_ops[f"eval_{n}_auc"] = metrics.auc(labels=lab, predictions=p, mask=mask)
            metric_ops[f"eval_{n}_accuracy"] = metrics.accuracy(labels=lab, predictions=(p >= 0.5).to(torch.float32), mask=mask)
        return EstimatorSpec(mode, loss=loss, eval_metric_ops={
            **metric_ops, **group_auc_metric_ops(params, [(n, lab, p) for n, lab, p, mask in tasks if mask is None])})

    assert mode == ModeKeys.TRAIN
    opt_cls = LazyAdamOptimizer if params.get("lazy_adam") else AdamOptimizer      # lazy_adam: labelled deviation (§8f-1)
    optimizer = opt_cls(learning_rate=params["learning_rate"], beta1=0.9, beta2=0.999, epsilon=1e-8)
    train_op = optimizer.minimize(loss=loss)
    return EstimatorSpec(mode, loss=loss, train_op=train_op, predictions=dict(zip(names, probs)))
