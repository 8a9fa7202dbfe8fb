"""Torch restatement of the reference's PLE forward (algorithm/PLE/ple.py:147-254, extraction_network.py:4-85,
MMOE/tower_layer.py:19-28) for (variables by TF name, encoded features, labels, params), built on tests/mmoe_ref.gate_mix and
oracle/ref_ops / ref_models — it lives here because oracle/ is frozen.  TEST INFRASTRUCTURE ONLY: the product path never
imports it.  Run in float64 it is the reference the GPU tests compare against (pinned to the goldens by
tests/test_ple_host.py); run in float32 it is their `ref32` guard.

Also `cgc`: the CGC block alone (gates + mix with a selection table, optionally summed), the reference of ops.cgc_mix."""
import torch

from oracle import ref_models as M
from oracle import ref_ops as R
from tests import mmoe_ref


def cgc(x, ws, experts, selection, sum_outputs=False):
    """-> (outs, [p_g]): outs the per-gate mixes [B, H], or with sum_outputs their tf.add_n (left to right) as ONE tensor."""
    outs, ps = mmoe_ref.gate_mix(x, ws, experts, selection)
    if sum_outputs:
        total = outs[0]
        for o in outs[1:]:
            total = total + o
        return total, ps
    return outs, ps


def ple_selection(per_task, n_shared, all_gate=False):
    """experts numbered [task 0's.., task 1's.., .., shared..]; gate t over [its task's.., shared..]; the all-gate over all"""
    starts, at = [], 0
    for n in per_task:
        starts.append(at)
        at += n
    shared = list(range(at, at + n_shared))
    sel = [list(range(s, s + n)) + shared for s, n in zip(starts, per_task)]
    return sel + [list(range(at + n_shared))] if all_gate else sel


def _experts(P, x, scope, fmt_task, fmt_shared, tasks, per_task, n_shared):
    names = [fmt_task.format(task=t, j=j) for t, n in zip(tasks, per_task) for j in range(n)]
    names += [fmt_shared.format(j=j) for j in range(n_shared)]
    return [R.dense(x, P[f"{scope}{n}/kernel"], P[f"{scope}{n}/bias"], relu=True) for n in names]


def extraction_network(P, x, tasks, per_task, n_shared, name):
    """extraction_network.py:25-85"""
    experts = _experts(P, x, f"{name}/", "task_specific_expert_{task}_{j}", "shared_expert_{j}", tasks, per_task, n_shared)
    ws = [P[f"{name}/gate_{t}/kernel"] for t in tasks] + [P[f"{name}/all_gate/kernel"]]
    out, ps = cgc(x, ws, experts, ple_selection(per_task, n_shared, all_gate=True), sum_outputs=True)
    return out, ps, experts


def ple(P, feats, labels, params, training=False, dropout_masks=None):
    """-> {"logits", "probs", "gates" (per block), "experts" (per block: the ReLU outputs), and with labels "losses", "loss"}."""
    masks = list(dropout_masks or [])
    dense_in = M.input_layer(P, feats, params["dense_feature_columns"], "dense_input/input_layer")
    cat = M.input_layer(P, feats, params["category_feature_columns"], "category_input/input_layer", {})
    x = torch.cat([dense_in, cat], dim=-1)                                          # ple.py:169
    tasks = list(params["task_names"])
    per_task, n_shared = [int(n) for n in params["num_experts_per_task"]], int(params["num_experts_in_shared"])
    gates, experts_seen = [], []
    for i in range(int(params["num_extract_network"])):                             # :173-180
        x, ps, ex = extraction_network(P, x, tasks, per_task, n_shared, f"extract_network_{i}")
        gates.append(ps)
        experts_seen.append(ex)
    ex = _experts(P, x, "", "task_specific_experts_final/task_specific_expert_final_{task}_{j}",
                  "shared_experts_final/shared_expert_final_{j}", tasks, per_task, n_shared)        # :185-210
    ws = [P[f"task_specific_experts_final/task_gate_final/gate_final_{t}/kernel"] for t in tasks]
    towers, ps = cgc(x, ws, ex, ple_selection(per_task, n_shared))                  # :213-226
    gates.append(ps)
    experts_seen.append(ex)
    n_hidden, k = len(params["hidden_units"]), 0
    logits = {}
    for tower, task in zip(towers, tasks):                                          # :229-235: one `tower` scope, auto names run on
        net = tower
        for _ in range(n_hidden):
            dn = "dense" if k == 0 else f"dense_{k}"
            bn = "batch_normalization" if k == 0 else f"batch_normalization_{k}"
            net = R.dense(net, P[f"tower/{dn}/kernel"], P[f"tower/{dn}/bias"], relu=True)
            net = M._dropout(net, params, training, masks)
            if params.get("batch_norm"):
                net = R.batch_norm(net, P[f"tower/{bn}/gamma"], P[f"tower/{bn}/beta"], P[f"tower/{bn}/moving_mean"],
                                   P[f"tower/{bn}/moving_variance"], training)
            k += 1
        logits[task] = R.dense(net, P[f"tower/tower_{task}_logit/kernel"], P[f"tower/tower_{task}_logit/bias"])
    out = {"logits": logits, "probs": {t: torch.sigmoid(v) for t, v in logits.items()}, "gates": gates, "experts": experts_seen}
    if labels is not None:
        out["losses"] = {t: R.ce_loss(labels[t], v) for t, v in logits.items()}     # :251-253
        total = None
        for v in out["losses"].values():                                            # tf.add_n, :254
            total = v if total is None else total + v
        out["loss"] = total
    return out
