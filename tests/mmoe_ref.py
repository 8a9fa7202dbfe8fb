"""Torch restatement of the reference's MMoE forward (algorithm/MMOE/mmoe.py:183-249, tower_layer.py:19-28) for
(variables by TF name, encoded features, labels, params), in the style of oracle/ref_models.py — it lives here because
oracle/ is frozen.  TEST INFRASTRUCTURE ONLY: the product path never imports it.  Run in float64 it is the reference the
GPU tests compare against (pinned to the goldens by tests/test_mmoe_host.py); run in float32 it is their `ref32` guard.

Also `gate_mix`: the MMoE / CGC block alone (gates + mix with a selection table), the reference of ops.gate_mix."""
import torch

from oracle import ref_models as M
from oracle import ref_ops as R


def gate_mix(x, gate_kernels, experts, selection=None):
    """mmoe.py:208-232 with a selection table: gate g = softmax(x @ Wg) over the experts selection[g] (default: all).
    -> ([out_g [B, H]], [p_g [B, n_g]])"""
    E = len(experts)
    selection = [list(range(E)) for _ in gate_kernels] if selection is None else selection
    outs, ps = [], []
    for w, sel in zip(gate_kernels, selection):
        p = torch.softmax(x @ w, dim=-1)                                            # :209-213 (bias-free, softmax activation)
        stack = torch.stack([experts[e] for e in sel], dim=1)                       # :204-205  (B, n_g, H)
        outs.append(torch.matmul(stack.transpose(1, 2), p.unsqueeze(-1)).squeeze(-1))      # :221-225
        ps.append(p)
    return outs, ps


def mmoe(P, feats, labels, params, training=False, dropout_masks=None):
    """-> {"logits": {task: [B, 1]}, "probs": {task: [B, 1]}, "gates": [p_g], and with labels "losses": {task: scalar},
    "loss": their sum}.  Tower order dense(relu) -> dropout -> BN (tower_layer.py:20-24); batch statistics when `training`;
    training-mode dropout takes its keep masks from `dropout_masks` (call order)."""
    masks = list(dropout_masks or [])
    dense_in = M.input_layer(P, feats, params["dense_feature_columns"], "dense_input/input_layer")
    cat = M.input_layer(P, feats, params["category_feature_columns"], "category_input/input_layer", {})
    x = torch.cat([dense_in, cat], dim=-1)                                          # :195
    experts = [R.dense(x, P[f"experts/expert_{i}/kernel"], P[f"experts/expert_{i}/bias"], relu=True)
               for i in range(int(params["num_experts"]))]                          # :199-202
    towers, gates = gate_mix(x, [P[f"gates/gate_{i}/kernel"] for i in range(int(params["num_tasks"]))], experts)
    n_hidden, k = len(params["hidden_units"]), 0
    logits = {}
    for tower, task in zip(towers, params["task_names"]):                           # :230-235: one `tower` scope, auto names run on
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
    out = {"logits": logits, "probs": {t: torch.sigmoid(v) for t, v in logits.items()}, "gates": gates}
    if labels is not None:
        out["losses"] = {t: R.ce_loss(labels[t], v) for t, v in logits.items()}     # :247-248
        total = None
        for v in out["losses"].values():                                            # tf.add_n, :249
            total = v if total is None else total + v
        out["loss"] = total
    return out
