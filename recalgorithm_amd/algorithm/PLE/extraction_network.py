"""PLE's extraction network — MI355X drop-in for the reference's algorithm/PLE/extraction_network.py: same signature,
same variables (`<name>/shared_expert_<j>`, `<name>/task_specific_expert_<task>_<j>`, `<name>/gate_<task>`,
`<name>/all_gate`), same value: tf.add_n of the task outputs and the all-gate output, ONE [B, expert_hidden_units] tensor
(extraction_network.py:85 — a reference quirk, reproduced).

All the experts of the block are one `nn.expert_layers` call (one autograd node: E GEMM launches each way, the input
gradients chained through beta * C), the T + 1 gates, their softmax, the mixes and the sum are one kernel each way
(nn.cgc_layer -> ops.cgc_mix, csrc/cgc.hip)."""
from __future__ import annotations

from ... import nn
from ...variables import variable_scope


def expert_order(num_experts_per_task, num_experts_in_shared):
    """The block's expert numbering: [task 0's.., task 1's.., .., shared..] (the column order of `all_gate`,
    extraction_network.py:49,69-70).  -> (first index of each task's experts, indices of the shared experts)"""
    starts, at = [], 0
    for n in num_experts_per_task:
        starts.append(at)
        at += int(n)
    return starts, list(range(at, at + int(num_experts_in_shared)))


def task_selection(num_experts_per_task, num_experts_in_shared):
    """Gate t mixes [its task's experts.., the shared experts..] (extraction_network.py:51, ple.py:213)."""
    starts, shared = expert_order(num_experts_per_task, num_experts_in_shared)
    return [list(range(s, s + int(n))) + shared for s, n in zip(starts, num_experts_per_task)]


def extraction_network(input, task_names, num_experts_per_task, num_experts_in_shared, expert_hidden_units, name):
    """-> (B, expert_hidden_units); extraction_network.py:4-85."""
    num_experts_per_task = [int(n) for n in num_experts_per_task]
    names = [f"task_specific_expert_{task}_{j}" for task, n in zip(task_names, num_experts_per_task) for j in range(n)]
    names += [f"shared_expert_{j}" for j in range(int(num_experts_in_shared))]
    selection = task_selection(num_experts_per_task, num_experts_in_shared) + [list(range(len(names)))]
    chain = nn.InputGradChain()
    with variable_scope(name):
        experts = nn.expert_layers(input, expert_hidden_units, len(names), chain=chain, names=names)
        return nn.cgc_layer(input, experts, [f"gate_{task}" for task in task_names] + ["all_gate"], selection,
                            sum_outputs=True, chain=chain)
