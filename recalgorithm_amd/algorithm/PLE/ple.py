"""PLE (Tang et al., RecSys 2020) entry point — MI355X drop-in for the reference's algorithm/PLE/ple.py: same flags
(`num_extract_network`, `num_experts_per_task`, `num_experts_in_shared`, `expert_hidden_units`, `num_tasks`, `task_names`
included), `create_feature_columns`, `example_parser` (a label dict with one key per task),
`ple_model_fn(features, labels, mode, params)`, `main`, same variable scopes (`extract_network_<i>/...`,
`shared_experts_final/shared_expert_final_<j>`, `task_specific_experts_final/task_specific_expert_final_<task>_<j>`,
`task_specific_experts_final/task_gate_final/gate_final_<task>`, `tower/...` as MMoE) and prediction keys.

Every CGC block — an extraction network, or the final one in front of the towers — is E expert GEMM launches over the
block's input plus ONE gate-softmax-mix kernel each way (ops.cgc_mix, csrc/cgc.hip); the towers and the T-task loss tail
are MMoE's.

    python -m recalgorithm_amd.algorithm.PLE.ple --task_names=read_comment,like,click_avatar --batch_size=4096
"""
from __future__ import annotations

from typing import Tuple

import torch

from ... import feature_column as fc
from ... import flags, nn
from ...model_tail import finish_multitask_model_fn
from ...variables import variable_scope
from .. import _common as common
from ..MMOE.tower_layer import tower_layer
from ..utils import parse_example
from .extraction_network import extraction_network, task_selection

# flags: the reference's algorithm/PLE/ple.py:21-50
common.define_common_flags(batch_size=1024, learning_rate=0.005)
flags.DEFINE_string("hidden_units", "512,256,128",
                    "Comma-separated list of number of units in each hidden layer of the final output part")
flags.DEFINE_boolean("batch_norm", True, "Perform batch normalization (True or False)")
flags.DEFINE_float("dropout_rate", 0.1, "Dropout rate")
flags.DEFINE_integer("num_extract_network", 1, "Numbers of extract network be stacked")
flags.DEFINE_string("num_experts_per_task", "5,5,5", "Comma-separated list of number of experts per task")
flags.DEFINE_integer("num_experts_in_shared", 10, "Number of shared experts")
flags.DEFINE_integer("expert_hidden_units", 256, "All experts output dimension either in CGC or in extraction network")
flags.DEFINE_integer("num_tasks", 3, "Number of tasks, that's number of gates")
flags.DEFINE_string("task_names", "read_comment,like,click_avatar",
                    "Comma-separated list of task names, each must be in keys of tfrecord file")
FLAGS = flags.FLAGS


def create_feature_columns() -> Tuple[list, list, list]:
    """-> (dense_feature_columns, category_feature_columns, label_feature_columns); ple.py:56-126 (the columns of MMoE,
    one numeric label column per task name)."""
    cols, feedid_emb = common.wechat_category_columns(
        {"userid": 16, "device": 2, "authorid": 4, "bgm_song_id": 4, "bgm_singer_id": 4, "manual_tag_list": 4, "feedid": 16})
    label_cols = [fc.numeric_column(task_name, default_value=0.0) for task_name in FLAGS.task_names.split(",")]
    return common.dense_columns(), cols + feedid_emb, label_cols


total_feature_columns: list = []
label_feature_columns: list = []


def example_parser(serialized_example):
    """Batch of serialized tf.train.Example -> (features, {task_name: (B, 1)}); ple.py:129-144."""
    spec = fc.make_parse_example_spec(total_feature_columns + label_feature_columns)
    features = parse_example(serialized_example, spec)
    labels = {task_name: features.pop(task_name) for task_name in FLAGS.task_names.split(",")}
    return features, labels


example_parser.columns_getter = lambda: (total_feature_columns, label_feature_columns)     # (the native decoder: utils.py)


def ple_model_fn(features, labels, mode, params):
    """ple.py:147-307."""
    with variable_scope("dense_input"):
        dense_input = fc.input_layer(features, params["dense_feature_columns"])
    with variable_scope("category_input"):
        category_input = fc.input_layer(features, params["category_feature_columns"])
    input = torch.cat([dense_input, category_input], dim=-1)
    task_names = list(params["task_names"])
    per_task = [int(n) for n in params["num_experts_per_task"]]
    n_shared = int(params["num_experts_in_shared"])

    for i in range(int(params["num_extract_network"])):                  # ple.py:173-180: a level hands ONE tensor on
        input = extraction_network(input=input, task_names=task_names, num_experts_per_task=per_task,
                                   num_experts_in_shared=n_shared, expert_hidden_units=params["expert_hidden_units"],
                                   name=f"extract_network_{i}")

    # the final CGC in front of the towers (ple.py:185-226): the same block without an all-gate and without the sum
    names = [f"task_specific_experts_final/task_specific_expert_final_{task}_{j}"
             for task, n in zip(task_names, per_task) for j in range(n)]
    names += [f"shared_experts_final/shared_expert_final_{j}" for j in range(n_shared)]
    chain = nn.InputGradChain()
    experts = nn.expert_layers(input, params["expert_hidden_units"], len(names), chain=chain, names=names)
    with variable_scope("task_specific_experts_final"):
        towers = nn.cgc_layer(input, experts, [f"task_gate_final/gate_final_{task}" for task in task_names],
                              task_selection(per_task, n_shared), chain=chain)

    with variable_scope("tower"):
        logits = {task_name: tower_layer(x, params["hidden_units"], mode, params["batch_norm"], params["dropout_rate"],
                                         task_name) for x, task_name in zip(towers, task_names)}
    return finish_multitask_model_fn(mode, logits, labels, params)


def main(unused_argv):
    global total_feature_columns, label_feature_columns
    dense_cols, category_cols, label_feature_columns = create_feature_columns()
    total_feature_columns = dense_cols + category_cols
    params = {
        "dense_feature_columns": dense_cols,
        "category_feature_columns": category_cols,
        "hidden_units": FLAGS.hidden_units.split(","),
        "dropout_rate": FLAGS.dropout_rate,
        "batch_norm": FLAGS.batch_norm,
        "learning_rate": FLAGS.learning_rate,
        "num_tasks": FLAGS.num_tasks,
        "expert_hidden_units": FLAGS.expert_hidden_units,
        "task_names": FLAGS.task_names.split(","),
        "num_extract_network": FLAGS.num_extract_network,
        "num_experts_per_task": [int(x) for x in FLAGS.num_experts_per_task.split(",")],
        "num_experts_in_shared": FLAGS.num_experts_in_shared,
    }
    print(params)
    # ple.py:333: the number of tasks must match the list of task names and the list of expert counts
    assert params["num_tasks"] == len(params["task_names"]) == len(params["num_experts_per_task"]), \
        "num_tasks must equals both length of task_names and length of num_experts_per_task"
    common.run_estimator(ple_model_fn, params, example_parser, predictions_writer=common.write_multitask_predictions)
    print("after evaluate")


if __name__ == "__main__":
    flags.run(main)
