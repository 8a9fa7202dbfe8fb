"""MMoE (Ma et al., KDD 2018) entry point — MI355X drop-in for /root/reference algorithm/MMOE/mmoe.py: same flags
(`num_experts`, `expert_hidden_units`, `num_tasks`, `task_names` included), `create_feature_columns`, `example_parser`
(a label dict with one key per task), `mmoe_model_fn(features, labels, mode, params)`, `main`, same variable scopes
(`experts/expert_<i>`, `gates/gate_<i>`, `tower/dense[_n]`, `tower/batch_normalization[_n]`, `tower/tower_<task>_logit`)
and prediction keys (`<task>_probabilities`).

The expert layers are E GEMM launches over the shared input, the T softmax gates and the per-task mix of the experts are
ONE kernel each way (ops.gate_mix, csrc/mmoe.hip), the towers run on the fp32-MFMA dense kernels with the fused
dropout / BatchNorm epilogues, the T losses and their sum are one launch (ops.multitask_sigmoid_cross_entropy).

    python -m recalgorithm_amd.algorithm.MMOE.mmoe --task_names=read_comment,like,click_avatar --batch_size=4096
"""
from __future__ import annotations

from typing import Tuple

import torch

from ... import feature_column as fc
from ... import flags, nn
from ...model_tail import finish_multitask_model_fn
from ...variables import variable_scope
from .. import _common as common
from ..utils import parse_example
from .tower_layer import tower_layer

# flags: /root/reference algorithm/MMOE/mmoe.py:16-44
common.define_common_flags(batch_size=1024, learning_rate=0.005)
flags.DEFINE_string("hidden_units", "512,256,128",
                    "Comma-separated list of number of units in each hidden layer of the final output part")
flags.DEFINE_boolean("batch_norm", True, "Perform batch normalization (True or False)")
flags.DEFINE_float("dropout_rate", 0.1, "Dropout rate")
flags.DEFINE_integer("num_experts", 3, "Number of experts")
flags.DEFINE_integer("expert_hidden_units", 512, "Expert module output dimension")
flags.DEFINE_integer("num_tasks", 3, "Number of tasks, that's number of gates")
flags.DEFINE_string("task_names", "read_comment,like,click_avatar",
                    "Comma-separated list of task names, each must be in keys of tfrecord file")
FLAGS = flags.FLAGS


def create_feature_columns() -> Tuple[list, list, list]:
    """-> (dense_feature_columns, category_feature_columns, label_feature_columns); mmoe.py:49-121 (the columns of DCN,
    one numeric label column per task name)."""
    cols, feedid_emb = common.wechat_category_columns(
        {"userid": 16, "device": 2, "authorid": 4, "bgm_song_id": 4, "bgm_singer_id": 4, "manual_tag_list": 4, "feedid": 16})
    label_cols = [fc.numeric_column(task_name, default_value=0.0) for task_name in FLAGS.task_names.split(",")]
    return common.dense_columns(), cols + feedid_emb, label_cols


total_feature_columns: list = []
label_feature_columns: list = []


def example_parser(serialized_example):
    """Batch of serialized tf.train.Example -> (features, {task_name: (B, 1)}); mmoe.py:124-140."""
    spec = fc.make_parse_example_spec(total_feature_columns + label_feature_columns)
    features = parse_example(serialized_example, spec)
    labels = {task_name: features.pop(task_name) for task_name in FLAGS.task_names.split(",")}
    return features, labels


example_parser.columns_getter = lambda: (total_feature_columns, label_feature_columns)     # (the native decoder: utils.py)


def mmoe_model_fn(features, labels, mode, params):
    """mmoe.py:183-287."""
    with variable_scope("dense_input"):
        dense_input = fc.input_layer(features, params["dense_feature_columns"])
    with variable_scope("category_input"):
        category_input = fc.input_layer(features, params["category_feature_columns"])
    concat_all_input = torch.cat([dense_input, category_input], dim=-1)

    # concat_all_input feeds the E expert layers and the T gates: its 1 + E input gradients are summed inside the expert
    # layers' input-gradient GEMMs (nn.InputGradChain)
    chain = nn.InputGradChain()
    with variable_scope("experts"):
        experts = nn.expert_layers(concat_all_input, params["expert_hidden_units"], params["num_experts"], chain=chain)
    with variable_scope("gates"):
        # the gates, the [B, E, H] concat and the per-task matmul of mmoe.py:208-232: one kernel
        towers, _gates = nn.gate_mix(concat_all_input, experts, params["num_tasks"], chain=chain)

    with variable_scope("tower"):
        task_names = params["task_names"]
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
        "num_experts": FLAGS.num_experts,
        "num_tasks": FLAGS.num_tasks,
        "expert_hidden_units": FLAGS.expert_hidden_units,
        "task_names": FLAGS.task_names.split(","),
    }
    # mmoe.py:305: the number of tasks must match the list of task names
    assert params["num_tasks"] == len(params["task_names"]), "num_tasks must equals length of task_names"
    common.run_estimator(mmoe_model_fn, params, example_parser, predictions_writer=write_predictions)
    print("after evaluate")


# mmoe.py:341-351, shared with the other multi-task scripts
write_predictions = common.write_multitask_predictions


if __name__ == "__main__":
    flags.run(main)
