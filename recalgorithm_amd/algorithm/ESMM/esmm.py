"""ESMM entry point (Ma et al., "Entire Space Multi-Task Model: An Effective Approach for Estimating Post-Click Conversion
Rate", SIGIR 2018).  The upstream zoo lists ESMM in its multi-task table and has no file for it, so there is nothing to compare
line by line: the surface follows the upstream author's conventions as mirrored in algorithm/MMOE — the common flags,
`hidden_units`, `batch_norm`, `dropout_rate`, `create_feature_columns`, `example_parser` (a label dict with one key per task),
`esmm_model_fn(features, labels, mode, params)`, `main`, `write_predictions`, the scopes `dense_input`, `category_input`,
`tower/dense[_n]`, `tower/batch_normalization[_n]`, `tower/tower_ctr_logit`, `tower/tower_cvr_logit`, and the prediction keys
`ctr_probabilities`, `cvr_probabilities`, `ctcvr_probabilities`.  tests/esmm_ref.py is the float64 restatement the model answers
to.

Two towers over the shared embeddings: the CTR tower is trained on the click (`--ctr_task_name`, click_avatar), the CVR tower
only through pCTCVR = pCTR * pCVR against click AND conversion (`--cvr_task_name`, follow) over ALL impressions — it never sees a
loss over the clicked rows alone, which is the paper's answer to sample-selection bias and data sparsity.  Both loss terms, the
three probabilities and both logit gradients are one launch (ops.esmm_loss, csrc/esmm.hip); evaluation reports the CVR metrics
over the clicked impressions (masked metrics, include/recalgo_maskmetrics.h).

The towers are ordinary dense layers over one input, so its two input gradients are added by autograd (one elementwise launch):
nn.InputGradChain belongs to the expert layers' own autograd node and has nothing to chain through here.

    python -m recalgorithm_amd.algorithm.ESMM.esmm --ctr_task_name=click_avatar --cvr_task_name=follow --batch_size=4096
"""
from __future__ import annotations

import csv
from typing import Tuple

import torch

from ... import feature_column as fc
from ... import flags
from ...model_tail import finish_esmm_model_fn
from ...variables import variable_scope
from .. import _common as common
from ..MMOE.tower_layer import tower_layer
from ..utils import eval_input_fn, parse_example

common.define_common_flags(batch_size=1024, learning_rate=0.005)
flags.DEFINE_string("hidden_units", "512,256,128",
                    "Comma-separated list of number of units in each hidden layer of the final output part")
flags.DEFINE_boolean("batch_norm", True, "Perform batch normalization (True or False)")
flags.DEFINE_float("dropout_rate", 0.1, "Dropout rate")
flags.DEFINE_string("ctr_task_name", "click_avatar", "Label of the first step of the funnel (the click), a key of the tfrecord file")
flags.DEFINE_string("cvr_task_name", "follow", "Label of the second step of the funnel (the conversion), a key of the tfrecord file")
FLAGS = flags.FLAGS

PREDICTION_KEYS = ("ctr_probabilities", "cvr_probabilities", "ctcvr_probabilities")


def task_names() -> list:
    return [FLAGS.ctr_task_name, FLAGS.cvr_task_name]


def create_feature_columns() -> Tuple[list, list, list]:
    """-> (dense_feature_columns, category_feature_columns, label_feature_columns): MMoE's columns, one numeric label column for
    the click and one for the conversion."""
    cols, feedid_emb = common.wechat_category_columns(
        {"userid": 16, "device": 2, "authorid": 4, "bgm_song_id": 4, "bgm_singer_id": 4, "manual_tag_list": 4, "feedid": 16})
    label_cols = [fc.numeric_column(task_name, default_value=0.0) for task_name in task_names()]
    return common.dense_columns(), cols + feedid_emb, label_cols


total_feature_columns: list = []
label_feature_columns: list = []


def example_parser(serialized_example):
    """Batch of serialized tf.train.Example -> (features, {task_name: (B, 1)}) for the two task names."""
    spec = fc.make_parse_example_spec(total_feature_columns + label_feature_columns)
    features = parse_example(serialized_example, spec)
    labels = {task_name: features.pop(task_name) for task_name in task_names()}
    return features, labels


example_parser.columns_getter = lambda: (total_feature_columns, label_feature_columns)     # (the native decoder: utils.py)


def esmm_model_fn(features, labels, mode, params):
    with variable_scope("dense_input"):
        dense_input = fc.input_layer(features, params["dense_feature_columns"])
    with variable_scope("category_input"):
        category_input = fc.input_layer(features, params["category_feature_columns"])
    concat_all_input = torch.cat([dense_input, category_input], dim=-1)

    with variable_scope("tower"):       # one scope: the auto-numbered dense / batch_normalization names run on across the towers
        ctr_logit, cvr_logit = (tower_layer(concat_all_input, params["hidden_units"], mode, params["batch_norm"],
                                            params["dropout_rate"], name) for name in ("ctr", "cvr"))
    return finish_esmm_model_fn(mode, ctr_logit, cvr_logit, labels, params)


def main(unused_argv):
    global total_feature_columns, label_feature_columns
    dense_cols, category_cols, label_feature_columns = create_feature_columns()
    total_feature_columns = dense_cols + category_cols
    if FLAGS.ctr_task_name == FLAGS.cvr_task_name:
        raise ValueError("--ctr_task_name and --cvr_task_name name the two steps of a funnel: two different labels")
    params = {
        "dense_feature_columns": dense_cols,
        "category_feature_columns": category_cols,
        "hidden_units": FLAGS.hidden_units.split(","),
        "dropout_rate": FLAGS.dropout_rate,
        "batch_norm": FLAGS.batch_norm,
        "learning_rate": FLAGS.learning_rate,
        "ctr_task_name": FLAGS.ctr_task_name,
        "cvr_task_name": FLAGS.cvr_task_name,
    }
    common.run_estimator(esmm_model_fn, params, example_parser, predictions_writer=write_predictions)


def write_predictions(estimator, example_parser, out_csv="predictions.csv"):
    """One column per prediction key, as the multi-task scripts write theirs (common.write_multitask_predictions)."""
    results = estimator.predict(input_fn=lambda: eval_input_fn(
        filepath=FLAGS.eval_data, example_parser=example_parser, batch_size=FLAGS.batch_size))
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + list(PREDICTION_KEYS))
        for i, r in enumerate(results):
            w.writerow([i] + [float(r[k].reshape(-1)[0]) for k in PREDICTION_KEYS])


if __name__ == "__main__":
    flags.run(main)
