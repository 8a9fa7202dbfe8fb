"""Wide&Deep (Cheng et al., DLRS 2016) entry point — MI355X drop-in for the reference's algorithm/WideAndDeep/wide_and_deep.py:
same flags and defaults, `create_feature_columns()` -> (wide_part_feature_columns, deep_part_feature_columns),
`example_parser`, `wide_and_deep_model_fn(features, labels, mode, params)`, `main`, the variable names
`wide_part/wide_part_variables/{kernel,bias}` and `deep_part/...`, the prediction key `probabilities`.

The wide part — crossed_column([userid, manual_tag_list], 100000) -> indicator -> dense(1) — is ONE HIP launch that hashes
the crosses on the device and never builds the [B, 100000] multi-hot (nn.crossed_indicator_dense, csrc/wide.hip); its logit
joins the fused logit / loss launch of the deep tower as an addend.  It trains with FTRL (estimator.FtrlOptimizer: the
touched buckets, fused with the deterministic per-bucket gradient sum), the deep part with Adam, from one backward pass.

    python -m recalgorithm_amd.algorithm.WideAndDeep.wide_and_deep --batch_size=4096
"""
from __future__ import annotations

import os
from typing import Any, List, Tuple

from ... import estimator as est
from ... import feature_column as fc
from ... import flags, nn
from ...estimator import ModeKeys
from ...model_tail import finish_model_fn
from ...variables import variable_scope
from .. import _common as common
from ..utils import parse_example

# flags: the reference's algorithm/WideAndDeep/wide_and_deep.py:12-39 (no `learning_rate`: one rate per part)
flags.DEFINE_string("model_dir", "./model_dir", "Directory where model parameters, graph, etc are saved")
flags.DEFINE_string("output_dir", "./output_dir", "Directory where pb file are saved")
flags.DEFINE_string("train_data", "../../dataset/wechat_algo_data1/tfrecord/train.tfrecord", "Path to the train data")
flags.DEFINE_string("eval_data", "../../dataset/wechat_algo_data1/tfrecord/test.tfrecord", "Path to the evaluation data")
flags.DEFINE_string("vocabulary_dir", "../../dataset/wechat_algo_data1/vocabulary/", "Folder where the vocabulary file is stored")
flags.DEFINE_integer("num_epochs", 1, "Epoch of training phase")
flags.DEFINE_integer("train_steps", 10000, "Number of (global) training steps to perform")
flags.DEFINE_integer("shuffle_buffer_size", 10000, "Dataset shuffle buffer size")
flags.DEFINE_integer("num_parallel_readers", -1, "Number of parallel readers for training data")
flags.DEFINE_integer("save_checkpoints_steps", 1000, "Save checkpoints every this many steps")
flags.DEFINE_integer("batch_size", 1024, "Training batch size")
flags.DEFINE_float("wide_part_learning_rate", 0.005, "Wide part learning rate")
flags.DEFINE_float("deep_part_learning_rate", 0.001, "Deep part learning rate")
flags.DEFINE_string("deep_part_optimizer", "Adam",
                    "Wide part optimizer, supported strings are in {'Adagrad', 'Adam', 'Ftrl', 'RMSProp', 'SGD'}")
flags.DEFINE_string("hidden_units", "512,256,128",
                    "Comma-separated list of number of units in each hidden layer of the deep part")
flags.DEFINE_boolean("batch_norm", True, "Perform batch normalization (True or False)")
flags.DEFINE_float("dropout_rate", 0, "Dropout rate")
FLAGS = flags.FLAGS

HASH_BUCKET_SIZE = 100000       # wide_and_deep.py:121


def create_feature_columns() -> Tuple[List[Any], List[Any]]:
    """-> (wide_part_feature_columns, deep_part_feature_columns); wide_and_deep.py:58-126."""
    deep_part_feature_columns = common.dense_columns()
    vocab = lambda key, fname=None: fc.categorical_column_with_vocabulary_file(
        key, os.path.join(FLAGS.vocabulary_dir, (fname or key) + ".txt"))
    userid, feedid, device, authorid = vocab("userid"), vocab("feedid"), vocab("device"), vocab("authorid")
    bgm_song_id, bgm_singer_id = vocab("bgm_song_id"), vocab("bgm_singer_id")
    manual_tag_list = vocab("manual_tag_list", "manual_tag_id")
    his_read_comment_7d_seq = vocab("his_read_comment_7d_seq", "feedid")
    deep_part_feature_columns += [
        fc.embedding_column(userid, 16), fc.embedding_column(device, 2), fc.embedding_column(authorid, 4),
        fc.embedding_column(bgm_song_id, 4), fc.embedding_column(bgm_singer_id, 4),
        fc.embedding_column(manual_tag_list, 4, combiner="mean")]
    deep_part_feature_columns += fc.shared_embedding_columns([feedid, his_read_comment_7d_seq], 16, combiner="mean")
    cross_userid_manualtag = fc.crossed_column([userid, manual_tag_list], hash_bucket_size=HASH_BUCKET_SIZE)
    wide_part_feature_columns = [fc.indicator_column(cross_userid_manualtag)]
    return wide_part_feature_columns, deep_part_feature_columns


total_feature_columns: list = []


def example_parser(serialized_example):
    """Batch of serialized tf.train.Example -> (features, {"read_comment": (B, 1)}); wide_and_deep.py:129-145."""
    spec = fc.make_parse_example_spec(total_feature_columns + common.label_columns())
    features = parse_example(serialized_example, spec)
    read_comment = features.pop("read_comment")
    return features, {"read_comment": read_comment}


def _decoder_columns():
    """the native decoder reads base columns: the crossed column contributes the two vocabulary columns it crosses"""
    cols = []
    for c in total_feature_columns:
        cols += list(c.categorical_column.keys) if fc.is_crossed_indicator(c) else [c]
    return cols, common.label_columns()


example_parser.columns_getter = _decoder_columns     # native decoder hook


def _deep_part_optimizer(params):
    """wide_and_deep.py:260-271.  (Its 'RMSProp' and 'ftrl' branches assign to params[...] and leave `deep_part_optimizer`
    unbound: a NameError in the reference itself.)"""
    name = params["deep_part_optimizer"]
    if name == "Adam":
        return est.AdamOptimizer(learning_rate=params["deep_part_learning_rate"], beta1=0.9, beta2=0.999, epsilon=1e-8)
    if name in ("Adagrad", "SGD"):
        raise NotImplementedError(f"--deep_part_optimizer={name}: only Adam has a kernel here")
    raise ValueError(f"--deep_part_optimizer={name}: the reference defines no optimizer for it (NameError at wide_and_deep.py:272)")


def wide_and_deep_model_fn(features, labels, mode, params):
    """wide_and_deep.py:194-307."""
    training = mode == ModeKeys.TRAIN
    with variable_scope("wide_part"):
        # fc.input_layer + tf.layers.dense(wide_input, 1, name="wide_part_variables"), :209-210
        wide_logit = nn.crossed_indicator_dense(features, params["wide_part_feature_columns"], 1, name="wide_part_variables",
                                                training=training)
    with variable_scope("deep_part"):
        net = fc.input_layer(features, params["deep_part_feature_columns"])
        for unit in params["hidden_units"]:
            # dense(relu) -> [dropout] -> [batch_normalization], :217-221
            net = nn.dense_relu_dropout_bn(net, unit, params["dropout_rate"] if "dropout_rate" in params else None,
                                           bool(params["batch_norm"]), training)
        deep_logit = nn.dense(net, 1)
    # :225; the wide logit joins the lazily evaluated head as an addend of the fused logit / loss launch
    total_logit = wide_logit + deep_logit

    def train_op(loss):
        # :251-276: FTRL on wide_part, the chosen optimizer on deep_part, one backward pass, one global step
        wide_part_vars = est.get_collection(est.GraphKeys.TRAINABLE_VARIABLES, scope="wide_part")
        deep_part_vars = est.get_collection(est.GraphKeys.TRAINABLE_VARIABLES, scope="deep_part")
        wide_part_optimizer = est.FtrlOptimizer(learning_rate=params["wide_part_learning_rate"])
        wide_part_op = wide_part_optimizer.minimize(loss=loss, global_step=est.get_global_step(), var_list=wide_part_vars)
        deep_part_op = _deep_part_optimizer(params).minimize(loss=loss, global_step=None, var_list=deep_part_vars)
        return est.group(wide_part_op, deep_part_op)

    return finish_model_fn(mode, total_logit, labels, params, train_op=train_op)


def main(unused_argv):
    global total_feature_columns
    wide_columns, deep_columns = create_feature_columns()
    total_feature_columns = wide_columns + deep_columns
    params = {
        "wide_part_feature_columns": wide_columns,
        "deep_part_feature_columns": deep_columns,
        "hidden_units": FLAGS.hidden_units.split(","),
        "dropout_rate": FLAGS.dropout_rate,
        "batch_norm": FLAGS.batch_norm,
        "deep_part_optimizer": FLAGS.deep_part_optimizer,
        "wide_part_learning_rate": FLAGS.wide_part_learning_rate,
        "deep_part_learning_rate": FLAGS.deep_part_learning_rate,
    }
    common.run_estimator(wide_and_deep_model_fn, params, example_parser)
    print("after evaluate")


if __name__ == "__main__":
    flags.run(main)
