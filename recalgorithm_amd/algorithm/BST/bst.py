"""BST (Behavior Sequence Transformer) entry point — MI355X drop-in for the reference's algorithm/BST/bst.py: same flags,
`create_feature_columns` (5 lists), `example_parser`, `bst_model_fn(features, labels, mode, params)`, `main`, scopes
(`dense_input`, `category_input`, `target_input`, `his_seq_input`, `transformer_part`, `dnn_part`), prediction key
`probabilities`.

    python -m recalgorithm_amd.algorithm.BST.bst --num_transformer_block=1 --num_transformer_heads=3

The sequence length T enters the result three times — the softmax runs over all T keys, LayerNorm's moments and the final
pooling over all T rows, padded ones included — so by default T is what the reference's is: the longest history of the
batch + 1.  `--static_sequence_length` (not a reference flag, default off) pads every batch to sequence_max_length + 1
instead: the step then has static shapes and can be captured (estimator.GraphedTrainStep).  That equals the reference
exactly when the batch holds a history of the full sequence_max_length, and differs from it on a batch that does not.
"""
from __future__ import annotations

from typing import Tuple

import torch

from ... import feature_column as fc
from ... import flags, nn
from ...estimator import ModeKeys
from ...model_tail import finish_model_fn
from ...variables import variable_scope
from .. import _common as common
from .transformer_layer import bst_transformer

common.define_common_flags()
flags.DEFINE_string("hidden_units", "512,256,128", "Comma-separated list of number of units in each hidden layer of the deep part")
flags.DEFINE_boolean("batch_norm", True, "Perform batch normalization (True or False)")
flags.DEFINE_float("dropout_rate", 0.1, "Dropout rate")
flags.DEFINE_integer("sequence_max_length", 50, "Maximal length of user behavior sequence")
flags.DEFINE_integer("num_transformer_block", 1, "Number of transformer block")
flags.DEFINE_integer("num_transformer_heads", 3, "Number of heads in every transformer block")
flags.DEFINE_enum("pooling_method", "sum", ["sum", "mean"], "Pooling method in transformer final output")
flags.DEFINE_boolean("static_sequence_length", False,
                     "Pad every batch to sequence_max_length + 1 rows (static shapes for a captured step) instead of the batch's "
                     "longest history + 1 (the reference)")
FLAGS = flags.FLAGS


def create_feature_columns() -> Tuple[list, list, list, list, list]:
    """-> (dense, category, target_feedid, sequence, label) feature columns; bst.py:53-130.
    feedid / his_read_comment_7d_seq are *sequence* categorical columns sharing one 16-wide table;
    [0] is the target feed, [1] the history (shared_embedding_columns keeps input order)."""
    dims = {"userid": 16, "device": 2, "authorid": 4, "bgm_song_id": 4, "bgm_singer_id": 4,
            "manual_tag_list": 4, "feedid": 16}
    cols, feedid_emb = common.wechat_category_columns(dims, sequence_feed=True)
    return common.dense_columns(), cols, [feedid_emb[0]], [feedid_emb[1]], common.label_columns()


total_feature_columns: list = []
label_feature_columns: list = []
example_parser = common.make_example_parser(lambda: (total_feature_columns, label_feature_columns))


def bst_model_fn(features, labels, mode, params):
    """bst.py:151-259."""
    training = mode == ModeKeys.TRAIN
    parts = []
    with variable_scope("dense_input"):
        dense_cols = params.get("dense_feature_columns") or []
        if dense_cols:
            parts.append(fc.input_layer(features, dense_cols))
    # the three lookups are issued together: their `prepare` work is one launch per arena (sparse.batch_lookups)
    from recalgorithm_amd import sparse as _sparse
    static_T = int(params["sequence_max_length"]) if params.get("static_sequence_length") else None
    with _sparse.batch_lookups():
        with variable_scope("category_input"):
            category_input = fc.input_layer(features, params["category_feature_columns"])
        with variable_scope("target_input"):
            target_input, _ = fc.sequence_input_layer(features, params["target_feedid_feature_columns"], max_length=1)   # (B, 1, K)
        with variable_scope("his_seq_input"):
            seq_input, seq_length = fc.sequence_input_layer(features, params["sequence_feature_columns"], max_length=static_T)

    with variable_scope("transformer_part"):
        out = torch.cat([target_input, seq_input], dim=1)                            # (B, T + 1, K)
        blocks = int(params["num_transformer_block"])
        keys_length = seq_length + 1
        for i in range(blocks):
            out = bst_transformer(queries=out, keys=out, values=out, keys_length=keys_length,
                                  heads=params["num_transformer_heads"], index=i,
                                  max_length=params["sequence_max_length"] + 1, use_position_embedding=True,
                                  # the reduction over all rows (bst.py:195-198) rides in the last block's last kernel
                                  pool=params["pooling_method"] if i == blocks - 1 else None)
        if blocks == 0:
            out = out.sum(dim=1) if params["pooling_method"] == "sum" else out.mean(dim=1)

    with variable_scope("dnn_part"):
        net = torch.cat(parts + [category_input, out], dim=-1)
        for unit in params["hidden_units"]:
            bn = bool(params["batch_norm"])
            drop = "dropout_rate" in params and 0.0 < params["dropout_rate"] < 1.0
            net = nn.dense(net, unit, activation=None, bn_stats=bn and training)
            if bn:
                net = nn.batch_normalization(net, training=training)
            if drop:
                net = nn.dropout(net, params["dropout_rate"], training=training)
        logit = nn.dense(net, 1)
    return finish_model_fn(mode, logit, labels, params)


def main(unused_argv):
    global total_feature_columns, label_feature_columns
    dense_cols, category_cols, target_cols, seq_cols, label_feature_columns = create_feature_columns()
    total_feature_columns = dense_cols + category_cols + target_cols + seq_cols
    params = {
        "dense_feature_columns": dense_cols,
        "category_feature_columns": category_cols,
        "sequence_feature_columns": seq_cols,
        "target_feedid_feature_columns": target_cols,
        "hidden_units": FLAGS.hidden_units.split(","),
        "dropout_rate": FLAGS.dropout_rate,
        "batch_norm": FLAGS.batch_norm,
        "learning_rate": FLAGS.learning_rate,
        "sequence_max_length": FLAGS.sequence_max_length,
        "num_transformer_block": FLAGS.num_transformer_block,
        "num_transformer_heads": FLAGS.num_transformer_heads,
        "pooling_method": FLAGS.pooling_method,
        "static_sequence_length": FLAGS.static_sequence_length,
    }
    common.run_estimator(bst_model_fn, params, example_parser)


if __name__ == "__main__":
    flags.run(main)
