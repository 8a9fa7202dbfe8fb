"""DIEN (Deep Interest Evolution Network) entry point — MI355X drop-in for /root/reference algorithm/DIEN/dien.py: same
flags, `create_feature_columns` (6 lists), `example_parser`, `dien_model_fn(features, labels, mode, params)`, `main`, scopes
(`target_input`, `his_seq_input`, `seq_encoder` with the `fcn` stack INSIDE it, dien.py:240), prediction key `probabilities`,
Dice / PReLU MLP, tf.contrib.opt.LazyAdamOptimizer.  The interest module — GRU, attention, AGRU / AUGRU — is two launches
each way (csrc/dien.hip through rnn.dynamic_rnn).

    python -m recalgorithm_amd.algorithm.DIEN.dien --custom_gru_type=AUGRU --activation=dice

Two labelled differences from the reference's call sequence, neither observable in any output or gradient
(tests/test_dien_host.py proves both on the float64 restatement, bit for bit):
  * the first GRU gets `sequence_length` as well (dien.py:202 runs it over all T rows): the rows h[t >= L] that differ reach
    only replaced attention scores (weight exactly 0) and copied-through steps;
  * --sequence_max_length (not a reference flag; 0 = the batch's longest history, as the reference) pads the history to a
    static T, so that the step has static shapes and can be captured; a replaced score adds an exact 0 to the softmax's sum.
--use_auxiliary_loss=True raises: the reference's block (dien.py:259-300) slices a rank-1 tensor and cannot run.
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
from .custom_grucell import AGRUCell, AUGRUCell, GRUCell
from .rnn import attention_scores, dynamic_rnn

common.define_common_flags()
flags.DEFINE_string("hidden_units", "512,256,128", "Comma-separated list of number of units in each hidden layer of the deep part")
flags.DEFINE_boolean("batch_norm", True, "Perform batch normalization (True or False)")
flags.DEFINE_float("dropout_rate", 0.1, "Dropout rate")
flags.DEFINE_string("activation", "dice", "Dense layer activation, supported strings are in {'prelu', dice'}")
flags.DEFINE_boolean("use_auxiliary_loss", False, "Whether to use auxiliary loss.")
flags.DEFINE_integer("negative_sample_number", 3, "The number of negative samples per positive sample.")
flags.DEFINE_string("custom_gru_type", "AGRU", "The Type of custom GRU cell, supported strings are in {'AGRU', AUGRU'}")
flags.DEFINE_integer("gru_output_units", 8, "output dimension of gru cell.")
flags.DEFINE_integer("sequence_max_length", 0, "Pad the history to this many steps (static shapes: the training step can be "
                     "captured); 0 = the longest history of the batch, as the reference")
FLAGS = flags.FLAGS

AUXILIARY_LOSS = ("use_auxiliary_loss: the reference's auxiliary-loss block cannot run as written (dien.py:259-265: it slices the "
                  "rank-1 `sequnence_length` with [:, 1:, :], and the author notes \"以下代码无法运行\"); there is no stated "
                  "arithmetic to reproduce")


def create_feature_columns() -> Tuple[list, list, list, list, list, list]:
    """-> (dense, category, target_feedid, sequence, negative_sequence, label) feature columns; dien.py:58-145.  ONE 16-wide
    table shared by three sequence columns, two of them over the same key: feedid, his_read_comment_7d_seq and the
    negative-sample column, which the reference also reads from `his_read_comment_7d_seq` (dien.py:121)."""
    userid, device = common.vocab_column("userid"), common.vocab_column("device")
    authorid, bgm_song_id = common.vocab_column("authorid"), common.vocab_column("bgm_song_id")
    bgm_singer_id = common.vocab_column("bgm_singer_id")
    manual_tag_list = common.vocab_column("manual_tag_list", "manual_tag_id")
    feedid = common.vocab_column("feedid", sequence=True)
    his = common.vocab_column("his_read_comment_7d_seq", "feedid", sequence=True)
    neg = common.vocab_column("his_read_comment_7d_seq", "feedid", sequence=True)
    feedid_emb = fc.shared_embedding_columns([feedid, his, neg], 16, combiner="mean")
    category = [fc.embedding_column(userid, 16), fc.embedding_column(device, 2), fc.embedding_column(authorid, 4),
                fc.embedding_column(bgm_song_id, 4), fc.embedding_column(bgm_singer_id, 4),
                fc.embedding_column(manual_tag_list, 4, combiner="mean")]
    return common.dense_columns(), category, [feedid_emb[0]], [feedid_emb[1]], [feedid_emb[2]], common.label_columns()


total_feature_columns: list = []
label_feature_columns: list = []
example_parser = common.make_example_parser(lambda: (total_feature_columns, label_feature_columns))


def dien_model_fn(features, labels, mode, params):
    """dien.py:166-353."""
    training = mode == ModeKeys.TRAIN
    if params.get("use_auxiliary_loss"):
        raise NotImplementedError(AUXILIARY_LOSS)
    if params["custom_gru_type"] not in ("AGRU", "AUGRU"):           # (the reference falls back to AGRU silently, dien.py:220-223)
        raise ValueError(f"custom_gru_type={params['custom_gru_type']!r}: supported strings are AGRU and AUGRU")
    parts = []
    with variable_scope("dense_input"):
        dense_cols = params.get("dense_feature_columns") or []
        if dense_cols:
            parts.append(fc.input_layer(features, dense_cols))
    from recalgorithm_amd import sparse as _sparse
    static_T = int(params.get("sequence_max_length") or 0) or None
    with _sparse.batch_lookups():
        with variable_scope("category_input"):
            category_input = fc.input_layer(features, params["category_feature_columns"])
        with variable_scope("target_input"):
            target_input, _ = fc.sequence_input_layer(features, params["target_feedid_feature_columns"], max_length=1)
            target_input = target_input.squeeze(1)                                   # (B, H)
        with variable_scope("his_seq_input"):
            seq_input, seq_length = fc.sequence_input_layer(features, params["sequence_feature_columns"], max_length=static_T)

    with variable_scope("seq_encoder"):
        nh = int(params["gru_output_units"])
        h, _ = dynamic_rnn(cell=GRUCell(num_units=nh), inputs=seq_input, sequence_length=seq_length, dtype=torch.float32)
        scores = attention_scores(target_input)         # dien.py:205-218: computed by the second recurrence's launch
        custom_gru_cell = AUGRUCell(nh) if params["custom_gru_type"] == "AUGRU" else AGRUCell(nh)
        _, final_state = dynamic_rnn(custom_gru_cell, h, scores, sequence_length=seq_length, dtype=torch.float32)   # (B, nh)
        concat_all = torch.cat(parts + [category_input, target_input, final_state], dim=-1)
        with variable_scope("fcn"):
            net = concat_all
            for i, unit in enumerate(params["hidden_units"]):
                # dense -> dice | prelu -> batch_normalization -> dropout (dien.py:244-252): one autograd node in a training step
                net = nn.dense_activation_bn(net, unit, "dice" if params["activation"] == "dice" else "prelu", i + 1,
                                             bool(params["batch_norm"]), training,
                                             dropout_rate=params["dropout_rate"] if "dropout_rate" in params else None)
            logit = nn.dense(net, 1)
    return finish_model_fn(mode, logit, labels, dict(params, lazy_adam=True))          # dien.py:328: LazyAdamOptimizer


def main(unused_argv):
    global total_feature_columns, label_feature_columns
    dense_cols, category_cols, target_cols, seq_cols, neg_cols, label_feature_columns = create_feature_columns()
    # (dien.py:361 adds the negative-sample column too: it reads the same key from the same file, so the parse spec is the same)
    total_feature_columns = dense_cols + category_cols + target_cols + seq_cols + neg_cols
    params = {
        "dense_feature_columns": dense_cols,
        "category_feature_columns": category_cols,
        "sequence_feature_columns": seq_cols,
        "negative_sequence_feature_columns": neg_cols,
        "target_feedid_feature_columns": target_cols,
        "hidden_units": FLAGS.hidden_units.split(","),
        "dropout_rate": FLAGS.dropout_rate,
        "batch_norm": FLAGS.batch_norm,
        "learning_rate": FLAGS.learning_rate,
        "activation": FLAGS.activation,
        "use_auxiliary_loss": FLAGS.use_auxiliary_loss,
        "negative_sample_number": FLAGS.negative_sample_number,
        "custom_gru_type": FLAGS.custom_gru_type,
        "gru_output_units": FLAGS.gru_output_units,
        "sequence_max_length": FLAGS.sequence_max_length,
    }
    common.run_estimator(dien_model_fn, params, example_parser)


if __name__ == "__main__":
    flags.run(main)
