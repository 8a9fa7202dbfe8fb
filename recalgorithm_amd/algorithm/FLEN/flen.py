"""FLEN entry point (Chen et al., "FLEN: Leveraging Field for Scalable CTR Prediction", arXiv 1911.04690).  The upstream zoo
names FLEN on its to-do list and has no file for it, so there is nothing to compare line by line: the surface follows the upstream
author's conventions as mirrored in algorithm/AutoInt and algorithm/NFM — the common flags, `create_feature_columns`,
`example_parser`, `flen_model_fn(features, labels, mode, params)`, `main`, the scopes `dense_input/dense_logit`, `fwbi_part`,
`deep_part`, `prediction_part/flen_logit`, and the prediction keys `logit`, `probabilities`.  tests/flen_ref.py is the float64
restatement the model answers to.

  * per-field embeddings: gather / bag-mean kernels, one input_layer per column (the seven columns of AFM and NFM);
  * `field_groups` maps the columns onto M field groups (default: user, item, context); the field-wise bi-interaction
    (nn.field_wise_bi_interaction: one fused HIP kernel each way, csrc/flen.hip) gives the M field-wise embeddings e and the
    bi-interaction vector h — the MF term across the groups and the FM term inside each — with Dicefactor (`dicefactor_rate`)
    dropping path components when training;
  * the MLP reads [dense_input ; e]: the M field-wise embeddings, not the F field rows (the paper's scalability point);
  * flen_logit = dense([h ; MLP output], 1); total = dense_logit + flen_logit; the loss tail is the fused logit / loss kernel.

The categorical first-order term of the paper's linear part is left out, as in AutoInt here: the linear part is dense_logit over
the dense features alone.

    python -m recalgorithm_amd.algorithm.FLEN.flen --field_groups="userid,device;feedid,authorid,manual_tag_list;bgm_song_id,bgm_singer_id" --dicefactor_rate=0.1
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
from .field_wise_bi_interaction import field_wise_bi_interaction

DEFAULT_FIELD_GROUPS = "userid,device;feedid,authorid,manual_tag_list;bgm_song_id,bgm_singer_id"

common.define_common_flags(batch_size=1024, learning_rate=0.005)
flags.DEFINE_integer("embedding_dim", 8, "Embedding dimension")
flags.DEFINE_string("field_groups", DEFAULT_FIELD_GROUPS,
                    "Field groups: groups separated by ';', the column keys of a group by ',' (every column in exactly one group)")
flags.DEFINE_string("hidden_units", "512,256,128", "Comma-separated list of number of units in each hidden layer")
flags.DEFINE_boolean("batch_norm", True, "Perform batch normalization (True or False)")
flags.DEFINE_float("dropout_rate", 0.0, "Dropout rate of the MLP")
flags.DEFINE_float("dicefactor_rate", 0.0, "Dicefactor: dropout rate of the bi-linear paths of the field-wise bi-interaction")
FLAGS = flags.FLAGS

# (after this script's own flags: NFM's script defines hidden_units, batch_norm and dropout_rate with other defaults, and the first
# definition of a name in a process is the one that holds)
from ..NFM.nfm import sibling_category_columns  # noqa: E402


def create_feature_columns() -> Tuple[list, list, list]:
    """-> (dense_feature_columns, category_feature_columns, label_feature_columns): AFM's and NFM's columns."""
    return common.dense_columns(), sibling_category_columns(FLAGS.embedding_dim), common.label_columns()


total_feature_columns: list = []
label_feature_columns: list = []
example_parser = common.make_example_parser(lambda: (total_feature_columns, label_feature_columns))


def parse_hidden_units(text) -> list:
    """"512,256" -> [512, 256], "" -> []; a list passes through."""
    if isinstance(text, str):
        return [int(u) for u in text.split(",") if u.strip()]
    return [int(u) for u in text]


def parse_field_groups(text, keys) -> list:
    """"a,b;c" and the column keys in list order -> group_of, one group index per column (groups numbered in the order `text`
    names them).  A list of lists of keys passes as `text` too.  ValueError: fewer than two groups, an empty group, a key that
    is no column, a key named twice, a column in no group."""
    groups = [[k.strip() for k in g.split(",") if k.strip()] for g in text.split(";")] if isinstance(text, str) \
        else [[str(k) for k in g] for g in text]
    keys = list(keys)
    if len(groups) < 2 or any(not g for g in groups):
        raise ValueError(f"field_groups: at least two groups, none of them empty, got {text!r}")
    owner = {}
    for m, g in enumerate(groups):
        for k in g:
            if k not in keys:
                raise ValueError(f"field_groups: {k!r} is no category column (the columns: {keys})")
            if k in owner:
                raise ValueError(f"field_groups: {k!r} appears more than once")
            owner[k] = m
    missing = [k for k in keys if k not in owner]
    if missing:
        raise ValueError(f"field_groups: every column belongs to exactly one group; {missing} are in none")
    return [owner[k] for k in keys]


def flen_model_fn(features, labels, mode, params):
    training = mode == ModeKeys.TRAIN
    cols = params["category_feature_columns"]
    group_of = parse_field_groups(params.get("field_groups", DEFAULT_FIELD_GROUPS), [c.key for c in cols])
    with variable_scope("dense_input"):
        dense_input = fc.input_layer(features, params["dense_feature_columns"])
        dense_logit = nn.dense(dense_input, 1, name="dense_logit")
    with variable_scope("fwbi_part"):
        fields = fc.input_layers_concat(features, cols)                           # (batch, F * embedding_dim), list order
        e, h = field_wise_bi_interaction(fields, group_of, float(params.get("dicefactor_rate") or 0.0), training,
                                         fused=params.get("fused_fwbi"))
    with variable_scope("deep_part"):
        net = torch.cat([dense_input, e], dim=1)                                  # the M field-wise embeddings, not the F rows
        for unit in parse_hidden_units(params.get("hidden_units", "")):
            net = nn.dense_relu_dropout_bn(net, unit, params.get("dropout_rate"), params["batch_norm"], training)
    with variable_scope("prediction_part"):
        flen_logit = nn.dense(torch.cat([h, net], dim=1), 1, name="flen_logit")
    total_logit = dense_logit + flen_logit
    return finish_model_fn(mode, total_logit, labels, params,
                           predictions=lambda prob: {"logit": total_logit, "probabilities": prob})


def main(unused_argv):
    global total_feature_columns, label_feature_columns
    dense, cat, label_feature_columns = create_feature_columns()
    total_feature_columns = dense + cat
    parse_field_groups(FLAGS.field_groups, [c.key for c in cat])                  # (a bad grouping fails before any data is read)
    params = {"dense_feature_columns": dense, "category_feature_columns": cat, "embedding_dim": FLAGS.embedding_dim,
              "field_groups": FLAGS.field_groups, "hidden_units": parse_hidden_units(FLAGS.hidden_units),
              "batch_norm": FLAGS.batch_norm, "dropout_rate": FLAGS.dropout_rate, "dicefactor_rate": FLAGS.dicefactor_rate,
              "learning_rate": FLAGS.learning_rate}
    common.run_estimator(flen_model_fn, params, example_parser)


if __name__ == "__main__":
    flags.run(main)
