"""AutoInt entry point (Song et al., "AutoInt: Automatic Feature Interaction Learning via Self-Attentive Neural Networks", CIKM
2019, arXiv 1810.11921).  The upstream zoo names AutoInt on its to-do list and has no file for it, so there is nothing to compare
line by line: the surface follows the upstream author's conventions as mirrored in algorithm/AFM and algorithm/NFM — the common
flags, `create_feature_columns`, `example_parser`, `autoint_model_fn(features, labels, mode, params)`, `main`, the scopes
`dense_input/dense_logit`, `interacting_part`, `prediction_part/autoint_logit`, `deep_part`, and the prediction keys `logit`,
`probabilities`.  tests/autoint_ref.py is the float64 restatement the model answers to.

  * per-field embeddings: gather / bag-mean kernels, one input_layer per column (the seven columns of AFM and NFM);
  * `num_interacting_layers` interacting layers (nn.interacting_layer: one fused HIP kernel each way per layer, csrc/autoint.hip):
    D = embedding_dim into the first, head_num * att_embedding_size from then on; no scaling, biases, layer norm or dropout;
  * autoint_logit = dense(flattened attention output, 1); with `hidden_units` (AutoInt+) an MLP over the field embeddings adds
    deep_logit; the loss tail is the fused logit / loss kernel.

    python -m recalgorithm_amd.algorithm.AutoInt.autoint --num_interacting_layers=3 --head_num=2 --att_embedding_size=8
"""
from __future__ import annotations

from typing import Tuple

from ... import feature_column as fc
from ... import flags, nn
from ...estimator import ModeKeys
from ...model_tail import finish_model_fn
from ...variables import variable_scope
from .. import _common as common
from .interacting_layer import interacting_layer

common.define_common_flags(batch_size=1024, learning_rate=0.005)
flags.DEFINE_integer("embedding_dim", 8, "Embedding dimension")
flags.DEFINE_integer("att_embedding_size", 8, "Width of one attention head")
flags.DEFINE_integer("head_num", 2, "Number of attention heads")
flags.DEFINE_integer("num_interacting_layers", 3, "Number of interacting layers")
flags.DEFINE_boolean("use_residual", True, "Add the residual projection of a layer's input to its output (True or False)")
flags.DEFINE_string("hidden_units", "", "Comma-separated list of number of units in each hidden layer (empty: AutoInt; else AutoInt+)")
flags.DEFINE_boolean("batch_norm", True, "Perform batch normalization (True or False)")
flags.DEFINE_float("dropout_rate", 0.0, "Dropout rate")
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
    """"" -> [] (AutoInt), "256,128" -> [256, 128] (AutoInt+); a list passes through."""
    if isinstance(text, str):
        return [int(u) for u in text.split(",") if u.strip()]
    return [int(u) for u in text]


def autoint_model_fn(features, labels, mode, params):
    training = mode == ModeKeys.TRAIN
    cols = params["category_feature_columns"]
    F = len(cols)
    with variable_scope("dense_input"):
        dense_input = fc.input_layer(features, params["dense_feature_columns"])
        dense_logit = nn.dense(dense_input, 1, name="dense_logit")
    with variable_scope("interacting_part"):
        fields = fc.input_layers_concat(features, cols)                           # (batch, F * embedding_dim), list order
        att_out = fields
        for i in range(int(params["num_interacting_layers"])):
            att_out = interacting_layer(att_out, F, int(params["att_embedding_size"]), int(params["head_num"]),
                                        bool(params["use_residual"]), index=i)
    with variable_scope("prediction_part"):
        autoint_logit = nn.dense(att_out, 1, name="autoint_logit")                # on (batch, F * head_num * att_embedding_size)
    total_logit = dense_logit + autoint_logit
    hidden_units = parse_hidden_units(params.get("hidden_units", ""))
    if hidden_units:
        with variable_scope("deep_part"):
            net = fields
            for unit in hidden_units:
                net = nn.dense_relu_dropout_bn(net, unit, params.get("dropout_rate"), params["batch_norm"], training)
            deep_logit = nn.dense(net, 1, name="deep_logit")
        total_logit = total_logit + deep_logit
    return finish_model_fn(mode, total_logit, labels, params,
                           predictions=lambda prob: {"logit": total_logit, "probabilities": prob})


def main(unused_argv):
    global total_feature_columns, label_feature_columns
    dense, cat, label_feature_columns = create_feature_columns()
    total_feature_columns = dense + cat
    params = {"dense_feature_columns": dense, "category_feature_columns": cat, "embedding_dim": FLAGS.embedding_dim,
              "att_embedding_size": FLAGS.att_embedding_size, "head_num": FLAGS.head_num,
              "num_interacting_layers": FLAGS.num_interacting_layers, "use_residual": FLAGS.use_residual,
              "hidden_units": parse_hidden_units(FLAGS.hidden_units), "batch_norm": FLAGS.batch_norm,
              "dropout_rate": FLAGS.dropout_rate, "learning_rate": FLAGS.learning_rate}
    common.run_estimator(autoint_model_fn, params, example_parser)


if __name__ == "__main__":
    flags.run(main)
