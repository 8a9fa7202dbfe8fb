"""DCN-V2 entry point (Wang et al., "DCN V2: Improved Deep & Cross Network and Practical Lessons for Web-scale Learning to Rank
Systems", WWW 2021, arXiv 2008.13535).  The upstream zoo has no file for it, so there is nothing to compare line by line: the
surface is algorithm/DCN/dcn.py's — its flags, `create_feature_columns`, `example_parser`, `dcnv2_model_fn(features, labels,
mode, params)`, `main`, the scopes `dense_input`, `category_input`, `cross_part`, `dnn_part`, `output_part` and the prediction
keys `logit`, `probabilities`.  tests/dcnv2_ref.py is the float64 restatement the model answers to.

  * `cross_parameterization=mix` (the form the paper recommends, eq. 4): per layer a mixture of `num_experts` experts of rank
    `low_rank` with a softmax gate — nn.cross_mix_layer, one fused HIP entry each way per layer (csrc/dcnv2.hip);
    `matrix` (eq. 1): x0 * (xl W + b) + xl with a full W, on the dense engine;
  * `structure=parallel` concatenates the cross and deep branches, as DCN does; `stacked` runs the deep branch on the cross output.

    python -m recalgorithm_amd.algorithm.DCNV2.dcnv2 --num_cross_layer=2 --low_rank=32 --num_experts=4 --batch_size=4096
"""
from __future__ import annotations

import torch

from ... import feature_column as fc
from ... import flags, nn
from ...model_tail import finish_model_fn
from ...variables import variable_scope
from .. import _common as common
from .cross_layer import cross_matrix_network, cross_mix_network

common.define_common_flags(batch_size=1024, learning_rate=0.005)
flags.DEFINE_string("hidden_units", "512,256,128", "Comma-separated list of number of units in each hidden layer")
flags.DEFINE_integer("num_cross_layer", 2, "Number of cross layers")
flags.DEFINE_enum("cross_parameterization", "mix", ["mix", "matrix"], "Cross layer form: mixture of low-rank experts, or full matrix")
flags.DEFINE_integer("low_rank", 32, "Rank of an expert of the mix form")
flags.DEFINE_integer("num_experts", 4, "Experts per cross layer of the mix form")
flags.DEFINE_enum("structure", "parallel", ["parallel", "stacked"], "Cross and deep branches side by side, or deep on the cross output")
FLAGS = flags.FLAGS

# (after this script's own flags: DCN's script defines num_cross_layer with another default, and the first definition of a name
# in a process is the one that holds)
from ..DCN.dcn import create_feature_columns  # noqa: E402,F401  (DCN's columns)

total_feature_columns: list = []
label_feature_columns: list = []
example_parser = common.make_example_parser(lambda: (total_feature_columns, label_feature_columns))


def parse_hidden_units(text) -> list:
    """"512,256" -> [512, 256]; "" -> []; a list passes through."""
    if isinstance(text, str):
        return [int(u) for u in text.split(",") if u.strip()]
    return [int(u) for u in text]


def dcnv2_model_fn(features, labels, mode, params):
    form, structure = params.get("cross_parameterization", "mix"), params.get("structure", "parallel")
    if form not in ("mix", "matrix") or structure not in ("parallel", "stacked"):
        raise ValueError(f"dcnv2_model_fn: cross_parameterization={form!r} (mix | matrix), structure={structure!r} (parallel | stacked)")
    with variable_scope("dense_input"):
        dense_cols = params.get("dense_feature_columns") or []
        dense_input = fc.input_layer(features, dense_cols) if dense_cols else None
    with variable_scope("category_input"):
        category_input = fc.input_layer(features, params["category_feature_columns"])
    concat_all = category_input if dense_input is None else torch.cat([dense_input, category_input], dim=-1)

    with variable_scope("cross_part"):
        if form == "mix":
            cross_vec = cross_mix_network(concat_all, params["num_cross_layer"], params.get("low_rank", 32),
                                          params.get("num_experts", 4), fused=params.get("cross_fused"))
        else:
            cross_vec = cross_matrix_network(concat_all, params["num_cross_layer"])

    hidden_units = parse_hidden_units(params["hidden_units"])
    with variable_scope("dnn_part"):
        dnn_vec = cross_vec if structure == "stacked" else concat_all
        for i, unit in enumerate(hidden_units):
            dnn_vec = nn.dense(dnn_vec, unit, activation="relu", name=f"dnn_dense_{i}")

    with variable_scope("output_part"):
        output = dnn_vec if structure == "stacked" else nn.concat([cross_vec, dnn_vec], axis=-1)
        logit = nn.dense(output, 1, activation=None)

    return finish_model_fn(mode, logit, labels, params,
                           predictions=lambda prob: {"logit": logit, "probabilities": prob})


def main(unused_argv):
    global total_feature_columns, label_feature_columns
    dense_cols, category_cols, label_feature_columns = create_feature_columns()
    total_feature_columns = dense_cols + category_cols
    params = {"category_feature_columns": category_cols, "dense_feature_columns": dense_cols,
              "hidden_units": parse_hidden_units(FLAGS.hidden_units), "num_cross_layer": FLAGS.num_cross_layer,
              "cross_parameterization": FLAGS.cross_parameterization, "low_rank": FLAGS.low_rank,
              "num_experts": FLAGS.num_experts, "structure": FLAGS.structure, "learning_rate": FLAGS.learning_rate}
    common.run_estimator(dcnv2_model_fn, params, example_parser)


if __name__ == "__main__":
    flags.run(main)
