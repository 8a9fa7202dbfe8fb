"""DeepCrossing entry point — MI355X drop-in for the reference's algorithm/DeepCrossing/deepcrossing.py: same flags,
`create_feature_columns`, `example_parser`, `deepcrossing_model_fn(features, labels, mode, params)`, `main`, scopes
(`dense_input`, `category_input`, `residual_module`, the unnamed head `dense`), prediction keys (`logit`, `probabilities`).
The embedding gather, the residual stack and the loss tail are hand-written HIP kernels: the stack is nn.residual_stack,
which runs all units as ONE launch each way (csrc/residual.hip) below nn.RESIDUAL_COMPOSED_FROM_D columns — the reference's
82 among them — and as the dense engine's layers from there on.  params["fused_residual"] (not a reference key; None = that default)
forces either path.

    python -m recalgorithm_amd.algorithm.DeepCrossing.deepcrossing --residual_network_num=3 --batch_size=4096
"""
from __future__ import annotations

from typing import Tuple

import torch

from ... import feature_column as fc
from ... import flags, nn
from ...model_tail import finish_model_fn
from ...variables import variable_scope
from .. import _common as common
from .residual_unit import residual_unit  # noqa: F401  (the reference's import; the model_fn runs the units as one stack)

# flags: deepcrossing.py:20-37
common.define_common_flags(ragged_capacity=False)         # (this script keeps exactly the reference's flag list)
flags.DEFINE_integer("residual_internal_dim", 128, "Residual module internal dimension")
flags.DEFINE_integer("residual_network_num", 1, "Numbers of residual networks")
FLAGS = flags.FLAGS


def create_feature_columns() -> Tuple[list, list, list]:
    """-> (dense_feature_columns, category_feature_columns, label_feature_columns); deepcrossing.py:42-110."""
    dims = {"userid": 16, "device": 2, "authorid": 4, "bgm_song_id": 4, "bgm_singer_id": 4, "manual_tag_list": 4, "feedid": 16}
    cols, feedid_emb = common.wechat_category_columns(dims)
    return common.dense_columns(), cols + feedid_emb, common.label_columns()


total_feature_columns: list = []
label_feature_columns: list = []
example_parser = common.make_example_parser(lambda: (total_feature_columns, label_feature_columns))


def deepcrossing_model_fn(features, labels, mode, params):
    """deepcrossing.py:131-213."""
    with variable_scope("dense_input"):
        dense_cols = params.get("dense_feature_columns") or []
        dense_input = fc.input_layer(features, dense_cols) if dense_cols else None
    with variable_scope("category_input"):
        category_input = fc.input_layer(features, params["category_feature_columns"])
    concat_all = category_input if dense_input is None else torch.cat([dense_input, category_input], dim=-1)

    with variable_scope("residual_module"):
        # deepcrossing.py:155-157 chains residual_unit(net, internal_dim, index=i): the same variables, the stack as one op
        net = nn.residual_stack(concat_all, params["residual_internal_dim"], params["residual_network_num"],
                                fused=params.get("fused_residual"))

    logit = nn.dense(net, 1, activation=None)
    return finish_model_fn(mode, logit, labels, params,
                           predictions=lambda prob: {"logit": logit, "probabilities": prob})


def main(unused_argv):
    global total_feature_columns, label_feature_columns
    dense_cols, category_cols, label_feature_columns = create_feature_columns()
    total_feature_columns = dense_cols + category_cols
    params = {
        "category_feature_columns": category_cols,
        "dense_feature_columns": dense_cols,
        "residual_internal_dim": FLAGS.residual_internal_dim,
        "residual_network_num": FLAGS.residual_network_num,
        "learning_rate": FLAGS.learning_rate,
    }
    common.run_estimator(deepcrossing_model_fn, params, example_parser)


if __name__ == "__main__":
    flags.run(main)
