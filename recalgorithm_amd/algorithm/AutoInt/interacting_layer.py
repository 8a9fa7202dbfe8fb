"""`interacting_layer`: one multi-head self-attention layer over the field embeddings (AutoInt, eqs. 5-8), in the manner of
the upstream author's layer files (DeepCrossing/residual_unit.py): a thin function over nn.interacting_layer, which owns the
variables and runs the layer as one fused kernel each way (csrc/autoint.hip)."""
from __future__ import annotations

from ... import nn


def interacting_layer(input, field_num, att_embedding_size=8, head_num=2, use_res=True, index=0):
    """input [batch, field_num * D] -> relu(multi-head attention over the fields (+ input W_res)),
    [batch, field_num * head_num * att_embedding_size]."""
    return nn.interacting_layer(input, field_num, att_embedding_size, head_num, use_res, index)
