"""`field_wise_bi_interaction`: FLEN's interaction layer over the field embeddings (Chen et al., arXiv 1911.04690, section 3.3),
in the manner of the upstream author's layer files (DeepCrossing/residual_unit.py): a thin function over
nn.field_wise_bi_interaction, which owns the variables and runs the layer as one fused kernel each way (csrc/flen.hip)."""
from __future__ import annotations

from ... import nn


def field_wise_bi_interaction(input, group_of, dicefactor_rate=0.0, training=False, fused=None):
    """input [batch, len(group_of) * K] -> (the M field-wise embeddings [batch, M * K], the MF term across the field groups plus
    the FM term inside each [batch, K]); Dicefactor drops path components when training."""
    return nn.field_wise_bi_interaction(input, group_of, dicefactor_rate, training, fused=fused)
