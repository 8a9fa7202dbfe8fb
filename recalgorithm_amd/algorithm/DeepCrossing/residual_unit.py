"""`residual_unit` of the reference's algorithm/DeepCrossing/residual_unit.py:4-22, same signature: the one-unit case of the
fused residual stack (nn.residual_stack; csrc/residual.hip)."""
from __future__ import annotations

from ... import nn


def residual_unit(input, internal_dim=None, index=None):
    """relu(input + dense_<index>_1(relu(dense_<index>_0(input)))) -> a tensor of input's shape."""
    return nn.residual_unit(input, internal_dim, index)
