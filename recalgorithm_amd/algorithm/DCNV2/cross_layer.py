"""DCN-V2's cross layers, in the manner of algorithm/DCN/cross_layer.py: `cross_mix_layer` / `cross_mix_network` (the mixture
of low-rank experts, eq. 4 of the paper: nn.cross_mix_layer, one fused HIP entry each way per layer, csrc/dcnv2.hip) and
`cross_matrix_layer` / `cross_matrix_network` (the full-matrix form, eq. 1, on the dense engine)."""
from __future__ import annotations

import torch

from ... import nn
from ...nn import cross_mix_layer, cross_mix_network  # noqa: F401  (the model's names for them)
from ...variables import variable_scope


def cross_matrix_layer(x0: torch.Tensor, xl: torch.Tensor, index: int) -> torch.Tensor:
    """x0 * (xl W + b) + xl with W [D, D]: variables cross_layer_<index>/kernel (glorot-uniform) and /bias (zeros) — one dense
    layer without activation and one torch.addcmul."""
    with variable_scope(f"cross_layer_{index}"):
        lin = nn.dense(xl, int(x0.shape[-1]), activation=None, name="matrix")
    return torch.addcmul(xl, x0, lin)


def cross_matrix_network(x0: torch.Tensor, num_cross_layer: int) -> torch.Tensor:
    xl = x0
    for i in range(int(num_cross_layer)):
        xl = cross_matrix_layer(x0, xl, i)
    return xl
