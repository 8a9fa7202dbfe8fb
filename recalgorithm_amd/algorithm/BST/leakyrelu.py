"""`leakyrelu(x, leak)` of the reference's algorithm/BST/leakyrelu.py: 0.5 (1 + leak) x + 0.5 (1 - leak) |x|.  Inside a
BST block the activation (leak = 0.01: 0.505 x + 0.495 |x|) is part of the fused FFN kernel (csrc/bst.hip); this function
is the reference's call surface for anything else, plain tensor arithmetic."""
from __future__ import annotations

import torch


def leakyrelu(x: torch.Tensor, leak: float = 0.01) -> torch.Tensor:
    f1 = 0.5 * (1 + leak)
    f2 = 0.5 * (1 - leak)
    return f1 * x + f2 * torch.abs(x)
