"""`bst_transformer` of the reference's algorithm/BST/transformer_layer.py:6-81, same signature.  BST calls it with
queries = keys = values (bst.py:187-194) and a position embedding; that is what the two fused kernels per direction of
csrc/bst.hip compute (nn.bst_transformer), anything else is refused."""
from __future__ import annotations

from typing import Optional

from ... import nn


def bst_transformer(queries, keys, values, keys_length, heads, index, max_length, use_position_embedding=True,
                    pool: Optional[str] = None):
    """-> [B, T, d], the block's output — or, with pool='sum' | 'mean' (not a reference argument), the reduction over all T
    rows that bst.py:195-198 applies to the last block, fused into the block's last kernel."""
    if keys is not queries or values is not queries:
        raise NotImplementedError("bst_transformer: the fused block serves self-attention (queries is keys is values, bst.py:187)")
    if not use_position_embedding:
        raise NotImplementedError("bst_transformer: the fused block adds the position embedding (bst.py:194)")
    return nn.bst_transformer(queries, keys_length, heads, index, max_length, pool=pool)
