"""`dynamic_rnn` of /root/reference algorithm/DIEN/rnn.py:443 (vendored TensorFlow, patched to hand att_scores[:, t] to the
cell) as a thin router to the recurrences of csrc/dien.hip.

    h, _ = dynamic_rnn(GRUCell(nh), inputs, sequence_length=lengths)                        -> nn.dien_gru
    states, final = dynamic_rnn(AUGRUCell(nh), h, attention_scores(target), lengths)        -> nn.dien_evolve

The reference computes the attention scores between the two calls with seven TF ops (dien.py:205-218); here they are part of
the second launch, so `att_scores` is an AttentionScores holder: what the scores are computed FROM (the target embedding),
filled with the scores [B, T, 1] once the launch has run."""
from __future__ import annotations

from typing import Optional

import torch

from ... import nn
from .custom_grucell import AGRUCell, AUGRUCell, GRUCell, _Cell


class AttentionScores:
    """softmax over all T of where(t < L, h[b, t] . (attention_project_matrix target_b), -2^32 + 1)  (dien.py:205-218)"""

    def __init__(self, target: torch.Tensor):
        self.target = target
        self.value: Optional[torch.Tensor] = None       # [B, T, 1] after dynamic_rnn


def attention_scores(target: torch.Tensor) -> AttentionScores:
    return AttentionScores(target)


def dynamic_rnn(cell, inputs, att_scores=None, sequence_length=None, dtype=None):
    """-> (outputs [B, T, nh], final state): rows t >= sequence_length of the outputs are zero, the state is copied through.
    GRUCell: the final state is not formed (the reference discards it, dien.py:202) and comes back as None."""
    if not isinstance(cell, _Cell):
        raise TypeError("dynamic_rnn: cell must be a GRUCell, AGRUCell or AUGRUCell of this package")
    if dtype not in (None, torch.float32):
        raise NotImplementedError("dynamic_rnn: float32 only")
    if isinstance(cell, GRUCell):
        if att_scores is not None:
            raise ValueError("dynamic_rnn: a GRUCell takes no att_scores")
        return nn.dien_gru(inputs, sequence_length, cell.state_size), None
    if not isinstance(att_scores, AttentionScores) or sequence_length is None:
        raise ValueError("dynamic_rnn: an AGRUCell / AUGRUCell needs att_scores=attention_scores(target) and a sequence_length")
    final, att, states = nn.dien_evolve(inputs, att_scores.target, sequence_length, cell.kind, return_states=True)
    att_scores.value = att.unsqueeze(-1)
    return states, final
