"""Task tower — drop-in for /root/reference algorithm/MMOE/tower_layer.py:4-29."""
from __future__ import annotations

from ... import nn
from ...estimator import ModeKeys


def tower_layer(x, hidden_units, mode, batch_norm=True, dropout_rate=0.1, name=""):
    """dense(relu) -> dropout -> batch_normalization per hidden unit (tower_layer.py:19-24: auto-named `dense[_n]`,
    `batch_normalization[_n]` inside the caller's scope, so the numbering runs on across the tasks), then the one-unit
    `tower_<name>_logit` head (:26).  -> the task logit [B, 1] (un-evaluated in a TRAIN step: nn.LazyLogit)."""
    training = mode == ModeKeys.TRAIN
    net = x
    for unit in hidden_units:
        net = nn.dense_relu_dropout_bn(net, unit, dropout_rate, bool(batch_norm), training)
    return nn.dense(net, 1, name=f"tower_{name}_logit")
