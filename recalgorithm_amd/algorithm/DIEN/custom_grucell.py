"""The cells of /root/reference algorithm/DIEN/custom_grucell.py as thin objects: they carry the cell's kind and width,
`rnn.dynamic_rnn` routes them to the fused recurrences of csrc/dien.hip (nn.dien_evolve), which hold the arithmetic —
[r, u] = sigmoid([x, h] Wg + bg), c = tanh([x, r * h] Wc + bc), then
    AGRUCell:  h' = (1 - a) h + a c
    AUGRUCell: u' = (1 - a) u, h' = u' h + (1 - u') c
with the attention score a of the step.  The reference's cells override __call__, so their variables carry no cell-name
scope: <scope>/rnn/{gates,candidate}/{kernel,bias}, gates bias initialised to 1."""
from __future__ import annotations


class _Cell:
    kind = None

    def __init__(self, num_units, activation=None, reuse=None, kernel_initializer=None, bias_initializer=None):
        if activation is not None or kernel_initializer is not None or bias_initializer is not None:
            raise NotImplementedError(f"{type(self).__name__}: the kernels serve tanh, the scope's default kernel initializer and "
                                      "the cell's default biases (1 for the gates, 0 for the candidate)")
        self._num_units = int(num_units)

    @property
    def state_size(self):
        return self._num_units

    @property
    def output_size(self):
        return self._num_units


class GRUCell(_Cell):
    """tf.nn.rnn_cell.GRUCell(num_units): variables <scope>/rnn/gru_cell/{gates,candidate}/{kernel,bias}"""
    kind = "GRU"


class AGRUCell(_Cell):
    kind = "AGRU"


class AUGRUCell(_Cell):
    kind = "AUGRU"
