"""Generate tests/golden/model_dien.npz, model_dien_augru_dropout.npz and model_dien_augru_prelu.npz by executing the
reference's own, unmodified algorithm/DIEN/dien.py and custom_grucell.py against oracle/tf1_shim — the DIEN sibling of
scripts/gen_golden_bst.py (same B = 48 batch: history lengths 0..8, one empty history, OOV ids; same labels, same key scheme),
kept outside the frozen oracle/ folder.

    python scripts/gen_golden_dien.py            # rewrites the three files
    python scripts/gen_golden_dien.py --check    # regenerates in memory, compares bit for bit with the committed files

What dien.py and custom_grucell.py use and the shim does not define is added HERE, to the imported shim module and to
sys.modules (oracle/ is left untouched):
  * the tensorflow.python.ops.* modules custom_grucell.py imports: rnn_cell.RNNCell / LayerRNNCell (with zero_state),
    math_ops (sigmoid, tanh), array_ops (split), init_ops (constant_initializer), variable_scope, and
    tensorflow.contrib.rnn.python.ops.core_rnn_cell._Linear;
  * tf.nn.rnn_cell.GRUCell, tf.contrib.opt.LazyAdamOptimizer, tf.compat.v1.logging;
  * a module `rnn` with a `dynamic_rnn`, in place of the reference's rnn.py.

THE FOLLOWING ARE RESTATEMENTS, NOT TENSORFLOW, written from knowledge of the TF 1.14 sources; no TensorFlow exists where
this runs to confirm them.
  * dynamic_rnn restates the reference's rnn.py:443-812 — 1454 lines of vendored TensorFlow internals (TensorArray,
    while_loop, cond) patched to hand att_scores[:, t] to the cell — as what it computes: a variable scope `rnn`, a zero
    initial state, a loop over the T steps, and with sequence_length the rule of rnn.py:201-219, where(time >= sequence_length)
    copies the state through and emits a zero output row.
  * GRUCell: variables <scope>/gru_cell/{gates,candidate}/{kernel,bias} (the layer's own name scope), ONE gates product split
    into r | u, the reset gate applied before the candidate's product, gates bias initialised to 1.0, candidate bias to 0,
    kernels by the scope's default initializer (glorot uniform), new_h = u * h + (1 - u) * c.
  * _Linear: `kernel` [sum of the inputs' widths, out] and `bias` [out] (zeros unless an initializer is given) in the scope it
    is constructed in; concat(inputs, 1) @ kernel + bias.  custom_grucell.py's cells override __call__, so they add no scope of
    their own: their variables are <scope>/{gates,candidate}/{kernel,bias}.
  * LazyAdamOptimizer: one step from zero moments.  A row outside the batch's IndexedSlices has g = 0, m = v = 0 and does not
    move under either optimizer, a row inside takes the same formula: the FIRST step of LazyAdam equals tf.train.AdamOptimizer's,
    which is what the shim's optimizer applies.  (Where the two differ — from the second step on — is tested against
    oracle.ref_ops.lazy_adam_step, not against a golden.)

The seed of each golden is the first of 4242, 4243, .. for which no gradient array is all zero (meta/seed).

Keys: var/<name>, predict/probabilities, train/loss, grad/<name>, var_after/<name>, aux/dropout_mask_<i> (call order),
eval/loss, eval/accuracy, eval/auc, flag/<flag>, meta/learning_rate, meta/seed.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

FLAGS = dict(hidden_units="16,8", gru_output_units=8, learning_rate=0.005, batch_norm=True, use_auxiliary_loss=False)
CONFIGS = {"model_dien": dict(FLAGS, custom_gru_type="AGRU", activation="dice", dropout_rate=0.0),
           "model_dien_augru_dropout": dict(FLAGS, custom_gru_type="AUGRU", activation="dice", dropout_rate=0.1),
           "model_dien_augru_prelu": dict(FLAGS, custom_gru_type="AUGRU", activation="prelu", dropout_rate=0.0)}


def extend_shim(tf):
    """Add the names listed in the module docstring to the imported shim and to sys.modules."""
    class RNNCell:
        def __init__(self, _reuse=None, name=None, **_kw):
            self._reuse = _reuse

        def zero_state(self, batch_size, dtype=None):
            return tf.zeros((tf._int(batch_size), self.state_size))

    class _Linear:
        def __init__(self, args, output_size, build_bias, bias_initializer=None, kernel_initializer=None):
            total = sum(int(a.get_shape()[-1]) for a in args)
            self.kernel = tf.get_variable("kernel", (total, output_size), initializer=kernel_initializer)
            self.bias = tf.get_variable("bias", (output_size,), initializer=bias_initializer or tf.zeros_initializer()) \
                if build_bias else None

        def __call__(self, args):
            out = torch.cat([tf._raw(a) for a in args], dim=1) @ self.kernel.t
            return tf.T(out if self.bias is None else out + self.bias.t)

    class GRUCell(RNNCell):
        def __init__(self, num_units, **_kw):
            super().__init__()
            self._num_units = num_units
            self._gates = self._candidate = None

        state_size = output_size = property(lambda self: self._num_units)

        def __call__(self, inputs, state):
            with tf.variable_scope("gru_cell"):
                if self._gates is None:
                    with tf.variable_scope("gates"):
                        self._gates = _Linear([inputs, state], 2 * self._num_units, True, bias_initializer=tf.constant_initializer(1.0))
                value = torch.sigmoid(tf._raw(self._gates([inputs, state])))
                r, u = value[:, :self._num_units], value[:, self._num_units:]
                r_state = tf.T(r * tf._raw(state))
                if self._candidate is None:
                    with tf.variable_scope("candidate"):
                        self._candidate = _Linear([inputs, r_state], self._num_units, True)
                c = torch.tanh(tf._raw(self._candidate([inputs, r_state])))
            new_h = tf.T(u * tf._raw(state) + (1 - u) * c)
            return new_h, new_h

    def dynamic_rnn(cell, inputs, att_scores=None, sequence_length=None, initial_state=None, dtype=None, scope=None, **_kw):
        x = tf._raw(inputs)
        B, T_, _ = x.shape
        att = None if att_scores is None else tf._raw(att_scores)
        L = None if sequence_length is None else tf._raw(sequence_length).reshape(-1).to(torch.int64)
        with tf.variable_scope(scope or "rnn"):
            state = initial_state if initial_state is not None else cell.zero_state(B, dtype)
            outputs = []
            for t in range(T_):
                step = tf.T(x[:, t])
                out, new = cell(step, state) if att is None else cell(step, state, tf.T(att[:, t]))
                if L is not None:
                    done = (t >= L)[:, None]
                    out = tf.T(torch.where(done, torch.zeros_like(tf._raw(out)), tf._raw(out)))
                    new = tf.T(torch.where(done, tf._raw(state), tf._raw(new)))
                outputs.append(tf._raw(out))
                state = new
        stacked = torch.stack(outputs, dim=1) if outputs else x.new_zeros(B, 0, cell.output_size)
        return tf.T(stacked), state

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    ops = module("tensorflow.python.ops",
                 math_ops=module("tensorflow.python.ops.math_ops", sigmoid=tf.sigmoid, tanh=lambda x, name=None: tf.T(torch.tanh(tf._raw(x)))),
                 init_ops=module("tensorflow.python.ops.init_ops", constant_initializer=lambda value=0, dtype=None: tf.constant_initializer(value)),
                 array_ops=module("tensorflow.python.ops.array_ops",
                                  split=lambda value, num_or_size_splits, axis=0: [tf.T(p) for p in torch.chunk(tf._raw(value), num_or_size_splits, dim=axis)]),
                 variable_scope=module("tensorflow.python.ops.variable_scope", variable_scope=tf.variable_scope),
                 rnn_cell=module("tensorflow.python.ops.rnn_cell", RNNCell=RNNCell, LayerRNNCell=RNNCell))
    module("tensorflow.python", ops=ops)
    module("tensorflow.contrib.rnn.python.ops.core_rnn_cell", _Linear=_Linear)
    module("rnn", dynamic_rnn=dynamic_rnn)
    tf.nn.rnn_cell = types.SimpleNamespace(GRUCell=GRUCell)
    tf.contrib.opt = types.SimpleNamespace(LazyAdamOptimizer=tf.train.AdamOptimizer)
    tf.compat.v1.logging = types.SimpleNamespace(set_verbosity=lambda *_: None, ERROR=40, INFO=20)


def one(tf, m, name, overrides, sfeats, dense, labels, seed):
    dense_c, cat, tgt, seq, neg, _label = m.create_feature_columns()
    F = m.FLAGS
    params = {"dense_feature_columns": dense_c, "category_feature_columns": cat, "sequence_feature_columns": seq,
              "negative_sequence_feature_columns": neg, "target_feedid_feature_columns": tgt,
              "hidden_units": F.hidden_units.split(","), "dropout_rate": F.dropout_rate, "batch_norm": F.batch_norm,
              "learning_rate": F.learning_rate, "activation": F.activation, "use_auxiliary_loss": F.use_auxiliary_loss,
              "negative_sample_number": F.negative_sample_number, "custom_gru_type": F.custom_gru_type,
              "gru_output_units": F.gru_output_units}
    feats = {}
    for c in dense_c + cat + tgt + seq:
        if c.key in sfeats:
            feats[c.key] = sfeats[c.key]
        elif c.key in G.DENSE:
            feats[c.key] = tf.T(torch.from_numpy(dense[:, G.DENSE.index(c.key)].reshape(-1, 1).copy()))
    M = tf.estimator.ModeKeys
    d = {}
    tf.reset_default_graph(seed=seed)                 # PREDICT on a fresh graph; variables are created here
    spec = m.dien_model_fn(feats, None, M.PREDICT, params)
    g = tf.get_default_graph()
    for vn, var in g.vars.items():
        d[f"var/{vn}"] = G._np(var).copy()
    for k, v in spec.predictions.items():
        d[f"predict/{k}"] = G._np(v)
    g.uid.clear(); g.collections.clear(); g.scope.clear()          # TRAIN on the same variables
    lab = {"read_comment": tf.T(torch.from_numpy(labels.copy()))}
    spec = m.dien_model_fn(feats, lab, M.TRAIN, params)
    d["train/loss"] = G._np(spec.loss)
    for i, mk in enumerate(g.collections.get("__dropout_masks__", [])):
        d[f"aux/dropout_mask_{i}"] = mk.numpy().copy()
    grads = spec.train_op.run()
    for vn, gv in grads.items():
        d[f"grad/{vn}"] = G._np(gv)
    for vn, var in g.vars.items():
        d[f"var_after/{vn}"] = G._np(var).copy()
    g.uid.clear(); g.collections.clear(); g.scope.clear()          # EVAL after the step
    spec = m.dien_model_fn(feats, lab, M.EVAL, params)
    d["eval/loss"] = G._np(spec.loss)
    d["eval/accuracy"] = G._np(spec.eval_metric_ops["eval_accuracy"][0])
    d["eval/auc"] = G._np(spec.eval_metric_ops["eval_auc"][0])
    for k, v in overrides.items():
        d[f"flag/{k}"] = np.asarray(v)
    d["meta/learning_rate"] = np.asarray(params["learning_rate"])
    d["meta/seed"] = np.asarray(seed)
    return d


def generate():
    tf = G._use_shim()
    extend_shim(tf)
    out = {}
    sfeats, dense, labels = G.make_batch(48, seed=77)
    with tempfile.TemporaryDirectory() as vd:
        vocab_dir = os.path.join(vd, "vocabulary") + "/"
        G.write_vocab_dir(vocab_dir)
        for name, overrides in CONFIGS.items():
            sys.modules.pop("custom_grucell", None)
            m = G._import_ref("DIEN", "dien")
            for k, v in overrides.items():
                setattr(m.FLAGS, k, v)
            m.FLAGS.vocabulary_dir = vocab_dir
            for seed in range(4242, 4262):
                d = one(tf, m, name, overrides, sfeats, dense, labels, seed)
                if all(np.any(v) for k, v in d.items() if k.startswith("grad/")):
                    break
            else:
                raise SystemExit(f"{name}: an all-zero gradient with every seed tried")
            out[name] = d
    return out


def main():
    if not os.path.isdir(os.path.join(G.REF, "DIEN")):
        raise SystemExit("gen_golden_dien.py needs the reference folder (authoring container only)")
    check = "--check" in sys.argv[1:]
    allg = generate()
    bad = []
    for name, d in allg.items():
        path = os.path.join(G.OUT, name + ".npz")
        if check:
            old = dict(np.load(path, allow_pickle=False))
            if sorted(old) != sorted(d):
                bad.append(f"{name}: key sets differ")
                continue
            for k in d:
                a, b = np.asarray(d[k]), old[k]
                if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
                    bad.append(f"{name}: {k} differs")
            print(f"[golden] {name}.npz  checked ({len(d)} arrays)")
        else:
            np.savez_compressed(path, **d)
            print(f"[golden] {name}.npz  ({len(d)} arrays, seed {int(d['meta/seed'])})")
    if bad:
        raise SystemExit("\n".join(bad))


if __name__ == "__main__":
    main()
