"""Generate tests/golden/model_bst.npz and tests/golden/model_bst_two_blocks_mean_dropout.npz by executing the reference's
own, unmodified algorithm/BST/bst.py (with its transformer_layer.py and leakyrelu.py) against oracle/tf1_shim — the BST
sibling of scripts/gen_golden_wdl.py (same B = 48 batch: history lengths 0..8, one empty history, OOV ids; same labels, same
key scheme), kept outside the frozen oracle/ folder.

    python scripts/gen_golden_bst.py            # rewrites the two files
    python scripts/gen_golden_bst.py --check    # regenerates in memory, compares bit for bit with the committed files

The names bst.py uses that the shim does not define are added HERE, to the imported shim module (oracle/ is left
untouched): tf.range, tf.abs, tf.nn.embedding_lookup, tf.contrib.layers.layer_norm, a tf.sequence_mask that honours a float
dtype, and a tf.nn.softmax that models the float32 mask add (below).

LAYER_NORM BELOW IS A RESTATEMENT, NOT TENSORFLOW.  tf.contrib.layers.layer_norm's defaults (begin_norm_axis=1: moments per
example over the whole [T, d] block; begin_params_axis=-1: gamma and beta of shape [d]; variance epsilon 1e-12; variables
<scope>/LayerNorm[_n]/{beta, gamma}; tf.nn.moments and tf.nn.batch_normalization arithmetic) are written from knowledge of
the TF 1.15 sources; no TensorFlow exists where this runs to confirm them.

THE MASK.  transformer_layer.py:53-61 adds float32(-2**32 + 1) = -4294967296.0 to every score of the QUERY rows >=
keys_length.  In TensorFlow's float32 that add absorbs the score (every |s| < 128 is below half an ulp of 2**32): the row
becomes a constant, its softmax exactly uniform, and the add's gradient — the identity — still reaches the scores.  The shim
computes in float64, where the same add keeps the score (softmax is shift invariant: the row would come out as if it were
not masked at all).  So the softmax installed here replaces every row whose entries are all below -2**31 by the constant
-4294967296.0 with a straight-through gradient, `c + (x - x.detach())`: the float32 step, in float64.  tests/bst_ref.py
states the same rule and tests/test_bst_host.py checks it against torch's own float32 arithmetic.

Keys: var/<name>, predict/probabilities, train/loss, grad/<name>, var_after/<name>, aux/dropout_mask_<i> (call order),
eval/loss, eval/accuracy, eval/auc, flag/<flag>, meta/learning_rate.
"""
from __future__ import annotations

import builtins
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

FLAGS = dict(hidden_units="16,8", learning_rate=0.005, batch_norm=True, sequence_max_length=50, num_transformer_heads=3)
CONFIGS = {"model_bst": dict(FLAGS, num_transformer_block=1, pooling_method="sum", dropout_rate=0.0),
           "model_bst_two_blocks_mean_dropout": dict(FLAGS, num_transformer_block=2, pooling_method="mean", dropout_rate=0.1)}
MASK_ADD = -4294967296.0        # float32(-2 ** 32 + 1)


def extend_shim(tf):
    """Add the names listed in the module docstring to the imported shim."""
    # tf.range and tf.abs become attributes of the shim MODULE, whose own code calls the builtins of the same names: both stay
    # usable as those (a _Range iterates as Python ints, abs of a plain number is the builtin's)
    class _Range(tf.T):
        def __iter__(self):
            return iter(self.t.tolist())

        def __len__(self):
            return int(self.t.numel())
    tf.range = lambda *a, **_kw: _Range(torch.arange(*[tf._int(v) for v in a]))
    tf.abs = lambda x, name=None: tf.T(tf._raw(x).abs()) if isinstance(x, (tf.T, torch.Tensor)) else builtins.abs(x)
    tf.nn.embedding_lookup = lambda params, ids, **_kw: tf.T(tf._raw(params)[tf._raw(ids)])

    shim_sequence_mask = tf.sequence_mask

    def sequence_mask(lengths, maxlen=None, dtype=None):
        """the shim's mask is boolean whatever `dtype`; transformer_layer.py:53-55 does arithmetic on a float one"""
        mask = shim_sequence_mask(lengths, maxlen)
        return tf.cast(mask, dtype) if dtype in (tf.float32, tf.float64) else mask
    tf.sequence_mask = sequence_mask

    def softmax(x, axis=-1, name=None):
        x = tf._raw(x)
        assert int(axis) in (-1, x.dim() - 1)
        masked = (x < -2.0 ** 31).all(dim=-1, keepdim=True)
        assert bool(((x < -2.0 ** 31).any(dim=-1, keepdim=True) == masked).all()), "a row is masked as a whole or not at all"
        x = torch.where(masked, MASK_ADD + (x - x.detach()), x)
        return tf.T(torch.softmax(x, dim=-1))
    tf.nn.softmax = softmax

    def layer_norm(inputs, center=True, scale=True, begin_norm_axis=1, begin_params_axis=-1, scope=None, **_kw):
        x = tf._raw(inputs)
        assert center and scale and begin_norm_axis == 1 and begin_params_axis == -1
        d = x.shape[-1]
        with tf.variable_scope(scope, default_name="LayerNorm"):
            beta = tf.get_variable("beta", (d,), initializer=tf.zeros_initializer())
            gamma = tf.get_variable("gamma", (d,), initializer=tf.ones_initializer())
        axes = tuple(range(1, x.dim()))
        mean = x.mean(dim=axes, keepdim=True)                            # tf.nn.moments
        var = ((x - mean) ** 2).mean(dim=axes, keepdim=True)
        inv = torch.rsqrt(var + 1e-12) * gamma.t                         # tf.nn.batch_normalization
        return tf.T(x * inv + (beta.t - mean * inv))
    tf.contrib.layers.layer_norm = layer_norm


def generate():
    tf = G._use_shim()
    extend_shim(tf)
    out = {}
    B = 48
    sfeats, dense, labels = G.make_batch(B, seed=77)
    with tempfile.TemporaryDirectory() as vd:
        vocab_dir = os.path.join(vd, "vocabulary") + "/"
        G.write_vocab_dir(vocab_dir)
        for name, overrides in CONFIGS.items():
            for stale in ("transformer_layer", "leakyrelu"):
                sys.modules.pop(stale, None)
            m = G._import_ref("BST", "bst")
            for k, v in overrides.items():
                setattr(m.FLAGS, k, v)
            m.FLAGS.vocabulary_dir = vocab_dir
            dense_c, cat, tgt, seq, _label = m.create_feature_columns()
            F = m.FLAGS
            params = {"dense_feature_columns": dense_c, "category_feature_columns": cat, "sequence_feature_columns": seq,
                      "target_feedid_feature_columns": tgt, "hidden_units": F.hidden_units.split(","),
                      "dropout_rate": F.dropout_rate, "batch_norm": F.batch_norm, "learning_rate": F.learning_rate,
                      "sequence_max_length": F.sequence_max_length, "num_transformer_block": F.num_transformer_block,
                      "num_transformer_heads": F.num_transformer_heads, "pooling_method": F.pooling_method}
            feats = {}
            for c in dense_c + cat + tgt + seq:
                if c.key in sfeats:
                    feats[c.key] = sfeats[c.key]
                elif c.key in G.DENSE:
                    feats[c.key] = tf.T(torch.from_numpy(dense[:, G.DENSE.index(c.key)].reshape(-1, 1).copy()))
            M = tf.estimator.ModeKeys
            d = {}
            tf.reset_default_graph(seed=4242)                 # PREDICT on a fresh graph; variables are created here
            spec = m.bst_model_fn(feats, None, M.PREDICT, params)
            g = tf.get_default_graph()
            for vn, var in g.vars.items():
                d[f"var/{vn}"] = G._np(var).copy()
            for k, v in spec.predictions.items():
                d[f"predict/{k}"] = G._np(v)
            g.uid.clear(); g.collections.clear(); g.scope.clear()          # TRAIN on the same variables
            lab = {"read_comment": tf.T(torch.from_numpy(labels.copy()))}
            spec = m.bst_model_fn(feats, lab, M.TRAIN, params)
            d["train/loss"] = G._np(spec.loss)
            for i, mk in enumerate(g.collections.get("__dropout_masks__", [])):
                d[f"aux/dropout_mask_{i}"] = mk.numpy().copy()
            grads = spec.train_op.run()
            for vn, gv in grads.items():
                d[f"grad/{vn}"] = G._np(gv)
            for vn, var in g.vars.items():
                d[f"var_after/{vn}"] = G._np(var).copy()
            g.uid.clear(); g.collections.clear(); g.scope.clear()          # EVAL after the step
            spec = m.bst_model_fn(feats, lab, M.EVAL, params)
            d["eval/loss"] = G._np(spec.loss)
            d["eval/accuracy"] = G._np(spec.eval_metric_ops["eval_accuracy"][0])
            d["eval/auc"] = G._np(spec.eval_metric_ops["eval_auc"][0])
            for k, v in overrides.items():
                d[f"flag/{k}"] = np.asarray(v)
            d["meta/learning_rate"] = np.asarray(params["learning_rate"])
            out[name] = d
    return out


def main():
    if not os.path.isdir(G.REF):
        raise SystemExit("gen_golden_bst.py needs the reference folder (authoring container only)")
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
            print(f"[golden] {name}.npz  ({len(d)} arrays)")
    if bad:
        raise SystemExit("\n".join(bad))


if __name__ == "__main__":
    main()
