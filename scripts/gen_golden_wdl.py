"""Generate tests/golden/model_wdl.npz and tests/golden/model_wdl_dropout.npz by executing the reference's own, unmodified
algorithm/WideAndDeep/wide_and_deep.py against oracle/tf1_shim — the Wide&Deep sibling of scripts/gen_golden_ple.py (same
B = 48 batch, same labels, same key scheme), kept outside the frozen oracle/ folder.

    python scripts/gen_golden_wdl.py            # rewrites the two files
    python scripts/gen_golden_wdl.py --check    # regenerates in memory, compares bit for bit with the committed files

The names wide_and_deep.py uses that the shim does not define are added HERE, to the imported shim module (oracle/ is left
untouched): fc.crossed_column and an indicator over it, tf.train.FtrlOptimizer, minimize(var_list=), tf.get_collection by
scope over TRAINABLE_VARIABLES, tf.group, tf.norm, tf.summary.histogram.

THE HASH AND FTRL BELOW ARE RESTATEMENTS, NOT TENSORFLOW.  The cross hash (sparse_cross_op.cc HashCrosser on int64 ids with
fingerprint.h FingerprintCat64 and hash_key 0xDECAFCAFFE) and ApplyFtrl (initial_accumulator_value 0.1, l1 = l2 = 0,
lr_power -0.5) are written from knowledge of the TF 1.14 sources; no TensorFlow exists where this runs to confirm them.
What the goldens pin is the reference's COMPOSITION: which columns are crossed, the dense update of every bucket by FTRL
(so: untouched buckets are zeroed by the first step), Adam on the deep part only, one backward pass.

hash_bucket_size is overridden to 64 (the reference hard-codes 100000): the goldens stay small and buckets collide.
Keys: var/<name>, predict/probabilities, train/loss, grad/<name>, var_after/<name>, slot/<name>/Ftrl (accum) and
slot/<name>/Ftrl_1 (linear) after the step, aux/dropout_mask_<i> (call order), eval/loss, eval/accuracy, eval/auc,
flag/<flag>, meta/hash_bucket_size, meta/wide_part_learning_rate, meta/deep_part_learning_rate.
"""
from __future__ import annotations

import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

HASH_BUCKET_SIZE = 64
FLAGS = dict(hidden_units="16,8", batch_norm=True, wide_part_learning_rate=0.005, deep_part_learning_rate=0.001,
             deep_part_optimizer="Adam")
CONFIGS = {"model_wdl": dict(FLAGS, dropout_rate=0.0), "model_wdl_dropout": dict(FLAGS, dropout_rate=0.1)}

_MASK = (1 << 64) - 1
_KMUL = 0xc6a4a7935bd1e995


def _cat64(a, b):
    sm = lambda v: v ^ (v >> 47)
    r = a ^ _KMUL
    r ^= (sm((b * _KMUL) & _MASK) * _KMUL) & _MASK
    r = (r * _KMUL) & _MASK
    r = (sm(r) * _KMUL) & _MASK
    return sm(r)


def extend_shim(tf):
    """Add the names listed in the module docstring to the imported shim."""
    fc = tf.feature_column

    class _Crossed:
        """crossed_column over two vocabulary columns: one cross per pair of the example's ids, -1 (OOV) crossed as
        0xFFFFFFFFFFFFFFFF; behaves as a categorical column of hash_bucket_size buckets for the shim's indicator"""

        def __init__(self, keys, hash_bucket_size, hash_key=None):
            self.keys = list(keys)
            self.num_buckets = int(HASH_BUCKET_SIZE)
            self.hash_key = 0xDECAFCAFFE if hash_key is None else int(hash_key)
            self.key = self.name = "_X_".join(sorted(k.name for k in self.keys))

        def ids(self, features):
            a, b = (k.ids(features) for k in self.keys)
            return [[_cat64(_cat64(self.hash_key, u & _MASK), t & _MASK) % self.num_buckets for u in ua for t in tb]
                    for ua, tb in zip(a, b)]

    fc.crossed_column = lambda keys, hash_bucket_size, hash_key=None: _Crossed(keys, hash_bucket_size, hash_key)
    tf.GraphKeys.TRAINABLE_VARIABLES = "trainable_variables"
    shim_get_collection = tf.get_collection

    def get_collection(key, scope=None):
        if key == tf.GraphKeys.TRAINABLE_VARIABLES:
            # (TF variable names end in ":0", and wide_and_deep.py:281-285 compares them so: views named that way)
            return [tf.T(v.t, name=n + ":0") for n, v in tf.get_default_graph().vars.items()
                    if v.trainable and (scope is None or n.startswith(scope))]
        return shim_get_collection(key, scope)
    tf.get_collection = get_collection
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))     # TF keeps hyper-parameters as float32

    class _Op:
        def __init__(self, opt, loss, var_list):
            self.opt, self.loss = opt, loss
            gv = tf.get_default_graph().vars
            self.var_list = [v for v in gv.values() if v.trainable] if var_list is None else \
                [gv[v.name.split(":")[0]] for v in var_list]

    class Adam:
        def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, **_kw):
            self.lr, self.beta1, self.beta2, self.eps = learning_rate, beta1, beta2, epsilon
            self.step, self.m, self.v = 0, {}, {}

        def minimize(self, loss, global_step=None, var_list=None, **_kw):
            return _Op(self, loss, var_list)

        def apply(self, var_list, grads):
            self.step += 1
            lr, b1, b2, eps = f32(self.lr), f32(self.beta1), f32(self.beta2), f32(self.eps)
            lr_t = lr * math.sqrt(1 - b2 ** self.step) / (1 - b1 ** self.step)
            with torch.no_grad():
                for v in var_list:
                    g = grads[v.name]
                    m = self.m.setdefault(v.name, torch.zeros_like(v.t))
                    s = self.v.setdefault(v.name, torch.zeros_like(v.t))
                    m.mul_(b1).add_(g * (1 - b1))
                    s.mul_(b2).add_(g * g * (1 - b2))
                    v.t.sub_(lr_t * m / (s.sqrt() + eps))

    class Ftrl:
        """ApplyFtrl, lr_power = -0.5, on every variable of var_list, DENSELY (the reference's wide gradient is dense)"""

        def __init__(self, learning_rate, initial_accumulator_value=0.1, l1_regularization_strength=0.0,
                     l2_regularization_strength=0.0, **_kw):
            self.lr, self.init, self.l1, self.l2 = learning_rate, initial_accumulator_value, l1_regularization_strength, l2_regularization_strength
            self.accum, self.linear = {}, {}

        def minimize(self, loss, global_step=None, var_list=None, **_kw):
            return _Op(self, loss, var_list)

        def apply(self, var_list, grads):
            lr, l1, l2 = f32(self.lr), f32(self.l1), f32(self.l2)
            with torch.no_grad():
                for v in var_list:
                    g = grads[v.name]
                    accum = self.accum.setdefault(v.name, torch.full_like(v.t, f32(self.init)))
                    linear = self.linear.setdefault(v.name, torch.zeros_like(v.t))
                    new_accum = accum + g * g
                    linear.add_(g - (new_accum.sqrt() - accum.sqrt()) / lr * v.t)
                    quad = new_accum.sqrt() / lr + 2 * l2
                    v.t.copy_(torch.where(linear.abs() > l1, (torch.sign(linear) * l1 - linear) / quad, torch.zeros_like(linear)))
                    accum.copy_(new_accum)

    class _Group:
        """tf.group of minimize ops over ONE loss: one backward pass, UPDATE_OPS, then every optimizer on its var_list"""

        def __init__(self, *ops):
            self.ops = ops

        def run(self):
            g = tf.get_default_graph()
            tv = [v for v in g.vars.values() if v.trainable]
            for v in tv:
                v.t.grad = None
            tf._raw(self.ops[0].loss).backward()
            grads = {v.name: (torch.zeros_like(v.t) if v.t.grad is None else v.t.grad.clone()) for v in tv}
            for u in g.collections[tf.GraphKeys.UPDATE_OPS]:
                u()
            claimed = [v.name for op in self.ops for v in op.var_list]
            assert sorted(claimed) == sorted(v.name for v in tv), "the optimizers' var_lists do not partition the variables"
            for op in self.ops:
                op.opt.apply(op.var_list, grads)
            return grads

    tf.train.AdamOptimizer, tf.train.FtrlOptimizer = Adam, Ftrl
    tf.group = lambda *ops, **_kw: _Group(*ops)
    tf.norm = lambda x, **_kw: tf.T(tf._raw(x).norm())
    tf.summary.histogram = lambda *a, **k: None
    return Ftrl


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
            m = G._import_ref("WideAndDeep", "wide_and_deep")
            for k, v in overrides.items():
                setattr(m.FLAGS, k, v)
            m.FLAGS.vocabulary_dir = vocab_dir
            wide_c, deep_c = m.create_feature_columns()
            params = {"wide_part_feature_columns": wide_c, "deep_part_feature_columns": deep_c,
                      "hidden_units": m.FLAGS.hidden_units.split(","), "dropout_rate": m.FLAGS.dropout_rate,
                      "batch_norm": m.FLAGS.batch_norm, "deep_part_optimizer": m.FLAGS.deep_part_optimizer,
                      "wide_part_learning_rate": m.FLAGS.wide_part_learning_rate,
                      "deep_part_learning_rate": m.FLAGS.deep_part_learning_rate}
            feats = {}
            keys = [c.key for c in deep_c] + [k.key for c in wide_c for k in c.categorical_column.keys]
            for key in keys:
                if key in sfeats:
                    feats[key] = sfeats[key]
                elif key in G.DENSE:
                    feats[key] = tf.T(torch.from_numpy(dense[:, G.DENSE.index(key)].reshape(-1, 1).copy()))
            M = tf.estimator.ModeKeys
            d = {}
            tf.reset_default_graph(seed=4242)                 # PREDICT on a fresh graph; variables are created here
            spec = m.wide_and_deep_model_fn(feats, None, M.PREDICT, params)
            g = tf.get_default_graph()
            for vn, var in g.vars.items():
                d[f"var/{vn}"] = G._np(var).copy()
            for k, v in spec.predictions.items():
                d[f"predict/{k}"] = G._np(v)
            g.uid.clear(); g.collections.clear(); g.scope.clear()          # TRAIN on the same variables
            lab = {"read_comment": tf.T(torch.from_numpy(labels.copy()))}
            spec = m.wide_and_deep_model_fn(feats, lab, M.TRAIN, params)
            d["train/loss"] = G._np(spec.loss)
            for i, mk in enumerate(g.collections.get("__dropout_masks__", [])):
                d[f"aux/dropout_mask_{i}"] = mk.numpy().copy()
            grads = spec.train_op.run()
            for vn, gv in grads.items():
                d[f"grad/{vn}"] = G._np(gv)
            for vn, var in g.vars.items():
                d[f"var_after/{vn}"] = G._np(var).copy()
            ftrl = [op.opt for op in spec.train_op.ops if hasattr(op.opt, "accum")]
            assert len(ftrl) == 1
            for vn in ftrl[0].accum:
                d[f"slot/{vn}/Ftrl"] = ftrl[0].accum[vn].numpy().copy()
                d[f"slot/{vn}/Ftrl_1"] = ftrl[0].linear[vn].numpy().copy()
            g.uid.clear(); g.collections.clear(); g.scope.clear()          # EVAL after the step
            spec = m.wide_and_deep_model_fn(feats, lab, M.EVAL, params)
            d["eval/loss"] = G._np(spec.loss)
            d["eval/accuracy"] = G._np(spec.eval_metric_ops["eval_accuracy"][0])
            d["eval/auc"] = G._np(spec.eval_metric_ops["eval_auc"][0])
            for k, v in overrides.items():
                d[f"flag/{k}"] = np.asarray(v)
            d["meta/hash_bucket_size"] = np.asarray(HASH_BUCKET_SIZE)
            d["meta/wide_part_learning_rate"] = np.asarray(params["wide_part_learning_rate"])
            d["meta/deep_part_learning_rate"] = np.asarray(params["deep_part_learning_rate"])
            out[name] = d
    return out


def main():
    if not os.path.isdir(G.REF):
        raise SystemExit("gen_golden_wdl.py needs the reference folder (authoring container only)")
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
