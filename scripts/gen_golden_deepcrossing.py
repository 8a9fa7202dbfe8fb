"""Generate tests/golden/model_deepcrossing.npz and tests/golden/model_deepcrossing_three_units.npz by executing the
reference's own, unmodified algorithm/DeepCrossing/deepcrossing.py (with its residual_unit.py) against oracle/tf1_shim — the
DeepCrossing sibling of scripts/gen_golden_bst.py (same B = 48 batch, same labels, same key scheme), kept outside the frozen
oracle/ folder.  The script uses nothing the shim lacks.

    python scripts/gen_golden_deepcrossing.py            # rewrites the two files
    python scripts/gen_golden_deepcrossing.py --check    # regenerates in memory, compares bit for bit with the committed files

THE RELU MARGIN.  The run is float64; a kernel evaluates the same pre-activations in float32, within about 1e-6 of their
scale.  An element that close to zero could take the other side of a ReLU on the GPU and move a gradient by O(|g|): such a
golden would test the initialiser's seed, not the kernel.  So the generator records the input of every tf.nn.relu call of
the PREDICT and TRAIN runs (2 L per run: residual_unit.py:18 and :20) and asserts that none lies within MARGIN x (the
largest |pre-activation| of that call) of zero; a seed that violates it is passed over for the next one, and the seed a
golden was made with is part of it (meta/seed).

Keys: var/<name>, predict/{logit, probabilities}, train/loss, grad/<name>, var_after/<name>, eval/loss, eval/accuracy,
eval/auc, flag/<flag>, meta/learning_rate, meta/seed, meta/relu_margin (the smallest |pre-activation| / largest of a call).
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

CONFIGS = {"model_deepcrossing": dict(learning_rate=0.005, residual_network_num=1, residual_internal_dim=128),
           "model_deepcrossing_three_units": dict(learning_rate=0.005, residual_network_num=3, residual_internal_dim=32)}
FIRST_SEED, SEEDS = 4242, 16
MARGIN = 2e-5


def run(tf, m, params, feats, labels, seed):
    """PREDICT, TRAIN (one Adam step), EVAL of the reference's model_fn on a graph seeded with `seed`
    -> (the golden's arrays, the smallest relative |pre-activation| of a ReLU call)"""
    M = tf.estimator.ModeKeys
    pre = []
    shim_relu = tf.nn.relu

    def relu(x, name=None):
        pre.append(tf._raw(x).detach().clone())
        return shim_relu(x)
    tf.nn.relu = relu
    try:
        d = {}
        tf.reset_default_graph(seed=seed)                     # PREDICT on a fresh graph; variables are created here
        spec = m.deepcrossing_model_fn(feats, None, M.PREDICT, params)
        g = tf.get_default_graph()
        for vn, var in g.vars.items():
            d[f"var/{vn}"] = G._np(var).copy()
        for k, v in spec.predictions.items():
            d[f"predict/{k}"] = G._np(v)
        g.uid.clear(); g.collections.clear(); g.scope.clear()          # TRAIN on the same variables
        lab = {"read_comment": tf.T(torch.from_numpy(labels.copy()))}
        spec = m.deepcrossing_model_fn(feats, lab, M.TRAIN, params)
        d["train/loss"] = G._np(spec.loss)
        n_train = len(pre)
        grads = spec.train_op.run()
        for vn, gv in grads.items():
            d[f"grad/{vn}"] = G._np(gv)
        for vn, var in g.vars.items():
            d[f"var_after/{vn}"] = G._np(var).copy()
        g.uid.clear(); g.collections.clear(); g.scope.clear()          # EVAL after the step
        spec = m.deepcrossing_model_fn(feats, lab, M.EVAL, params)
        d["eval/loss"] = G._np(spec.loss)
        d["eval/accuracy"] = G._np(spec.eval_metric_ops["eval_accuracy"][0])
        d["eval/auc"] = G._np(spec.eval_metric_ops["eval_auc"][0])
    finally:
        tf.nn.relu = shim_relu
    L = int(params["residual_network_num"])
    assert n_train == 4 * L and len(pre) == 6 * L, "two ReLU calls per unit and run"
    # (the EVAL run's calls are on the updated variables, which no kernel test evaluates a mask on: PREDICT and TRAIN only)
    margin = min(float(z.abs().min() / z.abs().max()) for z in pre[:n_train])
    return d, margin


def generate():
    tf = G._use_shim()
    out = {}
    sfeats, dense, labels = G.make_batch(48, seed=77)
    with tempfile.TemporaryDirectory() as vd:
        vocab_dir = os.path.join(vd, "vocabulary") + "/"
        G.write_vocab_dir(vocab_dir)
        for name, overrides in CONFIGS.items():
            sys.modules.pop("residual_unit", None)
            m = G._import_ref("DeepCrossing", "deepcrossing")
            for k, v in overrides.items():
                setattr(m.FLAGS, k, v)
            m.FLAGS.vocabulary_dir = vocab_dir
            dense_c, cat, _label = m.create_feature_columns()
            F = m.FLAGS
            params = {"category_feature_columns": cat, "dense_feature_columns": dense_c,
                      "residual_internal_dim": F.residual_internal_dim, "residual_network_num": F.residual_network_num,
                      "learning_rate": F.learning_rate}
            feats = {}
            for c in dense_c + cat:
                if c.key in sfeats:
                    feats[c.key] = sfeats[c.key]
                elif c.key in G.DENSE:
                    feats[c.key] = tf.T(torch.from_numpy(dense[:, G.DENSE.index(c.key)].reshape(-1, 1).copy()))
            for seed in range(FIRST_SEED, FIRST_SEED + SEEDS):
                d, margin = run(tf, m, params, feats, labels, seed)
                if margin > MARGIN:
                    break
                print(f"[golden] {name}: seed {seed} puts a pre-activation at {margin:.2e} of its layer's scale; next seed")
            else:
                raise SystemExit(f"{name}: no seed of {SEEDS} keeps every pre-activation {MARGIN} of its scale away from zero")
            for k, v in overrides.items():
                d[f"flag/{k}"] = np.asarray(v)
            d["meta/learning_rate"] = np.asarray(params["learning_rate"])
            d["meta/seed"] = np.asarray(seed)
            d["meta/relu_margin"] = np.asarray(margin)
            out[name] = d
    return out


def main():
    if not os.path.isdir(G.REF):
        raise SystemExit("gen_golden_deepcrossing.py needs the reference folder (authoring container only)")
    check = "--check" in sys.argv[1:]
    bad = []
    for name, d in generate().items():
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
            print(f"[golden] {name}.npz  ({len(d)} arrays, seed {int(d['meta/seed'])}, relu margin {float(d['meta/relu_margin']):.2e})")
    if bad:
        raise SystemExit("\n".join(bad))


if __name__ == "__main__":
    main()
