"""Generate tests/golden/model_ple.npz and tests/golden/model_ple_two_levels_dropout.npz by executing the reference's own,
unmodified algorithm/PLE/ple.py (and its extraction_network.py) against oracle/tf1_shim — the PLE sibling of
scripts/gen_golden_mmoe.py (same B = 48 batch, same labels, same key scheme), kept outside the frozen oracle/ folder.
Unequal expert counts per task (2, 1, 3 + 2 shared) so that an ordering mistake of the mirror cannot cancel.

    python scripts/gen_golden_ple.py            # rewrites the two files
    python scripts/gen_golden_ple.py --check    # regenerates in memory, compares bit for bit with the committed files

Runs only where the reference folder exists (oracle.gen_golden.REF); the tests use the committed .npz files.  Keys:
  var/<name>, predict/<task>_probabilities, train/loss, grad/<name>, var_after/<name>, aux/dropout_mask_<i> (call order),
  eval/loss, eval/<task>_accuracy, eval/<task>_auc, in/label_<task> (the labels of the tasks the shared batch does not
  carry, from a seeded generator), flag/<flag>, meta/learning_rate.
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

TASKS = ["read_comment", "like", "click_avatar"]
FLAGS = dict(hidden_units="16,8", learning_rate=0.005, batch_norm=True, num_tasks=3, expert_hidden_units=12,
             num_experts_per_task="2,1,3", num_experts_in_shared=2, task_names=",".join(TASKS))
CONFIGS = {"model_ple": dict(FLAGS, num_extract_network=1, dropout_rate=0.0),                  # ple.py:45: one level
           "model_ple_two_levels_dropout": dict(FLAGS, num_extract_network=2, dropout_rate=0.1)}   # level 1: In == H


def generate():
    tf = G._use_shim()
    tf.newaxis = None                      # (the one name ple.py:193 uses that the shim does not define)
    out = {}
    B = 48
    sfeats, dense, labels = G.make_batch(B, seed=77)
    rng = np.random.default_rng(7707)
    task_labels = {"read_comment": labels}
    for t in TASKS[1:]:
        task_labels[t] = (rng.random((B, 1)) < 0.3).astype(np.float64)
    with tempfile.TemporaryDirectory() as vd:
        vocab_dir = os.path.join(vd, "vocabulary") + "/"
        G.write_vocab_dir(vocab_dir)
        for name, overrides in CONFIGS.items():
            m = G._import_ref("PLE", "ple")
            for k, v in overrides.items():
                setattr(m.FLAGS, k, v)
            m.FLAGS.vocabulary_dir = vocab_dir
            dense_c, cat, _label = m.create_feature_columns()
            params = {"dense_feature_columns": dense_c, "category_feature_columns": cat,
                      "hidden_units": m.FLAGS.hidden_units.split(","), "dropout_rate": m.FLAGS.dropout_rate,
                      "batch_norm": m.FLAGS.batch_norm, "learning_rate": m.FLAGS.learning_rate,
                      "num_tasks": m.FLAGS.num_tasks, "expert_hidden_units": m.FLAGS.expert_hidden_units,
                      "task_names": m.FLAGS.task_names.split(","), "num_extract_network": m.FLAGS.num_extract_network,
                      "num_experts_per_task": [int(x) for x in m.FLAGS.num_experts_per_task.split(",")],
                      "num_experts_in_shared": m.FLAGS.num_experts_in_shared}
            feats = {}
            for c in dense_c + cat:
                if c.key in sfeats:
                    feats[c.key] = sfeats[c.key]
                elif c.key in G.DENSE:
                    feats[c.key] = tf.T(torch.from_numpy(dense[:, G.DENSE.index(c.key)].reshape(-1, 1).copy()))
            M = tf.estimator.ModeKeys
            d = {}
            tf.reset_default_graph(seed=4242)                 # PREDICT on a fresh graph; variables are created here
            spec = m.ple_model_fn(feats, None, M.PREDICT, params)
            g = tf.get_default_graph()
            for vn, var in g.vars.items():
                d[f"var/{vn}"] = G._np(var).copy()
            for k, v in spec.predictions.items():
                d[f"predict/{k}"] = G._np(v)
            g.uid.clear(); g.collections.clear(); g.scope.clear()          # TRAIN on the same variables
            lab = {t: tf.T(torch.from_numpy(task_labels[t].copy())) for t in TASKS}
            spec = m.ple_model_fn(feats, lab, M.TRAIN, params)
            d["train/loss"] = G._np(spec.loss)
            for i, mk in enumerate(g.collections.get("__dropout_masks__", [])):
                d[f"aux/dropout_mask_{i}"] = mk.numpy().copy()
            grads = spec.train_op.run()
            for vn, gv in grads.items():
                d[f"grad/{vn}"] = G._np(gv)
            for vn, var in g.vars.items():
                d[f"var_after/{vn}"] = G._np(var).copy()
            g.uid.clear(); g.collections.clear(); g.scope.clear()          # EVAL after the step
            spec = m.ple_model_fn(feats, lab, M.EVAL, params)
            d["eval/loss"] = G._np(spec.loss)
            for t in TASKS:
                d[f"eval/{t}_accuracy"] = G._np(spec.eval_metric_ops[f"eval_{t}_accuracy"][0])
                d[f"eval/{t}_auc"] = G._np(spec.eval_metric_ops[f"eval_{t}_auc"][0])
            for t in TASKS[1:]:
                d[f"in/label_{t}"] = task_labels[t]
            for k, v in overrides.items():
                d[f"flag/{k}"] = np.asarray(v)
            d["meta/learning_rate"] = np.asarray(params["learning_rate"])
            out[name] = d
    return out


def main():
    if not os.path.isdir(G.REF):
        raise SystemExit("gen_golden_ple.py needs the reference folder (authoring container only)")
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
