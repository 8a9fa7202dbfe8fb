"""AFM attention measurements on the MI355X: nn.afm_attention on the fused kernels (csrc/afm.hip) against the composed chain
(bilinear pair products, the dense engine on [B * P, K], the head, attention_pool), forward and forward + backward, and the
full captured AFM training step on both paths.  Self-contained: synthetic inputs from seeds, nothing read from outside the tree.
Prints one JSON line (and writes it with --out).

    python scripts/bench_afm.py [--replays 200] [--steps 200] [--out profiles/afm_bench.json]

op:    nn.afm_attention(fused=True / False) at (B 4096, F 26, K 16, t 128), bench.py --model afm's shape, and at one small
       shape (B 256, F 7, K 8, t 16): the forward under no_grad and forward + backward + the deferred weight-gradient sums
       (ops.flush_dense_splits; the fused path leaves none), each captured once; the graphs alternate in one process, medians
       over the replays.
step:  bench.py --model afm's estimator (26 fields x emb16, 16 dense features, attention factor 128, B 4096), captured
       (GraphedTrainStep), with params["afm_fused"] = None (the default: the kernels) and False (the composed chain: the step
       as it was before the kernels existed, the same code path).  Three runs of each, alternating; the median of each and the
       spread (max - min) of the composed step's three are reported, and `faster_than_spread` says whether the difference of
       the medians exceeds that spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_ple import _graph, _time_alternating  # noqa: E402


def bench_op(dev, B, F, K, t, replays):
    from recalgorithm_amd import nn, ops
    from recalgorithm_amd.variables import VariableStore, use_store
    gen = torch.Generator().manual_seed(1000 * F + 10 * K + t)
    fields = torch.randn(B, F * K, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(B, K, generator=gen).to(dev)
    store = VariableStore(dev, seed=3)
    with use_store(store):
        store.building = True
        w, b = store.get_variable("attention_w", (K, t)), store.get_variable("attention_b", (t,))
        h = store.get_variable("attention_h", (t, 1))
        store.finalize()
    with torch.no_grad():
        w.data.copy_(torch.randn(K, t, generator=gen) / K ** 0.5)
        b.data.copy_(torch.randn(t, generator=gen) * 0.3)
        h.data.copy_(torch.randn(t, 1, generator=gen) / t ** 0.5)

    def both(fused):
        def step():
            with use_store(store):
                store.begin_call()
                fields.grad = None
                out = nn.afm_attention(fields, F, K, w, b, h, fused=fused)
                out.backward(g)
                ops.flush_dense_splits()
            return out

        def forward():
            with use_store(store), torch.no_grad():
                store.begin_call()
                return nn.afm_attention(fields, F, K, w, b, h, fused=fused)
        return forward, step
    fns = [*both(True), *both(False)]                  # fused fwd, fused fwd+bwd, composed fwd, composed fwd+bwd
    outs = []
    for fn in (fns[1], fns[3]):
        o = fn().detach().clone()
        outs.append((o, fields.grad.clone(), w.grad.clone(), b.grad.clone(), h.grad.clone()))
    agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(*outs))
    graphs = [_graph(fn)[0] for fn in fns]
    med, mins = _time_alternating(graphs, replays)
    P = F * (F - 1) // 2
    flop = 2.0 * B * P * K * t                          # one product pair w
    res = {"shape": {"B": B, "F": F, "K": K, "t": t, "P": P}, "fused_vs_composed_max_rel_diff": agree,
           "fused_fwd_ms": med[0], "fused_fwd_bwd_ms": med[1], "composed_fwd_ms": med[2], "composed_fwd_bwd_ms": med[3],
           "fused_fwd_min_ms": mins[0], "fused_fwd_bwd_min_ms": mins[1], "composed_fwd_min_ms": mins[2], "composed_fwd_bwd_min_ms": mins[3],
           "speedup_fwd": med[2] / med[0], "speedup_fwd_bwd": med[3] / med[1],
           # matrix work the fused kernels issue: forward 1 product; backward 2 (both orientations of the recomputation) + dw + dpair
           "fused_fwd_TF": flop / (med[0] * 1e-3) / 1e12, "fused_bwd_TF": 4 * flop / ((med[1] - med[0]) * 1e-3) / 1e12}
    return res


def make_estimator(dev, B, fused):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    from recalgorithm_amd.algorithm.AFM.afm import afm_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=26, max_vocab=1_000_000, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES],
              "category_feature_columns": [fc.embedding_column(c, 16) for c in cats], "learning_rate": 0.005,
              "embedding_dim": 16, "attention_factor": 128, "afm_fused": fused}
    est = Estimator(model_fn=afm_model_fn, params=params, config=RunConfig(device=dev, seed=42))
    feats, labels, _ = synth.device_features(spec, B, dev)
    est.build(feats, labels)
    return est, feats, labels


def bench_step(dev, B, steps):
    from recalgorithm_amd.estimator import GraphedTrainStep
    runs = {}
    for name, fused in (("fused", None), ("composed", False)):
        est, feats, labels = make_estimator(dev, B, fused)
        runs[name] = GraphedTrainStep(est.train_step, feats, labels, warmup=3)
    times = {k: [] for k in runs}
    for g in runs.values():
        for _ in range(20):
            g()
    torch.cuda.synchronize()
    for _ in range(3):
        for name, g in runs.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                g()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(times["composed"]) - min(times["composed"])
    return {"batch": B, "fused_step_ms": med["fused"], "composed_step_ms": med["composed"], "fused_step_runs_ms": times["fused"],
            "composed_step_runs_ms": times["composed"], "composed_spread_ms": spread,
            "fused_examples_per_s": B / (med["fused"] * 1e-3), "composed_examples_per_s": B / (med["composed"] * 1e-3),
            "faster_than_spread": med["composed"] - med["fused"] > spread,
            "fused_loss": float(runs["fused"]()), "composed_loss": float(runs["composed"]()),
            "config": "26 fields x emb16 + 16 dense features; 325 pairs; attention factor 128; composed = afm_fused False, the "
                      "step before the kernels existed"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_afm.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "afm", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "op": bench_op(dev, a.batch, 26, 16, 128, a.replays), "op_small": bench_op(dev, 256, 7, 8, 16, a.replays),
           "step": bench_step(dev, a.batch, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
