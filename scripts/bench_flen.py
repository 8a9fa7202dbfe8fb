"""FLEN measurements on the MI355X: the field-wise bi-interaction with Dicefactor on the fused kernels (ops.flen_interaction,
csrc/flen.hip) against the same arithmetic composed from torch ops (index_select, sums, products, autograd; the mask from
ops.dropout_keep_mask), forward and forward + backward, and the full captured FLEN training step.  Self-contained: synthetic
inputs from seeds, nothing read from outside the tree.  Prints one JSON line (and writes it with --out).

    python scripts/bench_flen.py [--replays 200] [--steps 200] [--out profiles/flen_bench.json]

layer: (B, F, M, K) = (4096, 26, 4, 16) with groups f % 4, (4096, 7, 3, 8) with the dataset's grouping, (4096, 64, 8, 64) with
       groups f % 8, each with Dicefactor off and at 0.1 (the hash): the forward under no_grad and forward + backward (dx and the
       three parameter gradients, from gradients of both e and h), each captured once as one graph; the four graphs of a case
       alternate in one call, medians of three rounds.  bytes: the op's algorithmic traffic (x in, e and h out; x, g_e, g_h in and
       dx out for the backward) and the time it takes at 8 TB/s, for scale — the op is a few MB and is not expected to reach it.
       fused_vs_composed_max_rel_diff is the largest difference of an output of the two, relative to the output's largest
       element.
step:  synthetic 7 single-valued fields x emb8 in the dataset's three groups, 16 dense features, hidden units 512,256,128 with
       BatchNorm, Dicefactor off (the flags' defaults), B 4096, captured (GraphedTrainStep): medians of three runs, with the
       kernels and with the composed arithmetic.
"""
import argparse
import json
import os
import statistics
import sys
import time
from itertools import combinations

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_ple import _graph, _time_alternating  # noqa: E402

DATASET_GROUPS = (0, 1, 0, 1, 2, 2, 1)
SHAPES = [(4096, 26, 4, 16, tuple(f % 4 for f in range(26))), (4096, 7, 3, 8, DATASET_GROUPS), (4096, 64, 8, 64, tuple(f % 8 for f in range(64)))]
RATES = (0.0, 0.1)
HBM = 8e12


def indices(group_of, M, dev):
    """the index tensors of the composed arithmetic, made once outside the captured region"""
    members = [torch.tensor([f for f, g in enumerate(group_of) if g == m], device=dev) for m in range(M)]
    first, second = (torch.tensor(ix, device=dev) for ix in zip(*combinations(range(M), 2)))
    return members, first, second


def composed(x, F, idx, r_mf, r_fm, bias, dice=None):
    """the arithmetic from framework ops: what the fused kernels replace (nn.field_wise_bi_interaction(fused=False))"""
    from recalgorithm_amd import ops
    B, M, K = x.shape[0], r_fm.shape[0], bias.shape[0]
    xs = x.reshape(B, F, K)
    members, first, second = idx
    e = torch.stack([xs.index_select(1, idx).sum(1) for idx in members], dim=1)
    q = torch.stack([xs.index_select(1, idx).square().sum(1) for idx in members], dim=1)
    paths = torch.cat([r_mf[:, None] * (e.index_select(1, first) * e.index_select(1, second)), r_fm[:, None] * (e * e - q)], dim=1)
    if dice is not None:
        paths = paths * (ops.dropout_keep_mask(tuple(paths.shape), dice, x.device) * dice.scale)
    return e.reshape(B, M * K), bias + paths.sum(1)


def bench_layer(dev, B, F, M, K, group_of, rate, replays):
    from recalgorithm_amd import ops
    gen = torch.Generator().manual_seed(100000 * M + 1000 * F + 10 * K)
    rnd = lambda *s: torch.randn(*s, generator=gen)          # noqa: E731
    P = M * (M - 1) // 2
    x = rnd(B, F * K).to(dev).requires_grad_(True)
    ws = [(1.0 + 0.3 * rnd(P)), (0.5 + 0.2 * rnd(M)), 0.5 * rnd(K)]
    ws = [w.to(dev).requires_grad_(True) for w in ws]
    g_e, g_h = rnd(B, M * K).to(dev), rnd(B, K).to(dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    dice = ops.DropSpec(rate, None, 42, 0, step) if rate > 0 else None
    idx = indices(group_of, M, dev)
    layers = {"fused": lambda: ops.flen_interaction(x, F, group_of, *ws, dice=dice),
              "composed": lambda: composed(x, F, idx, *ws, dice=dice)}

    def both(layer):
        def forward():
            with torch.no_grad():
                return list(layer())

        def fwd_bwd():
            e, h = layer()
            return [e.detach(), h.detach()] + list(torch.autograd.grad([e, h], [x] + ws, [g_e, g_h]))
        return forward, fwd_bwd
    fns = [*both(layers["fused"]), *both(layers["composed"])]        # fused fwd, fused fwd+bwd, composed fwd, composed fwd+bwd
    a, b = fns[1](), fns[3]()
    agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
    graphs = [_graph(fn)[0] for fn in fns]
    rounds = [_time_alternating(graphs, replays) for _ in range(3)]
    med = [statistics.median(r_[0][i] for r_ in rounds) for i in range(4)]
    mins = [min(r_[1][i] for r_ in rounds) for i in range(4)]
    fwd_bytes, bwd_bytes = 4 * B * K * (F + M + 1), 4 * B * K * (2 * F + M + 1)
    return {"shape": {"B": B, "F": F, "M": M, "K": K}, "dicefactor_rate": rate, "fused_vs_composed_max_rel_diff": agree,
            "fused_fwd_ms": med[0], "fused_fwd_bwd_ms": med[1], "composed_fwd_ms": med[2], "composed_fwd_bwd_ms": med[3],
            "fused_fwd_min_ms": mins[0], "fused_fwd_bwd_min_ms": mins[1], "composed_fwd_min_ms": mins[2], "composed_fwd_bwd_min_ms": mins[3],
            "speedup_fwd": med[2] / med[0], "speedup_fwd_bwd": med[3] / med[1],
            "fwd_mbytes": fwd_bytes / 1e6, "fwd_bwd_mbytes": (fwd_bytes + bwd_bytes) / 1e6,
            "t_hbm_fwd_ms": fwd_bytes / HBM * 1e3, "t_hbm_fwd_bwd_ms": (fwd_bytes + bwd_bytes) / HBM * 1e3}


def make_estimator(dev, B, fused):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    from recalgorithm_amd.algorithm.FLEN.flen import flen_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=7, max_vocab=1_000_000, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    groups = [[n for n, g in zip(spec.names, DATASET_GROUPS) if g == m] for m in range(3)]
    params = {"dense_feature_columns": [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES],
              "category_feature_columns": [fc.embedding_column(c, 8) for c in cats], "embedding_dim": 8, "field_groups": groups,
              "hidden_units": [512, 256, 128], "batch_norm": True, "dropout_rate": 0.0, "dicefactor_rate": 0.0, "learning_rate": 0.005,
              "fused_fwbi": fused}
    est = Estimator(model_fn=flen_model_fn, params=params, config=RunConfig(device=dev, seed=42))
    feats, labels, _ = synth.device_features(spec, B, dev)
    est.build(feats, labels)
    return est, feats, labels


def bench_step(dev, B, steps, fused):
    from recalgorithm_amd.estimator import GraphedTrainStep
    est, feats, labels = make_estimator(dev, B, fused)
    g = GraphedTrainStep(est.train_step, feats, labels, warmup=3)
    for _ in range(20):
        g()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            g()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps * 1e3)
    med = statistics.median(times)
    return {"batch": B, "fused": fused, "step_ms": med, "step_runs_ms": times, "examples_per_s": B / (med * 1e-3), "loss": float(g()),
            "config": "7 fields x emb8 in three groups (2, 3, 2), 16 dense features; hidden units 512,256,128 with BatchNorm; Dicefactor off"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flen.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "flen", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "layers": [bench_layer(dev, *s, rate, a.replays) for s in SHAPES for rate in RATES],
           "step": bench_step(dev, 4096, a.steps, True), "step_composed": bench_step(dev, 4096, a.steps, False)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
