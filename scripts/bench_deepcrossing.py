"""DeepCrossing measurements on the MI355X (bench.py is the project's yardstick and has no DeepCrossing entry): the fused
residual stack (csrc/residual.hip) against the same stack composed from nn.dense + ReLU, and the full captured training
step.  Self-contained: synthetic inputs from seeds, nothing read from outside the tree.  Prints one JSON line (and writes it
with --out).

    python scripts/bench_deepcrossing.py [--batch 4096] [--replays 200] [--steps 200] [--out profiles/deepcrossing_bench.json]

stack:  nn.residual_stack at B = 4096 for (D, H) = (82, 128) (the reference's columns), (128, 128), (256, 128) and (432, 128)
        (26 x 16 + 16 dense), 1 and 3 units, on a variable store of its own; per shape four captured graphs that alternate in
        ONE process, 20 warm-up replays each, then `--replays` timed ones in windows of 10: median, p10, p90 OF THE WINDOW
        MEANS (a mean of 10 replays spreads less than single replays do) of
          fused / composed forward            grad mode off (PREDICT / EVAL: the fused kernel saves nothing)
          fused / composed forward+backward   inside ops.loss_seed, as a training step runs it: the forward that saves, the
                                              backward, every weight-gradient launch and the step's ONE deferred reduction
        `fused_default_holds`: whether the fused forward+backward median is below the composed median by more than the
        composed measurement's own p10-p90 spread (of window means), in this run.
step:   the mirrored deepcrossing_model_fn with params["fused_residual"] = True and False (16 dense features + 8 id fields
        with the reference's embedding widths 16, 2, 4, 4, 4, 4, 16, 16: D = 82; single-valued ids) at B = 4096, captured
        (GraphedTrainStep): examples/s, and the kernel launches of one eager step counted with torch.profiler (None where the
        profiler gives no device events).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_ple import _graph, count_launches  # noqa: E402

SHAPES = [(82, 128), (128, 128), (256, 128), (432, 128)]
UNITS = [1, 3]
EMB = [16, 2, 4, 4, 4, 4, 16, 16]           # deepcrossing.py:94-100


def _quantiles(ts):
    ts = sorted(ts)
    q = lambda p: ts[min(len(ts) - 1, int(round(p * (len(ts) - 1))))]      # noqa: E731
    return {"median_ms": statistics.median(ts), "p10_ms": q(0.1), "p90_ms": q(0.9), "windows": len(ts)}


def time_alternating(graphs, replays, inner=10):
    """per graph: median, p10, p90 ms per replay; the graphs alternate, `inner` replays per timed window, 20 warm-up replays"""
    times = [[] for _ in graphs]
    for g in graphs:
        for _ in range(20):
            g.replay()
    torch.cuda.synchronize()
    for _ in range(max(math.ceil(replays / inner), 10)):
        for i, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                g.replay()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) / inner)
    return [_quantiles(t) for t in times]


def bench_stack(dev, B, D, H, L, replays):
    from recalgorithm_amd import nn, ops
    from recalgorithm_amd.variables import VariableStore, use_store
    gen = torch.Generator().manual_seed(1)
    x = (torch.rand(B, D, generator=gen) * 2 - 1).to(dev).requires_grad_(True)
    gy = (torch.rand(B, D, generator=gen) * 2 - 1).to(dev)
    store = VariableStore(dev, seed=3)
    assert ops.residual_supported(D, H, L)
    with use_store(store):
        store.building = True
        nn.residual_stack(torch.zeros(B, D, device=dev), H, L, fused=True)
        store.finalize()
        for name, v in store.vars.items():                   # biases off zero: both signs on both ReLUs
            if name.endswith("/bias"):
                v.data.copy_(((torch.rand(v.data.shape, generator=gen) * 2 - 1) * 0.2).to(dev))

        def run(fused, backward):
            def fn():
                store.begin_call()
                if not backward:
                    with torch.no_grad():
                        return nn.residual_stack(x, H, L, fused=fused)
                x.grad = None
                with ops.loss_seed(1.0):
                    y = nn.residual_stack(x, H, L, fused=fused)
                    y.backward(gy)
                ops.flush_dense_splits()
                return y
            return fn
        fns = [run(True, False), run(False, False), run(True, True), run(False, True)]
        outs = [f().detach().clone() for f in fns]
        grads = []
        for f in fns[2:]:
            f()
            grads.append(store.flat_grad.clone())
        agree = max(float((outs[0] - outs[1]).abs().max() / outs[1].abs().max()),
                    float((grads[0] - grads[1]).abs().max() / grads[1].abs().max()))
        graphs = [_graph(f)[0] for f in fns]
        q = time_alternating(graphs, replays)
    flops_fwd = 4.0 * B * D * H * L
    res = {"B": B, "D": D, "H": H, "units": L, "fused_by_default": bool(nn.residual_fused_default(D, H, L)),
           "fused_vs_composed_max_rel_diff": agree,
           "fused_forward": q[0], "composed_forward": q[1], "fused_forward_backward": q[2], "composed_forward_backward": q[3],
           "forward_gflop": flops_fwd / 1e9, "launches_forward": {"fused": 1, "composed": 3 * L},
           "launches_forward_backward": {"fused": 2 + 2 * L + 1, "composed": "3 forward + an add/ReLU backward and 2 merged dense backward launches per unit, + 1 reduction"}}
    spread = q[3]["p90_ms"] - q[3]["p10_ms"]
    res["composed_p10_p90_spread_ms"] = spread
    res["fused_default_holds"] = bool(q[2]["median_ms"] < q[3]["median_ms"] - spread)
    res["speedup_forward"] = q[1]["median_ms"] / q[0]["median_ms"]
    res["speedup_forward_backward"] = q[3]["median_ms"] / q[2]["median_ms"]
    return res


def make_estimator(dev, B, units, fused, internal_dim=128):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    from recalgorithm_amd.algorithm.DeepCrossing.deepcrossing import deepcrossing_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=len(EMB), max_vocab=100000, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES],
              "category_feature_columns": [fc.embedding_column(c, e) for c, e in zip(cats, EMB)],
              "residual_internal_dim": internal_dim, "residual_network_num": units, "learning_rate": 0.005,
              "fused_residual": fused}
    est = Estimator(deepcrossing_model_fn, params, RunConfig(device=dev, seed=5))
    feats, labels, _ = synth.device_features(spec, B, dev)
    est.build(feats, labels)
    return est, feats, labels


def bench_step(dev, B, steps, units, fused):
    from recalgorithm_amd.estimator import GraphedTrainStep
    est, feats, labels = make_estimator(dev, B, units, fused)
    g = GraphedTrainStep(est.train_step, feats, labels, warmup=3)
    for _ in range(20):
        g()
    torch.cuda.synchronize()
    windows = []
    for _ in range(10):
        t0 = time.perf_counter()
        for _ in range(max(steps // 10, 1)):
            g()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / max(steps // 10, 1) * 1e3)
    q = _quantiles(windows)
    est2, feats2, labels2 = make_estimator(dev, B, units, fused)
    n_launch, by_name = count_launches(est2, feats2, labels2)
    return {"batch": B, "units": units, "residual_stack": "fused" if fused else "composed", "step": q, "examples_per_s": B / (q["median_ms"] * 1e-3), "loss": float(g()),
            "kernel_launches_per_eager_step": n_launch, "most_launched": by_name,
            "config": f"{units} residual unit(s), internal dim 128, D = 82: 16 dense features + 8 single-valued id fields x emb "
                      f"{EMB}; Adam"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deepcrossing.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "deepcrossing", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "stack": [bench_stack(dev, a.batch, D, H, L, a.replays) for D, H in SHAPES for L in UNITS],
           "step": [bench_step(dev, a.batch, a.steps, L, fused) for L in UNITS for fused in (True, False)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
