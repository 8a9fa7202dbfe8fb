"""MMoE measurements on the MI355X (bench.py is the project's yardstick and has no MMoE entry): the gate-mix op against the
same block composed from what the tree offered before it, and the full training step.  Self-contained: synthetic inputs
from seeds, nothing read from outside the tree.  Prints one JSON line (and writes it with --out).

    python scripts/bench_mmoe.py [--batch 4096] [--replays 200] [--steps 200] [--out profiles/mmoe_bench.json]
    python scripts/bench_mmoe.py --trace-step     # a few captured steps and nothing else: the run to put under
                                                  # `rocprofv3 --kernel-trace --stats -- python scripts/bench_mmoe.py --trace-step`

op:    forward + backward + the deferred-sum launch of the gate kernels' gradients, under hipGraph replay, fused
       (ops.gate_mix) and baseline (G bias-free dense layers on the MFMA engine + torch.softmax + torch.stack / torch.bmm with
       autograd's backward) alternating in one process on the same inputs; medians over the replays.
bytes: the algorithmic traffic of the fused kernels (fp32): forward reads E and writes G [B, H] tensors and reads x;
       backward reads E + G and writes E [B, H] tensors, reads x and p and writes dx.  achieved GB/s = bytes / kernel-pair time
       of the replay (both launches + the reduction), against the 6.3 TB/s achievable copy rate; the working set fits the
       256 MB Infinity Cache, so the fraction can exceed 1.
step:  the mirrored model_fn at the reference's default configuration, captured (GraphedTrainStep), examples/s.
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

TASKS = ["read_comment", "like", "click_avatar"]
COPY_RATE = 6.3e12          # achievable HBM copy rate, bytes/s


def _graph(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def _time_alternating(graphs, replays, inner=10):
    """median ms per replay of each graph; the graphs alternate, `inner` replays per timed window"""
    times = [[] for _ in graphs]
    for g in graphs:
        for _ in range(20):
            g.replay()
    torch.cuda.synchronize()
    for _ in range(max(replays // inner, 5)):
        for i, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                g.replay()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) / inner)
    return [statistics.median(t) for t in times], [min(t) for t in times]


def bench_op(dev, B, In, E, G, H, replays):
    from recalgorithm_amd import nn, ops
    from recalgorithm_amd.variables import VariableStore, use_store
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, In, generator=gen).to(dev).requires_grad_(True)
    experts = [torch.relu(torch.randn(B, H, generator=gen)).to(dev).requires_grad_(True) for _ in range(E)]
    gouts = [torch.randn(B, H, generator=gen).to(dev) for _ in range(G)]
    store = VariableStore(dev, seed=3)
    with use_store(store):
        kernels = [store.get_variable(f"gate_{g}/kernel", (In, E)) for g in range(G)]
        store.pack()

        def fused():
            outs = ops.gate_mix(x, kernels, experts, anchor=store.anchor)
            grads = torch.autograd.grad(outs, [x, *experts], gouts)
            ops.flush_dense_splits()
            return [*outs, *grads]

        def baseline():
            gates = [torch.softmax(nn.dense_with(x, k), dim=-1) for k in kernels]
            stack = torch.stack(experts, dim=1)                                   # [B, E, H]
            outs = [torch.bmm(stack.transpose(1, 2), g.unsqueeze(-1)).squeeze(-1) for g in gates]
            grads = torch.autograd.grad(outs, [x, *experts], gouts)
            ops.flush_dense_splits()
            return [*outs, *grads]
        gf, of = _graph(fused)
        gf.replay()
        torch.cuda.synchronize()
        dw_f = [k.grad.clone() for k in kernels]
        gb, ob = _graph(baseline)
        gb.replay()
        torch.cuda.synchronize()
        dw_b = [k.grad.clone() for k in kernels]
        worst = 0.0
        for a, b in zip([*of, *dw_f], [*ob, *dw_b]):
            worst = max(worst, float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp(min=1e-30)))
        (tf, tb), (mf, mb) = _time_alternating([gf, gb], replays)
    fwd_bytes = 4 * (E * B * H + G * B * H + B * In)
    bwd_bytes = 4 * ((E + G) * B * H + E * B * H + 2 * B * In + B * G * E)
    return {"shape": {"B": B, "In": In, "E": E, "G": G, "H": H}, "fused_ms": tf, "baseline_ms": tb, "fused_min_ms": mf,
            "baseline_min_ms": mb, "speedup": tb / tf, "fused_vs_baseline_max_rel_diff": worst,
            "algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
            "fused_fwd_bwd_fraction_of_copy_rate": (fwd_bytes + bwd_bytes) / (tf * 1e-3) / COPY_RATE,
            "note": "fwd + bwd + reduction per replay; the 128 MB working set fits the 256 MB Infinity Cache, so the fraction can exceed 1"}


def make_estimator(dev, B):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import dense_columns
    from recalgorithm_amd.algorithm.MMOE.mmoe import mmoe_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=8, max_vocab=100000, seed=11, oov_frac=0.05, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    dims = (16, 16, 16, 4, 4, 4, 4, 2)      # + 16 dense features = the reference's 82 inputs
    params = {"dense_feature_columns": dense_columns(), "category_feature_columns": [fc.embedding_column(c, k) for c, k in zip(cats, dims)],
              "hidden_units": ["512", "256", "128"], "dropout_rate": 0.1, "batch_norm": True, "learning_rate": 0.005,
              "num_experts": 3, "num_tasks": 3, "expert_hidden_units": 512, "task_names": list(TASKS)}
    est = Estimator(mmoe_model_fn, params, RunConfig(device=dev, seed=5))
    feats, labels, _ = synth.device_features(spec, B, dev, extra_labels=TASKS[1:])
    est.build(feats, labels)
    return est, feats, labels


def bench_step(dev, B, steps):
    from recalgorithm_amd.estimator import GraphedTrainStep
    est, feats, labels = make_estimator(dev, B)
    g = GraphedTrainStep(est.train_step, feats, labels, warmup=3)
    for _ in range(20):
        g()
    torch.cuda.synchronize()
    windows = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(steps // 5):
            g()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / (steps // 5))
    ms = statistics.median(windows) * 1e3
    return {"batch": B, "step_ms": ms, "examples_per_s": B / (ms * 1e-3), "step_ms_min": min(windows) * 1e3,
            "loss": float(g()), "config": "hidden 512,256,128; 3 experts x 512; 3 tasks; BN; dropout 0.1; In 82"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mmoe.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    if a.trace_step:
        from recalgorithm_amd.estimator import GraphedTrainStep
        est, feats, labels = make_estimator(dev, a.batch)
        g = GraphedTrainStep(est.train_step, feats, labels, warmup=3)
        for _ in range(10):
            g()
        torch.cuda.synchronize()
        print(json.dumps({"traced_replays": 10, "batch": a.batch}))
        return
    res = {"bench": "mmoe", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "op": bench_op(dev, a.batch, 82, 3, 3, 512, a.replays),
           "op_e8_g5_h128": bench_op(dev, a.batch, 82, 8, 5, 128, a.replays),          # the EMAX = 8 arm
           "op_e16_g3_h128": bench_op(dev, a.batch, 82, 16, 3, 128, a.replays),        # the EMAX = 16 arm (spills in the backward)
           "step": bench_step(dev, a.batch, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
