"""DCN-V2 measurements on the MI355X: one cross layer (the mixture of low-rank experts) on the fused kernels (ops.dcnv2_layer,
csrc/dcnv2.hip) against the same layer composed from torch ops (einsum, tanh, softmax, autograd), forward and forward + backward,
and the full captured DCN-V2 training step.  Self-contained: synthetic inputs from seeds, nothing read from outside the tree.
Prints one JSON line (and writes it with --out).

    python scripts/bench_dcnv2.py [--replays 200] [--steps 200] [--out profiles/dcnv2_bench.json]

layer: (B, D, r, E) = (4096, 416, 32, 4), (4096, 416, 64, 4), (4096, 82, 32, 4), (4096, 416, 32, 1): the forward under no_grad and
       forward + backward (dx0, dxl and the five parameter gradients), each captured once as one graph; the four graphs of a
       shape alternate in one call, medians of three rounds.  t_min by SURVEY.md §8d's rule from the layer's algorithmic bytes
       (x0, xl in, y out; g, x0, xl in and dx0, dxl out for the backward; the weights and their gradients once) and FLOPs (the
       three products per expert and the gate; the backward's products counted once each, recomputation not), and the achieved
       fraction t_min / t_measured.  fused_vs_composed_max_rel_diff is the largest difference of an output of the two, relative
       to the output's largest element.
step:  synthetic 26 fields x emb16 (D = 416, no dense features), 2 cross layers of 4 experts of rank 32, parallel structure,
       hidden units 512,256,128, B 4096, captured (GraphedTrainStep): medians of three runs.
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

SHAPES = [(4096, 416, 32, 4), (4096, 416, 64, 4), (4096, 82, 32, 4), (4096, 416, 32, 1)]
HBM, PEAK = 8e12, 157.3e12                   # bytes/s, fp32 MFMA FLOP/s


def composed_layer(x0, xl, V, C, U, gate, bias):
    """the layer from framework ops: what the fused kernels replace (tests/dcnv2_ref.layer, nn.cross_mix_layer(fused=False))"""
    v = torch.tanh(torch.einsum("bd,edr->ber", xl, V))
    c = torch.tanh(torch.einsum("ber,ers->bes", v, C))
    u = torch.einsum("ber,edr->bed", c, U) + bias
    p = torch.softmax(xl @ gate.t(), dim=-1)
    return x0 * torch.einsum("be,bed->bd", p, u) + xl


def t_min(B, D, r, E):
    """-> (forward, forward + backward seconds by t_min = max(bytes / 8e12, flops / 157.3e12), forward FLOPs, backward FLOPs)"""
    w_bytes = 4 * (E * (2 * D * r + r * r + D) + D)
    fwd_bytes = 4 * B * 3 * D + w_bytes
    bwd_bytes = 4 * B * 5 * D + 2 * w_bytes
    fwd_flop = B * E * (2 * (2 * D * r + r * r) + 2 * D)
    bwd_flop = 2 * fwd_flop + B * E * 2 * D * r              # dx and dW of every product; q U_e once more for dp
    f = max(fwd_bytes / HBM, fwd_flop / PEAK)
    return f, f + max(bwd_bytes / HBM, bwd_flop / PEAK), fwd_flop, bwd_flop


def bench_layer(dev, B, D, r, E, replays):
    from recalgorithm_amd import ops
    gen = torch.Generator().manual_seed(100000 * E + 1000 * D + 10 * r)
    rnd = lambda *s: torch.randn(*s, generator=gen)          # noqa: E731
    x0, xl = (rnd(B, D).to(dev).requires_grad_(True) for _ in range(2))
    ws = [(rnd(E, D, r) / D ** 0.5), (rnd(E, r, r) / r ** 0.5), (rnd(E, D, r) / r ** 0.5), (rnd(E, D) / D ** 0.5), rnd(D) * 0.5]
    ws = [w.to(dev).requires_grad_(True) for w in ws]
    g = rnd(B, D).to(dev)
    layers = {"fused": lambda: ops.dcnv2_layer(x0, xl, *ws), "composed": lambda: composed_layer(x0, xl, *ws)}

    def both(layer):
        def forward():
            with torch.no_grad():
                return [layer()]

        def step():
            y = layer()
            return [y.detach()] + list(torch.autograd.grad(y, [x0, xl] + ws, g))
        return forward, step
    fns = [*both(layers["fused"]), *both(layers["composed"])]        # fused fwd, fused fwd+bwd, composed fwd, composed fwd+bwd
    a, b = fns[1](), fns[3]()
    agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
    graphs = [_graph(fn)[0] for fn in fns]
    rounds = [_time_alternating(graphs, replays) for _ in range(3)]
    med = [statistics.median(r_[0][i] for r_ in rounds) for i in range(4)]
    mins = [min(r_[1][i] for r_ in rounds) for i in range(4)]
    tf, tfb, fwd_flop, bwd_flop = t_min(B, D, r, E)
    return {"shape": {"B": B, "D": D, "r": r, "E": E}, "fused_vs_composed_max_rel_diff": agree,
            "fused_fwd_ms": med[0], "fused_fwd_bwd_ms": med[1], "composed_fwd_ms": med[2], "composed_fwd_bwd_ms": med[3],
            "fused_fwd_min_ms": mins[0], "fused_fwd_bwd_min_ms": mins[1], "composed_fwd_min_ms": mins[2], "composed_fwd_bwd_min_ms": mins[3],
            "speedup_fwd": med[2] / med[0], "speedup_fwd_bwd": med[3] / med[1],
            "fwd_mflop_per_example": fwd_flop / B / 1e6, "bwd_mflop_per_example": bwd_flop / B / 1e6,
            "t_min_fwd_ms": tf * 1e3, "t_min_fwd_bwd_ms": tfb * 1e3,
            "achieved_fwd": tf * 1e3 / med[0], "achieved_fwd_bwd": tfb * 1e3 / med[1]}


def make_estimator(dev, B):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm.DCNV2.dcnv2 import dcnv2_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=26, max_vocab=1_000_000)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": [], "category_feature_columns": [fc.embedding_column(c, 16) for c in cats], "learning_rate": 0.005,
              "hidden_units": [512, 256, 128], "num_cross_layer": 2, "cross_parameterization": "mix", "low_rank": 32, "num_experts": 4,
              "structure": "parallel"}
    est = Estimator(model_fn=dcnv2_model_fn, params=params, config=RunConfig(device=dev, seed=42))
    feats, labels, _ = synth.device_features(spec, B, dev)
    est.build(feats, labels)
    return est, feats, labels


def bench_step(dev, B, steps):
    from recalgorithm_amd.estimator import GraphedTrainStep
    est, feats, labels = make_estimator(dev, B)
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
    return {"batch": B, "step_ms": med, "step_runs_ms": times, "examples_per_s": B / (med * 1e-3), "loss": float(g()),
            "config": "26 fields x emb16 (D 416); 2 cross layers of 4 experts of rank 32, parallel; hidden units 512,256,128"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dcnv2.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "dcnv2", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "layers": [bench_layer(dev, *s, a.replays) for s in SHAPES], "step": bench_step(dev, 4096, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
