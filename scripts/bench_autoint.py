"""AutoInt measurements on the MI355X: one interacting layer on the fused kernels (ops.autoint_layer, csrc/autoint.hip) against
the same layer composed from torch ops (einsum, softmax, autograd), forward and forward + backward, and the full captured AutoInt
training step.  Self-contained: synthetic inputs from seeds, nothing read from outside the tree.  Prints one JSON line (and
writes it with --out).

    python scripts/bench_autoint.py [--replays 200] [--steps 200] [--out profiles/autoint_bench.json]

layer: (B, F, D, A, H) = (4096, 26, 16, 8, 2), (4096, 26, 16, 32, 2), (4096, 26, 64, 32, 2), (4096, 7, 8, 8, 2), with the residual
       term: the forward under no_grad and forward + backward (dx and the four weight gradients), each captured once as one
       graph; the four graphs of a shape alternate in one call, medians of three rounds.  t_min by SURVEY.md §8d's rule from the
       layer's algorithmic bytes (x in, y out; g, x, y in and dx out for the backward; the weights and their gradients once) and
       FLOPs (projections, Q K^T, P V, the residual; the backward's products counted once each, recomputation not), and the
       achieved fraction t_min / t_measured.  fused_vs_composed_max_rel_diff is the largest difference of an output of the two,
       relative to the output's largest element: 1e-5 and below, or one example's gradient where a ReLU whose pre-activation
       is within fp32 rounding of zero falls on different sides in the two (against float64 the composed layer is the one off
       at (4096, 26, 16, 8, 2): DESIGN.md §5).
step:  synthetic 26 fields x emb16 + 16 dense features, 3 layers of 2 heads of 8, no deep part, B 4096, captured
       (GraphedTrainStep): medians of three runs.
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

SHAPES = [(4096, 26, 16, 8, 2), (4096, 26, 16, 32, 2), (4096, 26, 64, 32, 2), (4096, 7, 8, 8, 2)]
HBM, PEAK = 8e12, 157.3e12                   # bytes/s, fp32 MFMA FLOP/s


def composed_layer(x, F, wq, wk, wv, wres):
    """the layer from framework ops: what the fused kernel replaces (tests/autoint_ref.layer on [B, F * D])"""
    B = x.shape[0]
    H, D, A = wq.shape
    x3 = x.reshape(B, F, D)
    q, k, v = (torch.einsum("bfd,hda->bhfa", x3, w) for w in (wq, wk, wv))
    p = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B, F, H * A)
    return torch.relu(o + x3 @ wres).reshape(B, F * H * A)


def t_min(B, F, D, A, H):
    """-> (forward, forward + backward seconds by t_min = max(bytes / 8e12, flops / 157.3e12), forward FLOPs, backward FLOPs)"""
    HA = H * A
    w_bytes = 4 * 4 * D * HA
    fwd_bytes = 4 * B * F * (D + HA) + w_bytes
    bwd_bytes = 4 * B * F * (2 * HA + 2 * D) + 2 * w_bytes
    proj = 2 * F * D * HA                                    # one [F, D] x [D, HA] product
    att = 2 * F * F * HA                                     # Q K^T or P V over all heads
    fwd_flop = B * (4 * proj + 2 * att)
    bwd_flop = B * (8 * proj + 4 * att)                      # dx and dW of four projections; dV, dP, dQ, dK
    f = max(fwd_bytes / HBM, fwd_flop / PEAK)
    return f, f + max(bwd_bytes / HBM, bwd_flop / PEAK), fwd_flop, bwd_flop


def bench_layer(dev, B, F, D, A, H, replays):
    from recalgorithm_amd import ops
    gen = torch.Generator().manual_seed(100000 * F + 1000 * D + 10 * A + H)
    rnd = lambda *s: torch.randn(*s, generator=gen)          # noqa: E731
    x = rnd(B, F * D).to(dev).requires_grad_(True)
    ws = [(rnd(H, D, A) / D ** 0.5).to(dev).requires_grad_(True) for _ in range(3)] + [(rnd(D, H * A) / D ** 0.5).to(dev).requires_grad_(True)]
    g = rnd(B, F * H * A).to(dev)
    layers = {"fused": lambda: ops.autoint_layer(x, F, *ws), "composed": lambda: composed_layer(x, F, *ws)}

    def both(layer):
        def forward():
            with torch.no_grad():
                return [layer()]

        def step():
            y = layer()
            return [y.detach()] + list(torch.autograd.grad(y, [x] + ws, g))
        return forward, step
    fns = [*both(layers["fused"]), *both(layers["composed"])]        # fused fwd, fused fwd+bwd, composed fwd, composed fwd+bwd
    a, b = fns[1](), fns[3]()
    agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
    graphs = [_graph(fn)[0] for fn in fns]
    rounds = [_time_alternating(graphs, replays) for _ in range(3)]
    med = [statistics.median(r[0][i] for r in rounds) for i in range(4)]
    mins = [min(r[1][i] for r in rounds) for i in range(4)]
    tf, tfb, fwd_flop, bwd_flop = t_min(B, F, D, A, H)
    return {"shape": {"B": B, "F": F, "D": D, "A": A, "H": H}, "fused_vs_composed_max_rel_diff": agree,
            "fused_fwd_ms": med[0], "fused_fwd_bwd_ms": med[1], "composed_fwd_ms": med[2], "composed_fwd_bwd_ms": med[3],
            "fused_fwd_min_ms": mins[0], "fused_fwd_bwd_min_ms": mins[1], "composed_fwd_min_ms": mins[2], "composed_fwd_bwd_min_ms": mins[3],
            "speedup_fwd": med[2] / med[0], "speedup_fwd_bwd": med[3] / med[1],
            "fwd_mflop_per_example": fwd_flop / B / 1e6, "bwd_mflop_per_example": bwd_flop / B / 1e6,
            "t_min_fwd_ms": tf * 1e3, "t_min_fwd_bwd_ms": tfb * 1e3,
            "achieved_fwd": tf * 1e3 / med[0], "achieved_fwd_bwd": tfb * 1e3 / med[1]}


def make_estimator(dev, B):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    from recalgorithm_amd.algorithm.AutoInt.autoint import autoint_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=26, max_vocab=1_000_000, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES],
              "category_feature_columns": [fc.embedding_column(c, 16) for c in cats], "learning_rate": 0.005, "embedding_dim": 16,
              "att_embedding_size": 8, "head_num": 2, "num_interacting_layers": 3, "use_residual": True, "hidden_units": [],
              "batch_norm": True, "dropout_rate": 0.0}
    est = Estimator(model_fn=autoint_model_fn, params=params, config=RunConfig(device=dev, seed=42))
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
            "config": "26 fields x emb16 + 16 dense features; 3 interacting layers of 2 heads of 8 with the residual term; no deep part"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autoint.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "autoint", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "layers": [bench_layer(dev, *s, a.replays) for s in SHAPES], "step": bench_step(dev, 4096, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
