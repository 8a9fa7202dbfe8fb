"""Wide&Deep measurements on the MI355X (bench.py is the project's yardstick and has no Wide&Deep entry): the crossed wide op
alone against the composition it replaces, and the full training step.  Self-contained: synthetic inputs from seeds,
nothing read from outside the tree.  Prints one JSON line (and writes it with --out).

    python scripts/bench_wdl.py [--batch 4096] [--replays 200] [--steps 200] [--out profiles/wdl_bench.json]

op:    forward + backward + one FTRL step of the wide part under hipGraph replay.  Fused: wide.cross_logit (hash + gather +
       logit, one launch), the plan (three launches) and the per-bucket ordered sum fused with FTRL (one launch), at the
       reference's hash_bucket_size 100000 and at `--baseline-buckets`.  Baseline, at `--baseline-buckets` only (the [B, H]
       multi-hot of B = 4096 x 100000 buckets is 1.6 GB): bucket ids given (the baseline is not charged the hash), a torch
       multi-hot built with index_put_(accumulate), matmul with the (H, 1) kernel + bias, autograd's backward (a dense
       (H, 1) gradient), and the dense FTRL update of every bucket written with torch elementwise ops — what TF executes.
       The graphs alternate in one process on the same inputs; medians over the replays.
step:  the mirrored model_fn (hidden 512,256,128, BatchNorm, 16 dense + 7 embedding columns, the tag bag, the crossed wide
       column of 100000 buckets) at B = 4096, captured (GraphedTrainStep), examples/s.
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

LR = 0.005


def make_batch(B, dev, seed=7):
    """users [B] and a tag bag of 0..5 tags per example (Zipf-like: hot users and tags repeat), on the device"""
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=6, max_vocab=100000, seed=seed, oov_frac=0.02, with_dense=True, with_tags=True)
    feats, labels, _ = synth.device_features(spec, B, dev)
    return spec, feats, labels


def bench_op(dev, B, H, replays, with_baseline):
    from recalgorithm_amd import wide
    from recalgorithm_amd.variables import Variable, VariableStore
    spec, feats, _ = make_batch(B, dev)
    users = feats[spec.names[0]].contiguous()
    tags = feats["manual_tag_list"]
    gen = torch.Generator().manual_seed(1)
    dlogit = (torch.randn(B, 1, generator=gen) / B).to(dev)
    store = VariableStore(dev, seed=3)
    st = wide.WideState(Variable("wide/kernel", (torch.rand(H, 1, generator=gen) - 0.5).to(dev)),
                        Variable("wide/bias", torch.zeros(1).to(dev)), H, wide.HASH_KEY)

    def fused():
        out = wide.cross_logit(store, st, users, tags.values, tags.offsets, training=True)
        out.backward(dlogit)
        st.apply_ftrl(LR, 0.0, 0.0, 0.1)
        return out

    def fused_forward():
        return wide.cross_logit(store, st, users, tags.values, tags.offsets, training=False)
    fused()                                  # (the first FTRL step zeroes the untouched buckets: eager, once)
    gf, _ = _graph(fused)
    g0, _ = _graph(fused_forward)
    graphs = [gf, g0]
    n_req = int(tags.offsets[-1])
    res = {"shape": {"B": B, "hash_bucket_size": H, "requests": n_req}}
    if with_baseline:
        ex, bk = st.last_requests(training=False)
        ex, bk = ex.long(), bk.long()
        kernel = (torch.rand(H, 1, generator=gen) - 0.5).to(dev).requires_grad_(True)
        bias = torch.zeros(1, device=dev, requires_grad=True)
        state = {"k": (torch.full((H, 1), 0.1, device=dev), torch.zeros(H, 1, device=dev)),
                 "b": (torch.full((1,), 0.1, device=dev), torch.zeros(1, device=dev))}
        ones = torch.ones(n_req, device=dev)

        def ftrl_(var, g, accum, linear):
            new = accum + g * g
            linear.add_(g - (new.sqrt() - accum.sqrt()) / LR * var)
            var.copy_(-linear / (new.sqrt() / LR))
            accum.copy_(new)

        def baseline():
            mh = torch.zeros(B, H, device=dev).index_put_((ex, bk), ones, accumulate=True)
            out = mh @ kernel + bias
            gk, gb = torch.autograd.grad(out, [kernel, bias], dlogit)
            with torch.no_grad():
                ftrl_(kernel, gk, *state["k"])
                ftrl_(bias, gb, *state["b"])
            return out
        gb_, _ = _graph(baseline)
        graphs.append(gb_)
    med, mins = _time_alternating(graphs, replays)
    res.update({"fused_ms": med[0], "fused_min_ms": mins[0], "fused_forward_ms": med[1],
                "fused_backward_and_ftrl_ms": med[0] - med[1]})
    if with_baseline:
        res.update({"baseline_ms": med[2], "baseline_min_ms": mins[2], "speedup": med[2] / med[0],
                    "baseline": "torch multi-hot (index_put_) + matmul + autograd + dense FTRL of every bucket; bucket ids given"})
    return res


def make_estimator(dev, B):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import dense_columns
    from recalgorithm_amd.algorithm.WideAndDeep.wide_and_deep import HASH_BUCKET_SIZE, wide_and_deep_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    spec, feats, labels = make_batch(B, dev)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    tag = fc.categorical_column_with_identity("manual_tag_list", spec.tag_vocab)
    deep = dense_columns() + [fc.embedding_column(c, k) for c, k in zip(cats, (16, 16, 2, 4, 4, 4))] + [fc.embedding_column(tag, 4)]
    wide_cols = [fc.indicator_column(fc.crossed_column([cats[0], tag], HASH_BUCKET_SIZE))]
    params = {"wide_part_feature_columns": wide_cols, "deep_part_feature_columns": deep, "hidden_units": ["512", "256", "128"],
              "dropout_rate": 0.0, "batch_norm": True, "deep_part_optimizer": "Adam", "wide_part_learning_rate": 0.005,
              "deep_part_learning_rate": 0.001}
    est = Estimator(wide_and_deep_model_fn, params, RunConfig(device=dev, seed=5))
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
    return {"batch": B, "step_ms": ms, "examples_per_s": B / (ms * 1e-3), "step_ms_min": min(windows) * 1e3, "loss": float(g()),
            "config": "hidden 512,256,128; BN; 16 dense + 6 id embeddings + the tag bag; crossed [first id, tag] x 100000 buckets"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--baseline-buckets", type=int, default=8192)      # [4096, 8192] fp32 multi-hot: 134 MB
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wdl.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "wdl", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "op_reference_buckets": bench_op(dev, a.batch, 100000, a.replays, with_baseline=False),
           "op_baseline_buckets": bench_op(dev, a.batch, a.baseline_buckets, a.replays, with_baseline=True),
           "step": bench_step(dev, a.batch, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
