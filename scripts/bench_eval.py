"""Estimator.evaluate on the MI355X (bench.py is the project's yardstick and times training only): examples/s and ms/batch of
evaluate() for DCN, DeepFM (BatchNorm) and MMoE (3 tasks) at the bench shapes, B = 4096, over 64 device-resident synthetic
batches, after three training steps (what train_and_evaluate evaluates: the tables carry deferred-Adam state).  Arms:

    host_metrics      RunConfig(device_metrics=False): eager EVAL model_fn, Metric.update() and float(loss) per batch
    device_eager      device_metrics=True, use_hip_graph=False: eager model_fn + one recalgo_metrics_update launch per batch
    device_captured   device_metrics=True, use_hip_graph=True: the EVAL step captured on the third batch and replayed

The script uses the public Estimator API only and probes RunConfig for `device_metrics`: on a tree without it there is one arm,
`parent` (evaluate() as that tree has it), so the same file run in a checkout of the parent commit gives the baseline; pass that
run's output with --parent to have its line recorded next to the arms (same box, same session: the boxes differ by ~4 %).
Each arm: 2 warm-up calls of evaluate(), then --repeats timed calls, the arms alternating; the median wall-clock time of a
call, which ends in the device-to-host read of the result.  The arms' result dicts must be equal: faster and different is not
faster.  `metrics_launch_ms`: the device time of recalgo_metrics_update alone (B rows, the model's slots): 200 launches captured
into one graph, HIP events around a replay, per launch (eager launches back to back would time the host's enqueue).

    python scripts/bench_eval.py [--batch 4096] [--batches 64] [--repeats 7] [--parent parent.json] [--out profiles/eval_bench.json]
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASKS = ("read_comment", "like", "click_avatar")
HIDDEN = ["512", "256", "128"]


def models():
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.io import synth

    def columns(spec):
        return [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]

    def dcn():
        from recalgorithm_amd.algorithm.DCN.dcn import dcn_model_fn
        spec = synth.SynthSpec(n_fields=26, max_vocab=1_000_000)
        return dcn_model_fn, {"category_feature_columns": [fc.embedding_column(c, 16) for c in columns(spec)], "dense_feature_columns": [],
                              "hidden_units": HIDDEN, "num_cross_layer": 3, "learning_rate": 0.005}, spec, ()

    def deepfm():
        from recalgorithm_amd.algorithm.DeepFM.deepfm import deepfm_model_fn
        spec = synth.SynthSpec(n_fields=26, max_vocab=1_000_000)
        cats = sorted(columns(spec), key=lambda c: c.key)
        return deepfm_model_fn, {"first_order_feature_columns": [fc.indicator_column(c) for c in cats],
                                 "second_order_feature_columns": [fc.embedding_column(c, 16) for c in cats],
                                 "hidden_units": HIDDEN, "dropout_rate": 0.0, "batch_norm": True, "learning_rate": 0.005}, spec, ()

    def mmoe():
        from recalgorithm_amd.algorithm._common import dense_columns
        from recalgorithm_amd.algorithm.MMOE.mmoe import mmoe_model_fn
        spec = synth.SynthSpec(n_fields=8, max_vocab=100000, seed=11, oov_frac=0.05, with_dense=True)
        dims = (16, 16, 16, 4, 4, 4, 4, 2)
        return mmoe_model_fn, {"dense_feature_columns": dense_columns(),
                               "category_feature_columns": [fc.embedding_column(c, k) for c, k in zip(columns(spec), dims)],
                               "hidden_units": HIDDEN, "dropout_rate": 0.1, "batch_norm": True, "learning_rate": 0.005,
                               "num_experts": 3, "num_tasks": 3, "expert_hidden_units": 512, "task_names": list(TASKS)}, spec, TASKS[1:]
    return {"dcn": dcn, "deepfm": deepfm, "mmoe": mmoe}


def metrics_launch_ms(dev, B, tasks, windows=5, launches=200):
    """device time of one recalgo_metrics_update: `tasks` accuracy slots + `tasks` AUC(200) slots over column views of a [B, tasks]
    probability matrix, with a loss; None on a tree without the kernel"""
    from recalgorithm_amd import ops
    if not hasattr(ops, "metrics_update"):
        return None
    from recalgorithm_amd.estimator import AUCMetric
    g = torch.Generator().manual_seed(3)
    prob = torch.rand(B, tasks, generator=g).to(dev)
    labels = [(torch.rand(B, 1, generator=g) < 0.04).float().to(dev) for _ in range(tasks)]
    hard = [(prob[:, i:i + 1] >= 0.5).float() for i in range(tasks)]
    th = AUCMetric(None, None).th.to(dev)
    slots = [("accuracy", labels[i], hard[i]) for i in range(tasks)] + [("auc", labels[i], prob[:, i:i + 1], th) for i in range(tasks)]
    loss = torch.tensor(0.7, device=dev)
    state = torch.zeros(ops.metrics_slot_table(slots)[2], dtype=torch.int64, device=dev)
    for _ in range(20):
        ops.metrics_update(slots, loss, state)
    torch.cuda.synchronize()
    # (eager launches back to back measure the host's enqueue rate: the launches are captured, the replay is timed)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            ops.metrics_update(slots, loss, state)
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / launches)
    return statistics.median(ts)


def bench_model(dev, name, make, args):
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    model_fn, params, spec, extra = make()
    kw = dict(extra_labels=extra) if extra else {}
    batches = [synth.device_features(spec, args.batch, dev, batch_index=i, **kw)[:2] for i in range(args.batches)]
    has = "device_metrics" in inspect.signature(RunConfig.__init__).parameters
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=11))
    est.train(lambda: iter(batches[:3]), log_every=0)
    arms = {"host_metrics": dict(device_metrics=False, use_hip_graph=True), "device_eager": dict(device_metrics=True, use_hip_graph=False),
            "device_captured": dict(device_metrics=True, use_hip_graph=True)} if has else {"parent": {}}

    def run(arm):
        for k, v in arms[arm].items():
            setattr(est.config, k, v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = est.evaluate(lambda: iter(batches))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    results = {arm: run(arm)[1] for arm in arms}
    for arm in arms:
        assert results[arm] == run(arm)[1], (name, arm, "two calls of evaluate() differ")
    first = next(iter(results.values()))
    assert all(r == first for r in results.values()), (name, results)
    times = {arm: [] for arm in arms}
    for _ in range(args.repeats):
        for arm in arms:
            times[arm].append(run(arm)[0])
    rows = {}
    for arm, ts in times.items():
        t = statistics.median(ts)
        rows[arm] = {"examples_per_s": args.batches * args.batch / t, "ms_per_batch": t * 1e3 / args.batches, "evaluate_ms": t * 1e3,
                     "evaluate_ms_min": min(ts) * 1e3, "evaluate_ms_max": max(ts) * 1e3}
        print(f"[{name}] {arm}: {rows[arm]['examples_per_s'] / 1e6:.3f} M examples/s, {rows[arm]['ms_per_batch']:.4f} ms/batch", file=sys.stderr, flush=True)
    launch = metrics_launch_ms(dev, args.batch, 1 + len(extra))
    return {"arms": rows, "metrics_launch_ms": launch, "slots": 2 * (1 + len(extra)), "result": first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent", default=None, help="the output of this script run in a checkout of the parent commit, same box")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_eval: needs a HIP device (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    per_model = {name: bench_model(dev, name, make, args) for name, make in models().items()}
    res = {"bench": "evaluate", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "shape": {"batch": args.batch, "batches": args.batches, "hidden_units": HIDDEN, "dcn_deepfm": "26 fields x emb 16",
                     "mmoe": "8 fields + 16 dense features, 3 experts x 512, 3 tasks"},
           "repeats": args.repeats, "models": per_model}
    if args.parent:
        parent = json.load(open(args.parent))
        for name, m in per_model.items():
            p = parent["models"][name]
            m["arms"]["parent"] = p["arms"]["parent"]
            m["parent_result_equal"] = p["result"] == m["result"]
            for arm in ("host_metrics", "device_eager", "device_captured"):
                m["arms"][arm]["speedup_over_parent"] = m["arms"][arm]["examples_per_s"] / p["arms"]["parent"]["examples_per_s"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
