"""The per-user AUC of Estimator.evaluate on the MI355X (bench.py is the project's yardstick and times training only).

evaluate() of DCN and of MMoE (3 tasks) at the bench shapes, B = 4096, over 64 device-resident synthetic batches whose userid
column is Zipf over 20 000 users, after three training steps.  Legs:

    plain             params without group_auc_key, RunConfig defaults (device metrics, captured): the path as it was
    host_loop         the key set, device_metrics=False: GroupAUCMetric.update() keeps host copies, result() counts in numpy
    device_eager      the key set, device_metrics=True, use_hip_graph=False: one recalgo_gauc_append launch more per batch
    device_captured   the key set, device_metrics=True, use_hip_graph=True: that launch inside the captured EVAL step

Each leg: 2 warm-up calls of evaluate(), then --repeats timed calls, the legs alternating; the median wall-clock time of a call,
which ends in the device-to-host read of the result.  The legs with the key must return the same dict, `plain` that dict without
the per-user keys, and the captured legs the same number of graph replays with and without the key.  On a tree without
GroupAUCMetric there is one leg, `parent` (evaluate() as that tree has it); pass that run's output with --parent to have its
line recorded next to the legs (same box, same session).

The launches alone, device time by HIP events:
    append    recalgo_gauc_append at B rows, T = 1 and T = 3: 200 launches captured into one graph, the cursor reset before each
              replay, per launch (eager launches back to back would time the host's enqueue)
    finish    recalgo_gauc_finish (two memsets and six kernels, enqueued eagerly, events around them; and the wall-clock time
              of the call up to a synchronise) on the dataset's test-split size, 609 037 rows over 20 000 Zipf users, and on
              65 536 rows of ONE user with 3.5 % positives

    python scripts/bench_gauc.py [--batch 4096] [--batches 64] [--repeats 3] [--parent parent.json] [--out profiles/gauc_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASKS = ("read_comment", "like", "click_avatar")
HIDDEN = ["512", "256", "128"]
USERS = 20000


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

    def mmoe():
        from recalgorithm_amd.algorithm._common import dense_columns
        from recalgorithm_amd.algorithm.MMOE.mmoe import mmoe_model_fn
        spec = synth.SynthSpec(n_fields=8, max_vocab=100000, seed=11, oov_frac=0.05, with_dense=True)
        dims = (16, 16, 16, 4, 4, 4, 4, 2)
        return mmoe_model_fn, {"dense_feature_columns": dense_columns(),
                               "category_feature_columns": [fc.embedding_column(c, k) for c, k in zip(columns(spec), dims)],
                               "hidden_units": HIDDEN, "dropout_rate": 0.1, "batch_norm": True, "learning_rate": 0.005,
                               "num_experts": 3, "num_tasks": 3, "expert_hidden_units": 512, "task_names": list(TASKS)}, spec, TASKS[1:]
    return {"dcn": dcn, "mmoe": mmoe}


def bench_model(dev, name, make, args):
    from recalgorithm_amd import estimator as E
    from recalgorithm_amd.io import synth
    model_fn, params, spec, extra = make()
    assert spec.vocabs[spec.names.index("userid")] == USERS
    kw = dict(extra_labels=extra) if extra else {}
    batches = [synth.device_features(spec, args.batch, dev, batch_index=i, **kw)[:2] for i in range(args.batches)]
    has = hasattr(E, "GroupAUCMetric")
    est = E.Estimator(model_fn, dict(params), E.RunConfig(device=dev, seed=11))
    est.train(lambda: iter(batches[:3]), log_every=0)
    keyed = dict(group_auc_key="userid", group_auc_groups=USERS)
    legs = {"plain": ({}, dict(device_metrics=True, use_hip_graph=True)),
            "host_loop": (keyed, dict(device_metrics=False, use_hip_graph=True)),
            "device_eager": (keyed, dict(device_metrics=True, use_hip_graph=False)),
            "device_captured": (keyed, dict(device_metrics=True, use_hip_graph=True))} if has else {"parent": ({}, {})}

    def run(leg):
        more, config = legs[leg]
        est.params = dict(params, **more)
        for k, v in config.items():
            setattr(est.config, k, v)
        replays = getattr(est, "graph_replays", 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = est.evaluate(lambda: iter(batches))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, getattr(est, "graph_replays", 0) - replays
    results, replays = {}, {}
    for leg in legs:
        _, results[leg], replays[leg] = run(leg)
    for leg in legs:
        assert results[leg] == run(leg)[1], (name, leg, "two calls of evaluate() differ")
    if has:
        assert results["host_loop"] == results["device_eager"] == results["device_captured"], (name, results)
        assert results["plain"] == {k: v for k, v in results["device_captured"].items() if not k.endswith("uauc")}, (name, results)
        assert replays["plain"] == replays["device_captured"] > 0 and replays["device_eager"] == 0, (name, replays)
    times = {leg: [] for leg in legs}
    for _ in range(args.repeats):
        for leg in legs:
            times[leg].append(run(leg)[0])
    rows = {}
    for leg, ts in times.items():
        t = statistics.median(ts)
        rows[leg] = {"examples_per_s": args.batches * args.batch / t, "ms_per_batch": t * 1e3 / args.batches, "evaluate_ms": t * 1e3,
                     "evaluate_ms_min": min(ts) * 1e3, "evaluate_ms_max": max(ts) * 1e3, "graph_replays": replays[leg]}
        print(f"[{name}] {leg}: {rows[leg]['examples_per_s'] / 1e6:.3f} M examples/s, {rows[leg]['ms_per_batch']:.4f} ms/batch, "
              f"{replays[leg]} replays", file=sys.stderr, flush=True)
    return {"legs": rows, "tasks": 1 + len(extra), "result": results["device_captured" if has else "parent"]}


def zipf_users(rng, n):
    from recalgorithm_amd.io import synth
    return synth.zipf_ids(rng, n, USERS)


def append_launch_ms(dev, B, T, repeats, launches=200):
    """device time of one recalgo_gauc_append over column views of a [B, T] probability matrix and an id column of a [B, 26] matrix"""
    from recalgorithm_amd import ops
    rng = np.random.default_rng([5, B, T])
    ids = torch.from_numpy(np.stack([zipf_users(rng, B)] * 26, axis=1)).to(dev)
    prob = torch.from_numpy(rng.random((B, T)).astype(np.float32)).to(dev)
    labels = [torch.from_numpy((rng.random((B, 1)) < 0.035).astype(np.float32)).to(dev) for _ in range(T)]
    columns = [(labels[t], prob[:, t:t + 1]) for t in range(T)]
    st = ops.gauc_state(USERS, T, launches * B, dev)
    for _ in range(20):
        ops.gauc_append(st, ids[:, 3], columns)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            ops.gauc_append(st, ids[:, 3], columns)
    ts = []
    for _ in range(2 + repeats):
        st.state[:ops.GAUC_STATE_HEADER_WORDS].zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / launches)
    assert st.state[:2].tolist() == [launches * B, 0]
    return statistics.median(ts[2:])


def finish_ms(dev, rows, one_group, repeats, T=1):
    """recalgo_gauc_finish over `rows` logged rows: (device ms by events, wall ms up to a synchronise, valid groups, the metric)"""
    from recalgorithm_amd import ops
    from recalgorithm_amd.estimator import group_auc_value
    rng = np.random.default_rng([6, rows, int(one_group)])
    users = np.full(rows, 7, np.int64) if one_group else zipf_users(rng, rows)
    ids = torch.from_numpy(users).to(dev)
    columns = [(torch.from_numpy((rng.random(rows) < 0.035).astype(np.float32)).to(dev), torch.from_numpy(rng.random(rows).astype(np.float32)).to(dev))
               for _ in range(T)]
    st = ops.gauc_state(USERS, T, rows, dev)
    ops.gauc_append(st, ids, columns)
    dev_ms, wall_ms = [], []
    for _ in range(2 + repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        ops.gauc_finish(st)
        b.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(a.elapsed_time(b))
    skipped, dropped, logged, num2, pos, neg = ops.gauc_counts(st.result, USERS, T)
    assert (skipped, dropped, logged) == (0, 0, rows)
    value, valid = group_auc_value(num2[0], pos[0], neg[0])
    return {"rows": rows, "groups": USERS, "tasks": T, "one_group": one_group, "device_ms": statistics.median(dev_ms[2:]),
            "wall_ms": statistics.median(wall_ms[2:]), "valid_groups": valid, "largest_group": int((pos[0] + neg[0]).max()),
            "pairs": int((pos[0] * neg[0]).sum()), "uauc": value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="the output of this script run in a checkout of the parent commit, same box")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gauc: needs a HIP device (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    per_model = {name: bench_model(dev, name, make, args) for name, make in models().items()}
    res = {"bench": "group_auc", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "shape": {"batch": args.batch, "batches": args.batches, "users": USERS, "hidden_units": HIDDEN, "dcn": "26 fields x emb 16",
                     "mmoe": "8 fields + 16 dense features, 3 experts x 512, 3 tasks"},
           "repeats": args.repeats, "models": per_model}
    from recalgorithm_amd import ops
    if hasattr(ops, "gauc_append"):
        res["append_launch_ms"] = {f"T{T}": append_launch_ms(dev, args.batch, T, args.repeats) for T in (1, 3)}
        res["finish"] = {"test_split": finish_ms(dev, 609037, False, args.repeats), "one_group": finish_ms(dev, 65536, True, args.repeats)}
        print(json.dumps({"append_launch_ms": res["append_launch_ms"], "finish": res["finish"]}), file=sys.stderr, flush=True)
    if args.parent:
        parent = json.load(open(args.parent))
        for name, m in per_model.items():
            p = parent["models"][name]
            m["legs"]["parent"] = p["legs"]["parent"]
            m["parent_result_equal"] = p["result"] == {k: v for k, v in m["result"].items() if not k.endswith("uauc")}
            for leg in ("plain", "host_loop", "device_eager", "device_captured"):
                m["legs"][leg]["rate_over_parent"] = m["legs"][leg]["examples_per_s"] / p["legs"]["parent"]["examples_per_s"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
