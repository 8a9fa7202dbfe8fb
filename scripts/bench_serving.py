"""Serving measurements on the MI355X (bench.py is the project's yardstick and has no serving entry): DeepFM and DCN at the bench
shape (26 fields x emb 16, MLP 512,256,128) exported and served, requests of n in {1, 16, 64, 256, 1024, 4096} serialized
tf.train.Example protos, four paths:

    predict          ServingModel.predict: Python decode (algorithm.utils.parse_example), eager PREDICT model_fn
    native_eager     ServingModel.serve without compile(): native decode (recalgo_examples_*), eager model_fn
    compiled         serve() after compile() with the fused tower off: native decode, one captured graph of the per-layer kernels
    compiled_tower   the same with the hidden stack as ONE launch (ops.serve_tower) at every bucket

Per path and n: decode_ms (median, the decode alone on the host), device_ms (compiled paths: one graph replay, HIP events over
windows of replays, the two graphs alternating; eager paths: HIP events around the eager model_fn, launch gaps included) and
end_to_end_ms (median wall clock of one request, protos in, numpy out).  `tower_alone`: the tower launch against the captured
per-layer chain it replaces, with and without BatchNorm, on the bench widths.  `serve_tower_max_rows` is the value the numbers
support for nn.SERVE_TOWER_MAX_ROWS: the largest n such that compiled_tower's device_ms is no larger than compiled's at that n and
at every smaller one, on DeepFM (whose stack folds a BatchNorm per layer); 0 when there is none.  `serve_tower_plain_stacks`, for
nn.SERVE_TOWER_PLAIN_STACKS: whether that also holds on DCN, whose stack is plain dense(relu).  Self-contained: synthetic
vocabularies and records from seeds.

    python scripts/bench_serving.py [--replays 300] [--requests 30] [--out profiles/serving_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_ple import _graph, _time_alternating  # noqa: E402

SIZES = [1, 16, 64, 256, 1024, 4096]
UNITS = [512, 256, 128]


def models(spec, vocab_dir):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm.DCN.dcn import dcn_model_fn
    from recalgorithm_amd.algorithm.DeepFM.deepfm import deepfm_model_fn
    cats = [fc.categorical_column_with_vocabulary_file(n, vocab_dir + n + ".txt") for n in spec.names]
    first, second = [fc.indicator_column(c) for c in cats], [fc.embedding_column(c, 16) for c in cats]
    hidden = [str(u) for u in UNITS]
    return {"deepfm": (deepfm_model_fn, {"first_order_feature_columns": first, "second_order_feature_columns": second,
                                         "hidden_units": hidden, "dropout_rate": 0.0, "batch_norm": True, "learning_rate": 0.005},
                       first + second),
            "dcn": (dcn_model_fn, {"category_feature_columns": second, "dense_feature_columns": [], "hidden_units": hidden,
                                   "num_cross_layer": 3, "learning_rate": 0.005}, second)}


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def eager_device_ms(model, features, reps):
    from recalgorithm_amd.estimator import ModeKeys
    ts = []
    with torch.no_grad():
        for i in range(reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            model.estimator._call_model_fn(features, None, ModeKeys.PREDICT)
            b.record()
            b.synchronize()
            if i >= 3:
                ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def bench_model(dev, name, model_fn, params, columns, records, tmp, args):
    from recalgorithm_amd import export as E
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd import nn
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    recv = E.build_parsing_serving_input_receiver_fn(fc.make_parse_example_spec(columns))
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=11))
    est.build(recv(records[:16]), None, mode=ModeKeys.PREDICT)
    export_dir = E.export_model(est, os.path.join(tmp, name), recv)
    eager = E.ServingModel(model_fn, params, export_dir, device=dev)
    saved = nn.SERVE_TOWER_MAX_ROWS, nn.SERVE_TOWER_PLAIN_STACKS
    try:
        nn.SERVE_TOWER_MAX_ROWS = 0
        plain = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=SIZES)
        nn.SERVE_TOWER_MAX_ROWS, nn.SERVE_TOWER_PLAIN_STACKS = max(SIZES), True       # (the tower whatever the stack and the size)
        tower = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=SIZES)
    finally:
        nn.SERVE_TOWER_MAX_ROWS, nn.SERVE_TOWER_PLAIN_STACKS = saved
    assert all(b.tower for b in tower._buckets.values()) and not any(b.tower for b in plain._buckets.values())
    dec = eager._open_decoder()[0]
    rows = []
    for n in SIZES:
        req = records[:n]
        reps = max(3, min(args.requests, 4000 // n))
        want = eager.predict(req)["probabilities"]
        for other in (eager.serve(req), plain.serve(req), tower.serve(req)):          # faster and different is not faster
            err = float(abs(other["probabilities"] - want).max())
            assert err <= 1e-4, (name, n, err)
        assert plain._buckets and tower._buckets, "a request dropped the graphs"
        py_decode = median_ms(lambda: recv(req), max(3, reps // 3))
        native_decode = median_ms(lambda: dec.decode(req, threads=eager.DECODE_THREADS if n >= 256 else 0), reps)
        feats = eager._views(eager._decode_to(req, n)[0], n)
        eager_ms = eager_device_ms(eager, feats, max(5, reps // 2))
        (plain_ms, tower_ms), _ = _time_alternating([plain._buckets[n].graph, tower._buckets[n].graph], args.replays)
        e2e = {"predict": median_ms(lambda: eager.predict(req), max(3, reps // 3)), "native_eager": median_ms(lambda: eager.serve(req), reps),
               "compiled": median_ms(lambda: plain.serve(req), reps), "compiled_tower": median_ms(lambda: tower.serve(req), reps)}
        rows.append({"n": n, "paths": {
            "predict": {"decode_ms": py_decode, "device_ms": eager_ms, "end_to_end_ms": e2e["predict"]},
            "native_eager": {"decode_ms": native_decode, "device_ms": eager_ms, "end_to_end_ms": e2e["native_eager"]},
            "compiled": {"decode_ms": native_decode, "device_ms": plain_ms, "end_to_end_ms": e2e["compiled"]},
            "compiled_tower": {"decode_ms": native_decode, "device_ms": tower_ms, "end_to_end_ms": e2e["compiled_tower"]}}})
        print(f"[{name}] n={n}: device ms compiled {plain_ms:.4f} tower {tower_ms:.4f} eager {eager_ms:.3f} | decode ms python "
              f"{py_decode:.3f} native {native_decode:.4f} | end to end ms {e2e}", file=sys.stderr, flush=True)
    return rows


def bench_tower_alone(dev, replays, batch_norm):
    """the hidden stack alone, [B, 416] -> 512 -> 256 -> 128: ONE ops.serve_tower launch against the captured per-layer chain"""
    from recalgorithm_amd import export as E
    from recalgorithm_amd import nn
    from recalgorithm_amd.variables import VariableStore, use_store
    out = []
    for B in SIZES:
        store = VariableStore(dev, seed=3)
        x = torch.randn(B, 416, generator=torch.Generator().manual_seed(B)).to(dev)

        def chain():
            with torch.no_grad(), use_store(store):
                store.begin_call()
                net = x
                for u in UNITS:
                    net = nn.dense_relu_dropout_bn(net, u, 0.0, batch_norm, False)
                return nn._resolved(net)
        store.building = True
        chain()
        store.finalize()
        g = torch.Generator().manual_seed(1)
        for k, v in store.vars.items():                     # BatchNorm statistics of a trained model, not (0, 1)
            if k.endswith("moving_variance"):
                v.data.copy_(0.5 + torch.rand(v.data.shape, generator=g))
            elif k.split("/")[-1] in ("gamma", "beta", "moving_mean", "bias"):
                v.data.copy_((1.0 if k.endswith("gamma") else 0.0) + 0.2 * torch.randn(v.data.shape, generator=g))
        plan = nn.ServingPlan(max(SIZES), E.fold_batch_norms({k: v.data for k, v in store.vars.items()}), nn.BN_EPSILON)
        g_chain, y_chain = _graph(chain)
        store.serving, saved = plan, nn.SERVE_TOWER_PLAIN_STACKS
        nn.SERVE_TOWER_PLAIN_STACKS = True
        try:
            g_tower, y_tower = _graph(chain)
        finally:
            store.serving, nn.SERVE_TOWER_PLAIN_STACKS = None, saved
        g_chain.replay(), g_tower.replay()
        torch.cuda.synchronize()
        err = float((y_chain - y_tower).abs().max() / y_chain.abs().max())
        assert err <= 1e-5, (B, err)
        (chain_ms, tower_ms), (chain_min, tower_min) = _time_alternating([g_chain, g_tower], replays)
        out.append({"B": B, "per_layer_ms": chain_ms, "tower_ms": tower_ms, "per_layer_min_ms": chain_min, "tower_min_ms": tower_min,
                    "max_rel_diff": err})
        print(f"[tower alone, batch_norm={batch_norm}] B={B}: per-layer {chain_ms:.4f} ms, tower {tower_ms:.4f} ms", file=sys.stderr, flush=True)
    return out


def supported_max_rows(rows):
    """the largest n such that compiled_tower's device_ms is no larger than compiled's at n and at every smaller size; 0: none"""
    best = 0
    for r in rows:
        if r["paths"]["compiled_tower"]["device_ms"] > r["paths"]["compiled"]["device_ms"]:
            break
        best = r["n"]
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--requests", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_serving: needs a HIP device (a timing taken anywhere else says nothing)")
    from recalgorithm_amd.io import synth, tfrecord
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        spec = synth.SynthSpec(n_fields=26, max_vocab=100000, seed=41, oov_frac=0.02)
        vocab_dir = os.path.join(tmp, "vocabulary") + "/"
        synth.write_vocabularies(spec, vocab_dir)
        path = os.path.join(tmp, "requests.tfrecord")
        synth.write_tfrecord(spec, path, max(SIZES), chunk=max(SIZES))
        records = list(tfrecord.read_records(path))
        per_model = {name: bench_model(dev, name, fn, params, cols, records, tmp, args)
                     for name, (fn, params, cols) in models(spec, vocab_dir).items()}
    res = {"bench": "serving", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "shape": {"fields": 26, "embedding_dim": 16, "hidden_units": UNITS, "tower_in": 416},
           "request_sizes": SIZES, "replays": args.replays, "models": per_model,
           "tower_alone": {"batch_norm": bench_tower_alone(dev, args.replays, True), "plain": bench_tower_alone(dev, args.replays, False)},
           # DeepFM's stack folds a BatchNorm per layer, DCN's is plain dense(relu): the two settings of recalgorithm_amd/nn.py
           "serve_tower_max_rows": supported_max_rows(per_model["deepfm"]),
           "serve_tower_plain_stacks": supported_max_rows(per_model["dcn"]) >= supported_max_rows(per_model["deepfm"]) > 0}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
