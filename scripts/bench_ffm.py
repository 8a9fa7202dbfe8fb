"""FFM measurements on the MI355X: ops.ffm_interaction on the kernels of csrc/ffm.hip (they fetch the rows themselves) against
the composed chain (gather / bag means -> cat -> recalgo_ffm_pairs_*), and the training step on both paths.  Self-contained:
synthetic inputs from seeds, nothing read from outside the tree.  Prints one JSON line (and writes it with --out).

    python scripts/bench_ffm.py [--replays 200] [--steps 200] [--out profiles/ffm_bench.json]

op:        ops.ffm_interaction(fused=True / False), the forward under no_grad and forward + backward (the lookups' `prepare`
           launches included, the optimizer not), fused and composed in the same call, alternating, medians of three rounds.
             shape one  B 4096, F 26, K 16, every field single-valued (bench.py --model ffm's shape): four captured graphs;
             shape two  B 4096, F 7, K 8, the last field a bag of 0 .. 5 values (the reference's own shape): the composed path
                        synchronises (torch.unique, .item()) and cannot be captured, so both run eagerly, and the fused
                        path once more as graphs.
step:      bench.py --model ffm's estimator (26 fields x 25 sub-tables x emb16, B 4096), captured (GraphedTrainStep), with
           params["ffm_fused"] None and False.  Three runs of each, alternating.
reference: the reference's columns (six single-valued fields and one bag of 0 .. 5 values, K 8, B 4096): the eager step on the
           composed path (what it was) against the captured step on the fused path (the bag padded to its capacity).
Every comparison reports the medians, the spread (max - min) of the composed side's three and `faster_than_spread`."""
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
from scripts.bench_ple import _graph  # noqa: E402


def _rounds(fns, n, rounds=3):
    """fns: name -> callable that enqueues one unit of work.  -> name -> [ms per call] of `rounds` rounds, the names alternating"""
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / n * 1e3)
    return times


def _compare(times, fused, composed):
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(times[composed]) - min(times[composed])
    return {f"{fused}_ms": med[fused], f"{composed}_ms": med[composed], f"{fused}_runs_ms": times[fused],
            f"{composed}_runs_ms": times[composed], "composed_spread_ms": spread, "speedup": med[composed] / med[fused],
            "faster_than_spread": med[composed] - med[fused] > spread, "slower_than_spread": med[fused] - med[composed] > spread}


def _bags(B, vocab, seed, dev):
    from recalgorithm_amd.feature_column import Ragged
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, B)
    values = rng.integers(0, vocab, int(lens.sum())).astype(np.int64)
    values[rng.random(len(values)) < 0.02] = -1
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum(lens)
    return Ragged(torch.from_numpy(values).to(dev), torch.from_numpy(offsets).to(dev))


def bench_op(dev, B, F, K, vocab, with_bag, replays):
    from recalgorithm_amd import ops
    from recalgorithm_amd.variables import EmbeddingArena, VariableStore, use_store
    gen = torch.Generator().manual_seed(100 * F + K)
    store = VariableStore(dev, seed=3)
    arena = store.arenas["emb"] = EmbeddingArena("emb", K, dev, seed=5)
    names = [f"t{i}" for i in range(F)]
    for n in names:
        arena.add_table(n, (F - 1) * vocab)
    arena.materialize()
    single = list(range(F - 1 if with_bag else F))
    ids = torch.randint(0, vocab, (B, len(single)), generator=gen)
    ids[torch.rand(B, len(single), generator=gen) < 0.01] = -1
    ids = ids.to(dev)
    bags = {F - 1: _bags(B, vocab, F, dev)} if with_bag else {}
    g = torch.randn(B, 1, generator=gen).to(dev)
    vocabs = [vocab] * F

    def both(fused):
        def step():
            with use_store(store), torch.enable_grad():
                store.begin_call()
                out = ops.ffm_interaction(store, ids, bags, arena, names, vocabs, F, K, fused=fused)
                out.backward(g)
            return out

        def forward():
            with use_store(store), torch.no_grad():
                store.begin_call()
                return ops.ffm_interaction(store, ids, bags, arena, names, vocabs, F, K, fused=fused)
        return forward, step
    (ff, fs), (cf, cs) = both(True), both(False)
    agree = float((ff() - cf()).abs().max() / cf().abs().max())
    res = {"shape": {"B": B, "F": F, "K": K, "vocab_per_sub_table": vocab, "bag_fields": int(with_bag)},
           "arena_MB": arena.weight.numel() * 4 / 2 ** 20, "fused_vs_composed_max_rel_diff": agree,
           "operand_MB": B * F * (F - 1) * K * 4 / 2 ** 20}
    if not with_bag:
        graphs = {"fused_fwd": _graph(ff)[0], "fused_fwd_bwd": _graph(fs)[0], "composed_fwd": _graph(cf)[0], "composed_fwd_bwd": _graph(cs)[0]}
        t = _rounds({k: v.replay for k, v in graphs.items()}, replays)
        res["captured"] = True
    else:
        t = _rounds({"fused_fwd": ff, "fused_fwd_bwd": fs, "composed_fwd": cf, "composed_fwd_bwd": cs}, max(replays // 4, 10))
        res["captured"] = False                      # (the composed path synchronises: both eager here)
        graphs = {"fused_fwd": _graph(ff)[0], "fused_fwd_bwd": _graph(fs)[0]}
        tg = _rounds({k: v.replay for k, v in graphs.items()}, replays)
        res["fused_captured_fwd_ms"] = statistics.median(tg["fused_fwd"])
        res["fused_captured_fwd_bwd_ms"] = statistics.median(tg["fused_fwd_bwd"])
    res["fwd"] = _compare(t, "fused_fwd", "composed_fwd")
    res["fwd_bwd"] = _compare(t, "fused_fwd_bwd", "composed_fwd_bwd")
    return res


def bench_step(dev, B, steps):
    """bench.py --model ffm's estimator, captured, on both paths"""
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm.FFM.ffm import ffm_model_fn
    from recalgorithm_amd.estimator import Estimator, GraphedTrainStep, RunConfig
    from recalgorithm_amd.io import synth
    runs = {}
    for name, fused in (("fused", None), ("composed", False)):
        spec = synth.SynthSpec(n_fields=26, max_vocab=1_000_000)
        cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
        params = {"one_hot_category_feature_columns": [fc.indicator_column(c) for c in cats], "embedding_dim": 16,
                  "learning_rate": 0.005, "fields_vocabulary_size_tuple": [(c.key, c.num_buckets) for c in cats], "ffm_fused": fused}
        est = Estimator(model_fn=ffm_model_fn, params=params, config=RunConfig(device=dev, seed=42))
        feats, labels, _ = synth.device_features(spec, B, dev)
        est.build(feats, labels)
        runs[name] = GraphedTrainStep(est.train_step, feats, labels, warmup=3)
    t = _rounds({k: (lambda g=g: g()) for k, g in runs.items()}, steps)
    res = _compare(t, "fused", "composed")
    res.update({"batch": B, "fused_examples_per_s": B / (res["fused_ms"] * 1e-3), "composed_examples_per_s": B / (res["composed_ms"] * 1e-3),
                "fused_loss": float(runs["fused"]()), "composed_loss": float(runs["composed"]()),
                "config": "26 fields x 25 sub-tables x emb16, every field single-valued; composed = ffm_fused False, the step as it was"})
    return res


def bench_reference_columns(dev, B, steps):
    """six single-valued fields and one bag of 0 .. 5 values, K 8: eager composed against captured fused"""
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm.FFM.ffm import ffm_model_fn
    from recalgorithm_amd.estimator import Estimator, GraphedTrainStep, RunConfig
    vocabs = {"userid": 20000, "feedid": 100000, "device": 2, "authorid": 18000, "bgm_song_id": 25000, "bgm_singer_id": 17000,
              "manual_tag_list": 350}
    gen = torch.Generator().manual_seed(7)
    feats = {k: torch.randint(0, v, (B,), generator=gen).to(dev) for k, v in vocabs.items() if k != "manual_tag_list"}
    tags = _bags(B, vocabs["manual_tag_list"], 11, dev)
    labels = {"read_comment": (torch.rand(B, 1, generator=gen) < 0.05).float().to(dev)}
    runs, ests = {}, {}
    for name, fused in (("fused_captured", None), ("composed_eager", False)):
        cats = [fc.categorical_column_with_identity(k, v) for k, v in vocabs.items()]
        params = {"one_hot_category_feature_columns": [fc.indicator_column(c) for c in cats], "embedding_dim": 8, "learning_rate": 0.005,
                  "fields_vocabulary_size_tuple": [(c.key, c.num_buckets) for c in cats], "ffm_fused": fused}
        est = ests[name] = Estimator(model_fn=ffm_model_fn, params=params, config=RunConfig(device=dev, seed=42))
        f = dict(feats, manual_tag_list=fc.pad_ragged(tags, 5 * B) if fused is None else tags)
        est.build(f, labels)
        if fused is None:
            g = GraphedTrainStep(est.train_step, f, labels, warmup=3)
            runs[name] = lambda g=g: g()
        else:
            runs[name] = lambda est=est, f=f: est.train_step(f, labels)
    t = _rounds(runs, max(steps // 4, 10))
    res = _compare(t, "fused_captured", "composed_eager")
    res.update({"batch": B, "capture_refused": {k: e.capture_refused or e.store.data_dependent for k, e in ests.items()},
                "config": "userid, feedid, device, authorid, bgm_song_id, bgm_singer_id single-valued + manual_tag_list (0 .. 5 values, "
                          "padded to 5 per example for the capture), K 8"})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out: op, op_reference, step, reference")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ffm.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    skip = set(a.skip.split(","))
    res = {"bench": "ffm", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}
    sections = {"op": lambda: bench_op(dev, a.batch, 26, 16, 10000, False, a.replays),
                "op_reference": lambda: bench_op(dev, a.batch, 7, 8, 20000, True, a.replays),
                "step": lambda: bench_step(dev, a.batch, a.steps),
                "reference": lambda: bench_reference_columns(dev, a.batch, a.steps)}
    for name, fn in sections.items():
        if name in skip:
            continue
        try:
            res[name] = fn()
        except (NotImplementedError, ValueError, TypeError, KeyError, AttributeError) as e:
            # (a host-side refusal: the section says so and the others are still measured; a device error ends the run)
            res[name] = {"error": f"{type(e).__name__}: {e}"}
        print(f"[bench_ffm] {name}: {json.dumps(res[name])}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
