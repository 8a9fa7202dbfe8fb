"""Ragged inputs of fixed capacity on the MI355X (bench.py is the project's yardstick and feeds histories of one length): DCN with the
reference's columns — six id columns, the `manual_tag_list` bag (0..5 values), the `his_read_comment_7d_seq` bag (0..50 values),
16 dense features — on synthetic batches whose bag lengths really vary (SynthSpec.history_len unset).  Three legs, each in a child
process of its own under a time limit; the parent never opens the GPU:

    train     B = 4096, 32 rotating device-resident batches.  RunConfig(ragged_capacity=None) — every step eager, what the tree did
              before ragged capacities — and ragged_capacity="auto" in the same process, the arms alternating: ms per step (wall
              clock around the steps after the capture, the device drained at both ends), library launches of one eager step, the
              share of batches that overflowed.  A captured figure counts only if that share is at most 5 %; the nnz of the
              generated batches is checked against the auto capacity on the CPU first.
    kernel    the bag backward at the batch's two bag shapes (K = 4 and 16): recalgo_bag_mean_grad_rows against the torch
              composition it replaced, 200 launches each inside one captured graph, device time per launch.
    serving   serve() of 4096 and of 1 records with compile(ragged_capacity=...) against the eager serve(), end to end.

    python scripts/bench_ragged.py [--steps 400] [--out profiles/ragged_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N_BATCHES, HIDDEN = 4096, 32, "512,256,128"
LEG_SECONDS = {"train": 420, "kernel": 120, "serving": 420}


def _spec():
    from recalgorithm_amd.io import synth
    return synth.SynthSpec(n_fields=6, max_vocab=100000, seed=17, oov_frac=0.02, with_dense=True, with_history=True, with_tags=True)


def _dcn(vocab_dir):
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.DCN import dcn
    flags.FLAGS.vocabulary_dir = vocab_dir
    dense, cat, _ = dcn.create_feature_columns()
    params = {"category_feature_columns": cat, "dense_feature_columns": dense, "hidden_units": HIDDEN.split(","), "num_cross_layer": 1,
              "learning_rate": 0.005}
    return dcn.dcn_model_fn, params, dense + cat


class _Counting:
    """the loaded library, counting the calls of each recalgo_* entry"""

    def __init__(self, lib):
        self.__dict__.update(lib=lib, calls=0)

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("recalgo_"):
            return fn

        def call(*a):
            self.__dict__["calls"] += 1
            return fn(*a)
        return call


def leg_train(args):
    import torch
    from recalgorithm_amd import _lib
    from recalgorithm_amd.estimator import Estimator, RunConfig, ragged_auto_capacity
    from recalgorithm_amd.feature_column import Ragged
    from recalgorithm_amd.io import synth
    dev, spec = torch.device("cuda:0"), _spec()
    with tempfile.TemporaryDirectory() as tmp:
        synth.write_vocabularies(spec, tmp + "/")
        model_fn, params, _ = _dcn(tmp + "/")
        batches = [synth.device_features(spec, B, dev, batch_index=i)[:2] for i in range(N_BATCHES)]
        nnz = {k: [int(f[k].values.numel()) for f, _ in batches] for k, v in batches[0][0].items() if isinstance(v, Ragged)}
        # the CPU check: what "auto" settles on after the two warm-up batches, against every batch's nnz
        caps = {k: ragged_auto_capacity(max(v[:2])) for k, v in nnz.items()}
        expected_overflow = sum(any(nnz[k][i] > caps[k] for k in nnz) for i in range(N_BATCHES)) / N_BATCHES
        warm = 8                                 # steps before the clock starts: warm-up, capture, first replays

        def run(policy, steps):
            est = Estimator(model_fn, params, RunConfig(device=dev, seed=11, ragged_capacity=policy))
            t = {}

            def feed():
                for i in range(steps):
                    if i == warm:
                        torch.cuda.synchronize()
                        t["start"] = time.perf_counter()
                    yield batches[i % N_BATCHES]
            est.train(feed, log_every=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t["start"]) * 1e3 / (steps - warm)
            return ms, est
        times, ests = {"eager": [], "auto": []}, {}
        for _ in range(args.repeats):
            for arm, policy in (("eager", None), ("auto", "auto")):
                ms, ests[arm] = run(policy, args.steps)
                times[arm].append(ms)
        # library launches of one eager step (the captured arm replays them as one graph launch)
        counting, real = _Counting(_lib.load()), _lib.load
        _lib.load = lambda *a, **k: counting
        try:
            ests["eager"].train_step(*batches[0])
        finally:
            _lib.load = real
        auto = ests["auto"]
        share = auto.ragged_overflows / args.steps
        return {"shape": {"batch": B, "batches": N_BATCHES, "hidden_units": HIDDEN, "nnz_manual_tag_list": [min(nnz["manual_tag_list"]), max(nnz["manual_tag_list"])],
                          "nnz_his_read_comment_7d_seq": [min(nnz["his_read_comment_7d_seq"]), max(nnz["his_read_comment_7d_seq"])]},
                "steps": args.steps, "timed_steps": args.steps - warm, "repeats": args.repeats,
                "eager_ms_per_step": statistics.median(times["eager"]), "eager_ms_per_step_all": times["eager"],
                "captured_ms_per_step": statistics.median(times["auto"]), "captured_ms_per_step_all": times["auto"],
                "speedup": statistics.median(times["eager"]) / statistics.median(times["auto"]),
                "library_launches_per_eager_step": counting.calls, "graph_launches_per_captured_step": 1,
                "graph_replays": auto.graph_replays, "capture_refused": auto.capture_refused, "auto_capacity": auto._ragged_caps,
                "overflow_share": share, "overflow_share_expected_from_nnz": expected_overflow, "captured_figure_counts": share <= 0.05}


def leg_kernel(args):
    import torch
    from recalgorithm_amd import ops
    from recalgorithm_amd.io import synth
    from scripts.bench_ple import _time_alternating
    dev, spec = torch.device("cuda:0"), _spec()
    feats, _, _ = synth.device_features(spec, B, dev, batch_index=0)
    out = {}
    for key, K in (("manual_tag_list", 4), ("his_read_comment_7d_seq", 16)):
        values, offsets = feats[key].values.contiguous(), feats[key].offsets.contiguous()
        g = torch.randn(B, K, generator=torch.Generator().manual_seed(K)).to(dev)
        rows = torch.empty(values.numel(), K, device=dev)

        def composition():
            bag = torch.searchsorted(offsets[1:], torch.arange(values.numel(), device=dev), right=True).clamp_(max=B - 1)
            cnt = torch.zeros(B, device=dev).index_add_(0, bag, (values >= 0).float()).clamp_(min=1.0)
            return g[bag] / cnt[bag].unsqueeze(1)

        def kernel():
            return ops.bag_mean_grad_rows(values, offsets, g, out=rows)
        ok = values >= 0
        assert torch.equal(composition()[ok], kernel()[ok]), key
        graphs = []
        for fn in (composition, kernel):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(200):
                    fn()
            graphs.append(gr)
        (comp_ms, kern_ms), _ = _time_alternating(graphs, 50, inner=1)
        out[key] = {"nnz": int(values.numel()), "K": K, "composition_us": comp_ms * 1e3 / 200, "kernel_us": kern_ms * 1e3 / 200,
                    "speedup": comp_ms / kern_ms, "rows_bytes": int(values.numel()) * K * 4}
    return out


def leg_serving(args):
    import torch
    from recalgorithm_amd import export as E
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    from recalgorithm_amd.io import synth, tfrecord
    dev, spec = torch.device("cuda:0"), _spec()
    with tempfile.TemporaryDirectory() as tmp:
        synth.write_vocabularies(spec, tmp + "/")
        path = os.path.join(tmp, "requests.tfrecord")
        synth.write_tfrecord(spec, path, 4096, chunk=4096)
        records = list(tfrecord.read_records(path))
        model_fn, params, columns = _dcn(tmp + "/")
        recv = E.build_parsing_serving_input_receiver_fn(fc.make_parse_example_spec(columns))
        est = Estimator(model_fn, params, RunConfig(device=dev, seed=11))
        est.build(recv(records[:16]), None, mode=ModeKeys.PREDICT)
        export_dir = E.export_model(est, os.path.join(tmp, "dcn"), recv)
        eager = E.ServingModel(model_fn, params, export_dir, device=dev)
        graphs = E.ServingModel(model_fn, params, export_dir, device=dev).compile(
            batch_sizes=(1, 4096), ragged_capacity={"manual_tag_list": 5, "his_read_comment_7d_seq": spec.max_history})
        out = {}
        for n in (1, 4096):
            req = records[:n]
            want, got = eager.serve(req), graphs.serve(req)      # (the first request teaches both decoders the two bags)
            assert graphs.compiled_buckets == [1, 4096] and graphs.ragged_overflows == 0
            assert all((want[k] == got[k]).all() for k in want), "faster and different is not faster"
            reps = 200 if n == 1 else 15
            ms = {}
            for _ in range(3):
                for arm, model in (("eager", eager), ("compiled", graphs)):
                    ts = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        model.serve(req)
                        ts.append((time.perf_counter() - t0) * 1e3)
                    ms.setdefault(arm, []).append(statistics.median(ts))
            out[str(n)] = {"eager_ms": statistics.median(ms["eager"]), "compiled_ms": statistics.median(ms["compiled"]),
                           "speedup": statistics.median(ms["eager"]) / statistics.median(ms["compiled"]), "requests": reps * 3}
        out["ragged_overflows"] = graphs.ragged_overflows
        return out


LEGS = {"train": leg_train, "kernel": leg_kernel, "serving": leg_serving}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process and print its JSON")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_ragged: needs a HIP device (a timing taken anywhere else says nothing)")
        res = LEGS[args.leg](args)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return
    res = {"bench": "ragged", "date": time.strftime("%Y-%m-%d")}
    for leg in ("train", "kernel", "serving"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--steps", str(args.steps), "--repeats", str(args.repeats)]
        try:
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=LEG_SECONDS[leg])
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_ragged: the {leg} leg ran past {LEG_SECONDS[leg]} s; nothing further is started")
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:            # (after a failed GPU step nothing further is started)
            sys.exit(f"bench_ragged: the {leg} leg failed with exit status {p.returncode}\n{p.stderr[-3000:]}")
        res[leg] = json.loads(line[len("RESULT "):])
        res.setdefault("device", res[leg].pop("device"))
        print(f"[{leg}] {json.dumps(res[leg])}", file=sys.stderr, flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
