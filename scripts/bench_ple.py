"""PLE measurements on the MI355X (bench.py is the project's yardstick and has no PLE entry): the CGC op at the two block
shapes of the reference's default configuration against the same block composed from what the tree offered before it, the
expert GEMMs of both blocks on their own, and the full training step.  Self-contained: synthetic inputs from seeds, nothing
read from outside the tree.  Prints one JSON line (and writes it with --out).

    python scripts/bench_ple.py [--batch 4096] [--replays 200] [--steps 200] [--out profiles/ple_bench.json]
    python scripts/bench_ple.py --trace-step      # a few captured steps and nothing else: the run to put under
                                                  # `rocprofv3 --kernel-trace --stats -- python scripts/bench_ple.py --trace-step`

op:      forward + backward + the deferred-sum launch of the gate kernels' gradients, under hipGraph replay, fused
         (ops.cgc_mix) and baseline (the composition the reference graph implies: G bias-free dense layers on the MFMA engine
         + torch.softmax + torch.stack / torch.bmm per gate (+ the adds of tf.add_n in the summed block) with autograd's
         backward) alternating in one process on the same inputs; medians over the replays.  A forward-only graph of the fused
         op is timed in the same alternation: backward (+ reduction) = pair - forward.
bytes:   the algorithmic traffic of the fused kernels (fp32), M = 1 output (summed block) or G: forward reads E [B, H] tensors
         and x, writes M [B, H] tensors and p; backward reads E + M and writes E [B, H] tensors, reads x and p, writes dx and
         the partial rows.  Fraction = bytes / time / the 6.3 TB/s achievable copy rate; the working set (105 MB of experts)
         fits the 256 MB Infinity Cache, so a fraction can exceed what HBM alone allows.
experts: nn.expert_layers alone at each block's shape (25 GEMM launches forward; 25 merged input- / weight-gradient launches
         and the deferred sums backward), under hipGraph replay: the share of the step that a grouped expert GEMM could win.
step:    the mirrored model_fn at the reference's default configuration, captured (GraphedTrainStep), examples/s; the
         kernel launches of ONE eager step counted with torch.profiler (None where the profiler is not available).
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
PER_TASK, SHARED, H = (5, 5, 5), 10, 256


def selection(all_gate):
    starts = [sum(PER_TASK[:t]) for t in range(len(PER_TASK))]
    shared = list(range(sum(PER_TASK), sum(PER_TASK) + SHARED))
    sel = [list(range(s, s + n)) + shared for s, n in zip(starts, PER_TASK)]
    return sel + [list(range(sum(PER_TASK) + SHARED))] if all_gate else sel


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


def bench_op(dev, B, In, sel, sum_outputs, replays):
    from recalgorithm_amd import _lib, nn, ops
    from recalgorithm_amd.variables import VariableStore, use_store
    E, G, NT = sum(PER_TASK) + SHARED, len(sel), sum(len(s) for s in sel)
    M = 1 if sum_outputs else G
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, In, generator=gen).to(dev).requires_grad_(True)
    experts = [torch.relu(torch.randn(B, H, generator=gen)).to(dev).requires_grad_(True) for _ in range(E)]
    gouts = [torch.randn(B, H, generator=gen).to(dev) for _ in range(M)]
    store = VariableStore(dev, seed=3)
    with use_store(store):
        kernels = [store.get_variable(f"gate_{g}/kernel", (In, len(s))) for g, s in enumerate(sel)]
        store.pack()

        def outs_of(r):
            return [r] if sum_outputs else list(r)

        def fused():
            outs = outs_of(ops.cgc_mix(x, kernels, experts, sel, sum_outputs=sum_outputs, anchor=store.anchor))
            grads = torch.autograd.grad(outs, [x, *experts], gouts)
            ops.flush_dense_splits()
            return [*outs, *grads]

        def fused_forward():
            with torch.no_grad():
                return outs_of(ops.cgc_mix(x, kernels, experts, sel, sum_outputs=sum_outputs, anchor=store.anchor))

        def baseline():
            outs = []
            for k, s in zip(kernels, sel):
                gate = torch.softmax(nn.dense_with(x, k), dim=-1)
                stack = torch.stack([experts[e] for e in s], dim=1)                   # [B, n_g, H]
                outs.append(torch.bmm(stack.transpose(1, 2), gate.unsqueeze(-1)).squeeze(-1))
            if sum_outputs:                                                           # tf.add_n
                total = outs[0]
                for o in outs[1:]:
                    total = total + o
                outs = [total]
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
        g0, _ = _graph(fused_forward)
        (tf, tb, t0), (mf, mb, m0) = _time_alternating([gf, gb, g0], replays)
    rows = int(_lib.load().recalgo_cgc_partial_rows(B, In, NT))
    fwd_bytes = 4 * (E * B * H + M * B * H + B * In + B * NT)
    bwd_bytes = 4 * ((E + M) * B * H + E * B * H + 2 * B * In + B * NT + rows * In * NT)
    return {"shape": {"B": B, "In": In, "E": E, "G": G, "H": H, "NT": NT, "sum_outputs": bool(sum_outputs)},
            "fused_ms": tf, "baseline_ms": tb, "fused_min_ms": mf, "baseline_min_ms": mb, "speedup": tb / tf,
            "fused_forward_ms": t0, "fused_forward_min_ms": m0, "fused_backward_and_reduce_ms": tf - t0,
            "fused_vs_baseline_max_rel_diff": worst,
            "algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
            "forward_fraction_of_copy_rate": fwd_bytes / (t0 * 1e-3) / COPY_RATE,
            "backward_fraction_of_copy_rate": bwd_bytes / ((tf - t0) * 1e-3) / COPY_RATE,
            "note": "backward = (fwd + bwd + reduction replay) - (forward-only replay); the working set fits the Infinity Cache"}


def bench_experts(dev, B, In, replays):
    """nn.expert_layers alone: 25 experts of H units over one [B, In] input, forward and backward"""
    from recalgorithm_amd import nn, ops
    from recalgorithm_amd.variables import VariableStore, use_store, variable_scope
    E = sum(PER_TASK) + SHARED
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(B, In, generator=gen).to(dev).requires_grad_(True)
    gouts = [torch.randn(B, H, generator=gen).to(dev) for _ in range(E)]
    store = VariableStore(dev, seed=3)
    with use_store(store):
        store.building = True
        with variable_scope("experts"):
            nn.expert_layers(x, H, E)
        store.building = False
        store.pack()

        def fwd_bwd():
            with variable_scope("experts"):
                ys = nn.expert_layers(x, H, E)
            (dx,) = torch.autograd.grad(ys, [x], gouts)
            ops.flush_dense_splits()
            return dx

        def fwd():
            with torch.no_grad(), variable_scope("experts"):
                return nn.expert_layers(x, H, E)
        g1, _ = _graph(fwd_bwd)
        g0, _ = _graph(fwd)
        (t1, t0), _ = _time_alternating([g1, g0], replays)
    flops = 2.0 * B * In * H * E
    return {"shape": {"B": B, "In": In, "E": E, "H": H}, "forward_ms": t0, "backward_ms": t1 - t0, "forward_and_backward_ms": t1,
            "forward_tflops": flops / (t0 * 1e-3) / 1e12, "launches_forward": E}


def make_estimator(dev, B):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import dense_columns
    from recalgorithm_amd.algorithm.PLE.ple import ple_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=8, max_vocab=100000, seed=11, oov_frac=0.05, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    dims = (16, 16, 16, 4, 4, 4, 4, 2)      # + 16 dense features = the reference's 82 inputs
    params = {"dense_feature_columns": dense_columns(), "category_feature_columns": [fc.embedding_column(c, k) for c, k in zip(cats, dims)],
              "hidden_units": ["512", "256", "128"], "dropout_rate": 0.1, "batch_norm": True, "learning_rate": 0.005,
              "num_tasks": 3, "expert_hidden_units": H, "task_names": list(TASKS), "num_extract_network": 1,
              "num_experts_per_task": list(PER_TASK), "num_experts_in_shared": SHARED}
    est = Estimator(ple_model_fn, params, RunConfig(device=dev, seed=5))
    feats, labels, _ = synth.device_features(spec, B, dev, extra_labels=TASKS[1:])
    est.build(feats, labels)
    return est, feats, labels


def count_launches(est, feats, labels):
    """kernel launches of one eager training step, by torch.profiler; (None, {}) where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        for _ in range(3):
            est.train_step(feats, labels)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            est.train_step(feats, labels)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if getattr(e, "device_type", None) is not None
                 and "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        if not names:
            return None, {}
        top = {}
        for n in names:
            key = n.replace("(anonymous namespace)::", "").replace("void ", "").split("<")[0].split("(")[0][-60:]
            top[key] = top.get(key, 0) + 1
        return len(names), dict(sorted(top.items(), key=lambda kv: -kv[1])[:12])
    except Exception as e:              # noqa: BLE001  (a measurement aid: the timings below do not depend on it)
        return None, {"error": f"{type(e).__name__}: {e}"[:200]}


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
    loss = float(g())
    est2, feats2, labels2 = make_estimator(dev, B)
    n_launch, by_name = count_launches(est2, feats2, labels2)
    return {"batch": B, "step_ms": ms, "examples_per_s": B / (ms * 1e-3), "step_ms_min": min(windows) * 1e3, "loss": loss,
            "kernel_launches_per_eager_step": n_launch, "most_launched": by_name,
            "config": "hidden 512,256,128; 5+5+5 task + 10 shared experts x 256; 1 extraction network; 3 tasks; BN; dropout 0.1; In 82"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ple.py measures on a HIP device; none found")
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
    res = {"bench": "ple", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "op_level0": bench_op(dev, a.batch, 82, selection(True), True, a.replays),        # extraction network: summed
           "op_final": bench_op(dev, a.batch, 256, selection(False), False, a.replays),      # final CGC: three outputs
           "experts_level0": bench_experts(dev, a.batch, 82, a.replays),
           "experts_final": bench_experts(dev, a.batch, 256, a.replays),
           "step": bench_step(dev, a.batch, a.steps)}
    ex = res["experts_level0"]["forward_and_backward_ms"] + res["experts_final"]["forward_and_backward_ms"]
    cgc = res["op_level0"]["fused_ms"] + res["op_final"]["fused_ms"]
    res["share_of_step"] = {"expert_gemms_2x25_each_way": ex / res["step"]["step_ms"], "cgc_kernels": cgc / res["step"]["step_ms"],
                            "note": "isolated hipGraph replays over the captured step's time: in the step the launches overlap nothing "
                                    "(one stream), so the shares are comparable; cache state differs"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
