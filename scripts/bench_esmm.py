"""ESMM measurements on the MI355X: the entire-space loss tail (ops.esmm_loss, csrc/esmm.hip) against the same logit-space
arithmetic composed from torch ops and against the two-task sigmoid-CE tail, the full captured ESMM training step beside the MMoE
step, and evaluate() of ESMM with its masked metrics on the host loop, on the device eagerly and captured.  Self-contained:
synthetic inputs from seeds, nothing read from outside the tree.  Prints one JSON line (and writes it with --out).

    python scripts/bench_esmm.py [--replays 200] [--steps 200] [--out profiles/esmm_bench.json]

tail:  forward + backward (both logit gradients) at B 4096 and B 65536, logits N(0, 3), click 30 %, conversion 40 %:
         fused      ops.esmm_loss: one launch
         composed   (a) include/recalgo_esmm.h's arithmetic from torch ops (softplus, logsumexp, autograd)
         multitask  (b) ops.multitask_sigmoid_cross_entropy with T = 2 at the same B: the yardstick for "a loss tail's launch"
       each captured once as one graph; the three graphs alternate in one call, medians of three rounds.
step:  synthetic 8 single-valued fields (emb 16,16,16,4,4,4,4,2) + 16 dense features = 82 inputs, two towers 512,256,128 with
       BatchNorm and dropout 0.1, B 4096, captured (GraphedTrainStep); the MMoE step of scripts/bench_mmoe.py in the same call.
eval:  evaluate() over 64 device-resident batches of 4096 after three training steps, the arms of scripts/bench_eval.py
       alternating; their result dicts must be equal.
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
from scripts.bench_ple import _graph, _time_alternating, count_launches  # noqa: E402

DIMS = (16, 16, 16, 4, 4, 4, 4, 2)      # + 16 dense features = MMoE's 82 inputs


def softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def composed(a, b, y, c):
    """the header's arithmetic from framework ops: what the fused kernel replaces -> (total, losses, prob)"""
    z = y * c
    l_ctr = (torch.clamp(a, min=0) - a * y + torch.log1p(torch.exp(-a.abs()))).mean()
    log_p = -softplus(-a) - softplus(-b)
    lam = torch.logsumexp(torch.stack([-a, -b, -a - b], dim=1), dim=1)
    l_ctcvr = (-z * log_p - (1 - z) * (lam + log_p)).mean()
    p_ctr, p_cvr = torch.sigmoid(a), torch.sigmoid(b)
    return l_ctr + l_ctcvr, torch.stack([l_ctr, l_ctcvr]), torch.stack([p_ctr, p_cvr, p_ctr * p_cvr], dim=1)


def bench_tail(dev, B, replays):
    from recalgorithm_amd import ops
    gen = torch.Generator().manual_seed(B)
    a, b = (3.0 * torch.randn(B, generator=gen)).to(dev).requires_grad_(True), (3.0 * torch.randn(B, generator=gen)).to(dev).requires_grad_(True)
    y, c = (torch.rand(B, generator=gen) < 0.3).float().to(dev), (torch.rand(B, generator=gen) < 0.4).float().to(dev)

    def run(tail):
        def fn():
            total, losses, prob = tail()
            return [total.detach(), losses.detach(), prob.detach()] + list(torch.autograd.grad(total, [a, b]))
        return fn
    fns = [run(lambda: ops.esmm_loss(a, b, y, c)), run(lambda: composed(a, b, y, c)),
           run(lambda: ops.multitask_sigmoid_cross_entropy([a.reshape(-1, 1), b.reshape(-1, 1)], [y.reshape(-1, 1), c.reshape(-1, 1)]))]
    u, v = fns[0](), fns[1]()
    agree = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(u, v))
    graphs = [_graph(fn)[0] for fn in fns]
    rounds = [_time_alternating(graphs, replays) for _ in range(3)]
    med = [statistics.median(r_[0][i] for r_ in rounds) for i in range(3)]
    mins = [min(r_[1][i] for r_ in rounds) for i in range(3)]
    return {"B": B, "fused_vs_composed_max_rel_diff": agree, "fused_ms": med[0], "composed_ms": med[1], "multitask_t2_ms": med[2],
            "fused_min_ms": mins[0], "composed_min_ms": mins[1], "multitask_t2_min_ms": mins[2],
            "composed_over_fused": med[1] / med[0], "fused_over_multitask_t2": med[0] / med[2]}


def funnel_labels(B, dev, i):
    """clicks 30 %, conversions 40 %, drawn here (synth's labels are independent 2 % draws: almost no conversions)"""
    g = torch.Generator().manual_seed(977 + i)
    return {"click_avatar": (torch.rand(B, 1, generator=g) < 0.3).float().to(dev), "follow": (torch.rand(B, 1, generator=g) < 0.4).float().to(dev)}


def make_estimator(dev, B, seed=5):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import dense_columns
    from recalgorithm_amd.algorithm.ESMM.esmm import esmm_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=8, max_vocab=100000, seed=11, oov_frac=0.05, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": dense_columns(), "category_feature_columns": [fc.embedding_column(c, k) for c, k in zip(cats, DIMS)],
              "hidden_units": ["512", "256", "128"], "dropout_rate": 0.1, "batch_norm": True, "learning_rate": 0.005,
              "ctr_task_name": "click_avatar", "cvr_task_name": "follow"}
    est = Estimator(esmm_model_fn, params, RunConfig(device=dev, seed=seed))
    feats = synth.device_features(spec, B, dev)[0]
    labels = funnel_labels(B, dev, 0)
    est.build(feats, labels)
    return est, spec, feats, labels


def windows_of(g, steps):
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
    return windows


def bench_steps(dev, B, steps):
    """the captured ESMM step and the captured MMoE step of scripts/bench_mmoe.py, two rounds each, alternating"""
    from recalgorithm_amd.estimator import GraphedTrainStep
    from scripts.bench_mmoe import make_estimator as make_mmoe
    est, _, feats, labels = make_estimator(dev, B)
    mm, mfeats, mlabels = make_mmoe(dev, B)
    graphs = {"esmm": GraphedTrainStep(est.train_step, feats, labels, warmup=3), "mmoe": GraphedTrainStep(mm.train_step, mfeats, mlabels, warmup=3)}
    runs = {"esmm": [], "mmoe": []}
    for _ in range(2):
        for name, g in graphs.items():
            runs[name] += windows_of(g, steps)
    loss = {name: float(g()) for name, g in graphs.items()}
    out = {}
    for name, ws in runs.items():
        ms = statistics.median(ws) * 1e3
        out[name] = {"batch": B, "step_ms": ms, "examples_per_s": B / (ms * 1e-3), "step_ms_min": min(ws) * 1e3, "loss": loss[name]}
    est2, _, feats2, labels2 = make_estimator(dev, B)
    n_launch, by_name = count_launches(est2, feats2, labels2)
    out["esmm"].update(kernel_launches_per_eager_step=n_launch, most_launched=by_name,
                       config="two towers 512,256,128; BN; dropout 0.1; In 82; click 30 %, conversion 40 %")
    mm2, mfeats2, mlabels2 = make_mmoe(dev, B)
    out["mmoe"].update(kernel_launches_per_eager_step=count_launches(mm2, mfeats2, mlabels2)[0],
                       config="scripts/bench_mmoe.py: hidden 512,256,128; 3 experts x 512; 3 tasks; BN; dropout 0.1; In 82")
    out["esmm_over_mmoe_examples_per_s"] = out["esmm"]["examples_per_s"] / out["mmoe"]["examples_per_s"]
    return out


def bench_eval(dev, B, n_batches, repeats):
    from recalgorithm_amd.io import synth
    est, spec, _, _ = make_estimator(dev, B, seed=11)
    batches = [(synth.device_features(spec, B, dev, batch_index=i)[0], funnel_labels(B, dev, i)) for i in range(n_batches)]
    est.train(lambda: iter(batches[:3]), log_every=0)
    arms = {"host_metrics": dict(device_metrics=False, use_hip_graph=True), "device_eager": dict(device_metrics=True, use_hip_graph=False),
            "device_captured": dict(device_metrics=True, use_hip_graph=True)}

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
        assert results[arm] == run(arm)[1], (arm, "two calls of evaluate() differ")
    first = next(iter(results.values()))
    assert all(r == first for r in results.values()), results
    times = {arm: [] for arm in arms}
    for _ in range(repeats):
        for arm in arms:
            times[arm].append(run(arm)[0])
    rows = {}
    for arm, ts in times.items():
        t = statistics.median(ts)
        rows[arm] = {"examples_per_s": n_batches * B / t, "ms_per_batch": t * 1e3 / n_batches, "evaluate_ms": t * 1e3,
                     "evaluate_ms_min": min(ts) * 1e3, "evaluate_ms_max": max(ts) * 1e3}
    return {"batch": B, "batches": n_batches, "repeats": repeats, "arms": rows, "slots": 6, "masked_slots": 2, "result": first,
            "captured_over_host": rows["device_captured"]["examples_per_s"] / rows["host_metrics"]["examples_per_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_esmm.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "esmm", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "tail": [bench_tail(dev, B, a.replays) for B in (4096, 65536)],
           "step": bench_steps(dev, 4096, a.steps),
           "evaluate": bench_eval(dev, 4096, a.batches, a.repeats)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
