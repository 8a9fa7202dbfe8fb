"""DIEN interest-module measurements on the MI355X (bench.py is the project's yardstick and has no DIEN entry): each of the four
entries of include/recalgo_dien.h alone, the module (GRU -> attention -> AUGRU) through ops.dien_gru / ops.dien_evolve, and the
same module composed from torch ops step by step on the same device — what a framework executes for it: per step a concat, a
matmul, a sigmoid, a split, a second concat and matmul, a tanh, the blend and the sequence_length select, T times, twice.
Self-contained: synthetic inputs from seeds, nothing read from outside the tree.  Prints one JSON line (and writes it with
--out).

    python scripts/bench_dien.py [--batch 4096] [--replays 200] [--steps 200] [--out profiles/dien_bench.json]

Every timed thing is ONE captured hipGraph (the composed module too: its thousands of launches replay without the host), the
graphs alternate in one process, medians over the replays.  Two length distributions: `zipf` (io/synth.zipf_ids over 0..T:
most histories are short, which the kernels skip and the composed module cannot) and `full` (every history T long).
step: the mirrored dien_model_fn captured (GraphedTrainStep) at B = 4096: ms, examples/s, the launches of one eager step."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_ple import _graph, _time_alternating  # noqa: E402

MASK_VALUE = -4294967296.0
CELL = ("Wg", "bg", "Wc", "bc")
ECELL = ("w_att", "eWg", "ebg", "eWc", "ebc")


def make_inputs(B, T, na, nh, dev, lengths, seed=1):
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return ((torch.rand(*shape, generator=gen) * 2 - 1) * scale).to(dev)

    def glorot(r, c):
        return rnd(r, c, scale=math.sqrt(6.0 / (r + c)))
    return {"x": rnd(B, T, na), "target": rnd(B, na), "lengths": lengths.to(torch.int32).to(dev), "g_h": rnd(B, T, nh),
            "g_final": rnd(B, nh), "Wg": glorot(na + nh, 2 * nh), "bg": 1 + rnd(2 * nh, scale=0.2), "Wc": glorot(na + nh, nh),
            "bc": rnd(nh, scale=0.2), "w_att": glorot(nh, na), "eWg": glorot(2 * nh, 2 * nh), "ebg": 1 + rnd(2 * nh, scale=0.2),
            "eWc": glorot(2 * nh, nh), "ebc": rnd(nh, scale=0.2)}


def composed_recurrence(x, live, Wg, bg, Wc, bc, att=None):
    B, T, _ = x.shape
    nh = bc.shape[0]
    h = x.new_zeros(B, nh)
    outs = []
    for t in range(T):
        g = torch.sigmoid(torch.cat([x[:, t], h], dim=1) @ Wg + bg)
        r, u = g[:, :nh], g[:, nh:]
        c = torch.tanh(torch.cat([x[:, t], r * h], dim=1) @ Wc + bc)
        if att is not None:
            u = (1 - att[:, t:t + 1]) * u
        new = u * h + (1 - u) * c
        m = live[:, t:t + 1]
        h = torch.where(m, new, h)
        outs.append(torch.where(m, new, torch.zeros_like(new)))
    return torch.stack(outs, dim=1), h


def composed_module(c, x, target, p):
    """GRU (with lengths, as the product calls it) -> attention -> AUGRU, torch fp32"""
    h, _ = composed_recurrence(x, c["live"], *p[:4])
    s = torch.einsum("btj,bj->bt", h, target @ p[4].t())
    att = torch.softmax(torch.where(c["live"], s, torch.full_like(s, MASK_VALUE)), dim=1)
    return composed_recurrence(h, c["live"], *p[5:], att=att)[1]


def bench_module(dev, B, T, na, nh, lengths, replays):
    from recalgorithm_amd import _lib, ops
    c = make_inputs(B, T, na, nh, dev, lengths)
    c["live"] = torch.arange(T, device=dev)[None, :] < c["lengths"][:, None]
    lib = _lib.load()
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    mode = ops.DIEN_MODES["AUGRU"]
    h, states = torch.empty(B, T, nh, device=dev), torch.empty(B, T, nh, device=dev)
    att, final = torch.empty(B, T, device=dev), torch.empty(B, nh, device=dev)
    dx, dh, dtarget = torch.empty(B, T, na, device=dev), torch.empty(B, T, nh, device=dev), torch.empty(B, na, device=dev)
    gg, ge = [torch.empty_like(c[k]) for k in CELL], [torch.empty_like(c[k]) for k in ECELL]
    ws_g = torch.empty(int(lib.recalgo_dien_gru_bwd_workspace_bytes(B, na, nh)), dtype=torch.uint8, device=dev)
    ws_e = torch.empty(int(lib.recalgo_dien_evolve_bwd_workspace_bytes(B, na, nh)), dtype=torch.uint8, device=dev)
    ev_in = [P(h), P(c["target"]), P(c["lengths"]), *[P(c[k]) for k in ECELL]]

    def gru_fwd():
        lib.recalgo_dien_gru_fwd(P(c["x"]), P(c["lengths"]), *[P(c[k]) for k in CELL], B, T, na, nh, P(h), st())

    def gru_bwd():
        lib.recalgo_dien_gru_bwd(P(c["x"]), P(c["lengths"]), P(h), *[P(c[k]) for k in CELL], P(c["g_h"]), B, T, na, nh, P(dx),
                                 *[P(t) for t in gg], P(ws_g), st())

    def evolve_fwd():
        lib.recalgo_dien_evolve_fwd(*ev_in, B, T, na, nh, mode, P(att), P(states), P(final), st())

    def evolve_bwd():
        lib.recalgo_dien_evolve_bwd(*ev_in, P(att), P(states), P(c["g_final"]), B, T, na, nh, mode, P(dh), P(dtarget),
                                    *[P(t) for t in ge], P(ws_e), st())
    gru_fwd(), evolve_fwd()
    names = ["gru_fwd", "gru_bwd", "evolve_fwd", "evolve_bwd"]
    entries = (gru_fwd, gru_bwd, evolve_fwd, evolve_bwd)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("x", "target") + CELL + ECELL}
    params = [leaves[k] for k in CELL + ECELL]

    def fused():
        for t in leaves.values():
            t.grad = None
        hh = ops.dien_gru(leaves["x"], c["lengths"], *params[:4])
        f = ops.dien_evolve(hh, leaves["target"], c["lengths"], *params[4:], mode="AUGRU")[0]
        f.backward(c["g_final"])
        return f

    def fused_forward():
        with torch.no_grad():
            hh = ops.dien_gru(leaves["x"], c["lengths"], *params[:4])
            return ops.dien_evolve(hh, leaves["target"], c["lengths"], *params[4:], mode="AUGRU")[0]

    def composed():
        for t in leaves.values():
            t.grad = None
        f = composed_module(c, leaves["x"], leaves["target"], params)
        f.backward(c["g_final"])
        return f

    def composed_forward():
        with torch.no_grad():
            return composed_module(c, leaves["x"], leaves["target"], params)
    a, gx = fused().detach().clone(), leaves["x"].grad.clone()
    b, rx = composed().detach().clone(), leaves["x"].grad.clone()
    agree = {"final": float((a - b).abs().max() / b.abs().max()), "dx": float((gx - rx).abs().max() / rx.abs().max())}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        composed()
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t0) / 3 * 1e3
    graphs = [_graph(f)[0] for f in entries + (fused, fused_forward, composed, composed_forward)]
    med, mins = _time_alternating(graphs, replays)
    res = {"shape": {"B": B, "T": T, "na": na, "nh": nh, "mode": "AUGRU"},
           "lengths": {"mean": float(lengths.float().mean()), "max": int(lengths.max()), "zero": int((lengths == 0).sum())},
           "fused_vs_composed_max_rel_diff": agree}
    for i, n in enumerate(names):
        res[f"{n}_ms"], res[f"{n}_min_ms"] = med[i], mins[i]
    res.update({"fused_fwd_bwd_ms": med[4], "fused_fwd_bwd_min_ms": mins[4], "fused_fwd_ms": med[5], "fused_fwd_min_ms": mins[5],
                "composed_fwd_bwd_ms": med[6], "composed_fwd_bwd_min_ms": mins[6], "composed_fwd_ms": med[7],
                "composed_fwd_bwd_eager_host_clock_ms": eager_ms,
                "speedup_fwd_bwd": med[6] / med[4], "speedup_fwd": med[7] / med[5],
                "fused_launches_fwd_bwd": 6, "composed": "per step: cat, matmul, sigmoid, cat, matmul, tanh, blend, where x 2; "
                "einsum scores, where, softmax; autograd (torch, fp32), captured as one hipGraph"})
    return res


def make_estimator(dev, B, T=50):
    """The mirrored dien_model_fn over synthetic device-resident features: 7 profile fields + the target feed + a history of T
    feeds sharing one 16-wide table; AUGRU, dice, hidden 512,256,128, BatchNorm, dropout 0.1, LazyAdam, sequence_max_length T."""
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm.DIEN.dien import dien_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=8, max_vocab=100000, with_history=True, history_len=T)
    cmap = {n: fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)}
    his = fc.categorical_column_with_identity("his_read_comment_7d_seq", cmap["feedid"].num_buckets)
    his.is_sequence = True
    feed = cmap.pop("feedid")
    feed.is_sequence = True
    shared = fc.shared_embedding_columns([feed, his, his], 16, combiner="mean")
    params = {"dense_feature_columns": [], "category_feature_columns": [fc.embedding_column(c, 16) for c in cmap.values()],
              "target_feedid_feature_columns": [shared[0]], "sequence_feature_columns": [shared[1]],
              "negative_sequence_feature_columns": [shared[2]], "hidden_units": ["512", "256", "128"], "dropout_rate": 0.1,
              "batch_norm": True, "learning_rate": 0.005, "activation": "dice", "use_auxiliary_loss": False,
              "negative_sample_number": 3, "custom_gru_type": "AUGRU", "gru_output_units": 8, "sequence_max_length": T}
    est = Estimator(dien_model_fn, params, RunConfig(device=dev, seed=5))
    feats, labels, _ = synth.device_features(spec, B, dev)
    est.build(feats, labels)
    return est, feats, labels


def bench_step(dev, B, steps):
    """The full captured training step (GraphedTrainStep): ms, examples/s, and the kernel launches of one eager step."""
    import statistics
    from recalgorithm_amd.estimator import GraphedTrainStep
    from scripts.bench_ple import count_launches
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
    est2, feats2, labels2 = make_estimator(dev, B)
    n_launch, by_name = count_launches(est2, feats2, labels2)
    return {"batch": B, "step_ms": ms, "examples_per_s": B / (ms * 1e-3), "step_ms_min": min(windows) * 1e3, "loss": float(g()),
            "kernel_launches_per_eager_step": n_launch, "most_launched": by_name,
            "config": "AUGRU, nh = 8, static T = 50 (every history 50 long); dice; hidden 512,256,128; BN; dropout 0.1; LazyAdam; "
                      "7 profile fields + target feed + history x emb16"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dien.py measures on a HIP device; none found")
    from recalgorithm_amd.io import synth
    dev = torch.device("cuda", 0)
    T, na, nh = 50, 16, 8
    zipf = torch.from_numpy(synth.zipf_ids(np.random.default_rng(1), a.batch, T + 1).astype(np.int64)).clamp(0, T)
    res = {"bench": "dien", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "zipf": bench_module(dev, a.batch, T, na, nh, zipf, a.replays),
           "full": bench_module(dev, a.batch, T, na, nh, torch.full((a.batch,), T, dtype=torch.int64), a.replays),
           "step": bench_step(dev, a.batch, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
