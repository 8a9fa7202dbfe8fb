"""BST measurements on the MI355X (bench.py is the project's yardstick and has no BST entry): each of the four kernels of the
transformer block alone, the same block composed from torch ops on the same device, and the full captured training step.
Self-contained: synthetic inputs from seeds, nothing read from outside the tree.  Prints one JSON line (and writes it with
--out).

    python scripts/bench_bst.py [--batch 4096] [--replays 200] [--steps 200] [--out profiles/bst_bench.json]

kernels:  recalgo_bst_attn_fwd / attn_bwd / ffn_fwd / ffn_bwd at the C ABI (B = 4096, T = 51, d = 16, H = 3, sum pooling;
          keys_length uniform in 1..51), one captured launch each (the backward entries: their kernel + the column sum).
block:    forward + backward of one block through ops.bst_attention / ops.bst_ffn (four launches + two column sums) against
          the block composed from torch ops — einsum projections, softmax over [B, H, T, T], matmuls, layer norm as
          moments + elementwise, autograd — on the same inputs.  The composed path writes the 128 MB [B, H, T, T] tensor
          several times; the fused one never forms it.  The graphs alternate in one process; medians over the replays.
step:     the mirrored bst_model_fn (1 block, 3 heads, sum pooling, hidden 512,256,128, BatchNorm, dropout 0.1, 7 profile
          fields + the target feed + a full 50-long history, --static_sequence_length) at B = 4096, captured
          (GraphedTrainStep), examples/s.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_ple import _graph, _time_alternating  # noqa: E402

MASK_ADD = -4294967296.0


def make_inputs(B, T, d, H, dev, seed=1):
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return ((torch.rand(*shape, generator=gen) * 2 - 1) * scale).to(dev)
    kl = torch.randint(1, T + 1, (B,), generator=gen, dtype=torch.int32)
    x = rnd(B, T, d) * (torch.arange(T)[None, :, None] < kl[:, None, None]).to(dev)
    lim = math.sqrt(6.0 / (2 * d))
    return {"x": x.contiguous(), "keys_length": kl.to(dev), "pos": rnd(T, d, scale=0.3),
            "w_q": rnd(H, d, d, scale=lim), "w_k": rnd(H, d, d, scale=lim), "w_v": rnd(H, d, d, scale=lim),
            "w_o": rnd(H * d, d, scale=math.sqrt(6.0 / (H * d + d))), "gamma": 1 + rnd(d, scale=0.2), "beta": rnd(d, scale=0.2),
            "ffn_w": rnd(d, d, scale=lim), "ffn_b": rnd(d, scale=0.1), "gamma2": 1 + rnd(d, scale=0.2), "beta2": rnd(d, scale=0.2),
            "g_n1": rnd(B, T, d), "g_pool": rnd(B, d)}


ATTN = ("pos", "w_q", "w_k", "w_v", "w_o", "gamma", "beta")
FFN = ("ffn_w", "ffn_b", "gamma2", "beta2")


def composed_block(c, x, params):
    """one block + sum pooling from torch ops (tests/bst_ref.py's arithmetic in float32: the literal mask add)"""
    pos, w_q, w_k, w_v, w_o, gamma, beta, ffn_w, ffn_b, gamma2, beta2 = params
    B, T, d = x.shape
    H = w_q.shape[0]

    def layer_norm(v, g, b):
        mean = v.mean(dim=(1, 2), keepdim=True)
        var = ((v - mean) ** 2).mean(dim=(1, 2), keepdim=True)
        inv = torch.rsqrt(var + 1e-12) * g
        return v * inv + (b - mean * inv)
    xp = x + pos[:T]
    q = torch.einsum("bik,hkj->bhij", xp, w_q)
    k = torch.einsum("bik,hkj->bhij", xp, w_k)
    v = torch.einsum("bik,hkj->bhij", x, w_v)
    s = q @ k.transpose(-1, -2) / math.sqrt(d) + c["mask"]
    heads = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, T, H * d)
    n1 = layer_norm(heads @ w_o + xp, gamma, beta)
    h = n1 @ ffn_w + ffn_b
    out = layer_norm(0.505 * h + 0.495 * h.abs() + n1, gamma2, beta2)
    return out.sum(dim=1)


def bench_block(dev, B, T, d, H, replays):
    from recalgorithm_amd import _lib, ops
    c = make_inputs(B, T, d, H, dev)
    lib = _lib.load()
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    n1, out, pool = torch.empty(B, T, d, device=dev), torch.empty(B, T, d, device=dev), torch.empty(B, d, device=dev)
    dx, dn1, dpos = torch.empty(B, T, d, device=dev), torch.empty(B, T, d, device=dev), torch.empty(T, d, device=dev)
    ga = [torch.empty_like(c[k]) for k in ATTN[1:]]
    gf = [torch.empty_like(c[k]) for k in FFN]
    ws_a = torch.empty(int(lib.recalgo_bst_attn_bwd_workspace_bytes(B, T, d, H)), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(int(lib.recalgo_bst_ffn_bwd_workspace_bytes(B, d)), dtype=torch.uint8, device=dev)

    def attn_fwd():
        lib.recalgo_bst_attn_fwd(P(c["x"]), P(c["pos"]), P(c["keys_length"]), *[P(c[k]) for k in ATTN[1:]], B, T, d, H, P(n1), None, st())

    def attn_bwd():
        lib.recalgo_bst_attn_bwd(P(c["x"]), P(c["pos"]), P(c["keys_length"]), *[P(c[k]) for k in ATTN[1:6]], P(c["g_n1"]), B, T, d, H,
                                 P(dx), P(dpos), *[P(t) for t in ga], P(ws_a), st())

    def ffn_fwd():
        lib.recalgo_bst_ffn_fwd(P(n1), *[P(c[k]) for k in FFN], B, T, d, 0, P(out), P(pool), None, st())

    def ffn_bwd():
        lib.recalgo_bst_ffn_bwd(P(n1), *[P(c[k]) for k in FFN[:3]], None, P(c["g_pool"]), B, T, d, 0, P(dn1), *[P(t) for t in gf],
                                P(ws_f), st())
    attn_fwd()
    names = ["attn_fwd", "attn_bwd", "ffn_fwd", "ffn_bwd"]
    graphs = [_graph(f)[0] for f in (attn_fwd, attn_bwd, ffn_fwd, ffn_bwd)]

    leaves = {k: c[k].clone().requires_grad_(True) for k in ("x",) + ATTN + FFN}

    def fused():
        for t in leaves.values():
            t.grad = None
        n = ops.bst_attention(leaves["x"], c["keys_length"], *[leaves[k] for k in ATTN])
        _, pl = ops.bst_ffn(n, *[leaves[k] for k in FFN], pool="sum", want_out=False)
        pl.backward(c["g_pool"])
        return pl
    c["mask"] = ((torch.arange(T, device=dev)[None, :] >= c["keys_length"][:, None]).float() * MASK_ADD)[:, None, :, None]

    def composed():
        for t in leaves.values():
            t.grad = None
        pl = composed_block(c, leaves["x"], [leaves[k] for k in ATTN + FFN])
        pl.backward(c["g_pool"])
        return pl

    def composed_forward():
        with torch.no_grad():
            return composed_block(c, leaves["x"], [leaves[k] for k in ATTN + FFN])
    a, b = fused().detach().clone(), composed().detach().clone()
    agree = float((a - b).abs().max() / b.abs().max())
    graphs += [_graph(f)[0] for f in (fused, composed, composed_forward)]
    med, mins = _time_alternating(graphs, replays)
    res = {"shape": {"B": B, "T": T, "d": d, "H": H}, "fused_vs_composed_max_rel_diff": agree}
    for i, n in enumerate(names):
        res[f"{n}_ms"], res[f"{n}_min_ms"] = med[i], mins[i]
    res.update({"fused_fwd_ms": med[0] + med[2], "fused_block_fwd_bwd_ms": med[4], "fused_block_fwd_bwd_min_ms": mins[4],
                "composed_block_fwd_bwd_ms": med[5], "composed_block_fwd_bwd_min_ms": mins[5], "composed_fwd_ms": med[6],
                "speedup_fwd_bwd": med[5] / med[4], "speedup_fwd": med[6] / (med[0] + med[2]),
                "composed": "einsum projections, softmax over [B, H, T, T], matmuls, layer norm from moments, autograd (torch, fp32)"})
    return res


def make_estimator(dev, B, blocks=1, heads=3, pooling="sum"):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm.BST.bst import bst_model_fn
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=8, max_vocab=100000, with_history=True, history_len=50)
    cmap = {n: fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)}
    his = fc.categorical_column_with_identity("his_read_comment_7d_seq", cmap["feedid"].num_buckets)
    his.is_sequence = True
    feed = cmap.pop("feedid")
    feed.is_sequence = True
    shared = fc.shared_embedding_columns([feed, his], 16, combiner="mean")
    params = {"dense_feature_columns": [], "category_feature_columns": [fc.embedding_column(c, 16) for c in cmap.values()],
              "target_feedid_feature_columns": [shared[0]], "sequence_feature_columns": [shared[1]],
              "hidden_units": ["512", "256", "128"], "dropout_rate": 0.1, "batch_norm": True, "learning_rate": 0.005,
              "sequence_max_length": 50, "num_transformer_block": blocks, "num_transformer_heads": heads,
              "pooling_method": pooling, "static_sequence_length": True}
    est = Estimator(bst_model_fn, params, RunConfig(device=dev, seed=5))
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
    windows = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(steps // 5):
            g()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / (steps // 5))
    ms = statistics.median(windows) * 1e3
    return {"batch": B, "step_ms": ms, "examples_per_s": B / (ms * 1e-3), "step_ms_min": min(windows) * 1e3, "loss": float(g()),
            "config": "1 block, 3 heads, sum pooling, T = 51 (static); hidden 512,256,128; BN; dropout 0.1; 7 profile fields + "
                      "target feed + 50-long history x emb16"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bst.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "bst", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "block": bench_block(dev, a.batch, 51, 16, 3, a.replays), "step": bench_step(dev, a.batch, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
