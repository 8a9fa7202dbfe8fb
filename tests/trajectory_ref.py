"""The oracle's N-step training trajectory on rotating sub-batches of the golden batch (CPU, torch only), and the bound
an fp32 implementation of the same N steps is held to.

One step = getattr(oracle.ref_models, <model>)(P, feats, labels, params, training=True, ...) -> loss.backward() ->
oracle.ref_ops.adam_tf1_step on every variable that got a gradient, step numbers 1..N.  The start is the golden's
variables ROUNDED TO float32 (what a device holds: the float64 and the float32 run and the kernels then start from the
same numbers), with DIN's activation alphas moved off 1 (alpha = 1 makes Dice / PReLU the identity: every dense -> BN pair
is then affine and the gradients of the biases and BN shifts in front of a BatchNorm cancel analytically — noise that Adam
turns into O(lr) moves; tests/test_gpu_models.py::test_fused_train_step_matches_unfused_graph moves them the same way).

Batches: three sorted subsets of 32 of the 48 golden examples, used 0, 1, 2, 0, 1, 2 — ids leave the batch and come back,
so table rows lag behind the step counter and are caught up.  Training-mode dropout (the *_dropout goldens, NFM's
hard-coded one) takes one seeded keep mask per dropout call and step.

Bound (per element of a variable p, float64 oracle quantities only; tests/util.py::assert_adam_update pushed through N steps):
    tol      = tight + sum_k lr_t(k) * tol_g(k) / (sqrt(v64_k) + eps)
    tight    = N * (1e-5 * lr + 6e-8 * |p64|)                           p64: the float64 variable after step N
    tol_g(k) = 1e-5 * (|g64_k| + rms(g64_k)) + 1e-6 * max|g64_k|       the gradient tolerance the one-step tests accept
    lr_t(k)  = lr * sqrt(1 - b2^k) / (1 - b1^k)                         constants rounded to float32 as in adam_tf1_step
"""
import math

import torch

from oracle import ref_models as M
from oracle import ref_ops as R
from tests import golden_util as GU

N_STEPS = 6
BATCH = 32
ORDER = (0, 1, 2, 0, 1, 2)
BN_MOMENTUM = 0.99
# Seed of the keep masks.  Not every draw is a fair input: under seed 7 one element of FiBiNET's bgm_song_id table meets
# |g| ~ eps / sqrt(1 - b2) at step 1 (an ill-conditioned Adam move, 6e-5 wide, inside the bound's second term), which shifts the
# step-2 forward of every example with that id; the float32 oracle then leaves 6 .. 251 elements of dnn_part/dense/kernel outside
# `tight` depending only on the ORDER of the examples.  tests/test_trajectory_host.py holds the inputs to the condition that a
# reordered float32 run passes the guards the kernels face; 8 is the first seed that meets it on every model.
MASK_SEED = 8
# BatchNorm moving means that follow an ill-conditioned bias (model -> {moving_mean: the bias in front of it}).  A unit of
# `fcn/dense` whose pre-activation keeps one sign over every batch passes PReLU as an affine map: in front of the training-mode
# BatchNorm its bias then has an analytically zero gradient, fp32 leaves rounding noise there, and Adam's g / (sqrt(v) + eps)
# turns noise into O(lr) moves (the bound's second term is large exactly on those elements).  The loss never sees such a
# bias — the BatchNorm subtracts it — but the batch MEAN the moving average accumulates does, with slope <= 1 (PReLU with
# alpha in [0.25, 0.75] is 1-Lipschitz).  The float32 oracle alone misses assert_close(reduced=True, floor=1e-7) there by 36 x
# (tests/test_trajectory_host.py measures it), so these tensors get, per channel, the bias's own bound pushed through the
# moving average: (1 - 0.99^N) * tol[bias].  Channels with a well-conditioned bias keep the plain tolerance (tol ~ tight).
MOVING_FOLLOWS_BIAS = {"model_din_prelu_softmax": {"fcn/batch_normalization/moving_mean": "fcn/dense/bias"}}


def batch_indices():
    """Three sorted 32-of-48 subsets, drawn one after the other from one generator (seed 3)."""
    g = torch.Generator().manual_seed(3)
    return [torch.randperm(48, generator=g)[:BATCH].sort().values for _ in range(3)]


def cut(sfeats, labels, idx):
    """The examples `idx` of a string batch: lists of lists (string / ragged features) and [B, 1] tensors, per example."""
    out = {}
    for k, v in sfeats.items():
        out[k] = v[idx].clone() if isinstance(v, torch.Tensor) else [v[int(i)] for i in idx]
    return out, labels[idx].clone()


class Setup:
    """Everything the host test and the GPU test share for one golden model (built once per model and process)."""

    def __init__(self, name, vocab_dir):
        self.name = name
        self.model_fn, self.params, self.oracle_name = GU.mirror_setup(name, vocab_dir)
        d = GU.load(name)
        self.lr = float(d["meta/learning_rate"])
        sfeats, labels = GU.string_batch()
        self.batches = [cut(sfeats, labels, idx) for idx in batch_indices()]      # (string features, labels [32, 1] float64)
        gv = GU.golden_to_oracle_vars(name, GU.section(d, "var/"), self.params)
        self.start = {k: torch.from_numpy(v.copy()).float().double() for k, v in gv.items()}
        g = torch.Generator().manual_seed(99)
        for k in sorted(self.start):
            if "alpha" in k:
                self.start[k] = (0.25 + 0.5 * torch.rand(self.start[k].shape, generator=g)).float().double()
        # keep masks: as many per step as the golden's TRAIN run drew, same widths, BATCH rows; NFM's first call has the
        # hard-coded rate 0.1, every other call the model's dropout_rate
        widths = [int(m.shape[1]) for m in GU.dropout_masks(d)]
        rates = [float(self.params.get("dropout_rate") or 0.0)] * len(widths)
        if self.oracle_name == "nfm" and widths:
            rates[0] = 0.1
        g = torch.Generator().manual_seed(MASK_SEED)
        self.masks = [[(torch.rand(BATCH, w, generator=g) >= r).double() for w, r in zip(widths, rates)] for _ in ORDER]
        self._runs = {}

    def encoded(self, b, dtype):
        from tests.test_oracle_golden import _encode
        sf, labels = self.batches[b]
        feats = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
                 for k, v in _encode(self.params, sf).items()}
        return feats, {"read_comment": labels.to(dtype)}

    def run(self, dtype):
        if dtype not in self._runs:
            self._runs[dtype] = run_oracle(self, dtype)
        return self._runs[dtype]

    def run_reordered(self, seed):
        """The float32 run with the examples of every batch permuted (features, labels and keep-mask rows alike): the same
        computation to the last term, summed in another order — a second sample of what fp32 rounding does to these inputs."""
        g = torch.Generator().manual_seed(seed)
        perms = [torch.randperm(BATCH, generator=g) for _ in self.batches]
        other = Setup.__new__(Setup)
        other.__dict__.update(self.__dict__)
        other.batches = [({k: (v[p].clone() if isinstance(v, torch.Tensor) else [v[int(i)] for i in p]) for k, v in sf.items()}, lb[p].clone())
                         for (sf, lb), p in zip(self.batches, perms)]
        other.masks = [[m[perms[b]] for m in step] for step, b in zip(self.masks, ORDER)]
        return run_oracle(other, torch.float32)


def run_oracle(s: Setup, dtype, mutate=None):
    """`mutate` (tests/test_trajectory_host.py: the bound must notice them): "stale_step" takes lr_t of the step before from
    step 2 on; "lazy_rows" leaves table rows without a gradient in a step untouched (LazyAdam instead of dense semantics).
    -> {"loss": [N], "grad": [N x {name: g}], "m": [...], "v": [...], "vars": [...] (after the step), "moving": [N x {name: value}],
    "final": {name: p}}.
    Gradients, moments and variables of a step are clones: nothing returned aliases the running state."""
    fn = getattr(M, s.oracle_name)
    P = {k: v.clone().to(dtype) for k, v in s.start.items()}
    m = {k: torch.zeros_like(v) for k, v in P.items()}
    v_ = {k: torch.zeros_like(v) for k, v in P.items()}
    enc = {b: s.encoded(b, dtype) for b in set(ORDER)}
    out = {"loss": [], "grad": [], "m": [], "v": [], "moving": [], "vars": []}
    import inspect
    has_bn = "bn_state" in inspect.signature(fn).parameters
    has_masks = "dropout_masks" in inspect.signature(fn).parameters
    for k, b in enumerate(ORDER, start=1):
        for p in P.values():
            p.grad = None
            p.requires_grad_(p.is_floating_point())
        feats, labels = enc[b]
        kw, bn = {}, {}
        if has_bn:
            kw["bn_state"] = bn
        if has_masks and s.masks[k - 1]:
            kw["dropout_masks"] = [x.to(dtype) for x in s.masks[k - 1]]
        res = fn(P, feats, labels, s.params, training=True, **kw)
        res["loss"].backward()
        out["loss"].append(res["loss"].detach().clone())
        grads = {n: p.grad.detach().clone() for n, p in P.items() if p.grad is not None}
        with torch.no_grad():
            for n, g in grads.items():
                if mutate == "lazy_rows" and n.endswith("embedding_weights"):
                    rows = g.reshape(g.shape[0], -1).abs().sum(1) > 0
                    p_, m_, vv = P[n][rows], m[n][rows], v_[n][rows]
                    R.adam_tf1_step(p_, g[rows], m_, vv, k, s.lr)
                    P[n][rows], m[n][rows], v_[n][rows] = p_, m_, vv
                    continue
                R.adam_tf1_step(P[n], g, m[n], v_[n], max(k - 1, 1) if mutate == "stale_step" else k, s.lr)
            for scope, (mean, var) in bn.items():        # assign_moving_average, decay 0.99
                P[f"{scope}/moving_mean"].mul_(BN_MOMENTUM).add_(mean, alpha=1 - BN_MOMENTUM)
                P[f"{scope}/moving_variance"].mul_(BN_MOMENTUM).add_(var, alpha=1 - BN_MOMENTUM)
        out["grad"].append(grads)
        out["m"].append({n: m[n].clone() for n in grads})
        out["v"].append({n: v_[n].clone() for n in grads})
        out["vars"].append({n: P[n].detach().clone() for n in grads})
        out["moving"].append({n: p.detach().clone() for n, p in P.items() if "/moving_" in n and "dice_bn" not in n})
    out["final"] = {n: p.detach().clone() for n, p in P.items()}
    out["trainable"] = sorted({n for g in out["grad"] for n in g})
    return out


def lr_t(lr, k, beta1=0.9, beta2=0.999):
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    lr, beta1, beta2 = f32(lr), f32(beta1), f32(beta2)
    return lr * math.sqrt(1.0 - beta2 ** k) / (1.0 - beta1 ** k)


def bounds(ref64, lr):
    """name -> (tol, tight) for every variable of the float64 run (module docstring)."""
    eps = float(torch.tensor(1e-8, dtype=torch.float32))
    n = len(ref64["grad"])
    out = {}
    for name, p in ref64["final"].items():
        if not p.is_floating_point():
            continue
        tight = n * (1e-5 * lr + 6e-8 * p.double().abs())
        tol = tight.clone()
        for k in range(1, n + 1):
            g = ref64["grad"][k - 1].get(name)
            if g is None:
                continue
            g = g.double().abs()
            tol_g = 1e-5 * (g + g.pow(2).mean().sqrt()) + 1e-6 * g.max()
            tol = tol + lr_t(lr, k) * tol_g / (ref64["v"][k - 1][name].double().sqrt() + eps)
        out[name] = (tol, tight)
    return out


def excluded(s: Setup, ref64):
    """The tensors no free-running comparison can hold (the capped set): attention_part/f3_att/bias under softmax (shift
    invariance: its gradient sum_t ds_t is exactly 0), and a bias / beta whose float64 gradient is at most 1e-12 x the largest
    gradient of its sibling kernel / gamma at EVERY step (an analytic zero: what an fp32 run has there is rounding noise, which
    Adam's g / (sqrt(v) + eps) turns into O(lr) moves)."""
    out = set()
    if s.params.get("use_softmax") and "attention_part/f3_att/bias" in ref64["final"]:
        out.add("attention_part/f3_att/bias")
    for name in ref64["trainable"]:
        sib = name[:-5] + "/kernel" if name.endswith("/bias") else name[:-5] + "/gamma" if name.endswith("/beta") else None
        if sib is None or not all(name in g and sib in g for g in ref64["grad"]):
            continue
        if all(float(g[name].abs().max()) <= 1e-12 * float(g[sib].abs().max()) for g in ref64["grad"]):
            out.add(name)
    return sorted(out)


def worst_ratio(values, ref64, bnd, skip=()):
    """-> (worst |p - p64| / tol, its tensor, {name: elements outside tight}) over the trainable variables not in `skip`."""
    worst, where, outside = 0.0, "", {}
    for name in ref64["trainable"]:
        if name in skip or name not in values:
            continue
        tol, tight = bnd[name]
        err = (values[name].detach().double().cpu().reshape(tol.shape) - ref64["final"][name].double()).abs()
        r = float((err / tol).max()) if err.numel() else 0.0
        outside[name] = int((err > tight).sum())
        if r > worst:
            worst, where = r, name
    return worst, where, outside


def moving_ratio(a, ref, extra=0.0):
    """worst |a - ref| / tol under tests/util.py::assert_close(reduced=True, floor=1e-7) (+ a per-element `extra`)."""
    ref = ref.double().reshape(-1)
    tol = 1e-5 * (ref.abs() + ref.pow(2).mean().sqrt()) + 1e-6 * ref.abs().max() + 1e-7 + extra
    return float(((a.detach().double().cpu().reshape(-1) - ref).abs() / tol).max())


def moving_extra(name, bnd):
    """moving tensor -> the per-channel allowance of MOVING_FOLLOWS_BIAS."""
    return {mv: (1.0 - BN_MOMENTUM ** N_STEPS) * bnd[bias][0].reshape(-1)
            for mv, bias in MOVING_FOLLOWS_BIAS.get(name, {}).items()}
