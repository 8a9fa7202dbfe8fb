"""-m gpu: MMoE on the MI355X — ops.gate_mix (csrc/mmoe.hip) against float64, the multi-task loss, the mirrored model_fn
against the two reference-generated goldens and against tests/mmoe_ref.py at the reference's default configuration, the
captured Estimator run, the abandoned-step contract, export + serving, and the script's main().
Tolerance: the project's standing 1e-5 bound and strict guard (tests/util.py assert_close with ref32=)."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import ref_ops as R
from recalgorithm_amd import feature_column as fc
from recalgorithm_amd.estimator import Estimator, GraphedTrainStep, ModeKeys, RunConfig
from recalgorithm_amd.io import synth
from tests import mmoe_ref
from tests.golden_protocol import check_on_device, judge_step_against_oracle
from tests.test_mmoe_host import CASE, GOLDENS, TASKS
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ple_selection():
    """a CGC-style table over 8 experts (extraction_network.py): experts 0-1 shared, each of three tasks owns two; every task
    gate mixes its own two + the two shared, one `all` gate mixes everything (five more gates reuse the task tables)"""
    own = {0: [2, 3], 1: [4, 5], 2: [6, 7]}
    sel = [own[g % 3] + [0, 1] for g in range(7)]
    return sel + [list(range(8))]


def _inputs(B, In, E, G, H, selection, seed, scale=1.0, relu=False):
    gen = torch.Generator().manual_seed(seed)
    selection = [list(range(E)) for _ in range(G)] if selection is None else selection
    x = torch.randn(B, In, generator=gen, dtype=torch.float64)
    ws = [torch.randn(In, len(s), generator=gen, dtype=torch.float64) * (scale / In ** 0.5) for s in selection]
    ex = [torch.randn(B, H, generator=gen, dtype=torch.float64) for _ in range(E)]
    if relu:
        ex = [torch.relu(t) for t in ex]
    gs = [torch.randn(B, H, generator=gen, dtype=torch.float64) for _ in range(G)]
    return x, ws, ex, gs, selection


def _reference(x, ws, ex, gs, selection, dtype, relu=False):
    """-> (outs, gates, dx, dws, dexs) of tests/mmoe_ref.gate_mix in `dtype` (gs[g] None: that gate gets no gradient; relu:
    the experts are ReLU outputs and d_expert is the gradient at the pre-activation)"""
    x = x.detach().clone().to(dtype).requires_grad_(True)
    ws = [w.detach().clone().to(dtype).requires_grad_(True) for w in ws]
    pre = [t.detach().clone().to(dtype).requires_grad_(True) for t in ex]
    outs, ps = mmoe_ref.gate_mix(x, ws, [torch.relu(t) for t in pre] if relu else pre, selection)
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gs) if g is not None)
    grads = torch.autograd.grad(loss, [x, *ws, *pre], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [x, *ws, *pre])]
    G = len(ws)
    return [o.detach() for o in outs], torch.cat(ps, dim=1).detach(), grads[0], grads[1:1 + G], grads[1 + G:]


def _unaligned(t, dev):
    """the tensor on the device at a base address that is 4- but not 16-byte aligned"""
    buf = torch.empty(t.numel() + 8, device=dev, dtype=torch.float32)
    off = 1 + (-(buf.data_ptr() // 4) % 4)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _run_hip(dev, x, ws, ex, gs, selection, relu=False, unaligned=False, strided_grad=False, unaligned_grad=False):
    from recalgorithm_amd import nn, ops
    xd = x.float().to(dev).requires_grad_(True)
    wd = [w.float().to(dev).requires_grad_(True) for w in ws]
    if unaligned:
        ed = [_unaligned(t.float(), dev).requires_grad_(True) for t in ex]
    else:
        ed = [t.float().to(dev).requires_grad_(True) for t in ex]
    if relu:
        for t in ed:
            t._recalgo_relu_src = nn.ReluSource()
    outs, p = ops.gate_mix(xd, wd, ed, selection, return_gates=True)
    upstream = []
    for g in gs:
        if g is None:
            continue
        gd = _unaligned(g.float(), dev) if unaligned_grad else g.float().to(dev)
        if strided_grad:                     # a non-contiguous upstream gradient: every other column of a twice as wide tensor
            wide = torch.zeros(g.shape[0], 2 * g.shape[1], device=dev)
            wide[:, ::2] = gd
            gd = wide[:, ::2]
            assert not gd.is_contiguous()
        upstream.append(gd)
    torch.autograd.backward([o for o, g in zip(outs, gs) if g is not None], upstream)
    return outs, p, xd.grad, [w.grad for w in wd], [t.grad for t in ed]


def _check(dev, shape, seed, what, **kw):
    B, In, E, G, H, selection = shape
    drop_gate = kw.pop("drop_gate", None)
    scale = kw.pop("scale", 1.0)
    relu = kw.get("relu", False)
    x, ws, ex, gs, selection = _inputs(B, In, E, G, H, selection, seed, scale=scale, relu=relu)
    if relu:
        # ReLU outputs given as the experts: the reference differentiates at the pre-activation, where relu(t) == t > 0
        ex = [t.clamp(min=0) for t in ex]
    if drop_gate is not None:
        gs[drop_gate] = None
    r64 = _reference(x, ws, ex, gs, selection, torch.float64, relu=relu)
    r32 = _reference(x, ws, ex, gs, selection, torch.float32, relu=relu)
    outs, p, dx, dws, dexs = _run_hip(dev, x, ws, ex, gs, selection, **kw)
    assert_close(p, r64[1], what=f"{what} gates", ref32=r32[1])
    assert float((p.sum(dim=1) - len(selection)).abs().max()) < 1e-5 * len(selection)
    for g, o in enumerate(outs):
        assert_close(o, r64[0][g], what=f"{what} out{g}", ref32=r32[0][g])
    assert_close(dx, r64[2], what=f"{what} dx", ref32=r32[2])
    for g, dw in enumerate(dws):
        if dw is None:
            assert gs[g] is None or float(r64[3][g].abs().max()) == 0.0
            continue
        assert_close(dw, r64[3][g], what=f"{what} dW{g}", reduced=True, ref32=r32[3][g])       # (a sum over the batch)
    for e, de in enumerate(dexs):
        assert_close(de, r64[4][e], what=f"{what} d_expert{e}", ref32=r32[4][e])
    return outs, p, dx, dws, dexs


SHAPES = {"default": (4096, 82, 3, 3, 512, None), "tiny": (37, 5, 1, 1, 4, None), "ple": (1000, 82, 8, 8, 128, ple_selection()),
          "sixteen": (130, 20, 16, 10, 8, None)}


@pytest.mark.parametrize("case", list(SHAPES))
def test_gate_mix_against_float64(dev, case):
    _check(dev, SHAPES[case], 11, case)


def test_gate_mix_relu_experts_get_a_masked_gradient(dev):
    _check(dev, (500, 82, 3, 3, 64, None), 12, "relu experts", relu=True)


@pytest.mark.parametrize("arm", ["unaligned", "unaligned_grad", "strided_grad", "null_grad"])
def test_gate_mix_other_arms(dev, arm):
    """unaligned: expert base pointers off 16-byte alignment select the scalar-access arm of both kernels; unaligned_grad:
    aligned experts, but contiguous upstream gradients off 16-byte alignment — the backward entry point's own detection
    (outputs and expert gradients are allocated by the op and always aligned);
    strided_grad: a non-contiguous upstream gradient is made contiguous by the host side; null_grad: a gate nobody
    differentiates reaches the kernel as a NULL pointer."""
    kw = {"unaligned": dict(unaligned=True), "unaligned_grad": dict(unaligned_grad=True), "strided_grad": dict(strided_grad=True), "null_grad": dict(drop_gate=1)}[arm]
    _check(dev, (777, 82, 3, 3, 128, None), 13, arm, **kw)
    if arm == "null_grad":
        _check(dev, SHAPES["ple"], 14, "ple null_grad", drop_gate=7)


def test_gate_mix_large_gate_logits(dev):
    """gate logits of magnitude ~80 (scaled gate kernels): the max-subtracted softmax stays finite and sums to 1"""
    shape = (600, 82, 4, 3, 64, None)
    x, ws, _, _, _ = _inputs(*shape, 15, scale=40.0)
    assert float((x @ ws[0]).abs().max()) > 80.0
    outs, p, *_ = _check(dev, shape, 15, "large logits", scale=40.0)
    assert torch.isfinite(p).all() and all(torch.isfinite(o).all() for o in outs)
    assert float((p.view(600, 3, 4).sum(dim=2) - 1).abs().max()) < 1e-5


def test_gate_mix_is_deterministic_and_capturable(dev):
    from recalgorithm_amd import ops
    x, ws, ex, gs, sel = _inputs(4096, 82, 3, 3, 512, None, 16)
    a = _run_hip(dev, x, ws, ex, gs, sel)
    b = _run_hip(dev, x, ws, ex, gs, sel)

    def flat(r):
        return [*r[0], r[1], r[2], *r[3], *r[4]]
    for i, (u, v) in enumerate(zip(flat(a), flat(b))):
        assert_bit_exact(u, v, f"second run, tensor {i}")
    # hipGraph: forward + backward captured once, replayed three times on the same inputs
    xd = x.float().to(dev).requires_grad_(True)
    wd = [w.float().to(dev).requires_grad_(True) for w in ws]
    ed = [t.float().to(dev).requires_grad_(True) for t in ex]
    gd = [g.float().to(dev) for g in gs]

    def step():
        outs, p = ops.gate_mix(xd, wd, ed, sel, return_gates=True)
        grads = torch.autograd.grad(outs, [xd, *wd, *ed], gd)
        return [*outs, p, *grads]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    eager = [*a[0], a[1], a[2], *a[3], *a[4]]
    for i, (u, v) in enumerate(zip(captured, eager)):
        assert_bit_exact(u, v, f"graph replay, tensor {i}")


def test_gate_mix_limits(dev):
    from recalgorithm_amd import _lib, ops
    x = torch.zeros(8, 82, device=dev)
    with pytest.raises(NotImplementedError):
        ops.gate_mix(x, [torch.zeros(82, 3, device=dev)], [torch.zeros(8, 6, device=dev) for _ in range(3)])      # H % 4
    with pytest.raises(ValueError):
        ops.gate_mix(x, [torch.zeros(82, 0, device=dev)], [torch.zeros(8, 8, device=dev) for _ in range(3)], [[]])  # empty gate
    with pytest.raises(NotImplementedError):
        ops.gate_mix(x, [torch.zeros(82, 17, device=dev)], [torch.zeros(8, 8, device=dev) for _ in range(17)])    # E > 16
    with pytest.raises(NotImplementedError):
        ops.gate_mix(torch.zeros(8, 400, device=dev), [torch.zeros(400, 12, device=dev)],
                     [torch.zeros(8, 8, device=dev) for _ in range(12)])                                           # LDS budget
    # the entry point checks again: an error code (raised by the binding), never a launch
    lib = _lib.load()
    import ctypes
    n_sel, sel = (ctypes.c_int * 1)(3), (ctypes.c_int * 3)(0, 1, 2)
    e = [torch.zeros(8, 6, device=dev) for _ in range(3)]
    w, o, p = torch.zeros(82, 3, device=dev), torch.zeros(8, 6, device=dev), torch.zeros(8, 3, device=dev)
    with pytest.raises(_lib.RecalgoError, match="recalgo_gate_mix_fwd failed with hipError_t=[1-9]"):
        lib.recalgo_gate_mix_fwd(ops._p(x), 82, ops._ptr_array([w]), n_sel, sel, ops._ptr_array(e), 8, 82, 3, 1, 6,
                                 ops._ptr_array([o]), ops._p(p), ops._stream(x))


@pytest.mark.parametrize("T,B", [(3, 4096), (1, 1000), (5, 37)])
def test_multitask_loss_against_float64(dev, T, B):
    from recalgorithm_amd import ops
    gen = torch.Generator().manual_seed(17 + T)
    lg = [torch.randn(B, 1, generator=gen, dtype=torch.float64) * 4 for _ in range(T)]
    lb = [(torch.rand(B, 1, generator=gen) < 0.3).double() for _ in range(T)]

    def ref(dtype):
        xs = [t.detach().clone().to(dtype).requires_grad_(True) for t in lg]
        losses = [R.ce_loss(y.to(dtype), v) for y, v in zip(lb, xs)]
        total = losses[0]
        for v in losses[1:]:
            total = total + v
        total.backward()
        return total.detach(), torch.stack(losses).detach(), torch.cat([torch.sigmoid(v) for v in xs], 1).detach(), [v.grad for v in xs]
    r64, r32 = ref(torch.float64), ref(torch.float32)
    xd = [t.float().to(dev).requires_grad_(True) for t in lg]
    yd = [t.float().to(dev) for t in lb]
    total, losses, prob = ops.multitask_sigmoid_cross_entropy(xd, yd)
    total.backward()
    assert_close(total, r64[0], what="total loss", ref32=r32[0])
    assert_close(losses, r64[1], what="task losses", ref32=r32[1])
    assert_close(prob, r64[2], what="probabilities", ref32=r32[2])
    for t in range(T):
        assert_close(xd[t].grad, r64[3][t], what=f"dlogit {t}", ref32=r32[3][t])
        # every task's loss is the single-task kernel's value bit for bit
        one, p1 = ops.sigmoid_cross_entropy(xd[t].detach(), yd[t])
        assert_bit_exact(losses[t], one, f"task {t} loss vs sigmoid_cross_entropy")
        assert_bit_exact(prob[:, t:t + 1].contiguous(), p1, f"task {t} probabilities vs sigmoid_cross_entropy")
    if T == 1:
        x1 = xd[0].detach().clone().requires_grad_(True)
        one, _ = ops.sigmoid_cross_entropy(x1, yd[0])
        one.backward()
        assert_bit_exact(total, one, "T = 1 total")
        assert_bit_exact(xd[0].grad, x1.grad, "T = 1 dlogit")
    with ops.loss_seed(0.5):                 # the seed baked into the gradients (Estimator.train_step under data parallelism)
        x2 = [t.detach().clone().requires_grad_(True) for t in xd]
        tot2, _, _ = ops.multitask_sigmoid_cross_entropy(x2, yd)
    tot2.backward(torch.full_like(tot2, 0.5))
    for t in range(T):
        assert_close(x2[t].grad, 0.5 * r64[3][t], what=f"seeded dlogit {t}")


# ---- the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_model_golden(dev, name, tmp_path):
    check_on_device(dev, CASE, name, tmp_path)


DIMS = (16, 16, 16, 4, 4, 4, 4, 2)          # 66 embedding columns + 16 dense features = the reference's 82 inputs


def make(dev, B=4096, hidden=("512", "256", "128"), H=512, dropout_rate=0.1, batch_norm=True, seed=5, **run):
    from recalgorithm_amd.algorithm._common import dense_columns
    from recalgorithm_amd.algorithm.MMOE.mmoe import mmoe_model_fn
    spec = synth.SynthSpec(n_fields=8, max_vocab=400, seed=11, oov_frac=0.05, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": dense_columns(), "category_feature_columns": [fc.embedding_column(c, k) for c, k in zip(cats, DIMS)],
              "hidden_units": list(hidden), "dropout_rate": dropout_rate, "batch_norm": batch_norm, "learning_rate": 0.005,
              "num_experts": 3, "num_tasks": 3, "expert_hidden_units": H, "task_names": list(TASKS)}
    est = Estimator(mmoe_model_fn, params, RunConfig(device=dev, seed=seed, **run))
    batches = [synth.device_features(spec, B, dev, batch_index=i, extra_labels=TASKS[1:])[:2] for i in range(4)]
    est.build(*batches[0])
    return est, params, batches


def _oracle_inputs(est, feats, labels, dtype):
    P = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in est.store.named_arrays().items()}
    cf = {k: (v.cpu().to(dtype) if v.is_floating_point() else v.cpu()) for k, v in feats.items()}
    return P, cf, {k: v.cpu().to(dtype) for k, v in labels.items()}


def expert_pattern():
    """tests/test_gpu_baseline_shapes.py's _ReluPattern + the expert layers, which do not go through nn.dense"""
    from recalgorithm_amd import nn
    from tests.test_gpu_baseline_shapes import _ReluPattern

    class Pattern(_ReluPattern):
        def record_hip(self, call):
            real = nn.expert_layers

            def experts(*a, **k):
                ys = real(*a, **k)
                self.masks.extend((y.detach() > 0).cpu() for y in ys)
                return ys
            nn.expert_layers = experts
            try:
                return super().record_hip(call)
            finally:
                nn.expert_layers = real
    return Pattern()


def test_default_configuration_step_against_float64(dev):
    """B 4096, hidden_units 512,256,128, 3 experts of 512 units, 3 tasks, BatchNorm on, dropout 0.1 (the keep masks of the
    library's hash stream recorded and handed to both oracles).  Gradients are compared conditional on the HIP forward's ReLU
    pattern, as tests/test_gpu_baseline_shapes.py does (see its _ReluPattern)."""
    from recalgorithm_amd import nn, ops
    B = 4096
    est, params, batches = make(dev)
    feats, labels = batches[0]
    assert torch.cat([v for k, v in sorted(feats.items()) if v.is_floating_point()], 1).shape[1] == 16
    P, cf, cl = _oracle_inputs(est, feats, labels, torch.float64)
    P32, cf32, cl32 = _oracle_inputs(est, feats, labels, torch.float32)
    before = {k: v.detach().cpu().double().clone() for k, v in est.store.named_arrays().items()}
    pattern = expert_pattern()
    nn.DROPOUT_SPECS[:] = []
    spec = pattern.record_hip(lambda: est._call_model_fn(feats, labels, ModeKeys.TRAIN))
    dspecs = list(nn.DROPOUT_SPECS)
    assert len(dspecs) == 9 and all(d.mask is None for d in dspecs)
    masks = [ops.dropout_keep_mask((B, w), d, dev).cpu() for d, w in zip(dspecs, (512, 256, 128) * 3)]
    assert all(0.88 < float(m.mean()) < 0.92 for m in masks)
    assert len(pattern.masks) == 3 + 9
    for pm, km in zip(pattern.masks[3:], masks):         # dropout fused into the dense epilogue: the recorded outputs are the dropped tensors
        pattern.kept[id(pm)] = km
    ref = pattern.oracle(lambda: mmoe_ref.mmoe(P, cf, cl, params, training=True, dropout_masks=[m.clone() for m in masks]), check=True)
    ref["loss"].backward()
    r32 = pattern.oracle(lambda: mmoe_ref.mmoe(P32, cf32, cl32, params, training=True, dropout_masks=[m.clone() for m in masks]))
    r32["loss"].backward()
    for shape, n_flip, dist in pattern.flips:
        assert dist < 1e-4 and n_flip < 64, f"activation pattern differs beyond rounding at layer {shape}"
    assert_close(spec.loss, ref["loss"], what="mmoe loss", ref32=r32["loss"])
    for t in TASKS:
        assert_close(spec.predictions[f"{t}_probabilities"], ref["probs"][t], what=f"mmoe {t} prob", ref32=r32["probs"][t])
    judge_step_against_oracle(est, spec, P, P32, before, params["learning_rate"], "mmoe", 40)


def _state(est):
    est.store.sync()
    out = dict(est.store.named_arrays())
    out["__flat_m__"], out["__flat_v__"] = est.store.flat_m, est.store.flat_v
    for n, ar in est.store.arenas.items():
        if ar.m is not None:
            out[f"__{n}.m__"], out[f"__{n}.v__"] = ar.m, ar.v
    return out


def check_captured_run_equals_eager(make, dev):
    """five steps eager, and three eager + capture + two replays, of the estimators `make(dev)` builds (shared with
    tests/test_gpu_ple.py)"""
    a, _, batches = make(dev)
    b, _, _ = make(dev)
    feats, labels = batches[0]
    for _ in range(5):
        la = a.train_step(feats, labels)
    g = GraphedTrainStep(b.train_step, feats, labels, warmup=3)
    g()
    lb = g()
    torch.cuda.synchronize()
    assert int(a.store.opt_state["step"]) == int(b.store.opt_state["step"]) == 5
    assert_bit_exact(lb, la, "captured loss")
    A, B_ = _state(a), _state(b)
    assert set(A) == set(B_)
    for k in A:
        assert_bit_exact(B_[k], A[k], f"captured vs eager {k}")


def test_captured_run_equals_eager_bit_for_bit(dev):
    """the reference's default configuration"""
    check_captured_run_equals_eager(make, dev)


class _AbandonedStep(Exception):
    pass


def check_abandoned_step(make, dev, monkeypatch, kw, n_dense_bwd, colsums_left):
    """A step whose backward stops with an exception at its last dense_bwd (of `n_dense_bwd`; at least `colsums_left` of the
    gates' column sums and the towers' six split sums are parked by then) never reaches the optimizer's drain; the steps that
    follow are bit-identical to those of an estimator that never ran it (the contract tests/test_gpu_models.py pins for DCN,
    DeepFM and PNN).  `kw` has no BatchNorm: a training-mode forward updates the moving averages by design, also in an
    abandoned step.  Shared with tests/test_gpu_ple.py."""
    from recalgorithm_amd import ops
    a, _, batches = make(dev, **kw)
    b, _, _ = make(dev, **kw)
    real = ops.dense_bwd
    calls = {"n": 0, "at": None, "left": None}

    def dense_bwd(*args, **k):
        calls["n"] += 1
        if calls["n"] == calls["at"]:
            calls["left"] = (len(ops._colsum_pending), len(ops._dense_pending))
            raise _AbandonedStep()
        return real(*args, **k)
    monkeypatch.setattr(ops, "dense_bwd", dense_bwd)
    b.train_step(*batches[1])
    n_calls, calls["n"] = calls["n"], 0
    assert n_calls == n_dense_bwd
    a.train_step(*batches[1])
    calls["n"], calls["at"] = 0, n_calls
    with pytest.raises(_AbandonedStep):
        a.train_step(*batches[0])
    assert calls["left"][0] >= colsums_left and calls["left"][1] >= 6, calls["left"]
    calls["at"] = None
    for est in (a, b):
        for bt in (batches[2], batches[0], batches[3]):
            est.train_step(*bt)
            assert not ops._colsum_pending and not ops._dense_pending
    torch.cuda.synchronize()
    assert int(a.store.opt_state["step"]) == int(b.store.opt_state["step"]) == 4
    A, B_ = _state(a), _state(b)
    assert set(A) == set(B_)
    for k in B_:
        assert_bit_exact(A[k], B_[k], f"after the abandoned step: {k}")


def test_abandoned_step_leaves_nothing_to_the_next(dev, monkeypatch):
    """the last dense_bwd is the expert layers': the gate-mix backward has parked the gate kernels' column sums by then.
    Two hidden layers per tower, then the three expert layers; the three gates' column sums."""
    kw = dict(B=300, hidden=("64", "32"), H=64, dropout_rate=0.0, batch_norm=False)
    check_abandoned_step(make, dev, monkeypatch, kw, 6 + 3, 3)


def _write_dataset(tmp_path, n):
    spec = synth.SynthSpec(n_fields=6, max_vocab=300, seed=5, oov_frac=0.1, with_dense=True, with_history=True, with_tags=True)
    vocab_dir = str(tmp_path / "vocabulary") + "/"
    synth.write_vocabularies(spec, vocab_dir)
    path = str(tmp_path / "train.tfrecord")
    synth.write_tfrecord(spec, path, n, chunk=256)
    return vocab_dir, path


def test_serving_returns_the_three_probabilities(dev, tmp_path):
    from recalgorithm_amd import export as E
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.MMOE import mmoe as m
    from recalgorithm_amd.algorithm.utils import eval_input_fn
    from recalgorithm_amd.io import tfrecord
    vocab_dir, path = _write_dataset(tmp_path, 600)
    flags.FLAGS.vocabulary_dir, flags.FLAGS.task_names = vocab_dir, ",".join(TASKS)
    dense, cat, label = m.create_feature_columns()
    m.total_feature_columns, m.label_feature_columns = dense + cat, label
    params = {"dense_feature_columns": dense, "category_feature_columns": cat, "hidden_units": ["32", "16"], "dropout_rate": 0.1,
              "batch_norm": True, "learning_rate": 0.005, "num_experts": 3, "num_tasks": 3, "expert_hidden_units": 32,
              "task_names": list(TASKS)}
    est = Estimator(m.mmoe_model_fn, params, RunConfig(device=dev, seed=11))
    est.train(lambda: eval_input_fn(path, m.example_parser, 200), log_every=0)
    assert est.global_step == 3
    metrics = est.evaluate(lambda: eval_input_fn(path, m.example_parser, 200))
    assert {f"eval_{t}_{k}" for t in TASKS for k in ("auc", "accuracy")} <= set(metrics)
    preds = list(est.predict(lambda: eval_input_fn(path, m.example_parser, 200)))
    keys = {f"{t}_probabilities" for t in TASKS}
    assert len(preds) == 600 and set(preds[0]) == keys
    recv = E.build_parsing_serving_input_receiver_fn(fc.make_parse_example_spec(dense + cat))
    export_dir = E.BestExporter(name="best_exporter", serving_input_receiver_fn=recv, exports_to_keep=5).export(
        est, str(tmp_path / "export"), None, metrics, True)
    served = E.ServingModel(m.mmoe_model_fn, params, export_dir, device=dev)
    out = served.predict(list(tfrecord.read_records(path))[:200])
    assert set(out) == keys
    for k in keys:
        want = torch.tensor([float(p[k].reshape(-1)[0]) for p in preds[:200]])
        assert torch.equal(torch.from_numpy(out[k]).reshape(-1), want), f"served {k} differs from PREDICT"


def test_main_trains_and_prints_the_six_metrics(dev, tmp_path):
    """python -m recalgorithm_amd.algorithm.MMOE.mmoe on synthetic 3-label TFRecords, as a child process"""
    vocab_dir, path = _write_dataset(tmp_path, 1200)
    cmd = [sys.executable, "-m", "recalgorithm_amd.algorithm.MMOE.mmoe", f"--train_data={path}", f"--eval_data={path}",
           f"--vocabulary_dir={vocab_dir}", f"--model_dir={tmp_path / 'model_dir'}", "--batch_size=256", "--train_steps=4",
           "--hidden_units=32,16", "--expert_hidden_units=32", "--shuffle_buffer_size=0"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for t in TASKS:
        for kind in ("auc", "accuracy"):
            line = [ln for ln in r.stdout.splitlines() if ln.startswith(f"eval_{t}_{kind}: ")]
            assert line, f"eval_{t}_{kind} not printed:\n{r.stdout[-2000:]}"
            assert 0.0 <= float(line[-1].split(": ")[1]) <= 1.0
    assert "after evaluate" in r.stdout
    rows = open(tmp_path / "predictions.csv").read().splitlines()
    assert rows[0] == "," + ",".join(f"{t}_probabilities" for t in TASKS) and len(rows) == 1201
