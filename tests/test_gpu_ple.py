"""-m gpu: PLE on the MI355X — ops.cgc_mix (csrc/cgc.hip) against float64 at the reference's default block shapes, at every
limit and at the other arms, once more under the guarded allocations of tests/redzone.py; the mirrored model_fn against
the two reference-generated goldens and against tests/ple_ref.py at the reference's default configuration, the captured
Estimator run, the abandoned-step contract, and the script's main().
Tolerance: the project's standing 1e-5 bound and strict guard (tests/util.py assert_close with ref32=)."""
import os
import subprocess
import sys

import pytest
import torch

from recalgorithm_amd import feature_column as fc
from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
from recalgorithm_amd.io import synth
from tests import ple_ref
from tests.golden_protocol import check_on_device, judge_step_against_oracle
from tests.redzone import guarded
from tests.test_gpu_mmoe import DIMS, _oracle_inputs, _unaligned, check_abandoned_step, check_captured_run_equals_eager, expert_pattern
from tests.test_mmoe_host import TASKS
from tests.test_ple_host import CASE, GOLDENS
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL0 = ple_ref.ple_selection([5, 5, 5], 10, all_gate=True)       # 3 task gates of 15 and the all-gate of 25: NT = 70
FINAL = ple_ref.ple_selection([5, 5, 5], 10)                       # 3 task gates of 15: NT = 45
# a 32-wide gate, a gate with a duplicate, six more: E = 32, G = 8, n_g = 32 at once
LIMITS = [list(range(32)), [3, 3, 7]] + [[i, 31 - i] for i in range(6)]


def _inputs(B, In, E, H, selection, seed, scale=1.0, relu=False, n_grads=None):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, In, generator=gen, dtype=torch.float64)
    ws = [torch.randn(In, len(s), generator=gen, dtype=torch.float64) * (scale / In ** 0.5) for s in selection]
    ex = [torch.randn(B, H, generator=gen, dtype=torch.float64) for _ in range(E)]
    if relu:
        ex = [torch.relu(t) for t in ex]
    gs = [torch.randn(B, H, generator=gen, dtype=torch.float64) for _ in range(len(selection) if n_grads is None else n_grads)]
    return x, ws, ex, gs


def _reference(x, ws, ex, gs, selection, sum_outputs, dtype, relu=False):
    """-> (outs, gates, dx, dws, dexs) of tests/ple_ref.cgc in `dtype` (gs[g] None: that gate gets no gradient; relu: the
    experts are ReLU outputs and d_expert is the gradient at the pre-activation)"""
    x = x.detach().clone().to(dtype).requires_grad_(True)
    ws = [w.detach().clone().to(dtype).requires_grad_(True) for w in ws]
    pre = [t.detach().clone().to(dtype).requires_grad_(True) for t in ex]
    outs, ps = ple_ref.cgc(x, ws, [torch.relu(t) for t in pre] if relu else pre, selection, sum_outputs)
    outs = [outs] if sum_outputs else outs
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gs) if g is not None)
    grads = torch.autograd.grad(loss, [x, *ws, *pre], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [x, *ws, *pre])]
    G = len(ws)
    return [o.detach() for o in outs], torch.cat(ps, dim=1).detach(), grads[0], grads[1:1 + G], grads[1 + G:]


def _run_hip(dev, x, ws, ex, gs, selection, sum_outputs, relu=False, unaligned=False, strided_grad=False, unaligned_grad=False):
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
    outs, p = ops.cgc_mix(xd, wd, ed, selection, sum_outputs=sum_outputs, return_gates=True)
    outs = [outs] if sum_outputs else outs
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


_REFS = {}          # (case key) -> (inputs, float64 reference, float32 reference): computed once, shared, left unchanged


def _case(shape, seed, scale=1.0, relu=False, drop_gate=None):
    B, In, E, H, selection, sum_outputs = shape
    key = (B, In, E, H, tuple(map(tuple, selection)), sum_outputs, seed, scale, relu, drop_gate)
    if key not in _REFS:
        x, ws, ex, gs = _inputs(B, In, E, H, selection, seed, scale=scale, relu=relu, n_grads=1 if sum_outputs else None)
        if drop_gate is not None:
            gs[drop_gate] = None
        _REFS[key] = ((x, ws, ex, gs), _reference(x, ws, ex, gs, selection, sum_outputs, torch.float64, relu=relu),
                      _reference(x, ws, ex, gs, selection, sum_outputs, torch.float32, relu=relu))
    return _REFS[key]


def _check(dev, shape, seed, what, scale=1.0, relu=False, drop_gate=None, **kw):
    B, In, E, H, selection, sum_outputs = shape
    (x, ws, ex, gs), r64, r32 = _case(shape, seed, scale, relu, drop_gate)
    outs, p, dx, dws, dexs = _run_hip(dev, x, ws, ex, gs, selection, sum_outputs, relu=relu, **kw)
    assert_close(p, r64[1], what=f"{what} gates", ref32=r32[1])
    at = 0
    for s in selection:                      # each gate sums to 1
        assert float((p[:, at:at + len(s)].sum(dim=1) - 1).abs().max()) < 1e-5, what
        at += len(s)
    assert len(outs) == (1 if sum_outputs else len(selection))
    for g, o in enumerate(outs):
        assert_close(o, r64[0][g], what=f"{what} out{g}", ref32=r32[0][g])
    assert_close(dx, r64[2], what=f"{what} dx", ref32=r32[2])
    for g, dw in enumerate(dws):
        assert dw is not None
        assert_close(dw, r64[3][g], what=f"{what} dW{g}", reduced=True, ref32=r32[3][g])       # (a sum over the batch)
    for e, de in enumerate(dexs):
        assert_close(de, r64[4][e], what=f"{what} d_expert{e}", ref32=r32[4][e])
    return outs, p, dx, dws, dexs


# (B, In, E, H, table, sum_outputs)
CASES = {
    "level0": (261, 82, 25, 256, LEVEL0, True),              # the default extraction network
    "final": (261, 256, 25, 256, FINAL, False),              # the default final CGC: 46 KiB of staged gate kernels
    "tiny": (5, 3, 2, 4, [[1, 0]], False),
    "tiny_sum": (5, 3, 2, 4, [[1, 0]], True),
    "limits": (70, 40, 32, 8, LIMITS, False),                # E = 32, G = 8, n_g = 32, a duplicate
    "limits_sum": (70, 40, 32, 8, LIMITS, True),
    "ragged": (33, 20, 5, 1028, [list(range(5))] * 3, False),        # H / 4 = 257: a fifth lane pass with one live lane
    "ragged_sum": (33, 20, 5, 1028, [list(range(5))] * 3, True),
}


def _rounds_case(H=256):
    """B = 2 * (rows one backward pass covers) + 1 at the default extraction network's shape (In 82, E 25, the level-0
    table, H 256, summed): every workgroup walks three backward rounds — the dWg registers carried across them, the per-round
    zeroing of the dot products — the last with a single live row in the whole grid; the forward walks two.  The rows per
    pass come from recalgo_cgc_partial_rows (the backward grid) and the rows per workgroup it implies."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    grid = int(lib.recalgo_cgc_partial_rows(1 << 24, 82, 70))
    per_wg = next(b for b in range(1, 4096) if lib.recalgo_cgc_partial_rows(b + 1, 82, 70) == 2)
    assert grid >= 2 and int(lib.recalgo_cgc_partial_rows(grid * per_wg, 82, 70)) == grid
    return (2 * grid * per_wg + 1, 82, 25, H, LEVEL0, True)


@pytest.mark.parametrize("case", list(CASES))
def test_cgc_mix_against_float64(dev, case):
    _check(dev, CASES[case], 21, case)


@pytest.mark.parametrize("H", [256, 16])
def test_cgc_mix_several_rounds_and_a_ragged_last_one(dev, H):
    """H 256: the shape the issue names (every lane streams a chunk).  H 16: the same rounds with 4 of 64 lanes live."""
    shape = _rounds_case(H)
    assert shape[0] > 2048
    _check(dev, shape, 22, f"rounds H={H}")


@pytest.mark.parametrize("sum_outputs", [False, True])
def test_cgc_mix_relu_experts_get_a_masked_gradient(dev, sum_outputs):
    _check(dev, (200, 82, 7, 64, ple_ref.ple_selection([2, 1, 3], 1, all_gate=sum_outputs), sum_outputs), 23, "relu experts",
           relu=True)


ARM_SHAPE = (301, 82, 7, 128, ple_ref.ple_selection([2, 1, 2], 2), False)
ARM_SHAPE_SUM = (301, 82, 7, 128, ple_ref.ple_selection([2, 1, 2], 2, all_gate=True), True)


@pytest.mark.parametrize("arm", ["unaligned", "unaligned_grad", "strided_grad", "null_grad"])
def test_cgc_mix_other_arms(dev, arm):
    """unaligned: expert base pointers off 16-byte alignment select the scalar-access arm of both kernels; unaligned_grad:
    aligned experts, but a contiguous upstream gradient off 16-byte alignment — the backward entry point's own detection;
    strided_grad: a non-contiguous upstream gradient is made contiguous by the host side; null_grad (no-sum only): a gate
    nobody differentiates reaches the kernel as a NULL pointer."""
    if arm == "null_grad":
        _check(dev, ARM_SHAPE, 24, arm, drop_gate=1)
        _check(dev, CASES["limits"], 24, "limits null_grad", drop_gate=0)
        return
    kw = {arm: True}
    _check(dev, ARM_SHAPE, 24, arm, **kw)
    _check(dev, ARM_SHAPE_SUM, 24, arm + " sum", **kw)


def test_cgc_mix_large_gate_logits(dev):
    """gate logits of magnitude > 80 (scaled gate kernels): the max-subtracted softmax stays finite, each gate sums to 1"""
    shape = (300, 82, 25, 64, LEVEL0, True)
    (x, ws, _, _), _, _ = _case(shape, 25, scale=40.0)
    assert float((x @ ws[0]).abs().max()) > 80.0
    outs, p, *_ = _check(dev, shape, 25, "large logits", scale=40.0)
    assert torch.isfinite(p).all() and all(torch.isfinite(o).all() for o in outs)


def test_cgc_mix_is_deterministic_and_capturable(dev):
    from recalgorithm_amd import ops
    for shape in (CASES["level0"], CASES["final"]):
        B, In, E, H, sel, sum_outputs = shape
        (x, ws, ex, gs), _, _ = _case(shape, 21)
        a = _run_hip(dev, x, ws, ex, gs, sel, sum_outputs)
        b = _run_hip(dev, x, ws, ex, gs, sel, sum_outputs)

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
            outs, p = ops.cgc_mix(xd, wd, ed, sel, sum_outputs=sum_outputs, return_gates=True)
            outs = [outs] if sum_outputs else outs
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
        for i, (u, v) in enumerate(zip(captured, flat(a))):
            assert_bit_exact(u, v, f"graph replay, tensor {i}")


def test_cgc_mix_limits(dev):
    import ctypes

    from recalgorithm_amd import _lib, ops
    x = torch.zeros(8, 82, device=dev)
    e3 = [torch.zeros(8, 8, device=dev) for _ in range(3)]
    with pytest.raises(NotImplementedError):
        ops.cgc_mix(x, [torch.zeros(82, 3, device=dev)], [torch.zeros(8, 6, device=dev) for _ in range(3)], [[0, 1, 2]])   # H % 4
    with pytest.raises(ValueError):
        ops.cgc_mix(x, [torch.zeros(82, 0, device=dev)], e3, [[]])                                                      # empty gate
    with pytest.raises(NotImplementedError):
        ops.cgc_mix(x, [torch.zeros(82, 33, device=dev)], [torch.zeros(8, 8, device=dev) for _ in range(33)], [list(range(33))])
    with pytest.raises(NotImplementedError):
        ops.cgc_mix(torch.zeros(8, 512, device=dev), [torch.zeros(512, 20, device=dev)] * 3, e3, [[0, 1, 2] * 6 + [0, 1]] * 3)   # LDS
    # the entry point checks again: an error code (raised by the binding), never a launch
    lib = _lib.load()
    n_sel, sel = (ctypes.c_int * 1)(3), (ctypes.c_int * 3)(0, 1, 2)
    e = [torch.zeros(8, 6, device=dev) for _ in range(3)]
    w, o, p = torch.zeros(82, 3, device=dev), torch.zeros(8, 6, device=dev), torch.zeros(8, 3, device=dev)
    with pytest.raises(_lib.RecalgoError, match="recalgo_cgc_fwd failed with hipError_t=[1-9]"):
        lib.recalgo_cgc_fwd(ops._p(x), 82, ops._ptr_array([w]), n_sel, sel, ops._ptr_array(e), 8, 82, 3, 1, 6, 0,
                            ops._ptr_array([o]), ops._p(p), ops._stream(x))
    sel_bad = (ctypes.c_int * 3)(0, 1, 3)                    # an expert index past E
    with pytest.raises(_lib.RecalgoError, match="recalgo_cgc_fwd failed with hipError_t=[1-9]"):
        lib.recalgo_cgc_fwd(ops._p(x), 82, ops._ptr_array([w]), n_sel, sel_bad, ops._ptr_array(e3), 8, 82, 3, 1, 8, 0,
                            ops._ptr_array([torch.zeros(8, 8, device=dev)]), ops._p(p), ops._stream(x))


def test_kernel_cases_under_the_redzone_guard(dev):
    """tests/test_gpu_redzone.py cannot list a new module; the fences, the NaN poison and the launch record work for any entry
    reached through _lib.load().  Every kernel-level case above once more, inside guarded(): no byte outside an output, a
    gradient or the partial rows is written, and no element of them is left unwritten (0xFF.. is a NaN: assert_close fails)."""
    with guarded() as g:
        for case in CASES:
            _check(dev, CASES[case], 21, case + " (guarded)")
        for H in (256, 16):
            _check(dev, _rounds_case(H), 22, f"rounds H={H} (guarded)")
        for sum_outputs in (False, True):
            _check(dev, (200, 82, 7, 64, ple_ref.ple_selection([2, 1, 3], 1, all_gate=sum_outputs), sum_outputs), 23,
                   "relu experts (guarded)", relu=True)
        for arm in ("unaligned", "unaligned_grad", "strided_grad"):
            _check(dev, ARM_SHAPE, 24, arm + " (guarded)", **{arm: True})
            _check(dev, ARM_SHAPE_SUM, 24, arm + " sum (guarded)", **{arm: True})
        _check(dev, ARM_SHAPE, 24, "null_grad (guarded)", drop_gate=1)
        assert {"recalgo_cgc_fwd", "recalgo_cgc_bwd", "recalgo_cgc_partial_rows", "recalgo_cgc_supported"} <= g.launched
        assert g.records_at("ops.py"), "the op's buffers were not allocated under the guard"


# ---- the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GOLDENS))
def test_model_golden(dev, name, tmp_path):
    check_on_device(dev, CASE, name, tmp_path)


def make(dev, B=1000, hidden=("512", "256", "128"), H=256, per_task=(5, 5, 5), shared=10, levels=1, dropout_rate=0.1,
         batch_norm=True, seed=5, **run):
    from recalgorithm_amd.algorithm._common import dense_columns
    from recalgorithm_amd.algorithm.PLE.ple import ple_model_fn
    spec = synth.SynthSpec(n_fields=8, max_vocab=400, seed=11, oov_frac=0.05, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": dense_columns(), "category_feature_columns": [fc.embedding_column(c, k) for c, k in zip(cats, DIMS)],
              "hidden_units": list(hidden), "dropout_rate": dropout_rate, "batch_norm": batch_norm, "learning_rate": 0.005,
              "num_tasks": 3, "expert_hidden_units": H, "task_names": list(TASKS), "num_extract_network": levels,
              "num_experts_per_task": list(per_task), "num_experts_in_shared": shared}
    est = Estimator(ple_model_fn, params, RunConfig(device=dev, seed=seed, **run))
    batches = [synth.device_features(spec, B, dev, batch_index=i, extra_labels=TASKS[1:])[:2] for i in range(4)]
    est.build(*batches[0])
    return est, params, batches


def test_default_configuration_step_against_float64(dev):
    """The reference's defaults — 5+5+5 task experts and 10 shared of 256 units, one extraction network, hidden_units
    512,256,128, 3 tasks, BatchNorm on, dropout 0.1 (the keep masks of the library's hash stream recorded and handed to both
    oracles) — at B = 1000 (the kernel cases cover large B).  Gradients are compared conditional on the HIP forward's ReLU
    pattern, as tests/test_gpu_mmoe.py does (tests/test_gpu_baseline_shapes.py _ReluPattern)."""
    from recalgorithm_amd import nn, ops
    B = 1000
    est, params, batches = make(dev)
    feats, labels = batches[0]
    P, cf, cl = _oracle_inputs(est, feats, labels, torch.float64)
    P32, cf32, cl32 = _oracle_inputs(est, feats, labels, torch.float32)
    before = {k: v.detach().cpu().double().clone() for k, v in est.store.named_arrays().items()}
    pattern = expert_pattern()
    nn.DROPOUT_SPECS[:] = []
    spec = pattern.record_hip(lambda: est._call_model_fn(feats, labels, ModeKeys.TRAIN))
    dspecs = list(nn.DROPOUT_SPECS)
    assert len(dspecs) == 9 and all(d.mask is None for d in dspecs)
    masks = [ops.dropout_keep_mask((B, w), d, dev).cpu() for d, w in zip(dspecs, (512, 256, 128) * 3)]
    assert all(0.85 < float(m.mean()) < 0.95 for m in masks)
    assert len(pattern.masks) == 50 + 9      # two blocks of 25 experts, then the towers
    for pm, km in zip(pattern.masks[50:], masks):        # dropout fused into the dense epilogue: the recorded outputs are the dropped tensors
        pattern.kept[id(pm)] = km
    ref = pattern.oracle(lambda: ple_ref.ple(P, cf, cl, params, training=True, dropout_masks=[m.clone() for m in masks]), check=True)
    ref["loss"].backward()
    r32 = pattern.oracle(lambda: ple_ref.ple(P32, cf32, cl32, params, training=True, dropout_masks=[m.clone() for m in masks]))
    r32["loss"].backward()
    for shape, n_flip, dist in pattern.flips:
        assert dist < 1e-4 and n_flip < 64, f"activation pattern differs beyond rounding at layer {shape}"
    assert_close(spec.loss, ref["loss"], what="ple loss", ref32=r32["loss"])
    for t in TASKS:
        assert_close(spec.predictions[f"{t}_probabilities"], ref["probs"][t], what=f"ple {t} prob", ref32=r32["probs"][t])
    judge_step_against_oracle(est, spec, P, P32, before, params["learning_rate"], "ple", 2 * 50 + 7 + 21)


def test_captured_run_equals_eager_bit_for_bit(dev):
    """the reference's default configuration"""
    check_captured_run_equals_eager(make, dev)


def test_abandoned_step_leaves_nothing_to_the_next(dev, monkeypatch):
    """the last dense_bwd is the extraction network's expert layers': both CGC backwards have parked the gate kernels' column
    sums by then.  The small configuration of MMoE's test: two hidden layers per tower, the final block's experts, the extraction
    network's; both blocks' gates."""
    kw = dict(B=300, hidden=("64", "32"), H=64, per_task=(2, 1, 3), shared=2, dropout_rate=0.0, batch_norm=False)
    check_abandoned_step(make, dev, monkeypatch, kw, 6 + 8 + 8, 3 + 4)


def test_main_trains_and_prints_the_six_metrics(dev, tmp_path):
    """python -m recalgorithm_amd.algorithm.PLE.ple on synthetic 3-label TFRecords, as a child process"""
    spec = synth.SynthSpec(n_fields=6, max_vocab=300, seed=5, oov_frac=0.1, with_dense=True, with_history=True, with_tags=True)
    vocab_dir = str(tmp_path / "vocabulary") + "/"
    synth.write_vocabularies(spec, vocab_dir)
    path = str(tmp_path / "train.tfrecord")
    synth.write_tfrecord(spec, path, 1200, chunk=256)
    cmd = [sys.executable, "-m", "recalgorithm_amd.algorithm.PLE.ple", f"--train_data={path}", f"--eval_data={path}",
           f"--vocabulary_dir={vocab_dir}", f"--model_dir={tmp_path / 'model_dir'}", "--batch_size=256", "--train_steps=4",
           "--hidden_units=32,16", "--expert_hidden_units=32", "--num_experts_per_task=2,1,3", "--num_experts_in_shared=2",
           "--num_extract_network=2", "--shuffle_buffer_size=0"]
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
