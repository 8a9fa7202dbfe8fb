"""-m gpu: the fused AFM attention kernels (csrc/afm.hip, include/recalgo_afm.h) behind nn.afm_attention(fused=True) and, where
they serve the shape, behind fused=None: parity with tests/afm_ref.py at every shape the kernels change path (one pair, a
masked tile, whole tiles, every K arm, several column tiles, the limits of F, K and t, a batch that does not fill its last
workgroup), the refusals, row independence, the partial rows at the C ABI under guarded allocations, the PREDICT form, large
scores, run to run and under torch.cuda.graph, and the model on both paths against the float64 oracle model."""
import ctypes

import pytest
import torch

from recalgorithm_amd import _lib, ops
from tests import afm_ref as R
from tests.test_gpu_afm import make_step, run_op
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu
REDUCED = ("dw", "dbias", "dh")

# (B, F, K, t)
SHAPES = [(1, 2, 8, 16),         # P = 1: the softmax is 1, ds = 0
          (5, 3, 4, 32),         # K = 4: one MFMA k-step
          (2, 6, 4, 16),         # P = 15: one tile, one row masked
          (3, 16, 8, 16),        # P = 120: 7.5 tiles
          (3, 17, 8, 48),        # P = 136: 8.5 tiles; t = 3 column tiles
          (5, 5, 12, 32),        # K = 12
          (3, 6, 20, 16),        # K = 20
          (2, 33, 4, 16),        # P = 528: exactly 33 tiles
          (130, 7, 8, 16),       # the golden's F and K; B not a multiple of the waves per workgroup
          (67, 9, 16, 128),
          (33, 26, 16, 128),     # the bench shape's P = 325
          (3, 64, 8, 32),        # P = 2016, the limit
          (3, 4, 32, 256)]       # K and t at their limits
MID = (67, 9, 16, 128)


def _count(monkeypatch, names=("recalgo_afm_attention_fwd", "recalgo_afm_attention_bwd")):
    """counting wrappers around the library's entries -> {name: calls}"""
    lib, calls = _lib.load(), {}
    for name in names:
        real = getattr(lib, name)
        calls[name] = 0

        def counted(*a, _real=real, _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


@pytest.mark.parametrize("B,F,K,t", SHAPES)
def test_parity(dev, B, F, K, t):
    x, r64, r32 = R.case(B, F, K, t)
    got = run_op(dev, x, fused=True)
    for k in R.NAMES:
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        assert_close(got[k], r64[k], what=f"nn.afm_attention(fused=True) B={B} F={F} K={K} t={t} {k}", reduced=k in REDUCED,
                     ref32=r32[k])


def test_fused_none_takes_the_kernel(dev, monkeypatch):
    x, _, _ = R.case(*MID)
    calls = _count(monkeypatch)
    run_op(dev, x, fused=False)
    assert calls == {"recalgo_afm_attention_fwd": 0, "recalgo_afm_attention_bwd": 0}
    got = run_op(dev, x, fused=None)
    assert calls == {"recalgo_afm_attention_fwd": 1, "recalgo_afm_attention_bwd": 1}
    want = run_op(dev, x, fused=True)
    for k in R.NAMES:
        assert_bit_exact(got[k], want[k], f"fused=None against fused=True, {k}")


@pytest.mark.parametrize("B,F,K,t", [(4, 7, 8, 12), (4, 7, 6, 16), (4, 65, 4, 16), (4, 7, 8, 272)])
def test_unserved_shapes_are_refused(dev, B, F, K, t):
    step = make_step(dev, R.inputs(B, F, K, t), fused=True)
    with pytest.raises(ValueError, match=r"afm_attention\(fused=True\): no fused kernel serves"):
        step()


def _rows_of(x, rows):
    """the case `x` cut down to the examples `rows`, in that order"""
    return dict(x, fields=x["fields"][rows].clone(), g=x["g"][rows].clone())


def test_a_row_depends_on_that_row_alone(dev):
    x, _, _ = R.case(*MID)
    whole = run_op(dev, x, fused=True)
    for r in (0, 31, 66):
        alone = run_op(dev, _rows_of(x, [r]), fused=True)
        five = run_op(dev, _rows_of(x, [1, 2, 5, r, 7]), fused=True)
        for k in ("out", "d_fields"):
            assert_bit_exact(alone[k][0], whole[k][r], f"row {r} alone, {k}")
            assert_bit_exact(five[k][3], whole[k][r], f"row {r} as the fourth of five, {k}")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _run_entries(lib, dev, x, with_scores=True):
    """Both C entries on buffers of exactly the documented sizes (call under tests/redzone.guarded) ->
    (out, scores, {d_fields, dw, db, dh})"""
    B, F, K = x["fields"].shape
    t, P = x["w"].shape[1], F * (F - 1) // 2
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fields, w, b, h, g = (x[k].contiguous().to(dev) for k in ("fields", "w", "bias", "h", "g"))
    out = torch.empty(B, K, device=dev)
    scores = torch.empty(B, P, device=dev) if with_scores else None
    lib.recalgo_afm_attention_fwd(_p(fields), _p(w), _p(b), _p(h), B, F, K, t, _p(out), _p(scores), st)
    if not with_scores:
        return out, None, None
    grads = {"d_fields": torch.empty(B, F * K, device=dev), "dw": torch.empty(K, t, device=dev), "db": torch.empty(t, device=dev),
             "dh": torch.empty(t, device=dev)}
    ws = ops._workspace(int(lib.recalgo_afm_bwd_workspace_bytes(B, F, K, t)), torch.device(dev))
    lib.recalgo_afm_attention_bwd(_p(g), _p(fields), _p(w), _p(b), _p(h), _p(scores), B, F, K, t, *[_p(v) for v in grads.values()],
                                  _p(ws), st)
    return out, scores, grads


@pytest.mark.parametrize("B,F,K,t", [(5, 3, 4, 32), (33, 26, 16, 128)])
def test_the_outputs_are_the_fixed_order_sums_of_the_partial_rows(dev, B, F, K, t):
    """dw, db and dh ARE tests/dense_ref.colsum_fixed_order of the workspace's rows [dw | db | dh], bit for bit; the workspace
    is exactly as large as the query says and the guard finds no store outside any buffer.  Without `scores` (PREDICT, EVAL)
    the forward gives the same `out` bits."""
    from tests.redzone import guarded
    from tests.test_gpu_colsums import _assert_outputs_are_the_sums, _workspace_of
    x, r64, r32 = R.case(B, F, K, t)
    with guarded() as g:
        lib = _lib.load()
        rows = int(lib.recalgo_afm_bwd_partial_rows(B, F, K, t))
        assert rows == -(-B // 4) and int(lib.recalgo_afm_bwd_workspace_bytes(B, F, K, t)) == rows * (K * t + 2 * t) * 4
        out, scores, grads = _run_entries(lib, dev, x)
        ws = _workspace_of(g)
        assert ws.numel() == max(rows * (K * t + 2 * t), 4)
        _assert_outputs_are_the_sums(ws, rows, {k: grads[k] for k in ("dw", "db", "dh")}, f"afm_attention_bwd B={B} F={F} K={K} t={t}")
        plain, _, _ = _run_entries(lib, dev, x, with_scores=False)
        assert_bit_exact(plain, out, "out without scores against out with scores")
        assert {"recalgo_afm_attention_fwd", "recalgo_afm_attention_bwd"} <= g.launched
        assert_close(scores, r64["s"], what=f"the saved scores B={B} F={F} K={K} t={t}", ref32=r32["s"])
        for k, name in (("out", "out"), ("d_fields", "d_fields"), ("dw", "dw"), ("db", "dbias"), ("dh", "dh")):
            got = out if k == "out" else grads[k]
            assert_close(got.reshape(r64[name].shape), r64[name], what=f"the C entries B={B} F={F} K={K} t={t} {k}",
                         reduced=name in REDUCED, ref32=r32[name])


LARGE = {"bias = 1, h = 5": R.LARGE_SCORES["bias = 1, h = 5"], "h x 450": dict(B=33, F=7, K=8, t=16, h_scale=450.0)}


@pytest.mark.parametrize("name", list(LARGE))
def test_large_scores(dev, name):
    """bias = +1, h = +5 at (67, 9, 16, 128): scores of 550 .. 1186.  h scaled by 450 at (33, 7, 8, 16): scores from -1178 to
    +338; exp() of an unshifted score would overflow or vanish.  Every output is finite and parity holds with the floor of
    afm_ref.fp32_floor (4 x the float32 restatement's own deviation)."""
    x, r64, r32 = R.case(**LARGE[name])
    if name == "h x 450":
        assert float(r64["s"].min()) < -1000 and float(r64["s"].max()) > 300
    got = run_op(dev, x, fused=True)
    for k in R.NAMES:
        assert bool(torch.isfinite(got[k]).all()), k
        assert_close(got[k], r64[k], what=f"nn.afm_attention(fused=True), {name}: {k}", reduced=k in REDUCED, ref32=r32[k],
                     floor=R.fp32_floor(r64, r32, k))


def _captured_three_times(run, first, what):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for i in range(3):
        for c in captured:
            c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, u, w_ in zip(R.NAMES, captured, first):
            assert_bit_exact(u, w_, f"{what}: replay {i}, {name}")


def test_two_runs_and_three_replays_give_the_same_bits(dev):
    """the step (forward + backward + flush_dense_splits), then the forward alone: eagerly twice, once on a side stream (the
    warm-up a capture needs), captured and replayed three times"""
    x, _, _ = R.case(*MID)
    step = make_step(dev, x, fused=True)
    B, F, K = x["fields"].shape
    fields = x["fields"].reshape(B, F * K).to(dev)
    w, b, h = (x[k].to(dev) for k in ("w", "bias", "h"))

    def forward():
        with torch.no_grad():
            return [ops.afm_attention(fields, F, K, w, b, h)]
    for run, what in ((step, "step"), (forward, "forward")):
        first = [o.clone() for o in run()]
        for name, u, w_ in zip(R.NAMES, run(), first):
            assert_bit_exact(u, w_, f"{what}: second eager run, {name}")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        _captured_three_times(run, first, what)
        if what == "step":
            assert_bit_exact(forward()[0], first[0], "the forward without scores against the step's out")


# ---- the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["afm_fused=True", "afm_fused=False"])
def test_the_model_on_both_paths_follows_the_fp64_oracle(dev, fused, tmp_path, monkeypatch):
    """model_afm's columns with attention_factor = 16 (F = 7, K = 8, t = 16: served) on the variables the estimator drew, the
    attention network's and p redrawn at a scale where the scores differ: PREDICT, the TRAIN loss, every gradient and one Adam
    step against oracle.ref_models.afm in float64, with the floor of the float32 oracle's own deviation
    (golden_protocol.judge_step_against_oracle).  Under True a TRAIN step launches each fused entry exactly once (PREDICT the
    forward once more), under False neither runs."""
    from recalgorithm_amd.estimator import ModeKeys
    from tests.golden_protocol import build_on_device, judge_step_against_oracle, run_oracle
    from tests.test_gpu_golden import suite_case
    case = suite_case("model_afm")
    inner = case.mirror_setup

    def setup(name, vocab_dir):
        model_fn, params = inner(name, vocab_dir)
        return model_fn, dict(params, attention_factor=16, afm_fused=fused)
    case.mirror_setup = setup
    est, golden, feats, lab = build_on_device(dev, case, "model_afm", tmp_path)
    arrays = est.store.named_arrays()
    gen = torch.Generator().manual_seed(16)
    for k, v in arrays.items():
        if k.startswith("attention_part/") or k == "prediction_score_part/p":
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.5)
        elif k.startswith("pair_interaction_part/"):
            v.copy_(torch.randn(*v.shape, generator=gen))
    assert tuple(arrays["attention_part/attention_w"].shape) == (8, 16)
    variables = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
    before = {k: v.detach().cpu().double().clone() for k, v in arrays.items()}
    r64 = run_oracle(case, golden, torch.float64, variables=variables)
    r32 = run_oracle(case, golden, torch.float32, variables=variables)

    calls = _count(monkeypatch)
    pr = est._call_model_fn(feats, None, ModeKeys.PREDICT)
    assert calls == {"recalgo_afm_attention_fwd": int(fused), "recalgo_afm_attention_bwd": 0}
    assert_close(pr.predictions["probabilities"], r64["predict"]["prob"], what=f"afm (t = 16, afm_fused={fused}) predict",
                 ref32=r32["predict"]["prob"])
    spec = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
    assert_close(spec.loss, r64["loss"], what=f"afm (t = 16, afm_fused={fused}) loss", ref32=r32["loss"])
    judge_step_against_oracle(est, spec, r64["P"], r32["P"], before, golden.params["learning_rate"], f"afm t=16 afm_fused={fused}", 8)
    assert calls == {"recalgo_afm_attention_fwd": 2 * int(fused), "recalgo_afm_attention_bwd": int(fused)}
