"""GPU: DeepCrossing's residual stack (csrc/residual.hip, include/recalgo_res.h).
  * forward and backward at the C ABI against tests/deepcrossing_ref.py in float64 (ref32 = the same restatement in float32),
    under the guarded, poisoned allocations of tests/redzone.py; every aligned width once on aligned buffers (the 16-byte
    arm) and once on views offset by 4 bytes (the 4-byte arm), the two bit-equal; the backward's saved activations are made
    on the host, so its expectation uses the masks of the very arrays the kernel reads: no element is excluded;
  * properties: two runs bit-equal; a row's bits do not depend on the batch around it; a stack of 3 is three one-unit calls;
    W1 = 0, b1 = 0 gives relu(x); save = 0 gives the last slab of save = 1;
  * every refusal the header lists returns an error and leaves the outputs at the guard's poison;
  * ops.residual_stack / nn.residual_stack against float64: the path nn.residual_stack chooses by itself on both sides of its
    width limit and at H = 40, either path forced, their agreement;
  * the model AS IT SHIPS (no switch is touched): both goldens through the mirrored deepcrossing_model_fn, 3 eager steps
    against the float64 oracle's own trajectory (tests/trajectory_ref.py's bound), and 40 hipGraph replays of the captured
    step bit for bit against eager launches — the replays also with the composed layers forced (params["fused_residual"])."""
import ctypes
import functools

import pytest
import torch

from recalgorithm_amd import _lib, ops
from tests import deepcrossing_ref as R
from tests.redzone import guarded
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

ROWS = 32                   # rows of a workgroup of csrc/residual.hip: B = 64 fills its tiles, B = 1, 17, 67 leave a partial one
# (B, D, H, L): every D of {1, 4, 82, 83, 96, 432, 512} with a B that is a multiple of the row tile and one that is not
CASES = [(67, 82, 128, 1), (67, 82, 32, 3), (17, 512, 256, 3), (1, 1, 16, 1),
         (64, 1, 48, 3), (67, 1, 16, 1), (64, 4, 16, 1), (17, 4, 128, 3), (64, 82, 128, 1), (17, 82, 48, 3),
         (64, 83, 48, 1), (67, 83, 16, 3), (64, 96, 128, 3), (67, 96, 48, 1), (64, 432, 128, 1), (17, 432, 128, 3),
         (67, 432, 256, 1), (64, 512, 16, 1)]
assert len(CASES) <= 40 and {c[1] for c in CASES} == {1, 4, 82, 83, 96, 432, 512}
assert all({c[0] % ROWS == 0 for c in CASES if c[1] == D} == {True, False} for D in (1, 4, 82, 83, 96, 432, 512))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _table(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _references(B, D, H, L):
    """(case, forward fp64, forward fp32, backward inputs, backward fp64, backward fp32), computed once per shape.  The
    backward's hs, ys are the float64 forward rounded to float32: the arrays the kernel is given, whose masks both
    expectations use."""
    case = R.random_stack(B, D, H, L, seed=1000 * D + 10 * H + L + B)
    c32 = R.cast(case, torch.float32)
    f64 = R.stack_forward(case["x"], case["w0"], case["b0"], case["w1"], case["b1"])
    f32 = R.stack_forward(c32["x"], c32["w0"], c32["b0"], c32["w1"], c32["b1"])
    hs, ys = f64[0].float(), f64[1].float()
    b64 = R.stack_backward(case["g"], hs.double(), ys.double(), case["w0"], case["w1"])
    b32 = R.stack_backward(c32["g"], hs, ys, c32["w0"], c32["w1"])
    return case, f64, f32, (hs, ys), b64, b32


def _out(g, dev, shape, shifted):
    """an output buffer full of NaN: the guard's poisoned allocation, or (shifted) a guarded buffer one element off 16 bytes"""
    if not shifted:
        return torch.empty(*shape, device=dev)
    return g.input(torch.full(shape, float("nan")), dev, shifted=True, const=False)


def run_forward(g, dev, case, save=1, shifted=False, lib=None):
    lib = lib or _lib.load()
    B, D = case["x"].shape
    L, H = len(case["w0"]), case["w0"][0].shape[1]
    x = g.input(case["x"].float(), dev, shifted=shifted)
    w = {k: [g.input(t.float(), dev, shifted=shifted) for t in case[k]] for k in ("w0", "b0", "w1", "b1")}
    hs = _out(g, dev, (L, B, H), shifted) if save else None
    ys = _out(g, dev, (L, B, D) if save else (B, D), shifted)
    lib.recalgo_res_stack_fwd(_ptr(x), _table(w["w0"]), _table(w["b0"]), _table(w["w1"]), _table(w["b1"]), B, D, H, L, int(save),
                              _ptr(hs), _ptr(ys), _stream())
    return hs, ys


def run_backward(g, dev, case, hs, ys, shifted=False, lib=None):
    lib = lib or _lib.load()
    L, B, D = ys.shape
    H = hs.shape[2]
    gi, hsd, ysd = (g.input(t.float(), dev, shifted=shifted) for t in (case["g"], hs, ys))
    w0, w1 = ([g.input(t.float(), dev, shifted=shifted) for t in case[k]] for k in ("w0", "w1"))
    dzs, dhs, dx = _out(g, dev, (L, B, D), shifted), _out(g, dev, (L, B, H), shifted), _out(g, dev, (B, D), shifted)
    lib.recalgo_res_stack_bwd(_ptr(gi), _ptr(hsd), _ptr(ysd), _table(w0), _table(w1), B, D, H, L, _ptr(dzs), _ptr(dhs), _ptr(dx),
                              _stream())
    return dzs, dhs, dx


@pytest.mark.parametrize("B,D,H,L", CASES)
def test_forward_at_the_abi_against_float64(dev, B, D, H, L):
    case, f64, f32, _, _, _ = _references(B, D, H, L)
    what = f"B={B} D={D} H={H} L={L}"
    with guarded() as g:
        runs = {}
        for shifted in ((False, True) if D % 4 == 0 else (False,)):
            arm = "4-byte arm" if (shifted or D % 4) else "16-byte arm"
            hs, ys = runs[shifted] = run_forward(g, dev, case, save=1, shifted=shifted)
            for l in range(L):
                assert_close(hs[l], f64[0][l], what=f"{what} {arm} hs[{l}]", ref32=f32[0][l])
                assert_close(ys[l], f64[1][l], what=f"{what} {arm} ys[{l}]", ref32=f32[1][l])
            _, y0 = run_forward(g, dev, case, save=0, shifted=shifted)
            assert_bit_exact(y0, ys[L - 1], f"{what} {arm}: save = 0 against the last slab of save = 1")
        if True in runs:
            assert_bit_exact(runs[True][0], runs[False][0], f"{what}: hs of the two arms")
            assert_bit_exact(runs[True][1], runs[False][1], f"{what}: ys of the two arms")
        assert "recalgo_res_stack_fwd" in g.launched


@pytest.mark.parametrize("B,D,H,L", CASES)
def test_backward_at_the_abi_against_float64(dev, B, D, H, L):
    case, _, _, (hs, ys), b64, b32 = _references(B, D, H, L)
    what = f"B={B} D={D} H={H} L={L}"
    with guarded() as g:
        runs = {}
        for shifted in ((False, True) if D % 4 == 0 else (False,)):
            arm = "4-byte arm" if (shifted or D % 4) else "16-byte arm"
            got = runs[shifted] = run_backward(g, dev, case, hs, ys, shifted=shifted)
            for name, a, r64, r32 in zip(("dzs", "dhs", "dx"), got, b64, b32):
                assert_close(a, r64, what=f"{what} {arm} {name}", ref32=r32)
            dzs, dhs = got[0].cpu(), got[1].cpu()
            # under a zero mask: +0.0 exactly (all bits)
            assert bool((dzs[ys <= 0].view(torch.int32) == 0).all()) and bool((dhs[hs <= 0].view(torch.int32) == 0).all()), what
        if True in runs:
            for name, a, b in zip(("dzs", "dhs", "dx"), runs[True], runs[False]):
                assert_bit_exact(a, b, f"{what}: {name} of the two arms")
        assert "recalgo_res_stack_bwd" in g.launched


# ---- properties ---------------------------------------------------------------------------------------------------------------------
def _rows(case, n):
    return dict(case, x=case["x"][:n], g=case["g"][:n])


def test_two_runs_are_bit_equal_and_rows_do_not_depend_on_the_batch(dev):
    B, D, H, L = 67, 82, 32, 3
    case, _, _, (hs, ys), _, _ = _references(B, D, H, L)
    with guarded() as g:
        a, b = run_forward(g, dev, case), run_forward(g, dev, case)
        for name, x, y in zip(("hs", "ys"), a, b):
            assert_bit_exact(x, y, f"two forward runs: {name}")
        ba, bb = run_backward(g, dev, case, hs, ys), run_backward(g, dev, case, hs, ys)
        for name, x, y in zip(("dzs", "dhs", "dx"), ba, bb):
            assert_bit_exact(x, y, f"two backward runs: {name}")
        # rows 0..15 of the B = 67 run against a B = 16 run on those rows
        small = run_forward(g, dev, _rows(case, 16))
        assert_bit_exact(small[0], a[0][:, :16], "hs of rows 0..15")
        assert_bit_exact(small[1], a[1][:, :16], "ys of rows 0..15")
        sb = run_backward(g, dev, _rows(case, 16), hs[:, :16], ys[:, :16])
        assert_bit_exact(sb[0], ba[0][:, :16], "dzs of rows 0..15")
        assert_bit_exact(sb[1], ba[1][:, :16], "dhs of rows 0..15")
        assert_bit_exact(sb[2], ba[2][:16], "dx of rows 0..15")


def test_a_stack_of_three_is_three_one_unit_calls(dev):
    B, D, H, L = 67, 82, 32, 3
    case, _, _, (hs, ys), _, _ = _references(B, D, H, L)
    unit = lambda l, **kw: dict({k: ([v[l]] if isinstance(v, list) else v) for k, v in case.items()}, **kw)    # noqa: E731
    with guarded() as g:
        fh, fy = run_forward(g, dev, case)
        x = case["x"]
        for l in range(L):
            h1, y1 = run_forward(g, dev, unit(l, x=x))
            assert_bit_exact(h1[0], fh[l], f"forward: hs[{l}]")
            assert_bit_exact(y1[0], fy[l], f"forward: ys[{l}]")
            x = y1[0].cpu()
        dzs, dhs, dx = run_backward(g, dev, case, hs, ys)
        grad = case["g"]
        for l in range(L - 1, -1, -1):
            dz1, dh1, dx1 = run_backward(g, dev, unit(l, g=grad), hs[l:l + 1], ys[l:l + 1])
            assert_bit_exact(dz1[0], dzs[l], f"backward: dzs[{l}]")
            assert_bit_exact(dh1[0], dhs[l], f"backward: dhs[{l}]")
            grad = dx1.cpu()
        assert_bit_exact(dx1, dx, "backward: dx")


@pytest.mark.parametrize("B,D,H", [(67, 82, 128), (17, 96, 48)])
def test_zero_second_layer_gives_relu_of_the_input(dev, B, D, H):
    case = R.random_stack(B, D, H, 1, seed=5)
    case["w1"], case["b1"] = [torch.zeros(H, D, dtype=torch.float64)], [torch.zeros(D, dtype=torch.float64)]
    with guarded() as g:
        _, ys = run_forward(g, dev, case)
        assert_bit_exact(ys[0], torch.relu(case["x"].float()), "y = relu(x)")


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks_refuse_before_any_launch(dev):
    B, D, H, L = 17, 82, 32, 3
    case, _, _, (hs_h, ys_h), _, _ = _references(B, D, H, L)
    with guarded() as g:
        lib = _lib.load()
        x, gi, hsd, ysd = (g.input(t.float(), dev) for t in (case["x"], case["g"], hs_h, ys_h))
        w = {k: [g.input(t.float(), dev) for t in case[k]] for k in ("w0", "b0", "w1", "b1")}
        tabs = [_table(w[k]) for k in ("w0", "b0", "w1", "b1")]
        hs, ys = torch.empty(L, B, 512, device=dev), torch.empty(L, B, 513, device=dev)
        dzs, dhs, dx = torch.empty(L, B, 513, device=dev), torch.empty(L, B, 512, device=dev), torch.empty(B, 513, device=dev)
        off2 = lambda t: ctypes.c_void_p(t.data_ptr() + 2)                  # noqa: E731
        null_entry = (ctypes.c_void_p * L)(w["w0"][0].data_ptr(), None, w["w0"][2].data_ptr())
        odd_entry = (ctypes.c_void_p * L)(w["w1"][0].data_ptr(), w["w1"][1].data_ptr() + 2, w["w1"][2].data_ptr())

        def refused(fn, *a):
            with pytest.raises(_lib.RecalgoError, match="failed with hipError_t=1$"):
                fn(*a, _stream())
        fwd, bwd = lib.recalgo_res_stack_fwd, lib.recalgo_res_stack_bwd
        for D_, H_, L_ in ((0, H, L), (513, H, L), (D, 0, L), (D, 8, L), (D, 40, L), (D, 272, L), (D, H, 0), (D, H, 9)):
            refused(fwd, _ptr(x), *tabs, B, D_, H_, L_, 1, _ptr(hs), _ptr(ys))
            refused(bwd, _ptr(gi), _ptr(hsd), _ptr(ysd), tabs[0], tabs[2], B, D_, H_, L_, _ptr(dzs), _ptr(dhs), _ptr(dx))
        refused(fwd, _ptr(x), *tabs, 0, D, H, L, 1, _ptr(hs), _ptr(ys))
        refused(fwd, None, *tabs, B, D, H, L, 1, _ptr(hs), _ptr(ys))
        refused(fwd, _ptr(x), *tabs, B, D, H, L, 1, _ptr(hs), None)
        refused(fwd, _ptr(x), *tabs, B, D, H, L, 1, None, _ptr(ys))                     # save != 0 without hs
        refused(fwd, off2(x), *tabs, B, D, H, L, 1, _ptr(hs), _ptr(ys))
        refused(fwd, _ptr(x), *tabs, B, D, H, L, 1, off2(hs), _ptr(ys))
        refused(fwd, _ptr(x), *tabs, B, D, H, L, 0, None, off2(ys))
        for i in range(4):
            refused(fwd, _ptr(x), *tabs[:i], None, *tabs[i + 1:], B, D, H, L, 1, _ptr(hs), _ptr(ys))
        refused(fwd, _ptr(x), null_entry, *tabs[1:], B, D, H, L, 1, _ptr(hs), _ptr(ys))
        refused(fwd, _ptr(x), *tabs[:2], odd_entry, tabs[3], B, D, H, L, 1, _ptr(hs), _ptr(ys))
        good = [_ptr(gi), _ptr(hsd), _ptr(ysd), tabs[0], tabs[2], B, D, H, L, _ptr(dzs), _ptr(dhs), _ptr(dx)]
        for i in (0, 1, 2, 3, 4, 9, 10, 11):
            refused(bwd, *good[:i], None, *good[i + 1:])
        refused(bwd, *good[:8], 0, *good[9:])
        refused(bwd, *good[:5], 0, *good[6:])
        refused(bwd, off2(gi), *good[1:])
        refused(bwd, *good[:11], off2(dx))
        refused(bwd, *good[:3], null_entry, *good[4:])
        refused(bwd, *good[:4], odd_entry, *good[5:])
        torch.cuda.synchronize()
        for name, t in (("hs", hs), ("ys", ys), ("dzs", dzs), ("dhs", dhs), ("dx", dx)):
            assert bool(torch.isnan(t).all()), f"a refused call wrote {name}"
        assert not {"recalgo_res_stack_fwd", "recalgo_res_stack_bwd"} & g.launched
    x = torch.zeros(4, 82, device=dev)
    from recalgorithm_amd.variables import Variable
    V = lambda *s: [Variable("v", torch.zeros(*s, device=dev))]              # noqa: E731
    with pytest.raises(ValueError, match="the kernels serve"):
        ops.residual_stack(x, V(82, 40), V(40), V(40, 82), V(82))
    with pytest.raises(ValueError, match="W1 has shape"):
        ops.residual_stack(x, V(82, 32), V(32), V(32, 81), V(82))


# ---- the autograd op ----------------------------------------------------------------------------------------------------------------
def _op_run(dev, case, fused, in_step):
    """nn.residual_stack on a store of its own holding the case's parameters -> {y, dx, d<param>_<l>} after flush_dense_splits"""
    from recalgorithm_amd import nn
    from recalgorithm_amd.variables import VariableStore, use_store
    B, D = case["x"].shape
    L, H = len(case["w0"]), case["w0"][0].shape[1]
    store = VariableStore(dev, seed=3)
    with use_store(store):
        store.building = True
        nn.residual_stack(torch.zeros(B, D, device=dev), H, L, fused=fused)    # registration: the variables, no launch
        store.finalize()
        names = {"w0": "dense_{}_0/kernel", "b0": "dense_{}_0/bias", "w1": "dense_{}_1/kernel", "b1": "dense_{}_1/bias"}
        for k, pat in names.items():
            for l in range(L):
                store.vars[pat.format(l)].data.copy_(case[k][l].float())
        x = case["x"].float().to(dev).requires_grad_(True)
        with ops.loss_seed(1.0) if in_step else torch.enable_grad():
            store.begin_call()
            y = nn.residual_stack(x, H, L, fused=fused)
            (y * case["g"].float().to(dev)).sum().backward()
        ops.flush_dense_splits()
        with torch.no_grad():
            y0 = nn.residual_stack(x.detach(), H, L, fused=fused)         # grad mode off: save = 0
        out = {"y": y.detach(), "y no_grad": y0, "dx": x.grad}
        for k, pat in names.items():
            for l in range(L):
                out[f"d{k}_{l}"] = store.vars[pat.format(l)].grad.clone()
        return out


def _op_reference(case, dtype):
    c = R.cast(case, dtype)
    leaves = {k: [t.clone().requires_grad_(True) for t in c[k]] for k in ("w0", "b0", "w1", "b1")}
    x = c["x"].clone().requires_grad_(True)
    y = R.stack_forward(x, leaves["w0"], leaves["b0"], leaves["w1"], leaves["b1"])[1][-1]
    (y * c["g"]).sum().backward()
    out = {"y": y.detach(), "y no_grad": y.detach(), "dx": x.grad}
    out.update({f"d{k}_{l}": t.grad for k, ts in leaves.items() for l, t in enumerate(ts)})
    return out


# fused: None = nn.residual_stack's own choice (fused at D = 82 where the kernels serve H, composed at H = 40 and at D = 432)
@pytest.mark.parametrize("B,D,H,L,fused", [(67, 82, 32, 2, None), (67, 82, 40, 2, None), (67, 82, 32, 2, False), (67, 432, 32, 2, None),
                                           (67, 432, 32, 2, True)])
@pytest.mark.parametrize("in_step", [False, True])
def test_autograd_op_against_float64(dev, B, D, H, L, fused, in_step):
    from recalgorithm_amd import nn
    assert ops.residual_supported(D, H, L) == (H % 16 == 0)
    assert nn.residual_fused_default(D, H, L) == (H % 16 == 0 and D == 82)
    case = R.random_stack(B, D, H, L, seed=77 + H + D)
    r64, r32 = _op_reference(case, torch.float64), _op_reference(case, torch.float32)
    with guarded() as g:
        got = _op_run(dev, case, fused=fused, in_step=in_step)
        ran = {"recalgo_res_stack_fwd", "recalgo_res_stack_bwd"} & g.launched
        fused = nn.residual_fused_default(D, H, L) if fused is None else fused
        assert ran == ({"recalgo_res_stack_fwd", "recalgo_res_stack_bwd"} if fused else set()), ran
    assert sorted(got) == sorted(r64) and len(got) == 3 + 4 * L
    for k in r64:
        assert_close(got[k], r64[k], what=f"nn.residual_stack H={H} fused={fused} in_step={in_step} {k}", ref32=r32[k],
                     reduced=k.startswith("d") and k != "dx")
    if fused:                                # where both paths serve the shape they agree
        other = _op_run(dev, case, fused=False, in_step=in_step)
        for k in r64:
            scale = float(r64[k].abs().max())
            assert float((got[k].double() - other[k].double()).abs().max()) <= 2e-5 * scale, k
        assert_bit_exact(got["y"], got["y no_grad"], "save = 1 and save = 0")


# ---- the model ------------------------------------------------------------------------------------------------------------------
from recalgorithm_amd import feature_column as fc  # noqa: E402
from recalgorithm_amd.estimator import HOUSEKEEPING_EVERY, Estimator, GraphedTrainStep, RunConfig, _tree_tensors  # noqa: E402
from recalgorithm_amd.io import synth  # noqa: E402
from tests import golden_util as GU  # noqa: E402
from tests import trajectory_ref as T  # noqa: E402
from tests.golden_protocol import check_on_device  # noqa: E402
from tests.test_deepcrossing_host import CASE, GOLDENS, mirror_setup  # noqa: E402
from tests.test_gpu_replay_models import _differences, _state  # noqa: E402
from tests.test_mmoe_host import encode  # noqa: E402


@pytest.mark.parametrize("name", list(GOLDENS))
def test_model_golden(dev, name, tmp_path):
    """Both goldens through the mirrored deepcrossing_model_fn as it ships (at the reference's D = 82 the residual stack runs
    on the fused kernels): variable names, PREDICT (logit and probabilities), loss, every gradient, the Adam step, EVAL."""
    from recalgorithm_amd import nn
    assert all(nn.residual_fused_default(82, H, L) for L, H in ((1, 128), (3, 32)))
    check_on_device(dev, CASE, name, tmp_path)


def test_forcing_a_path_the_kernels_do_not_serve_is_refused(dev):
    from recalgorithm_amd import nn
    from recalgorithm_amd.variables import VariableStore, use_store
    with use_store(VariableStore(dev, seed=3)):
        with pytest.raises(ValueError, match="do not serve"):
            nn.residual_stack(torch.zeros(4, 82, device=dev), 40, 1, fused=True)


EMB = (16, 2, 4, 4, 4, 4, 16, 16)           # the reference's embedding widths (deepcrossing.py:94-100)


def make_deepcrossing(dev, fused, B=256, units=2, internal_dim=128, max_vocab=500, seed=42):
    """A DeepCrossing estimator over synthetic device-resident features: the 16 dense features and 8 id columns of the
    reference's widths, D = 82; `fused`: params["fused_residual"]."""
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    from recalgorithm_amd.algorithm.DeepCrossing.deepcrossing import deepcrossing_model_fn
    spec = synth.SynthSpec(n_fields=len(EMB), max_vocab=max_vocab, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES],
              "category_feature_columns": [fc.embedding_column(c, e) for c, e in zip(cats, EMB)],
              "residual_internal_dim": internal_dim, "residual_network_num": units, "learning_rate": 0.005, "fused_residual": fused}
    est = Estimator(model_fn=deepcrossing_model_fn, params=params, config=RunConfig(device=dev, seed=seed))
    feats, labels, _ = synth.device_features(spec, B, dev, batch_index=0)
    est.build(feats, labels)
    return est, spec


WARMUP, STEPS, N_BATCHES = 3, 40, 5


@pytest.mark.parametrize("fused", [None, False], ids=["as shipped (fused)", "composed"])
def test_captured_step_replays_what_eager_steps_compute(dev, fused):
    """40 hipGraph replays of the captured step (B 256, 2 units) against eager launches on rotating batches, bit for bit
    (tests/test_gpu_replay_models.py's comparison), as the model ships and with the composed layers forced."""
    assert STEPS > HOUSEKEEPING_EVERY
    (eager, spec), (graphed, _) = make_deepcrossing(dev, fused), make_deepcrossing(dev, fused)
    batches = [synth.device_features(spec, 256, dev, batch_index=i)[:2] for i in range(N_BATCHES)]
    keep = [[t.clone() for _, t in _tree_tensors({"f": b[0], "l": b[1]}, "b")] for b in batches]
    for _ in range(WARMUP):
        eager.train_step(*batches[0])
    le = []
    for i in range(STEPS):
        le.append(eager.train_step(*batches[i % N_BATCHES]).clone())
        if (i + 1) % HOUSEKEEPING_EVERY == 0:
            eager.store.housekeeping()
    first = _state(eager, le)
    assert int(first["step counter"]) == WARMUP + STEPS and all(torch.isfinite(l).all() for l in le)
    assert float(le[-1]) != float(le[0])
    g = GraphedTrainStep(graphed.train_step, *batches[0], warmup=WARMUP)
    lg = [g(*batches[i % N_BATCHES]).clone() for i in range(STEPS)]
    diff = _differences(first, _state(graphed, lg))
    assert not diff, f"{STEPS} replays of the captured step differ from eager launches in {diff[:8]} ({len(diff)} in all)"
    assert all(torch.equal(t, k) for b, kept in zip(batches, keep) for (_, t), k in zip(_tree_tensors({"f": b[0], "l": b[1]}, "b"), kept))


N_TRAJECTORY = 3


def _oracle_trajectory(params, start, batches, lr, dtype):
    """N_TRAJECTORY free-running steps of the oracle (tests/trajectory_ref.run_oracle's record, for R.deepcrossing)"""
    from oracle import ref_ops as O
    P = {k: v.clone().to(dtype) for k, v in start.items()}
    m, v_ = {k: torch.zeros_like(v) for k, v in P.items()}, {k: torch.zeros_like(v) for k, v in P.items()}
    out = {"loss": [], "grad": [], "v": []}
    for k, b in enumerate(T.ORDER[:N_TRAJECTORY], start=1):
        for p in P.values():
            p.grad = None
            p.requires_grad_(True)
        sf, labels = batches[b]
        feats = {n: (t.to(dtype) if isinstance(t, torch.Tensor) and t.is_floating_point() else t) for n, t in encode(params, sf).items()}
        res = R.deepcrossing(P, feats, {"read_comment": labels.to(dtype)}, params, training=True)
        res["loss"].backward()
        grads = {n: p.grad.detach().clone() for n, p in P.items() if p.grad is not None}
        with torch.no_grad():
            for n, gr in grads.items():
                O.adam_tf1_step(P[n], gr, m[n], v_[n], k, lr)
        out["loss"].append(res["loss"].detach().clone())
        out["grad"].append(grads)
        out["v"].append({n: v_[n].clone() for n in grads})
    out["final"] = {n: p.detach().clone() for n, p in P.items()}
    out["trainable"] = sorted({n for gr in out["grad"] for n in gr})
    return out


def test_three_steps_follow_the_fp64_oracle(dev, tmp_path):
    """3 eager Estimator.train_step calls of the model as it ships on rotating sub-batches of the golden batch (three units) against the float64
    oracle's own free-running trajectory, inside tests/trajectory_ref.bounds (float64 quantities only); the float32 oracle
    itself must sit below half of that bound for the test to be one of the kernels."""
    name = "model_deepcrossing_three_units"
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup(name, vocab_dir)
    d = GU.load(name)
    lr = float(d["meta/learning_rate"])
    sfeats, labels = GU.string_batch()
    batches = [T.cut(sfeats, labels, idx) for idx in T.batch_indices()]
    start = {k: torch.from_numpy(v.copy()).float().double() for k, v in GU.section(d, "var/").items()}
    r64, r32 = (_oracle_trajectory(params, start, batches, lr, dt) for dt in (torch.float64, torch.float32))
    bnd = T.bounds(r64, lr)
    w32, where32, out32 = T.worst_ratio(r32["final"], r64, bnd)
    assert w32 <= 0.5, f"the fp32 reference alone uses {w32:.3f} of the bound at {where32}"

    est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, use_hip_graph=False))
    host = [({k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sf.items()}, {"read_comment": lb.float()})
            for sf, lb in batches]
    est.build(*host[0])
    dev_batches = [est._to_device(f, l) for f, l in host]
    arrays = est.store.named_arrays()
    assert sorted(arrays) == sorted(start)
    for k, v in start.items():
        arrays[k].copy_(v.float().reshape(arrays[k].shape))
    losses = [est.train_step(*dev_batches[b]).clone() for b in T.ORDER[:N_TRAJECTORY]]
    torch.cuda.synchronize()
    for k, (l, l64, l32) in enumerate(zip(losses, r64["loss"], r32["loss"]), start=1):
        print(f"{name} step {k}: loss {float(l):.9g} fp64 oracle {float(l64):.9g} fp32 oracle {float(l32):.9g}")
        assert_close(l, l64, what=f"{name} loss of step {k}", ref32=l32)
    assert int(est.store.opt_state["step"]) == N_TRAJECTORY
    after = est.store.named_arrays()
    assert len(r64["trainable"]) == GOLDENS[name]
    wk, wherek, outk = T.worst_ratio({k: after[k] for k in r64["trainable"]}, r64, bnd)
    print(f"{name}: worst |p - p64| / tol after {N_TRAJECTORY} steps: kernels {wk:.3f} ({wherek}) | fp32 oracle {w32:.3f} ({where32})")
    assert wk <= 1.0, f"{name}: {wherek} is {wk:.3f} x the bound after {N_TRAJECTORY} steps (fp32 oracle: {w32:.3f} at {where32})"
    for k in outk:
        assert outk[k] <= 1.5 * out32[k] + 10, f"{name} {k}: {outk[k]} elements outside the tight bound, the fp32 oracle leaves {out32[k]}"
    assert not bool(est.store.flat_grad.any()), "flat_grad is not zero after the step"
