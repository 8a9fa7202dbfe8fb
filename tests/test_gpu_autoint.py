"""-m gpu: AutoInt's interacting layer (csrc/autoint.hip, include/recalgo_autoint.h) behind ops.autoint_layer and
nn.interacting_layer, and the model (algorithm/AutoInt/autoint.py): parity with tests/autoint_ref.py at every shape the kernels
change path, large scores, a dead ReLU, row independence, the partial rows at the C ABI under guarded allocations, the refusals,
run to run and under torch.cuda.graph, a stack against single calls, the model against the float64 restatement (PREDICT, loss,
every gradient, one Adam step, the launches counted), captured training with single-valued columns and with the bag under
ragged_capacity, a three-step trajectory, evaluate on the device metrics path and serving from an export."""
import ctypes

import pytest
import torch

from recalgorithm_amd import _lib, nn, ops
from recalgorithm_amd.variables import VariableStore, use_store
from tests import autoint_ref as R
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu
ENTRIES = ("recalgo_autoint_layer_fwd", "recalgo_autoint_layer_bwd")
MID = (67, 9, 16, 8, 2, True)


def _dev(x, dev):
    return {k: (None if v is None else v.to(dev).contiguous()) for k, v in x.items()}


def run_op(dev, x, grad=True):
    """ops.autoint_layer on plain tensors, forward + backward -> {y, dx, dwq, dwk, dwv[, dwres]} in the reference's shapes"""
    t = _dev(x, dev)
    B, F, D = x["x"].shape
    xs = t["x"].reshape(B, F * D).requires_grad_(grad)
    ws = [None if t[k] is None else t[k].requires_grad_(grad) for k in ("wq", "wk", "wv", "wres")]
    if not grad:
        with torch.no_grad():
            return {"y": ops.autoint_layer(xs, F, *ws).reshape(B, F, -1)}
    y = ops.autoint_layer(xs, F, *ws)
    y.backward(t["g"].reshape(B, -1))
    out = {"y": y.detach().reshape(B, F, -1), "dx": xs.grad.reshape(B, F, D), "dwq": ws[0].grad, "dwk": ws[1].grad, "dwv": ws[2].grad}
    if ws[3] is not None:
        out["dwres"] = ws[3].grad
    return out


def _count(monkeypatch, names=ENTRIES):
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


@pytest.mark.parametrize("B,F,D,A,H,res", R.SHAPES)
def test_parity(dev, B, F, D, A, H, res):
    x, r64, r32 = R.case(B, F, D, A, H, res)
    got = run_op(dev, x)
    assert sorted(got) == sorted(R.names_of(x))
    for k in R.names_of(x):
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        assert_close(got[k], r64[k], what=f"ops.autoint_layer B={B} F={F} D={D} A={A} H={H} res={res} {k}", reduced=k in R.REDUCED,
                     ref32=r32[k])
    assert_bit_exact(run_op(dev, x, grad=False)["y"], got["y"], "the forward with grad disabled")


@pytest.mark.parametrize("B,F,D,A,H", [(4200, 3, 4, 4, 1), (2100, 7, 16, 8, 2)])
def test_more_examples_than_the_grid_has_waves(dev, B, F, D, A, H):
    """The forward's grid is at most 1024 workgroups and the backward's 512, of four waves here: past 4096 and 2048 examples a
    wave serves a second and a third one over the same LDS, and its weight gradients accumulate over them."""
    rows = int(_lib.load().recalgo_autoint_bwd_partial_rows(B, F, D, A, H))
    assert rows == 512 and B > 4 * rows
    x, r64, r32 = R.case(B, F, D, A, H, True)
    got = run_op(dev, x)
    for k in R.names_of(x):
        assert_close(got[k], r64[k], what=f"ops.autoint_layer B={B} F={F} D={D} A={A} H={H} {k}", reduced=k in R.REDUCED, ref32=r32[k])


def test_large_scores(dev):
    """x, Wq and Wk scaled by 3 at (67, 9, 16, 8, 2): scores of +-1600, where exp() of an unshifted score overflows.  Every output
    is finite and parity holds with the floor of afm_ref.fp32_floor: 4 x the float32 restatement's own deviation (it leaves 312
    elements of dx outside the plain bound itself)."""
    from tests.afm_ref import fp32_floor
    x, r64, r32 = R.case(**R.LARGE)
    assert float(r64["s"].max()) > 1000 and float(r64["s"].min()) < -1000
    got = run_op(dev, x)
    for k in R.names_of(x):
        assert bool(torch.isfinite(got[k]).all()), k
        assert_close(got[k], r64[k], what=f"ops.autoint_layer, large scores: {k}", reduced=k in R.REDUCED, ref32=r32[k],
                     floor=fp32_floor(r64, r32, k))


def test_a_dead_relu_gives_exact_zeros(dev):
    """x >= 0, Wv <= 0, no residual term: every P V is <= 0, so y is exactly 0 and every gradient is exactly 0"""
    x = dict(R.inputs(33, 9, 16, 8, 2, res=False, seed=5))
    x["x"], x["wv"] = x["x"].abs(), -x["wv"].abs()
    got = run_op(dev, x)
    assert sorted(got) == ["dwk", "dwq", "dwv", "dx", "y"]
    for k, v in got.items():
        assert bool((v == 0).all()), k


def _rows_of(x, rows):
    return dict(x, x=x["x"][rows].clone(), g=x["g"][rows].clone())


def test_a_row_depends_on_that_row_alone(dev):
    x, _, _ = R.case(*MID)
    whole = run_op(dev, x)
    for r in (0, 31, 66):
        alone = run_op(dev, _rows_of(x, [r]))
        five = run_op(dev, _rows_of(x, [1, 2, 5, r, 7]))
        for k in ("y", "dx"):
            assert_bit_exact(alone[k][0], whole[k][r], f"row {r} alone, {k}")
            assert_bit_exact(five[k][3], whole[k][r], f"row {r} as the fourth of five, {k}")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("B,F,D,A,H,res", [(1, 2, 4, 4, 1, True), (33, 26, 16, 8, 2, True), (33, 26, 16, 8, 2, False)])
def test_the_outputs_are_the_fixed_order_sums_of_the_partial_rows(dev, B, F, D, A, H, res):
    """At the C ABI on buffers of exactly the documented sizes, under the guard: the dW are tests/dense_ref.colsum_fixed_order of
    the workspace's rows [dWq | dWk | dWv | dWres], bit for bit; the workspace is exactly as large as the query says; no store
    lands outside any buffer."""
    from tests.redzone import guarded
    from tests.test_gpu_colsums import _assert_outputs_are_the_sums, _workspace_of
    x, r64, r32 = R.case(B, F, D, A, H, res)
    width = (4 if res else 3) * H * D * A
    with guarded() as g:
        lib = _lib.load()
        rows = int(lib.recalgo_autoint_bwd_partial_rows(B, F, D, A, H))
        nbytes = int(lib.recalgo_autoint_bwd_workspace_bytes(B, F, D, A, H, int(res)))
        assert rows == -(-B // 4) and nbytes == rows * width * 4
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        t = _dev(x, dev)
        y = torch.empty(B, F * H * A, device=dev)
        lib.recalgo_autoint_layer_fwd(_p(t["x"]), _p(t["wq"]), _p(t["wk"]), _p(t["wv"]), _p(t["wres"]), B, F, D, A, H, _p(y), st)
        grads = {"dwq": torch.empty(H, D, A, device=dev), "dwk": torch.empty(H, D, A, device=dev), "dwv": torch.empty(H, D, A, device=dev)}
        if res:
            grads["dwres"] = torch.empty(D, H * A, device=dev)
        dx = torch.empty(B, F * D, device=dev)
        ws = ops._workspace(nbytes, torch.device(dev))
        lib.recalgo_autoint_layer_bwd(_p(t["g"]), _p(t["x"]), _p(y), _p(t["wq"]), _p(t["wk"]), _p(t["wv"]), _p(t["wres"]), B, F, D, A, H,
                                      _p(dx), _p(grads["dwq"]), _p(grads["dwk"]), _p(grads["dwv"]), _p(grads.get("dwres")), _p(ws), st)
        wsf = _workspace_of(g)
        assert wsf.numel() == max(rows * width, 4)
        _assert_outputs_are_the_sums(wsf, rows, grads, f"autoint_layer_bwd B={B} F={F} D={D} A={A} H={H} res={res}")
        assert set(ENTRIES) <= g.launched
        got = dict(grads, y=y.reshape(B, F, -1), dx=dx.reshape(B, F, D))
        for k in R.names_of(x):
            assert_close(got[k], r64[k], what=f"the C entries B={B} F={F} D={D} A={A} H={H} res={res} {k}", reduced=k in R.REDUCED,
                         ref32=r32[k])


@pytest.mark.parametrize("F,D,A,H", [(1, 8, 8, 2), (65, 8, 8, 2), (7, 68, 8, 2), (7, 6, 8, 2), (7, 8, 36, 1), (7, 8, 6, 2), (7, 8, 8, 5),
                                     (7, 8, 32, 3)])
def test_shapes_outside_the_domain_are_refused(dev, F, D, A, H, monkeypatch):
    calls = _count(monkeypatch)
    z = lambda *s: torch.zeros(*s, device=dev)               # noqa: E731
    with pytest.raises(ValueError, match="the kernels serve"):
        ops.autoint_layer(z(4, F * D), F, z(H, D, A), z(H, D, A), z(H, D, A), z(D, H * A))
    with pytest.raises(ValueError, match="x must be a non-empty"):
        ops.autoint_layer(z(0, 56), 7, z(2, 8, 8), z(2, 8, 8), z(2, 8, 8))
    with pytest.raises(ValueError, match="wv must be a contiguous float32 tensor on x's device"):
        ops.autoint_layer(z(4, 56), 7, z(2, 8, 8), z(2, 8, 8), torch.zeros(2, 8, 8))
    assert calls == {n: 0 for n in ENTRIES}


def test_two_runs_and_three_replays_give_the_same_bits(dev):
    """forward + backward: eagerly twice, once on a side stream (the warm-up a capture needs), captured and replayed three times"""
    x, _, _ = R.case(*MID)
    t = _dev(x, dev)
    B, F, D = x["x"].shape
    xs = t["x"].reshape(B, F * D).requires_grad_(True)
    ws = [t[k].requires_grad_(True) for k in ("wq", "wk", "wv", "wres")]
    g = t["g"].reshape(B, -1)

    def run():
        y = ops.autoint_layer(xs, F, *ws)
        return [y.detach()] + list(torch.autograd.grad(y, [xs] + ws, g))
    first = [o.clone() for o in run()]
    for name, u, w_ in zip(R.NAMES, run(), first):
        assert_bit_exact(u, w_, f"second eager run, {name}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for i in range(3):
        for c in captured:
            c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, u, w_ in zip(R.NAMES, captured, first):
            assert_bit_exact(u, w_, f"replay {i}, {name}")


def test_three_layers_are_three_single_calls(dev):
    """nn.interacting_layer three times on a store of its own against three ops.autoint_layer calls on the same values: y, dx
    and every variable's gradient bit for bit; D = 8 into the first layer, H A = 16 from then on"""
    B, F, K, A, H, L = 33, 7, 8, 8, 2, 3
    store = VariableStore(dev, seed=3)
    with use_store(store):
        store.building = True
        out = torch.zeros(B, F * K, device=dev)
        for i in range(L):
            out = nn.interacting_layer(out, F, A, H, True, i)
        assert tuple(out.shape) == (B, F * H * A) and not bool(out.any())
        store.finalize()
    names = [[f"interacting_layer_{i}_w_{n}" for n in ("query", "key", "value", "res")] for i in range(L)]
    assert sorted(store.vars) == sorted(n for ns in names for n in ns)
    assert tuple(store.vars[names[0][0]].data.shape) == (H, K, A) and tuple(store.vars[names[1][3]].data.shape) == (H * A, H * A)
    gen = torch.Generator().manual_seed(11)
    x0 = torch.randn(B, F * K, generator=gen).to(dev)
    g = torch.randn(B, F * H * A, generator=gen).to(dev)
    x = x0.clone().requires_grad_(True)
    with use_store(store):
        store.begin_call()
        y = x
        for i in range(L):
            y = nn.interacting_layer(y, F, A, H, True, i)
        y.backward(g)
        ops.flush_dense_splits()
    plain = [[store.vars[n].data.clone().requires_grad_(True) for n in ns] for ns in names]
    x2 = x0.clone().requires_grad_(True)
    y2 = x2
    for ws in plain:
        y2 = ops.autoint_layer(y2, F, *ws)
    y2.backward(g)
    assert_bit_exact(y, y2, "y of the stack")
    assert_bit_exact(x.grad, x2.grad, "dx of the stack")
    for ns, ws in zip(names, plain):
        for n, w in zip(ns, ws):
            assert_bit_exact(store.vars[n].grad, w.grad, f"d({n})")
    assert float(y.detach().abs().max()) > 0 and float(x.grad.abs().max()) > 0


# ---- the model ---------------------------------------------------------------------------------------------------------------------
from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig  # noqa: E402
from tests import golden_util as GU  # noqa: E402
from tests.test_autoint_host import autoint_setup  # noqa: E402
from tests.test_mmoe_host import encode  # noqa: E402

L_DEFAULT = 3


def _redraw(est, seed=16):
    """The interacting weights as N(0, 1) / sqrt(D), the distribution of autoint_ref.inputs, over tables of order 1: the softmax
    is not flat (glorot-uniform over the default tables leaves scores of order 0.01; here they reach +-16 and a row's largest
    weight averages 0.57, 0.37 and 0.22 in the three layers against 1/7 = 0.14).  Not wider: at 1.5 / sqrt(D) the scores of the
    third layer reach +-138, the regime test_large_scores judges by its floor, where the float32 restatement itself leaves up to
    a quarter of a gradient's elements outside the strict bound.  The logit kernels larger; BatchNorm's moving statistics stay."""
    arrays = est.store.named_arrays()
    gen = torch.Generator().manual_seed(seed)
    for k, v in arrays.items():
        if "interacting_layer_" in k:
            v.copy_(torch.randn(*v.shape, generator=gen) / v.shape[-2] ** 0.5)
        elif k.endswith("/embedding_weights"):
            v.copy_(torch.randn(*v.shape, generator=gen))
        elif k.endswith("_logit/kernel"):
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.3)
    return arrays


def _on_device(dev, tmp_path, **flags):
    """-> (estimator, params, device features, device labels) of the model on the 48 rows of the shared string batch"""
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = autoint_setup(vocab_dir, **flags)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, use_hip_graph=False))
    est.build(feats, lab)
    return est, params, *est._to_device(feats, lab)


def _oracle(params, variables, dtype, train=True):
    sfeats, labels = GU.string_batch()
    P = {k: v.clone().to(dtype).requires_grad_(not k.split("/")[-1].startswith("moving_")) for k, v in variables.items()}
    feats = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in encode(params, sfeats).items()}
    with torch.no_grad():
        predict = R.autoint(P, feats, None, params, training=False)
    out = R.autoint(P, feats, {"read_comment": labels.to(dtype)}, params, training=True)
    out["loss"].backward()
    return {"predict": predict, "loss": out["loss"].detach(), "P": P}


@pytest.mark.parametrize("hidden", ["", "32,16"], ids=["AutoInt", "AutoInt+ 32,16"])
def test_the_model_follows_the_fp64_restatement(dev, hidden, tmp_path, monkeypatch):
    """The dataset's columns (F = 7, embedding_dim 8), 3 layers of 2 heads of 8, with and without the deep part: PREDICT, the
    TRAIN loss, every gradient and one Adam step against tests/autoint_ref.autoint in float64, with the floor of the float32
    restatement's own deviation (golden_protocol.judge_step_against_oracle).  A TRAIN step launches each entry once per layer,
    PREDICT the forward once per layer."""
    from tests.golden_protocol import judge_step_against_oracle
    est, params, feats, lab = _on_device(dev, tmp_path, hidden_units=hidden)
    arrays = _redraw(est)
    variables = {k: v.detach().cpu().double() for k, v in arrays.items()}
    before = {k: v.clone() for k, v in variables.items()}
    r64, r32 = _oracle(params, variables, torch.float64), _oracle(params, variables, torch.float32)
    p = r64["predict"]["prob"]
    assert float(p.max() - p.min()) > 0.05, "the redrawn variables tell the rows apart"
    calls = _count(monkeypatch)
    pr = est._call_model_fn(feats, None, ModeKeys.PREDICT)
    assert calls == {ENTRIES[0]: L_DEFAULT, ENTRIES[1]: 0}
    what = f"autoint hidden_units={hidden!r}"
    assert list(pr.predictions) == ["logit", "probabilities"]
    assert_close(pr.predictions["probabilities"], r64["predict"]["prob"], what=f"{what} predict", ref32=r32["predict"]["prob"])
    assert_close(pr.predictions["logit"], r64["predict"]["logit"], what=f"{what} logit", ref32=r32["predict"]["logit"])
    spec = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
    assert_close(spec.loss, r64["loss"], what=f"{what} loss", ref32=r32["loss"])
    n_min = 7 + 2 + 4 * L_DEFAULT + 2 + (0 if not hidden else 2 * (2 + 2) + 2)       # tables, dense_logit, layers, autoint_logit, deep
    judge_step_against_oracle(est, spec, r64["P"], r32["P"], before, params["learning_rate"], what, n_min)
    assert calls == {ENTRIES[0]: 2 * L_DEFAULT, ENTRIES[1]: L_DEFAULT}


# ---- captured training ---------------------------------------------------------------------------------------------------------------
def _synthetic(dev, B=256, fields=8, K=8, seed=42, **run):
    """the model over synthetic device-resident features: 16 dense features and `fields` single-valued id columns"""
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    from recalgorithm_amd.algorithm.AutoInt.autoint import autoint_model_fn
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=fields, max_vocab=500, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES],
              "category_feature_columns": [fc.embedding_column(c, K) for c in cats], "embedding_dim": K, "att_embedding_size": 8,
              "head_num": 2, "num_interacting_layers": 3, "use_residual": True, "hidden_units": [32, 16], "batch_norm": True,
              "dropout_rate": 0.0, "learning_rate": 0.005}
    est = Estimator(model_fn=autoint_model_fn, params=params, config=RunConfig(device=dev, seed=seed, **run))
    feats, labels, _ = synth.device_features(spec, B, dev, batch_index=0)
    est.build(feats, labels)
    return est, spec


def test_captured_step_replays_what_eager_steps_compute(dev):
    """three hipGraph replays of the captured step (B 256, 8 single-valued columns, AutoInt+) against eager launches on rotating
    batches, bit for bit (tests/test_gpu_replay_models.py's comparison)"""
    from recalgorithm_amd.estimator import GraphedTrainStep, _tree_tensors
    from recalgorithm_amd.io import synth
    from tests.test_gpu_replay_models import _differences, _state
    WARMUP, STEPS, N_BATCHES = 3, 3, 3
    (eager, spec), (graphed, _) = _synthetic(dev), _synthetic(dev)
    batches = [synth.device_features(spec, 256, dev, batch_index=i)[:2] for i in range(N_BATCHES)]
    keep = [[t.clone() for _, t in _tree_tensors({"f": b[0], "l": b[1]}, "b")] for b in batches]
    for _ in range(WARMUP):
        eager.train_step(*batches[0])
    le = [eager.train_step(*batches[i % N_BATCHES]).clone() for i in range(STEPS)]
    first = _state(eager, le)
    assert int(first["step counter"]) == WARMUP + STEPS and all(torch.isfinite(l).all() for l in le)
    assert float(le[-1]) != float(le[0])
    g = GraphedTrainStep(graphed.train_step, *batches[0], warmup=WARMUP)
    lg = [g(*batches[i % N_BATCHES]).clone() for i in range(STEPS)]
    diff = _differences(first, _state(graphed, lg))
    assert not diff, f"{STEPS} replays of the captured step differ from eager launches in {diff[:8]} ({len(diff)} in all)"
    assert all(torch.equal(t, k) for b, kept in zip(batches, keep) for (_, t), k in zip(_tree_tensors({"f": b[0], "l": b[1]}, "b"), kept))


_bag_model = {}


def _bag_batches(tmp_path_factory):
    """(model_fn, params, four host batches of the 48 shared rows: 0 .. 2 with rolled rows and cut bags, 3 the rows themselves)"""
    from tests.test_gpu_ragged import _encoded, _roll_cut
    if not _bag_model:
        vocab_dir = GU.write_vocab_dir(str(tmp_path_factory.mktemp("autoint") / "vocabulary"))
        model_fn, params = autoint_setup(vocab_dir)
        base = _encoded(params)
        _bag_model["m"] = (model_fn, params, [_roll_cut(*base, s, keep) for s, keep in ((5, 3), (11, 2), (17, 4))] + [_roll_cut(*base, 0, 8)])
    return _bag_model["m"]


def test_captured_steps_with_the_bag_are_the_eager_steps(dev, tmp_path_factory):
    """the dataset's columns with the manual_tag_list bag under ragged_capacity, no model-specific code: two eager warm-up steps,
    the capture, three replays — losses and variables bit for bit those of eager steps"""
    from tests.test_gpu_ragged import _assert_same_run, _nnz, _steps, _to
    model_fn, params, batches = _bag_batches(tmp_path_factory)
    assert set(_nnz(batches[3])) == {"manual_tag_list"}
    caps = {"manual_tag_list": -(-max(_nnz(b)["manual_tag_list"] for b in batches) // 48)}
    sequence = [batches[i] for i in (0, 1, 2, 3, 0, 1)]
    place = lambda b: _to(b, dev)                            # noqa: E731
    eager = _steps(dev, model_fn, params, sequence, place, use_hip_graph=True, ragged_capacity=None)
    assert eager[0].graph_replays == 0
    graphed = _steps(dev, model_fn, params, sequence, place, use_hip_graph=True, ragged_capacity=caps)
    est = graphed[0]
    assert est.capture_refused is None and est.ragged_overflows == 0 and est.graph_replays == 6 - 2 - 1
    _assert_same_run(graphed, eager, f"autoint, ragged_capacity={caps}")


def test_three_steps_follow_the_fp64_restatement(dev, tmp_path):
    """3 eager Estimator.train_step calls on rotating sub-batches of the shared batch against the float64 restatement's own
    free-running trajectory, inside tests/trajectory_ref.bounds; the float32 restatement itself must sit below half of that
    bound for the test to be one of the kernels."""
    from oracle import ref_ops as O
    from tests import trajectory_ref as T
    N = 3
    est, params, _, _ = _on_device(dev, tmp_path)             # the flags' defaults: 3 layers, no deep part
    arrays = _redraw(est)
    start = {k: v.detach().cpu().double() for k, v in arrays.items()}
    lr = float(params["learning_rate"])
    sfeats, labels = GU.string_batch()
    batches = [T.cut(sfeats, labels, idx) for idx in T.batch_indices()]

    def trajectory(dtype):
        P = {k: v.clone().to(dtype) for k, v in start.items()}
        m, v_ = {k: torch.zeros_like(v) for k, v in P.items()}, {k: torch.zeros_like(v) for k, v in P.items()}
        out = {"loss": [], "grad": [], "v": []}
        for k, b in enumerate(T.ORDER[:N], start=1):
            for n, p in P.items():
                p.grad = None
                p.requires_grad_(not n.split("/")[-1].startswith("moving_"))
            sf, lb = batches[b]
            feats = {n: (t.to(dtype) if isinstance(t, torch.Tensor) and t.is_floating_point() else t) for n, t in encode(params, sf).items()}
            bn_state = {}
            res = R.autoint(P, feats, {"read_comment": lb.to(dtype)}, params, training=True, bn_state=bn_state)
            res["loss"].backward()
            grads = {n: p.grad.detach().clone() for n, p in P.items() if p.grad is not None}
            with torch.no_grad():
                for n, gr in grads.items():
                    O.adam_tf1_step(P[n], gr, m[n], v_[n], k, lr)
                for scope, (mean, var) in bn_state.items():          # the moving statistics: momentum 0.99
                    P[f"{scope}/moving_mean"].mul_(0.99).add_(0.01 * mean)
                    P[f"{scope}/moving_variance"].mul_(0.99).add_(0.01 * var)
            out["loss"].append(res["loss"].detach().clone())
            out["grad"].append(grads)
            out["v"].append({n: v_[n].clone() for n in grads})
        out["final"] = {n: p.detach().clone() for n, p in P.items()}
        out["trainable"] = sorted({n for gr in out["grad"] for n in gr})
        return out
    r64, r32 = trajectory(torch.float64), trajectory(torch.float32)
    bnd = T.bounds(r64, lr)
    w32, where32, out32 = T.worst_ratio({k: r32["final"][k] for k in r64["trainable"]}, r64, bnd)
    assert w32 <= 0.5, f"the fp32 restatement alone uses {w32:.3f} of the bound at {where32}"
    host = [({k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sf.items()}, {"read_comment": lb.float()}) for sf, lb in batches]
    dev_batches = [est._to_device(f, l) for f, l in host]
    losses = [est.train_step(*dev_batches[b]).clone() for b in T.ORDER[:N]]
    torch.cuda.synchronize()
    for k, (l, l64, l32) in enumerate(zip(losses, r64["loss"], r32["loss"]), start=1):
        assert_close(l, l64, what=f"autoint loss of step {k}", ref32=l32)
    assert int(est.store.opt_state["step"]) == N
    after = est.store.named_arrays()
    assert len(r64["trainable"]) == 7 + 2 + 4 * L_DEFAULT + 2             # tables, dense_logit, the layers, autoint_logit
    wk, wherek, outk = T.worst_ratio({k: after[k] for k in r64["trainable"]}, r64, bnd)
    print(f"autoint: worst |p - p64| / tol after {N} steps: kernels {wk:.3f} ({wherek}) | fp32 restatement {w32:.3f} ({where32})")
    assert wk <= 1.0, f"autoint: {wherek} is {wk:.3f} x the bound after {N} steps (fp32 restatement: {w32:.3f} at {where32})"
    for k in outk:
        assert outk[k] <= 1.5 * out32[k] + 10, f"autoint {k}: {outk[k]} elements outside the tight bound, the fp32 restatement leaves {out32[k]}"


# ---- evaluate and serving ------------------------------------------------------------------------------------------------------------
def test_evaluate_on_the_device_is_the_host_loop(dev, tmp_path_factory):
    from tests.test_gpu_ragged import _to
    model_fn, params, batches = _bag_batches(tmp_path_factory)
    sequence = [_to(batches[i], dev) for i in (0, 1, 2, 0, 1, 3)]
    results = {}
    for name, run in (("host loop", dict(device_metrics=False, use_hip_graph=False)),
                      ("device, eager", dict(device_metrics=True, use_hip_graph=False)),
                      ("device, captured", dict(device_metrics=True, use_hip_graph=True, ragged_capacity=8))):
        est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, **run))
        est.build(*sequence[0])
        for b in sequence[:2]:
            est.train_step(*b)
        results[name] = est.evaluate(lambda: iter(sequence))
        if name == "device, captured":
            assert est.graph_replays == 6 - 2 - 1 and est.ragged_overflows == 0 and est.capture_refused is None
    want = results["host loop"]
    assert {"eval_accuracy", "eval_auc", "loss", "global_step"} <= set(want) and 0.0 < want["loss"]
    for name, got in results.items():
        assert got == want and list(got) == list(want), name


def test_an_export_predicts_what_the_estimator_predicts(dev, tmp_path):
    """ServingModel.predict and the uncompiled serve() on an export against estimator.predict, bit for bit.  (compile() is left
    out: with the bag it needs a ragged_capacity of the request, nothing of the model.)"""
    import numpy as np

    from recalgorithm_amd import export as E
    from recalgorithm_amd import feature_column as fc
    from tests.test_gpu_serving import golden_records
    est, params, feats, lab = _on_device(dev, tmp_path, hidden_units="32,16")
    _redraw(est)
    est.train_step(feats, lab)
    sfeats, _ = GU.string_batch()
    host = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    want = list(est.predict(lambda: iter([host])))
    assert len(want) == 48 and sorted(want[0]) == ["logit", "probabilities"]
    recv = E.build_parsing_serving_input_receiver_fn(fc.make_parse_example_spec(GU.all_columns(params)))
    export_dir = E.export_model(est, str(tmp_path / "export"), recv)
    model = E.ServingModel(est.model_fn, params, export_dir, device=dev)
    records = golden_records()
    for got, what in ((model.predict(records), "predict"), (model.serve(records), "serve")):
        assert sorted(got) == ["logit", "probabilities"]
        for k in got:
            assert np.array_equal(np.asarray(got[k]).reshape(48, -1), np.stack([w[k] for w in want]).reshape(48, -1)), (what, k)
    p = np.stack([w["probabilities"] for w in want])
    assert float(p.max() - p.min()) > 0.01
