"""-m gpu: DCN-V2's cross layer (csrc/dcnv2.hip, include/recalgo_dcnv2.h) behind ops.dcnv2_layer and nn.cross_mix_layer /
nn.cross_mix_network, and the model (algorithm/DCNV2/dcnv2.py): parity of every output with tests/dcnv2_ref.py at every shape the
kernels change path, once with xl being x0, a batch beyond the partial-row cap, large gate scores, saturated projections, row
independence, the partial rows at the C ABI under guarded allocations, the refusals, run to run and under torch.cuda.graph, a
stack against single calls, the model against the float64 restatement (PREDICT, loss, every gradient, one Adam step) for both
parameterizations and structures, a three-step trajectory, captured training with single-valued columns and with a bag under
ragged_capacity, evaluate on the device metrics path and serving from an export."""
import ctypes

import pytest
import torch

from recalgorithm_amd import _lib, nn, ops
from recalgorithm_amd.variables import VariableStore, use_store
from tests import dcnv2_ref as R
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu
ENTRIES = ("recalgo_dcnv2_layer_fwd", "recalgo_dcnv2_layer_bwd")
WEIGHTS = ("V", "C", "U", "gate", "bias")
GRADS = dict(zip(WEIGHTS, ("dV", "dC", "dU", "dgate", "dbias")))
MID = (67, 20, 8, 3)


def _dev(x, dev):
    return {k: (None if v is None else v.to(dev).contiguous()) for k, v in x.items()}


def run_op(dev, x, grad=True, same=False):
    """ops.dcnv2_layer on plain tensors, forward + backward -> {y, dx0, dxl, dV, dC, dU[, dgate], dbias}; same: xl IS x0"""
    t = _dev(x, dev)
    x0 = t["x0"].requires_grad_(grad)
    xl = x0 if same else t["xl"].requires_grad_(grad)
    ws = [None if t[k] is None else t[k].requires_grad_(grad) for k in WEIGHTS]
    if not grad:
        with torch.no_grad():
            return {"y": ops.dcnv2_layer(x0, xl, *ws)}
    y = ops.dcnv2_layer(x0, xl, *ws)
    y.backward(t["g"])
    out = {"y": y.detach(), "dx0": x0.grad}
    if not same:
        out["dxl"] = xl.grad
    for k, w in zip(WEIGHTS, ws):
        if w is not None:
            out[GRADS[k]] = w.grad
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


def _judge(got, x, r64, r32, what, same=False, floor=None):
    assert sorted(got) == sorted(R.names_of(x, same))
    for k in R.names_of(x, same):
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        assert bool(torch.isfinite(got[k]).all()), k
        extra = {} if floor is None else {"floor": floor(r64, r32, k)}
        assert_close(got[k], r64[k], what=f"{what} {k}", reduced=k in R.REDUCED, ref32=r32[k], **extra)


@pytest.mark.parametrize("B,D,r,E", R.SHAPES)
def test_parity(dev, B, D, r, E):
    """every output against the float64 restatement; a single expert runs without a gate"""
    x, r64, r32 = R.case(B, D, r, E, gated=E > 1)
    got = run_op(dev, x)
    _judge(got, x, r64, r32, f"ops.dcnv2_layer B={B} D={D} r={r} E={E}")
    assert_bit_exact(run_op(dev, x, grad=False)["y"], got["y"], "the forward with grad disabled")


def test_parity_with_a_gate_over_one_expert(dev):
    x, r64, r32 = R.case(17, 12, 8, 1, gated=True)
    got = run_op(dev, x)
    _judge(got, x, r64, r32, "ops.dcnv2_layer, E = 1 with a gate")
    assert bool((got["dgate"] == 0).all())


def test_parity_with_xl_being_x0(dev):
    """a stack's first layer: one tensor for both, dx0 + dxl as its gradient"""
    x, r64, r32 = R.case(33, 82, 8, 2, same=True)
    got = run_op(dev, x, same=True)
    _judge(got, x, r64, r32, "ops.dcnv2_layer, xl is x0", same=True)
    assert_bit_exact(run_op(dev, x, grad=False, same=True)["y"], got["y"], "the forward with grad disabled")


def test_more_examples_than_the_partial_rows_and_the_grid_serve(dev):
    """B = 16403 at D 8, r 4, E 2: 1026 tiles for a grid of 1024 workgroups, and 65 x 16 tiles for 64 partial rows — a workgroup
    takes a second tile, a partial row more than 16"""
    B, D, r, E = 16403, 8, 4, 2
    rows = int(_lib.load().recalgo_dcnv2_bwd_partial_rows(B, D, r, E))
    C = _lib.SERVING_HEADERS["recalgo_dcnv2.h"].constants
    assert rows == C["RECALGO_DCNV2_MAX_PARTIAL_ROWS"] == 64
    assert B > rows * C["RECALGO_DCNV2_ROW_TILES"] * C["RECALGO_DCNV2_TILE"] and -(-B // C["RECALGO_DCNV2_TILE"]) > 1024
    x, r64, r32 = R.case(B, D, r, E)
    _judge(run_op(dev, x), x, r64, r32, f"ops.dcnv2_layer B={B} D={D} r={r} E={E}")


def test_large_gate_scores(dev):
    """the gate scaled by 400 at (67, 20, 8, 3): scores of +-1000, where exp() of an unshifted score overflows.  Every output is
    finite and parity holds with the floor of afm_ref.fp32_floor: 4 x the float32 restatement's own deviation."""
    from tests.afm_ref import fp32_floor
    x, r64, r32 = R.case(**R.LARGE_GATE)
    assert float(r64["s"].max()) > 1000 and float(r64["s"].min()) < -1000
    _judge(run_op(dev, x), x, r64, r32, "ops.dcnv2_layer, large gate scores:", floor=fp32_floor)


def test_saturated_projections(dev):
    """V scaled by 40: |xl V| is above 20 in most places, tanh is 1 to the last bit there and 1 - v^2 exactly 0"""
    x, r64, r32 = R.case(**R.SATURATED)
    pre = torch.einsum("bd,edr->ber", x["xl"].double(), x["V"].double()).abs()
    assert float((pre > 20).double().mean()) > 0.5
    _judge(run_op(dev, x), x, r64, r32, "ops.dcnv2_layer, saturated projections:")


def _rows_of(x, rows):
    return dict(x, x0=x["x0"][rows].clone(), xl=x["xl"][rows].clone(), g=x["g"][rows].clone())


def test_a_row_depends_on_that_row_alone(dev):
    x, _, _ = R.case(*MID)
    whole = run_op(dev, x)
    for r in (0, 31, 66):
        alone = run_op(dev, _rows_of(x, [r]))
        five = run_op(dev, _rows_of(x, [1, 2, 5, r, 7]))
        for k in ("y", "dx0", "dxl"):
            assert_bit_exact(alone[k][0], whole[k][r], f"row {r} alone, {k}")
            assert_bit_exact(five[k][3], whole[k][r], f"row {r} as the fourth of five, {k}")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("B,D,r,E,gated", [(1, 4, 4, 1, False), (33, 82, 8, 2, True), (300, 20, 8, 3, True), (19, 416, 32, 4, True)])
def test_the_outputs_are_the_fixed_order_sums_of_the_partial_rows(dev, B, D, r, E, gated):
    """At the C ABI on buffers of exactly the documented sizes, under the guard: the parameter gradients are
    tests/dense_ref.colsum_fixed_order of the workspace's rows [dV | dC | dU | dgate | dbias], bit for bit; the workspace is
    exactly as large as the query says; no store lands outside any buffer."""
    from tests.redzone import guarded
    from tests.test_gpu_colsums import _assert_outputs_are_the_sums, _workspace_of
    x, r64, r32 = R.case(B, D, r, E, gated=gated)
    row_max = E * (2 * D * r + r * r + D) + D
    with guarded() as g:
        lib = _lib.load()
        rows = int(lib.recalgo_dcnv2_bwd_partial_rows(B, D, r, E))
        nbytes = int(lib.recalgo_dcnv2_bwd_workspace_bytes(B, D, r, E))
        assert rows == -(-(-(-B // 16)) // 16) and nbytes == 4 * (rows * row_max + B * (4 * E * r + 4))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        t = _dev(x, dev)
        y = torch.empty(B, D, device=dev)
        lib.recalgo_dcnv2_layer_fwd(_p(t["x0"]), _p(t["xl"]), _p(t["V"]), _p(t["C"]), _p(t["U"]), _p(t["gate"]), _p(t["bias"]), B, D, r, E,
                                    _p(y), st)
        grads = {"dV": torch.empty(E, D, r, device=dev), "dC": torch.empty(E, r, r, device=dev), "dU": torch.empty(E, D, r, device=dev)}
        if gated:
            grads["dgate"] = torch.empty(E, D, device=dev)
        grads["dbias"] = torch.empty(D, device=dev)
        dx0, dxl = torch.empty(B, D, device=dev), torch.empty(B, D, device=dev)
        ws = ops._workspace(nbytes, torch.device(dev))
        lib.recalgo_dcnv2_layer_bwd(_p(t["g"]), _p(t["x0"]), _p(t["xl"]), _p(t["V"]), _p(t["C"]), _p(t["U"]), _p(t["gate"]), _p(t["bias"]),
                                    B, D, r, E, _p(dx0), _p(dxl), _p(grads["dV"]), _p(grads["dC"]), _p(grads["dU"]), _p(grads.get("dgate")),
                                    _p(grads["dbias"]), _p(ws), st)
        wsf = _workspace_of(g)
        assert wsf.numel() == max(nbytes // 4, 4)
        _assert_outputs_are_the_sums(wsf, rows, grads, f"dcnv2_layer_bwd B={B} D={D} r={r} E={E} gated={gated}")
        assert set(ENTRIES) <= g.launched
        got = dict(grads, y=y, dx0=dx0, dxl=dxl)
        _judge(got, x, r64, r32, f"the C entries B={B} D={D} r={r} E={E} gated={gated}")


@pytest.mark.parametrize("B,D,r,E", [(4, 3, 8, 2), (4, 513, 8, 2), (4, 20, 6, 2), (4, 20, 68, 2), (4, 20, 8, 0), (4, 20, 8, 5), (0, 20, 8, 2)])
def test_shapes_outside_the_domain_are_refused(dev, B, D, r, E, monkeypatch):
    """the op raises, the ABI returns hipErrorInvalidValue, the queries return 0 and nothing is launched"""
    from tests.redzone import guarded
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device=dev)               # noqa: E731
    Ez = max(E, 1)
    t = [z(max(B, 1), D), z(max(B, 1), D), z(Ez, D, r), z(Ez, r, r), z(Ez, D, r), z(Ez, D), z(D)]
    out = [z(max(B, 1), D), z(max(B, 1), D), z(Ez, D, r), z(Ez, r, r), z(Ez, D, r), z(Ez, D), z(D), z(1024)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.recalgo_dcnv2_bwd_partial_rows(B, D, r, E) == 0 and lib.recalgo_dcnv2_bwd_workspace_bytes(B, D, r, E) == 0
    if B > 0:
        assert lib.recalgo_dcnv2_supported(D, r, E) == 0
    with guarded() as g:
        with pytest.raises(_lib.RecalgoError, match="recalgo_dcnv2_layer_fwd failed with hipError_t=1$"):
            lib.recalgo_dcnv2_layer_fwd(*[_p(a) for a in t], B, D, r, E, _p(out[0]), st)
        with pytest.raises(_lib.RecalgoError, match="recalgo_dcnv2_layer_bwd failed with hipError_t=1$"):
            lib.recalgo_dcnv2_layer_bwd(_p(out[0]), *[_p(a) for a in t], B, D, r, E, *[_p(a) for a in out], st)
        assert not (set(ENTRIES) & g.launched)
    calls = _count(monkeypatch)
    with pytest.raises(ValueError, match="the kernels serve|must be non-empty"):
        ops.dcnv2_layer(t[0][:B] if B == 0 else t[0], t[1][:B] if B == 0 else t[1], *(t[2:] if E > 0 else [a[:0] for a in t[2:6]] + [t[6]]))
    assert calls == {n: 0 for n in ENTRIES}


def test_a_null_operand_and_half_a_gate_pair_are_refused(dev, monkeypatch):
    from tests.redzone import guarded
    lib = _lib.load()
    x, _, _ = R.case(*MID)
    t = _dev(x, dev)
    B, D, r, E = MID
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = [t[k] for k in ("x0", "xl") + WEIGHTS]
    outs = [torch.empty_like(a) for a in ins] + [torch.empty(int(lib.recalgo_dcnv2_bwd_workspace_bytes(B, D, r, E)) // 4, device=dev)]
    with guarded() as g:
        for i in range(7):
            with pytest.raises(_lib.RecalgoError, match="hipError_t=1$"):
                lib.recalgo_dcnv2_layer_fwd(*[None if j == i else _p(a) for j, a in enumerate(ins)], B, D, r, E, _p(outs[0]), st)
        for i in range(16):
            args = [_p(t["g"])] + [_p(a) for a in ins] + [_p(a) for a in outs]
            args[i] = None
            with pytest.raises(_lib.RecalgoError, match="hipError_t=1$"):
                lib.recalgo_dcnv2_layer_bwd(*args[:8], B, D, r, E, *args[8:], st)
        one = [a[:1].contiguous() if a.dim() > 1 and a.shape[0] == E else a for a in ins]           # a single expert: half a pair
        o1 = [torch.empty_like(a) for a in one] + [outs[-1]]
        for i in (6, 13):
            args = [_p(t["g"])] + [_p(a) for a in one] + [_p(a) for a in o1]
            args[i] = None
            with pytest.raises(_lib.RecalgoError, match="hipError_t=1$"):
                lib.recalgo_dcnv2_layer_bwd(*args[:8], B, D, r, 1, *args[8:], st)
        assert not (set(ENTRIES) & g.launched)
    calls = _count(monkeypatch)
    with pytest.raises(ValueError, match="only a single expert runs without a gate"):
        ops.dcnv2_layer(t["x0"], t["xl"], t["V"], t["C"], t["U"], None, t["bias"])
    assert calls == {n: 0 for n in ENTRIES}


def test_two_runs_and_three_replays_give_the_same_bits(dev):
    """forward + backward: eagerly twice, once on a side stream (the warm-up a capture needs), captured and replayed three times"""
    x, _, _ = R.case(300, 20, 8, 3)
    t = _dev(x, dev)
    x0, xl = t["x0"].requires_grad_(True), t["xl"].requires_grad_(True)
    ws = [t[k].requires_grad_(True) for k in WEIGHTS]

    def run():
        y = ops.dcnv2_layer(x0, xl, *ws)
        return [y.detach()] + list(torch.autograd.grad(y, [x0, xl] + ws, t["g"]))
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


def test_three_layers_are_three_single_calls(dev, monkeypatch):
    """nn.cross_mix_network of three layers on a store of its own against three ops.dcnv2_layer calls on the same values: y, dx
    and every variable's gradient bit for bit, one forward and one backward entry per layer; the composed layer (fused=False)
    agrees within the bound"""
    B, D, r, E, L = 33, 20, 8, 3, 3
    store = VariableStore(dev, seed=3)
    with use_store(store):
        store.building = True
        out = nn.cross_mix_network(torch.zeros(B, D, device=dev), L, r, E)
        assert tuple(out.shape) == (B, D) and not bool(out.any())
        store.finalize()
    names = [[f"cross_layer_{i}/{n}" for n in WEIGHTS] for i in range(L)]
    assert sorted(store.vars) == sorted(n for ns in names for n in ns)
    gen = torch.Generator().manual_seed(11)
    for ns in names:
        store.vars[ns[4]].data.copy_(torch.randn(D, generator=gen) * 0.3)
        store.vars[ns[3]].data.copy_(torch.randn(E, D, generator=gen) * 0.5)
    xs = torch.randn(B, D, generator=gen).to(dev)
    g = torch.randn(B, D, generator=gen).to(dev)
    calls = _count(monkeypatch)
    x = xs.clone().requires_grad_(True)
    with use_store(store):
        store.begin_call()
        y = nn.cross_mix_network(x, L, r, E)
        assert calls == {ENTRIES[0]: L, ENTRIES[1]: 0}
        y.backward(g)
        ops.flush_dense_splits()
    assert calls == {ENTRIES[0]: L, ENTRIES[1]: L}
    kept = {n: store.vars[n].grad.clone() for ns in names for n in ns}
    plain = [[store.vars[n].data.clone().requires_grad_(True) for n in ns] for ns in names]
    x2 = xs.clone().requires_grad_(True)
    y2 = x2
    for ws in plain:
        y2 = ops.dcnv2_layer(x2, y2, *ws)
    y2.backward(g)
    assert_bit_exact(y, y2, "y of the stack")
    assert_bit_exact(x.grad, x2.grad, "dx of the stack")
    for ns, ws in zip(names, plain):
        for n, w in zip(ns, ws):
            assert_bit_exact(kept[n], w.grad, f"d({n})")
    assert float(y.detach().abs().max()) > 0 and float(x.grad.abs().max()) > 0
    # the composed layer on the same store
    x3 = xs.clone().requires_grad_(True)
    with use_store(store):
        store.begin_call()
        y3 = nn.cross_mix_network(x3, L, r, E, fused=False)
        y3.backward(g)
    assert calls == {ENTRIES[0]: 2 * L, ENTRIES[1]: 2 * L}
    # the float64 restatement of the stack judges both
    P64 = {f"cross_part/{n}": store.vars[n].data.detach().cpu().double().requires_grad_(True) for ns in names for n in ns}
    P32 = {k: v.detach().float().requires_grad_(True) for k, v in P64.items()}
    refs = []
    for P, dt in ((P64, torch.float64), (P32, torch.float32)):
        xr = xs.cpu().to(dt).requires_grad_(True)
        yr = R.cross_mix(P, xr, L)
        yr.backward(g.cpu().to(dt))
        refs.append((yr.detach(), xr.grad))
    for what, yy, xx, grads in (("fused", y, x, kept), ("composed", y3, x3, {n: store.vars[n].grad for ns in names for n in ns})):
        assert_close(yy, refs[0][0], what=f"{what} stack y", ref32=refs[1][0])
        assert_close(xx.grad, refs[0][1], what=f"{what} stack dx", ref32=refs[1][1])
        for n, gr in grads.items():
            assert_close(gr, P64[f"cross_part/{n}"].grad, what=f"{what} stack d({n})", reduced=True, ref32=P32[f"cross_part/{n}"].grad)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig  # noqa: E402
from tests.test_dcnv2_host import dcnv2_setup, expected_variables  # noqa: E402

FORMS = [("mix", "parallel"), ("mix", "stacked"), ("matrix", "parallel")]


def _redraw(est, seed=16):
    """The cross weights over inputs of order 1 so that the gate is not flat and tanh not linear (glorot-uniform over the default
    tables leaves projections of order 0.01): V as N(0, 1) / sqrt(D), C and U as N(0, 1) / sqrt(r), the gate as N(0, 1) / sqrt(D), a
    bias of order 0.3, tables of order 0.5, the matrix form's W as N(0, 0.5) / sqrt(D)."""
    arrays = est.store.named_arrays()
    gen = torch.Generator().manual_seed(seed)
    for k, v in arrays.items():
        leaf = k.split("/")[-1]
        if "cross_layer_" in k and leaf in ("V", "gate"):
            v.copy_(torch.randn(*v.shape, generator=gen) / v.shape[1] ** 0.5)
        elif "cross_layer_" in k and leaf in ("C", "U"):
            v.copy_(torch.randn(*v.shape, generator=gen) / v.shape[-1] ** 0.5)
        elif "cross_layer_" in k and leaf == "bias":
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.3)
        elif "cross_layer_" in k and leaf == "kernel":
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.5 / v.shape[0] ** 0.5)
        elif k.endswith("/embedding_weights"):
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.5)
        elif k == "output_part/dense/kernel":
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.3)
    return arrays


def _model(dev, B=64, run=None, **flags):
    from recalgorithm_amd.io import synth
    model_fn, params, spec = dcnv2_setup(**flags)
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, **(run or dict(use_hip_graph=False))))
    feats, labels, _ = synth.device_features(spec, B, dev, batch_index=0)
    est.build(feats, labels)
    return est, params, spec, feats, labels


def _host_batch(feats, labels, dtype):
    cf = {k: v.cpu() for k, v in feats.items() if isinstance(v, torch.Tensor)}
    cf = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in cf.items()}
    return cf, {k: v.cpu().to(dtype) for k, v in labels.items()}


def _oracle(params, variables, feats, labels, dtype):
    P = {k: v.clone().to(dtype).requires_grad_(True) for k, v in variables.items()}
    cf, cl = _host_batch(feats, labels, dtype)
    with torch.no_grad():
        predict = R.dcnv2(P, cf, None, params)
    out = R.dcnv2(P, cf, cl, params, training=True)
    out["loss"].backward()
    return {"predict": predict, "loss": out["loss"].detach(), "P": P}


@pytest.mark.parametrize("form,structure", FORMS)
def test_the_model_follows_the_fp64_restatement(dev, form, structure, monkeypatch):
    """B 64 on small columns (16 dense features and 6 id columns of width 4: D = 40), two cross layers (3 experts of rank 8), two
    hidden layers: PREDICT, the TRAIN loss, every gradient and one Adam step against tests/dcnv2_ref.dcnv2 in float64, with the
    floor of the float32 restatement's own deviation (golden_protocol.judge_step_against_oracle); no variable is missing or extra.
    The mix form launches each entry once per layer, the matrix form neither."""
    from tests.golden_protocol import judge_step_against_oracle
    est, params, spec, feats, lab = _model(dev, cross_parameterization=form, structure=structure)
    arrays = _redraw(est)
    want = expected_variables(params, 40, 6, 4)
    assert sorted(k for k in arrays if not k.endswith("/embedding_weights")) == sorted(want)
    variables = {k: v.detach().cpu().double() for k, v in arrays.items()}
    before = {k: v.clone() for k, v in variables.items()}
    r64, r32 = _oracle(params, variables, feats, lab, torch.float64), _oracle(params, variables, feats, lab, torch.float32)
    p = r64["predict"]["prob"]
    assert float(p.max() - p.min()) > 0.05, "the redrawn variables tell the rows apart"
    L = params["num_cross_layer"] if form == "mix" else 0
    calls = _count(monkeypatch)
    pr = est._call_model_fn(feats, None, ModeKeys.PREDICT)
    assert calls == {ENTRIES[0]: L, ENTRIES[1]: 0}
    what = f"dcnv2 {form} {structure}"
    assert list(pr.predictions) == ["logit", "probabilities"]
    assert_close(pr.predictions["probabilities"], r64["predict"]["prob"], what=f"{what} predict", ref32=r32["predict"]["prob"])
    assert_close(pr.predictions["logit"], r64["predict"]["logit"], what=f"{what} logit", ref32=r32["predict"]["logit"])
    spec_ = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
    assert_close(spec_.loss, r64["loss"], what=f"{what} loss", ref32=r32["loss"])
    assert all(p_.grad is not None for k, p_ in r64["P"].items()), "every variable of the restatement has a gradient"
    judge_step_against_oracle(est, spec_, r64["P"], r32["P"], before, params["learning_rate"], what, len(want) + 6)
    assert calls == {ENTRIES[0]: 2 * L, ENTRIES[1]: L}


def test_three_steps_follow_the_fp64_restatement(dev):
    """3 eager Estimator.train_step calls on three synthetic batches of 64 against the float64 restatement's own free-running
    trajectory, inside tests/trajectory_ref.bounds; the float32 restatement itself must sit below half of that bound for the test
    to be one of the kernels."""
    from oracle import ref_ops as O
    from recalgorithm_amd.io import synth
    from tests import trajectory_ref as T
    N = 3
    est, params, spec, _, _ = _model(dev)
    arrays = _redraw(est)
    start = {k: v.detach().cpu().double() for k, v in arrays.items()}
    lr = float(params["learning_rate"])
    dev_batches = [synth.device_features(spec, 64, dev, batch_index=i)[:2] for i in range(N)]

    def trajectory(dtype):
        P = {k: v.clone().to(dtype) for k, v in start.items()}
        m, v_ = {k: torch.zeros_like(v) for k, v in P.items()}, {k: torch.zeros_like(v) for k, v in P.items()}
        out = {"loss": [], "grad": [], "v": []}
        for k in range(1, N + 1):
            for p in P.values():
                p.grad = None
                p.requires_grad_(True)
            cf, cl = _host_batch(*dev_batches[k - 1], dtype)
            res = R.dcnv2(P, cf, cl, params, training=True)
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
    r64, r32 = trajectory(torch.float64), trajectory(torch.float32)
    bnd = T.bounds(r64, lr)
    w32, where32, out32 = T.worst_ratio({k: r32["final"][k] for k in r64["trainable"]}, r64, bnd)
    assert w32 <= 0.5, f"the fp32 restatement alone uses {w32:.3f} of the bound at {where32}"
    losses = [est.train_step(*b).clone() for b in dev_batches]
    torch.cuda.synchronize()
    for k, (l, l64, l32) in enumerate(zip(losses, r64["loss"], r32["loss"]), start=1):
        assert_close(l, l64, what=f"dcnv2 loss of step {k}", ref32=l32)
    assert int(est.store.opt_state["step"]) == N
    after = est.store.named_arrays()
    assert len(r64["trainable"]) == len(start)
    wk, wherek, outk = T.worst_ratio({k: after[k] for k in r64["trainable"]}, r64, bnd)
    print(f"dcnv2: worst |p - p64| / tol after {N} steps: kernels {wk:.3f} ({wherek}) | fp32 restatement {w32:.3f} ({where32})")
    assert wk <= 1.0, f"dcnv2: {wherek} is {wk:.3f} x the bound after {N} steps (fp32 restatement: {w32:.3f} at {where32})"
    for k in outk:
        assert outk[k] <= 1.5 * out32[k] + 10, f"dcnv2 {k}: {outk[k]} elements outside the tight bound, the fp32 restatement leaves {out32[k]}"


# ---- captured training ---------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_what_eager_steps_compute(dev):
    """three hipGraph replays of the captured step (B 256, single-valued columns) against eager launches on rotating batches, bit
    for bit (tests/test_gpu_replay_models.py's comparison)"""
    from recalgorithm_amd.estimator import GraphedTrainStep, _tree_tensors
    from recalgorithm_amd.io import synth
    from tests.test_gpu_replay_models import _differences, _state
    WARMUP, STEPS, N_BATCHES = 3, 3, 3
    run = dict()
    (eager, _, spec, _, _), (graphed, _, _, _, _) = _model(dev, B=256, run=run), _model(dev, B=256, run=run)
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


def _dataset_setup(vocab_dir):
    """(model_fn, params) on the dataset's own columns (DCN's: D = 82, with the manual_tag_list bag and the shared feedid table)"""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.DCNV2 import dcnv2 as m
    flags.FLAGS.vocabulary_dir = vocab_dir
    dense, cat, _ = m.create_feature_columns()
    return m.dcnv2_model_fn, {"category_feature_columns": cat, "dense_feature_columns": dense, "hidden_units": [32, 16], "num_cross_layer": 2,
                              "cross_parameterization": "mix", "low_rank": 8, "num_experts": 3, "structure": "parallel", "learning_rate": 0.005}


def _bag_batches(tmp_path_factory):
    """(model_fn, params, four host batches of the 48 shared rows: 0 .. 2 with rolled rows and cut bags, 3 the rows themselves)"""
    from tests import golden_util as GU
    from tests.test_gpu_ragged import _encoded, _roll_cut
    if not _bag_model:
        vocab_dir = GU.write_vocab_dir(str(tmp_path_factory.mktemp("dcnv2") / "vocabulary"))
        model_fn, params = _dataset_setup(vocab_dir)
        base = _encoded(params)
        _bag_model["m"] = (model_fn, params, [_roll_cut(*base, s, keep) for s, keep in ((5, 3), (11, 2), (17, 4))] + [_roll_cut(*base, 0, 8)])
    return _bag_model["m"]


def test_captured_steps_with_the_bags_are_the_eager_steps(dev, tmp_path_factory):
    """the dataset's columns (D = 82) with their bags under ragged_capacity, no model-specific code: two eager warm-up steps, the
    capture, three replays — losses and variables bit for bit those of eager steps"""
    from tests.test_gpu_ragged import _assert_same_run, _nnz, _steps, _to
    model_fn, params, batches = _bag_batches(tmp_path_factory)
    bags = sorted(_nnz(batches[3]))
    assert "manual_tag_list" in bags
    caps = {k: -(-max(_nnz(b)[k] for b in batches) // 48) for k in bags}
    sequence = [batches[i] for i in (0, 1, 2, 3, 0, 1)]
    place = lambda b: _to(b, dev)                            # noqa: E731
    eager = _steps(dev, model_fn, params, sequence, place, use_hip_graph=True, ragged_capacity=None)
    assert eager[0].graph_replays == 0
    graphed = _steps(dev, model_fn, params, sequence, place, use_hip_graph=True, ragged_capacity=caps)
    est = graphed[0]
    assert est.capture_refused is None and est.ragged_overflows == 0 and est.graph_replays == 6 - 2 - 1
    _assert_same_run(graphed, eager, f"dcnv2, ragged_capacity={caps}")


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
    out: with the bags it needs a ragged_capacity of the request, nothing of the model.)"""
    import numpy as np

    from recalgorithm_amd import export as E
    from recalgorithm_amd import feature_column as fc
    from tests import golden_util as GU
    from tests.test_gpu_serving import golden_records
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = _dataset_setup(vocab_dir)
    sfeats, labels = GU.string_batch()
    host = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, use_hip_graph=False))
    est.build(host, lab)
    _redraw(est)
    est.train_step(*est._to_device(host, lab))
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
