"""-m gpu: FLEN's field-wise bi-interaction with Dicefactor (csrc/flen.hip, include/recalgo_flen.h) behind ops.flen_interaction and
nn.field_wise_bi_interaction, and the model (algorithm/FLEN/flen.py): parity of every output with tests/flen_ref.py at every shape
the kernels change path — without Dicefactor, with an explicit keep mask, with the hash — a large offset, a batch beyond the
partial-row cap, row independence, the partial rows at the C ABI under guarded allocations, the refusals, run to run and under
torch.cuda.graph, the composed path, the model against the float64 restatement (PREDICT, loss, every gradient, one Adam step, all
masks injected), a three-step trajectory, captured training with single-valued columns and with the bag under ragged_capacity (both
with Dicefactor on the hash), evaluate on the device metrics path and serving from an export."""
import ctypes

import pytest
import torch

from recalgorithm_amd import _lib, nn, ops
from recalgorithm_amd.variables import VariableStore, use_store
from tests import flen_ref as R
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu
ENTRIES = ("recalgo_flen_fwd", "recalgo_flen_bwd")
WEIGHTS = ("r_mf", "r_fm", "bias")
GRADS = dict(zip(WEIGHTS, ("dr_mf", "dr_fm", "dbias")))
MID = (67, 7, 3, 8, R.DATASET_GROUPS)


def _dev(v, dev):
    return {k: (None if t is None else t.to(dev).contiguous()) for k, t in v.items()}


def _spec(dev, B, M, K, mask=None, step=None, rate=R.RATE, seed=12345, call=3):
    """the DropSpec of Dicefactor: an explicit keep mask, or the hash keyed by (seed, call, step)"""
    return ops.DropSpec(rate, None if mask is None else mask.to(dev).contiguous(), seed, call, step)


def run_op(dev, v, groups, grad=True, dice=None):
    """ops.flen_interaction on plain tensors, forward + backward -> {e, h, dx, dr_mf, dr_fm, dbias}"""
    t = _dev(v, dev)
    F = len(groups)
    x = t["x"].requires_grad_(grad)
    ws = [t[k].requires_grad_(grad) for k in WEIGHTS]
    if not grad:
        with torch.no_grad():
            e, h = ops.flen_interaction(x, F, groups, *ws, dice=dice)
            return {"e": e, "h": h}
    e, h = ops.flen_interaction(x, F, groups, *ws, dice=dice)
    torch.autograd.backward([e, h], [t["g_e"], t["g_h"]])
    out = {"e": e.detach(), "h": h.detach(), "dx": x.grad}
    for k, w in zip(WEIGHTS, ws):
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


def _judge(got, r64, r32, what, floor=None):
    assert sorted(got) == sorted(R.NAMES)
    for k in R.NAMES:
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        assert bool(torch.isfinite(got[k]).all()), k
        extra = {} if floor is None else {"floor": floor(r64, r32, k)}
        assert_close(got[k], r64[k], what=f"{what} {k}", reduced=k in R.REDUCED, ref32=r32[k], **extra)


def _singles(groups, M):
    return [m for m in range(M) if groups.count(m) == 1]


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_parity(dev, name):
    """every output against the float64 restatement, no Dicefactor; the FM gradient of a group of one field is exactly 0"""
    B, F, M, K, groups = R.SHAPES[name]
    v, r64, r32 = R.case(B, F, M, K, groups)
    got = run_op(dev, v, groups)
    _judge(got, r64, r32, f"ops.flen_interaction {name}")
    off = run_op(dev, v, groups, grad=False)
    assert_bit_exact(off["e"], got["e"], "e of the forward with grad disabled")
    assert_bit_exact(off["h"], got["h"], "h of the forward with grad disabled")
    single = _singles(groups, M)
    assert bool((got["dr_fm"][single] == 0).all()), "dr_fm of a group of one field"


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_parity_with_an_explicit_keep_mask(dev, name):
    B, F, M, K, groups = R.SHAPES[name]
    v, r64, r32 = R.case(B, F, M, K, groups, masked=True)
    d = _spec(dev, B, M, K, mask=v["keep"])
    got = run_op(dev, v, groups, dice=d)
    _judge(got, r64, r32, f"ops.flen_interaction {name}, explicit mask:")
    off = run_op(dev, v, groups, grad=False, dice=d)
    assert_bit_exact(off["h"], got["h"], "h of the forward with grad disabled")
    assert bool((got["dr_fm"][_singles(groups, M)] == 0).all())
    plain = R.case(B, F, M, K, groups)[1]
    assert not torch.equal(r64["h"], plain["h"]) or B * K < 8, "the mask changes h"


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_parity_with_the_hash(dev, name):
    """the mask the hash stands for (ops.dropout_keep_mask, the same spec) fed to the restatement: forward and backward agree
    with it; after the device step counter advances the mask and the output differ"""
    B, F, M, K, groups = R.SHAPES[name]
    P = M * (M - 1) // 2
    v = R.inputs(B, F, M, K, groups)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    d = _spec(dev, B, M, K, step=step)
    keep = ops.dropout_keep_mask((B, P + M, K), d, torch.device(dev)).cpu()
    assert set(keep.unique().tolist()) <= {0.0, 1.0}
    if keep.numel() >= 1000:
        assert abs(float(keep.mean()) - (1 - R.RATE)) < 0.05
    r64, r32 = R.reference(v, groups, torch.float64, keep=keep), R.reference(v, groups, torch.float32, keep=keep)
    got = run_op(dev, v, groups, dice=d)
    _judge(got, r64, r32, f"ops.flen_interaction {name}, hash:")
    step += 1
    keep2 = ops.dropout_keep_mask((B, P + M, K), d, torch.device(dev)).cpu()
    again = run_op(dev, v, groups, dice=d)
    assert not torch.equal(keep2, keep), "the next step draws another mask"
    assert not torch.equal(again["h"], got["h"]) and torch.equal(again["e"], got["e"])
    r64b, r32b = R.reference(v, groups, torch.float64, keep=keep2), R.reference(v, groups, torch.float32, keep=keep2)
    _judge(again, r64b, r32b, f"ops.flen_interaction {name}, hash, next step:")


def test_a_large_offset(dev):
    """x = 100 + N(0, 1) at (67, 7, 3, 8): e^2 and q of order 1e4 .. 1e5.  Every output is finite and parity holds with the floor
    of afm_ref.fp32_floor: 4 x the float32 restatement's own deviation."""
    from tests.afm_ref import fp32_floor
    B, F, M, K, groups = R.CANCELLATION
    for masked in (False, True):
        v, r64, r32 = R.case(B, F, M, K, groups, offset=100.0, masked=masked)
        d = _spec(dev, B, M, K, mask=v["keep"]) if masked else None
        _judge(run_op(dev, v, groups, dice=d), r64, r32, f"ops.flen_interaction, x = 100 + N(0, 1), masked={masked}:", floor=fp32_floor)


def test_more_examples_than_the_partial_rows_and_the_grid_serve(dev):
    """F 2, M 2, K 4: one lane per example, 64 examples per workgroup and at most 512 workgroups either way — B = 512 * 64 + 64 + 3
    gives 514 tiles: two workgroups take a second tile, the last of them a partial one"""
    F, M, K, groups = 2, 2, 4, (0, 1)
    C = _lib.SERVING_HEADERS["recalgo_flen.h"].constants
    T = C["RECALGO_FLEN_LANES"] // (K // 4)
    B = C["RECALGO_FLEN_MAX_PARTIAL_ROWS"] * T + T + 3
    rows = int(_lib.load().recalgo_flen_bwd_partial_rows(B, F, M, K))
    assert T == 64 and rows == C["RECALGO_FLEN_MAX_PARTIAL_ROWS"] == 512 and -(-B // T) == rows + 2 and B % T
    for masked in (False, True):
        v, r64, r32 = R.case(B, F, M, K, groups, masked=masked)
        d = _spec(dev, B, M, K, mask=v["keep"]) if masked else None
        _judge(run_op(dev, v, groups, dice=d), r64, r32, f"ops.flen_interaction B={B} masked={masked}")


def _rows_of(v, rows):
    return dict(v, x=v["x"][rows].clone(), g_e=v["g_e"][rows].clone(), g_h=v["g_h"][rows].clone(),
                keep=None if v["keep"] is None else v["keep"][rows].clone())


@pytest.mark.parametrize("shape", [MID, (67, 7, 3, 12, R.DATASET_GROUPS)], ids=["K8", "K12"])
def test_a_row_depends_on_that_row_alone(dev, shape):
    B, F, M, K, groups = shape
    v, _, _ = R.case(*shape, masked=True)

    def run(u):
        return run_op(dev, u, groups, dice=_spec(dev, u["x"].shape[0], M, K, mask=u["keep"]))
    whole = run(v)
    for r in (0, 31, 66):
        alone = run(_rows_of(v, [r]))
        five = run(_rows_of(v, [1, 2, 5, r, 7]))
        for k in ("e", "h", "dx"):
            assert_bit_exact(alone[k][0], whole[k][r], f"row {r} alone, {k}")
            assert_bit_exact(five[k][3], whole[k][r], f"row {r} as the fourth of five, {k}")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _groups(groups):
    arr = (ctypes.c_int32 * len(groups))(*groups)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


@pytest.mark.parametrize("name,B", [("smallest", 1), ("dataset", 17), ("three_lanes", 300), ("limits", 5), ("interleaved", 19)])
def test_the_outputs_are_the_fixed_order_sums_of_the_partial_rows(dev, name, B):
    """At the C ABI on buffers of exactly the documented sizes, under the guard: the parameter gradients are
    tests/dense_ref.colsum_fixed_order of the workspace's rows [dr_mf | dr_fm | dbias], bit for bit; the workspace is exactly as
    large as the query says; no store lands outside any buffer."""
    from tests.redzone import guarded
    from tests.test_gpu_colsums import _assert_outputs_are_the_sums, _workspace_of
    _, F, M, K, groups = R.SHAPES[name]
    P = M * (M - 1) // 2
    v, r64, r32 = R.case(B, F, M, K, groups, masked=True)
    keepalive, gp = _groups(groups)
    with guarded() as g:
        lib = _lib.load()
        rows = int(lib.recalgo_flen_bwd_partial_rows(B, F, M, K))
        nbytes = int(lib.recalgo_flen_bwd_workspace_bytes(B, F, M, K))
        assert rows == -(-B // (64 // (K // 4))) and nbytes == 4 * rows * (P + M + K)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        t = _dev(v, dev)
        cd, keep = ops._cdrop(_spec(dev, B, M, K, mask=t["keep"]))
        e, h = torch.empty(B, M * K, device=dev), torch.empty(B, K, device=dev)
        lib.recalgo_flen_fwd(_p(t["x"]), gp, _p(t["r_mf"]), _p(t["r_fm"]), _p(t["bias"]), cd, B, F, M, K, _p(e), _p(h), st)
        grads = {"dr_mf": torch.empty(P, device=dev), "dr_fm": torch.empty(M, device=dev), "dbias": torch.empty(K, device=dev)}
        dx = torch.empty(B, F * K, device=dev)
        ws = ops._workspace(nbytes, torch.device(dev))
        lib.recalgo_flen_bwd(_p(t["g_e"]), _p(t["g_h"]), _p(t["x"]), gp, _p(t["r_mf"]), _p(t["r_fm"]), cd, B, F, M, K, _p(dx),
                             _p(grads["dr_mf"]), _p(grads["dr_fm"]), _p(grads["dbias"]), _p(ws), st)
        wsf = _workspace_of(g)
        assert wsf.numel() == max(nbytes // 4, 4)
        _assert_outputs_are_the_sums(wsf, rows, grads, f"flen_bwd {name} B={B}")
        assert set(ENTRIES) <= g.launched
        _judge(dict(grads, e=e, h=h, dx=dx), r64, r32, f"the C entries {name} B={B}")
    del keepalive, keep


@pytest.mark.parametrize("B,F,M,K", [(4, 1, 2, 8), (4, 65, 2, 8), (4, 7, 1, 8), (4, 9, 9, 8), (4, 3, 4, 8), (4, 7, 3, 6), (4, 7, 3, 68),
                                     (4, 7, 3, 0), (0, 7, 3, 8)])
def test_shapes_outside_the_domain_are_refused(dev, B, F, M, K, monkeypatch):
    """the op raises, the ABI returns hipErrorInvalidValue, the queries return 0 and nothing is launched"""
    from tests.redzone import guarded
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device=dev)               # noqa: E731
    Bz, Kz, P = max(B, 1), max(K, 4), max(M * (M - 1) // 2, 1)
    groups = tuple(f % max(M, 1) for f in range(F))
    keepalive, gp = _groups(groups)
    x, r_mf, r_fm, bias = z(Bz, F * Kz), z(P), z(M), z(Kz)
    e, h, ws = z(Bz, M * Kz), z(Bz, Kz), z(1024)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.recalgo_flen_bwd_partial_rows(B, F, M, K) == 0 and lib.recalgo_flen_bwd_workspace_bytes(B, F, M, K) == 0
    if B > 0:
        assert lib.recalgo_flen_supported(F, M, K) == 0
    with guarded() as g:
        with pytest.raises(_lib.RecalgoError, match="recalgo_flen_fwd failed with hipError_t=1$"):
            lib.recalgo_flen_fwd(_p(x), gp, _p(r_mf), _p(r_fm), _p(bias), None, B, F, M, K, _p(e), _p(h), st)
        with pytest.raises(_lib.RecalgoError, match="recalgo_flen_bwd failed with hipError_t=1$"):
            lib.recalgo_flen_bwd(_p(e), _p(h), _p(x), gp, _p(r_mf), _p(r_fm), None, B, F, M, K, _p(torch.zeros_like(x)), _p(z(P)), _p(z(M)),
                                 _p(z(Kz)), _p(ws), st)
        assert not (set(ENTRIES) & g.launched)
    calls = _count(monkeypatch)
    with pytest.raises(ValueError, match="the kernels serve|must be a non-empty"):
        ops.flen_interaction(x[:B] if B == 0 else x, F, groups, r_mf if M > 1 else r_mf[:0], r_fm, bias if K else bias[:0])
    assert calls == {n: 0 for n in ENTRIES}
    del keepalive


def test_every_other_refusal_of_the_header(dev, monkeypatch):
    """a group index outside [0, M), an empty group, a NULL operand (dice excepted), misalignment (16 bytes for x, dx, e, g_e, h,
    g_h and an explicit mask, 4 for the small vectors), a Dicefactor rate outside (0, 1): hipErrorInvalidValue, nothing launched.
    (Arguments checked on the host; every pointer is a valid one or NULL.)"""
    from tests.redzone import guarded
    lib = _lib.load()
    B, F, M, K, groups = MID
    P = M * (M - 1) // 2
    v, _, _ = R.case(*MID, masked=True)
    t = _dev(v, dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keepalive, gp = _groups(groups)
    z = lambda *s: torch.zeros(*s, device=dev)               # noqa: E731
    e, h, dx, d_mf, d_fm, d_b = z(B, M * K), z(B, K), z(B, F * K), z(P), z(M), z(K)
    ws = z(int(lib.recalgo_flen_bwd_workspace_bytes(B, F, M, K)) // 4)
    wide = z(B * F * K + 4)                                   # a 16-byte operand one float off: a view into a larger buffer
    narrow = z(2 * K + 2).view(torch.uint8)[2:]               # a 4-byte operand two bytes off
    Drop = _lib.STRUCTS["recalgo_dropout_t"]

    def fwd(**o):
        a = dict(x=_p(t["x"]), g=gp, r_mf=_p(t["r_mf"]), r_fm=_p(t["r_fm"]), bias=_p(t["bias"]), dice=None, e=_p(e), h=_p(h))
        a.update(o)
        return lib.recalgo_flen_fwd(a["x"], a["g"], a["r_mf"], a["r_fm"], a["bias"], a["dice"], B, F, M, K, a["e"], a["h"], st)

    def bwd(**o):
        a = dict(g_e=_p(t["g_e"]), g_h=_p(t["g_h"]), x=_p(t["x"]), g=gp, r_mf=_p(t["r_mf"]), r_fm=_p(t["r_fm"]), dice=None, dx=_p(dx),
                 d_mf=_p(d_mf), d_fm=_p(d_fm), d_b=_p(d_b), ws=_p(ws))
        a.update(o)
        return lib.recalgo_flen_bwd(a["g_e"], a["g_h"], a["x"], a["g"], a["r_mf"], a["r_fm"], a["dice"], B, F, M, K, a["dx"], a["d_mf"],
                                    a["d_fm"], a["d_b"], a["ws"], st)
    refused = lambda: pytest.raises(_lib.RecalgoError, match="hipError_t=1$")     # noqa: E731
    with guarded() as g:
        for fn, names16, names4 in ((fwd, ("x", "e", "h"), ("r_mf", "r_fm", "bias")),
                                    (bwd, ("g_e", "g_h", "x", "dx"), ("r_mf", "r_fm", "d_mf", "d_fm", "d_b", "ws"))):
            for bad in ((0, 1, 0, 1, 3, 2, 1), (0, 1, 0, 1, -1, 2, 1), (0, 1, 0, 1, 1, 1, 1), (1, 1, 2, 1, 2, 2, 1)):
                ka, bp = _groups(bad)
                with refused():
                    fn(g=bp)
            for n in names16 + names4 + ("g",):
                with refused():
                    fn(**{n: None})
            for n in names16:
                with refused():
                    fn(**{n: ctypes.c_void_p(wide.data_ptr() + 4)})
            for n in names4:
                with refused():
                    fn(**{n: ctypes.c_void_p(narrow.data_ptr())})
            for rate in (0.0, 1.0, -0.25, 2.0):
                d = Drop(rate, None, 5, 0, None)
                with refused():
                    fn(dice=ctypes.byref(d))
            d = Drop(0.3, t["keep"].data_ptr() + 4, 5, 0, None)
            with refused():
                fn(dice=ctypes.byref(d))
        assert not (set(ENTRIES) & g.launched)
    calls = _count(monkeypatch)
    for bad in ((0, 1, 0, 1, 3, 2, 1), (0, 1, 0, 1, 1, 1, 1)):
        with pytest.raises(ValueError, match="group_of must map"):
            ops.flen_interaction(t["x"], F, bad, t["r_mf"], t["r_fm"], t["bias"])
    with pytest.raises(ValueError, match=r"rate must lie in \(0, 1\)"):
        ops.flen_interaction(t["x"], F, groups, t["r_mf"], t["r_fm"], t["bias"], dice=ops.DropSpec(1.0, None, 1, 0, None))
    with pytest.raises(ValueError, match="explicit keep mask"):
        ops.flen_interaction(t["x"], F, groups, t["r_mf"], t["r_fm"], t["bias"], dice=ops.DropSpec(0.3, t["keep"][:, :2].contiguous(), 1, 0, None))
    assert calls == {n: 0 for n in ENTRIES}
    del keepalive


def test_dicefactor_over_too_many_path_components_is_refused(dev):
    """B (P + M) K >= 2^32 with dice: refused on the host arguments (the operands are small, valid buffers: nothing reads them)"""
    from tests.redzone import guarded
    lib = _lib.load()
    F, M, K, groups = 7, 3, 8, R.DATASET_GROUPS
    B = -(-(1 << 32) // 48)
    z = lambda *s: torch.zeros(*s, device=dev)               # noqa: E731
    keepalive, gp = _groups(groups)
    d = _lib.STRUCTS["recalgo_dropout_t"](0.3, None, 5, 0, None)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    small = z(64)
    with guarded() as g:
        with pytest.raises(_lib.RecalgoError, match="hipError_t=1$"):
            lib.recalgo_flen_fwd(_p(small), gp, _p(small), _p(small), _p(small), ctypes.byref(d), B, F, M, K, _p(small), _p(small), st)
        with pytest.raises(_lib.RecalgoError, match="hipError_t=1$"):
            lib.recalgo_flen_bwd(_p(small), _p(small), _p(small), gp, _p(small), _p(small), ctypes.byref(d), B, F, M, K, _p(small), _p(small),
                                 _p(small), _p(small), _p(small), st)
        assert not (set(ENTRIES) & g.launched)
    del keepalive


def test_two_runs_and_three_replays_give_the_same_bits(dev):
    """forward + backward with Dicefactor on the hash, the step counter held fixed: eagerly twice, once on a side stream (the
    warm-up a capture needs), captured and replayed three times"""
    B, F, M, K, groups = 300, 7, 3, 12, R.SHAPES["three_lanes"][4]
    v = R.inputs(B, F, M, K, groups)
    t = _dev(v, dev)
    x = t["x"].requires_grad_(True)
    ws = [t[k].requires_grad_(True) for k in WEIGHTS]
    step = torch.full((1,), 7, dtype=torch.int64, device=dev)
    d = _spec(dev, B, M, K, step=step)

    def run():
        e, h = ops.flen_interaction(x, F, groups, *ws, dice=d)
        return [e.detach(), h.detach()] + list(torch.autograd.grad([e, h], [x] + ws, [t["g_e"], t["g_h"]]))
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
    step += 1                                                 # the captured launches read the counter: a new mask per replay
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(captured[1], first[1]) and torch.equal(captured[0], first[0])


@pytest.mark.parametrize("name", ["dataset", "interleaved", "singletons"])
def test_the_layer_on_a_store_fused_and_composed(dev, name, monkeypatch):
    """nn.field_wise_bi_interaction on a store of its own: fused=True is one entry each way and bit for bit ops.flen_interaction
    on the same values; fused=False launches neither and is in parity with the restatement, and with the kernels, with and
    without an injected mask; None picks the kernels; not training applies no Dicefactor."""
    B, F, M, K, groups = R.SHAPES[name]
    store = VariableStore(dev, seed=3)
    with use_store(store):
        store.building = True
        e0, h0 = nn.field_wise_bi_interaction(torch.zeros(B, F * K, device=dev), groups, R.RATE, True)
        assert tuple(e0.shape) == (B, M * K) and tuple(h0.shape) == (B, K)
        store.finalize()
    assert sorted(store.vars) == ["bias", "r_fm", "r_mf"]
    calls = _count(monkeypatch)
    for masked in (False, True):
        v, r64, r32 = R.case(B, F, M, K, groups, masked=masked)
        t = _dev(v, dev)
        for n in WEIGHTS:
            store.vars[n].data.copy_(t[n])
        got = {}
        for fused in (True, False, None):
            before = dict(calls)
            x = t["x"].clone().requires_grad_(True)
            nn.DROPOUT_KEEP_MASKS[:] = [v["keep"]] if masked else []
            try:
                with use_store(store):
                    store.begin_call()
                    e, h = nn.field_wise_bi_interaction(x, groups, R.RATE if masked else 0.0, True, fused=fused)
                    torch.autograd.backward([e, h], [t["g_e"], t["g_h"]])
                    ops.flush_dense_splits()
                assert not nn.DROPOUT_KEEP_MASKS
            finally:
                nn.DROPOUT_KEEP_MASKS[:] = []
            n_ = 0 if fused is False else 1
            assert calls == {k: before[k] + n_ for k in ENTRIES}, fused
            got[fused] = {"e": e.detach(), "h": h.detach(), "dx": x.grad, **{GRADS[n]: store.vars[n].grad.clone() for n in WEIGHTS}}
            _judge(got[fused], r64, r32, f"nn.field_wise_bi_interaction {name} fused={fused} masked={masked}:")
        plain = run_op(dev, v, groups, dice=_spec(dev, B, M, K, mask=v["keep"]) if masked else None)
        for k in R.NAMES:
            assert_bit_exact(got[True][k], plain[k], f"the layer against the op, {k}")
            assert_bit_exact(got[None][k], plain[k], f"fused=None against the op, {k}")
            assert_close(got[False][k], got[True][k].cpu().double(), what=f"composed against fused {name} {k}", reduced=k in R.REDUCED)
    # not training: no Dicefactor, no mask consumed, on either path
    v, r64, r32 = R.case(B, F, M, K, groups)
    for fused in (True, False):
        with use_store(store), torch.no_grad():
            store.begin_call()
            e, h = nn.field_wise_bi_interaction(t["x"], groups, R.RATE, False, fused=fused)
        assert_close(h, r64["h"], what=f"not training, fused={fused}, h", ref32=r32["h"])
    with pytest.raises(ValueError, match=r"fused=True\): no fused kernel serves"):
        with use_store(VariableStore(dev)) as s2:
            s2.building = True
            nn.field_wise_bi_interaction(torch.zeros(4, 3 * 6, device=dev), (0, 1, 0), fused=True)
            s2.finalize()
            nn.field_wise_bi_interaction(torch.zeros(4, 3 * 6, device=dev), (0, 1, 0), fused=True)


def test_the_composed_path_draws_the_hash_mask_the_kernels_draw(dev):
    """Dicefactor on the hash stream (no injected mask): the composed path takes its mask from ops.dropout_keep_mask with the
    spec the kernels get, so both paths drop the same path components"""
    B, F, M, K, groups = R.SHAPES["dataset"]
    store = VariableStore(dev, seed=3)
    with use_store(store):
        store.building = True
        nn.field_wise_bi_interaction(torch.zeros(B, F * K, device=dev), groups, R.RATE, True)
        store.finalize()
    v = R.inputs(B, F, M, K, groups)
    t = _dev(v, dev)
    for n in WEIGHTS:
        store.vars[n].data.copy_(t[n])
    hs = []
    for fused in (True, False):
        with use_store(store), torch.no_grad():
            store.begin_call()
            hs.append(nn.field_wise_bi_interaction(t["x"], groups, R.RATE, True, fused=fused)[1])
    assert_close(hs[1], hs[0].cpu().double(), what="composed against fused, the hash's mask, h")
    plain = R.reference(v, groups, torch.float64)["h"]
    assert float((hs[0].cpu().double() - plain).abs().max()) > 1e-3, "Dicefactor was applied"


# ---- the model ---------------------------------------------------------------------------------------------------------------------
from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig  # noqa: E402
from tests import golden_util as GU  # noqa: E402
from tests.test_flen_host import FLAG_DEFAULTS, TWO_GROUPS, expected_variables, flen_setup  # noqa: E402
from tests.test_mmoe_host import encode  # noqa: E402


def _redraw(est, seed=16):
    """Tables of order 0.5 (the field-wise embeddings of order 1), r_mf as 1 + 0.3 N(0, 1), r_fm as 0.5 + 0.2 N(0, 1), a bias of
    order 0.3, the logit kernels larger, so that h tells the rows apart; BatchNorm's moving statistics stay."""
    arrays = est.store.named_arrays()
    gen = torch.Generator().manual_seed(seed)
    for k, v in arrays.items():
        if k == "fwbi_part/r_mf":
            v.copy_(1.0 + 0.3 * torch.randn(*v.shape, generator=gen))
        elif k == "fwbi_part/r_fm":
            v.copy_(0.5 + 0.2 * torch.randn(*v.shape, generator=gen))
        elif k == "fwbi_part/bias":
            v.copy_(0.3 * torch.randn(*v.shape, generator=gen))
        elif k.endswith("/embedding_weights"):
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.5)
        elif k.endswith("_logit/kernel"):
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.3)
    return arrays


def _on_device(dev, tmp_path, **flags):
    """-> (estimator, params, device features, device labels) of the model on the 48 rows of the shared string batch"""
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = flen_setup(vocab_dir, **dict(dict(hidden_units="32,16"), **flags))
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, use_hip_graph=False))
    est.build(feats, lab)
    return est, params, *est._to_device(feats, lab)


def _masks(params, M, K=8, B=48, seed=5):
    """the keep masks of one TRAIN call in call order: Dicefactor's [B, P + M, K], then one per hidden layer"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    if params["dicefactor_rate"] > 0:
        out.append((torch.rand(B, M * (M - 1) // 2 + M, K, generator=gen) >= params["dicefactor_rate"]).float())
    if params["dropout_rate"] > 0:
        out += [(torch.rand(B, int(u), generator=gen) >= params["dropout_rate"]).float() for u in params["hidden_units"]]
    return out


def _oracle(params, variables, dtype, masks):
    sfeats, labels = GU.string_batch()
    P = {k: v.clone().to(dtype).requires_grad_(not k.split("/")[-1].startswith("moving_")) for k, v in variables.items()}
    feats = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in encode(params, sfeats).items()}
    lab = {"read_comment": labels.to(dtype)}
    with torch.no_grad():
        predict = R.flen(P, feats, None, params, training=False)
        evaluate = R.flen(P, feats, lab, params, training=False)
    out = R.flen(P, feats, lab, params, training=True, dropout_masks=[m.to(dtype) for m in masks])
    out["loss"].backward()
    return {"predict": predict, "eval_loss": evaluate["loss"], "loss": out["loss"].detach(), "P": P}


@pytest.mark.parametrize("groups,M", [(FLAG_DEFAULTS["field_groups"], 3), (TWO_GROUPS, 2)], ids=["default groups", "two groups"])
def test_the_model_follows_the_fp64_restatement(dev, groups, M, tmp_path, monkeypatch):
    """The dataset's columns (F = 7, embedding_dim 8), hidden 32,16 with BatchNorm, Dicefactor 0.3 and MLP dropout 0.2, every mask
    injected through nn.DROPOUT_KEEP_MASKS in call order: PREDICT, EVAL's loss (neither applies Dicefactor nor consumes a mask),
    the TRAIN loss, every gradient and one Adam step against tests/flen_ref.flen in float64, with the floor of the float32
    restatement's own deviation (golden_protocol.judge_step_against_oracle).  A TRAIN step launches each entry once."""
    from tests.golden_protocol import judge_step_against_oracle
    est, params, feats, lab = _on_device(dev, tmp_path, field_groups=groups, dicefactor_rate=0.3, dropout_rate=0.2)
    arrays = _redraw(est)
    want = expected_variables(params, M)
    assert sorted(k for k in arrays if not k.endswith("/embedding_weights")) == sorted(want)
    variables = {k: v.detach().cpu().double() for k, v in arrays.items()}
    before = {k: v.clone() for k, v in variables.items()}
    masks = _masks(params, M)
    assert len(masks) == 3
    r64, r32 = _oracle(params, variables, torch.float64, masks), _oracle(params, variables, torch.float32, masks)
    p = r64["predict"]["prob"]
    assert float(p.max() - p.min()) > 0.05, "the redrawn variables tell the rows apart"
    calls = _count(monkeypatch)
    what = f"flen M={M}"
    nn.DROPOUT_KEEP_MASKS[:] = list(masks)
    try:
        with torch.no_grad():
            pr = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
        assert len(nn.DROPOUT_KEEP_MASKS) == 3, "PREDICT and EVAL drop nothing"
        assert calls == {ENTRIES[0]: 2, ENTRIES[1]: 0}
        assert list(pr.predictions) == ["logit", "probabilities"]
        assert_close(pr.predictions["probabilities"], r64["predict"]["prob"], what=f"{what} predict", ref32=r32["predict"]["prob"])
        assert_close(pr.predictions["logit"], r64["predict"]["logit"], what=f"{what} logit", ref32=r32["predict"]["logit"])
        assert_close(ev.loss, r64["eval_loss"], what=f"{what} eval loss", ref32=r32["eval_loss"])
        spec = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
        assert not nn.DROPOUT_KEEP_MASKS, "TRAIN consumed Dicefactor's mask and the two hidden layers'"
    finally:
        nn.DROPOUT_KEEP_MASKS[:] = []
    assert_close(spec.loss, r64["loss"], what=f"{what} loss", ref32=r32["loss"])
    assert abs(float(r64["loss"]) - float(r64["eval_loss"])) > 1e-4, "the masks change the loss"
    n_min = 7 + 2 + 3 + 2 * (2 + 2) + 2                       # tables, dense_logit, the layer, two hidden layers with BatchNorm, flen_logit
    judge_step_against_oracle(est, spec, r64["P"], r32["P"], before, params["learning_rate"], what, n_min)
    assert calls == {ENTRIES[0]: 3, ENTRIES[1]: 1}


def test_three_steps_follow_the_fp64_restatement(dev, tmp_path):
    """3 eager Estimator.train_step calls on rotating sub-batches of the shared batch against the float64 restatement's own
    free-running trajectory, inside tests/trajectory_ref.bounds; the float32 restatement itself must sit below half of that
    bound for the test to be one of the kernels."""
    from oracle import ref_ops as O
    from tests import trajectory_ref as T
    N = 3
    est, params, _, _ = _on_device(dev, tmp_path)
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
            res = R.flen(P, feats, {"read_comment": lb.to(dtype)}, params, training=True, bn_state=bn_state)
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
        assert_close(l, l64, what=f"flen loss of step {k}", ref32=l32)
    assert int(est.store.opt_state["step"]) == N
    after = est.store.named_arrays()
    assert len(r64["trainable"]) == 7 + 2 + 3 + 2 * (2 + 2) + 2
    wk, wherek, outk = T.worst_ratio({k: after[k] for k in r64["trainable"]}, r64, bnd)
    print(f"flen: worst |p - p64| / tol after {N} steps: kernels {wk:.3f} ({wherek}) | fp32 restatement {w32:.3f} ({where32})")
    assert wk <= 1.0, f"flen: {wherek} is {wk:.3f} x the bound after {N} steps (fp32 restatement: {w32:.3f} at {where32})"
    for k in outk:
        assert outk[k] <= 1.5 * out32[k] + 10, f"flen {k}: {outk[k]} elements outside the tight bound, the fp32 restatement leaves {out32[k]}"


# ---- captured training ---------------------------------------------------------------------------------------------------------------
def _synthetic(dev, B=256, fields=8, K=8, seed=42, **run):
    """the model over synthetic device-resident features: 16 dense features and `fields` single-valued id columns in three field
    groups, Dicefactor 0.1 on the hash"""
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    from recalgorithm_amd.algorithm.FLEN.flen import flen_model_fn
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=fields, max_vocab=500, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES],
              "category_feature_columns": [fc.embedding_column(c, K) for c in cats], "embedding_dim": K,
              "field_groups": [list(spec.names[0::3]), list(spec.names[1::3]), list(spec.names[2::3])], "hidden_units": [32, 16],
              "batch_norm": True, "dropout_rate": 0.0, "dicefactor_rate": 0.1, "learning_rate": 0.005}
    est = Estimator(model_fn=flen_model_fn, params=params, config=RunConfig(device=dev, seed=seed, **run))
    feats, labels, _ = synth.device_features(spec, B, dev, batch_index=0)
    est.build(feats, labels)
    return est, spec


def test_captured_step_replays_what_eager_steps_compute(dev, monkeypatch):
    """three hipGraph replays of the captured step (B 256, 8 single-valued columns, Dicefactor 0.1 on the hash: the mask follows
    the device step counter, so replays and eager steps draw the same masks) against eager launches on rotating batches, bit for
    bit (tests/test_gpu_replay_models.py's comparison)"""
    from recalgorithm_amd.estimator import GraphedTrainStep, _tree_tensors
    from recalgorithm_amd.io import synth
    from tests.test_gpu_replay_models import _differences, _state
    WARMUP, STEPS, N_BATCHES = 3, 3, 3
    calls = _count(monkeypatch)
    (eager, spec), (graphed, _) = _synthetic(dev), _synthetic(dev)
    batches = [synth.device_features(spec, 256, dev, batch_index=i)[:2] for i in range(N_BATCHES)]
    keep = [[t.clone() for _, t in _tree_tensors({"f": b[0], "l": b[1]}, "b")] for b in batches]
    for _ in range(WARMUP):
        eager.train_step(*batches[0])
    le = [eager.train_step(*batches[i % N_BATCHES]).clone() for i in range(STEPS)]
    assert calls == {n: WARMUP + STEPS for n in ENTRIES}
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
    """(model_fn, params, four host batches of the 48 shared rows: 0 .. 2 with rolled rows and cut bags, 3 the rows themselves);
    Dicefactor 0.1 on the hash"""
    from tests.test_gpu_ragged import _encoded, _roll_cut
    if not _bag_model:
        vocab_dir = GU.write_vocab_dir(str(tmp_path_factory.mktemp("flen") / "vocabulary"))
        model_fn, params = flen_setup(vocab_dir, hidden_units="32,16", dicefactor_rate=0.1)
        base = _encoded(params)
        _bag_model["m"] = (model_fn, params, [_roll_cut(*base, s, keep) for s, keep in ((5, 3), (11, 2), (17, 4))] + [_roll_cut(*base, 0, 8)])
    return _bag_model["m"]


def test_captured_steps_with_the_bag_are_the_eager_steps(dev, tmp_path_factory):
    """the dataset's columns with the manual_tag_list bag under ragged_capacity, Dicefactor on the hash, no model-specific code: two
    eager warm-up steps, the capture, three replays — losses and variables bit for bit those of eager steps"""
    from tests.test_gpu_ragged import _assert_same_run, _nnz, _steps, _to
    model_fn, params, batches = _bag_batches(tmp_path_factory)
    assert params["dicefactor_rate"] == 0.1
    assert set(_nnz(batches[3])) == {"manual_tag_list"}
    caps = {"manual_tag_list": -(-max(_nnz(b)["manual_tag_list"] for b in batches) // 48)}
    sequence = [batches[i] for i in (0, 1, 2, 3, 0, 1)]
    place = lambda b: _to(b, dev)                            # noqa: E731
    eager = _steps(dev, model_fn, params, sequence, place, use_hip_graph=True, ragged_capacity=None)
    assert eager[0].graph_replays == 0
    graphed = _steps(dev, model_fn, params, sequence, place, use_hip_graph=True, ragged_capacity=caps)
    est = graphed[0]
    assert est.capture_refused is None and est.ragged_overflows == 0 and est.graph_replays == 6 - 2 - 1
    _assert_same_run(graphed, eager, f"flen, ragged_capacity={caps}")


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
    est, params, feats, lab = _on_device(dev, tmp_path, dicefactor_rate=0.1)
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
