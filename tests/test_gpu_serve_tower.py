"""-m gpu: recalgo_serve_tower_fwd (include/recalgo_serve.h, csrc/serve.hip) at the C ABI.
  * the tower against tests/serve_ref.py in float64, `ref32` = the header's stated order restated in float32, at the project's
    bound (tests/util.assert_close, default factor and slack): B in {1, 15, 16, 17, 48}, K0 in {5, 48, 416, 1024}, the widths
    [16], [32, 16], [512, 256, 128], [512, 512, 512, 512] and two that give a wave three tiles or none, relu on every layer and
    mixed, with and without scale / shift, a layer without a bias;
  * a row's result does not depend on the batch, bit for bit;
  * every invalid call is refused with hipErrorInvalidValue before any launch: the poisoned `out` stays as it was;
  * the widest and the narrowest case once more between fenced, poisoned allocations (tests/redzone.py)."""
import ctypes
import functools

import pytest
import torch

from recalgorithm_amd import _lib, ops
from tests import serve_ref as R
from tests.redzone import guarded
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

ROWS = 16                   # rows of a workgroup of csrc/serve.hip: B = 16, 48 fill its tiles; 1, 15, 17 leave a partial one
# name -> (K0, units, relu_bits, layers with scale / shift, layers without a bias, the B to run)
CASES = {
    "narrowest": (5, [16], 0b1, {0}, set(), (1, 15, 16, 17, 48)),
    "two_layers_mixed": (48, [32, 16], 0b01, {0}, {1}, (1, 15, 16, 17, 48)),
    "bench_tower_bn": (416, [512, 256, 128], 0b111, {0, 1, 2}, set(), (1, 17, 48)),
    "bench_tower_plain": (416, [512, 256, 128], 0b111, set(), set(), (16,)),
    "widest": (1024, [512, 512, 512, 512], 0b1011, {0, 1, 3}, {2}, (15, 17)),
    "long_k_one_tile": (1024, [16], 0b1, set(), set(), (17,)),
    "k_tail_wide": (5, [512, 512, 512, 512], 0b1111, {0, 1, 2, 3}, set(), (48,)),
    "three_tiles_and_none": (48, [400, 48], 0b11, {1}, {0}, (15, 48)),      # 25 tiles: waves of 4 and 3; 3 tiles: waves of 1 and 0
    "odd_k": (417, [128], 0b0, {0}, set(), (17,)),                            # K0 % 4 != 0 on a K0 of more than one chunk
}
BMAX = 48
assert {b for c in CASES.values() for b in c[5]} == {1, 15, 16, 17, 48}
assert {c[0] for c in CASES.values()} >= {5, 48, 416, 1024}
assert all(any(c[1] == u for c in CASES.values()) for u in ([16], [32, 16], [512, 256, 128], [512] * 4))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _table(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(x [48, K0], layers, float64 result, float32 result in the header's order): once per case, rows shared by every B"""
    K0, units, relu_bits, scaled, nobias, _ = CASES[name]
    x, layers = R.random_tower(BMAX, K0, units, relu_bits, scaled, nobias, seed=sum(map(ord, name)))
    return x, layers, R.tower64(x, layers), R.tower32(x, layers)


def _place(dev, layers, g=None):
    put = (lambda t: g.input(t.float(), dev)) if g is not None else (lambda t: t.float().to(dev))
    return [tuple(None if t is None else put(t) for t in ly[:4]) for ly in layers]


def run_tower(dev, x, layers, relu_bits, g=None, out=None):
    lib = _lib.load()
    xd = g.input(x.float(), dev) if g is not None else x.float().to(dev)
    dl = _place(dev, layers, g)
    units = [int(ly[0].shape[1]) for ly in layers]
    out = torch.full((x.shape[0], units[-1]), float("nan"), device=dev) if out is None else out
    lib.recalgo_serve_tower_fwd(_ptr(xd), *[_table([ly[i] for ly in dl]) for i in range(4)], (ctypes.c_int * len(units))(*units),
                                len(units), relu_bits, x.shape[0], x.shape[1], _ptr(out), _stream())
    return out


@pytest.mark.parametrize("name,B", [(n, b) for n, c in CASES.items() for b in c[5]])
def test_tower_at_the_abi_against_float64(dev, name, B):
    x, layers, r64, r32 = _reference(name)
    K0, units, relu_bits = CASES[name][:3]
    out = run_tower(dev, x[:B], layers, relu_bits)
    assert_close(out, r64[:B], what=f"{name} B={B} K0={K0} units={units}", ref32=r32[:B])
    # the wrapper of ops.py launches the same entry on the same arguments
    dl = _place(dev, layers)
    got = ops.serve_tower(x[:B].float().to(dev), [ly + (bool((relu_bits >> l) & 1),) for l, ly in enumerate(dl)])
    assert_bit_exact(got, out, f"{name} B={B}: ops.serve_tower against the entry point")


@pytest.mark.parametrize("name", ["bench_tower_bn", "two_layers_mixed", "k_tail_wide"])
def test_a_row_does_not_depend_on_the_batch(dev, name):
    x, layers, _, _ = _reference(name)
    relu_bits = CASES[name][2]
    full = run_tower(dev, x, layers, relu_bits)
    assert_bit_exact(run_tower(dev, x, layers, relu_bits), full, f"{name}: two runs")
    for i in (0, 15, 16, 47):
        assert_bit_exact(run_tower(dev, x[i:i + 1], layers, relu_bits)[0], full[i], f"{name}: row {i} alone against row {i} of B = 48")
    assert_bit_exact(run_tower(dev, x[16:33], layers, relu_bits), full[16:33], f"{name}: rows 16..32 as a batch of 17")


def test_unaligned_x_takes_the_four_byte_arm_with_the_same_bits(dev):
    x, layers, _, _ = _reference("two_layers_mixed")                      # K0 = 48: the 16-byte arm when x is aligned
    relu_bits = CASES["two_layers_mixed"][2]
    aligned = run_tower(dev, x[:17], layers, relu_bits)
    with guarded() as g:
        lib = _lib.load()
        xs = g.input(x[:17].float(), dev, shifted=True)
        dl = _place(dev, layers, g)
        out = torch.empty(17, 16, device=dev)
        lib.recalgo_serve_tower_fwd(_ptr(xs), *[_table([ly[i] for ly in dl]) for i in range(4)], (ctypes.c_int * 2)(32, 16), 2, relu_bits,
                                    17, 48, _ptr(out), _stream())
        assert_bit_exact(out, aligned, "x one element off 16 bytes")


@pytest.mark.parametrize("name,B", [("widest", 17), ("narrowest", 17), ("narrowest", 1)])
def test_between_fenced_poisoned_allocations(dev, name, B):
    x, layers, r64, r32 = _reference(name)
    with guarded() as g:
        out = run_tower(dev, x[:B], layers, CASES[name][2], g=g, out=torch.empty(B, CASES[name][1][-1], device=dev))
        assert_close(out, r64[:B], what=f"guarded {name} B={B}", ref32=r32[:B])
        assert "recalgo_serve_tower_fwd" in g.launched


def test_invalid_calls_are_refused_before_any_launch(dev):
    x, layers, _, _ = _reference("two_layers_mixed")
    K0, units, relu_bits = CASES["two_layers_mixed"][:3]
    B, L = 17, 2
    with guarded() as g:
        lib = _lib.load()
        xd = g.input(x[:B].float(), dev)
        dl = _place(dev, [(w, b if b is not None else torch.zeros(w.shape[1]), s if s is not None else torch.ones(w.shape[1]),
                           t if t is not None else torch.zeros(w.shape[1])) for w, b, s, t, _ in layers], g)
        W, Bv, S, T = ([ly[i] for ly in dl] for i in range(4))
        out = torch.empty(B, 512, device=dev)                                 # poisoned: 0xFF.. is a NaN
        ints = lambda *u: (ctypes.c_int * len(u))(*u)                         # noqa: E731
        off2 = lambda t: ctypes.c_void_p(t.data_ptr() + 2)                    # noqa: E731
        entry2 = lambda ts, i: (ctypes.c_void_p * L)(*[t.data_ptr() + (2 if j == i else 0) for j, t in enumerate(ts)])      # noqa: E731
        good = [_ptr(xd), _table(W), _table(Bv), _table(S), _table(T), ints(*units), L, relu_bits, B, K0, _ptr(out)]

        def refused(**change):
            a = list(good)
            for i, v in change.items():
                a[int(i[1:])] = v
            with pytest.raises(_lib.RecalgoError, match="recalgo_serve_tower_fwd failed with hipError_t=1$"):
                lib.recalgo_serve_tower_fwd(*a, _stream())
        for bad_units in ((32, 8), (32, 24), (528, 16), (0, 16), (32, -16)):
            refused(_5=ints(*bad_units))
        refused(_6=0)
        refused(_6=5, _5=ints(32, 32, 32, 32, 16))
        refused(_9=0)
        refused(_9=1025)
        refused(_8=0)
        refused(_8=-3)
        for i in (0, 1, 5, 10):                                               # x, w, units, out
            refused(**{f"_{i}": None})
        refused(_1=_table([W[0], None]))                                      # a NULL kernel
        refused(_4=_table([None, T[1]]))                                      # a scale without its shift
        refused(_4=None)
        refused(_0=off2(xd))
        refused(_10=off2(out))
        for i, ts in ((1, W), (2, Bv), (3, S), (4, T)):
            refused(**{f"_{i}": entry2(ts, 1)})
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a refused call wrote out"
        assert "recalgo_serve_tower_fwd" not in g.launched
        # and the same arguments unchanged are served
        lib.recalgo_serve_tower_fwd(*good, _stream())
        assert "recalgo_serve_tower_fwd" in g.launched
    xd = torch.zeros(4, 48, device=dev)
    w = lambda k, n: torch.zeros(k, n, device=dev)                            # noqa: E731
    with pytest.raises(ValueError, match="the kernel serves"):
        ops.serve_tower(xd, [(w(48, 24), None, None, None, True)])
    with pytest.raises(ValueError, match="its input has 32 columns"):
        ops.serve_tower(xd, [(w(48, 32), None, None, None, True), (w(48, 16), None, None, None, True)])
    with pytest.raises(ValueError, match="scale without a shift"):
        ops.serve_tower(xd, [(w(48, 32), None, torch.ones(32, device=dev), None, True)])
