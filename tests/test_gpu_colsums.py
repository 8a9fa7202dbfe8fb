"""-m gpu: the determinism contract of every two-pass backward, at the C ABI.

Each workgroup of a backward kernel leaves one partial row; a second pass adds the rows of each column in ONE fixed order
(csrc/slab_sum.h: sixteen interleaved sums of the rows g, g + 16, .., then the sixteen in order), which
tests/dense_ref.colsum_fixed_order restates in fp32 on the CPU.

  * the outputs ARE that sum of the workspace's partial rows, bit for bit, for every entry whose header states the partial-row
    layout and leaves the workspace readable: bst_attn_bwd, bst_ffn_bwd, dien_gru_bwd, dien_evolve_bwd, cross_bwd
    (defer_reduce = 0) and din_attention_bwd, at 1, 3, 17 (one row group with a second row) and cap (from cap + 5 workgroups'
    worth of examples, clamped) partial rows;
  * the immediate second pass (the entry's own) and the deferred one (the same recalgo_colsum_t jobs through
    recalgo_dense_bwd_weights_reduce, as a training step runs them) give the same bits: cross_bwd and din_attention_bwd.

Every buffer is a guarded, poisoned allocation of tests/redzone.py."""
import ctypes
import math

import pytest
import torch

from recalgorithm_amd import _lib
from tests import bst_ref, dien_ref
from tests import test_gpu_bst as bst
from tests import test_gpu_dien as dien
from tests.dense_ref import colsum_fixed_order
from tests.redzone import guarded
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu

ROW_COUNTS = ("1", "3", "17", "cap")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _workspace_of(g):
    """the workspace the last backward entry under the guard `g` was given, as floats"""
    return [r for r in g.records if r.kind == "workspace"][-1].body.view(torch.float32)


def _assert_outputs_are_the_sums(ws, rows, outs, what):
    """outs: the gradients in the order of the partial row's layout; the row is exactly as long as they are together"""
    width = sum(o.numel() for o in outs.values())
    ws = ws.cpu()
    assert ws.numel() >= rows * width, what
    off = 0
    for name, o in outs.items():
        want = colsum_fixed_order(ws[off:], rows, width, o.numel())
        assert_bit_exact(o.reshape(-1), want, f"{what} {name}: the fixed-order sum of {rows} partial rows")
        off += o.numel()


def _batch_for(partial_rows, want):
    """The batch size that yields `want` partial rows, from the entry's own query (no waves-per-workgroup constant here):
    'cap' is cap + 5 workgroups' worth of examples, which the entry clamps to cap."""
    per = next(B for B in range(1, 1 << 12) if partial_rows(B + 1) == 2)        # examples per workgroup
    cap = partial_rows(1 << 30)
    B, rows = ((cap + 5) * per, cap) if want == "cap" else (int(want) * per, int(want))
    assert partial_rows(B) == rows and math.ceil(B / per) == (cap + 5 if want == "cap" else rows)
    return B, rows


@pytest.mark.parametrize("B", (1, 3, 17, bst.CAP + 5))
def test_bst_outputs_are_the_fixed_order_sums(dev, B):
    T, d, H = 2, 4, 1
    case = bst_ref.random_case(B, T, d, H, seed=B)
    rows = min(B, bst.CAP)
    with guarded() as g:
        got = bst.run_attention(g, dev, case, B, T, d, H)
        outs = {"d" + k: got["d" + k] for k in bst_ref.ATTN_PARAMS}            # dpos | dw_q | dw_k | dw_v | dw_o | dgamma | dbeta
        _assert_outputs_are_the_sums(_workspace_of(g), rows, outs, f"bst_attn_bwd B={B}")
        n1 = torch.randn(B, T, d, generator=torch.Generator().manual_seed(B))
        got = bst.run_ffn(g, dev, case, n1, B, T, d, "mean", True, True)
        outs = {"d" + k: got["d" + k] for k in bst_ref.FFN_PARAMS}             # dw | db | dgamma | dbeta
        _assert_outputs_are_the_sums(_workspace_of(g), rows, outs, f"bst_ffn_bwd B={B}")


@pytest.mark.parametrize("B", (1, 3, 17, dien.CAP + 5))
def test_dien_outputs_are_the_fixed_order_sums(dev, B):
    T, na, nh = 2, 4, 4
    rows = min(B, dien.CAP)
    with guarded() as g:
        case = dien_ref.random_case(B, T, na, nh, dien_ref.GRU, seed=B)
        got = dien.run_gru(g, dev, case, B, T, na, nh)
        outs = {"d" + k: got["d" + k] for k in dien_ref.CELL_PARAMS}           # dWg | dbg | dWc | dbc
        _assert_outputs_are_the_sums(_workspace_of(g), rows, outs, f"dien_gru_bwd B={B}")
        case = dien_ref.random_case(B, T, na, nh, dien_ref.AUGRU, seed=B + 1)
        got = dien.run_evolve(g, dev, case, B, T, na, nh)
        outs = {k: got[k] for k in dien.EVOLVE_GRADS}                          # dw_att | dWg | dbg | dWc | dbc
        _assert_outputs_are_the_sums(_workspace_of(g), rows, outs, f"dien_evolve_bwd B={B}")


# ---- cross_bwd ------------------------------------------------------------------------------------------------------------------
CROSS_D, CROSS_L = 8, 2


def _run_cross(lib, dev, B, rows, defer):
    """-> (dw, db, workspace as floats): defer = 0 the entry's own second pass, 1 the two jobs the header names"""
    d, L = CROSS_D, CROSS_L
    gen = torch.Generator().manual_seed(B)
    x0, g = torch.randn(B, d, generator=gen).to(dev), torch.randn(B, d, generator=gen).to(dev)
    w, b = (torch.randn(L, d, generator=gen) / math.sqrt(d)).to(dev), (torch.randn(L, d, generator=gen) * 0.1).to(dev)
    dx0, dw, db = torch.empty(B, d, device=dev), torch.empty(L, d, device=dev), torch.empty(L, d, device=dev)
    nbytes = int(lib.recalgo_cross_bwd_workspace_bytes(B, d, L))
    assert nbytes == 4 * rows * 2 * L * d
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lib.recalgo_cross_bwd(_p(x0), d, _p(w), _p(b), _p(g), d, None, B, d, L, _p(dx0), None if defer else _p(dw), None if defer else _p(db),
                          _p(ws), defer, _st())
    if defer:
        colsum_t = _lib.STRUCTS["recalgo_colsum_t"]
        sums = (colsum_t * 2)(colsum_t(ws.data_ptr(), dw.data_ptr(), rows, 2 * L * d, L * d),
                              colsum_t(ws.data_ptr() + 4 * L * d, db.data_ptr(), rows, 2 * L * d, L * d))
        lib.recalgo_dense_bwd_weights_reduce((_lib.STRUCTS["recalgo_dense_split_t"] * 1)(), 0, sums, 2, None, _st())
    return dw, db, ws.view(torch.float32)


@pytest.mark.parametrize("want", ROW_COUNTS)
def test_cross_outputs_are_the_fixed_order_sums(dev, want):
    with guarded():
        lib = _lib.load()
        B, rows = _batch_for(lib.recalgo_cross_bwd_partial_rows, want)
        dw, db, ws = _run_cross(lib, dev, B, rows, defer=0)
        _assert_outputs_are_the_sums(ws, rows, {"dw": dw, "db": db}, f"cross_bwd B={B}")       # [dw_0 .. | db_0 ..]


@pytest.mark.parametrize("want", ROW_COUNTS)
def test_cross_immediate_equals_deferred(dev, want):
    with guarded():
        lib = _lib.load()
        B, rows = _batch_for(lib.recalgo_cross_bwd_partial_rows, want)
        dw, db, ws = _run_cross(lib, dev, B, rows, defer=0)
        dw1, db1, ws1 = _run_cross(lib, dev, B, rows, defer=1)
        assert_bit_exact(ws1, ws, f"cross_bwd B={B}: the partial rows, deferred against immediate")
        assert_bit_exact(dw1, dw, f"cross_bwd B={B} dw: deferred against immediate")
        assert_bit_exact(db1, db, f"cross_bwd B={B} db: deferred against immediate")


# ---- din_attention_bwd ------------------------------------------------------------------------------------------------------------
DIN_H, DIN_T = 4, 3
DIN_SHAPES = {"d_f1_w": (4 * DIN_H, 64), "d_f1_b": (64,), "d_f2_w": (64, 32), "d_f2_b": (32,), "d_f3_w": (32, 1), "d_f3_b": (1,)}


def _run_din(lib, dev, B, rows, defer):
    """-> ({name: gradient} in the partial row's order, workspace as floats): defer = 1 passes d_f1_w = NULL and sums the six
    runs of columns as six jobs"""
    H, T = DIN_H, DIN_T
    gen = torch.Generator().manual_seed(B)
    q, keys, g = torch.randn(B, H, generator=gen), torch.randn(B, T, H, generator=gen), torch.randn(B, H, generator=gen)
    lens = torch.randint(0, T + 1, (B,), generator=gen, dtype=torch.int32)
    lens[0] = T
    keys = keys * (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(-1)
    ws_ = [torch.randn(*s, generator=gen) / math.sqrt(s[0]) for s in DIN_SHAPES.values()]
    q, keys, g, lens, *ws_ = (t.to(dev) for t in (q, keys, g, lens, *ws_))
    dq, dk = torch.empty(B, H, device=dev), torch.empty(B, T, H, device=dev)
    grads = {k: torch.empty(*s, device=dev) for k, s in DIN_SHAPES.items()}
    pf = int(lib.recalgo_din_attention_bwd_partial_floats(H))
    assert pf == sum(t.numel() for t in grads.values())
    nbytes = int(lib.recalgo_din_attention_bwd_workspace_bytes(B, T, H))
    assert nbytes == 4 * rows * pf
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lib.recalgo_din_attention_bwd(_p(q), _p(keys), _p(lens), *[_p(t) for t in ws_], _p(g), B, T, H, 1, _p(dq), _p(dk),
                                  *[None if defer else _p(t) for t in grads.values()], _p(ws), _st())
    if defer:
        colsum_t = _lib.STRUCTS["recalgo_colsum_t"]
        sums, off = (colsum_t * 6)(), 0
        for i, t in enumerate(grads.values()):
            sums[i] = colsum_t(ws.data_ptr() + 4 * off, t.data_ptr(), rows, pf, t.numel())
            off += t.numel()
        lib.recalgo_dense_bwd_weights_reduce((_lib.STRUCTS["recalgo_dense_split_t"] * 1)(), 0, sums, 6, None, _st())
    return grads, ws.view(torch.float32)


@pytest.mark.parametrize("want", ROW_COUNTS)
def test_din_outputs_are_the_fixed_order_sums(dev, want):
    with guarded():
        lib = _lib.load()
        B, rows = _batch_for(lib.recalgo_din_attention_bwd_partial_rows, want)
        grads, ws = _run_din(lib, dev, B, rows, defer=0)
        _assert_outputs_are_the_sums(ws, rows, grads, f"din_attention_bwd B={B}")


@pytest.mark.parametrize("want", ROW_COUNTS)
def test_din_immediate_equals_deferred(dev, want):
    with guarded():
        lib = _lib.load()
        B, rows = _batch_for(lib.recalgo_din_attention_bwd_partial_rows, want)
        grads, ws = _run_din(lib, dev, B, rows, defer=0)
        grads1, ws1 = _run_din(lib, dev, B, rows, defer=1)
        assert_bit_exact(ws1, ws, f"din_attention_bwd B={B}: the partial rows, deferred against immediate")
        for k in grads:
            assert_bit_exact(grads1[k], grads[k], f"din_attention_bwd B={B} {k}: deferred against immediate")
