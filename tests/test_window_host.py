"""tests/window.py on the CPU: the frame would fail a wrong kernel, and the table of strided ABI parameters is complete.

The stand-ins below are torch-only "kernels" over CPU frames: one correct, four with a planted fault of the kind a strided
operand invites (a write one column past the window, the window written at column 0, the input read from column 0, the last
row skipped).  Every fault must be caught by the same assertions tests/test_gpu_windows.py makes; the correct one passes.
"""
import importlib

import pytest
import torch

from recalgorithm_amd import _abi, _lib
from tests import window
from tests.util import assert_bit_exact, assert_close
from tests.window import Frame

ROWS, W = 7, 6
# (stride, col): a gap on both sides; col = 0; flush against the right edge (col + width == stride); odd stride and column
PLACES = [(W + 4, 2), (W + 3, 0), (W + 5, 5), (W + 3, 1), (W, 0)]


# ---- the stand-ins: out[r, :] = 2 * x[r, :] (fp32), out[r, :] = table[ids[r, :]] (int64 ids) ------------------------------------
def _rows(buf, base, rows, stride):
    return buf[base:base + rows * stride].view(rows, stride)


def k_correct(x, out, op):
    out.window.copy_(op(x.window))


def k_one_column_past(x, out, op):
    k_correct(x, out, op)
    row = out.rows - 2
    flat = out.lead + row * out.stride + out.col + out.width            # (the right edge: column 0 of the next row)
    out.buf[flat] = 1


def k_window_at_column_0(x, out, op):
    out.full[:, :out.width].copy_(op(x.window))


def k_reads_column_0(x, out, op):
    out.window.copy_(op(x.full[:, :x.width]))


def k_skips_last_row(x, out, op):
    out.window[:-1].copy_(op(x.window[:-1]))


def k_writes_its_input(x, out, op):
    k_correct(x, out, op)
    x.window[0, 0] = 0


def _check(x, out, ref):
    """the assertions of tests/test_gpu_windows.py, in its order"""
    if out.dtype == torch.float32:
        assert_close(out.get(), ref.double(), what="window")
    assert_bit_exact(out.get(), ref, "window")
    out.assert_outside_untouched("out")
    x.assert_unchanged("x")


def _float_case(place_x, place_out):
    gen = torch.Generator().manual_seed(5)
    v = torch.randn(ROWS, W, generator=gen)
    x = Frame(ROWS, W, *place_x).put(v)
    out = Frame(ROWS, W, *place_out)
    return x, out, (lambda t: 2.0 * t), 2.0 * v


def _id_case(place_x, place_out):
    """an int64 id operand with a decoy in its gaps -> an int64 output: table[id], -1 skipped (0)"""
    gen = torch.Generator().manual_seed(6)
    table = torch.arange(100, 117, dtype=torch.int64)
    ids = torch.randint(-1, 16, (ROWS, W), generator=gen)
    op = lambda t: torch.where(t >= 0, table[t.clamp(min=0)], torch.zeros((), dtype=torch.int64))
    x = Frame(ROWS, W, *place_x, dtype=torch.int64, decoy=16).put(ids)
    out = Frame(ROWS, W, *place_out, dtype=torch.int64)
    return x, out, op, op(ids)


CASES = {"fp32": _float_case, "int64": _id_case}


@pytest.mark.parametrize("kind", sorted(CASES))
@pytest.mark.parametrize("place_out", PLACES)
@pytest.mark.parametrize("place_x", PLACES)
def test_a_correct_stand_in_passes(kind, place_x, place_out):
    x, out, op, ref = CASES[kind](place_x, place_out)
    k_correct(x, out, op)
    _check(x, out, ref)


@pytest.mark.parametrize("kind", sorted(CASES))
@pytest.mark.parametrize("place_out", PLACES[:-1])
def test_a_write_one_column_past_the_window_is_caught(kind, place_out):
    x, out, op, ref = CASES[kind](PLACES[0], place_out)
    k_one_column_past(x, out, op)
    with pytest.raises(AssertionError, match="written outside the window"):
        _check(x, out, ref)


@pytest.mark.parametrize("kind", sorted(CASES))
@pytest.mark.parametrize("place_out", [p for p in PLACES if p[1] != 0])
def test_the_window_written_at_column_0_is_caught(kind, place_out):
    x, out, op, ref = CASES[kind](PLACES[0], place_out)
    k_window_at_column_0(x, out, op)
    with pytest.raises(AssertionError):
        _check(x, out, ref)
    with pytest.raises(AssertionError, match="written outside the window"):     # both assertions see it, each alone
        out.assert_outside_untouched("out")


@pytest.mark.parametrize("kind", sorted(CASES))
@pytest.mark.parametrize("place_x", [p for p in PLACES if p[1] != 0])
def test_an_input_read_from_column_0_is_caught(kind, place_x):
    """fp32: the gap is NaN and reaches the result; int64: the gap is the decoy, a VALID id that changes it (-1 would be skipped)"""
    x, out, op, ref = CASES[kind](place_x, PLACES[0])
    k_reads_column_0(x, out, op)
    with pytest.raises(AssertionError, match="non-finite" if kind == "fp32" else "not bit-exact"):
        _check(x, out, ref)


@pytest.mark.parametrize("kind", sorted(CASES))
@pytest.mark.parametrize("place_out", PLACES)
def test_a_skipped_last_row_is_caught(kind, place_out):
    """an output window starts as poison: NaN as fp32 (assert_close's finiteness), -1 as int64 (never a table value)"""
    x, out, op, ref = CASES[kind](PLACES[0], place_out)
    k_skips_last_row(x, out, op)
    with pytest.raises(AssertionError, match="non-finite" if kind == "fp32" else "not bit-exact"):
        _check(x, out, ref)


@pytest.mark.parametrize("kind", sorted(CASES))
def test_a_written_input_is_caught(kind):
    x, out, op, ref = CASES[kind](PLACES[0], PLACES[1])
    k_writes_its_input(x, out, op)
    with pytest.raises(AssertionError, match="an input frame was written"):
        _check(x, out, ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.int32])
def test_frame_layout_and_poison(dtype):
    f = Frame(3, 4, 9, 5, dtype=dtype)
    assert f.lead >= f.stride and f.tail >= f.stride and f.buf.numel() == f.lead + 3 * 9 + f.tail
    assert bool((f.buf.view(torch.uint8) == window.POISON).all())
    if dtype == torch.float32:
        assert bool(torch.isnan(f.buf).all())
    else:
        assert bool((f.buf == -1).all())
    assert f.base_ptr == f.buf.data_ptr() + f.lead * f.item and f.base_ptr % 16 == f.buf.data_ptr() % 16
    assert f.window.shape == (3, 4) and f.window.data_ptr() == f.base_ptr + 5 * f.item and f.window.stride(0) == 9
    f.assert_outside_untouched()
    with pytest.raises(AssertionError, match="call .put first"):
        f.assert_unchanged()
    f.buf[0] = 0                                    # the very first element of the lead
    with pytest.raises(AssertionError, match="before row 0"):
        f.assert_outside_untouched()
    g = Frame(3, 4, 9, 5, dtype=dtype)
    g.buf[-1] = 0                                   # the very last element of the tail
    with pytest.raises(AssertionError, match="past the last row"):
        g.assert_outside_untouched()


def test_a_decoy_fills_the_gaps_of_an_id_frame():
    f = Frame(3, 2, 5, 2, dtype=torch.int64, decoy=7).put(torch.tensor([[1, -1], [2, 3], [-1, 0]]))
    assert f.full[:, :2].eq(7).all() and f.full[:, 4:].eq(7).all() and f.buf[:f.lead].eq(7).all() and f.buf[-f.tail:].eq(7).all()
    assert f.window.tolist() == [[1, -1], [2, 3], [-1, 0]]
    f.assert_outside_untouched()
    f.assert_unchanged()
    with pytest.raises(AssertionError):
        Frame(3, 2, 5, 2, dtype=torch.int64, decoy=-1)              # every lookup skips -1: no decoy


# ---- the gap stays closed: every strided parameter of the headers names its test ----------------------------------------------
def _declared():
    found = set()
    for header in _lib.every_header():
        found |= window.strided_parameters(_abi._text(header))
    return found


def test_the_reader_finds_parameters_and_struct_fields():
    text = """/* int no_stride */ typedef struct { const float* p; int a_stride, b_col; int64_t row_stride; int n; } recalgo_x_t;
    int recalgo_f(const float* x, int ldx, int K, int64_t user_stride, float* y, int ld_mask, int ldx2, int r_ldx, int cold,
                  recalgo_stream_t stream);"""
    assert window.strided_parameters(text) == {("recalgo_x_t", "a_stride"), ("recalgo_x_t", "b_col"), ("recalgo_x_t", "row_stride"),
                                               ("recalgo_f", "ldx"), ("recalgo_f", "user_stride"), ("recalgo_f", "ld_mask")}


def test_every_strided_parameter_of_the_headers_names_the_test_that_drives_it():
    declared = _declared()
    assert ("recalgo_embedding_gather_fwd", "out_col") in declared and ("recalgo_lookup_job_t", "out_col") in declared
    missing, stale = declared - set(window.COVERAGE), set(window.COVERAGE) - declared
    assert not missing, f"strided parameters without a test in tests/window.py COVERAGE: {sorted(missing)}"
    assert not stale, f"COVERAGE rows for parameters no header declares: {sorted(stale)}"


def test_the_named_tests_exist():
    for key, test_id in window.COVERAGE.items():
        module, name = test_id.split("::")
        assert hasattr(importlib.import_module(module), name), f"{key}: {test_id} does not exist"
