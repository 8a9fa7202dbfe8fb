"""A poisoned frame around a window: operands of the C ABI placed inside a wider buffer (plain PyTorch, no native code).

About a dozen entry points of include/*.h let the caller put an operand inside a wider row-major buffer (out_stride / out_col,
g_stride / g_col, x_stride, pool_stride / pool_col, ldx / lddx, user_stride / tag_stride): a lookup or interaction kernel writes
its share of a concatenated activation in place.  tests/redzone.py guards the two ENDS of a contiguous allocation; a kernel that
writes column out_col + width of the neighbouring row, or reads g from column 0 where g_col was due, stays inside the buffer
and is invisible to it.  A Frame is the buffer such an operand lives in:

    [ lead | row 0: stride elements | row 1 | .. | row rows-1 | tail ]        lead, tail >= one stride
                 [col, col + width) of every row is the WINDOW

Every byte that is not window is 0xFF (a NaN as fp32, -1 as int32 / int64: the poison of tests/redzone.py), or - an int64 id
operand, whose lookups skip -1 - the bytes of a caller-supplied DECOY id: a valid id that changes the result when a kernel
reads it.  An output frame's window starts as poison too: an element the kernel never writes fails assert_close's finiteness
check (and assert_bit_exact against a finite reference).

    out = Frame(B, F * K, stride, col, device=dev)                 # an output
    g = Frame(B, F * K, stride, col, device=dev).put(values)       # an input: .put writes the window only
    lib.recalgo_..(.., out.ptr, out.stride, out.col, ..)           # .ptr: row 0, column 0 (the base the ABI takes)
    out.window                                                     # the [rows, width] view at `col`
    out.assert_outside_untouched()                                 # every byte outside the window still holds its fill
    g.assert_unchanged()                                           # the whole frame equals its clone taken after .put

An operand that the ABI addresses by its first ELEMENT (ldx of recalgo_cgc_fwd, user_stride) takes .window_ptr with col = 0,
or the address of column `col`, which is the same thing to the kernel.

The comparisons are on integer views of the bytes (NaN != NaN would hide every poison check done on floats).

COVERAGE, below, names for every strided parameter of the headers the test that drives it with a non-trivial value;
tests/test_window_host.py keeps it equal to what the headers declare.
"""
from __future__ import annotations

import ctypes
import re

import torch

POISON = 0xFF


class Frame:
    def __init__(self, rows, width, stride, col=0, dtype=torch.float32, device="cpu", decoy=None):
        assert rows >= 1 and width >= 1 and 0 <= col and col + width <= stride, (rows, width, stride, col)
        self.rows, self.width, self.stride, self.col, self.dtype = rows, width, stride, col, dtype
        self.item = torch.empty(0, dtype=dtype).element_size()
        # lead and tail: at least one stride, rounded up so that row 0 starts 16-byte aligned (the kernels' 16-byte arms are
        # selected by stride and column, as they are for a caller's own 16-byte aligned activation buffer)
        per16 = 16 // self.item
        self.lead = self.tail = (stride + per16 - 1) // per16 * per16
        n = self.lead + rows * stride + self.tail
        if decoy is None:
            self.buf = torch.full((n * self.item,), POISON, dtype=torch.uint8, device=device).view(dtype)
        else:
            assert dtype == torch.int64 and int(decoy) >= 0, "a decoy is a valid id: every lookup skips -1"
            self.buf = torch.full((n,), int(decoy), dtype=dtype, device=device)
        self.decoy = decoy
        self.fill = self.buf.view(torch.uint8).clone()            # what every byte outside the window must still hold
        self.full = self.buf[self.lead:self.lead + rows * stride].view(rows, stride)
        self.window = self.full[:, col:col + width]
        keep = torch.ones(n, dtype=torch.bool, device=device)
        keep[self.lead:self.lead + rows * stride].view(rows, stride)[:, col:col + width] = False
        self._outside = keep
        self._clone = None
        assert self.base_ptr % 16 == 0 or device == "cpu" or torch.device(device).type == "cpu"

    # ---- addresses ----------------------------------------------------------------------------------------------------------
    @property
    def base_ptr(self) -> int:
        """the address of row 0, column 0"""
        return self.full.data_ptr()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.base_ptr)

    @property
    def window_ptr(self):
        """the address of row 0, column `col`: for operands the ABI addresses by their first element (a leading dimension)"""
        return ctypes.c_void_p(self.window.data_ptr())

    # ---- contents -----------------------------------------------------------------------------------------------------------
    def put(self, values):
        """writes the window only; the frame as it is now is what assert_unchanged() compares with"""
        values = torch.as_tensor(values)
        assert values.numel() == self.rows * self.width, (tuple(values.shape), self.rows, self.width)
        self.window.copy_(values.reshape(self.rows, self.width).to(self.dtype))
        self._clone = self.buf.view(torch.uint8).clone()
        return self

    def get(self):
        """the window as a contiguous host tensor"""
        return self.window.detach().cpu().contiguous()

    def _where(self, bad_bytes) -> str:
        first = int(torch.nonzero(bad_bytes.cpu())[0]) // self.item - self.lead
        n = int(bad_bytes.sum())
        if first < 0:
            return f"{n} bytes differ, the first {-first} elements before row 0"
        if first >= self.rows * self.stride:
            return f"{n} bytes differ, the first {first - self.rows * self.stride} elements past the last row"
        return f"{n} bytes differ, the first at row {first // self.stride}, column {first % self.stride}"

    def assert_outside_untouched(self, what=""):
        """every byte outside the window still holds its fill (integer views of the bytes)"""
        bad = (self.buf.view(torch.uint8) != self.fill) & self._outside.repeat_interleave(self.item)
        if bool(bad.any()):
            raise AssertionError(f"{what}: written outside the window [{self.col}, {self.col + self.width}) of rows of "
                                 f"{self.stride}: {self._where(bad)}")

    def assert_unchanged(self, what=""):
        """an input: the whole frame, window included, equals its clone taken after .put"""
        assert self._clone is not None, "assert_unchanged() is for inputs: call .put first"
        bad = self.buf.view(torch.uint8) != self._clone
        if bool(bad.any()):
            raise AssertionError(f"{what}: an input frame was written: {self._where(bad)}")


# ---- the strided parameters of the ABI and the tests that drive them ---------------------------------------------------------------
STRIDED_NAME = re.compile(r"\w+_stride|\w+_col|ld[a-z_]*")


def strided_parameters(text: str) -> set:
    """{(entry point or struct, name)} of every int / int64_t parameter or struct field of a header's text whose name ends in
    _stride or _col or matches ld[a-z_]* (pool_stride / pool_col are of the first kind)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = set()
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(recalgo_\w+_t)\s*;", text):
        for stmt in m.group(1).split(";"):
            d = re.fullmatch(r"\s*(?:const\s+)?(int|int64_t)\s+([\w\s,]+?)\s*", stmt, flags=re.S)
            if d:
                found |= {(m.group(2), n.strip()) for n in d.group(2).split(",") if STRIDED_NAME.fullmatch(n.strip())}
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*recalgo_\w+_t\s*;", " ", text)
    for m in re.finditer(r"\b(recalgo_\w+)\s*\(([^(){};]*)\)\s*;", text):
        for p in m.group(2).split(","):
            d = re.fullmatch(r"\s*(?:const\s+)?(int|int64_t)\s+(\w+)\s*", p, flags=re.S)
            if d and STRIDED_NAME.fullmatch(d.group(2)):
                found.add((m.group(1), d.group(2)))
    return found


_W = "tests.test_gpu_windows::"
_DENSE_BWD = "tests.test_gpu_dense_abi::test_bwd_options_crossed"
_DENSE_FWD = "tests.test_gpu_dense_abi::test_fwd_options_crossed"
# (entry point or struct, parameter or field) -> the test that calls it with stride != width / column != 0 / ld != width
COVERAGE = {
    ("recalgo_embedding_gather_fwd", "out_stride"): _W + "test_gather_fwd",
    ("recalgo_embedding_gather_fwd", "out_col"): _W + "test_gather_fwd",
    ("recalgo_embedding_gather_fwd_deferred", "out_stride"): _W + "test_gather_fwd",
    ("recalgo_embedding_gather_fwd_deferred", "out_col"): _W + "test_gather_fwd",
    ("recalgo_embedding_gather_bwd", "g_stride"): _W + "test_gather_bwd",
    ("recalgo_embedding_gather_bwd", "g_col"): _W + "test_gather_bwd",
    ("recalgo_embedding_bag_mean_fwd_deferred", "out_stride"): _W + "test_bag_mean_fwd",
    ("recalgo_embedding_bag_mean_fwd_deferred", "out_col"): _W + "test_bag_mean_fwd",
    ("recalgo_embedding_bag_mean_bwd", "g_stride"): _W + "test_bag_mean_bwd",
    ("recalgo_embedding_bag_mean_bwd", "g_col"): _W + "test_bag_mean_bwd",
    ("recalgo_lookup_job_t", "out_stride"): _W + "test_lookup_multi",
    ("recalgo_lookup_job_t", "out_col"): _W + "test_lookup_multi",
    ("recalgo_cross_fwd", "x_stride"): _W + "test_cross_stack",
    ("recalgo_cross_fwd", "out_stride"): _W + "test_cross_stack",
    ("recalgo_cross_bwd", "x_stride"): _W + "test_cross_stack",
    ("recalgo_cross_bwd", "g_stride"): _W + "test_cross_stack",
    ("recalgo_cross_layer_fwd", "x_stride"): _W + "test_cross_layer",
    ("recalgo_cross_layer_fwd", "out_stride"): _W + "test_cross_layer",
    ("recalgo_cross_layer_bwd", "x_stride"): _W + "test_cross_layer",
    ("recalgo_cross_layer_bwd", "g_stride"): _W + "test_cross_layer",
    ("recalgo_gather_cross_fwd", "x_stride"): _W + "test_gather_cross",
    ("recalgo_gather_cross_fwd", "out_stride"): _W + "test_gather_cross",
    ("recalgo_cin_layer_fwd", "pool_stride"): _W + "test_cin_layer",
    ("recalgo_cin_layer_fwd", "pool_col"): _W + "test_cin_layer",
    ("recalgo_cin_layer_bwd", "pool_stride"): _W + "test_cin_layer",
    ("recalgo_cin_layer_bwd", "pool_col"): _W + "test_cin_layer",
    ("recalgo_bilinear_fwd", "out_stride"): _W + "test_bilinear",
    ("recalgo_bilinear_fwd", "out_col"): _W + "test_bilinear",
    ("recalgo_bilinear_bwd", "g_stride"): _W + "test_bilinear",
    ("recalgo_bilinear_bwd", "g_col"): _W + "test_bilinear",
    ("recalgo_cgc_fwd", "ldx"): _W + "test_cgc",
    ("recalgo_cgc_bwd", "ldx"): _W + "test_cgc",
    ("recalgo_cgc_bwd", "lddx"): _W + "test_cgc",
    ("recalgo_gate_mix_fwd", "ldx"): _W + "test_gate_mix",
    ("recalgo_gate_mix_bwd", "ldx"): _W + "test_gate_mix",
    ("recalgo_gate_mix_bwd", "lddx"): _W + "test_gate_mix",
    ("recalgo_wide_cross_fwd", "user_stride"): _W + "test_wide_cross",
    ("recalgo_wide_cross_fwd", "tag_stride"): _W + "test_wide_cross",
    ("recalgo_dense_bwd_rider_supported", "ldx"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider_supported", "ldg"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider_supported", "lddx"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider", "ldx"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider", "ldg"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider", "ldc"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider", "lddx"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider", "ld_mask"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider", "c_x_stride"): _W + "test_dense_bwd_rider",
    ("recalgo_dense_bwd_rider", "c_g_stride"): _W + "test_dense_bwd_rider",
    ("recalgo_metrics_slot_t", "label_stride"): _W + "test_metrics_label_stride",
    ("recalgo_scatter_source_t", "g_stride"): _W + "test_scatter_source_window",
    ("recalgo_scatter_source_t", "g_col"): _W + "test_scatter_source_window",
    # driven with non-trivial values by the tests these entries already had
    ("recalgo_metrics_slot_t", "prediction_stride"): "tests.test_gpu_metrics::test_one_auc_slot",
    ("recalgo_dense_fwd", "ldx"): _DENSE_FWD,
    ("recalgo_dense_fwd", "ldy"): _DENSE_FWD,
    ("recalgo_dense_bwd_input", "ldg"): _DENSE_BWD,
    ("recalgo_dense_bwd_input", "ldc"): _DENSE_BWD,
    ("recalgo_dense_bwd_input", "lddx"): _DENSE_BWD,
    ("recalgo_dense_bwd_weights", "ldx"): _DENSE_BWD,
    ("recalgo_dense_bwd_weights", "ldg"): _DENSE_BWD,
    ("recalgo_dense_bwd", "ldx"): _DENSE_BWD,
    ("recalgo_dense_bwd", "ldg"): _DENSE_BWD,
    ("recalgo_dense_bwd", "ldc"): _DENSE_BWD,
    ("recalgo_dense_bwd", "lddx"): _DENSE_BWD,
    ("recalgo_dense_bwd", "ld_mask"): _DENSE_BWD,
    ("recalgo_colsum_t", "row_stride"): "tests.test_gpu_dense_abi::test_reduce_column_sums",
    ("recalgo_din_attention_bwd_joined", "ldg"): "tests.test_gpu_dispatch_arms::test_din_generic_arm_joined",
    ("recalgo_din_attention_bwd_joined", "ld_extra"): "tests.test_gpu_dispatch_arms::test_din_generic_arm_joined",
    ("recalgo_pnn_features_fwd", "ld_phi"): "tests.test_gpu_pnn::test_pnn_product_layer_pieces",
    ("recalgo_pnn_features_bwd", "ld_dphi"): "tests.test_gpu_pnn::test_pnn_product_layer_pieces",
    ("recalgo_bag_mean_grad_rows", "g_stride"): "tests.test_gpu_ragged::test_bag_mean_grad_rows",
    ("recalgo_bag_mean_grad_rows", "g_col"): "tests.test_gpu_ragged::test_bag_mean_grad_rows",
}
