"""CPU: ragged features of fixed capacity without a GPU.
  * feature_column.pad_ragged and the contract of a padded Ragged;
  * the capacity policy of RunConfig(ragged_capacity=): int, dict, "auto" with its rounding rule; the overflow decision; a dense
    [B] id vector presented as a Ragged; Estimator._fit_ragged on a CPU store;
  * the serving span layout of a bucket with bags (export.ragged_span_layout) and how a decoded request fills it;
  * include/recalgo_ragged.h literally: names, signatures, the recorded hash, every refusal before any launch, its place in _lib's
    header tables and the per-header checks of tests/test_abi.py;
  * tests/ragged_ref.py, the numpy restatement of recalgo_bag_mean_grad_rows, against the torch composition it replaces, on the
    CPU: the yardstick of tests/test_gpu_ragged.py is what trained before."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ragged_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_ragged.h")
NAME = "recalgo_ragged.h"
DECLARED = ["recalgo_ragged_abi_version", "recalgo_ragged_pad", "recalgo_bag_mean_grad_rows"]
LAUNCHES = ["recalgo_ragged_pad", "recalgo_bag_mean_grad_rows"]
FAKE = 0x10000           # a non-NULL, 16-byte aligned address: the refusals below happen before anything is read through it


# ---- pad_ragged -----------------------------------------------------------------------------------------------------------------
def test_pad_ragged_on_the_host():
    from recalgorithm_amd.feature_column import Ragged, pad_ragged
    values, offsets = (torch.from_numpy(a) for a in R.bags(5))
    r = Ragged(values, offsets)
    nnz = int(offsets[-1])
    assert nnz == values.numel() == 15
    p = pad_ragged(r, 2 * nnz + 1)
    assert p.values.dtype == torch.int64 and p.values.numel() == 2 * nnz + 1
    assert torch.equal(p.values[:nnz], values) and bool((p.values[nnz:] == -1).all())
    assert p.offsets is offsets and torch.equal(values, torch.from_numpy(R.bags(5)[0])), "offsets untouched, the source too"
    assert np.array_equal(p.values.numpy(), R.pad(values.numpy(), 2 * nnz + 1))
    assert pad_ragged(r, nnz) is r, "capacity == nnz: nothing to do"
    again = pad_ragged(p, 2 * nnz + 1)
    assert again is p, "padding an already padded Ragged changes nothing"
    wider = pad_ragged(p, 3 * nnz)
    assert torch.equal(wider.values[:nnz], values) and bool((wider.values[nnz:] == -1).all()) and wider.values.numel() == 3 * nnz
    back = pad_ragged(wider, nnz)
    assert torch.equal(back.values, values), "a padded Ragged may shrink down to its nnz"
    with pytest.raises(ValueError, match="15 values do not fit a capacity of 14"):
        pad_ragged(r, nnz - 1)
    with pytest.raises(ValueError, match="do not fit"):
        pad_ragged(wider, nnz - 1)
    empty = pad_ragged(Ragged(torch.zeros(0, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)), 3)
    assert empty.values.tolist() == [-1, -1, -1]


# ---- the capacity policy --------------------------------------------------------------------------------------------------------
def test_capacity_policy():
    from recalgorithm_amd import estimator as E
    assert E.ragged_capacity_for(None, "a", 64) is None
    assert E.ragged_capacity_for(8, "a", 64) == 512 and E.ragged_capacity_for(8, "b", 1) == 8
    assert E.ragged_capacity_for({"a": 4, "b": 50}, "a", 64) == 256 and E.ragged_capacity_for({"a": 4, "b": 50}, "b", 64) == 3200
    assert E.ragged_capacity_for({"a": 4}, "c", 64) is None, "a dict without the key gives no capacity: such a batch stays eager"
    assert E.ragged_capacity_for("auto", "a", 64) is None and E.ragged_capacity_for("auto", "a", 64, max_nnz=1000) == 2048
    # ceil(1.25 * max_nnz / 1024) * 1024
    want = lambda m: int(np.ceil(1.25 * m / 1024)) * 1024
    for m in (0, 1, 819, 820, 1638, 1639, 4096, 10240, 102400, 204799, 204800, 10 ** 7 + 3):
        assert E.ragged_auto_capacity(m) == want(m), m
    assert [E.ragged_auto_capacity(m) for m in (0, 1, 819, 820, 4096)] == [0, 1024, 1024, 2048, 5120]
    assert all(E.ragged_auto_capacity(m) >= 1.25 * m for m in range(0, 5000, 7))
    for bad in (0, -1, True, 2.5, "AUTO", {"a": 0}, {"a": "4"}, [4]):
        with pytest.raises(ValueError, match="ragged_capacity"):
            E.RunConfig(device="cpu", ragged_capacity=bad)
    assert E.RunConfig(device="cpu").ragged_capacity is None, "off by default: a ragged batch runs eagerly, as before"
    assert E.RunConfig(device="cpu", ragged_capacity="auto").ragged_capacity == "auto"
    d = {"a": 4}
    cfg = E.RunConfig(device="cpu", ragged_capacity=d)
    d["a"] = 5
    assert cfg.ragged_capacity == {"a": 4}


def test_overflow_decision_and_dense_vectors():
    from recalgorithm_amd import estimator as E
    assert not E.ragged_overflows(512, 512) and E.ragged_overflows(513, 512) and not E.ragged_overflows(0, 0)
    assert E.ragged_overflows(0, None), "no capacity: the eager route"
    r = E.dense_as_ragged(torch.tensor([3, -1, 0, 7]))
    assert r.values.tolist() == [3, -1, 0, 7] and r.offsets.tolist() == [0, 1, 2, 3, 4] and r.offsets.dtype == torch.int64
    r2 = E.dense_as_ragged(torch.tensor([[3], [-1]]))
    assert r2.values.tolist() == [3, -1] and r2.offsets.tolist() == [0, 1, 2]
    # the -1 is a bag without a valid value: a zero gradient row, the divisor clamped to 1 (as an empty bag's)
    g = np.arange(8, dtype=np.float32).reshape(4, 2) + 1
    rows = R.grad_rows(r.values.numpy(), r.offsets.numpy(), g)
    assert np.array_equal(rows, np.array([[1, 2], [0, 0], [5, 6], [7, 8]], np.float32))


def test_fit_ragged_on_a_cpu_store():
    from recalgorithm_amd import estimator as E
    from recalgorithm_amd.feature_column import Ragged
    bag = lambda lens: Ragged(torch.arange(sum(lens)), torch.tensor([0] + list(np.cumsum(lens))))
    dense = torch.rand(4, 1)

    est = E.Estimator(lambda *a: None, {}, E.RunConfig(device="cpu", ragged_capacity={"tags": 2, "his": 3}))
    f, fits = est._fit_ragged({"tags": bag([2, 0, 1, 3]), "his": bag([3, 3, 3, 2]), "x": dense}, warm=True)
    assert fits and f["tags"].values.tolist() == [0, 1, 2, 3, 4, 5, -1, -1] and f["his"].values.numel() == 12 and f["x"] is dense
    assert f["tags"].offsets.tolist() == [0, 2, 2, 3, 6]
    over = {"tags": bag([2, 0, 1, 3]), "his": bag([3, 3, 3, 4]), "x": dense}
    f, fits = est._fit_ragged(over, warm=False)
    assert not fits and f is over and est.ragged_overflows == 1, "never truncated: the batch goes on as it came"
    # `tags` arrives as a dense id vector (no row of this batch holds two values)
    f, fits = est._fit_ragged({"tags": torch.tensor([5, -1, 2, 0]), "his": bag([1, 1, 1, 1]), "x": dense}, warm=False)
    assert fits and f["tags"].values.tolist() == [5, -1, 2, 0, -1, -1, -1, -1] and f["tags"].offsets.tolist() == [0, 1, 2, 3, 4]
    assert est.ragged_overflows == 1
    # a ragged key the dict does not name: no capacity, the eager route, counted
    f, fits = est._fit_ragged({"tags": bag([1, 1, 1, 1]), "his": bag([1, 1, 1, 1]), "other": bag([1, 0, 0, 0])}, warm=False)
    assert not fits and est.ragged_overflows == 2

    auto = E.Estimator(lambda *a: None, {}, E.RunConfig(device="cpu", ragged_capacity="auto"))
    for lens in ([300, 300, 300], [400, 400, 100]):
        f, fits = auto._fit_ragged({"his": bag(lens)}, warm=True)
        assert fits and f["his"].values.numel() == 2048                    # ceil(1.25 * 900 / 1024) * 1024
    f, fits = auto._fit_ragged({"his": bag([500, 500, 1000])}, warm=False)
    assert fits and f["his"].values.numel() == 2048 and auto._ragged_caps == {"his": 2048}, "settled when the warm-up ended"
    f, fits = auto._fit_ragged({"his": bag([1000, 1000, 49])}, warm=False)
    assert not fits and auto.ragged_overflows == 1 and auto._ragged_caps == {"his": 2048}

    off = E.Estimator(lambda *a: None, {}, E.RunConfig(device="cpu"))
    b = {"his": bag([1, 2])}
    f, fits = off._fit_ragged(b, warm=True)
    assert f is b and fits is True and off._capturable(b, True) is False, "None: a ragged batch is not static, as before"
    assert off._capturable({"x": dense}, True) is True

    est.store.data_dependent = "sequence_input_layer: max_length is None"
    assert est._capturable({"his": bag([1, 1])}, True) is False and est.capture_refused == "sequence_input_layer: max_length is None"
    b = {"his": bag([9, 9])}
    f, fits = est._fit_ragged(b, warm=False)
    assert f is b and fits is False and est.ragged_overflows == 2, "a refused model's batches are left alone"


def test_the_common_flag():
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm import _common as C
    C.define_ragged_capacity_flag()
    saved = dict(flags.FLAGS._overrides)
    try:
        for value, want in ((0, None), (-1, "auto"), (8, 8)):
            flags.FLAGS.ragged_capacity = value
            assert C.ragged_capacity_from_flags() == want
        flags.FLAGS.ragged_capacity = -2
        with pytest.raises(ValueError, match="ragged_capacity"):
            C.ragged_capacity_from_flags()
    finally:
        flags.FLAGS._overrides.clear()
        flags.FLAGS._overrides.update(saved)


# ---- the serving span -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 16])
def test_serving_span_layout(rows):
    from recalgorithm_amd import export as E
    F, NF = 7, 16
    caps = [("his_read_comment_7d_seq", 8), ("manual_tag_list", 4)]
    dense_end = E.ServingModel._span_bytes(rows, F, NF)[1]
    pieces, total = E.ragged_span_layout(rows, F, NF, caps)
    assert list(pieces) == [k for k, _ in caps]
    up = lambda n: (n + 15) // 16 * 16
    at = up(dense_end)
    for key, cap in caps:
        off_at, val_at, n_values = pieces[key]
        assert (off_at, val_at, n_values) == (at, at + up(8 * (rows + 1)), rows * cap), key
        assert off_at % 16 == 0 and val_at % 16 == 0
        at = val_at + up(8 * rows * cap)
    assert total == at and total % 16 == 0
    if rows == 1:
        assert dense_end == 64 + 64 and pieces == {"his_read_comment_7d_seq": (128, 144, 8), "manual_tag_list": (208, 224, 4)} and total == 256
    else:
        assert dense_end == 896 + 1024 and pieces == {"his_read_comment_7d_seq": (1920, 2064, 128), "manual_tag_list": (3088, 3232, 64)}
        assert total == 3744
    assert E.ragged_span_layout(rows, F, NF, []) == ({}, up(dense_end))

    # a decoded request of n rows into the pieces: the rows past it are empty bags, the values end in -1
    n = min(rows, 3)
    bags = {"his_read_comment_7d_seq": (np.arange(n + 1, dtype=np.int64) * 2, np.arange(2 * n, dtype=np.int64) + 100),
            "manual_tag_list": (np.array([0] + [1] * n, np.int64), np.array([9], np.int64))}
    host = np.full(total, 0x5A, np.uint8)
    assert E._fill_ragged_pieces(host, pieces, bags, rows, n)
    for key, (off_at, val_at, n_values) in pieces.items():
        o, v = host[off_at:off_at + 8 * (rows + 1)].view(np.int64), host[val_at:val_at + 8 * n_values].view(np.int64)
        offsets, values = bags[key]
        assert np.array_equal(o[:n + 1], offsets) and np.all(o[n + 1:] == offsets[n])
        assert np.array_equal(v[:len(values)], values) and np.all(v[len(values):] == -1)
    # one bag too many for its capacity: nothing is truncated, every piece holds empty bags, the caller serves eagerly
    big = dict(bags, manual_tag_list=(np.array([0] + [4 * rows + 1] * n, np.int64), np.arange(4 * rows + 1, dtype=np.int64)))
    assert not E._fill_ragged_pieces(host, pieces, big, rows, n)
    for key, (off_at, val_at, n_values) in pieces.items():
        assert np.all(host[off_at:off_at + 8 * (rows + 1)].view(np.int64) == 0) and np.all(host[val_at:val_at + 8 * n_values].view(np.int64) == -1)


# ---- the header -------------------------------------------------------------------------------------------------------------------
def test_header_literal_expectations():
    from recalgorithm_amd import _lib, build
    build.build(verbose=False)
    abi = _lib.SERVING_HEADERS[NAME]
    assert list(abi.functions) == DECLARED and abi.launches == LAUNCHES and list(abi.structs) == []
    lib = _lib.load()
    assert lib.recalgo_ragged_abi_version() == abi.version == 1 and abi.label == "RAGGED ABI"
    c_int, c_int64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    F = abi.functions
    assert F["recalgo_ragged_abi_version"] == (c_int, [])
    assert F["recalgo_ragged_pad"] == (c_int, [ptr, c_int64, ptr, c_int64, ptr])
    assert F["recalgo_bag_mean_grad_rows"] == (c_int, [ptr, ptr, c_int, c_int64, ptr, c_int, c_int, c_int, ptr, ptr])
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RECALGO_RAGGED_\w+) (0x[0-9A-Fa-f]+|\d+)", open(HEADER).read())
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_RAGGED_ABI_VERSION": 1}

    # every refusal returns hipErrorInvalidValue through the errcheck, before any launch (fake addresses: nothing is read)
    pad_refused = pytest.raises(_lib.RecalgoError, match="recalgo_ragged_pad failed with hipError_t=1$")
    for src, n, dst, cap in ((FAKE, 5, FAKE, 4), (FAKE, 1, FAKE, 0), (FAKE, -1, FAKE, 4), (None, 1, FAKE, 4), (FAKE, 1, None, 4),
                             (FAKE + 4, 1, FAKE, 4), (FAKE, 1, FAKE + 1, 4)):
        with pad_refused:
            lib.recalgo_ragged_pad(src, n, dst, cap, None)
    assert lib.recalgo_ragged_pad(None, 0, None, 0, None) == 0 and lib.recalgo_ragged_pad(FAKE, 0, FAKE, 0, None) == 0, "nothing to launch"

    rows_refused = pytest.raises(_lib.RecalgoError, match="recalgo_bag_mean_grad_rows failed with hipError_t=1$")
    ok = dict(values=FAKE, offsets=FAKE, B=4, capacity=8, g=FAKE, g_stride=4, g_col=0, K=4, rows=FAKE)
    order = list(ok)
    for bad in (dict(B=-1), dict(capacity=-1), dict(K=0), dict(g_col=-1), dict(g_stride=3), dict(g_col=1), dict(offsets=None),
                dict(values=None), dict(g=None), dict(rows=None), dict(values=FAKE + 4), dict(offsets=FAKE + 4), dict(g=FAKE + 2),
                dict(rows=FAKE + 1), dict(capacity=1 << 36)):
        with rows_refused:
            lib.recalgo_bag_mean_grad_rows(*[{**ok, **bad}[k] for k in order], None)
    assert lib.recalgo_bag_mean_grad_rows(*[{**ok, "capacity": 0, "values": None, "g": None, "rows": None}[k] for k in order], None) == 0


def test_the_header_tables():
    from recalgorithm_amd import _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers()
    assert list(_lib.every_header()) == list(_lib.HEADERS) + list(_lib.MORE_HEADERS) + list(_lib.SERVING_HEADERS)
    lib = _lib.load()
    for name, (res, args) in _lib.SERVING_HEADERS[NAME].functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name


def test_every_shared_abi_check_holds_for_the_new_header(monkeypatch):
    """tests/test_abi.py runs once per entry of _lib.HEADERS; with the table replaced by the union of all three, each of its
    per-header checks is called on the new header, and the all-pairs check on the union."""
    from recalgorithm_amd import _abi, _lib, build
    from tests import test_abi as A
    union = _lib.every_header()
    monkeypatch.setattr(_lib, "HEADERS", union)
    monkeypatch.setattr(A, "HEADERS", list(union))
    lib_path = build.build(verbose=False)
    A.test_header_declares_functions(NAME)
    A.test_library_exports_every_declared_symbol(NAME, lib_path)
    A.test_ctypes_binding_matches_header(NAME, lib_path)
    A.test_loaded_functions_carry_the_table(NAME, lib_path)
    A.test_declarations_do_not_change_without_a_version_bump(NAME)
    A.test_header_arg_counts_match_binding(NAME)
    A.test_header_arg_types_match_binding(NAME)
    A.test_header_is_self_contained(NAME)
    A.test_the_headers_share_no_name()
    A.test_stale_version_fails_loudly(NAME, lib_path, monkeypatch)
    assert _abi.read_record(NAME) == {1: _abi.declaration_hash(NAME)}, "include/recalgo_ragged.abi records version 1's hash"


# ---- the restatement against the composition it replaces ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 4, 16])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_the_restatement_is_the_torch_composition(B, K):
    values, offsets = R.bags(B, seed=K)
    nnz = len(values)
    rng = np.random.default_rng([B, K])
    g = rng.standard_normal((B, K)).astype(np.float32)
    ok = R.valid_rows(values.copy(), offsets)
    if B >= 5:
        assert offsets[1] == 0 and not ok[0:3].any() and ok[3] and offsets[4] - offsets[3] == 9, "empty, all OOV, one, nine"
    for capacity in (nnz, nnz + 1, (nnz + 255) // 256 * 256 + 3):
        v = R.pad(values, capacity)
        rows = R.grad_rows(v, offsets, g)
        want = R.composition(torch.from_numpy(v), torch.from_numpy(offsets), torch.from_numpy(g)).numpy()
        valid = R.valid_rows(v.copy(), offsets)
        assert rows.dtype == np.float32 and rows.shape == (capacity, K) and valid.sum() == ok.sum()
        assert np.array_equal(rows[valid].view(np.uint32), want[valid].view(np.uint32)), "bit for bit on the rows that carry a gradient"
        assert not rows[~valid].any(), "zeros everywhere else"
    # a gradient that is a column block of a wider matrix
    wide = rng.standard_normal((B, K + 7)).astype(np.float32)
    assert np.array_equal(R.grad_rows(values, offsets, wide, g_col=3, K=K), R.grad_rows(values, offsets, np.ascontiguousarray(wide[:, 3:3 + K])))


def test_the_restatement_without_values():
    offsets = np.zeros(4, np.int64)
    assert R.grad_rows(np.zeros(0, np.int64), offsets, np.ones((3, 4), np.float32)).shape == (0, 4)
    assert not R.grad_rows(R.pad(np.zeros(0, np.int64), 5), offsets, np.ones((3, 4), np.float32)).any()
