"""CPU: the serving path without a GPU.
  * export.plan_chunks: how a request is cut over the captured bucket sizes;
  * include/recalgo_serve.h literally: names, signatures, constants, the `supported` truth table at each limit and one past it,
    refusals before any launch; its place in _lib's header tables and every per-header check of tests/test_abi.py on it;
  * the BatchNorm fold (nn.fold_batch_norm, export.fold_batch_norms) against nn.batch_normalization(training=False) in float64;
  * tests/serve_ref.py: the float32 restatement in the header's order against the float64 one;
  * the serving switch is off by default and nn.SERVE_TOWER_MAX_ROWS is what profiles/serving_bench.json supports."""
import ctypes
import json
import os
import re

import pytest
import torch

from tests import serve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_serve.h")
NAME = "recalgo_serve.h"


# ---- plan_chunks --------------------------------------------------------------------------------------------------------------
def test_plan_chunks():
    from recalgorithm_amd.export import plan_chunks
    buckets = (64, 16, 256)                                   # (any order)
    assert plan_chunks(0, buckets) == []
    assert plan_chunks(1, buckets) == [(0, 1, 16)]
    assert plan_chunks(16, buckets) == [(0, 16, 16)] and plan_chunks(64, buckets) == [(0, 64, 64)]       # exactly a bucket
    assert plan_chunks(17, buckets) == [(0, 17, 64)] and plan_chunks(65, buckets) == [(0, 65, 256)]      # one above a bucket
    assert plan_chunks(256, buckets) == [(0, 256, 256)]
    assert plan_chunks(257, buckets) == [(0, 256, 256), (256, 1, 16)]
    assert plan_chunks(48, (16,)) == [(0, 16, 16), (16, 16, 16), (32, 16, 16)]
    for n in (257, 512, 600, 1000, 4097):
        chunks = plan_chunks(n, buckets)
        rows = [r for at, cnt, _ in chunks for r in range(at, at + cnt)]
        assert rows == list(range(n)), "every row once, in order"
        assert all(cnt <= size and size in buckets for _, cnt, size in chunks)
        assert all(size == 256 and cnt == 256 for _, cnt, size in chunks[:-1])
        last = chunks[-1]
        assert last[2] == min(b for b in buckets if b >= last[1]), "the rest goes to the smallest bucket that holds it"
    for bad in ((), (0, 16), (-4,)):
        with pytest.raises(ValueError):
            plan_chunks(3, bad)
    with pytest.raises(ValueError):
        plan_chunks(-1, buckets)


# ---- the header ---------------------------------------------------------------------------------------------------------------
DECLARED = ["recalgo_serve_abi_version", "recalgo_serve_tower_supported", "recalgo_serve_tower_fwd"]
LAUNCHES = ["recalgo_serve_tower_fwd"]


def _supported(lib, K0, units):
    return lib.recalgo_serve_tower_supported(K0, (ctypes.c_int * max(len(units), 1))(*units), len(units))


def test_header_literal_expectations():
    from recalgorithm_amd import _lib, build, ops
    build.build(verbose=False)
    abi = _lib.SERVING_HEADERS[NAME]
    assert list(abi.functions) == DECLARED and abi.launches == LAUNCHES and not abi.structs
    lib = _lib.load()
    assert lib.recalgo_serve_abi_version() == abi.version == 1 and abi.label == "SERVE ABI"
    c_int, c_uint, ptr = ctypes.c_int, ctypes.c_uint, ctypes.c_void_p
    F = abi.functions
    assert F["recalgo_serve_abi_version"] == (c_int, []) and F["recalgo_serve_tower_supported"] == (c_int, [c_int, ptr, c_int])
    assert F["recalgo_serve_tower_fwd"] == (c_int, [ptr] * 6 + [c_int, c_uint, c_int, c_int, ptr, ptr])
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RECALGO_SERVE_\w+) (0x[0-9A-Fa-f]+|\d+)", open(HEADER).read())
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_SERVE_ABI_VERSION": 1, "RECALGO_SERVE_MAX_LAYERS": 4, "RECALGO_SERVE_MAX_IN": 1024,
                                        "RECALGO_SERVE_MAX_UNITS": 512}
    assert (ops.SERVE_MAX_LAYERS, ops.SERVE_MAX_IN, ops.SERVE_MAX_UNITS) == (4, 1024, 512)
    # each limit and one past it (a host-side query: no device needed)
    assert _supported(lib, 416, []) == 0                                                            # L = 0
    assert _supported(lib, 416, [64] * 4) == 1 and _supported(lib, 416, [64] * 5) == 0              # L = 4, 5
    assert [_supported(lib, K0, [64]) for K0 in (0, 1, 1024, 1025)] == [0, 1, 1, 0]
    assert [_supported(lib, 48, [u]) for u in (0, 8, 16, 24, 32, 512, 520, 528)] == [0, 0, 1, 0, 1, 1, 0, 0]
    assert _supported(lib, 48, [512, 24, 16]) == 0 and _supported(lib, 48, [512, 16, 528]) == 0     # any layer
    assert lib.recalgo_serve_tower_supported(48, None, 1) == 0
    assert ops.serve_tower_supported(416, [512, 256, 128]) and not ops.serve_tower_supported(416, [])
    # a launch that returns an error raises through the errcheck (NULL buffers: refused before any launch)
    with pytest.raises(_lib.RecalgoError, match="recalgo_serve_tower_fwd failed with hipError_t=1$"):
        lib.recalgo_serve_tower_fwd(None, None, None, None, None, (ctypes.c_int * 1)(16), 1, 1, 1, 16, None, None)


def test_the_header_tables():
    """HEADERS and MORE_HEADERS are pinned, by length and order, by the host tests of the features that added them; the serving
    header is an entry of the third table, and load() has walked all three."""
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
    assert _abi.read_record(NAME) == {1: _abi.declaration_hash(NAME)}, "include/recalgo_serve.abi records version 1's hash"


# ---- the BatchNorm fold -------------------------------------------------------------------------------------------------------
def test_the_fold_is_batch_normalization_in_inference_mode():
    from recalgorithm_amd import export, nn
    from recalgorithm_amd.variables import VariableStore, use_store
    g = torch.Generator().manual_seed(7)
    C, B = 24, 9
    store = VariableStore("cpu", seed=1)
    x = torch.randn(B, C, generator=g, dtype=torch.float64)
    with use_store(store), store.variable_scope("tower"):
        nn.batch_normalization(x.float(), training=False)                       # registers gamma, beta and the moving statistics
        values = {"gamma": 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64), "beta": torch.randn(C, generator=g, dtype=torch.float64),
                  "moving_mean": torch.randn(C, generator=g, dtype=torch.float64),
                  "moving_variance": 0.05 + 2 * torch.rand(C, generator=g, dtype=torch.float64)}
        for k, v in values.items():
            store.vars[f"tower/batch_normalization/{k}"].data = v              # (float64 variables: the layer's arithmetic in float64)
    with use_store(store):
        store.begin_call()                                                      # (a new model_fn call: the auto names restart)
        with store.variable_scope("tower"):
            want = nn.batch_normalization(x, training=False)
    assert want.dtype == torch.float64
    scale, shift = nn.fold_batch_norm(values["gamma"], values["beta"], values["moving_mean"], values["moving_variance"], nn.BN_EPSILON)
    assert torch.equal(x * scale + shift, want)
    textbook = (x - values["moving_mean"]) / torch.sqrt(values["moving_variance"] + 1e-3) * values["gamma"] + values["beta"]
    assert float((want - textbook).abs().max()) <= 1e-13 * float(textbook.abs().max())
    rs, rsh = R.fold(values["gamma"], values["beta"], values["moving_mean"], values["moving_variance"], 1e-3)
    assert torch.allclose(rs, scale, rtol=1e-15, atol=0) and torch.allclose(rsh, shift, rtol=1e-14, atol=1e-15)
    # the table compile() computes once: one entry per BatchNorm, keyed by its gamma; an incomplete group is passed over
    arrays = {f"tower/batch_normalization/{k}": v for k, v in values.items()}
    arrays.update({"tower/dense/kernel": torch.zeros(3, 3), "other/gamma": torch.ones(4), "other/beta": torch.zeros(4)})
    folds = export.fold_batch_norms(arrays)
    assert list(folds) == ["tower/batch_normalization/gamma"]
    assert torch.equal(folds["tower/batch_normalization/gamma"][0], scale) and torch.equal(folds["tower/batch_normalization/gamma"][1], shift)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K0,units,relu_bits", [(5, [16], 1), (37, [32, 16], 0b01), (80, [48, 32, 16], 0b111)])
def test_the_ordered_float32_restatement_follows_the_float64_one(K0, units, relu_bits):
    x, layers = R.random_tower(7, K0, units, relu_bits, {0, len(units) - 1}, {1}, seed=K0)
    r64, r32 = R.tower64(x, layers), R.tower32(x, layers)
    assert r32.dtype == torch.float32 and r32.shape == r64.shape == (7, units[-1])
    scale = float(r64.abs().max())
    assert 0 < float((r32.double() - r64).abs().max()) <= 1e-5 * scale          # fp32 rounding, and nothing more
    # a layer without relu, scale and bias is the plain product: the chains' order shows only in the last bits
    w = layers[0][0]
    plain = R.tower32(x, [(w, None, None, None, False)])
    assert float((plain.double() - x @ w).abs().max()) <= 1e-5 * float((x @ w).abs().max())


# ---- the lazy tower -----------------------------------------------------------------------------------------------------------
def test_a_tower_is_a_value_a_kept_hidden_layer_is_not_overwritten():
    """h1 = dense(x); h2 = dense(h1) under the switch: two towers over the same input, the first still one layer deep — a
    model_fn that keeps h1 (a skip connection, an auxiliary head) gets h1's values, not h2's"""
    from recalgorithm_amd import nn
    from recalgorithm_amd.variables import Variable
    x = torch.zeros(3, 20)
    k1, b1, k2 = Variable("a/kernel", torch.zeros(20, 32)), Variable("a/bias", torch.zeros(32)), Variable("b/kernel", torch.zeros(32, 16))
    scale, shift = torch.ones(32), torch.zeros(32)
    t0 = nn.LazyTower(x)
    t1 = t0.with_layer(k1, b1)
    t1f = t1.with_fold(scale, shift)
    t2 = t1f.with_layer(k2, None)
    assert len({id(t) for t in (t0, t1, t1f, t2)}) == 4 and all(t.x is x for t in (t1, t1f, t2))
    assert t0.layers == () and t1.layers == ((k1, b1, None, None),) and t1f.layers == ((k1, b1, scale, shift),)
    assert t2.layers == ((k1, b1, scale, shift), (k2, None, None, None))
    assert t1.shape == t1f.shape == (3, 32) and t2.shape == (3, 16) and t2.units() == [32, 16] and t2.dim() == 2


# ---- the switch ---------------------------------------------------------------------------------------------------------------
def test_the_serving_switch_is_off_by_default_and_the_row_limit_is_the_measured_one():
    from recalgorithm_amd import nn
    from recalgorithm_amd.variables import VariableStore
    assert VariableStore("cpu").serving is None
    bench = json.load(open(os.path.join(ROOT, "profiles", "serving_bench.json")))
    assert bench["serve_tower_max_rows"] == nn.SERVE_TOWER_MAX_ROWS
    sizes = bench["request_sizes"]
    assert sizes == [1, 16, 64, 256, 1024, 4096]
    for model in ("deepfm", "dcn"):
        rows = bench["models"][model]
        assert [r["n"] for r in rows] == sizes and all(set(r["paths"]) == {"predict", "native_eager", "compiled", "compiled_tower"} for r in rows)
    # the limit: the largest measured size such that, on the model whose stack folds a BatchNorm per layer (DeepFM), the tower graph
    # is no slower than the per-layer graph there and at every smaller size; 0 when there is none.  Plain dense(relu) stacks
    # (DCN) take the tower only if the same holds for them up to that limit.
    def limit(model):
        best = 0
        for r in bench["models"][model]:
            if r["paths"]["compiled_tower"]["device_ms"] > r["paths"]["compiled"]["device_ms"]:
                break
            best = r["n"]
        return best
    assert nn.SERVE_TOWER_MAX_ROWS == limit("deepfm")
    assert bench["serve_tower_plain_stacks"] == nn.SERVE_TOWER_PLAIN_STACKS == (limit("dcn") >= limit("deepfm") > 0)
