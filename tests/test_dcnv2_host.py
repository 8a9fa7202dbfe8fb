"""CPU-only: include/recalgo_dcnv2.h (DCN-V2's mixture-of-low-rank-experts cross layer, csrc/dcnv2.hip) is a header of the library
like the others: listed in _lib.SERVING_HEADERS, bound by load(), and held to every per-header check of tests/test_abi.py (the
pattern of tests/test_autoint_host.py).  The domain table against the support query and against the RECALGO_REQUIRE lines of the
unit, the refusals of both launching entries on made-up addresses (nothing is launched, so no device is needed), the size queries;
tests/dcnv2_ref.py: the header's backward formulas written out against autograd, the single ungated expert, and the condition that
keeps the GPU parity tests honest (the float32 restatement alone meets their bound on every one of their shapes); the model's
flags and defaults, its variables for both parameterizations on the launch-free registration pass, and what the product imports."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import dcnv2_ref as R
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "recalgo_dcnv2.h"
LAUNCHES = {"recalgo_dcnv2_layer_fwd", "recalgo_dcnv2_layer_bwd"}
QUERIES = {"recalgo_dcnv2_abi_version", "recalgo_dcnv2_supported", "recalgo_dcnv2_bwd_partial_rows", "recalgo_dcnv2_bwd_workspace_bytes"}
LIMITS = {"RECALGO_DCNV2_MIN_D": 4, "RECALGO_DCNV2_MAX_D": 512, "RECALGO_DCNV2_MIN_R": 4, "RECALGO_DCNV2_MAX_R": 64,
          "RECALGO_DCNV2_MAX_E": 4, "RECALGO_DCNV2_TILE": 16, "RECALGO_DCNV2_ROW_TILES": 16, "RECALGO_DCNV2_MAX_PARTIAL_ROWS": 64}


def test_the_header_tables():
    from recalgorithm_amd import _abi, _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers() and NAME in _lib.every_header()
    abi = _lib.SERVING_HEADERS[NAME]
    assert (abi.version, abi.version_query, abi.label) == (1, "recalgo_dcnv2_abi_version", "DCNV2 ABI")
    assert _abi.read_record(NAME) == {1: _abi.declaration_hash(NAME)}
    assert set(abi.functions) == LAUNCHES | QUERIES
    assert set(abi.launches) == LAUNCHES and not abi.structs
    assert {k: abi.constants[k] for k in LIMITS} == LIMITS
    lib = _lib.load()
    assert lib.recalgo_dcnv2_abi_version() == 1
    for name, (res, args) in abi.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name
    # the argument order the header states
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert abi.functions["recalgo_dcnv2_supported"] == (I, [I] * 3)                                     # D, r, E
    assert abi.functions["recalgo_dcnv2_bwd_partial_rows"] == (I, [I] * 4)                              # B, D, r, E
    assert abi.functions["recalgo_dcnv2_bwd_workspace_bytes"] == (L, [I] * 4)
    assert abi.functions["recalgo_dcnv2_layer_fwd"] == (I, [P] * 7 + [I] * 4 + [P] * 2)                 # x0 .. bias, .., y, stream
    assert abi.functions["recalgo_dcnv2_layer_bwd"] == (I, [P] * 8 + [I] * 4 + [P] * 9)                 # g, x0 .. bias, .., dx0 .. ws, stream


def test_every_shared_abi_check_holds_for_the_new_header(monkeypatch):
    from recalgorithm_amd import _lib, build
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


# (D, r, E) -> served: on and one step past every limit, r off its grid, D off every grid (any D is served), negatives
TRUTH = [((3, 8, 2), 0), ((4, 8, 2), 1), ((5, 8, 2), 1), ((82, 8, 2), 1), ((511, 8, 2), 1), ((512, 8, 2), 1), ((513, 8, 2), 0),
         ((20, 0, 2), 0), ((20, 4, 2), 1), ((20, 6, 2), 0), ((20, 62, 2), 0), ((20, 64, 2), 1), ((20, 68, 2), 0),
         ((20, 8, 0), 0), ((20, 8, 1), 1), ((20, 8, 4), 1), ((20, 8, 5), 0),
         ((-20, 8, 2), 0), ((20, -8, 2), 0), ((20, 8, -2), 0),
         ((416, 32, 4), 1), ((416, 64, 4), 1), ((82, 32, 4), 1), ((416, 32, 1), 1), ((512, 64, 4), 1), ((4, 4, 1), 1)]


@pytest.mark.parametrize("shape,served", TRUTH)
def test_the_support_query(shape, served):
    from recalgorithm_amd import _lib, ops
    lib = _lib.load()
    assert lib.recalgo_dcnv2_supported(*shape) == served
    assert ops.dcnv2_supported(*shape) == bool(served)
    D, r, E = shape
    C = LIMITS
    assert bool(served) == (C["RECALGO_DCNV2_MIN_D"] <= D <= C["RECALGO_DCNV2_MAX_D"] and C["RECALGO_DCNV2_MIN_R"] <= r <= C["RECALGO_DCNV2_MAX_R"]
                            and r % 4 == 0 and 1 <= E <= C["RECALGO_DCNV2_MAX_E"])
    # the size queries answer 0 for what is not served, and for an empty batch
    assert (lib.recalgo_dcnv2_bwd_partial_rows(5, *shape) > 0) == bool(served)
    assert (lib.recalgo_dcnv2_bwd_workspace_bytes(5, *shape) > 0) == bool(served)
    assert lib.recalgo_dcnv2_bwd_workspace_bytes(0, *shape) == 0
    assert lib.recalgo_dcnv2_bwd_partial_rows(0, *shape) == 0 and lib.recalgo_dcnv2_bwd_partial_rows(-1, *shape) == 0


def test_the_domain_is_what_the_unit_requires():
    """csrc/dcnv2.hip: both launching entries open with the same RECALGO_REQUIRE lines — the batch and the shape through the one
    shape_ok() that the support query answers with, the pointers, the gate pair, the alignment — and shape_ok names every limit
    of the header and nothing else."""
    src = open(os.path.join(ROOT, "recalgorithm_amd", "csrc", "dcnv2.hip")).read()
    ok = re.search(r"bool shape_ok\(int D, int r, int E\) \{(.*?)\n\}", src, re.S).group(1)
    assert sorted(set(re.findall(r"RECALGO_DCNV2_\w+", ok))) == sorted(k for k in LIMITS if k.startswith(("RECALGO_DCNV2_MIN", "RECALGO_DCNV2_MAX_D",
                                                                                                           "RECALGO_DCNV2_MAX_R", "RECALGO_DCNV2_MAX_E")))
    assert "(r & 3) == 0" in ok and "E >= 1" in ok
    assert "recalgo_dcnv2_supported(int D, int r, int E) { return shape_ok(D, r, E) ? 1 : 0; }" in src
    for entry, n in (("recalgo_dcnv2_layer_fwd", 4), ("recalgo_dcnv2_layer_bwd", 5)):
        body = src[src.index(f"RECALGO_EXPORT int {entry}("):]
        body = body[:body.index("\n}\n")]
        req = re.findall(r"RECALGO_REQUIRE\((.*?)\);\n", body, re.S)
        assert len(req) == n, (entry, req)
        assert req[0] == "B >= 1 && shape_ok(D, r, E)"
        assert "gate != nullptr || E == 1" in req
        assert any(r_.startswith("aligned_to<4>(") for r_ in req)
        assert body.index("launch_lds<") > body.index(req[-1]), "nothing is launched before the last requirement"
    assert "(gate == nullptr) == (dgate == nullptr)" in src


def test_the_workspace_is_the_documented_layout():
    """R = min(ceil(ceil(B / 16) / 16), 64) rows of E (2 D r + r^2 + D) + D floats, then pc, dvpre, v, dcpre [B, E r] and ds [B, 4]"""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    for D, r, E in ((4, 4, 1), (5, 4, 2), (82, 8, 2), (416, 32, 4), (512, 64, 4), (20, 64, 3)):
        row = E * (2 * D * r + r * r + D) + D
        for B in (1, 16, 17, 256, 257, 4096, 16384, 16385, 1 << 20):
            rows = min(-(-(-(-B // 16)) // 16), 64)
            assert lib.recalgo_dcnv2_bwd_partial_rows(B, D, r, E) == rows, (B, D, r, E)
            assert lib.recalgo_dcnv2_bwd_workspace_bytes(B, D, r, E) == 4 * (rows * row + B * (4 * E * r + 4)), (B, D, r, E)
    assert 4 * (4 * (2 * 416 * 32 + 32 * 32 + 416) + 416) == 450_688           # the benchmark shape's row: 450 KB


def test_refusals_need_no_device():
    """Every refusal returns hipErrorInvalidValue through the errcheck before any launch (made-up addresses: nothing is read): an
    unsupported shape or B < 1, a NULL pointer other than the gate pair of a single expert, half a gate pair, no gate with E > 1,
    and a pointer that is not 4-byte aligned."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    B, D, r, E = 5, 20, 8, 2
    # x0, xl, V, C, U, gate, bias, B, D, r, E, y, stream
    fwd_ok = [P(0x10000 * (i + 1)) for i in range(7)] + [B, D, r, E, P(0x90000), None]
    # g, x0, xl, V, C, U, gate, bias, B, D, r, E, dx0, dxl, dV, dC, dU, dgate, dbias, workspace, stream
    bwd_ok = [P(0x10000 * (i + 1)) for i in range(8)] + [B, D, r, E] + [P(0x100000 * (i + 1)) for i in range(8)] + [None]
    cases = {"recalgo_dcnv2_layer_fwd": (fwd_ok, (7, 8, 9, 10), [0, 1, 2, 3, 4, 5, 6, 11], [0, 1, 2, 3, 4, 5, 6, 11]),
             "recalgo_dcnv2_layer_bwd": (bwd_ok, (8, 9, 10, 11), [0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18, 19],
                                         [0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18, 19])}
    for name, (ok, (iB, iD, iR, iE), not_null, pointers) in cases.items():
        fn = getattr(lib, name)
        refused = pytest.raises(_lib.RecalgoError, match=f"{name} failed with hipError_t=1$")

        def call(**changes):
            a = list(ok)
            for i, v in changes.items():
                a[int(i[1:])] = v
            return fn(*a)
        for i, v in ((iD, 3), (iD, 513), (iD, 0), (iD, -20), (iR, 6), (iR, 68), (iR, 0), (iR, -8), (iE, 0), (iE, 5), (iE, -1), (iB, 0), (iB, -1)):
            with refused:
                call(**{f"a{i}": v})
        for i in not_null:                                # (E = 2: the gate pair is required too)
            with refused:
                call(**{f"a{i}": None})
        for i in pointers:
            with refused:
                call(**{f"a{i}": P(ok[i].value + 2)})
    one = [1 if i == 11 else a for i, a in enumerate(bwd_ok)]               # E = 1: gate and dgate may both be NULL, not one of them
    for i in (6, 17):
        with pytest.raises(_lib.RecalgoError, match="recalgo_dcnv2_layer_bwd failed with hipError_t=1$"):
            lib.recalgo_dcnv2_layer_bwd(*[None if j == i else a for j, a in enumerate(one)])


def test_ops_refuse_on_the_host():
    """ops.dcnv2_layer raises ValueError before any launch (CPU tensors: a call that got as far as a launch would raise
    RecalgoError instead)"""
    from recalgorithm_amd import ops
    z = torch.zeros

    def call(B=4, D=20, r=8, E=2, **over):
        a = dict(x0=z(B, D), xl=z(B, D), V=z(E, D, r), C=z(E, r, r), U=z(E, D, r), gate=z(E, D), bias=z(D))
        a.update(over)
        return ops.dcnv2_layer(*a.values())
    for kw in (dict(D=3), dict(D=513), dict(r=6), dict(r=68), dict(E=5)):
        with pytest.raises(ValueError, match="the kernels serve 4 <= D <= 512, r % 4 == 0 with 4 <= r <= 64 and 1 <= E <= 4"):
            call(**kw)
    with pytest.raises(ValueError, match=r"V must be \[E, D, r\]"):
        call(V=z(20, 8))
    with pytest.raises(ValueError, match="the kernels serve"):
        call(V=z(0, 20, 8))                                                  # E = 0
    with pytest.raises(ValueError, match="x0 and xl must be non-empty"):
        call(B=0)
    with pytest.raises(ValueError, match="x0 and xl must be non-empty"):
        call(xl=z(4, 21))
    with pytest.raises(ValueError, match="only a single expert runs without a gate"):
        call(gate=None)
    with pytest.raises(ValueError, match="C has shape"):
        call(C=z(2, 8, 4))
    with pytest.raises(ValueError, match="gate has shape"):
        call(gate=z(20, 2))
    with pytest.raises(ValueError, match="x0 must be a contiguous float32 tensor on x0's device"):     # (a CPU tensor)
        call()


# ---- tests/dcnv2_ref.py --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gated", [((5, 5, 4, 2), True), ((4, 20, 8, 3), True), ((6, 12, 8, 1), False), ((6, 12, 8, 1), True)])
def test_the_headers_backward_formulas_are_autograds(shape, gated):
    x, r64, _ = R.case(*shape, gated=gated, seed=3)
    x64 = {k: (None if v is None else v.double()) for k, v in x.items()}
    by_hand = R.backward_by_hand(x64, x64["g"])
    for k in R.names_of(x)[1:]:
        assert torch.allclose(by_hand[k], r64[k], rtol=1e-11, atol=1e-13), k
    assert (by_hand["dgate"] is None) == (x["gate"] is None)


def test_a_single_expert_is_the_ungated_formula():
    """E = 1: the softmax over one score is 1 whatever the gate, so the layer is x0 * (tanh(tanh(xl V) C) U^T + bias) + xl, the gate
    has no gradient, and dxl has no gate term"""
    x, r64, _ = R.case(6, 12, 8, 1, gated=True, seed=3)
    xu, u64, _ = R.case(6, 12, 8, 1, gated=False, seed=3)
    d = {k: (None if v is None else v.double()) for k, v in x.items()}
    plain = d["x0"] * (torch.tanh(torch.tanh(d["xl"] @ d["V"][0]) @ d["C"][0]) @ d["U"][0].t() + d["bias"]) + d["xl"]
    assert torch.allclose(r64["y"], plain, rtol=1e-13, atol=1e-15) and torch.equal(r64["y"], u64["y"])
    assert bool((r64["p"] == 1).all()) and bool((r64["dgate"] == 0).all()) and u64["dgate"] is None
    for k in R.names_of(xu)[1:]:
        assert torch.allclose(r64[k], u64[k], rtol=1e-13, atol=1e-15), k


def test_xl_being_x0_adds_the_two_input_gradients():
    x, _, _ = R.case(5, 20, 8, 3, seed=2)
    both = R.reference(dict(x, xl=x["x0"]), torch.float64)
    same = R.reference(x, torch.float64, same=True)
    assert torch.allclose(same["dx0"], both["dx0"] + both["dxl"], rtol=1e-13, atol=1e-15) and same["dxl"] is None


@pytest.mark.parametrize("shape", R.SHAPES)
def test_the_float32_restatement_alone_meets_the_gpu_bound(shape):
    """What keeps tests/test_gpu_dcnv2.py's parity test one of the kernels: at every one of its shapes the same arithmetic in
    float32 torch passes the very assertion the kernels face."""
    x, r64, r32 = R.case(*shape, gated=shape[3] > 1)
    for k in R.names_of(x):
        assert_close(r32[k], r64[k], what=f"float32 restatement {shape} {k}", reduced=k in R.REDUCED, ref32=r32[k])


def test_the_edge_cases_are_what_they_say():
    x, r64, r32 = R.case(**R.LARGE_GATE)
    assert float(r64["s"].max()) > 1000 and float(r64["s"].min()) < -1000
    assert all(bool(torch.isfinite(r32[k]).all()) for k in R.names_of(x))
    x, r64, r32 = R.case(**R.SATURATED)
    pre = torch.einsum("bd,edr->ber", x["xl"].double(), x["V"].double()).abs()
    assert float((pre > 20).double().mean()) > 0.5
    assert all(bool(torch.isfinite(r32[k]).all()) for k in R.names_of(x))


# ---- the model ---------------------------------------------------------------------------------------------------------------------
FLAG_DEFAULTS = {"batch_size": 1024, "learning_rate": 0.005, "hidden_units": "512,256,128", "num_cross_layer": 2,
                 "cross_parameterization": "mix", "low_rank": 32, "num_experts": 4, "structure": "parallel"}


def test_flags_defaults_and_call_surface():
    """(in a child process: a model script imported earlier in this one defines flags of the same names)"""
    code = ("import json; from recalgorithm_amd.algorithm.DCNV2 import dcnv2 as m, cross_layer as l; "
            "acts = {a.dest: a.default for a in m.FLAGS._parser._actions if a.dest != 'help'}; "
            "rest = m.FLAGS._parse(['--cross_parameterization=matrix', '--structure=stacked', '--low_rank=16', '--num_experts=2', "
            "'--num_cross_layer=3']); "
            "print(json.dumps({'flags': acts, 'rest': rest, 'parsed': {k: getattr(m.FLAGS, k) for k in acts}, "
            "'callables': [n for n in ('create_feature_columns', 'example_parser', 'dcnv2_model_fn', 'main') if callable(getattr(m, n))], "
            "'layers': [n for n in ('cross_mix_layer', 'cross_mix_network', 'cross_matrix_layer', 'cross_matrix_network') "
            "if callable(getattr(l, n))], 'units': [m.parse_hidden_units(''), m.parse_hidden_units('32,16')]}))")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert {k: got["flags"][k] for k in FLAG_DEFAULTS} == FLAG_DEFAULTS
    assert {"model_dir", "train_data", "vocabulary_dir", "train_steps", "ragged_capacity"} <= set(got["flags"])
    changed = {"cross_parameterization": "matrix", "structure": "stacked", "low_rank": 16, "num_experts": 2, "num_cross_layer": 3}
    assert got["parsed"] == dict(got["flags"], **changed) and got["rest"] == []
    assert got["callables"] == ["create_feature_columns", "example_parser", "dcnv2_model_fn", "main"]
    assert len(got["layers"]) == 4 and got["units"] == [[], [32, 16]]
    bad = subprocess.run([sys.executable, "-c", "from recalgorithm_amd.algorithm.DCNV2 import dcnv2 as m; m.FLAGS._parse(['--structure=serial'])"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "invalid choice" in bad.stderr


def dcnv2_setup(n_fields=6, K=4, hidden=(32, 16), with_dense=True, **flags):
    """(model_fn, params, synth spec) of algorithm/DCNV2/dcnv2.py on small synthetic columns: 16 dense features and `n_fields`
    single-valued id columns of width K — D = 16 + n_fields K"""
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    from recalgorithm_amd.algorithm.DCNV2.dcnv2 import dcnv2_model_fn
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=n_fields, max_vocab=300, with_dense=with_dense, seed=11, oov_frac=0.05)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES] if with_dense else [],
              "category_feature_columns": [fc.embedding_column(c, K) for c in cats], "hidden_units": list(hidden),
              "num_cross_layer": 2, "cross_parameterization": "mix", "low_rank": 8, "num_experts": 3, "structure": "parallel",
              "learning_rate": 0.005}
    params.update(flags)
    return dcnv2_model_fn, params, spec


def expected_variables(params, D, n_fields, K):
    """name -> shape of every variable of the model but the embedding tables"""
    L, r, E = params["num_cross_layer"], params["low_rank"], params["num_experts"]
    want = {}
    for i in range(L):
        s = f"cross_part/cross_layer_{i}"
        if params["cross_parameterization"] == "mix":
            want.update({f"{s}/V": (E, D, r), f"{s}/C": (E, r, r), f"{s}/U": (E, D, r), f"{s}/gate": (E, D), f"{s}/bias": (D,)})
        else:
            want.update({f"{s}/matrix/kernel": (D, D), f"{s}/matrix/bias": (D,)})
    widths = [D] + [int(u) for u in params["hidden_units"]]
    for i in range(len(widths) - 1):
        want[f"dnn_part/dnn_dense_{i}/kernel"], want[f"dnn_part/dnn_dense_{i}/bias"] = (widths[i], widths[i + 1]), (widths[i + 1],)
    last = widths[-1] if params["structure"] == "stacked" else D + widths[-1]
    want["output_part/dense/kernel"], want["output_part/dense/bias"] = (last, 1), (1,)
    return want


@pytest.mark.parametrize("form,structure", [("mix", "parallel"), ("mix", "stacked"), ("matrix", "parallel"), ("matrix", "stacked")])
def test_variables_on_the_registration_pass(form, structure):
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    from recalgorithm_amd.io import synth
    model_fn, params, spec = dcnv2_setup(cross_parameterization=form, structure=structure)
    feats, lab, _ = synth.device_features(spec, 48, "cpu")
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    est.build(feats, lab)                    # registration pass only: no HIP call
    arrays = est.store.named_arrays()
    D = 16 + 6 * 4
    want = expected_variables(params, D, 6, 4)
    tables = sorted(k for k in arrays if k.endswith("/embedding_weights"))
    assert len(tables) == 6 and all(k.startswith("category_input/input_layer") and arrays[k].shape[1] == 4 for k in tables), tables
    assert sorted(k for k in arrays if k not in tables) == sorted(want)
    for k, shape in want.items():
        assert tuple(arrays[k].shape) == shape, (k, arrays[k].shape, shape)
    if form == "mix":
        w = arrays["cross_part/cross_layer_1/V"]                                # get_variable's default: glorot-uniform
        assert 0 < float(w.abs().max()) <= 1.0 and float(w.mean().abs()) < 0.1
        assert not bool(arrays["cross_part/cross_layer_1/bias"].any())
    est.store.building = True
    try:
        with torch.no_grad():
            pred = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
    finally:
        est.store.building = False
    assert list(pred.predictions) == ["logit", "probabilities"] and tuple(pred.predictions["probabilities"].shape) == (48, 1)
    assert sorted(ev.eval_metric_ops) == ["eval_accuracy", "eval_auc"]
    with pytest.raises(ValueError, match="cross_parameterization='vector'"):
        model_fn(feats, lab, ModeKeys.TRAIN, dict(params, cross_parameterization="vector"))


def test_the_product_imports_neither_the_tests_nor_the_oracle():
    files = [os.path.join(ROOT, "recalgorithm_amd", "algorithm", "DCNV2", f) for f in ("__init__.py", "dcnv2.py", "cross_layer.py")]
    files += [os.path.join(ROOT, "recalgorithm_amd", f) for f in ("ops.py", "nn.py", "_lib.py")] + [os.path.join(ROOT, "scripts", "bench_dcnv2.py")]
    for f in files:
        src = open(f).read()
        assert not re.search(r"^\s*(from|import)\s+(tests|oracle)\b", src, re.M), f
    code = ("import sys; from recalgorithm_amd.algorithm.DCNV2 import dcnv2; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('tests', 'oracle')]; assert not bad, bad")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
