"""CPU-only: include/recalgo_autoint.h (AutoInt's interacting layer as one kernel each way, csrc/autoint.hip) is a header of the
library like the others: listed in _lib.SERVING_HEADERS, bound by load(), and held to every per-header check of tests/test_abi.py
(the pattern of tests/test_ffm_host.py).  The support query's truth table on and one step past every limit, the refusals of both
launching entries on made-up addresses (nothing is launched, so no device is needed), the workspace query; tests/autoint_ref.py:
the header's backward formulas written out against autograd, two identities of the layer, and the condition that keeps the GPU
parity tests honest (the float32 restatement alone meets their bound on every one of their shapes); the model's flags and
defaults, and its variables on the launch-free registration pass."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import autoint_ref as R
from tests import golden_util as GU
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "recalgo_autoint.h"
LAUNCHES = {"recalgo_autoint_layer_fwd", "recalgo_autoint_layer_bwd"}
QUERIES = {"recalgo_autoint_abi_version", "recalgo_autoint_supported", "recalgo_autoint_bwd_partial_rows",
           "recalgo_autoint_bwd_workspace_bytes"}
LIMITS = {"RECALGO_AUTOINT_MIN_F": 2, "RECALGO_AUTOINT_MAX_F": 64, "RECALGO_AUTOINT_MIN_D": 4, "RECALGO_AUTOINT_MAX_D": 64,
          "RECALGO_AUTOINT_MIN_A": 4, "RECALGO_AUTOINT_MAX_A": 32, "RECALGO_AUTOINT_MAX_H": 4, "RECALGO_AUTOINT_MAX_HA": 64,
          "RECALGO_AUTOINT_MAX_PARTIAL_ROWS": 512}


def test_the_header_tables():
    from recalgorithm_amd import _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers()
    abi = _lib.SERVING_HEADERS[NAME]
    assert (abi.version, abi.version_query, abi.label) == (1, "recalgo_autoint_abi_version", "AUTOINT ABI")
    assert set(abi.functions) == LAUNCHES | QUERIES
    assert set(abi.launches) == LAUNCHES and not abi.structs
    assert {k: abi.constants[k] for k in LIMITS} == LIMITS
    lib = _lib.load()
    for name, (res, args) in abi.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name
    # the argument order the header states
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert abi.functions["recalgo_autoint_supported"] == (I, [I] * 4)                                   # F, D, A, H
    assert abi.functions["recalgo_autoint_bwd_partial_rows"] == (I, [I] * 5)                            # B, F, D, A, H
    assert abi.functions["recalgo_autoint_bwd_workspace_bytes"] == (L, [I] * 6)                         # B, F, D, A, H, has_res
    assert abi.functions["recalgo_autoint_layer_fwd"] == (I, [P] * 5 + [I] * 5 + [P] * 2)               # x, wq, wk, wv, wres, .., y, stream
    assert abi.functions["recalgo_autoint_layer_bwd"] == (I, [P] * 7 + [I] * 5 + [P] * 7)               # g, x, y, wq .. wres, .., dx, dwq .. ws, stream


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


# (F, D, A, H) -> served: on and one step past every limit, D and A off their grids, negatives, the dataset's, the benchmark's and
# the paper's shapes
TRUTH = [((1, 8, 8, 2), 0), ((2, 8, 8, 2), 1), ((64, 8, 8, 2), 1), ((65, 8, 8, 2), 0),
         ((7, 0, 8, 2), 0), ((7, 4, 8, 2), 1), ((7, 64, 8, 2), 1), ((7, 68, 8, 2), 0), ((7, 6, 8, 2), 0), ((7, 10, 8, 2), 0),
         ((7, 8, 0, 2), 0), ((7, 8, 4, 2), 1), ((7, 8, 32, 2), 1), ((7, 8, 36, 1), 0), ((7, 8, 6, 2), 0), ((7, 8, 10, 2), 0),
         ((7, 8, 8, 0), 0), ((7, 8, 8, 1), 1), ((7, 8, 8, 4), 1), ((7, 8, 8, 5), 0), ((7, 8, 4, 5), 0),
         ((7, 8, 16, 4), 1), ((7, 8, 20, 4), 0), ((7, 8, 32, 3), 0), ((7, 8, 24, 3), 0), ((7, 8, 20, 3), 1),
         ((-3, 8, 8, 2), 0), ((7, -8, 8, 2), 0), ((7, 8, -8, 2), 0), ((7, 8, 8, -2), 0),
         ((7, 8, 8, 2), 1), ((7, 16, 8, 2), 1), ((26, 16, 8, 2), 1), ((26, 16, 32, 2), 1), ((26, 64, 32, 2), 1), ((64, 64, 32, 2), 1),
         ((64, 64, 16, 4), 1), ((2, 4, 4, 1), 1)]


@pytest.mark.parametrize("shape,served", TRUTH)
def test_the_support_query(shape, served):
    from recalgorithm_amd import _lib, ops
    lib = _lib.load()
    assert lib.recalgo_autoint_supported(*shape) == served
    assert ops.autoint_supported(*shape) == bool(served)
    # the size queries answer 0 for what is not served, and for an empty batch
    assert (lib.recalgo_autoint_bwd_partial_rows(5, *shape) > 0) == bool(served)
    for has_res in (0, 1):
        assert (lib.recalgo_autoint_bwd_workspace_bytes(5, *shape, has_res) > 0) == bool(served)
        assert lib.recalgo_autoint_bwd_workspace_bytes(0, *shape, has_res) == 0
    assert lib.recalgo_autoint_bwd_partial_rows(0, *shape) == 0 and lib.recalgo_autoint_bwd_partial_rows(-1, *shape) == 0


def test_every_parity_shape_is_served():
    from recalgorithm_amd import ops
    assert len(R.SHAPES) == 12
    for B, F, D, A, H, _ in R.SHAPES:
        assert ops.autoint_supported(F, D, A, H), (F, D, A, H)


def _waves(F, D, A, H):
    """csrc/autoint.hip's backward LDS budget restated: the weights [D16][4 C16 + 17] for the workgroup; per wave X [F16][D16 + 1],
    Q, K, V, dZ [F16][C16 + 1], a head's dQ [F16][33] and three statistics of 64 query rows; 160 KiB in all"""
    r16 = lambda v: (v + 15) // 16 * 16                  # noqa: E731
    F16, D16, C16 = r16(F), r16(D), r16(H * A)
    shared, per_wave = D16 * (4 * C16 + 17), F16 * (D16 + 1) + 4 * F16 * (C16 + 1) + F16 * 33 + 3 * 64
    return next(w for w in (4, 2, 1) if 4 * (shared + w * per_wave) <= 160 * 1024)


def test_the_workspace_is_the_documented_rows():
    """rows = min(ceil(B / waves), 512), waves = 4, or 2 or 1 where a workgroup's LDS does not hold four examples' state (one wave
    fits at every corner of the domain); a row is [dWq | dWk | dWv | dWres] = 3 H D A + D H A floats, 3 H D A without the residual term."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    assert [_waves(*s) for s in ((7, 8, 8, 2), (26, 16, 8, 2), (26, 16, 32, 2), (26, 64, 32, 2), (64, 64, 32, 2), (64, 64, 16, 4))] == \
        [4, 4, 2, 2, 1, 1]
    for F, D, A, H in ((2, 4, 4, 1), (7, 8, 8, 2), (26, 16, 8, 2), (26, 16, 32, 2), (26, 64, 32, 2), (64, 64, 32, 2), (64, 64, 16, 4),
                       (64, 8, 4, 4), (33, 4, 32, 1), (48, 64, 32, 2)):
        waves = _waves(F, D, A, H)
        for B in (1, 3, 4, 5, 33, 130, 2048, 2049, 4096, 1 << 20):
            rows = min(-(-B // waves), 512)
            assert lib.recalgo_autoint_bwd_partial_rows(B, F, D, A, H) == rows, (B, F, D, A, H)
            assert lib.recalgo_autoint_bwd_workspace_bytes(B, F, D, A, H, 1) == rows * 4 * H * D * A * 4, (B, F, D, A, H)
            assert lib.recalgo_autoint_bwd_workspace_bytes(B, F, D, A, H, 0) == rows * 3 * H * D * A * 4, (B, F, D, A, H)


def test_refusals_need_no_device():
    """Every refusal returns hipErrorInvalidValue through the errcheck before any launch (made-up addresses: nothing is read): an
    unsupported shape or B < 1, a NULL pointer other than the optional pair, dwres without wres or the reverse, and a pointer that
    is not 4-byte aligned."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    B, F, D, A, H = 5, 7, 8, 8, 2
    # x, wq, wk, wv, wres, B, F, D, A, H, y, stream
    fwd_ok = [P(0x10000 * (i + 1)) for i in range(5)] + [B, F, D, A, H, P(0x90000), None]
    # g, x, y, wq, wk, wv, wres, B, F, D, A, H, dx, dwq, dwk, dwv, dwres, workspace, stream
    bwd_ok = [P(0x10000 * (i + 1)) for i in range(7)] + [B, F, D, A, H] + [P(0x100000 * (i + 1)) for i in range(6)] + [None]
    cases = {"recalgo_autoint_layer_fwd": (fwd_ok, (5, 6, 7, 8, 9), [0, 1, 2, 3, 10], [0, 1, 2, 3, 4, 10]),
             "recalgo_autoint_layer_bwd": (bwd_ok, (7, 8, 9, 10, 11), [0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 17],
                                           [0, 1, 2, 3, 4, 5, 6, 12, 13, 14, 15, 16, 17])}
    for name, (ok, (iB, iF, iD, iA, iH), not_null, pointers) in cases.items():
        fn = getattr(lib, name)
        refused = pytest.raises(_lib.RecalgoError, match=f"{name} failed with hipError_t=1$")

        def call(**changes):
            a = list(ok)
            for i, v in changes.items():
                a[int(i[1:])] = v
            return fn(*a)
        for i, v in ((iF, 1), (iF, 65), (iF, -7), (iD, 0), (iD, 6), (iD, 68), (iA, 0), (iA, 6), (iA, 36), (iH, 0), (iH, 5), (iH, -2),
                     (iB, 0), (iB, -1)):
            with refused:
                call(**{f"a{i}": v})
        with refused:                                     # H A = 96 > 64
            call(**{f"a{iA}": 32, f"a{iH}": 3})
        for i in not_null:
            with refused:
                call(**{f"a{i}": None})
        for i in pointers:
            with refused:
                call(**{f"a{i}": P(ok[i].value + 2)})
    with pytest.raises(_lib.RecalgoError, match="recalgo_autoint_layer_bwd failed with hipError_t=1$"):     # dwres without wres
        lib.recalgo_autoint_layer_bwd(*[None if i == 6 else a for i, a in enumerate(bwd_ok)])
    with pytest.raises(_lib.RecalgoError, match="recalgo_autoint_layer_bwd failed with hipError_t=1$"):     # wres without dwres
        lib.recalgo_autoint_layer_bwd(*[None if i == 16 else a for i, a in enumerate(bwd_ok)])


def test_ops_refuse_on_the_host():
    """ops.autoint_layer raises ValueError before any launch: unsupported sizes, wrong shapes, a non-fp32 or non-device tensor, an
    empty batch (CPU tensors: a call that got as far as a launch would raise RecalgoError instead)."""
    from recalgorithm_amd import ops
    z = torch.zeros
    with pytest.raises(ValueError, match="the kernels serve"):
        ops.autoint_layer(z(4, 7 * 6), 7, z(2, 6, 8), z(2, 6, 8), z(2, 6, 8))
    with pytest.raises(ValueError, match="the kernels serve"):
        ops.autoint_layer(z(4, 65 * 8), 65, z(2, 8, 8), z(2, 8, 8), z(2, 8, 8))
    with pytest.raises(ValueError, match=r"wq must be \[H, D, A\]"):
        ops.autoint_layer(z(4, 56), 7, z(16, 8), z(2, 8, 8), z(2, 8, 8))
    with pytest.raises(ValueError, match="x must be a non-empty"):
        ops.autoint_layer(z(0, 56), 7, z(2, 8, 8), z(2, 8, 8), z(2, 8, 8))
    with pytest.raises(ValueError, match="x must be a non-empty"):
        ops.autoint_layer(z(4, 57), 7, z(2, 8, 8), z(2, 8, 8), z(2, 8, 8))
    with pytest.raises(ValueError, match="wk has shape"):
        ops.autoint_layer(z(4, 56), 7, z(2, 8, 8), z(2, 8, 4), z(2, 8, 8))
    with pytest.raises(ValueError, match="wres has shape"):
        ops.autoint_layer(z(4, 56), 7, z(2, 8, 8), z(2, 8, 8), z(2, 8, 8), z(16, 8))
    with pytest.raises(ValueError, match="x must be a contiguous float32 tensor on x's device"):
        ops.autoint_layer(z(4, 56, dtype=torch.float64), 7, z(2, 8, 8), z(2, 8, 8), z(2, 8, 8))
    with pytest.raises(ValueError, match="x must be a contiguous float32 tensor on x's device"):        # (a CPU tensor)
        ops.autoint_layer(z(4, 56), 7, z(2, 8, 8), z(2, 8, 8), z(2, 8, 8))


# ---- tests/autoint_ref.py ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3, 8, 4, 3, True), (4, 17, 12, 8, 2, True), (6, 9, 16, 8, 2, False)])
def test_the_headers_backward_formulas_are_autograds(shape):
    x, r64, _ = R.case(*shape, seed=3)
    x64 = {k: (None if v is None else v.double()) for k, v in x.items()}
    by_hand = R.backward_by_hand(x64, x64["g"])
    assert bool((r64["y"] == 0).any()) and bool((r64["y"] > 0).any()), "both sides of the ReLU"
    for k in R.names_of(x)[1:]:
        assert torch.allclose(by_hand[k], r64[k], rtol=1e-11, atol=1e-13), k
    assert (by_hand["dwres"] is None) == (x["wres"] is None)


def test_zero_queries_give_the_field_mean_of_the_values():
    x, _, _ = R.case(4, 9, 16, 8, 2, False)
    x64 = {k: (None if v is None else v.double()) for k, v in x.items()}
    y, s, p = R.layer(x64["x"], torch.zeros_like(x64["wq"]), x64["wk"], x64["wv"], None, return_scores=True)
    assert bool((s == 0).all()) and torch.allclose(p, torch.full_like(p, 1.0 / 9), rtol=0, atol=1e-16)
    v = torch.einsum("bfd,hda->bhfa", x64["x"], x64["wv"]).mean(dim=2)                   # [B, H, A]: the field mean
    want = torch.relu(v.reshape(4, 1, 16).expand(4, 9, 16))
    assert torch.allclose(y, want, rtol=1e-13, atol=1e-15)


def test_a_permutation_of_the_fields_permutes_the_rows():
    x, r64, _ = R.case(4, 9, 16, 8, 2, True)
    perm = torch.randperm(9, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(perm, torch.arange(9))
    y = R.layer(x["x"].double()[:, perm], x["wq"].double(), x["wk"].double(), x["wv"].double(), x["wres"].double())
    assert torch.allclose(y, r64["y"][:, perm], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_the_float32_restatement_alone_meets_the_gpu_bound(shape):
    """What keeps tests/test_gpu_autoint.py's parity test one of the kernels: at every one of its shapes the same arithmetic in
    float32 torch passes the very assertion the kernels face."""
    x, r64, r32 = R.case(*shape)
    for k in R.names_of(x):
        assert_close(r32[k], r64[k], what=f"float32 restatement {shape} {k}", reduced=k in R.REDUCED, ref32=r32[k])


def test_the_large_score_case_is_one():
    """x and Wq, Wk scaled by 3: the scores reach +-1600 (an unshifted exp would overflow), and the float32 restatement itself
    leaves elements of dx outside the plain bound — the GPU test judges with the floor of 4 x its deviation."""
    from tests.afm_ref import outside_rtol
    x, r64, r32 = R.case(**R.LARGE)
    assert float(r64["s"].max()) > 1000 and float(r64["s"].min()) < -1000
    assert all(bool(torch.isfinite(r32[k]).all()) for k in R.names_of(x))
    assert outside_rtol(r32["dx"], r64["dx"]) > 100


# ---- the model ---------------------------------------------------------------------------------------------------------------------
FLAG_DEFAULTS = {"batch_size": 1024, "learning_rate": 0.005, "embedding_dim": 8, "att_embedding_size": 8, "head_num": 2,
                 "num_interacting_layers": 3, "use_residual": True, "hidden_units": "", "batch_norm": True, "dropout_rate": 0.0}


def autoint_setup(vocab_dir, **overrides):
    """(model_fn, params) of algorithm/AutoInt/autoint.py on the dataset's columns, from its own create_feature_columns()"""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.AutoInt import autoint as m
    flags.FLAGS.vocabulary_dir = vocab_dir
    fl = dict(FLAG_DEFAULTS, **overrides)
    flags.FLAGS.embedding_dim = fl["embedding_dim"]
    dense, cat, _ = m.create_feature_columns()
    return m.autoint_model_fn, {
        "dense_feature_columns": dense, "category_feature_columns": cat, "embedding_dim": fl["embedding_dim"],
        "att_embedding_size": fl["att_embedding_size"], "head_num": fl["head_num"],
        "num_interacting_layers": fl["num_interacting_layers"], "use_residual": fl["use_residual"],
        "hidden_units": m.parse_hidden_units(fl["hidden_units"]), "batch_norm": fl["batch_norm"], "dropout_rate": fl["dropout_rate"],
        "learning_rate": fl["learning_rate"]}


def test_flags_defaults_and_call_surface():
    """(in a child process: a model script imported earlier in this one defines flags of the same names)"""
    code = ("import json, inspect; from recalgorithm_amd.algorithm.AutoInt import autoint as m, interacting_layer as l; "
            "acts = {a.dest: a.default for a in m.FLAGS._parser._actions if a.dest != 'help'}; "
            "print(json.dumps({'flags': acts, 'parsed': {k: getattr(m.FLAGS, k) for k in acts}, "
            "'callables': [n for n in ('create_feature_columns', 'example_parser', 'autoint_model_fn', 'main') if callable(getattr(m, n))], "
            "'layer': str(inspect.signature(l.interacting_layer)), 'units': [m.parse_hidden_units(''), m.parse_hidden_units('32,16')]}))")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert {k: got["flags"][k] for k in FLAG_DEFAULTS} == FLAG_DEFAULTS and got["parsed"] == got["flags"]
    assert {"model_dir", "train_data", "vocabulary_dir", "train_steps", "ragged_capacity"} <= set(got["flags"])
    assert got["callables"] == ["create_feature_columns", "example_parser", "autoint_model_fn", "main"]
    assert got["layer"] == "(input, field_num, att_embedding_size=8, head_num=2, use_res=True, index=0)"
    assert got["units"] == [[], [32, 16]]


@pytest.mark.parametrize("hidden,use_res", [("", True), ("32,16", True), ("", False)])
def test_variables_on_the_registration_pass(hidden, use_res, tmp_path):
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = autoint_setup(vocab_dir, hidden_units=hidden, use_residual=use_res)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    est.build(feats, lab)                    # registration pass only: no HIP call
    arrays = est.store.named_arrays()
    F, K, H, A, L = 7, 8, 2, 8, 3
    want = {"dense_input/dense_logit/kernel": (16, 1), "dense_input/dense_logit/bias": (1,),
            "prediction_part/autoint_logit/kernel": (F * H * A, 1), "prediction_part/autoint_logit/bias": (1,)}
    for i in range(L):
        D = K if i == 0 else H * A
        for n in ("query", "key", "value"):
            want[f"interacting_part/interacting_layer_{i}_w_{n}"] = (H, D, A)
        if use_res:
            want[f"interacting_part/interacting_layer_{i}_w_res"] = (D, H * A)
    widths = [F * K] + [int(u) for u in hidden.split(",") if u]
    for i in range(len(widths) - 1):
        sfx = "" if i == 0 else f"_{i}"
        want[f"deep_part/dense{sfx}/kernel"], want[f"deep_part/dense{sfx}/bias"] = (widths[i], widths[i + 1]), (widths[i + 1],)
        for n in ("gamma", "beta", "moving_mean", "moving_variance"):
            want[f"deep_part/batch_normalization{sfx}/{n}"] = (widths[i + 1],)
    if hidden:
        want["deep_part/deep_logit/kernel"], want["deep_part/deep_logit/bias"] = (widths[-1], 1), (1,)
    tables = sorted(k for k in arrays if k.endswith("/embedding_weights"))
    assert len(tables) == F and all(k.startswith("interacting_part/input_layer") and arrays[k].shape[1] == K for k in tables), tables
    assert sorted(k for k in arrays if k not in tables) == sorted(want)
    for k, shape in want.items():
        assert tuple(arrays[k].shape) == shape, (k, arrays[k].shape, shape)
    w = arrays["interacting_part/interacting_layer_1_w_query"]              # get_variable's default: glorot-uniform
    assert 0 < float(w.abs().max()) <= 1.0 and float(w.mean().abs()) < 0.1
    est.store.building = True
    try:
        with torch.no_grad():
            pred = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
    finally:
        est.store.building = False
    assert list(pred.predictions) == ["logit", "probabilities"] and tuple(pred.predictions["probabilities"].shape) == (48, 1)
    assert sorted(ev.eval_metric_ops) == ["eval_accuracy", "eval_auc"]
