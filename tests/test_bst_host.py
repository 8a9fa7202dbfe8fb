"""CPU (no kernels launched): the BST feature's host side.
  * the mask rule tests/bst_ref.py restates: query rows >= keys_length have a softmax of exactly 1/T in float32 and still
    pass a gradient to Q and K; the float64 run models that step;
  * include/recalgo_bst.h, the fourth ABI header: its names, signatures, launches, sizes and constants, literally, and the
    constants re-exported (the checks every header gets, include/recalgo_bst.abi among them: tests/test_abi.py);
  * tests/bst_ref.py reproduces both goldens scripts/gen_golden_bst.py obtained by executing the reference's own bst.py on
    oracle/tf1_shim (predictions, loss, every gradient, the Adam step, the moving statistics, EVAL), the generator's --check
    round trip (where the reference folder exists);
  * the mirror's variables, flags and call surface on the launch-free registration pass; what --static_sequence_length
    changes and when it changes nothing."""
import ctypes
import os
import re

import pytest
import torch

from tests import bst_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_bst.h")


# ---- the mask rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("T", [1, 3, 7, 51])
def test_rows_past_keys_length_are_exactly_uniform_and_still_pass_gradients(T, dtype):
    B, d, H = 6, 16, 3
    case = R.random_case(B, T, d, H, seed=T)
    case["keys_length"] = torch.tensor([0, 1, T, T + 4, max(T - 1, 0), T // 2], dtype=torch.int32)
    c = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in case.items()}
    x = c["x"].clone().requires_grad_(True)
    p, q, k = R.probabilities(x, c["keys_length"], c["pos"], c["w_q"], c["w_k"])
    q.retain_grad(), k.retain_grad()
    kl = c["keys_length"].clamp(0, T).tolist()
    uniform = torch.tensor(1.0, dtype=dtype) / T

    def is_uniform(rows):
        # float32, the reference's arithmetic: exactly 1/T.  float64 (the straight-through model): every entry of a row is the
        # same number, 1/T up to the two roundings of a softmax that multiplies by a reciprocal
        if dtype == torch.float32:
            return bool(torch.all(rows == uniform))
        return bool(torch.all(rows == rows[..., :1])) and bool(torch.all((rows - uniform).abs() <= 2 * 2.3e-16 * uniform))
    for b in range(B):
        if kl[b] < T:
            assert is_uniform(p[b, :, kl[b]:, :]), f"example {b}: a masked row is not exactly 1/T"
        if kl[b] > 0 and T > 1:
            assert not is_uniform(p[b, :, :kl[b], :]), f"example {b}: a valid row is uniform"
    assert is_uniform(p[0]), "keys_length 0: every row is uniform"
    # the add's gradient is the identity: ds = p (dp - <p, dp>) with p = 1/T flows into Q and K of the masked rows
    w = torch.rand(p.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dtype)
    (p * w).sum().backward()
    if T > 1:
        assert bool((q.grad[0].abs().sum(dim=-1) > 0).all()) and bool((k.grad[0].abs().sum(dim=-1) > 0).all())
        for b in range(B):
            if kl[b] < T:
                assert bool((q.grad[b, :, kl[b]:].abs().sum(dim=-1) > 0).all()), f"example {b}: no dQ on a masked row"
    assert torch.isfinite(x.grad).all()


def test_float32_add_absorbs_and_float64_does_not():
    s = torch.tensor([[[[100.0, -127.0], [3.0, 0.5]]]])
    kl = torch.tensor([0])
    assert torch.all(R.add_mask(s, kl) == R.MASK_ADD)
    raw = s.double() + R.MASK_ADD
    assert not torch.all(raw == R.MASK_ADD), "float64 keeps the scores: the restatement has to model the fp32 step"
    assert torch.all(R.add_mask(s.double(), kl) == R.MASK_ADD)


# ---- include/recalgo_bst.h: what this feature expects of its header, literally (every generic check: tests/test_abi.py) -----------
DECLARED = ["recalgo_bst_abi_version", "recalgo_bst_supported", "recalgo_bst_attn_bwd_partial_rows",
            "recalgo_bst_attn_bwd_workspace_bytes", "recalgo_bst_ffn_bwd_partial_rows", "recalgo_bst_ffn_bwd_workspace_bytes",
            "recalgo_bst_attn_fwd", "recalgo_bst_attn_bwd", "recalgo_bst_ffn_fwd", "recalgo_bst_ffn_bwd"]
LAUNCHES = ["recalgo_bst_attn_fwd", "recalgo_bst_attn_bwd", "recalgo_bst_ffn_fwd", "recalgo_bst_ffn_bwd"]


def test_fourth_header_literal_expectations():
    from recalgorithm_amd import _lib, build, ops
    build.build(verbose=False)
    abi = _lib.HEADERS["recalgo_bst.h"]
    assert sorted(abi.functions) == sorted(DECLARED)
    assert abi.launches == LAUNCHES
    assert not abi.structs
    lib = _lib.load()
    assert lib.recalgo_bst_abi_version() == abi.version == 1
    c_int, i64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    F = abi.functions
    assert F["recalgo_bst_abi_version"] == (c_int, []) and F["recalgo_bst_ffn_bwd_partial_rows"] == (c_int, [c_int])
    assert F["recalgo_bst_supported"] == (c_int, [c_int] * 3) and F["recalgo_bst_attn_bwd_partial_rows"] == (c_int, [c_int])
    assert F["recalgo_bst_attn_bwd_workspace_bytes"] == (i64, [c_int] * 4) and F["recalgo_bst_ffn_bwd_workspace_bytes"] == (i64, [c_int] * 2)
    assert F["recalgo_bst_attn_fwd"] == (c_int, [ptr] * 9 + [c_int] * 4 + [ptr] * 3)
    assert F["recalgo_bst_attn_bwd"] == (c_int, [ptr] * 9 + [c_int] * 4 + [ptr] * 10)
    assert F["recalgo_bst_ffn_fwd"] == (c_int, [ptr] * 5 + [c_int] * 4 + [ptr] * 4)
    assert F["recalgo_bst_ffn_bwd"] == (c_int, [ptr] * 6 + [c_int] * 4 + [ptr] * 7)
    # the sizes and limits the header states (host-side queries: no device needed)
    assert [lib.recalgo_bst_supported(T, d, H) for T, d, H in ((1, 4, 1), (64, 16, 4), (51, 16, 3), (65, 16, 3), (51, 5, 3), (51, 16, 5))] \
        == [1, 1, 1, 0, 0, 0]
    assert lib.recalgo_bst_attn_bwd_partial_rows(3) == 3 and lib.recalgo_bst_attn_bwd_partial_rows(10 ** 6) == 512
    assert lib.recalgo_bst_attn_bwd_workspace_bytes(4096, 51, 16, 3) == 4 * 512 * (51 * 16 + 4 * 3 * 256 + 32)
    assert lib.recalgo_bst_ffn_bwd_workspace_bytes(7, 16) == 4 * 7 * (256 + 48)
    assert lib.recalgo_bst_attn_bwd_workspace_bytes(8, 65, 16, 3) == 0 and lib.recalgo_bst_ffn_bwd_workspace_bytes(8, 5) == 0
    # a launch that returns an error raises through the errcheck (NULL buffers: refused before any launch)
    with pytest.raises(_lib.RecalgoError, match="recalgo_bst_attn_fwd failed with hipError_t=1$"):
        lib.recalgo_bst_attn_fwd(*([None] * 9), 1, 1, 4, 1, None, None, None)
    with pytest.raises(_lib.RecalgoError, match="recalgo_bst_attn_bwd failed with hipError_t=1$"):
        lib.recalgo_bst_attn_bwd(*([None] * 9), 1, 1, 4, 1, *([None] * 10))
    with pytest.raises(_lib.RecalgoError, match="recalgo_bst_ffn_fwd failed with hipError_t=1$"):
        lib.recalgo_bst_ffn_fwd(*([None] * 5), 1, 1, 4, 0, None, None, None, None)
    with pytest.raises(_lib.RecalgoError, match="recalgo_bst_ffn_bwd failed with hipError_t=1$"):
        lib.recalgo_bst_ffn_bwd(*([None] * 6), 1, 1, 4, 0, *([None] * 7))
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RECALGO_BST_\w+) (0x[0-9A-Fa-f]+|\d+)", open(HEADER).read())
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_BST_ABI_VERSION": 1, "RECALGO_BST_MAX_T": 64, "RECALGO_BST_MAX_D": 16,
                                        "RECALGO_BST_MAX_HEADS": 4}
    assert (ops.BST_MAX_T, ops.BST_MAX_D, ops.BST_MAX_HEADS) == (64, 16, 4)


# ---- the goldens: tests/bst_ref.py against the reference's own sources run on oracle/tf1_shim ------------------------------------
import subprocess  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402

from tests import golden_util as GU  # noqa: E402
from tests.golden_protocol import GoldenCase, close, restate_on_host  # noqa: E402
from tests.test_mmoe_host import encode  # noqa: E402

GOLDENS = {"model_bst": 28, "model_bst_two_blocks_mean_dropout": 38}          # name -> gradient arrays


def mirror_setup(name, vocab_dir, **extra):
    """(model_fn, params) of the mirror for golden `name`, from the mirror's own create_feature_columns()."""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.BST import bst as m
    d = GU.load(name)
    fl = {k: (v.item() if v.shape == () else v) for k, v in GU.section(d, "flag/").items()}
    flags.FLAGS.vocabulary_dir = vocab_dir
    for k, v in fl.items():
        setattr(flags.FLAGS, k, v)
    dense, cat, tgt, seq, _ = m.create_feature_columns()
    return m.bst_model_fn, dict({
        "dense_feature_columns": dense, "category_feature_columns": cat, "sequence_feature_columns": seq,
        "target_feedid_feature_columns": tgt, "hidden_units": str(fl["hidden_units"]).split(","),
        "dropout_rate": float(fl["dropout_rate"]), "batch_norm": bool(fl["batch_norm"]), "learning_rate": float(fl["learning_rate"]),
        "sequence_max_length": int(fl["sequence_max_length"]), "num_transformer_block": int(fl["num_transformer_block"]),
        "num_transformer_heads": int(fl["num_transformer_heads"]), "pooling_method": str(fl["pooling_method"])}, **extra)


CASE = GoldenCase(mirror_setup=mirror_setup, oracle=R.bst, encode=encode, predictions={"probabilities": ("prob",)},
                  ordered_prediction_keys=True, n_grads=GOLDENS, n_masks=2)


@pytest.mark.parametrize("name", list(GOLDENS))
def test_restatement_reproduces_the_golden(name, tmp_path):
    """The goldens are float64 (the shim's stand-in for tf.float32, the mask's float32 step modelled): the restatement runs in
    float64, with the straight-through mask, at the bound of every model's restatement."""
    bn_state = {}
    golden, run = restate_on_host(CASE, name, tmp_path, bn_state=bn_state)
    feats, P, gg, ga = run["feats"], run["P"], golden.grad, golden.var_after
    lens = feats["his_read_comment_7d_seq"][1][1:] - feats["his_read_comment_7d_seq"][1][:-1]
    assert int(lens.min()) == 0 and int(lens.max()) == 8 and int((lens < 8).sum()) > 0, "the batch has padded rows and an empty history"
    # the position embedding: rows nobody reads keep a zero gradient; with two blocks the read rows hold both blocks' share
    gpos = gg["transformer_part/position_embedding"]
    assert gpos.shape == (51, 16) and np.all(gpos[9:] == 0.0) and np.all(np.abs(gpos[:9]).sum(axis=1) > 0)
    assert bn_state
    for scope, (mean, var) in bn_state.items():
        close(0.99 * P[f"{scope}/moving_mean"].detach() + 0.01 * mean, ga[f"{scope}/moving_mean"], f"{name} {scope} moving_mean")
        close(0.99 * P[f"{scope}/moving_variance"].detach() + 0.01 * var, ga[f"{scope}/moving_variance"], f"{name} {scope} moving_variance")


def test_restatement_in_float32_stays_at_float32_distance_from_the_golden(tmp_path):
    """The float32 run of the restatement (ref32 of the GPU tests: the literal mask add) agrees with the float64 golden to
    float32 rounding: the two mask rules are the same rule."""
    name = "model_bst_two_blocks_mean_dropout"
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    _, params = mirror_setup(name, vocab_dir)
    d = GU.load(name)
    sfeats, _ = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in encode(params, sfeats).items()}
    P = {k: torch.from_numpy(v.copy()).float() for k, v in GU.section(d, "var/").items()}
    out = R.bst(P, feats, None, params, training=False)
    assert out["prob"].dtype == torch.float32
    # 2 blocks x (a softmax, two LayerNorms with unit-scale outputs) + the tower: a few hundred roundings of 6e-8 relative on
    # values of order 1..10 ahead of a sigmoid whose slope is at most 1/4
    assert float((out["prob"].double() - torch.from_numpy(d["predict/probabilities"])).abs().max()) < 2e-5


def test_generator_check_round_trip():
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, "BST")):
        pytest.skip("the reference folder is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_golden_bst.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "model_bst.npz  checked" in r.stdout and "model_bst_two_blocks_mean_dropout.npz  checked" in r.stdout


# ---- the mirror on the launch-free registration pass ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GOLDENS))
def test_mirror_variables_on_the_registration_pass(name, tmp_path):
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup(name, vocab_dir)
    d = GU.load(name)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    est.build(feats, lab)                    # registration pass only: no HIP call
    arrays = est.store.named_arrays()
    gv = GU.section(d, "var/")
    assert not [k for k in gv if k not in arrays], "reference variables absent from the mirror"
    assert not [k for k in arrays if k not in gv], "mirror variables the reference does not have"
    for k, v in gv.items():
        assert tuple(arrays[k].shape) == tuple(v.shape), (k, arrays[k].shape, v.shape)
    pos = arrays["transformer_part/position_embedding"]
    assert float(pos.abs().max()) <= (6.0 / (51 + 16)) ** 0.5 and float(pos.abs().max()) > 0       # glorot-uniform
    assert torch.all(arrays["transformer_part/LayerNorm/gamma"] == 1) and torch.all(arrays["transformer_part/LayerNorm_1/beta"] == 0)
    est.store.building = True
    try:
        with torch.no_grad():
            pred = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
    finally:
        est.store.building = False
    assert list(pred.predictions) == ["probabilities"] and tuple(pred.predictions["probabilities"].shape) == (48, 1)
    assert sorted(ev.eval_metric_ops) == ["eval_accuracy", "eval_auc"]


def test_reference_flag_defaults_and_call_surface():
    """bst.py:21-48 (checked in a child process: a model script imported earlier in this one defines flags of the same names)"""
    code = ("from recalgorithm_amd.algorithm.BST import bst as m, transformer_layer as t, leakyrelu as l; F = m.FLAGS; "
            "print(F.batch_size, F.learning_rate, F.hidden_units, F.batch_norm, F.dropout_rate, F.sequence_max_length, "
            "F.num_transformer_block, F.num_transformer_heads, F.pooling_method, F.static_sequence_length, F.train_steps); "
            "print(all(callable(getattr(m, n)) for n in ('create_feature_columns', 'example_parser', 'bst_model_fn', 'main')), "
            "callable(t.bst_transformer), float(l.leakyrelu(__import__('torch').tensor(-2.0))))")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1024 0.005 512,256,128 True 0.1 50 1 3 sum False 10000"
    assert lines[-1].startswith("True True -0.0") and abs(float(lines[-1].split()[-1]) + 0.02) < 1e-6


def test_sizes_the_kernels_do_not_serve_are_refused_clearly(tmp_path):
    from recalgorithm_amd.estimator import Estimator, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup("model_bst", vocab_dir, num_transformer_heads=5)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    with pytest.raises(ValueError, match="there is no fallback"):
        est.build(feats, {"read_comment": labels.float()})


def test_static_sequence_length_equals_the_reference_exactly_when_a_history_is_full_length(tmp_path):
    """T enters the softmax width, LayerNorm's moments and the pooling: padding to sequence_max_length + 1 is the reference's
    computation when the batch's longest history IS sequence_max_length (8 in the golden batch), and another one otherwise."""
    name = "model_bst_two_blocks_mean_dropout"
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    _, params = mirror_setup(name, vocab_dir)
    d = GU.load(name)
    sfeats, _ = GU.string_batch()
    feats = encode(params, sfeats)
    P = {k: torch.from_numpy(v.copy()) for k, v in GU.section(d, "var/").items()}
    full = R.bst(P, feats, None, dict(params, static_sequence_length=True, sequence_max_length=8), training=False)
    assert torch.equal(full["prob"], R.bst(P, feats, None, params, training=False)["prob"])
    close(full["prob"], d["predict/probabilities"], "static T = longest history + 1")
    padded = R.bst(P, feats, None, dict(params, static_sequence_length=True), training=False)
    assert float((padded["prob"] - full["prob"]).abs().max()) > 1e-3
