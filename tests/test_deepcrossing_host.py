"""CPU (no kernels launched): the DeepCrossing feature's host side.
  * tests/deepcrossing_ref.py reproduces both goldens scripts/gen_golden_deepcrossing.py obtained by executing the
    reference's own deepcrossing.py on oracle/tf1_shim (predictions, loss, every gradient, the Adam step, EVAL) at 1e-10; the
    generator's --check round trip (where the reference folder exists); the float32 run of the restatement against float64;
  * no pre-activation of a ReLU of a committed golden lies within 2e-5 of its layer's scale of zero (the generator's rule,
    re-evaluated here from the committed variables);
  * the backward from given masks (what the kernel's backward entry computes) is autograd's backward of the forward;
  * include/recalgo_res.h, the fifth ABI header: its names, signatures, launches and constants, literally (the checks every
    header gets, include/recalgo_res.abi among them: tests/test_abi.py);
  * the mirror's variables on the launch-free registration pass, its flags (names, defaults, help texts) and call surface."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import deepcrossing_ref as R
from tests import golden_util as GU
from tests.golden_protocol import GoldenCase, load_golden, restate_on_host
from tests.test_mmoe_host import encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> gradient arrays: 7 embedding tables, kernel and bias of the head, 4 per residual unit
GOLDENS = {"model_deepcrossing": 13, "model_deepcrossing_three_units": 21}
UNITS = {"model_deepcrossing": (1, 128), "model_deepcrossing_three_units": (3, 32)}


def mirror_setup(name, vocab_dir, **extra):
    """(model_fn, params) of the mirror for golden `name`, from the mirror's own create_feature_columns()."""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.DeepCrossing import deepcrossing as m
    d = GU.load(name)
    fl = {k: (v.item() if v.shape == () else v) for k, v in GU.section(d, "flag/").items()}
    flags.FLAGS.vocabulary_dir = vocab_dir
    for k, v in fl.items():
        setattr(flags.FLAGS, k, v)
    dense, cat, _ = m.create_feature_columns()
    return m.deepcrossing_model_fn, dict({
        "category_feature_columns": cat, "dense_feature_columns": dense,
        "residual_internal_dim": int(fl["residual_internal_dim"]), "residual_network_num": int(fl["residual_network_num"]),
        "learning_rate": float(fl["learning_rate"])}, **extra)


CASE = GoldenCase(mirror_setup=mirror_setup, oracle=R.deepcrossing, encode=encode,
                  predictions={"logit": ("logit",), "probabilities": ("prob",)}, ordered_prediction_keys=True, n_grads=GOLDENS)


# ---- the goldens -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GOLDENS))
def test_restatement_reproduces_the_golden(name, tmp_path):
    golden, run = restate_on_host(CASE, name, tmp_path)
    L, H = UNITS[name]
    assert (int(golden.d["flag/residual_network_num"]), int(golden.d["flag/residual_internal_dim"])) == (L, H)
    D = 16 + 16 + 2 + 4 + 4 + 4 + 4 + 16 + 16                # 16 dense features + the eight embedding columns
    assert golden.var["residual_module/dense_0_0/kernel"].shape == (D, H) and D == 82
    assert golden.var[f"residual_module/dense_{L - 1}_1/kernel"].shape == (H, D)
    assert os.path.getsize(os.path.join(GU.GOLDEN, name + ".npz")) <= 600 * 1000


@pytest.mark.parametrize("name", list(GOLDENS))
def test_no_pre_activation_of_a_committed_golden_is_near_zero(name, tmp_path):
    """The generator's rule on the committed file: an fp32 evaluation cannot take the other side of any ReLU."""
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    _, params = mirror_setup(name, vocab_dir)
    golden = load_golden(CASE, name, params)
    sfeats, _ = GU.string_batch()
    P = {k: torch.from_numpy(v.copy()) for k, v in golden.var.items()}
    margins = R.relu_margins(P, encode(params, sfeats), params)
    assert len(margins) == 2 * UNITS[name][0]
    assert min(margins) > 2e-5, margins
    assert abs(min(margins) - float(golden.d["meta/relu_margin"])) <= 1e-9, "meta/relu_margin is the smallest of them"
    assert int(golden.d["meta/seed"]) >= 4242


def test_restatement_in_float32_stays_at_float32_distance_from_the_golden(tmp_path):
    """The float32 run of the restatement (ref32 of the GPU tests) against the float64 golden, at the bound of
    tests/test_bst_host.py's float32 check: a few hundred roundings of 6e-8 relative on values of order 1..10 ahead of a
    sigmoid whose slope is at most 1/4."""
    name = "model_deepcrossing_three_units"
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    _, params = mirror_setup(name, vocab_dir)
    d = GU.load(name)
    sfeats, _ = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in encode(params, sfeats).items()}
    P = {k: torch.from_numpy(v.copy()).float() for k, v in GU.section(d, "var/").items()}
    out = R.deepcrossing(P, feats, None, params, training=False)
    assert out["prob"].dtype == torch.float32
    assert float((out["prob"].double() - torch.from_numpy(d["predict/probabilities"])).abs().max()) < 2e-5


def test_generator_check_round_trip():
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, "DeepCrossing")):
        pytest.skip("the reference folder is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_golden_deepcrossing.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "model_deepcrossing.npz  checked" in r.stdout and "model_deepcrossing_three_units.npz  checked" in r.stdout


# ---- the bare stack ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,H,L", [(5, 7, 16, 1), (9, 82, 32, 3)])
def test_backward_from_given_masks_is_the_backward_of_the_forward(B, D, H, L):
    c = R.random_stack(B, D, H, L, seed=D)
    leaves = {k: [t.clone().requires_grad_(True) for t in c[k]] for k in ("w0", "b0", "w1", "b1")}
    x = c["x"].clone().requires_grad_(True)
    hs, ys = R.stack_forward(x, leaves["w0"], leaves["b0"], leaves["w1"], leaves["b1"])
    assert hs.shape == (L, B, H) and ys.shape == (L, B, D)
    assert bool((hs == 0).any()) and bool((hs > 0).any()) and bool((ys == 0).any()) and bool((ys > 0).any()), "both sides of both ReLUs"
    ys[-1].backward(c["g"])
    dzs, dhs, dx = R.stack_backward(c["g"], hs.detach(), ys.detach(), c["w0"], c["w1"])
    assert torch.allclose(dx, x.grad, rtol=1e-12, atol=1e-14)
    assert bool((dzs[ys.detach() <= 0] == 0).all()) and bool((dhs[hs.detach() <= 0] == 0).all())
    for l, grads in enumerate(R.weight_grads(c["x"], hs.detach(), ys.detach(), dzs, dhs)):
        for got, k in zip(grads, ("w0", "b0", "w1", "b1")):
            assert torch.allclose(got, leaves[k][l].grad, rtol=1e-12, atol=1e-14), (l, k)


# ---- include/recalgo_res.h: what this feature expects of its header, literally (every generic check: tests/test_abi.py) -------------
def test_fifth_header_literal_expectations():
    from recalgorithm_amd import _lib, build, ops
    build.build(verbose=False)
    assert list(_lib.HEADERS)[-1] == "recalgo_res.h" and len(_lib.HEADERS) == 5
    abi = _lib.HEADERS["recalgo_res.h"]
    assert list(abi.functions) == ["recalgo_res_abi_version", "recalgo_res_supported", "recalgo_res_stack_fwd", "recalgo_res_stack_bwd"]
    assert abi.launches == ["recalgo_res_stack_fwd", "recalgo_res_stack_bwd"] and not abi.structs
    lib = _lib.load()
    assert lib.recalgo_res_abi_version() == abi.version == 1
    c_int, ptr = ctypes.c_int, ctypes.c_void_p
    F = abi.functions
    assert F["recalgo_res_abi_version"] == (c_int, []) and F["recalgo_res_supported"] == (c_int, [c_int] * 3)
    assert F["recalgo_res_stack_fwd"] == (c_int, [ptr] * 5 + [c_int] * 5 + [ptr] * 3)
    assert F["recalgo_res_stack_bwd"] == (c_int, [ptr] * 5 + [c_int] * 4 + [ptr] * 4)
    assert abi.constants == {"RECALGO_RES_ABI_VERSION": 1, "RECALGO_RES_MAX_D": 512, "RECALGO_RES_MAX_H": 256, "RECALGO_RES_MAX_UNITS": 8}
    assert (ops.RES_MAX_D, ops.RES_MAX_H, ops.RES_MAX_UNITS) == (512, 256, 8)
    served = [(1, 16, 1), (82, 128, 1), (82, 32, 3), (432, 128, 3), (512, 256, 8), (83, 48, 2)]
    refused = [(0, 16, 1), (513, 16, 1), (82, 0, 1), (82, 8, 1), (82, 40, 1), (82, 272, 1), (82, 128, 0), (82, 128, 9)]
    assert [lib.recalgo_res_supported(*s) for s in served] == [1] * len(served)
    assert [lib.recalgo_res_supported(*s) for s in refused] == [0] * len(refused)
    # a launch that returns an error raises through the errcheck (NULL buffers: refused before any launch)
    with pytest.raises(_lib.RecalgoError, match="recalgo_res_stack_fwd failed with hipError_t=1$"):
        lib.recalgo_res_stack_fwd(*([None] * 5), 1, 82, 128, 1, 0, None, None, None)
    with pytest.raises(_lib.RecalgoError, match="recalgo_res_stack_bwd failed with hipError_t=1$"):
        lib.recalgo_res_stack_bwd(*([None] * 5), 1, 82, 128, 1, *([None] * 4))


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
    assert sorted(arrays) == sorted(gv), "the mirror's variable names are the reference's"
    for k, v in gv.items():
        assert tuple(arrays[k].shape) == tuple(v.shape), (k, arrays[k].shape, v.shape)
    L, H = UNITS[name]
    for i in range(L):                       # tf.layers.dense: glorot-uniform kernel, zero bias
        for j, fans in enumerate(((82, H), (H, 82))):
            kern, bias = arrays[f"residual_module/dense_{i}_{j}/kernel"], arrays[f"residual_module/dense_{i}_{j}/bias"]
            assert 0 < float(kern.abs().max()) <= (6.0 / sum(fans)) ** 0.5 and torch.all(bias == 0)
    est.store.building = True
    try:
        with torch.no_grad():
            pred = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
    finally:
        est.store.building = False
    assert list(pred.predictions) == ["logit", "probabilities"] and tuple(pred.predictions["probabilities"].shape) == (48, 1)
    assert sorted(ev.eval_metric_ops) == ["eval_accuracy", "eval_auc"]


REFERENCE_FLAGS = {         # deepcrossing.py:20-37: name -> (default, help)
    "model_dir": ("./model_dir", "Directory where model parameters, graph, etc are saved"),
    "output_dir": ("./output_dir", "Directory where pb file are saved"),
    "train_data": ("../../dataset/wechat_algo_data1/tfrecord/train.tfrecord", "Path to the train data"),
    "eval_data": ("../../dataset/wechat_algo_data1/tfrecord/test.tfrecord", "Path to the evaluation data"),
    "vocabulary_dir": ("../../dataset/wechat_algo_data1/vocabulary/", "Folder where the vocabulary file is stored"),
    "num_epochs": (1, "Epoch of training phase"),
    "train_steps": (10000, "Number of (global) training steps to perform"),
    "shuffle_buffer_size": (10000, "Dataset shuffle buffer size"),
    "num_parallel_readers": (-1, "Number of parallel readers for training data"),
    "save_checkpoints_steps": (1000, "Save checkpoints every this many steps"),
    "batch_size": (1024, "Training batch size"),
    "learning_rate": (0.005, "Learning rate"),
    "residual_internal_dim": (128, "Residual module internal dimension"),
    "residual_network_num": (1, "Numbers of residual networks"),
}


def test_reference_flags_and_call_surface():
    """(in a child process: a model script imported earlier in this one defines flags of the same names)"""
    code = ("import json, inspect; from recalgorithm_amd.algorithm.DeepCrossing import deepcrossing as m, residual_unit as r; "
            "acts = [a for a in m.FLAGS._parser._actions if a.dest != 'help']; "
            "print(json.dumps({'flags': {a.dest: [a.default, a.help] for a in acts}, "
            "'parsed': {a.dest: getattr(m.FLAGS, a.dest) for a in acts}, "
            "'callables': [n for n in ('create_feature_columns', 'example_parser', 'deepcrossing_model_fn', 'main') if callable(getattr(m, n))], "
            "'unit': str(inspect.signature(r.residual_unit)), 'same': m.residual_unit is r.residual_unit}))")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["flags"] == {k: list(v) for k, v in REFERENCE_FLAGS.items()}
    assert got["parsed"] == {k: v[0] for k, v in REFERENCE_FLAGS.items()}
    assert got["callables"] == ["create_feature_columns", "example_parser", "deepcrossing_model_fn", "main"]
    assert got["unit"] == "(input, internal_dim=None, index=None)" and got["same"]


def test_sizes_the_fused_kernels_do_not_serve_run_composed(tmp_path):
    """residual_internal_dim = 40 (not a multiple of 16): the same variables, the same arithmetic from dense layers."""
    from recalgorithm_amd.estimator import Estimator, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup("model_deepcrossing", vocab_dir, residual_internal_dim=40, residual_network_num=2)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    est.build(feats, {"read_comment": labels.float()})
    arrays = est.store.named_arrays()
    assert tuple(arrays["residual_module/dense_1_0/kernel"].shape) == (82, 40)
    assert tuple(arrays["residual_module/dense_1_1/kernel"].shape) == (40, 82) and "dense/kernel" in arrays
    assert np.prod(arrays["dense/kernel"].shape) == 82
