"""CPU (no kernels launched): the Wide&Deep feature's host side.
  * the crossed column's hash: the known answers, two implementations (numpy uint64, Python integers) against each other;
  * tests/wdl_ref.py (the float64 restatement the GPU tests compare against) reproduces both goldens that
    scripts/gen_golden_wdl.py obtained by executing the reference's own algorithm/WideAndDeep/wide_and_deep.py on
    oracle/tf1_shim: predictions, loss, every gradient, the variables and the FTRL slots after one step;
  * the generator's --check round trip (where the reference folder exists);
  * the two properties of FTRL the sparse update rests on;
  * the mirror's variables, flags, columns and parse spec on the launch-free registration pass;
  * include/recalgo_wide.h, the third ABI header: its names, signatures, launches, sizes and constants, literally, and the
    constants re-exported (the checks every header gets, include/recalgo_wide.abi among them: tests/test_abi.py);
  * the FTRL slots under TF's names through the checkpoint writer."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import golden_util as GU
from tests import wdl_ref as W
from tests.golden_protocol import GoldenCase, close, restate_on_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_wide.h")
GOLDENS = {"model_wdl": 19, "model_wdl_dropout": 19}          # name -> gradient arrays


def f32(x):
    return float(np.float32(x))


def mirror_setup(name, vocab_dir):
    """(model_fn, params) of the mirror for golden `name`, from the mirror's own create_feature_columns() with the golden's
    hash_bucket_size."""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.WideAndDeep import wide_and_deep as m
    d = GU.load(name)
    fl = {k: (v.item() if v.shape == () else v) for k, v in GU.section(d, "flag/").items()}
    flags.FLAGS.vocabulary_dir = vocab_dir
    for k, v in fl.items():
        setattr(flags.FLAGS, k, v)
    saved, m.HASH_BUCKET_SIZE = m.HASH_BUCKET_SIZE, int(d["meta/hash_bucket_size"])
    try:
        wide, deep = m.create_feature_columns()
    finally:
        m.HASH_BUCKET_SIZE = saved
    return m.wide_and_deep_model_fn, {
        "wide_part_feature_columns": wide, "deep_part_feature_columns": deep, "hidden_units": str(fl["hidden_units"]).split(","),
        "dropout_rate": float(fl["dropout_rate"]), "batch_norm": bool(fl["batch_norm"]),
        "deep_part_optimizer": str(fl["deep_part_optimizer"]), "wide_part_learning_rate": float(fl["wide_part_learning_rate"]),
        "deep_part_learning_rate": float(fl["deep_part_learning_rate"])}


# ---- 1. the hash ---------------------------------------------------------------------------------------------------------------
def test_hash_known_answers():
    mods = {(0, 0): (71304, 1), (1, 2): (1357, 0), (12345, 67): (20464, 2), (-1, 3): (49339, 0), (7, -1): (33121, 0),
            (2147483647, 349): (46439, 6)}
    assert set(mods) == set(W.KNOWN_ANSWERS)
    for (u, t), full in W.KNOWN_ANSWERS.items():
        h = int(W.cross_hash_np([u], [t])[0])
        assert h == full, (u, t, h)
        assert (h % 100000, h % 7) == mods[(u, t)]
        assert W.cross_hash_py(u, t) == full
    _, bk = W.buckets([12345, -1], [67, 3, 3], [0, 1, 3], 100000)
    assert bk.tolist() == [20464, 49339, 49339]
    _, bk7 = W.buckets([12345, -1], [67, 3, 3], [0, 1, 3], 7)
    assert bk7.tolist() == [2, 0, 0]


def test_hash_two_implementations_agree():
    rng = np.random.default_rng(20260)
    u = rng.integers(-1, 2 ** 31, size=10000, dtype=np.int64)
    t = rng.integers(-1, 2 ** 31, size=10000, dtype=np.int64)
    u[:4], t[:4] = [-1, 2 ** 31 - 1, -1, 2 ** 31 - 1], [-1, -1, 2 ** 31 - 1, 2 ** 31 - 1]
    got = W.cross_hash_np(u, t)
    assert got.dtype == np.uint64
    want = np.array([W.cross_hash_py(int(a), int(b)) for a, b in zip(u, t)], dtype=np.uint64)
    assert np.array_equal(got, want)
    assert len(set(got.tolist())) > 9990          # (a hash: the 10 000 pairs do not collapse)


# ---- 2. the restatement against the goldens ------------------------------------------------------------------------------------
WIDE = [W.WIDE_KERNEL, W.WIDE_BIAS]
# the golden-parity case; tests/test_gpu_wdl.py adds what its device run needs
CASE = GoldenCase(mirror_setup=mirror_setup, oracle=W.wide_and_deep, encode=W.encode, predictions={"probabilities": ("prob",)},
                  ordered_prediction_keys=True, predict_what="{name} predict", n_grads=GOLDENS, n_masks=2,
                  lr_key="meta/deep_part_learning_rate")


def _ftrl_step(golden, k, p, g):
    """the wide variables: one dense FTRL step (accum 0.1 as float32, linear 0) on the golden's gradient"""
    if k not in WIDE:
        return False
    d, name, slots = golden.d, golden.name, GU.section(golden.d, "slot/")
    v, a, l = W.ftrl_dense(p, torch.full_like(p, f32(W.FTRL_INITIAL_ACCUMULATOR)), torch.zeros_like(p), g,
                           f32(d["meta/wide_part_learning_rate"]))
    close(v, golden.var_after[k], f"{name} ftrl({k})")
    close(a, slots[f"{k}/Ftrl"], f"{name} accum({k})")
    close(l, slots[f"{k}/Ftrl_1"], f"{name} linear({k})")
    return True


@pytest.mark.parametrize("name", list(GOLDENS))
def test_restatement_reproduces_the_golden(name, tmp_path):
    d = GU.load(name)
    H = int(d["meta/hash_bucket_size"])
    _, params = mirror_setup(name, GU.write_vocab_dir(str(tmp_path / "vocabulary")))
    assert H == 64 and params["wide_part_feature_columns"][0].categorical_column.hash_bucket_size == H
    slots = GU.section(d, "slot/")
    assert sorted(slots) == sorted(f"{k}/{s}" for k in WIDE for s in ("Ftrl", "Ftrl_1"))
    golden, run = restate_on_host(CASE, name, tmp_path, other_step=_ftrl_step)
    gg, ga, feats, lr_w = golden.grad, golden.var_after, run["feats"], f32(d["meta/wide_part_learning_rate"])
    # the wide kernel: buckets nothing touched are EXACTLY zero after the step; the golden holds some, and collisions
    ex, bk = W.buckets(feats["userid"], *feats["manual_tag_list"], H)
    touched = np.zeros(H, dtype=bool)
    touched[bk] = True
    after = ga[W.WIDE_KERNEL].reshape(-1)
    assert (~touched).sum() >= 1 and np.all(after[~touched] == 0.0)
    assert np.all(d["var/" + W.WIDE_KERNEL].reshape(-1)[~touched] != 0.0), "an untouched bucket that started at zero shows nothing"
    assert np.all(gg[W.WIDE_KERNEL].reshape(-1)[~touched] == 0.0)
    per_bucket_examples = [len(set(ex[bk == j].tolist())) for j in range(H)]
    assert max(per_bucket_examples) >= 2, "no bucket is hit by two examples"
    # and the sparse update (touched buckets + the step-1 zeroing) gives the golden's kernel and slots
    kern = torch.from_numpy(d["var/" + W.WIDE_KERNEL].copy()).reshape(-1)
    tj = torch.from_numpy(np.nonzero(touched)[0])
    v, a, l = W.ftrl_sparse(kern, torch.full_like(kern, f32(0.1)), torch.zeros_like(kern), tj,
                            torch.from_numpy(gg[W.WIDE_KERNEL].copy()).reshape(-1)[tj], lr_w, first_step=True)
    close(v, after, f"{name} sparse ftrl kernel")
    assert torch.all(v[torch.from_numpy(~touched)] == 0.0)
    close(a, slots[W.WIDE_KERNEL + "/Ftrl"], f"{name} sparse ftrl accum")
    close(l, slots[W.WIDE_KERNEL + "/Ftrl_1"], f"{name} sparse ftrl linear")


# ---- 3. the generator ------------------------------------------------------------------------------------------------------------
def test_generator_check_round_trip():
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, "WideAndDeep")):
        pytest.skip("the reference folder is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_golden_wdl.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "model_wdl.npz  checked" in r.stdout and "model_wdl_dropout.npz  checked" in r.stdout


# ---- 4. FTRL properties ------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_ftrl_zero_gradient_is_the_bitwise_identity_from_step_two(dtype):
    gen = torch.Generator().manual_seed(5)
    n, lr = 257, f32(0.005)
    var = (torch.rand(n, generator=gen, dtype=torch.float64) - 0.5).to(dtype)
    accum, linear = torch.full((n,), f32(0.1), dtype=dtype), torch.zeros(n, dtype=dtype)
    zero = torch.zeros(n, dtype=dtype)
    # step 1 with g = 0: linear stays 0, so var becomes 0 (the glorot values do not survive the first step)
    v1, a1, l1 = W.ftrl_dense(var, accum, linear, zero, lr)
    assert torch.all(v1 == 0) and torch.equal(_bits(a1), _bits(accum)) and torch.all(l1 == 0)
    # a state some real steps have produced, then g = 0 again and again: nothing changes, bit for bit
    for _ in range(2):
        g = (torch.randn(n, generator=gen, dtype=torch.float64) * 1e-2).to(dtype)
        var, accum, linear = W.ftrl_dense(var, accum, linear, g, lr)
    assert bool((var != 0).all())
    v, a, l = var, accum, linear
    for step in range(3):
        v, a, l = W.ftrl_dense(v, a, l, zero, lr)
        if step == 0:
            # the first g = 0 update recomputes var from (linear, accum): the same expression the last real step evaluated
            assert torch.equal(_bits(v), _bits(var))
        assert torch.equal(_bits(v), _bits(var)) and torch.equal(_bits(a), _bits(accum)) and torch.equal(_bits(l), _bits(linear))


def test_three_dense_steps_equal_three_sparse_steps_plus_the_first_zeroing():
    gen = torch.Generator().manual_seed(6)
    n, lr = 64, f32(0.005)
    var0 = torch.rand(n, generator=gen, dtype=torch.float64) - 0.5
    dense = (var0.clone(), torch.full((n,), f32(0.1), dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
    sparse = tuple(t.clone() for t in dense)
    ever = torch.zeros(n, dtype=torch.bool)
    for step in range(3):
        touched = torch.randperm(n, generator=gen)[:20].sort().values
        ever[touched] = True
        g = torch.zeros(n, dtype=torch.float64)
        g[touched] = torch.randn(20, generator=gen, dtype=torch.float64) * 1e-2
        g[touched[0]] = 0.0                  # a touched bucket whose gradient sums to exactly 0
        dense = W.ftrl_dense(*dense, g, lr)
        sparse = W.ftrl_sparse(*sparse, touched, g[touched], lr, first_step=(step == 0))
        for a, b, what in zip(dense, sparse, ("var", "accum", "linear")):
            assert torch.equal(_bits(a), _bits(b)), f"step {step + 1}: {what}"
    assert (~ever).sum() > 0 and torch.all(dense[0][~ever] == 0.0)


# ---- 5. the registration pass ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GOLDENS))
def test_mirror_variables_and_columns_on_the_registration_pass(name, tmp_path):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup(name, vocab_dir)
    wide, deep = params["wide_part_feature_columns"], params["deep_part_feature_columns"]
    assert len(wide) == 1 and fc.is_crossed_indicator(wide[0]) and len(deep) == 16 + 8
    crossed = wide[0].categorical_column
    assert [k.key for k in crossed.keys] == ["userid", "manual_tag_list"] and crossed.hash_key == 0xDECAFCAFFE
    assert crossed.name == "manual_tag_list_X_userid" and wide[0].name == "manual_tag_list_X_userid_indicator"
    spec = fc.make_parse_example_spec(wide + deep)
    assert len(spec) == 16 + 8 and list(spec).count("userid") == 1 and list(spec).count("manual_tag_list") == 1
    assert fc.make_parse_example_spec(wide) == {**crossed.keys[0].parse_spec(), **crossed.keys[1].parse_spec()}
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
    est.store.building = True
    try:
        with torch.no_grad():
            pred = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
            tr = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
    finally:
        est.store.building = False
    assert list(pred.predictions) == ["probabilities"] and tuple(pred.predictions["probabilities"].shape) == (48, 1)
    assert pred.export_outputs == {"prediction": pred.predictions}
    assert sorted(ev.eval_metric_ops) == ["eval_accuracy", "eval_auc"] and ev.loss.dim() == 0
    # the train op: FTRL over wide_part, Adam over deep_part, together every trainable variable
    from recalgorithm_amd import estimator as E
    ops = tr.train_op.optimizer.ops
    assert [type(op.optimizer) for op in ops] == [E.FtrlOptimizer, E.AdamOptimizer]
    assert [v.name for v in ops[0].var_list] == [W.WIDE_KERNEL, W.WIDE_BIAS]
    assert sorted(v.name for v in ops[1].var_list) == sorted(k for k in GU.section(d, "grad/") if k.startswith("deep_part/"))
    assert (ops[0].optimizer.lr, ops[1].optimizer.lr) == (0.005, 0.001) and ops[0].optimizer.init == 0.1
    # an indicator over a crossed column never becomes a multi-hot
    with E.use_store(est.store):
        est.store.begin_call()
        with pytest.raises(NotImplementedError, match="never materialised"):
            fc.input_layer(feats, wide + deep[:1])


def test_reference_flag_defaults_and_call_surface():
    """wide_and_deep.py:12-39 (checked in a child process: a model script imported earlier in this one defines flags of the
    same names)"""
    code = ("from recalgorithm_amd.algorithm.WideAndDeep import wide_and_deep as m; F = m.FLAGS; "
            "print(F.batch_size, F.wide_part_learning_rate, F.deep_part_learning_rate, F.deep_part_optimizer, F.hidden_units, "
            "F.batch_norm, F.dropout_rate, F.train_steps, F.num_epochs, m.HASH_BUCKET_SIZE, hasattr(F, 'learning_rate')); "
            "print(all(callable(getattr(m, n)) for n in ('create_feature_columns', 'example_parser', 'wide_and_deep_model_fn', "
            "'main')), callable(m.example_parser.columns_getter))")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1024 0.005 0.001 Adam 512,256,128 True 0 10000 1 100000 False"
    assert lines[-1] == "True True"


def test_deep_part_optimizers_other_than_adam_say_so():
    from recalgorithm_amd.algorithm.WideAndDeep.wide_and_deep import _deep_part_optimizer
    for name in ("Adagrad", "SGD"):
        with pytest.raises(NotImplementedError, match=f"--deep_part_optimizer={name}"):
            _deep_part_optimizer({"deep_part_optimizer": name, "deep_part_learning_rate": 0.001})
    for name in ("RMSProp", "ftrl"):         # a NameError in the reference itself
        with pytest.raises(ValueError, match="NameError"):
            _deep_part_optimizer({"deep_part_optimizer": name, "deep_part_learning_rate": 0.001})


def test_data_parallel_is_refused_clearly(tmp_path):
    from recalgorithm_amd import parallel
    from recalgorithm_amd.estimator import Estimator, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup("model_wdl", vocab_dir)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    est.build(feats, {"read_comment": labels.float()})

    class OneRank:
        get_world_size = staticmethod(lambda group=None: 1)
        get_rank = staticmethod(lambda group=None: 0)
    with pytest.raises(NotImplementedError, match="crossed wide column"):
        parallel.attach_data_parallel(est, dist=OneRank)
    other = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    other.store.shard_at_build = object()    # (what attaching before the build leaves behind)
    with pytest.raises(NotImplementedError, match="crossed wide column"):
        other.build(feats, {"read_comment": labels.float()})


# ---- 6. include/recalgo_wide.h: what this feature expects of its header, literally (every generic check: tests/test_abi.py) ----
def test_third_header_literal_expectations():
    from recalgorithm_amd import _lib, build, ops, wide
    build.build(verbose=False)
    abi = _lib.HEADERS["recalgo_wide.h"]
    assert sorted(abi.functions) == sorted(["recalgo_wide_abi_version", "recalgo_wide_workspace_bytes",
                                            "recalgo_wide_state_workspace_bytes", "recalgo_wide_cross_fwd", "recalgo_wide_cross_plan",
                                            "recalgo_wide_cross_apply", "recalgo_wide_cross_reset"])
    assert abi.launches == ["recalgo_wide_cross_fwd", "recalgo_wide_cross_plan", "recalgo_wide_cross_apply", "recalgo_wide_cross_reset"]
    assert not abi.structs
    lib = _lib.load()
    assert lib.recalgo_wide_abi_version() == abi.version == 1
    c_int, i64, u64, ptr, flt = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_float
    F = abi.functions
    assert F["recalgo_wide_abi_version"] == (c_int, [])
    assert F["recalgo_wide_workspace_bytes"] == (i64, [c_int]) and F["recalgo_wide_state_workspace_bytes"] == (i64, [i64])
    assert F["recalgo_wide_cross_fwd"] == (c_int, [ptr, i64, ptr, ptr, i64, c_int, c_int, i64, u64, ptr, ptr, ptr, ptr, ptr, ptr])
    assert F["recalgo_wide_cross_plan"] == (c_int, [ptr, ptr, c_int, i64, ptr, ptr])
    assert F["recalgo_wide_cross_apply"] == (c_int, [ptr, ptr, c_int, i64, c_int] + [ptr] * 8 + [flt] * 3 + [c_int, ptr])
    assert F["recalgo_wide_cross_reset"] == (c_int, [ptr, ptr, c_int, ptr])
    # the sizes the header states
    assert lib.recalgo_wide_workspace_bytes(1000) == 16 + 5 * 4 * 1000 and lib.recalgo_wide_workspace_bytes(3) == 80
    assert lib.recalgo_wide_state_workspace_bytes(100000) == 800000
    assert lib.recalgo_wide_state_workspace_bytes(0) == 0 and lib.recalgo_wide_state_workspace_bytes(1 << 31) == 0
    # a launch that returns an error raises through the errcheck (NULL buffers: refused before any launch)
    with pytest.raises(_lib.RecalgoError, match="recalgo_wide_cross_fwd failed with hipError_t=[1-9]"):
        lib.recalgo_wide_cross_fwd(None, 1, None, None, 1, 1, 1, 7, 0, None, None, None, None, None, None)
    with pytest.raises(_lib.RecalgoError, match="recalgo_wide_cross_plan failed with hipError_t=[1-9]"):
        lib.recalgo_wide_cross_plan(None, None, 1, 7, None, None)
    with pytest.raises(_lib.RecalgoError, match="recalgo_wide_cross_apply failed with hipError_t=[1-9]"):
        lib.recalgo_wide_cross_apply(None, None, 1, 7, 0, *([None] * 8), 0.005, 0.0, 0.0, 0, None)
    with pytest.raises(_lib.RecalgoError, match="recalgo_wide_cross_reset failed with hipError_t=[1-9]"):
        lib.recalgo_wide_cross_reset(None, None, 1, None)
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RECALGO_WIDE_\w+) (0x[0-9A-Fa-f]+|\d+)", open(HEADER).read())
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_WIDE_ABI_VERSION": 1, "RECALGO_WIDE_HASH_KEY": 0xDECAFCAFFE,
                                        "RECALGO_WIDE_MAX_BUCKETS": 2 ** 31 - 1, "RECALGO_WIDE_APPLY_FTRL": 0, "RECALGO_WIDE_APPLY_GRAD": 1}
    assert ops.WIDE_HASH_KEY == wide.HASH_KEY == W.HASH_KEY == defines["RECALGO_WIDE_HASH_KEY"]
    assert ops.WIDE_MAX_BUCKETS == wide.MAX_BUCKETS == defines["RECALGO_WIDE_MAX_BUCKETS"]


# ---- 7. the slots through the checkpoints ------------------------------------------------------------------------------------------
def test_ftrl_slot_names_round_trip_through_the_checkpoint_writers(tmp_path):
    from recalgorithm_amd import wide
    from recalgorithm_amd.estimator import Estimator, RunConfig, collect_checkpoint_state, restore_checkpoint_state
    from recalgorithm_amd.io import tf_checkpoint
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup("model_wdl", vocab_dir)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    names = [f"{v}/{s}" for v in (W.WIDE_KERNEL, W.WIDE_BIAS) for s in ("Ftrl", "Ftrl_1")]

    def built():
        est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
        est.build(feats, lab)
        (st,) = wide.states(est.store).values()
        return est, st
    a, st = built()
    st.ensure_slots(0.1)
    assert sorted(st.slots) == sorted(names)
    gen = torch.Generator().manual_seed(9)
    for n in names:
        st.slots[n].copy_(torch.rand(st.slots[n].shape, generator=gen))
    st.ftrl_steps = 5
    a.global_step = 5
    # the TF checkpoint (the hand-back to the reference's tooling): TF's slot names, the variables' shapes
    prefix = a.save_tf_checkpoint(str(tmp_path / "model.ckpt-5"))
    listed = tf_checkpoint.list_variables(prefix)
    assert not [n for n in names if n not in listed]
    values = tf_checkpoint.read_checkpoint(prefix)
    assert values[W.WIDE_KERNEL + "/Ftrl"].shape == (64, 1) and values[W.WIDE_BIAS + "/Ftrl_1"].shape == (1,)
    b, sb = built()
    assert b.load_tf_checkpoint(prefix) == 5
    for n in names:
        assert torch.equal(sb.slots[n], st.slots[n]), n
    assert sb.ftrl_steps >= 1                # (restored slots: the first-step zeroing is behind the model)
    for k, v in a.store.named_arrays().items():
        assert torch.equal(b.store.named_arrays()[k], v), k
    # the native checkpoint state
    state, writer = collect_checkpoint_state(a.store, a.global_step)
    assert writer and sorted(state["ftrl_slots"]) == sorted(names)
    c, sc = built()
    assert restore_checkpoint_state(c.store, state, torch.device("cpu")) == 5
    for n in names:
        assert torch.equal(sc.slots[n], st.slots[n]), n
    assert sc.ftrl_steps == 5
