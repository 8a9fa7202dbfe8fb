"""-m gpu: Wide&Deep on the MI355X — the crossed wide op (csrc/wide.hip) against tests/wdl_ref.py: bucket ids exactly, the
logit, the deterministic per-bucket gradient and three FTRL steps against float64, all under the guarded allocations of
tests/redzone.py; the bias's path through the flat buffer; the mirrored model_fn against the two reference-generated
goldens, and a captured run against an eager one; an existing model through the changed minimize / finish_model_fn path.
Tolerance: the project's standing 1e-5 bound and strict guard (tests/util.py assert_close with ref32=)."""
import dataclasses

import numpy as np
import pytest
import torch

from recalgorithm_amd.estimator import Estimator, GraphedTrainStep, RunConfig
from recalgorithm_amd.feature_column import Ragged
from recalgorithm_amd.variables import Variable, VariableStore
from tests import golden_util as GU
from tests import wdl_ref as W
from tests.golden_protocol import build_on_device, check_on_device, gradient_floors, judge_adam_update, load_golden, load_variables
from tests.redzone import guarded
from tests.test_gpu_golden import suite_case
from tests.test_wdl_host import CASE, GOLDENS, f32
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu
LR = f32(0.005)
ACC0 = f32(0.1)
SHAPES = [(B, H) for B in (1, 3, 257) for H in (1, 7, 100000)]


def make_bags(B, seed):
    """-> (user ids [B], tag values, offsets [B + 1]) int64 host tensors: bags of 0..4 tags, empty bags, a repeated tag in one
    bag, ids of -1 on both sides; few users and tags, so that (user, tag) pairs repeat across examples"""
    rng = np.random.default_rng(seed)
    users = rng.integers(-1, 12, size=B)
    lens = rng.integers(0, 5, size=B)
    if B == 1:
        lens[0] = 3
    if B >= 3:
        lens[0], lens[1], lens[2] = 0, 4, 2
        users[1], users[2] = -1, 5
    offs = np.zeros(B + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    tags = rng.integers(-1, 9, size=int(offs[-1]))
    if B == 1:
        tags[:3] = [4, -1, 4]                 # a repeated tag, an OOV tag
    if B >= 3:
        tags[offs[1]:offs[2]] = [3, -1, 3, 7]
    return torch.from_numpy(users.astype(np.int64)), torch.from_numpy(tags.astype(np.int64)), torch.from_numpy(offs)


def one_pair(B):
    """every example on ONE (userid, tag): one bucket receives B requests"""
    return torch.full((B,), 7, dtype=torch.int64), torch.full((B,), 3, dtype=torch.int64), torch.arange(B + 1, dtype=torch.int64)


def make_state(dev, H, seed):
    from recalgorithm_amd import wide
    gen = torch.Generator().manual_seed(seed)
    store = VariableStore(dev)
    kernel = Variable("wide_part/wide_part_variables/kernel", ((torch.rand(H, 1, generator=gen) - 0.5)).to(dev))
    bias = Variable("wide_part/wide_part_variables/bias", (torch.rand(1, generator=gen) - 0.5).to(dev))
    return store, wide.WideState(kernel, bias, H, wide.HASH_KEY)


_REFS = {}          # computed once, shared, left unchanged


def forward_ref(B, H, seed, bags=None):
    key = ("fwd", B, H, seed, bags is not None)
    if key not in _REFS:
        u, t, o = bags or make_bags(B, seed)
        _, st = make_state("cpu", H, seed + 1)
        ex, bk = W.buckets(u, t, o, H)
        r64 = W.wide_logit(st.kernel.data.double(), st.bias.data.double(), u, t, o, H)
        r32 = W.wide_logit(st.kernel.data, st.bias.data, u, t, o, H)
        _REFS[key] = (ex, bk, r64, r32)
    return _REFS[key]


def check_forward(dev, B, H, seed, training, bags=None):
    from recalgorithm_amd import wide
    u, t, o = bags or make_bags(B, seed)
    ex, bk, r64, r32 = forward_ref(B, H, seed, bags)
    store, st = make_state(dev, H, seed + 1)
    out = wide.cross_logit(store, st, u.to(dev), t.to(dev), o.to(dev), training=training)
    got_ex, got_bk = st.last_requests(training)
    assert got_bk.dtype == torch.int32 and got_bk.cpu().tolist() == bk.tolist(), f"B={B} H={H}: bucket ids"
    assert got_ex.cpu().tolist() == ex.tolist()
    assert tuple(out.shape) == (B, 1)
    assert_close(out, r64, what=f"wide_logit B={B} H={H}", ref32=r32)
    return store, st, out


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", SHAPES)
def test_forward_buckets_exactly_and_logit_against_float64(dev, B, H):
    with guarded() as g:
        check_forward(dev, B, H, 31, training=False)
        _, st, _ = check_forward(dev, B, H, 31, training=True)
        # the counts of the TRAIN forward: one per request, per bucket
        _, bk, _, _ = forward_ref(B, H, 31)
        counts = st.table[:H].cpu()
        assert counts.tolist() == np.bincount(bk, minlength=H).tolist()
        st._reset_counts()
        assert int(st.table[:H].abs().sum()) == 0
        assert {"recalgo_wide_cross_fwd", "recalgo_wide_cross_reset", "recalgo_wide_workspace_bytes"} <= g.launched
        assert g.records_at("wide.py"), "the op's buffers were not allocated under the guard"


def test_forward_of_one_tag_per_example_and_of_all_empty_bags(dev):
    from recalgorithm_amd import wide
    with guarded():
        B, H = 70, 7
        u, t, o = one_pair(B)
        store, st = make_state(dev, H, 3)
        dense = wide.cross_logit(store, st, u.to(dev), t.to(dev), None, training=False)             # tags as a [B] column
        ragged = wide.cross_logit(store, st, u.to(dev), t.to(dev), o.to(dev), training=False)
        assert_bit_exact(dense, ragged, "dense tag column vs bags of one")
        j = W.cross_hash_py(7, 3) % H
        assert_bit_exact(dense, (st.bias.data + st.kernel.data[j]).expand(B, 1).contiguous(), "bias + kernel[bucket]")
        empty = wide.cross_logit(store, st, u.to(dev), torch.zeros(0, dtype=torch.int64, device=dev),
                                 torch.zeros(B + 1, dtype=torch.int64, device=dev), training=False)
        assert_bit_exact(empty, st.bias.data.expand(B, 1).contiguous(), "no request: the bias alone")


# ---- 2. backward + FTRL ---------------------------------------------------------------------------------------------------------
def ftrl_reference(B, H, seed, dtype, pair=False):
    """three steps over three batches in `dtype` -> per step (touched mask, bucket gradient, kernel, accum, linear, bias, bias
    accum, bias linear), and the inputs (bags, dlogit) of every step"""
    key = ("ftrl", B, H, seed, dtype, pair)
    if key in _REFS:
        return _REFS[key]
    _, st = make_state("cpu", H, seed + 1)
    k, b = st.kernel.data.reshape(-1).to(dtype), st.bias.data.to(dtype)
    ka, kl = torch.full_like(k, ACC0), torch.zeros_like(k)
    ba, bl = torch.full_like(b, ACC0), torch.zeros_like(b)
    gen = torch.Generator().manual_seed(seed + 2)
    steps, inputs = [], []
    for s in range(3):
        bags = one_pair(B) if pair else make_bags(B, seed + 10 * s)
        dlogit = (torch.randn(B, 1, generator=gen) * (0.5 / B)).float()
        ex, bk = W.buckets(*bags, H)
        g = torch.zeros(H, dtype=dtype)
        for e, j in zip(ex.tolist(), bk.tolist()):          # ascending request index
            g[j] = g[j] + dlogit[e, 0].to(dtype)
        touched = torch.zeros(H, dtype=torch.bool)
        touched[torch.from_numpy(bk)] = True
        k, ka, kl = W.ftrl_sparse(k, ka, kl, torch.nonzero(touched).reshape(-1), g[touched], LR, first_step=(s == 0))
        gb = dlogit.to(dtype).sum(dim=0) if dtype == torch.float64 else dlogit.sum(dim=0)
        b, ba, bl = W.ftrl_dense(b, ba, bl, gb, LR)
        steps.append((touched, g, k, ka, kl, b, ba, bl))
        inputs.append((bags, dlogit))
    _REFS[key] = (steps, inputs)
    return _REFS[key]


def run_ftrl(dev, B, H, seed, pair=False, materialize=False, check=True):
    """the three steps on the device; -> the final (kernel, accum, linear, bias, bias accum, bias linear)"""
    from recalgorithm_amd import wide
    r64, inputs = ftrl_reference(B, H, seed, torch.float64, pair)
    r32, _ = ftrl_reference(B, H, seed, torch.float32, pair)
    store, st = make_state(dev, H, seed + 1)
    kn, bn = st.kernel.name, st.bias.name
    what = f"B={B} H={H}"
    for s, ((u, t, o), dlogit) in enumerate(inputs):
        before = {n: x.detach().clone() for n, x in (("k", st.kernel.data), *st.slots.items())}
        out = wide.cross_logit(store, st, u.to(dev), t.to(dev), o.to(dev), training=True)
        out.backward(dlogit.to(dev))
        touched, g64, k64, ka64, kl64, b64, ba64, bl64 = r64[s]
        _, g32, k32, ka32, kl32, b32, ba32, bl32 = r32[s]
        if materialize:
            st.materialize_grad()
            if check:
                assert_close(st.kernel.grad.reshape(-1), g64, what=f"{what} step {s + 1} d(kernel)", reduced=True, ref32=g32)
                assert bool((st.kernel.grad.reshape(-1).cpu()[~touched] == 0).all())
        st.apply_ftrl(LR, 0.0, 0.0, ACC0)
        assert float(st.kernel.grad.abs().sum()) == 0.0 and float(st.bias.grad.abs().sum()) == 0.0
        assert int(st.table[:H].abs().sum()) == 0, "the per-bucket counts return to zero"
        if not check:
            continue
        tj = torch.nonzero(touched).reshape(-1)
        got = {"kernel": st.kernel.data.reshape(-1), "accum": st.slots[kn + "/Ftrl"].reshape(-1),
               "linear": st.slots[kn + "/Ftrl_1"].reshape(-1)}
        for name, a64, a32 in (("kernel", k64, k32), ("accum", ka64, ka32), ("linear", kl64, kl32)):
            assert_close(got[name].cpu()[tj], a64[tj], what=f"{what} step {s + 1} {name} (touched)", reduced=True, ref32=a32[tj])
        un = ~touched
        if s == 0:
            assert bool((got["kernel"].cpu()[un] == 0).all()), f"{what}: untouched buckets are exactly 0 after step 1"
            assert bool((got["accum"].cpu()[un] == ACC0).all()) and bool((got["linear"].cpu()[un] == 0).all())
        else:
            for name, prev in (("kernel", before["k"]), ("accum", before[kn + "/Ftrl"]), ("linear", before[kn + "/Ftrl_1"])):
                assert_bit_exact(got[name].cpu()[un], prev.reshape(-1).cpu()[un], f"{what} step {s + 1}: untouched {name}")
        for name, t_, a64, a32 in (("bias", st.bias.data, b64, b32), ("bias accum", st.slots[bn + "/Ftrl"], ba64, ba32),
                                   ("bias linear", st.slots[bn + "/Ftrl_1"], bl64, bl32)):
            assert_close(t_, a64, what=f"{what} step {s + 1} {name}", reduced=True, ref32=a32)
    assert st.ftrl_steps == 3
    return [x.detach().clone() for x in (st.kernel.data, st.slots[kn + "/Ftrl"], st.slots[kn + "/Ftrl_1"], st.bias.data,
                                         st.slots[bn + "/Ftrl"], st.slots[bn + "/Ftrl_1"])]


@pytest.mark.parametrize("B,H", SHAPES)
def test_backward_and_three_ftrl_steps_against_float64(dev, B, H):
    with guarded() as g:
        a = run_ftrl(dev, B, H, 41)
        b = run_ftrl(dev, B, H, 41, check=False)
        for i, (x, y) in enumerate(zip(a, b)):
            assert_bit_exact(x, y, f"B={B} H={H}: second run, tensor {i}")
        assert {"recalgo_wide_cross_plan", "recalgo_wide_cross_apply"} <= g.launched


def test_one_bucket_receives_three_hundred_requests(dev):
    with guarded():
        a = run_ftrl(dev, 300, 100000, 43, pair=True)
        b = run_ftrl(dev, 300, 100000, 43, pair=True, check=False)
        for i, (x, y) in enumerate(zip(a, b)):
            assert_bit_exact(x, y, f"300 requests on one bucket: second run, tensor {i}")
        assert int((a[0] != 0).sum()) == 1


def test_reading_the_gradient_first_changes_nothing(dev):
    """named_grads' route: the per-bucket sums written to kernel.grad, then the same FTRL step (which clears them)"""
    with guarded():
        plain = run_ftrl(dev, 257, 7, 45, check=False)
        read = run_ftrl(dev, 257, 7, 45, materialize=True)
        for i, (x, y) in enumerate(zip(plain, read)):
            assert_bit_exact(x, y, f"gradient read first: tensor {i}")


def test_an_abandoned_step_leaves_no_counts_behind(dev):
    from recalgorithm_amd import wide
    with guarded():
        B, H = 257, 7
        want = run_ftrl(dev, B, H, 41, check=False)
        _, inputs = ftrl_reference(B, H, 41, torch.float64)
        store, st = make_state(dev, H, 42)
        for s, ((u, t, o), dlogit) in enumerate(inputs):
            if s == 1:                       # a TRAIN forward (of another batch) whose backward never runs
                uu, tt, oo = make_bags(B, 999)
                wide.cross_logit(store, st, uu.to(dev), tt.to(dev), oo.to(dev), training=True)
                wide.cross_logit(store, st, uu.to(dev), tt.to(dev), oo.to(dev), training=False)      # and a PREDICT in between
            out = wide.cross_logit(store, st, u.to(dev), t.to(dev), o.to(dev), training=True)
            out.backward(dlogit.to(dev))
            st.apply_ftrl(LR, 0.0, 0.0, ACC0)
        kn = st.kernel.name
        for i, (x, y) in enumerate(zip(want[:3], (st.kernel.data, st.slots[kn + "/Ftrl"], st.slots[kn + "/Ftrl_1"]))):
            assert_bit_exact(y, x, f"after an abandoned forward: tensor {i}")


# ---- 3 / 4. the bias, the model -----------------------------------------------------------------------------------------------
def golden_estimator(dev, name, tmp_path):
    """-> (estimator holding the golden's variables, the batch as encoded ids on the device, its labels)"""
    est, golden, feats, lab = build_on_device(dev, GPU_CASE, name, tmp_path)
    assert sorted(golden.var) == sorted(est.store.named_arrays())
    load_variables(est, golden.var)
    return est, feats, lab


def flat_slice(store, var):
    off = (var.data.data_ptr() - store.flat.data_ptr()) // 4
    assert 0 <= off and off + var.data.numel() <= store.flat.numel()
    return slice(off, off + var.data.numel())


def _wide_state_after_the_step(est, produced):
    """what the golden judges of the wide part besides the variables: the FTRL slots, and what the Adam launch that sweeps the
    flat buffer left of the wide variables' moments and of the gradient slots"""
    from recalgorithm_amd import wide
    (st,) = wide.states(est.store).values()
    after = est.store.named_arrays()
    x = produced["extra"]
    x["wide_after"] = {v.name: after[v.name].detach().cpu() for v in (st.kernel, st.bias)}
    x["slots"] = {k: v.detach().cpu() for k, v in st.slots.items()}
    x["wide_adam_moments"] = {v.name: float(est.store.flat_m[flat_slice(est.store, v)].abs().sum()) +
                              float(est.store.flat_v[flat_slice(est.store, v)].abs().sum()) for v in (st.kernel, st.bias)}
    x["flat_grad"] = float(est.store.flat_grad.abs().sum())


def _judge_ftrl(golden, produced, k):
    """the wide variables: FTRL (then the Adam launch: the identity here) against var_after/ and the slots"""
    if not k.startswith("wide_part/"):
        return False
    name, x, slots = golden.name, produced["extra"], GU.section(golden.d, "slot/")
    assert_close(x["wide_after"][k], torch.from_numpy(golden.var_after[k]), what=f"{name} ftrl {k}", reduced=True)
    assert_close(x["slots"][k + "/Ftrl"], torch.from_numpy(slots[k + "/Ftrl"]), what=f"{name} {k}/Ftrl", reduced=True)
    assert_close(x["slots"][k + "/Ftrl_1"], torch.from_numpy(slots[k + "/Ftrl_1"]), what=f"{name} {k}/Ftrl_1", reduced=True)
    return True


def _judge_wide_zeros(case, golden, produced):
    x = produced["extra"]
    # buckets the batch did not touch: exactly zero, as in the golden
    zero = torch.from_numpy(golden.var_after[W.WIDE_KERNEL] == 0).reshape(-1)
    left = x["wide_after"][W.WIDE_KERNEL].reshape(-1)[zero]
    assert int(zero.sum()) >= 1 and bool((left == 0).all()), f"{golden.name}: an untouched bucket of {W.WIDE_KERNEL} is not zero"
    # the wide variables' Adam slots and gradient slots: exactly zero
    for k, total in x["wide_adam_moments"].items():
        assert total == 0.0, f"{golden.name}: {k} has Adam moments"
    assert x["flat_grad"] == 0.0, f"{golden.name}: flat_grad is not zero after the step"


# Wide&Deep on the device: the batch as encoded ids; ops.loss_seed(1.0) around TRAIN (a training step's setting: the wide logit
# joins the fused logit / loss launch) and an explicit ones seed; EVAL under no_grad (with grad enabled the lookups would
# register with the sparse plan as a training lookup); FTRL for the wide variables
GPU_CASE = dataclasses.replace(CASE, feed_encoded=True, loss_seed=1.0, eval_no_grad=True, other_optimizer=_judge_ftrl,
                               produce_extra=_wide_state_after_the_step, judge_extra=_judge_wide_zeros)


@pytest.mark.parametrize("name", list(GOLDENS))
def test_model_golden(dev, name, tmp_path):
    check_on_device(dev, GPU_CASE, name, tmp_path)


def rotated(feats, lab, k):
    """the batch with its examples rotated by k (same shapes, same number of bag entries)"""
    B = lab["read_comment"].shape[0]
    order = [(i + k) % B for i in range(B)]
    idx = torch.tensor(order, device=lab["read_comment"].device)
    out = {}
    for key, v in feats.items():
        if isinstance(v, Ragged):
            offs = v.offsets.cpu().tolist()
            vals = v.values.cpu()
            rows = [vals[offs[i]:offs[i + 1]] for i in order]
            new_offs = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
            out[key] = Ragged(torch.cat(rows).to(v.values.device), new_offs.to(v.offsets.device))
        else:
            out[key] = v[idx].contiguous()
    return out, {"read_comment": lab["read_comment"][idx].contiguous()}


def full_state(est):
    from recalgorithm_amd import wide
    est.store.sync()
    out = dict(est.store.named_arrays())
    out["__flat_m__"], out["__flat_v__"] = est.store.flat_m, est.store.flat_v
    for n, ar in est.store.arenas.items():
        out[f"__{n}.m__"], out[f"__{n}.v__"] = ar.m, ar.v
    for st in wide.states(est.store).values():
        out.update(st.slots)
    return out


@pytest.mark.parametrize("name", list(GOLDENS))
def test_three_captured_replays_equal_three_eager_steps_and_the_bias_keeps_no_adam_state(dev, name, tmp_path):
    from recalgorithm_amd import wide
    a, feats, lab = golden_estimator(dev, name, tmp_path / "a")
    b, _, _ = golden_estimator(dev, name, tmp_path / "b")
    batches = [rotated(feats, lab, k) for k in (0, 5, 11, 17)]
    la = [a.train_step(*bt) for bt in batches]
    b.train_step(*batches[0])                # (the first FTRL step zeroes the untouched buckets once: never part of a graph)
    g = GraphedTrainStep(b.train_step, *batches[1], warmup=0)
    lb = [g(*bt).clone() for bt in batches[1:]]
    torch.cuda.synchronize()
    assert int(a.store.opt_state["step"]) == int(b.store.opt_state["step"]) == 4
    for i, (x, y) in enumerate(zip(la[1:], lb)):
        assert_bit_exact(y, x, f"captured loss {i}")
    A, B_ = full_state(a), full_state(b)
    assert set(A) == set(B_) and W.WIDE_BIAS + "/Ftrl_1" in A
    for k in A:
        assert_bit_exact(B_[k], A[k], f"captured vs eager {k}")
    # the wide variables live in the flat buffer the Adam launch sweeps: their Adam moments stayed exactly zero, they moved
    for est in (a, b):
        (st,) = wide.states(est.store).values()
        for v in (st.kernel, st.bias):
            sl = flat_slice(est.store, v)
            assert float(est.store.flat_m[sl].abs().sum()) == 0.0 and float(est.store.flat_v[sl].abs().sum()) == 0.0
        assert float(st.slots[W.WIDE_BIAS + "/Ftrl"]) > ACC0 and float(st.bias.data) != 0.0
        assert st.ftrl_steps >= 1


# ---- 5. an existing model through the changed path -----------------------------------------------------------------------------
def test_deepfm_golden_step_through_the_changed_minimize_and_tail(dev, tmp_path):
    from recalgorithm_amd import estimator as E
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    name = "model_deepfm"
    model_fn, params, _ = GU.mirror_setup(name, vocab_dir)
    d = GU.load(name)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, use_hip_graph=False))
    est.build(feats, lab)
    feats, lab = est._to_device(feats, lab)
    golden = load_golden(suite_case(name), name, params)
    gv, ga, gg = golden.var, golden.var_after, golden.grad
    arrays = est.store.named_arrays()
    for k, v in gv.items():
        arrays[k].copy_(torch.from_numpy(v).float().reshape(arrays[k].shape))
    before = {k: v.detach().cpu().double().clone() for k, v in est.store.named_arrays().items()}
    loss = est.train_step(feats, lab)        # model_fn -> finish_model_fn -> AdamOptimizer.minimize(loss) -> apply_gradients
    assert_close(loss, torch.from_numpy(d["train/loss"]), what="deepfm loss")
    after = est.store.named_arrays()
    floors, n = gradient_floors(gg), 0
    for k in ga:
        if "moving_" in k or k not in gg:
            continue
        judge_adam_update(golden, k, after[k].detach().cpu().double() - before[k], before[k], floors, what=f"deepfm adam update {k}")
        n += 1
    assert n >= 15
    # the default train op is what it was: one Adam op over every variable, no var_list
    with E.use_store(est.store):
        est.store.begin_call()
        op = E.AdamOptimizer(0.005).minimize(torch.zeros(()))
    assert isinstance(op, E.TrainOp) and op.var_list is None


# ---- the drivers: TFRecords in, an export served ---------------------------------------------------------------------------------
def test_trains_from_tfrecords_and_serves_its_export(dev, tmp_path):
    from recalgorithm_amd import export as E
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd import flags, wide
    from recalgorithm_amd.algorithm.utils import eval_input_fn
    from recalgorithm_amd.algorithm.WideAndDeep import wide_and_deep as m
    from recalgorithm_amd.io import synth, tfrecord
    spec = synth.SynthSpec(n_fields=6, max_vocab=300, seed=5, oov_frac=0.1, with_dense=True, with_history=True, with_tags=True)
    vocab_dir = str(tmp_path / "vocabulary") + "/"
    synth.write_vocabularies(spec, vocab_dir)
    path = str(tmp_path / "train.tfrecord")
    synth.write_tfrecord(spec, path, 600, chunk=256)
    flags.FLAGS.vocabulary_dir = vocab_dir
    wide_cols, deep_cols = m.create_feature_columns()
    assert wide_cols[0].categorical_column.hash_bucket_size == 100000
    m.total_feature_columns = wide_cols + deep_cols
    params = {"wide_part_feature_columns": wide_cols, "deep_part_feature_columns": deep_cols, "hidden_units": ["32", "16"],
              "dropout_rate": 0.0, "batch_norm": True, "deep_part_optimizer": "Adam", "wide_part_learning_rate": 0.005,
              "deep_part_learning_rate": 0.001}
    est = Estimator(m.wide_and_deep_model_fn, params, RunConfig(device=dev, seed=11))
    est.train(lambda: eval_input_fn(path, m.example_parser, 200), log_every=0)
    assert est.global_step == 3
    (st,) = wide.states(est.store).values()
    assert st.ftrl_steps == 3
    kernel = est.store.named_arrays()[W.WIDE_KERNEL].reshape(-1)
    assert 0 < int((kernel != 0).sum()) < 3 * 600 * 5, "only buckets a batch touched are non-zero after training"
    metrics = est.evaluate(lambda: eval_input_fn(path, m.example_parser, 200))
    assert {"eval_auc", "eval_accuracy", "loss"} <= set(metrics) and 0.0 <= metrics["eval_auc"] <= 1.0
    preds = list(est.predict(lambda: eval_input_fn(path, m.example_parser, 200)))
    assert len(preds) == 600 and set(preds[0]) == {"probabilities"}
    recv = E.build_parsing_serving_input_receiver_fn(fc.make_parse_example_spec(wide_cols + deep_cols))
    export_dir = E.BestExporter(name="best_exporter", serving_input_receiver_fn=recv, exports_to_keep=5).export(
        est, str(tmp_path / "export"), None, metrics, True)
    served = E.ServingModel(m.wide_and_deep_model_fn, params, export_dir, device=dev)
    out = served.predict(list(tfrecord.read_records(path))[:200])
    want = torch.tensor([float(p["probabilities"].reshape(-1)[0]) for p in preds[:200]])
    assert torch.equal(torch.from_numpy(out["probabilities"]).reshape(-1), want), "served probabilities differ from PREDICT"
