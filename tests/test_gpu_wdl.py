"""-m gpu: Wide&Deep on the MI355X — the crossed wide op (csrc/wide.hip) against tests/wdl_ref.py: bucket ids exactly, the
logit, the deterministic per-bucket gradient and three FTRL steps against float64, all under the guarded allocations of
tests/redzone.py; the bias's path through the flat buffer; the mirrored model_fn against the two reference-generated
goldens, and a captured run against an eager one; an existing model through the changed minimize / finish_model_fn path.
Tolerance: the project's standing 1e-5 bound and strict guard (tests/util.py assert_close with ref32=)."""
import numpy as np
import pytest
import torch

from recalgorithm_amd.estimator import Estimator, GraphedTrainStep, ModeKeys, RunConfig
from recalgorithm_amd.feature_column import Ragged
from recalgorithm_amd.variables import Variable, VariableStore, named_grads
from tests import golden_util as GU
from tests import wdl_ref as W
from tests.redzone import guarded
from tests.test_wdl_host import GOLDENS, f32, mirror_setup
from tests.util import assert_adam_update, assert_bit_exact, assert_close

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
def golden_estimator(dev, name, tmp_path, seed=3):
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup(name, vocab_dir)
    d = GU.load(name)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=seed, use_hip_graph=False))
    est.build(feats, lab)
    # the batch as encoded ids on the device (what a training loop feeds): every categorical key the columns read
    enc = W.encode(params, sfeats)
    dfeats = {}
    for k, v in enc.items():
        if isinstance(v, tuple):
            dfeats[k] = Ragged(v[0].to(dev), v[1].to(dev))
        else:
            dfeats[k] = v.float().to(dev) if v.is_floating_point() else v.to(dev)
    dlab = {"read_comment": labels.float().to(dev)}
    arrays = est.store.named_arrays()
    gv = GU.section(d, "var/")
    assert sorted(gv) == sorted(arrays)
    for k, v in gv.items():
        arrays[k].copy_(torch.from_numpy(v).float().reshape(arrays[k].shape))
    return est, params, d, dfeats, dlab, sfeats, labels


def flat_slice(store, var):
    off = (var.data.data_ptr() - store.flat.data_ptr()) // 4
    assert 0 <= off and off + var.data.numel() <= store.flat.numel()
    return slice(off, off + var.data.numel())


@pytest.mark.parametrize("name", list(GOLDENS))
def test_model_golden(dev, name, tmp_path):
    from recalgorithm_amd import nn, ops, wide
    est, params, d, feats, lab, sfeats, labels = golden_estimator(dev, name, tmp_path)
    gv = GU.section(d, "var/")
    # the reference arithmetic's own fp32 rounding on this batch: the restatement in float32 on the golden's variables
    P32 = {k: torch.from_numpy(v.copy()).float().requires_grad_(True) for k, v in gv.items()}
    enc = W.encode(params, sfeats)
    f32s = {k: (v.float() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in enc.items()}
    masks = GU.dropout_masks(d)
    o32p = W.wide_and_deep(P32, f32s, None, params, training=False)
    o32 = W.wide_and_deep(P32, f32s, {"read_comment": labels.float()}, params, training=True, dropout_masks=[m.float() for m in masks])
    o32["loss"].backward()
    g32 = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in P32.items()}
    before = {k: v.detach().cpu().double().clone() for k, v in est.store.named_arrays().items()}
    pr = est._call_model_fn(feats, None, ModeKeys.PREDICT)
    assert list(pr.predictions) == ["probabilities"]
    assert_close(pr.predictions["probabilities"], torch.from_numpy(d["predict/probabilities"]), what=f"{name} predict", ref32=o32p["prob"])
    nn.DROPOUT_KEEP_MASKS[:] = masks
    with ops.loss_seed(1.0):                 # (a training step's setting: the wide logit joins the fused logit / loss launch)
        spec = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
    assert not nn.DROPOUT_KEEP_MASKS, "the mirror made fewer dropout calls than the reference"
    spec.loss.backward(torch.ones_like(spec.loss))
    grads = named_grads(est.store)           # (finishes the step's deferred sums: the fused tail's loss value among them)
    assert_close(spec.loss, torch.from_numpy(d["train/loss"]), what=f"{name} loss", ref32=o32["loss"])
    gg = GU.section(d, "grad/")
    assert sorted(gg) == sorted(k for k in grads if k in gg) and len(gg) == GOLDENS[name]
    gmax = {k: float(np.abs(v).max()) for k, v in gg.items()}
    dense_floor = 1e-6 * max(v for k, v in gmax.items() if "embedding_weights" not in k)
    for k, g in gg.items():
        sib = k.replace("/bias", "/kernel")
        floor = dense_floor + (1e-5 * gmax[sib] if k.endswith("/bias") and sib in gmax else 0.0)
        assert_close(grads[k], torch.from_numpy(g), what=f"{name} d({k})", reduced=True, floor=floor, ref32=g32.get(k))
    spec.train_op.optimizer.apply_gradients(est.store)
    after = est.store.named_arrays()
    ga, slots = GU.section(d, "var_after/"), GU.section(d, "slot/")
    lr_d = float(d["meta/deep_part_learning_rate"])
    (st,) = wide.states(est.store).values()
    for k, va in ga.items():
        ref_after = torch.from_numpy(va).reshape(before[k].shape)
        if k.startswith("wide_part/"):       # FTRL (then the Adam launch: the identity here)
            assert_close(after[k], ref_after, what=f"{name} ftrl {k}", reduced=True)
            assert_close(st.slots[k + "/Ftrl"], torch.from_numpy(slots[k + "/Ftrl"]), what=f"{name} {k}/Ftrl", reduced=True)
            assert_close(st.slots[k + "/Ftrl_1"], torch.from_numpy(slots[k + "/Ftrl_1"]), what=f"{name} {k}/Ftrl_1", reduced=True)
            continue
        ref_upd, upd = ref_after - torch.from_numpy(gv[k]).reshape(before[k].shape), after[k].detach().cpu().double() - before[k]
        if "moving_" in k:
            assert_close(upd, ref_upd, what=f"{name} {k} update", reduced=True, floor=1e-7)
            continue
        gref = torch.from_numpy(gg[k]).reshape(before[k].shape).abs()
        tol_g = 1e-5 * (gref + gref.pow(2).mean().sqrt()) + 1e-6 * gref.max() + dense_floor + \
            (1e-5 * gmax.get(k.replace("/bias", "/kernel"), 0.0) if k.endswith("/bias") else 0.0)
        assert_adam_update(upd, ref_upd, before[k], gref, tol_g, lr_d, what=f"{name} adam update {k}")
    # buckets the batch did not touch: exactly zero, as in the golden
    zero = torch.from_numpy(ga[W.WIDE_KERNEL] == 0).reshape(-1)
    assert int(zero.sum()) >= 1 and bool((after[W.WIDE_KERNEL].reshape(-1).cpu()[zero] == 0).all())
    # the wide variables' Adam slots and gradient slots: exactly zero
    for v in (st.kernel, st.bias):
        sl = flat_slice(est.store, v)
        assert float(est.store.flat_m[sl].abs().sum()) == 0.0 and float(est.store.flat_v[sl].abs().sum()) == 0.0
    assert float(est.store.flat_grad.abs().sum()) == 0.0
    # EVAL on the golden's state after the step
    for k, v in ga.items():
        after[k].copy_(torch.from_numpy(v).float().reshape(after[k].shape))
    with torch.no_grad():
        ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
    assert_close(ev.loss, torch.from_numpy(d["eval/loss"]), what=f"{name} eval loss")


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
    a, _, _, feats, lab, _, _ = golden_estimator(dev, name, tmp_path / "a")
    b, _, _, _, _, _, _ = golden_estimator(dev, name, tmp_path / "b")
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
    from oracle import ref_ops as R
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
    gv = GU.golden_to_oracle_vars(name, GU.section(d, "var/"), params)
    ga = GU.golden_to_oracle_vars(name, GU.section(d, "var_after/"), params)
    gg = GU.golden_to_oracle_vars(name, GU.section(d, "grad/"), params)
    arrays = est.store.named_arrays()
    for k, v in gv.items():
        arrays[k].copy_(torch.from_numpy(v).float().reshape(arrays[k].shape))
    before = {k: v.detach().cpu().double().clone() for k, v in est.store.named_arrays().items()}
    loss = est.train_step(feats, lab)        # model_fn -> finish_model_fn -> AdamOptimizer.minimize(loss) -> apply_gradients
    assert_close(loss, torch.from_numpy(d["train/loss"]), what="deepfm loss")
    after = est.store.named_arrays()
    lr = float(d["meta/learning_rate"])
    gmax = max(float(np.abs(v).max()) for k, v in gg.items() if "embedding_weights" not in k)
    n = 0
    for k, va in ga.items():
        if "moving_" in k or k not in gg:
            continue
        ref_upd = torch.from_numpy(va).reshape(before[k].shape) - torch.from_numpy(gv[k]).reshape(before[k].shape)
        upd = after[k].detach().cpu().double() - before[k]
        gref = torch.from_numpy(gg[k]).reshape(before[k].shape).abs()
        sib = k.replace("/bias", "/kernel")
        tol_g = 1e-5 * (gref + gref.pow(2).mean().sqrt()) + 1e-6 * gref.max() + 1e-6 * gmax + \
            (1e-5 * float(np.abs(gg[sib]).max()) if k.endswith("/bias") and sib in gg else 0.0)
        assert_adam_update(upd, ref_upd, before[k], gref, tol_g, lr, what=f"deepfm adam update {k}")
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
