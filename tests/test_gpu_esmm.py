"""-m gpu: ESMM's loss tail (include/recalgo_esmm.h, csrc/esmm.hip) and the model on it.

The kernel through ops.esmm_loss and at the C ABI against tests/esmm_ref.py in float64, the float32 restatement as `ref32`
(tests/test_esmm_host.py holds that one inside assert_close on the same inputs, so a failure here is the kernel's):
  * B in 1, 63, 64, 65, 1023, 1024, 1025, 4099 (a wave, the workgroup's 1024 threads, several rows per thread), logits N(0, 3),
    click 30 %, conversion 40 %; the 196-row edge grid up to |logit| = 30, finite everywhere, where the probability-space
    composition in torch fp32 on the device is not;
  * the CTR half bit for bit ops.sigmoid_cross_entropy; forward-only; run to run, on a side stream and in three replays;
  * under tests/redzone.guarded() with buffers of exactly the documented sizes; every refusal with nothing launched.
The model on the dataset's columns against esmm_ref.esmm: PREDICT, EVAL, TRAIN, every gradient, one Adam step; three steps inside
tests/trajectory_ref.bounds; the captured step against eager steps; an export."""
import ctypes

import numpy as np
import pytest
import torch

from recalgorithm_amd import _lib, nn, ops
from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
from tests import esmm_ref as R
from tests import golden_util as GU
from tests.redzone import guarded
from tests.test_esmm_host import esmm_setup, expected_variables, funnel_labels
from tests.test_mmoe_host import encode
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

ENTRY = "recalgo_esmm_loss_fwd_bwd"


def run_op(dev, v, forward_only=False):
    """ops.esmm_loss on the device copies of v = (a, b, y, c) -> {losses, total, prob[, d_ctr_logit, d_cvr_logit]}"""
    a, b, y, c = (t.to(dev) for t in v)
    if forward_only:
        with torch.no_grad():
            total, losses, prob = ops.esmm_loss(a, b, y, c)
        return {"losses": losses, "total": total, "prob": prob}
    a, b = a.requires_grad_(True), b.requires_grad_(True)
    total, losses, prob = ops.esmm_loss(a.reshape(-1, 1), b.reshape(-1, 1), y.reshape(-1, 1), c.reshape(-1, 1))
    assert not losses.requires_grad and not prob.requires_grad and total.dim() == 0
    da, db = torch.autograd.grad(total, [a, b])
    return {"losses": losses.detach(), "total": total.detach(), "prob": prob, "d_ctr_logit": da, "d_cvr_logit": db}


def _judge(got, r64, r32, what):
    for k in R.NAMES:
        if k in got:
            assert_close(got[k], r64[k], what=f"{what} {k}", reduced=k in R.REDUCED, ref32=r32[k])


@pytest.mark.parametrize("B", R.ROW_COUNTS)
def test_parity_with_the_fp64_restatement(dev, B):
    v, r64, r32 = R.case(B)
    got = run_op(dev, v)
    _judge(got, r64, r32, f"esmm B={B}")
    y, c = v[2], v[3]
    assert float(got["total"]) == float(got["losses"][0] + got["losses"][1]), "the sum, in that order"
    p = got["prob"].cpu()
    assert torch.equal(p[:, 2], p[:, 0] * p[:, 1]), "pCTCVR is the fp32 product of the two stored values"
    if B >= 1023:
        assert int(((c == 1) & (y == 0)).sum()) > 0, "rows with a conversion and no click exist"
    # z = y * c: a conversion without a click is none — the same bits as with those conversions cleared
    same = run_op(dev, (v[0], v[1], y, c * y))
    for k in R.NAMES:
        assert_bit_exact(same[k], got[k], f"z = y * c, {k}")


def test_the_edge_grid_is_finite_and_in_parity(dev):
    v, r64, r32 = R.case("grid")
    got = run_op(dev, v)
    for k in R.NAMES:
        assert bool(torch.isfinite(got[k]).all()), k
    _judge(got, r64, r32, "esmm edge grid")
    assert float(v[0].abs().max()) == 30.0
    # the same rows through the probability-space composition in torch fp32 on the device: what the kernel is for
    rows = R.probability_space_rows(*(t.to(dev) for t in v))
    assert rows.dtype == torch.float32 and int((~torch.isfinite(rows)).sum()) >= 1


@pytest.mark.parametrize("B", [65, 4099, "grid"])
def test_the_ctr_half_is_sigmoid_cross_entropy_bit_for_bit(dev, B):
    v, r64, _ = R.case(B)
    a, b, y, c = (t.to(dev) for t in v)
    a1 = a.clone().requires_grad_(True)
    loss1, prob1 = ops.sigmoid_cross_entropy(a1, y)
    (d1,) = torch.autograd.grad(loss1, [a1])
    a2 = a.clone().requires_grad_(True)
    total, losses, prob = ops.esmm_loss(a2, b.detach(), y, c)          # cvr_logit detached: only d_ctr_logit is handed out
    (d2,) = torch.autograd.grad(total, [a2])
    assert_bit_exact(losses[0], loss1.detach(), "L_ctr")
    assert_bit_exact(prob[:, 0].contiguous(), prob1.detach().reshape(-1), "pCTR")
    # d_ctr_logit = the CTR part + dl/da / B: wherever the second addend is below a quarter ulp of the first, the sum IS the CTR
    # part, bit for bit (rows with |a| large and z = 0: the second term's pull on a saturated click logit vanishes)
    ga, _ = R.gradients_by_hand(*(t.double() for t in v))
    n = a.numel()
    ctr64 = (torch.sigmoid(v[0].double()) - v[2].double()) / n
    quiet = (ga.abs() / n) < ctr64.abs() * 2.0 ** -26
    if B == "grid":                        # (N(0, 3) logits do not reach there)
        assert int(quiet.sum()) >= 10, "rows where the CTR part stands alone exist"
    assert torch.equal(d2.cpu()[quiet].view(torch.int32), d1.cpu()[quiet].view(torch.int32)), "the gradient's CTR part"
    # and everywhere: the difference of the two gradients is the second term's, to the rounding of the fp32 sum d_ctr_logit is —
    # half an ulp of a number of up to twice the largest CTR part: 2^-24 * 2 * max, and as much again to its power of two
    assert_close(d2 - d1, ga / n, what=f"B={B} d_ctr_logit minus the CTR part", floor=float(ctr64.abs().max()) * 2.0 ** -22)


@pytest.mark.parametrize("B", [1, 1025, "grid"])
def test_forward_only_gives_the_same_bits(dev, B, monkeypatch):
    v = R.case(B)[0]
    full = run_op(dev, v)
    seen = []
    lib = _lib.load()
    real = lib.recalgo_esmm_loss_fwd_bwd

    class Spy:
        def __getattr__(self, name):
            if name != ENTRY:
                return getattr(lib, name)
            return lambda *a: (seen.append((a[9], a[10])), real(*a))[1]
    monkeypatch.setattr(ops, "_lib_", lambda: Spy())
    fwd = run_op(dev, v, forward_only=True)
    assert seen == [(None, None)], "both gradients NULL under torch.no_grad"
    for k in ("losses", "total", "prob"):
        assert_bit_exact(fwd[k], full[k], f"forward only, {k}")


def test_two_runs_and_three_replays_give_the_same_bits(dev):
    """forward + backward eagerly twice, once on a side stream (the warm-up a capture needs), captured and replayed three times"""
    v = R.case(4099)[0]
    a, b, y, c = (t.to(dev) for t in v)
    a, b = a.requires_grad_(True), b.requires_grad_(True)
    names = ["total", "losses", "prob", "d_ctr_logit", "d_cvr_logit"]

    def run():
        total, losses, prob = ops.esmm_loss(a, b, y, c)
        return [total.detach(), losses, prob] + list(torch.autograd.grad(total, [a, b]))
    first = [o.clone() for o in run()]
    for name, u, w_ in zip(names, run(), first):
        assert_bit_exact(u, w_, f"second eager run, {name}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for name, u, w_ in zip(names, on_side, first):
        assert_bit_exact(u, w_, f"side stream, {name}")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for i in range(3):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, u, w_ in zip(names, captured, first):
            assert_bit_exact(u, w_, f"replay {i}, {name}")


def test_a_seeded_loss_bakes_the_seed_into_the_gradients(dev):
    v, r64, r32 = R.case(1023)
    a, b, y, c = (t.to(dev) for t in v)
    a, b = a.requires_grad_(True), b.requires_grad_(True)
    with ops.loss_seed(0.25):
        total, _, _ = ops.esmm_loss(a, b, y, c)
    total.backward(torch.tensor(0.25, device=dev))
    assert_close(a.grad, 0.25 * r64["d_ctr_logit"], what="seeded d_ctr_logit", ref32=0.25 * r32["d_ctr_logit"])
    assert_close(b.grad, 0.25 * r64["d_cvr_logit"], what="seeded d_cvr_logit", ref32=0.25 * r32["d_cvr_logit"])


# ---- at the C ABI ---------------------------------------------------------------------------------------------------------------
def _abi_call(dev, bufs, B, stream=None):
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return lib.recalgo_esmm_loss_fwd_bwd(*(ptr(bufs[k]) for k in ("a", "b", "y", "c")), B, 1.0,
                                         *(ptr(bufs[k]) for k in ("prob", "losses", "total", "da", "db")), st)


@pytest.mark.parametrize("B", [1, 65, 1025, 4099])
@pytest.mark.parametrize("backward", [True, False], ids=["fwd+bwd", "fwd"])
def test_guarded_buffers_of_exactly_the_documented_sizes(dev, B, backward):
    """every input and output between 0xFF redzones, the outputs exactly [B, 3], [2], [1], [B], [B]: the values are right (an
    element never written is a NaN), the redzones and the inputs untouched"""
    v, r64, r32 = R.case(B)
    with guarded() as g:
        bufs = dict(zip("abyc", (g.input(t, dev) for t in v)))
        bufs.update(prob=torch.empty(B, 3, device=dev), losses=torch.empty(2, device=dev), total=torch.empty(1, device=dev),
                    da=torch.empty(B, device=dev) if backward else None, db=torch.empty(B, device=dev) if backward else None)
        assert _abi_call(dev, bufs, B) == 0
        torch.cuda.synchronize()
        assert ENTRY in g.launched
    got = {"losses": bufs["losses"], "total": bufs["total"].reshape(()), "prob": bufs["prob"]}
    if backward:
        got.update(d_ctr_logit=bufs["da"], d_cvr_logit=bufs["db"])
    _judge(got, r64, r32, f"guarded B={B}")
    plain = run_op(dev, v, forward_only=not backward)
    for k in got:
        assert_bit_exact(got[k], plain[k], f"the ABI against ops.esmm_loss, {k}")


def test_every_refusal_launches_nothing(dev):
    """hipErrorInvalidValue for each refusal of the header, on real buffers filled with a sentinel: none of them is written"""
    B = 64
    v = R.case(B)[0]
    MAX = ops.ESMM_MAX_ROWS
    bufs = dict(zip("abyc", (t.to(dev) for t in v)))
    outs = dict(prob=torch.full((B, 3), -7.0, device=dev), losses=torch.full((2,), -7.0, device=dev), total=torch.full((1,), -7.0, device=dev),
                da=torch.full((B + 1,), -7.0, device=dev), db=torch.full((B + 1,), -7.0, device=dev))
    refused = pytest.raises(_lib.RecalgoError, match=f"{ENTRY} failed with hipError_t=1$")
    bad = [dict(B=0), dict(B=-1), dict(B=MAX + 1), dict(da=None), dict(db=None)]
    bad += [{k: None} for k in ("a", "b", "y", "c", "prob", "losses", "total")]
    bad += [{k: "odd"} for k in ("a", "b", "y", "c", "prob", "losses", "total", "da", "db")]
    for over in bad:
        args = {**bufs, **outs}
        n = over.pop("B", B)
        for k, val in over.items():
            # "odd": an address inside the buffer that is not 4-byte aligned (a uint8 view, one byte in)
            args[k] = args[k].reshape(-1).view(torch.uint8)[1:] if isinstance(val, str) else val
            assert args[k] is None or args[k].data_ptr() % 4 == (1 if isinstance(val, str) else 0)
        with refused:
            _abi_call(dev, args, n)
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs.values()), "a refused call launched nothing"
    assert _abi_call(dev, {**bufs, **outs}, B) == 0
    torch.cuda.synchronize()
    assert bool((outs["prob"] != -7.0).all()) and float(outs["da"][B]) == -7.0


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _redraw(est, seed=16):
    """tables of order 0.5 and larger logit kernels, so that the towers tell the rows apart; BatchNorm's moving statistics stay"""
    arrays = est.store.named_arrays()
    gen = torch.Generator().manual_seed(seed)
    for k, v in arrays.items():
        if k.endswith("/embedding_weights"):
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.5)
        elif k.endswith("_logit/kernel"):
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.5)
        elif k.endswith("_logit/bias"):
            v.copy_(torch.randn(*v.shape, generator=gen) * 0.3)
    return arrays


def _host_batch():
    sfeats, _ = GU.string_batch()
    return {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}, funnel_labels()


def _on_device(dev, tmp_path, **flags):
    """-> (estimator, params, device features, device labels) of the model on the 48 rows of the shared string batch"""
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = esmm_setup(vocab_dir, **dict(dict(hidden_units="32,16"), **flags))
    feats, lab = _host_batch()
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, use_hip_graph=False))
    est.build(feats, lab)
    return est, params, *est._to_device(feats, lab)


def _oracle(params, variables, dtype, masks):
    sfeats, _ = GU.string_batch()
    P = {k: v.clone().to(dtype).requires_grad_(not k.split("/")[-1].startswith("moving_")) for k, v in variables.items()}
    feats = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in encode(params, sfeats).items()}
    lab = {k: v.to(dtype) for k, v in funnel_labels().items()}
    with torch.no_grad():
        predict = R.esmm(P, feats, None, params, training=False)
        evaluate = R.esmm(P, feats, lab, params, training=False)
    out = R.esmm(P, feats, lab, params, training=True, dropout_masks=[m.to(dtype) for m in masks])
    out["loss"].backward()
    return {"predict": predict, "eval_loss": evaluate["loss"], "loss": out["loss"].detach(), "P": P}


def test_the_model_follows_the_fp64_restatement(dev, tmp_path, monkeypatch):
    """The dataset's columns, hidden 32,16 with BatchNorm and dropout 0.2, the four keep masks (two hidden layers in each tower)
    injected through nn.DROPOUT_KEEP_MASKS in call order: PREDICT, EVAL's loss, the TRAIN loss, every gradient and one Adam step
    against tests/esmm_ref.esmm in float64.  Each call with labels launches the loss entry once."""
    from tests.golden_protocol import judge_step_against_oracle
    est, params, feats, lab = _on_device(dev, tmp_path, dropout_rate=0.2)
    arrays = _redraw(est)
    assert sorted(k for k in arrays if not k.endswith("/embedding_weights")) == sorted(expected_variables(params, 82))
    variables = {k: v.detach().cpu().double() for k, v in arrays.items()}
    before = {k: v.clone() for k, v in variables.items()}
    gen = torch.Generator().manual_seed(5)
    masks = [(torch.rand(48, int(u), generator=gen) >= 0.2).float() for _ in ("ctr", "cvr") for u in params["hidden_units"]]
    r64, r32 = _oracle(params, variables, torch.float64, masks), _oracle(params, variables, torch.float32, masks)
    for t in ("ctr", "cvr"):
        p = r64["predict"]["probs"][t]
        assert float(p.max() - p.min()) > 0.05, "the redrawn variables tell the rows apart"
    calls = []
    lib = _lib.load()
    real = lib.recalgo_esmm_loss_fwd_bwd
    monkeypatch.setattr(lib, ENTRY, lambda *a: (calls.append(a[9] is not None), real(*a))[1], raising=False)
    nn.DROPOUT_KEEP_MASKS[:] = list(masks)
    try:
        with torch.no_grad():
            pr = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
        assert len(nn.DROPOUT_KEEP_MASKS) == 4, "PREDICT and EVAL drop nothing"
        assert calls == [False], "EVAL under no_grad: one forward-only launch; PREDICT launches none"
        assert list(pr.predictions) == ["ctr_probabilities", "cvr_probabilities", "ctcvr_probabilities"]
        for t in ("ctr", "cvr", "ctcvr"):
            assert_close(pr.predictions[f"{t}_probabilities"], r64["predict"]["probs"][t], what=f"esmm predict {t}",
                         ref32=r32["predict"]["probs"][t])
        assert_close(ev.loss, r64["eval_loss"], what="esmm eval loss", ref32=r32["eval_loss"])
        spec = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
        assert not nn.DROPOUT_KEEP_MASKS, "TRAIN consumed the four hidden layers' masks"
    finally:
        nn.DROPOUT_KEEP_MASKS[:] = []
    assert calls == [False, True]
    assert_close(spec.loss, r64["loss"], what="esmm loss", ref32=r32["loss"])
    assert abs(float(r64["loss"]) - float(r64["eval_loss"])) > 1e-4, "the masks change the loss"
    for t in ("ctr", "cvr"):
        g = r64["P"][f"tower/tower_{t}_logit/kernel"].grad
        assert float(g.max()) > 0 > float(g.min()), "both towers see gradient of both signs"
    n_min = 7 + 2 * (2 * 4 + 2)                               # tables, two towers of two hidden layers with BatchNorm and a logit
    judge_step_against_oracle(est, spec, r64["P"], r32["P"], before, params["learning_rate"], "esmm", n_min)


def test_three_steps_follow_the_fp64_restatement(dev, tmp_path):
    """3 eager Estimator.train_step calls on rotating sub-batches of the shared batch against the float64 restatement's own
    free-running trajectory, inside tests/trajectory_ref.bounds; the float32 restatement itself must sit below half of that
    bound for the test to be one of the kernels.  (No dropout: the device draws its masks from a hash the restatement has not.)"""
    from oracle import ref_ops as O
    from tests import trajectory_ref as T
    N = 3
    est, params, _, _ = _on_device(dev, tmp_path, dropout_rate=0.0)
    arrays = _redraw(est)
    start = {k: v.detach().cpu().double() for k, v in arrays.items()}
    lr = float(params["learning_rate"])
    sfeats, _ = GU.string_batch()
    both = torch.cat([funnel_labels()[k] for k in ("click_avatar", "follow")], dim=1)
    batches = [T.cut(sfeats, both, idx) for idx in T.batch_indices()]
    split = lambda lb, dtype: {"click_avatar": lb[:, 0:1].to(dtype).contiguous(), "follow": lb[:, 1:2].to(dtype).contiguous()}   # noqa: E731

    def trajectory(dtype):
        P = {k: v.clone().to(dtype) for k, v in start.items()}
        m, v_ = {k: torch.zeros_like(v) for k, v in P.items()}, {k: torch.zeros_like(v) for k, v in P.items()}
        out = {"loss": [], "grad": [], "v": []}
        for k, b in enumerate(T.ORDER[:N], start=1):
            for n, p in P.items():
                p.grad = None
                p.requires_grad_(not n.split("/")[-1].startswith("moving_"))
            sf, lb = batches[b]
            feats = {n: (t.to(dtype) if isinstance(t, torch.Tensor) and t.is_floating_point() else t) for n, t in encode(params, sf).items()}
            bn_state = {}
            res = R.esmm(P, feats, split(lb, dtype), params, training=True, bn_state=bn_state)
            res["loss"].backward()
            grads = {n: p.grad.detach().clone() for n, p in P.items() if p.grad is not None}
            with torch.no_grad():
                for n, gr in grads.items():
                    O.adam_tf1_step(P[n], gr, m[n], v_[n], k, lr)
                for scope, (mean, var) in bn_state.items():          # the moving statistics: momentum 0.99
                    P[f"{scope}/moving_mean"].mul_(0.99).add_(0.01 * mean)
                    P[f"{scope}/moving_variance"].mul_(0.99).add_(0.01 * var)
            out["loss"].append(res["loss"].detach().clone())
            out["grad"].append(grads)
            out["v"].append({n: v_[n].clone() for n in grads})
        out["final"] = {n: p.detach().clone() for n, p in P.items()}
        out["trainable"] = sorted({n for gr in out["grad"] for n in gr})
        return out
    r64, r32 = trajectory(torch.float64), trajectory(torch.float32)
    bnd = T.bounds(r64, lr)
    w32, where32, out32 = T.worst_ratio({k: r32["final"][k] for k in r64["trainable"]}, r64, bnd)
    assert w32 <= 0.5, f"the fp32 restatement alone uses {w32:.3f} of the bound at {where32}"
    host = [({k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sf.items()}, split(lb, torch.float32)) for sf, lb in batches]
    dev_batches = [est._to_device(f, l) for f, l in host]
    losses = [est.train_step(*dev_batches[b]).clone() for b in T.ORDER[:N]]
    torch.cuda.synchronize()
    for k, (l, l64, l32) in enumerate(zip(losses, r64["loss"], r32["loss"]), start=1):
        assert_close(l, l64, what=f"esmm loss of step {k}", ref32=l32)
    assert int(est.store.opt_state["step"]) == N
    after = est.store.named_arrays()
    assert len(r64["trainable"]) == 7 + 2 * (2 * 4 + 2)
    wk, wherek, outk = T.worst_ratio({k: after[k] for k in r64["trainable"]}, r64, bnd)
    print(f"esmm: worst |p - p64| / tol after {N} steps: kernels {wk:.3f} ({wherek}) | fp32 restatement {w32:.3f} ({where32})")
    assert wk <= 1.0, f"esmm: {wherek} is {wk:.3f} x the bound after {N} steps (fp32 restatement: {w32:.3f} at {where32})"
    for k in outk:
        assert outk[k] <= 1.5 * out32[k] + 10, f"esmm {k}: {outk[k]} elements outside the tight bound, the fp32 restatement leaves {out32[k]}"


# ---- captured training ---------------------------------------------------------------------------------------------------------------
def synthetic(dev, B=256, seed=42, **run):
    """(estimator, synth spec) of the model over synthetic device-resident features: 16 dense features and 8 single-valued id
    columns"""
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm._common import dense_columns
    from recalgorithm_amd.algorithm.ESMM.esmm import esmm_model_fn
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=8, max_vocab=400, seed=11, oov_frac=0.05, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": dense_columns(), "category_feature_columns": [fc.embedding_column(c, 8) for c in cats],
              "hidden_units": ["64", "32"], "dropout_rate": 0.1, "batch_norm": True, "learning_rate": 0.005,
              "ctr_task_name": "click_avatar", "cvr_task_name": "follow"}
    est = Estimator(model_fn=esmm_model_fn, params=params, config=RunConfig(device=dev, seed=seed, **run))
    est.build(*synthetic_batch(spec, B, dev, 0))
    return est, spec


def synthetic_batch(spec, B, dev, i):
    """synth's features of batch i with funnel labels drawn here: clicks 30 %, conversions 40 % (synth's own labels are 2 %
    positives drawn independently: almost no conversions among the clicks)"""
    from recalgorithm_amd.io import synth
    feats = synth.device_features(spec, B, dev, batch_index=i)[0]
    g = torch.Generator().manual_seed(977 + i)
    labels = {"click_avatar": (torch.rand(B, 1, generator=g) < 0.3).float().to(dev), "follow": (torch.rand(B, 1, generator=g) < 0.4).float().to(dev)}
    return feats, labels


def test_captured_step_replays_what_eager_steps_compute(dev):
    """three hipGraph replays of the captured step (B 256, dropout 0.1 on the hash: the mask follows the device step counter, so
    replays and eager steps draw the same masks) against eager launches on rotating batches, bit for bit"""
    from recalgorithm_amd.estimator import GraphedTrainStep, _tree_tensors
    from tests.test_gpu_replay_models import _differences, _state
    WARMUP, STEPS, N_BATCHES = 3, 3, 3
    (eager, spec), (graphed, _) = synthetic(dev), synthetic(dev)
    batches = [synthetic_batch(spec, 256, dev, i) for i in range(N_BATCHES)]
    keep = [[t.clone() for _, t in _tree_tensors({"f": b[0], "l": b[1]}, "b")] for b in batches]
    for _ in range(WARMUP):
        eager.train_step(*batches[0])
    le = [eager.train_step(*batches[i % N_BATCHES]).clone() for i in range(STEPS)]
    first = _state(eager, le)
    assert int(first["step counter"]) == WARMUP + STEPS and all(torch.isfinite(l).all() for l in le)
    assert float(le[-1]) != float(le[0])
    g = GraphedTrainStep(graphed.train_step, *batches[0], warmup=WARMUP)
    lg = [g(*batches[i % N_BATCHES]).clone() for i in range(STEPS)]
    diff = _differences(first, _state(graphed, lg))
    assert not diff, f"{STEPS} replays of the captured step differ from eager launches in {diff[:8]} ({len(diff)} in all)"
    assert all(torch.equal(t, k) for b, kept in zip(batches, keep) for (_, t), k in zip(_tree_tensors({"f": b[0], "l": b[1]}, "b"), kept))


# ---- serving ---------------------------------------------------------------------------------------------------------------------------
def test_an_export_predicts_what_the_estimator_predicts(dev, tmp_path):
    """ServingModel.predict and the uncompiled serve() on an export against estimator.predict: the three keys, bit for bit"""
    from recalgorithm_amd import export as E
    from recalgorithm_amd import feature_column as fc
    from tests.test_gpu_serving import golden_records
    est, params, feats, lab = _on_device(dev, tmp_path)
    _redraw(est)
    est.train_step(feats, lab)
    host, _ = _host_batch()
    want = list(est.predict(lambda: iter([host])))
    keys = ["ctr_probabilities", "cvr_probabilities", "ctcvr_probabilities"]
    assert len(want) == 48 and sorted(want[0]) == sorted(keys)
    recv = E.build_parsing_serving_input_receiver_fn(fc.make_parse_example_spec(GU.all_columns(params)))
    export_dir = E.export_model(est, str(tmp_path / "export"), recv)
    model = E.ServingModel(est.model_fn, params, export_dir, device=dev)
    records = golden_records()
    for got, what in ((model.predict(records), "predict"), (model.serve(records), "serve")):
        assert sorted(got) == sorted(keys)
        for k in got:
            assert np.array_equal(np.asarray(got[k]).reshape(48, -1), np.stack([w[k] for w in want]).reshape(48, -1)), (what, k)
    for k in keys[:2]:
        p = np.stack([w[k] for w in want])
        assert float(p.max() - p.min()) > 0.01, k
    assert np.array_equal(np.stack([w[keys[2]] for w in want]), np.stack([w[keys[0]] for w in want]) * np.stack([w[keys[1]] for w in want]))
