"""The golden-parity protocol, stated once: the proof that a mirrored model_fn on the HIP kernels reproduces the reference.

A golden (tests/golden/<name>.npz) holds what the reference's own sources computed on the shared 48-example batch: its
variables, PREDICT, the dropout keep masks it drew, the TRAIN loss, every gradient, the variables after one optimizer step
(BatchNorm's moving statistics among them) and EVAL on that state.  Three functions walk it:

  produce_on_device(dev, case, name, tmp_path)   runs the mirror on the device and returns plain dicts; asserts nothing
  judge(case, golden, produced, ref32)           pure, no device: every assertion, with the tolerance policy written here only
  restate_on_host(case, name, tmp_path)          the host-side twin: the float64 oracle reproduces the golden at 1e-10

What differs between models is a `GoldenCase`.  Its defaults are the strict form; a model that is looser declares it there.
tests/test_golden_protocol_host.py runs `judge` on the float64 oracle's output and on one mutation of it at a time."""
import contextlib
import re
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Union

import numpy as np
import torch

from oracle import ref_ops as R
from tests import golden_util as GU
from tests.util import assert_adam_update, assert_close

TOL = 1e-10         # restate_on_host: the bound of every comparison of the float64 oracle with a golden


@dataclass
class GoldenCase:
    mirror_setup: Callable                   # (name, vocab_dir) -> (model_fn, params)
    oracle: Callable                         # (P, feats, labels, params, training=, [dropout_masks=]) -> {"loss", "prob" | "probs"}
    encode: Callable                         # (params, string features) -> the oracle's feature batch
    tasks: Sequence[str] = ()                # multi-task: labels per task (in/label_<task>), predictions and metrics per task
    # PREDICT: prediction key -> path into the oracle's output; None: the keys of the golden's predict/ section ("probabilities"
    # -> "prob", any other key by its own name, no ref32 where the oracle has none) and no check of the key set
    predictions: Optional[Dict[str, tuple]] = None
    ordered_prediction_keys: bool = False    # list(predictions) == the keys, not sorted(...)
    predict_what: str = "{name} predict/{key}"
    n_grads: Union[None, int, Dict[str, int]] = None       # gradient arrays per golden (None: not counted)
    n_masks: Optional[int] = None            # restate_on_host: dropout calls of a golden with dropout_rate > 0
    lr_key: str = "meta/learning_rate"
    eval: bool = True                        # the golden has an eval/ section
    # ---- the explicit exceptions -------------------------------------------------------------------------------------------
    translate: Optional[Callable] = None     # (name, section, params) -> the section under the mirror's variable names
    golden_only: Optional[str] = None        # regex: golden variables the mirror may lack
    mirror_only: Optional[str] = None        # regex: mirror variables the golden may lack
    skip_absent: bool = False                # gradients / updated variables the mirror does not report are passed over
    feed_encoded: bool = False               # the device batch is the encoded ids (Ragged for bags), not the strings
    loss_seed: Optional[float] = None        # TRAIN runs under ops.loss_seed(...) and backward gets an explicit ones seed
    eval_no_grad: bool = False               # EVAL under torch.no_grad()
    # (golden, produced, variable name) -> bool: True where the variable has another optimizer than Adam, judged by the hook
    other_optimizer: Optional[Callable] = None
    produce_extra: Optional[Callable] = None               # (est, produced) after apply_gradients: fills produced["extra"]
    judge_extra: Optional[Callable] = None                 # (case, golden, produced) -> None: the model's own assertions

    def labels(self, d, labels):
        """float64 labels by task: the shared batch carries `read_comment`, the other tasks' are part of the golden"""
        if not self.tasks:
            return {"read_comment": labels}
        return {t: (labels if t == "read_comment" else torch.from_numpy(d[f"in/label_{t}"].copy())) for t in self.tasks}

    def prediction_paths(self, d):
        if self.predictions is not None:
            return self.predictions
        return {k: ({"probabilities": "prob"}.get(k, k),) for k in GU.section(d, "predict/")}

    def metric_keys(self):
        """EVAL metric key -> (key in the golden's eval/ section, label)"""
        kinds = ("accuracy", "auc")
        if self.tasks:
            return {f"eval_{t}_{kind}": (f"{t}_{kind}", f"{t} {kind}") for t in self.tasks for kind in kinds}
        return {f"eval_{kind}": (kind, kind) for kind in kinds}


@dataclass
class Golden:
    """A golden's sections under the mirror's variable names."""
    name: str
    d: dict
    params: dict
    var: dict
    grad: dict
    var_after: dict
    lr: float


def load_golden(case: GoldenCase, name, params) -> Golden:
    d = GU.load(name)
    tr = case.translate or (lambda name, section, params: section)
    return Golden(name, d, params, *(tr(name, GU.section(d, s), params) for s in ("var/", "grad/", "var_after/")), float(d[case.lr_key]))


def _path(out, path):
    for key in path:
        out = out.get(key) if isinstance(out, dict) else out[key]
        if out is None:
            return None
    return out


def _float_feats(feats, dtype):
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in feats.items()}


def run_oracle(case: GoldenCase, golden: Golden, dtype, variables=None, **train_kwargs):
    """The oracle in `dtype` on the golden's variables (or `variables`) -> {"predict", "loss", "grads", "P"}: PREDICT's output
    dict, the TRAIN loss with the golden's dropout masks, and every variable's gradient (zeros where autograd reports none)."""
    d = golden.d
    sfeats, labels = GU.string_batch()
    P = {k: torch.from_numpy(np.array(v)).to(dtype).requires_grad_(not k.split("/")[-1].startswith("moving_"))
         for k, v in (golden.var if variables is None else variables).items()}
    feats = _float_feats(case.encode(golden.params, sfeats), dtype)
    lab = {t: v.to(dtype) for t, v in case.labels(d, labels).items()}
    masks = [m.to(dtype) for m in GU.dropout_masks(d)]
    predict = case.oracle(P, feats, None, golden.params, training=False)
    train = case.oracle(P, feats, lab, golden.params, training=True, **({"dropout_masks": masks} if masks else {}), **train_kwargs)
    train["loss"].backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in P.items()}
    return {"predict": predict, "loss": train["loss"], "grads": grads, "P": P, "feats": feats, "labels": lab}


def restate32(case: GoldenCase, golden: Golden):
    """The reference arithmetic's own fp32 rounding on this batch (the oracle in float32 on the golden's variables):
    assert_close(ref32=) holds the kernels to 1.5 x its count of elements outside the strict bound."""
    return run_oracle(case, golden, torch.float32)


# ---- the producer: the mirror on the device ------------------------------------------------------------------------------------
def build_on_device(dev, case: GoldenCase, name, tmp_path, seed=3):
    """-> (estimator, golden, device features, device labels): the mirror built on `dev` from the string batch; the golden's
    variables are not loaded yet."""
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.feature_column import Ragged
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = case.mirror_setup(name, vocab_dir)
    golden = load_golden(case, name, params)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {t: v.float() for t, v in case.labels(golden.d, labels).items()}
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=seed, use_hip_graph=False))
    est.build(feats, lab)
    if case.feed_encoded:                    # the batch as encoded ids on the device (what a training loop feeds)
        dfeats = {}
        for k, v in case.encode(params, sfeats).items():
            if isinstance(v, tuple):
                dfeats[k] = Ragged(v[0].to(dev), v[1].to(dev))
            else:
                dfeats[k] = v.float().to(dev) if v.is_floating_point() else v.to(dev)
        feats, lab = dfeats, {t: v.to(dev) for t, v in lab.items()}
    else:
        feats, lab = est._to_device(feats, lab)
    return est, golden, feats, lab


def load_variables(est, values):
    arrays = est.store.named_arrays()
    for k, v in values.items():
        if k in arrays:
            arrays[k].copy_(torch.from_numpy(v).float().reshape(arrays[k].shape))


def produce_on_device(dev, case: GoldenCase, name, tmp_path):
    """Runs the mirror: build, load the golden's variables, PREDICT, the golden's masks into nn.DROPOUT_KEEP_MASKS, TRAIN,
    backward, named_grads, apply_gradients, load var_after/, EVAL.  -> (golden, produced); produced holds plain values only."""
    from recalgorithm_amd import nn, ops
    from recalgorithm_amd.estimator import ModeKeys
    from recalgorithm_amd.variables import named_grads
    est, golden, feats, lab = build_on_device(dev, case, name, tmp_path)
    out = {"variables": list(est.store.named_arrays()), "extra": {}}
    load_variables(est, golden.var)
    before = {k: v.detach().cpu().double().clone() for k, v in est.store.named_arrays().items()}
    pr = est._call_model_fn(feats, None, ModeKeys.PREDICT)
    out["predictions"] = {k: v.detach().cpu() for k, v in pr.predictions.items()}
    nn.DROPOUT_KEEP_MASKS[:] = GU.dropout_masks(golden.d)
    # (loss_seed: a training step's setting, under which a wide logit joins the fused logit / loss launch)
    with (ops.loss_seed(case.loss_seed) if case.loss_seed is not None else contextlib.nullcontext()):
        spec = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
    out["masks_consumed"] = not nn.DROPOUT_KEEP_MASKS
    nn.DROPOUT_KEEP_MASKS[:] = []
    if case.loss_seed is not None:
        spec.loss.backward(torch.ones_like(spec.loss))
    else:
        spec.loss.backward()
    grads = named_grads(est.store)           # (finishes the step's deferred sums: a fused tail's loss value among them)
    out["loss"] = spec.loss.detach().cpu()
    out["grads"] = {k: g.detach().cpu() for k, g in grads.items()}
    spec.train_op.optimizer.apply_gradients(est.store)
    after = est.store.named_arrays()
    out["before"] = before
    out["update"] = {k: after[k].detach().cpu().double() - before[k] for k in golden.var_after if k in after}
    if case.produce_extra is not None:
        case.produce_extra(est, out)
    if case.eval:
        # EVAL on the golden's state after the step (its variables and moving statistics loaded: the mirror's own step is judged
        # element by element with the bound that knows where a first Adam step is ill-conditioned; EVAL is judged on its own)
        load_variables(est, golden.var_after)
        with (torch.no_grad() if case.eval_no_grad else contextlib.nullcontext()):
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
        out["eval_loss"] = ev.loss.detach().cpu()
        out["eval_metrics"] = {}
        for key, metric in ev.eval_metric_ops.items():
            metric[0].update()
            out["eval_metrics"][key] = metric[0].result()
    return golden, out


# ---- the judge: every assertion, the tolerance policy ---------------------------------------------------------------------------
def gradient_floors(gg):
    """-> floor(k, base=0): base + the absolute floor of gradient k of a golden's grad/ section `gg`."""
    gmax = {k: float(np.abs(v).max()) for k, v in gg.items()}
    # batch-summed gradients downstream of a BatchNorm cancel (sum_b g_b = 0): their fp32 error is set by the size of the
    # terms, i.e. by the largest gradients of the dense stack
    dense_floor = 1e-6 * max(v for k, v in gmax.items() if "embedding_weights" not in k)

    def floor(k, base=0.0):
        # a bias ahead of a training-mode BatchNorm (or under a softmax) is an analytic zero: judged at its sibling kernel's scale
        return base + dense_floor + (1e-5 * gmax.get(k.replace("/bias", "/kernel"), 0.0) if k.endswith("/bias") else 0.0)
    return floor


def judge_adam_update(golden: Golden, k, upd, before, floors, what):
    """One TF1-Adam step of variable k against the golden's: step 1 moves by lr*g/(|g|+eps'), ill-conditioned where |g| ~ eps';
    the accepted gradient tolerance is pushed through that (tests/util.py assert_adam_update)."""
    ref_upd = torch.from_numpy(golden.var_after[k]).reshape(before.shape) - torch.from_numpy(golden.var[k]).reshape(before.shape)
    gref = torch.from_numpy(golden.grad[k]).reshape(before.shape).abs()
    tol_g = floors(k, 1e-5 * (gref + gref.pow(2).mean().sqrt()) + 1e-6 * gref.max())
    assert_adam_update(upd, ref_upd, before, gref, tol_g, golden.lr, what=what)


def judge(case: GoldenCase, golden: Golden, produced, ref32):
    name, d = golden.name, golden.d
    gv, gg, ga = golden.var, golden.grad, golden.var_after
    # the variable names, both ways
    have = set(produced["variables"])
    missing = [k for k in gv if k not in have and not (case.golden_only and re.search(case.golden_only, k))]
    assert not missing, f"golden (reference) variables absent from the mirror: {missing}"
    extra = [k for k in produced["variables"] if k not in gv and not (case.mirror_only and re.search(case.mirror_only, k))]
    assert not extra, f"mirror variables the reference does not have: {extra}"
    # PREDICT
    paths = case.prediction_paths(d)
    got_keys = list(produced["predictions"])
    if case.predictions is not None:
        if case.ordered_prediction_keys:
            assert got_keys == list(paths), f"{name}: prediction keys {got_keys}, expected {list(paths)}"
        else:
            assert sorted(got_keys) == sorted(paths), f"{name}: prediction keys {sorted(got_keys)}, expected {sorted(paths)}"
    for key, path in paths.items():
        assert key in produced["predictions"], f"{name}: no prediction {key!r} (the mirror has {got_keys})"
        assert_close(produced["predictions"][key], torch.from_numpy(d[f"predict/{key}"]),
                     what=case.predict_what.format(name=name, key=key), ref32=_path(ref32["predict"], path))
    # TRAIN: the dropout masks the reference drew, the loss, every gradient
    assert produced["masks_consumed"], "the mirror made fewer dropout calls than the reference"
    assert_close(produced["loss"], torch.from_numpy(d["train/loss"]), what=f"{name} loss", ref32=ref32["loss"])
    grads = produced["grads"]
    if not case.skip_absent:
        absent = [k for k in gg if k not in grads]
        assert not absent, f"{name}: gradients the mirror does not report: {absent}"
    if case.n_grads is not None:
        n = case.n_grads[name] if isinstance(case.n_grads, dict) else case.n_grads
        assert len(gg) == n, f"{name}: the golden holds {len(gg)} gradient arrays, expected {n}"
    floors = gradient_floors(gg)
    for k, g in gg.items():
        if k not in grads:
            continue
        assert_close(grads[k], torch.from_numpy(g), what=f"{name} d({k})", reduced=True, floor=floors(k), ref32=ref32["grads"].get(k))
    # one optimizer step: TF1-Adam with the ill-conditioned-element bound, BatchNorm's moving statistics
    before = produced["before"]
    for k, va in ga.items():
        if case.other_optimizer is not None and case.other_optimizer(golden, produced, k):
            continue
        if k not in produced["update"]:
            assert case.skip_absent, f"{name}: no update of {k} reported"
            continue
        ref_upd = torch.from_numpy(va).reshape(before[k].shape) - torch.from_numpy(gv[k]).reshape(before[k].shape)
        upd = produced["update"][k]
        if "moving_" in k:                   # BatchNorm moving statistics (momentum 0.99), updated by the forward
            # 1e-7 absolute: (1 - 0.99) * batch mean, where the mean of a centred activation is an analytic zero (DIN with
            # alpha = 1)
            assert_close(upd, ref_upd, what=f"{name} {k} update", reduced=True, floor=1e-7)
            continue
        judge_adam_update(golden, k, upd, before[k], floors, what=f"{name} adam update {k}")
    if case.judge_extra is not None:
        case.judge_extra(case, golden, produced)
    # EVAL on the golden's state after the step
    if case.eval:
        assert_close(produced["eval_loss"], torch.from_numpy(d["eval/loss"]), what=f"{name} eval loss")
        keys = case.metric_keys()
        assert sorted(produced["eval_metrics"]) == sorted(keys), f"{name}: eval metrics {sorted(produced['eval_metrics'])}"
        for key, (gkey, label) in keys.items():
            assert_close(torch.tensor(produced["eval_metrics"][key]), torch.from_numpy(d[f"eval/{gkey}"]), what=f"{name} eval {label}")


def judge_step_against_oracle(est, spec, P, P32, before, lr, label, n_min):
    """A synthetic estimator's TRAIN `spec` against the oracle run on the same variables in float64 (`P`, already
    back-propagated) and float32 (`P32`): backward, every gradient, one Adam step.  No golden: the floor of each gradient is
    4x the deviation of the reference arithmetic itself in fp32 (batch sums of B terms); at least `n_min` gradients."""
    from recalgorithm_amd.variables import named_grads
    spec.loss.backward()
    grads = named_grads(est.store)
    tol_gs, n = {}, 0
    for name, p in P.items():
        if p.grad is None:
            continue
        g32 = P32[name].grad
        noise = float((g32.double() - p.grad).abs().max())
        gref = p.grad.abs()
        tol_gs[name] = 1e-5 * (gref + gref.pow(2).mean().sqrt()) + 1e-6 * gref.max() + 4 * noise
        sib = name.replace("bias", "kernel")
        n += 1
        if name.endswith("/bias") and sib in P and P[sib].grad is not None and "logit" not in name and "expert" not in name:
            # a bias in front of a training-mode BatchNorm: its batch-summed gradient cancels analytically; judged at the scale
            # of its sibling kernel's gradient (tests/test_gpu_baseline_shapes.py)
            scale = float(P[sib].grad.abs().max())
            err = float((grads[name].cpu().double() - p.grad).abs().max())
            assert err <= 1e-5 * scale + 4 * noise, f"d({name}): err {err} scale {scale} noise {noise}"
            tol_gs[name] = tol_gs[name] + 1e-5 * scale
            continue
        assert_close(grads[name], p.grad, what=f"{label} d({name})", reduced=True, floor=4 * noise, ref32=g32)
    assert n >= n_min
    spec.train_op.optimizer.apply_gradients(est.store)
    after = est.store.named_arrays()
    for name, p in P.items():
        if p.grad is None:
            continue
        pp, m_, v_ = before[name].clone(), torch.zeros_like(before[name]), torch.zeros_like(before[name])
        R.adam_tf1_step(pp, p.grad, m_, v_, 1, lr)
        upd = after[name].detach().cpu().double() - before[name]
        assert_adam_update(upd, pp - before[name], before[name], p.grad, tol_gs[name], lr, what=f"{label} adam update {name}")
    assert float(est.store.flat_grad.abs().sum()) == 0.0


def check_on_device(dev, case: GoldenCase, name, tmp_path):
    """A model's whole GPU golden test."""
    golden, produced = produce_on_device(dev, case, name, tmp_path)
    judge(case, golden, produced, restate32(case, golden))


# ---- the host-side twin: the float64 oracle reproduces the golden ----------------------------------------------------------------
def close(a, b, what, tol=TOL):
    """max error against tol * max|b| (+ 1e-15: gradients that vanish analytically — a bias ahead of a training-mode BatchNorm —
    are fp64 rounding noise on both sides)."""
    a = torch.as_tensor(np.asarray(a.detach() if isinstance(a, torch.Tensor) else a), dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64).reshape(-1)
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    scale = max(float(b.abs().max()), 1e-30) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * scale + 1e-15, f"{what}: max err {err:.3e} at scale {scale:.3e}"


def oracle_eval(case: GoldenCase, golden: Golden, variables):
    """EVAL of the float64 oracle on `variables` -> (loss, {metric key: value}): accuracy at 0.5 and tf.metrics.auc"""
    sfeats, labels = GU.string_batch()
    lab = case.labels(golden.d, labels)
    P = {k: torch.from_numpy(np.array(v)) for k, v in variables.items()}
    ev = case.oracle(P, case.encode(golden.params, sfeats), lab, golden.params, training=False)
    metrics = {}
    for t in (case.tasks or ["read_comment"]):
        prob = ev["probs"][t] if case.tasks else ev["prob"]
        stem = f"eval_{t}_" if case.tasks else "eval_"
        metrics[stem + "accuracy"] = float(((prob >= 0.5).double() == lab[t]).double().mean())
        metrics[stem + "auc"] = float(R.tf_metrics_auc(lab[t], prob))
    return ev["loss"].detach(), metrics


def restate_on_host(case: GoldenCase, name, tmp_path, other_step=None, **train_kwargs):
    """PREDICT, the mask count, the loss, the gradient count, no all-zero gradient in the golden, each gradient, one
    R.adam_tf1_step per variable against var_after/ (other_step(golden, k, p, g) -> True: that variable's own optimizer, judged
    there), EVAL loss, accuracy and R.tf_metrics_auc — all at TOL.  -> (golden, the oracle run) for a model's further checks."""
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    _, params = case.mirror_setup(name, vocab_dir)
    golden = load_golden(case, name, params)
    d, gg, ga = golden.d, golden.grad, golden.var_after
    masks = GU.dropout_masks(d)
    if case.n_masks is not None:
        assert len(masks) == (case.n_masks if float(params["dropout_rate"]) > 0 else 0)
    run = run_oracle(case, golden, torch.float64, **train_kwargs)
    for key, path in case.prediction_paths(d).items():
        close(_path(run["predict"], path), d[f"predict/{key}"], f"{name} {key}")
    close(run["loss"], d["train/loss"], f"{name} loss")
    if case.n_grads is not None:
        assert len(gg) == (case.n_grads[name] if isinstance(case.n_grads, dict) else case.n_grads)
    assert not [k for k in gg if k not in run["P"]]
    assert not [k for k, g in gg.items() if not np.any(g)], "an all-zero gradient in the golden"
    for k, g in gg.items():
        close(run["grads"][k], g, f"{name} d({k})")
        p, gt = run["P"][k].detach().clone(), torch.from_numpy(g.copy())
        if other_step is not None and other_step(golden, k, p, gt):
            continue
        R.adam_tf1_step(p, gt, torch.zeros_like(p), torch.zeros_like(p), 1, golden.lr)       # one TF1-Adam step (A-10)
        close(p, ga[k], f"{name} adam({k})")
    # EVAL after the step: the updated variables, the moving statistics the TRAIN run left
    loss, metrics = oracle_eval(case, golden, ga)
    close(loss, d["eval/loss"], f"{name} eval loss")
    for key, (gkey, label) in case.metric_keys().items():
        close(metrics[key], d[f"eval/{gkey}"], f"{name} eval {label}")
    return golden, run
