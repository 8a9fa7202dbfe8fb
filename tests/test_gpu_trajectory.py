"""-m gpu: N = 6 fused training steps (Estimator.train_step: the product step, not driven op by op) of every golden model
on rotating sub-batches, against the float64 oracle's free-running trajectory (tests/trajectory_ref.py).  What no
one-step test sees is in play from step 2 on: lr_t and the beta powers, non-zero moments, the device step counter, the
lazily exact table Adam for rows that leave the batch and return (with RECALGO_ADAM_SWEEP_PERIOD = 4 a sweep falls
inside the run), the BatchNorm moving statistics, the dropout masks of later steps.

The bound is trajectory_ref.bounds (float64 oracle quantities only); tests/test_trajectory_host.py shows that the float32
oracle itself stays below half of it on every model, names the tensors excluded from it and why.  The eager step takes
batches of different ragged totals (`manual_tag_list`, the history), so the three subsets are used as drawn."""
import re

import pytest
import torch

from recalgorithm_amd.estimator import Estimator, RunConfig
from tests import golden_util as GU
from tests import trajectory_ref as T
from tests import util
from tests.test_trajectory_host import EXCLUDED, get_setup
from tests.util import assert_close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", GU.MODELS)
def test_six_steps_follow_the_fp64_oracle(dev, name, tmp_path, monkeypatch):
    from recalgorithm_amd import nn
    monkeypatch.setenv("RECALGO_ADAM_SWEEP_PERIOD", "4")
    s = get_setup(name, tmp_path)
    r64, r32 = s.run(torch.float64), s.run(torch.float32)
    ex = EXCLUDED.get(name, [])
    assert T.excluded(s, r64) == ex
    bnd = T.bounds(r64, s.lr)

    est = Estimator(s.model_fn, s.params, RunConfig(device=dev, seed=3, use_hip_graph=False))
    host = [({k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sf.items()}, {"read_comment": lb.float()})
            for sf, lb in s.batches]
    est.build(*host[0])
    batches = [est._to_device(f, l) for f, l in host]
    arrays = est.store.named_arrays()
    missing = [k for k in s.start if k not in arrays and "dice_bn" not in k]
    assert not missing, f"oracle variables absent from the mirror: {missing}"
    extra = [k for k in arrays if k not in s.start and not re.search(r"/(wl|bl)$", k)]
    assert not extra, f"mirror variables the oracle does not have: {extra}"
    for k, v in s.start.items():            # the golden's variables, DIN's alphas moved (trajectory_ref.Setup)
        if k in arrays:
            arrays[k].copy_(v.float().reshape(arrays[k].shape))

    nn.DROPOUT_KEEP_MASKS[:] = [m.float() for step in s.masks for m in step]       # call order, all steps
    try:
        losses = [est.train_step(*batches[b]).clone() for b in T.ORDER]
        torch.cuda.synchronize()
        assert not nn.DROPOUT_KEEP_MASKS, "the mirror made fewer dropout calls than the oracle"
    finally:
        del nn.DROPOUT_KEEP_MASKS[:]

    for k, (l, l64, l32) in enumerate(zip(losses, r64["loss"], r32["loss"]), start=1):
        print(f"{name} step {k}: loss {float(l):.9g} fp64 oracle {float(l64):.9g} fp32 oracle {float(l32):.9g}")
        assert_close(l, l64, what=f"{name} loss of step {k}", ref32=l32)
    assert int(est.store.opt_state["step"]) == T.N_STEPS

    after = est.store.named_arrays()
    trainable = [k for k in after if k in r64["final"] and "/moving_" not in k and "dice_bn" not in k]
    assert set(r64["trainable"]) <= set(trainable)
    # every trainable array inside the bound; a variable without a gradient in the oracle (AFM's / NFM's unused tables) has
    # tol = tight and must not have moved at all beyond it
    got = {k: after[k] for k in trainable}
    ref_view = dict(r64, trainable=trainable)
    wk, wherek, outk = T.worst_ratio(got, ref_view, bnd, skip=ex)
    w32, where32, out32 = T.worst_ratio(r32["final"], ref_view, bnd, skip=ex)
    print(f"{name}: worst |p - p64| / tol after {T.N_STEPS} steps: kernels {wk:.3f} ({wherek}) | fp32 oracle {w32:.3f} ({where32})")
    util.STRICT_LOG.append({"test": f"tests/test_gpu_trajectory.py::test_six_steps_follow_the_fp64_oracle[{name}]",
                            "what": f"{name} variables after {T.N_STEPS} steps [worst |p - p64| / tol: kernels {wk:.3f} at {wherek}, "
                                    f"fp32 oracle {w32:.3f}; counts: elements outside N*(1e-5*lr + 6e-8*|p64|)]",
                            "n": sum(int(after[k].numel()) for k in outk), "strict_fail": sum(outk.values()), "worst": wk,
                            "ref32_strict_fail": sum(out32.values())})
    assert wk <= 1.0, f"{name}: {wherek} is {wk:.3f} x the bound after {T.N_STEPS} steps (fp32 oracle: {w32:.3f} at {where32})"
    for k in outk:      # the strict guard's form (tests/util.py::assert_close): elements outside `tight`, per tensor
        assert outk[k] <= 1.5 * out32[k] + 10, (f"{name} {k}: {outk[k]} elements outside the tight bound, the fp32 oracle "
                                                f"leaves {out32[k]} (limit 1.5 x + 10)")

    # no gradient is left behind for the next step
    assert not bool(est.store.flat_grad.any()), "flat_grad is not zero after the step"
    for an, ar in est.store.arenas.items():
        assert not bool(ar.grad.any()), f"arena {an}: grad is not zero after the step"

    # BatchNorm moving statistics: the momentum-0.99 recursion over the float64 oracle's batch moments
    more = T.moving_extra(name, bnd)
    for k, ref in r64["moving"][-1].items():
        if k in more:
            r = T.moving_ratio(after[k], ref, more[k])
            print(f"{name} {k}: {r:.3f} x the amended moving-statistics tolerance (trajectory_ref.MOVING_FOLLOWS_BIAS)")
            assert r <= 1.0, f"{name} {k}: {r:.3f} x the tolerance"
        else:
            assert_close(after[k], ref, what=f"{name} {k} after {T.N_STEPS} steps", reduced=True, floor=1e-7)
