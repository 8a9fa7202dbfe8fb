"""CPU: the condition under which tests/test_gpu_trajectory.py is fair.  The oracle run in float32 must follow the oracle
run in float64 over the N = 6 Adam steps on the rotating sub-batches (tests/trajectory_ref.py) inside the bound the kernels
are held to — every element of every trainable variable, for every golden model — with head room: a reference that sat
near the bound by itself would make the GPU test a test of fp32, not of the kernels."""
import pytest
import torch

from tests import golden_util as GU
from tests import trajectory_ref as T

# The capped set of tensors outside any free-running comparison, per model (trajectory_ref.excluded finds it by rule;
# the rule's result must equal this list).  Every model not named here has none.
EXCLUDED = {
    # softmax is invariant under a shift of its logits: d loss / d f3_att/bias = sum_t ds_t = 0 exactly
    "model_din_prelu_softmax": ["attention_part/f3_att/bias"],
}

_SETUPS = {}


def get_setup(name, tmp_path):
    if name not in _SETUPS:
        _SETUPS[name] = T.Setup(name, GU.write_vocab_dir(str(tmp_path / "vocabulary")))
    return _SETUPS[name]


def test_batches_rotate_rows_out_and_back_in():
    idx = T.batch_indices()
    assert [len(i) for i in idx] == [T.BATCH] * 3 and all(bool((i[1:] > i[:-1]).all()) for i in idx)
    sets = [set(i.tolist()) for i in idx]
    # every batch has examples the next one lacks: their ids leave the step and return three steps later
    assert all(sets[a] - sets[(a + 1) % 3] for a in range(3))
    assert T.ORDER == (0, 1, 2, 0, 1, 2) and len(T.ORDER) == T.N_STEPS


@pytest.mark.parametrize("name", GU.MODELS)
def test_fp32_oracle_follows_fp64_oracle_inside_the_bound(name, tmp_path):
    s = get_setup(name, tmp_path)
    r64, r32 = s.run(torch.float64), s.run(torch.float32)
    assert len(r64["loss"]) == T.N_STEPS and all(torch.isfinite(l) for l in r64["loss"])
    assert len(r64["trainable"]) >= 10
    ex = T.excluded(s, r64)
    assert ex == EXCLUDED.get(name, []), f"{name}: tensors excluded by rule {ex} != the list written here"
    bnd = T.bounds(r64, s.lr)
    worst, where, outside = T.worst_ratio(r32["final"], r64, bnd, skip=ex)
    print(f"\n{name}: fp32 oracle vs fp64 oracle after {T.N_STEPS} steps: worst |p32 - p64| / tol = {worst:.3f} at {where}")
    assert worst <= 0.5, f"{name}: the fp32 reference alone uses {worst:.3f} of the bound at {where}"
    # the inputs are well conditioned: the same float32 arithmetic with the examples of every batch in another order (the
    # kernels sum in yet another) stays below half the bound and passes the count guard the kernels face, against this run
    for seed in (1, 2):
        w, wh, out = T.worst_ratio(s.run_reordered(seed)["final"], r64, bnd, skip=ex)
        print(f"{name}: fp32 oracle, examples reordered ({seed}): worst ratio {w:.3f} at {wh}, {sum(out.values())} elements outside tight "
              f"({sum(outside.values())} in the order above)")
        assert w <= 0.5, f"{name}: reordered fp32 reference at {w:.3f} of the bound ({wh})"
        for k in out:
            assert out[k] <= 1.5 * outside[k] + 10, f"{name} {k}: {out[k]} outside tight after reordering, {outside[k]} before"
    # the BatchNorm moving statistics under the GPU test's check: the fp32 oracle is inside it everywhere but on the
    # tensors trajectory_ref.MOVING_FOLLOWS_BIAS names (and explains), and inside the amended check there
    extra = T.moving_extra(name, bnd)
    plain = {n: T.moving_ratio(r32["moving"][-1][n], v) for n, v in r64["moving"][-1].items()}
    assert sorted(n for n, r in plain.items() if r > 0.5) == sorted(extra), plain
    for n in extra:
        r = T.moving_ratio(r32["moving"][-1][n], r64["moving"][-1][n], extra[n])
        print(f"{name}: {n}: fp32 oracle {plain[n]:.1f} x the plain moving-statistics tolerance, {r:.3f} x the amended one")
        assert r <= 0.5, (n, r)


@pytest.mark.parametrize("mutate", ["stale_step", "lazy_rows"])
def test_bound_notices_a_wrong_optimizer(mutate, tmp_path):
    """The bound is not slack: the float64 oracle with lr_t one step behind, or with table rows that skip the steps they are
    absent from (what a lazily evaluated table Adam that is NOT caught up computes), lands far outside it."""
    s = get_setup("model_dcn", tmp_path)
    r64 = s.run(torch.float64)
    worst, where, _ = T.worst_ratio(T.run_oracle(s, torch.float64, mutate=mutate)["final"], r64, T.bounds(r64, s.lr))
    print(f"\n{mutate}: worst ratio {worst:.1f} at {where}")
    assert worst > 10.0, (mutate, worst, where)
    if mutate == "lazy_rows":
        assert where.endswith("embedding_weights")
