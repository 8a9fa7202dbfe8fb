"""-m gpu: the masked streaming metrics (include/recalgo_maskmetrics.h) and evaluate() of ESMM on them.

The kernel at the C ABI against the brute-force counts of tests/esmm_ref.py, integers, so every comparison is ==:
  * n in {1, 1023, 1024, 1025, 4099} (a workgroup owns 1024 rows) x N in {2, 200, 1024}; per mask kind (all ones, all zeros, 30 %,
    one holding NaN, 0.5, its float32 successor, +-inf) an AUC and an accuracy slot, beside an unmasked pair, in ONE launch; 16 slots;
    labels, predictions and mask are the three columns of a [n, 3] matrix (step 3) inside a poisoned frame (tests/window.Frame);
  * mask NULL in every slot: the state words recalgo_metrics_update leaves.
evaluate() of ESMM on the host loop, on the device eagerly and captured: the same dict, key for key and bit for bit; no
Metric.update() on the device paths; one recalgo_maskmetrics_update and no recalgo_metrics_update per eager batch; MMoE still makes
only recalgo_metrics_update launches."""
import ctypes

import numpy as np
import pytest
import torch

from recalgorithm_amd import _lib, ops
from recalgorithm_amd.estimator import AccuracyMetric, AUCMetric, EvalAccumulator
from tests import esmm_ref as R
from tests import metrics_ref as MR
from tests.window import Frame

pytestmark = pytest.mark.gpu

_SLOT = _lib.SERVING_HEADERS["recalgo_maskmetrics.h"].structs["recalgo_maskmetrics_slot_t"]
_OLD = _lib.SERVING_HEADERS["recalgo_metrics.h"].structs["recalgo_metrics_slot_t"]
KINDS = ("ones", "zeros", "30 %", "nan")


def layout(N):
    """[(kind, N | None, mask kind | None)]: an unmasked pair, then per mask kind an AUC(N) and an accuracy slot"""
    return [(MR.AUC, N, None), (MR.ACCURACY, None, None)] + [s for k in KINDS for s in ((MR.AUC, N, k), (MR.ACCURACY, None, k))]


class Case:
    """`rounds` batches of n rows for a layout, on the host: per slot and round a [n, 3] float32 matrix (labels, predictions, mask)"""

    def __init__(self, n, slots, rounds=2, seed=0):
        self.n, self.slots, self.rounds = n, slots, rounds
        rng = np.random.default_rng([seed, n, len(slots)])
        self.th = [None if kind == MR.ACCURACY else MR.thresholds(N) for kind, N, _ in slots]
        self.data = []
        for r in range(rounds):
            per_slot = []
            for s, (kind, N, mk) in enumerate(slots):
                if kind == MR.AUC:
                    labels, p = MR.batch(n, self.th[s], seed=100 * seed + 10 * s + r)
                else:
                    labels = MR.EDGE_LABELS[rng.integers(0, 4, size=n)].copy()
                    p = (rng.random(n) < 0.5).astype(np.float32)
                # an unmasked slot's third column is a decoy: a mask that would drop every row, were it read
                mask = np.zeros(n, np.float32) if mk is None else R.mask_kinds(n, 1000 * seed + 10 * s + r)[mk]
                per_slot.append(np.stack([labels, p, mask], axis=1).astype(np.float32))
            self.data.append(per_slot)
        self.losses = [np.float32(v) for v in rng.uniform(0.1, 3.0, size=rounds)]

    def mask_of(self, r, s):
        return None if self.slots[s][2] is None else self.data[r][s][:, 2]

    def words(self):
        return MR.state_words([(k, N) for k, N, _ in self.slots])

    def run(self, dev, masked=True, drop_masks=False):
        """the launches (recalgo_maskmetrics_update, or recalgo_metrics_update with masked=False) -> (state on the host, frames)"""
        lib = _lib.load()
        table = ((_SLOT if masked else _OLD) * len(self.slots))()
        state = torch.zeros(self.words(), dtype=torch.int64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        th = [None if t is None else torch.from_numpy(t).to(dev) for t in self.th]
        frames = []
        for r in range(self.rounds):
            for s, (kind, N, mk) in enumerate(self.slots):
                f = Frame(self.n, 3, 3, 0, device=dev).put(torch.from_numpy(self.data[r][s]))
                frames.append(f)
                t, w = table[s], f.window
                t.kind, t.num_thresholds = kind, (N or 0)
                t.labels, t.predictions = w[:, 0].data_ptr(), w[:, 1].data_ptr()
                if kind == MR.AUC:
                    t.thresholds = th[s].data_ptr()
                if masked:
                    t.label_step = t.prediction_step = 3
                    t.mask, t.mask_step = (None, 0) if (mk is None or drop_masks) else (w[:, 2].data_ptr(), 3)
                else:
                    t.label_stride = t.prediction_stride = 3
            loss = torch.tensor([self.losses[r]], dtype=torch.float32, device=dev)
            update = lib.recalgo_maskmetrics_update if masked else lib.recalgo_metrics_update
            assert update(table, len(self.slots), loss.data_ptr(), self.n, state.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        for f in frames:
            f.assert_unchanged("an input frame")
        return state.cpu()

    def check(self, state):
        loss_sum = 0.0
        for v in self.losses:
            loss_sum += float(torch.tensor(v))
        assert int(state[1]) == self.rounds and state[:1].view(torch.float64).item().hex() == loss_sum.hex()
        for s, ((kind, N, mk), first) in enumerate(zip(self.slots, MR.slot_offsets([(k, n_) for k, n_, _ in self.slots]))):
            if kind == MR.ACCURACY:
                want = [sum(x) for x in zip(*(R.masked_accuracy(self.data[r][s][:, 0], self.data[r][s][:, 1], self.mask_of(r, s))
                                              for r in range(self.rounds)))]
                assert [int(state[first]), int(state[first + 1])] == want, f"slot {s} ({mk}): correct, total"
                if mk in (None, "ones"):
                    assert want[1] == self.rounds * self.n
                if mk == "zeros":
                    assert want == [0, 0]
                continue
            hist = state[first:first + 2 * (N + 1)].reshape(2, N + 1).numpy()
            want = sum(R.masked_hist(self.data[r][s][:, 0], self.data[r][s][:, 1], self.th[s], self.mask_of(r, s)) for r in range(self.rounds))
            assert np.array_equal(hist, want), f"slot {s} ({mk}): hist against the brute-force counts"
            if mk in (None, "ones"):
                assert np.array_equal(want, sum(MR.hist(self.data[r][s][:, 0], self.data[r][s][:, 1], self.th[s]) for r in range(self.rounds)))
            if mk == "zeros":
                assert not want.any()
            # and through the host class: fill_auc on the counts is what the masked update() adds up
            m = AUCMetric(None, None, N)
            for r in range(self.rounds):
                cols = torch.from_numpy(self.data[r][s])
                m.labels, m.predictions, m.mask = cols[:, 0:1], cols[:, 1:2], (None if mk is None else cols[:, 2:3])
                m.update()
            got = AUCMetric(None, None, N)
            EvalAccumulator.fill_auc(got, torch.from_numpy(hist.copy()))
            assert torch.equal(MR.host_counts(got), MR.host_counts(m)) and got.result() == m.result(), f"slot {s} ({mk})"


@pytest.mark.parametrize("N", [2, 200, 1024])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4099])
def test_masked_and_unmasked_slots_in_one_launch(dev, n, N):
    case = Case(n, layout(N), seed=1)
    case.check(case.run(dev))


def test_sixteen_slots(dev):
    slots = (layout(200) + layout(3))[:16]
    assert len(slots) == 16 and sum(1 for s in slots if s[2] is not None) == 12
    case = Case(257, slots, seed=2)
    case.check(case.run(dev))


@pytest.mark.parametrize("n", [1, 1025, 4099])
def test_a_null_mask_everywhere_is_recalgo_metrics_update(dev, n):
    """the same inputs through both entries, no mask given: the same state words, accuracy's total = n per batch among them"""
    case = Case(n, layout(200), seed=3)
    new, old = case.run(dev, masked=True, drop_masks=True), case.run(dev, masked=False)
    assert torch.equal(new, old)
    assert not torch.equal(new, case.run(dev)), "(the masks of this case do change the counts)"


def test_ops_maskmetrics_update_is_that_launch(dev):
    """the Python entry on the model's tensors: [B, 1] column views of a [B, 3] matrix, a 0-dim loss, None for an unmasked slot"""
    case = Case(300, layout(200), seed=4)
    state = torch.zeros(case.words(), dtype=torch.int64, device=dev)
    th = [None if t is None else torch.from_numpy(t).to(dev) for t in case.th]
    for r in range(case.rounds):
        slots = []
        for s, (kind, _, mk) in enumerate(case.slots):
            m = torch.from_numpy(case.data[r][s]).to(dev)
            mask = None if mk is None else m[:, 2:3]
            slots.append(("accuracy", m[:, 0:1], m[:, 1:2], mask) if kind == MR.ACCURACY else ("auc", m[:, 0:1], m[:, 1:2], th[s], mask))
        ops.maskmetrics_update(slots, torch.tensor(case.losses[r], device=dev), state)
    case.check(state.cpu())
    y, p = m[:, 0:1], m[:, 1:2]
    with pytest.raises(TypeError, match="mask must be float32"):
        ops.maskmetrics_update([("accuracy", y, p, m[:, 2:3].double())], None, state)
    with pytest.raises(ValueError, match="one element stride"):
        ops.maskmetrics_update([("accuracy", y, p, m[:, 1:3])], None, state)
    with pytest.raises(ValueError, match="one element stride"):
        ops.maskmetrics_update([("accuracy", y, p, m[:7, 2:3])], None, state)
    with pytest.raises(ValueError, match="state must be"):
        ops.maskmetrics_update([("accuracy", y, p, None)], None, state)


# ---- evaluate() -----------------------------------------------------------------------------------------------------------------
B, LAST, N_FULL = 64, 37, 5
_shared = {}


def _esmm(dev):
    """(estimator after three training steps, the six EVAL batches, the host loop's result): built once"""
    from tests.test_gpu_esmm import synthetic, synthetic_batch
    if "esmm" not in _shared:
        est, spec = synthetic(dev, seed=3, use_hip_graph=False, device_metrics=False)
        batches = [synthetic_batch(spec, b, dev, i) for i, b in enumerate([B] * N_FULL + [LAST])]
        train = synthetic_batch(spec, 256, dev, 50)
        for _ in range(3):
            est.train_step(*train)
        want = est.evaluate(lambda: iter(batches))
        _shared["esmm"] = (est, batches, want)
    return _shared["esmm"]


def _evaluate(est, batches, monkeypatch, **run):
    """evaluate() under `run`, with Metric.update() forbidden -> (result, calls per entry)"""
    from tests.test_gpu_metrics import _Counting

    def forbidden(self):
        raise AssertionError("Metric.update() ran under device_metrics=True")
    for cls in (AUCMetric, AccuracyMetric):
        monkeypatch.setattr(cls, "update", forbidden)
    lib = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    for k, v in run.items():
        monkeypatch.setattr(est.config, k, v)
    out = est.evaluate(lambda: iter(batches))
    return out, lib.calls.get("recalgo_maskmetrics_update", 0), lib.calls.get("recalgo_metrics_update", 0)


def test_evaluate_of_esmm_is_the_same_dict_on_the_three_paths(dev, monkeypatch):
    est, batches, want = _esmm(dev)
    assert list(want) == ["eval_ctr_auc", "eval_ctr_accuracy", "eval_ctcvr_auc", "eval_ctcvr_accuracy", "eval_cvr_auc", "eval_cvr_accuracy",
                          "loss", "global_step"]
    assert 0.0 < want["loss"] and all(np.isfinite(v) for v in want.values())
    # the mask matters: the CVR metrics over all impressions are other numbers
    clicked = sum(int((l["click_avatar"] > 0.5).sum()) for _, l in batches)
    assert 0 < clicked < N_FULL * B + LAST
    assert 0.0 < want["eval_cvr_auc"] < 1.0 and want["eval_cvr_auc"] != want["eval_ctcvr_auc"]
    got, masked, plain = _evaluate(est, batches, monkeypatch, device_metrics=True, use_hip_graph=False)
    assert got == want and list(got) == list(want), "device, eager"
    assert (masked, plain) == (N_FULL + 1, 0), "one recalgo_maskmetrics_update and no recalgo_metrics_update per eager batch"
    monkeypatch.undo()
    got, masked, plain = _evaluate(est, batches, monkeypatch, device_metrics=True, use_hip_graph=True)
    assert got == want and list(got) == list(want), "device, captured"
    # batches 1 and 2 eager, batch 3 captured (one call, recorded) and replayed, 4 and 5 replays, the batch of 37 eager
    assert (masked, plain) == (4, 0), "two eager batches, the capture, the partial batch: a replay calls nothing"
    monkeypatch.undo()
    assert est.config.device_metrics is False and est.evaluate(lambda: iter(batches)) == want, "the host loop is as it was"
    # a spec without a masked metric (MMoE, three tasks) still makes only the launches it made before masks existed
    from tests.test_gpu_metrics import _setup
    est, batches, want = _setup("mmoe", dev)
    got, masked, plain = _evaluate(est, batches, monkeypatch, device_metrics=True, use_hip_graph=False)
    assert got == want and list(got) == list(want)
    assert (masked, plain) == (0, N_FULL + 1)
