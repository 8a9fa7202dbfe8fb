"""-m gpu: the streaming-metrics kernel (include/recalgo_metrics.h) and evaluate() on it.

The kernel at the C ABI, against the host classes run on CPU copies of the same tensors (AUCMetric / AccuracyMetric; integer
counts, so every comparison is ==) and against tests/metrics_ref.py's numpy restatement of the bin rule:
  * n in {1, 63, 64, 65, 257, 4099} (wave, workgroup and multi-workgroup boundaries: a workgroup owns 1024 rows) x N in
    {2, 3, 200, 1024}; predictions at every threshold, its float32 neighbours, 0, 1, -0.0, outside [0, 1], NaN, +-inf; labels
    0, 1, 0.5 (a negative) and 0.50000006; a prediction stride of 3 beside a label stride of 1;
  * 1 slot, 6 slots (3 accuracy + 3 AUC, the multi-task layout) with a loss, 16 slots; three launches accumulate; a NULL loss
    leaves loss_sum and batches alone; loss_sum is the Python double sum of the fp32 losses, bit for bit;
  * once more under tests/redzone.py: nothing is written outside the state buffer, no input is touched.

evaluate() on DCN, DeepFM (BatchNorm) and MMoE (3 tasks), 5 batches of 64 rows and one of 37, after three training steps:
device metrics eager and device metrics captured each return exactly the dict of the host loop; with device metrics no
Metric.update() runs and there is one recalgo_metrics_update call per eager batch (none for a replay)."""
import ctypes

import numpy as np
import pytest
import torch

from recalgorithm_amd import _lib, ops
from recalgorithm_amd import feature_column as fc
from recalgorithm_amd.estimator import AccuracyMetric, AUCMetric, Estimator, EvalAccumulator, RunConfig
from recalgorithm_amd.io import synth
from tests import metrics_ref as R
from tests.redzone import guarded

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]
_SLOT = _lib.SERVING_HEADERS["recalgo_metrics.h"].structs["recalgo_metrics_slot_t"]


# ---- the kernel at the C ABI ----------------------------------------------------------------------------------------------------
class Case:
    """`rounds` batches of n rows for a list of slots [(R.AUC, N) | (R.ACCURACY, None)], on the host: per slot and round labels [n]
    and a [n, 3] matrix whose column 1 holds the predictions (columns 0 and 2: other values, a wrong stride would count them)."""

    def __init__(self, n, slots, rounds=3, seed=0):
        self.n, self.slots, self.rounds = n, slots, rounds
        rng = np.random.default_rng([seed, n, len(slots)])
        self.th = [None if kind == R.ACCURACY else R.thresholds(N) for kind, N in slots]
        self.data = []
        for r in range(rounds):
            per_slot = []
            for s, (kind, N) in enumerate(slots):
                if kind == R.AUC:
                    labels, p = R.batch(n, self.th[s], seed=100 * seed + 10 * s + r)
                else:
                    labels = R.EDGE_LABELS[rng.integers(0, 4, size=n)].copy()
                    p = (rng.random(n) < 0.5).astype(np.float32)
                    if n > 2:                       # NaN == NaN is false, on both sides
                        labels[2] = p[2] = np.nan
                mat = np.stack([1.0 - p, p, rng.random(n).astype(np.float32)], axis=1).astype(np.float32)
                per_slot.append((labels, mat))
            self.data.append(per_slot)
        self.losses = [np.float32(v) for v in rng.uniform(0.1, 3.0, size=rounds)]

    def host(self):
        """the host classes over CPU copies: ([filled-in Metric per slot], loss sum, batches)"""
        ms = []
        for s, (kind, N) in enumerate(self.slots):
            m = AUCMetric(None, None, N) if kind == R.AUC else AccuracyMetric(None, None)
            for r in range(self.rounds):
                labels, mat = self.data[r][s]
                m.labels, m.predictions = torch.from_numpy(labels).reshape(-1, 1), torch.from_numpy(mat)[:, 1:2]
                m.update()
            ms.append(m)
        loss_sum = 0.0
        for v in self.losses:
            loss_sum += float(torch.tensor(v))
        return ms, loss_sum, self.rounds

    def run(self, dev, place=None, zeros=torch.zeros, with_loss=True):
        """the launches -> the state buffer on the host (int64 words); place: host tensor -> its device copy"""
        place = place or (lambda t: t.to(dev))
        lib = _lib.load()
        table = (_SLOT * len(self.slots))()
        words = R.state_words(self.slots)
        assert lib.recalgo_metrics_state_bytes(table_of(self, table, None, dev, place), len(self.slots)) == 8 * words
        state = zeros(words, dtype=torch.int64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        keep = []
        for r in range(self.rounds):
            keep.append(table_of(self, table, r, dev, place, keep))
            loss = place(torch.tensor([self.losses[r]], dtype=torch.float32)) if with_loss else None
            keep.append(loss)
            lib.recalgo_metrics_update(table, len(self.slots), None if loss is None else loss.data_ptr(), self.n, state.data_ptr(), stream)
        torch.cuda.synchronize()
        return state.cpu()

    def check(self, state, with_loss=True):
        ms, loss_sum, batches = self.host()
        assert state.numel() == R.state_words(self.slots)
        if with_loss:
            assert int(state[1]) == batches
            assert state[:1].view(torch.float64).item().hex() == loss_sum.hex(), "loss_sum: the same double additions, bit for bit"
        else:
            assert int(state[0]) == 0 and int(state[1]) == 0, "a NULL loss leaves loss_sum and batches alone"
        for s, ((kind, N), first, m) in enumerate(zip(self.slots, R.slot_offsets(self.slots), ms)):
            if kind == R.ACCURACY:
                assert (float(state[first]), float(state[first + 1])) == (m.correct, m.total), f"slot {s}: correct, total"
                assert m.total == self.rounds * self.n
                continue
            hist = state[first:first + 2 * (N + 1)].reshape(2, N + 1)
            want = sum(R.hist(self.data[r][s][0], self.data[r][s][1][:, 1], self.th[s]) for r in range(self.rounds))
            assert np.array_equal(hist.numpy(), want), f"slot {s}: hist against the numpy restatement"
            got = AUCMetric(None, None, N)
            EvalAccumulator.fill_auc(got, hist)
            assert torch.equal(R.host_counts(got), R.host_counts(m)), f"slot {s}: tp / fp / fn / tn against AUCMetric.update"
            assert got.result() == m.result()


def table_of(case, table, r, dev, place, keep=None):
    """fills `table` for round r (None: kinds and sizes only); the device tensors it points to are appended to `keep`"""
    for s, (kind, N) in enumerate(case.slots):
        table[s].kind, table[s].num_thresholds = kind, (N or 0)
        if r is None:
            continue
        labels, mat = case.data[r][s]
        dl, dm = place(torch.from_numpy(labels)), place(torch.from_numpy(mat))
        keep += [dl, dm]
        table[s].labels, table[s].predictions = dl.data_ptr(), dm[:, 1].data_ptr()
        table[s].label_stride, table[s].prediction_stride = 1, 3
        if kind == R.AUC:
            dth = place(torch.from_numpy(case.th[s]))
            keep.append(dth)
            table[s].thresholds = dth.data_ptr()
    return table


SIX = [(R.ACCURACY, None)] * 3 + [(R.AUC, 200), (R.AUC, 2), (R.AUC, 1024)]
SIXTEEN = [(R.AUC, 200), (R.ACCURACY, None), (R.AUC, 3), (R.AUC, 1024)] * 4


@pytest.mark.parametrize("N", [2, 3, 200, 1024])
@pytest.mark.parametrize("n", SIZES)
def test_one_auc_slot(dev, n, N):
    case = Case(n, [(R.AUC, N)], seed=1)
    case.check(case.run(dev))


@pytest.mark.parametrize("n", SIZES)
def test_one_accuracy_slot_and_a_null_loss(dev, n):
    case = Case(n, [(R.ACCURACY, None)], seed=2)
    case.check(case.run(dev, with_loss=False), with_loss=False)


@pytest.mark.parametrize("n", SIZES)
def test_six_slots_with_a_loss(dev, n):
    case = Case(n, SIX, seed=3)
    case.check(case.run(dev))


def test_sixteen_slots(dev):
    case = Case(257, SIXTEEN, seed=4)
    case.check(case.run(dev))


@pytest.mark.parametrize("n,slots", [(4099, SIX), (65, SIXTEEN)], ids=["six", "sixteen"])
def test_guarded(dev, n, slots):
    """every input and the state buffer between 0xFF redzones: the counts are right, the redzones and the inputs untouched"""
    case = Case(n, slots, seed=5)
    with guarded() as g:
        state = case.run(dev, place=lambda t: g.input(t, dev), zeros=torch.zeros)
        assert "recalgo_metrics_update" in g.launched and any(r.kind == "zeros" for r in g.records)
    case.check(state)


def test_ops_metrics_update_is_that_launch(dev):
    """the Python entry on the model's tensors: a [B, 1] column view of a [B, T] matrix, [B, 1] labels, a 0-dim loss"""
    case = Case(300, SIX, rounds=2, seed=6)
    _, first, words = ops.metrics_slot_table([("accuracy", torch.zeros(1), torch.zeros(1))] * 3 + [
        ("auc", torch.zeros(1), torch.zeros(1), torch.zeros(N)) for _, N in SIX[3:]])
    assert first == R.slot_offsets(SIX) and words == R.state_words(SIX)
    state = torch.zeros(words, dtype=torch.int64, device=dev)
    th = [None if t is None else torch.from_numpy(t).to(dev) for t in case.th]
    for r in range(case.rounds):
        slots = []
        for s, (kind, _) in enumerate(SIX):
            labels, mat = case.data[r][s]
            dl, dm = torch.from_numpy(labels).to(dev).reshape(-1, 1), torch.from_numpy(mat).to(dev)
            slots.append(("accuracy", dl, dm[:, 1:2]) if kind == R.ACCURACY else ("auc", dl, dm[:, 1:2], th[s]))
        ops.metrics_update(slots, torch.tensor(case.losses[r], device=dev), state)
    case.check(state.cpu())
    with pytest.raises(TypeError):
        ops.metrics_update([("accuracy", dl.double(), dm[:, 1:2])], None, state)
    with pytest.raises(ValueError):
        ops.metrics_update([("accuracy", dl, dm[:, :2])], None, state)


# ---- evaluate() -----------------------------------------------------------------------------------------------------------------
B, LAST, N_FULL = 64, 37, 5


def _dcn(dev):
    from recalgorithm_amd.algorithm.DCN.dcn import dcn_model_fn
    spec = synth.SynthSpec(n_fields=8, max_vocab=500)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"category_feature_columns": [fc.embedding_column(c, 16) for c in cats], "dense_feature_columns": [],
              "hidden_units": ["64", "32"], "num_cross_layer": 3, "learning_rate": 0.005}
    return dcn_model_fn, params, spec, ()


def _deepfm(dev):
    from recalgorithm_amd.algorithm.DeepFM.deepfm import deepfm_model_fn
    spec = synth.SynthSpec(n_fields=8, max_vocab=500)
    cats = sorted([fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)], key=lambda c: c.key)
    params = {"first_order_feature_columns": [fc.indicator_column(c) for c in cats],
              "second_order_feature_columns": [fc.embedding_column(c, 16) for c in cats],
              "hidden_units": ["64", "32"], "dropout_rate": 0.0, "batch_norm": True, "learning_rate": 0.005}
    return deepfm_model_fn, params, spec, ()


def _mmoe(dev):
    from recalgorithm_amd.algorithm._common import dense_columns
    from recalgorithm_amd.algorithm.MMOE.mmoe import mmoe_model_fn
    from tests.test_gpu_mmoe import DIMS, TASKS
    spec = synth.SynthSpec(n_fields=8, max_vocab=400, seed=11, oov_frac=0.05, with_dense=True)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    params = {"dense_feature_columns": dense_columns(), "category_feature_columns": [fc.embedding_column(c, k) for c, k in zip(cats, DIMS)],
              "hidden_units": ["64", "32"], "dropout_rate": 0.1, "batch_norm": True, "learning_rate": 0.005,
              "num_experts": 3, "num_tasks": 3, "expert_hidden_units": 64, "task_names": list(TASKS)}
    return mmoe_model_fn, params, spec, tuple(TASKS[1:])


MODELS = {"dcn": _dcn, "deepfm": _deepfm, "mmoe": _mmoe}
_shared = {}


def _setup(name, dev):
    """(estimator after three training steps, the six EVAL batches, the host loop's result): built once per model"""
    if name not in _shared:
        model_fn, params, spec, extra = MODELS[name](dev)
        est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, use_hip_graph=False, device_metrics=False))
        sizes = [B] * N_FULL + [LAST]
        batches = [synth.device_features(spec, b, dev, batch_index=i, extra_labels=extra)[:2] for i, b in enumerate(sizes)]
        train = synth.device_features(spec, 256, dev, batch_index=50, extra_labels=extra)[:2]
        est.build(*train)
        for _ in range(3):
            est.train_step(*train)
        want = est.evaluate(lambda: iter(batches))
        assert 0.0 < want["loss"] and all(np.isfinite(v) for v in want.values())
        assert len(want) == 2 + 2 * (1 + len(extra))
        _shared[name] = (est, batches, want)
    return _shared[name]


class _Counting:
    """the loaded library, counting the calls of each recalgo_* entry"""

    def __init__(self, lib):
        self.__dict__.update(lib=lib, calls={})

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call if name.startswith("recalgo_") else fn


def _evaluate(est, batches, monkeypatch, **run):
    """evaluate() under `run`, with Metric.update() forbidden -> (result, calls of recalgo_metrics_update)"""
    def forbidden(self):
        raise AssertionError("Metric.update() ran under device_metrics=True")
    for cls in (AUCMetric, AccuracyMetric):
        monkeypatch.setattr(cls, "update", forbidden)
    lib = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    for k, v in run.items():
        monkeypatch.setattr(est.config, k, v)
    out = est.evaluate(lambda: iter(batches))
    return out, lib.calls.get("recalgo_metrics_update", 0)


@pytest.mark.parametrize("name", list(MODELS))
def test_device_metrics_return_the_host_loops_dict(dev, name, monkeypatch):
    est, batches, want = _setup(name, dev)
    got, launches = _evaluate(est, batches, monkeypatch, device_metrics=True, use_hip_graph=False)
    assert got == want and list(got) == list(want)
    assert launches == N_FULL + 1, "one recalgo_metrics_update per batch"


@pytest.mark.parametrize("name", list(MODELS))
def test_the_captured_eval_step_returns_that_dict_too(dev, name, monkeypatch):
    est, batches, want = _setup(name, dev)
    got, launches = _evaluate(est, batches, monkeypatch, device_metrics=True, use_hip_graph=True)
    assert got == want and list(got) == list(want)
    # batches 1 and 2 eager, batch 3 captured (one call, recorded) and replayed, 4 and 5 replays, the batch of 37 eager
    assert launches == 4, "two eager batches, the capture, the partial batch: a replay calls nothing"


@pytest.mark.parametrize("name", list(MODELS))
def test_evaluate_never_calls_update_under_device_metrics(dev, name, monkeypatch):
    """fails without the feature: evaluate() then runs the host loop, whose first update() raises"""
    est, batches, want = _setup(name, dev)
    got, launches = _evaluate(est, batches[:2] + batches[-1:], monkeypatch, device_metrics=True, use_hip_graph=False)
    assert launches == 3 and got["global_step"] == want["global_step"] and set(got) == set(want)
    monkeypatch.undo()
    assert est.config.device_metrics is False and est.evaluate(lambda: iter(batches)) == want, "the host loop is as it was"
