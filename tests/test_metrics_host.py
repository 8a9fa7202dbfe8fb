"""CPU: the evaluation metrics without a GPU.
  * include/recalgo_metrics.h literally: names, signatures, the slot struct, constants, the state-size query at each limit and one
    past it, every refusal before any launch; its place in _lib's header tables and every per-header check of tests/test_abi.py;
  * EvalAccumulator.fill_auc / fill_accuracy: integer histograms (tests/metrics_ref.py, the header's bin rule in numpy) become
    exactly the tp / fp / fn / tn that AUCMetric.update adds up, on random data and on the edge set (every threshold, its
    float32 neighbours, NaN, +-inf, labels at and just above 0.5), over several batches;
  * evaluate() on a CPU store: RunConfig(device_metrics=True), the default, takes the host loop there and returns what the loop
    over Metric.update() returns."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_metrics.h")
NAME = "recalgo_metrics.h"

DECLARED = ["recalgo_metrics_abi_version", "recalgo_metrics_state_bytes", "recalgo_metrics_update"]
LAUNCHES = ["recalgo_metrics_update"]
FAKE = 0x10000           # a non-NULL, 16-byte aligned address: the refusals below happen before anything is read through it


def _table(abi, slots):
    """slots: [dict(field=value)] over a valid AUC(200) slot at fake addresses"""
    Slot = abi.structs["recalgo_metrics_slot_t"]
    t = (Slot * max(len(slots), 1))()
    for i, over in enumerate(slots):
        d = dict(labels=FAKE, predictions=FAKE, thresholds=FAKE, kind=R.AUC, num_thresholds=200, label_stride=1, prediction_stride=1)
        d.update(over)
        for k, v in d.items():
            setattr(t[i], k, v)
    return t


def test_header_literal_expectations():
    from recalgorithm_amd import _lib, build, ops
    build.build(verbose=False)
    abi = _lib.SERVING_HEADERS[NAME]
    assert list(abi.functions) == DECLARED and abi.launches == LAUNCHES and list(abi.structs) == ["recalgo_metrics_slot_t"]
    lib = _lib.load()
    assert lib.recalgo_metrics_abi_version() == abi.version == 1 and abi.label == "METRICS ABI"
    c_int, c_int64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    F = abi.functions
    assert F["recalgo_metrics_abi_version"] == (c_int, []) and F["recalgo_metrics_state_bytes"] == (c_int64, [ptr, c_int])
    assert F["recalgo_metrics_update"] == (c_int, [ptr, c_int, ptr, c_int, ptr, ptr])
    assert abi.structs["recalgo_metrics_slot_t"]._fields_ == [("labels", ptr), ("predictions", ptr), ("thresholds", ptr), ("kind", c_int),
                                                              ("num_thresholds", c_int), ("label_stride", c_int), ("prediction_stride", c_int)]
    assert ctypes.sizeof(abi.structs["recalgo_metrics_slot_t"]) == 40
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RECALGO_METRICS_\w+) (0x[0-9A-Fa-f]+|\d+)", open(HEADER).read())
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_METRICS_ABI_VERSION": 1, "RECALGO_METRICS_MAX_SLOTS": 16, "RECALGO_METRICS_MAX_THRESHOLDS": 1024,
                                        "RECALGO_METRICS_AUC": 0, "RECALGO_METRICS_ACCURACY": 1}
    assert (ops.METRICS_MAX_SLOTS, ops.METRICS_MAX_THRESHOLDS, ops.METRICS_KINDS) == (16, 1024, {"auc": R.AUC, "accuracy": R.ACCURACY})

    # the state-size query (host side): the documented layout, each limit and one past it
    size = lambda slots: lib.recalgo_metrics_state_bytes(_table(abi, slots), len(slots))
    assert size([{}]) == 8 * (2 + 2 * 201) == 8 * R.state_words([(R.AUC, 200)])
    assert size([dict(kind=R.ACCURACY)]) == 8 * 4
    six = [{}, dict(kind=R.ACCURACY), dict(num_thresholds=2), dict(kind=R.ACCURACY), dict(num_thresholds=1024), dict(kind=R.ACCURACY)]
    assert size(six) == 8 * R.state_words([(R.AUC, 200), (R.ACCURACY, None), (R.AUC, 2), (R.ACCURACY, None), (R.AUC, 1024), (R.ACCURACY, None)])
    assert [size([dict(num_thresholds=N)]) for N in (1, 2, 1024, 1025)] == [0, 8 * 8, 8 * 2052, 0]
    assert size([]) == 0 and size([{}] * 16) == 8 * (2 + 16 * 402) and size([{}] * 17) == 0
    assert size([dict(kind=2)]) == 0 and size([dict(kind=-1)]) == 0 and lib.recalgo_metrics_state_bytes(None, 1) == 0
    assert size([dict(kind=R.ACCURACY, num_thresholds=0, thresholds=None)]) == 8 * 4       # (an accuracy slot's N is not read)

    # every refusal returns hipErrorInvalidValue through the errcheck, before any launch (fake addresses: nothing is read)
    refused = pytest.raises(_lib.RecalgoError, match="recalgo_metrics_update failed with hipError_t=1$")

    def update(slots, n_slots=None, loss=None, n=64, state=FAKE):
        t = None if slots is None else _table(abi, slots)
        return lib.recalgo_metrics_update(t, len(slots) if n_slots is None else n_slots, loss, n, state, None)
    for n in (0, -1):
        with refused:
            update([{}], n=n)
    for count in (0, 17, -1):
        with refused:
            update([{}] * 17, n_slots=count)
    for N in (1, 0, 1025):
        with refused:
            update([dict(num_thresholds=N)])
    with refused:
        update(None, n_slots=1)
    with refused:
        update([{}], state=None)
    for field in ("labels", "predictions", "thresholds"):
        with refused:
            update([{}, {field: None}])
        for off in (1, 2, 3):
            with refused:
                update([{field: FAKE + off}])
    for bad in (dict(kind=2), dict(label_stride=0), dict(prediction_stride=0), dict(prediction_stride=-3)):
        with refused:
            update([bad])
    for off in (1, 2, 4, 7):
        with refused:
            update([{}], state=FAKE + off)
    for off in (1, 2, 3):
        with refused:
            update([{}], loss=FAKE + off)
    with refused:
        update([dict(kind=R.ACCURACY, thresholds=None), dict(kind=R.ACCURACY, labels=None)])      # any slot


def test_the_header_tables():
    from recalgorithm_amd import _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers()
    assert list(_lib.every_header()) == list(_lib.HEADERS) + list(_lib.MORE_HEADERS) + list(_lib.SERVING_HEADERS)
    lib = _lib.load()
    for name, (res, args) in _lib.SERVING_HEADERS[NAME].functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name


def test_every_shared_abi_check_holds_for_the_new_header(monkeypatch):
    """tests/test_abi.py runs once per entry of _lib.HEADERS; with the table replaced by the union of all three, each of its
    per-header checks is called on the new header, and the all-pairs check on the union."""
    from recalgorithm_amd import _abi, _lib, build
    from tests import test_abi as A
    union = _lib.every_header()
    monkeypatch.setattr(_lib, "HEADERS", union)
    monkeypatch.setattr(A, "HEADERS", list(union))
    lib_path = build.build(verbose=False)
    A.test_header_declares_functions(NAME)
    A.test_library_exports_every_declared_symbol(NAME, lib_path)
    A.test_ctypes_binding_matches_header(NAME, lib_path)
    A.test_loaded_functions_carry_the_table(NAME, lib_path)
    A.test_declarations_do_not_change_without_a_version_bump(NAME)
    A.test_header_arg_counts_match_binding(NAME)
    A.test_header_arg_types_match_binding(NAME)
    A.test_header_is_self_contained(NAME)
    A.test_the_headers_share_no_name()
    A.test_stale_version_fails_loudly(NAME, lib_path, monkeypatch)
    assert _abi.read_record(NAME) == {1: _abi.declaration_hash(NAME)}, "include/recalgo_metrics.abi records version 1's hash"


# ---- counts -> tp / fp / fn / tn ------------------------------------------------------------------------------------------------
def _batches(N, kind):
    th = R.thresholds(N)
    if kind == "random":
        rng = np.random.default_rng([7, N])
        return [((rng.random(n) < 0.3).astype(np.float32), rng.random(n).astype(np.float32)) for n in (257, 64, 1)]
    return [R.batch(n, th, seed=s) for s, n in enumerate((3 * N + 12, 65, 4099))]


@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("N", [2, 3, 200, 1024])
def test_the_histogram_becomes_the_counts_update_adds_up(N, kind):
    from recalgorithm_amd.estimator import AUCMetric, EvalAccumulator
    from oracle import ref_ops
    host = AUCMetric(None, None, num_thresholds=N)
    assert np.array_equal(host.th.numpy(), R.thresholds(N)), "the numpy restatement of the thresholds"
    total = np.zeros((2, N + 1), np.int64)
    for labels, p in _batches(N, kind):
        host.labels, host.predictions = torch.from_numpy(labels).reshape(-1, 1), torch.from_numpy(p).reshape(-1, 1)
        host.update()
        h = R.hist(labels, p, host.th.numpy())
        assert h.sum() == len(p)
        total += h
    if kind == "edge":
        assert np.count_nonzero(total.sum(0)) == N + 1 and total.sum(1).min() > 0, "every bin, both classes"
        # a NaN lands in bin 0, +inf in bin N, a threshold itself below its own bin: p > th[j] is strict
        th = host.th.numpy()
        assert list(R.bins(np.array([np.nan, np.inf, -np.inf], np.float32), th)) == [0, N, 0]
        assert list(R.bins(th, th)) == list(range(N)) and list(R.bins(np.nextafter(th, np.float32(np.inf)), th)) == list(range(1, N + 1))
        assert list(R.hist(R.EDGE_LABELS, np.full(4, 0.25, np.float32), th).sum(1)) == [2, 2]
    filled = AUCMetric(None, None, num_thresholds=N)
    EvalAccumulator.fill_auc(filled, torch.from_numpy(total.reshape(-1)))
    assert filled.tp.dtype == torch.float64 and filled.tp.shape == (N,)
    assert torch.equal(R.host_counts(filled), R.host_counts(host))
    assert filled.result() == host.result()
    if kind == "random":                    # (float64 thresholds there: a prediction next to a threshold may fall on the other side)
        labels = np.concatenate([b[0] for b in _batches(N, kind)])
        p = np.concatenate([b[1] for b in _batches(N, kind)])
        assert abs(filled.result() - ref_ops.tf_metrics_auc(torch.from_numpy(labels), torch.from_numpy(p), N)) <= 1e-12


def test_fill_accuracy():
    from recalgorithm_amd.estimator import AccuracyMetric, EvalAccumulator
    labels = torch.tensor([0.0, 1.0, 1.0, float("nan"), 0.0]).reshape(-1, 1)
    preds = torch.tensor([0.0, 1.0, 0.0, float("nan"), 1.0]).reshape(-1, 1)
    host = AccuracyMetric(labels, preds)
    host.update()
    host.update()
    filled = AccuracyMetric(None, None)
    EvalAccumulator.fill_accuracy(filled, 4, 10)
    assert (filled.correct, filled.total) == (host.correct, host.total) == (4.0, 10.0) and filled.result() == host.result() == 0.4


def test_element_strides():
    from recalgorithm_amd import ops
    m = torch.zeros(8, 3)
    assert [ops.metrics_element_stride(t) for t in (m[:, 1:2], m[:, 0], torch.zeros(8, 1), torch.zeros(8), torch.zeros(1, 1), m)] == [3, 3, 1, 1, 1, 1]
    assert ops.metrics_element_stride(m[:, :2]) is None and ops.metrics_element_stride(torch.zeros(1, 1).expand(8, 1)) is None


# ---- evaluate() on a CPU store --------------------------------------------------------------------------------------------------
def _cpu_model_fn(features, labels, mode, params):
    from recalgorithm_amd.estimator import EstimatorSpec, metrics
    from recalgorithm_amd.variables import get_variable
    w = get_variable("w", [4, 1])
    logit = features["x"] @ w.data
    y = labels["read_comment"]
    prob = torch.sigmoid(logit)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    return EstimatorSpec(mode, loss=loss, eval_metric_ops={"eval_accuracy": metrics.accuracy(labels=y, predictions=(prob >= 0.5).float()),
                                                           "eval_auc": metrics.auc(labels=y, predictions=prob)})


@pytest.mark.parametrize("run", [dict(), dict(device_metrics=True), dict(device_metrics=False), dict(device_metrics=True, use_hip_graph=True)],
                         ids=["default", "device_metrics", "host_metrics", "device_metrics+graph"])
def test_evaluate_on_a_cpu_store_takes_the_host_loop(run, monkeypatch):
    from recalgorithm_amd import estimator as E
    from oracle import ref_ops
    g = torch.Generator().manual_seed(5)
    batches = [({"x": torch.randn(n, 4, generator=g)}, {"read_comment": (torch.rand(n, 1, generator=g) < 0.4).float()}) for n in (48, 48, 48, 21)]
    cfg = E.RunConfig(device="cpu", seed=3, **{"use_hip_graph": False, **run})
    assert cfg.device_metrics is run.get("device_metrics", True)
    est = E.Estimator(_cpu_model_fn, {}, cfg)
    updates = []
    for cls in (E.AUCMetric, E.AccuracyMetric):
        real = cls.update
        monkeypatch.setattr(cls, "update", lambda self, real=real: (updates.append(type(self).__name__), real(self))[1])
    out = est.evaluate(lambda: iter(batches))
    assert list(out) == ["eval_accuracy", "eval_auc", "loss", "global_step"] and out["global_step"] == 0
    assert updates == ["AccuracyMetric", "AUCMetric"] * 4, "the host loop: one update() per metric and batch"
    w = est.store.vars["w"].data
    logits = [f["x"] @ w for f, _ in batches]
    prob, y = torch.sigmoid(torch.cat(logits)), torch.cat([l["read_comment"] for _, l in batches])
    loss_sum = 0.0
    for lg, (_, l) in zip(logits, batches):
        loss_sum += float(torch.nn.functional.binary_cross_entropy_with_logits(lg, l["read_comment"]))
    assert out["loss"] == loss_sum / 4
    assert out["eval_accuracy"] == float(((prob >= 0.5).float() == y).sum()) / 165
    assert abs(out["eval_auc"] - ref_ops.tf_metrics_auc(y, prob)) <= 1e-12
    assert out == est.evaluate(lambda: iter(batches)) and est.evaluate(lambda: iter(batches), steps=2)["loss"] != out["loss"]
    assert est.evaluate(lambda: iter(())) == {"loss": 0.0, "global_step": 0}
