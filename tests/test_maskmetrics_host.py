"""CPU: the masked evaluation metrics without a GPU.
  * include/recalgo_maskmetrics.h literally: names, signatures, the slot struct (recalgo_metrics_slot_t's fields, then the mask),
    constants, the state-size query against recalgo_metrics_state_bytes, every refusal before any launch, the .abi record; its
    place in _lib's header tables and every per-header check of tests/test_abi.py;
  * AUCMetric.update / AccuracyMetric.update with a mask against the brute-force counts of tests/esmm_ref.py over several batches,
    one with no row selected and one whose mask holds NaN; merge carries the mask; metrics.group_auc takes none;
  * EvalAccumulator.serves: a CPU spec is never served, with or without a mask; evaluate() on a CPU store returns the masked
    values of the host loop."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import esmm_ref as R
from tests import metrics_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_maskmetrics.h")
NAME = "recalgo_maskmetrics.h"
DECLARED = ["recalgo_maskmetrics_abi_version", "recalgo_maskmetrics_state_bytes", "recalgo_maskmetrics_update"]
LAUNCHES = ["recalgo_maskmetrics_update"]
FAKE = 0x10000           # a non-NULL, 16-byte aligned address: the refusals below happen before anything is read through it


def _table(abi, slots, struct="recalgo_maskmetrics_slot_t"):
    """slots: [dict(field=value)] over a valid masked AUC(200) slot at fake addresses"""
    Slot = abi.structs[struct]
    t = (Slot * max(len(slots), 1))()
    for i, over in enumerate(slots):
        d = dict(labels=FAKE, predictions=FAKE, thresholds=FAKE, kind=MR.AUC, num_thresholds=200, label_step=1, prediction_step=1,
                 mask=FAKE, mask_step=1)
        d.update(over)
        for k, v in d.items():
            setattr(t[i], k, v)
    return t


def test_header_literal_expectations():
    from recalgorithm_amd import _lib, build
    build.build(verbose=False)
    abi, old = _lib.SERVING_HEADERS[NAME], _lib.SERVING_HEADERS["recalgo_metrics.h"]
    assert list(abi.functions) == DECLARED and abi.launches == LAUNCHES and list(abi.structs) == ["recalgo_maskmetrics_slot_t"]
    lib = _lib.load()
    assert lib.recalgo_maskmetrics_abi_version() == abi.version == 1 and abi.label == "MASKMETRICS ABI"
    c_int, c_int64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    F = abi.functions
    assert F["recalgo_maskmetrics_abi_version"] == (c_int, []) and F["recalgo_maskmetrics_state_bytes"] == (c_int64, [ptr, c_int])
    assert F["recalgo_maskmetrics_update"] == (c_int, [ptr, c_int, ptr, c_int, ptr, ptr]) == old.functions["recalgo_metrics_update"]
    fields = abi.structs["recalgo_maskmetrics_slot_t"]._fields_
    assert fields == [("labels", ptr), ("predictions", ptr), ("thresholds", ptr), ("kind", c_int), ("num_thresholds", c_int),
                      ("label_step", c_int), ("prediction_step", c_int), ("mask", ptr), ("mask_step", c_int)]
    # recalgo_metrics_slot_t's fields, type for type, the two strides under their `_step` names, then the mask
    assert [(n.replace("_stride", "_step"), t) for n, t in old.structs["recalgo_metrics_slot_t"]._fields_] == fields[:7]
    assert ctypes.sizeof(abi.structs["recalgo_maskmetrics_slot_t"]) == 56
    text = open(HEADER).read()
    assert not re.search(r"\b(ld\w*|\w+_stride|\w+_col)\s*[;,)]", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RECALGO_MASKMETRICS_\w+) (0x[0-9A-Fa-f]+|\d+)", text)
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_MASKMETRICS_ABI_VERSION": 1, "RECALGO_MASKMETRICS_MAX_SLOTS": 16,
                                        "RECALGO_MASKMETRICS_MAX_THRESHOLDS": 1024, "RECALGO_MASKMETRICS_AUC": 0,
                                        "RECALGO_MASKMETRICS_ACCURACY": 1}
    assert {k.replace("MASKMETRICS", "METRICS"): v for k, v in abi.constants.items()} == old.constants

    # the state-size query (host side): recalgo_metrics.h's layout, each limit and one past it; the mask changes nothing
    size = lambda slots: lib.recalgo_maskmetrics_state_bytes(_table(abi, slots), len(slots))
    assert size([{}]) == 8 * (2 + 2 * 201) == 8 * MR.state_words([(MR.AUC, 200)]) == size([dict(mask=None)])
    assert size([dict(kind=MR.ACCURACY)]) == 8 * 4
    six = [{}, dict(kind=MR.ACCURACY), dict(num_thresholds=2, mask=None), dict(kind=MR.ACCURACY, mask=None), dict(num_thresholds=1024),
           dict(kind=MR.ACCURACY)]
    assert size(six) == 8 * MR.state_words([(MR.AUC, 200), (MR.ACCURACY, None), (MR.AUC, 2), (MR.ACCURACY, None), (MR.AUC, 1024),
                                            (MR.ACCURACY, None)])
    unmasked = (old.structs["recalgo_metrics_slot_t"] * 6)()
    for s, over in zip(unmasked, six):
        s.kind, s.num_thresholds = over.get("kind", MR.AUC), over.get("num_thresholds", 200)
    assert size(six) == lib.recalgo_metrics_state_bytes(unmasked, 6)
    assert [size([dict(num_thresholds=N)]) for N in (1, 2, 1024, 1025)] == [0, 8 * 8, 8 * 2052, 0]
    assert size([]) == 0 and size([{}] * 16) == 8 * (2 + 16 * 402) and size([{}] * 17) == 0
    assert size([dict(kind=2)]) == 0 and size([dict(kind=-1)]) == 0 and lib.recalgo_maskmetrics_state_bytes(None, 1) == 0

    # every refusal returns hipErrorInvalidValue through the errcheck, before any launch (fake addresses: nothing is read)
    refused = pytest.raises(_lib.RecalgoError, match="recalgo_maskmetrics_update failed with hipError_t=1$")

    def update(slots, n_slots=None, loss=None, n=64, state=FAKE):
        t = None if slots is None else _table(abi, slots)
        return lib.recalgo_maskmetrics_update(t, len(slots) if n_slots is None else n_slots, loss, n, state, None)
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
    for field in ("labels", "predictions", "thresholds", "mask"):
        for off in (1, 2, 3):
            with refused:
                update([{field: FAKE + off}])
    for bad in (dict(kind=2), dict(label_step=0), dict(prediction_step=0), dict(prediction_step=-3), dict(mask_step=0), dict(mask_step=-1)):
        with refused:
            update([bad])
        with refused:
            update([dict(mask=None), bad])     # any slot
    for off in (1, 2, 4, 7):
        with refused:
            update([{}], state=FAKE + off)
    for off in (1, 2, 3):
        with refused:
            update([{}], loss=FAKE + off)
    with refused:
        update([dict(kind=MR.ACCURACY, thresholds=None), dict(kind=MR.ACCURACY, labels=None)])


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
    assert _abi.read_record(NAME) == {1: _abi.declaration_hash(NAME)}, "include/recalgo_maskmetrics.abi records version 1's hash"


# ---- the host metrics with a mask ------------------------------------------------------------------------------------------------
def _batches(N, sizes=(257, 64, 1, 300), seed=3):
    """[(labels, predictions, mask)] float32: masks 30 %, all zeros (no row selected), one row, and one holding NaN"""
    th = MR.thresholds(N)
    kinds = ["30 %", "zeros", "ones", "nan"]
    out = []
    for i, (n, kind) in enumerate(zip(sizes, kinds)):
        labels, p = MR.batch(n, th, seed + i)
        out.append((labels, p, R.mask_kinds(n, seed + i)[kind]))
    return th, out


@pytest.mark.parametrize("N", [2, 200])
def test_the_masked_auc_update_counts_what_brute_force_counts(N):
    from recalgorithm_amd.estimator import AUCMetric, metrics
    th, batches = _batches(N)
    m, same = metrics.auc(None, None, num_thresholds=N, mask=None)
    assert m is same and type(m) is AUCMetric and m.mask is None
    plain = AUCMetric(None, None, N)
    hist = np.zeros((2, N + 1), np.int64)
    for labels, p, mask in batches:
        m.labels, m.predictions, m.mask = (torch.from_numpy(t).reshape(-1, 1) for t in (labels, p, mask))
        m.update()
        plain.labels, plain.predictions = m.labels, m.predictions
        plain.update()
        hist += R.masked_hist(labels, p, th, mask)
    assert np.isnan(batches[3][2]).any() and not batches[1][2].any()
    part = sum(int(R.takes_part(mask, len(mask)).sum()) for _, _, mask in batches)
    assert 0 < part == hist.sum() < sum(len(b[0]) for b in batches)
    above = hist[:, ::-1].cumsum(1)[:, ::-1][:, 1:]             # above[y][j] = sum over bin > j of hist[y][bin]
    total = hist.sum(1, keepdims=True)
    want = np.stack([above[1], above[0], (total - above)[1], (total - above)[0]]).astype(np.float64)
    assert np.array_equal(MR.host_counts(m).numpy(), want), "tp, fp, fn, tn"
    assert not np.array_equal(MR.host_counts(plain).numpy(), want), "the mask changes the counts"
    assert 0.0 <= m.result() <= 1.0


def test_the_masked_accuracy_update_counts_what_brute_force_counts():
    from recalgorithm_amd.estimator import AccuracyMetric, metrics
    _, batches = _batches(200)
    m, same = metrics.accuracy(None, None, mask=None)
    assert m is same and type(m) is AccuracyMetric and m.mask is None
    correct = total = 0
    for labels, p, mask in batches:
        hard = (p >= 0.5).astype(np.float32)
        m.labels, m.predictions, m.mask = (torch.from_numpy(t).reshape(-1, 1) for t in (labels, hard, mask))
        m.update()
        c, t = R.masked_accuracy(labels, hard, mask)
        correct, total = correct + c, total + t
    assert (m.correct, m.total) == (float(correct), float(total)) and 0 < correct < total
    assert m.result() == correct / total
    # no row selected at all: 0 / max(0, 1)
    e = AccuracyMetric(torch.ones(5, 1), torch.ones(5, 1), torch.zeros(5, 1))
    e.update()
    assert (e.correct, e.total, e.result()) == (0.0, 0.0, 0.0)
    e = AccuracyMetric(torch.ones(3), torch.ones(3), torch.tensor([float("nan"), 0.5, 0.50000006]))
    e.update()
    assert (e.correct, e.total) == (1.0, 1.0), "NaN and 0.5 take no part, the next float32 does"


def test_merge_carries_the_mask_and_group_auc_has_none():
    from recalgorithm_amd.estimator import AccuracyMetric, AUCMetric, metrics
    mask = torch.ones(4, 1)
    for cls in (AUCMetric, AccuracyMetric):
        first, later = cls(None, None), cls(torch.zeros(4, 1), torch.zeros(4, 1), mask=mask)
        first.merge(later)
        assert first.mask is mask and first.labels is later.labels
    assert list(inspect.signature(metrics.auc).parameters) == ["labels", "predictions", "num_thresholds", "mask"]
    assert list(inspect.signature(metrics.accuracy).parameters) == ["labels", "predictions", "mask"]
    assert "mask" not in inspect.signature(metrics.group_auc).parameters


def test_a_cpu_spec_is_not_served_and_the_host_loop_applies_the_mask():
    from recalgorithm_amd import estimator as E
    from recalgorithm_amd.variables import get_variable
    y, p, mask = torch.zeros(4, 1), torch.zeros(4, 1), torch.ones(4, 1)
    spec = E.EstimatorSpec("eval", loss=torch.zeros(()), eval_metric_ops={"a": E.metrics.auc(y, p, mask=mask), "b": E.metrics.accuracy(y, p)})
    assert E.EvalAccumulator.serves(spec, "cuda") is False and E.EvalAccumulator.of(spec, "cuda") is None

    def model_fn(features, labels, mode, params):
        w = get_variable("w", [4, 1])
        prob = torch.sigmoid(features["x"] @ w.data)
        c, click = labels["follow"], labels["click_avatar"]
        hard = (prob >= 0.5).float()
        return E.EstimatorSpec(mode, loss=prob.mean(), eval_metric_ops={
            "auc": E.metrics.auc(c, prob), "masked_auc": E.metrics.auc(c, prob, mask=click),
            "accuracy": E.metrics.accuracy(c, hard), "masked_accuracy": E.metrics.accuracy(c, hard, mask=click)})
    g = torch.Generator().manual_seed(5)
    batches = [({"x": torch.randn(n, 4, generator=g)}, {"follow": (torch.rand(n, 1, generator=g) < 0.4).float(),
                                                        "click_avatar": (torch.rand(n, 1, generator=g) < 0.3).float()}) for n in (48, 48, 21)]
    est = E.Estimator(model_fn, {"learning_rate": 0.01}, E.RunConfig(device="cpu", seed=3, use_hip_graph=False))
    out = est.evaluate(lambda: iter(batches))
    assert list(out) == ["auc", "masked_auc", "accuracy", "masked_accuracy", "loss", "global_step"]
    w = est.store.vars["w"].data
    prob = torch.cat([torch.sigmoid(f["x"] @ w) for f, _ in batches]).reshape(-1)
    c = torch.cat([l["follow"] for _, l in batches]).reshape(-1)
    click = torch.cat([l["click_avatar"] for _, l in batches]).reshape(-1) > 0.5
    sub = E.AUCMetric(c[click], prob[click])
    sub.update()
    assert out["masked_auc"] == sub.result() != out["auc"]
    hard = (prob >= 0.5).float()
    assert out["masked_accuracy"] == float((hard == c)[click].sum()) / float(click.sum()) != out["accuracy"]
