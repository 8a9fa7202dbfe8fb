"""CPU: the per-group AUC (uAUC / GAUC) without a GPU.
  * include/recalgo_gauc.h literally: names, signatures, the column struct, constants, both size queries at the documented layout,
    at each limit and one past it, every refusal before any launch; its place in _lib's header tables and every per-header check
    of tests/test_abi.py;
  * GroupAUCMetric over several update() calls against tests/gauc_ref.py's brute-force restatement: the integers exactly, both
    weightings as the floats of the one shared function; each valid group against sklearn's roc_auc_score to 1e-12 (the two differ
    by a handful of float64 roundings per group, each <= 2**-52); the edge semantics one by one;
  * evaluate() on a CPU store: with params["group_auc_key"] the host loop returns eval_uauc over all batches, without it exactly
    the keys it returned before; the params and flag plumbing, RunConfig(group_auc_capacity=), the ValueErrors of the tails."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import gauc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_gauc.h")
NAME = "recalgo_gauc.h"

DECLARED = ["recalgo_gauc_abi_version", "recalgo_gauc_state_bytes", "recalgo_gauc_workspace_bytes", "recalgo_gauc_append",
            "recalgo_gauc_finish"]
LAUNCHES = ["recalgo_gauc_append", "recalgo_gauc_finish"]
FAKE = 0x10000           # a non-NULL, 16-byte aligned address: the refusals below happen before anything is read through it
MAX_G, MAX_C = 1 << 24, 1 << 28


def _columns(abi, cols):
    """cols: [dict(field=value)] over a valid column at fake addresses"""
    Column = abi.structs["recalgo_gauc_column_t"]
    t = (Column * max(len(cols), 1))()
    for i, over in enumerate(cols):
        d = dict(labels=FAKE, predictions=FAKE, label_step=1, prediction_step=1)
        d.update(over)
        for k, v in d.items():
            setattr(t[i], k, v)
    return t


def _pad(v, m):
    return (v + m - 1) // m * m


def state_bytes(G, T, C):
    return _pad(64 + _pad(C, 4) * (5 + 4 * T), 8)


def workspace_bytes(G, T, C):
    Gp = _pad(G, 256)
    return _pad(4 * (3 * Gp + _pad(Gp // 256, 256) + 256) + _pad(C, 4) * (5 + 4 * T), 8)


def test_header_literal_expectations():
    from recalgorithm_amd import _lib, build, ops
    build.build(verbose=False)
    abi = _lib.SERVING_HEADERS[NAME]
    assert list(abi.functions) == DECLARED and abi.launches == LAUNCHES and list(abi.structs) == ["recalgo_gauc_column_t"]
    lib = _lib.load()
    assert lib.recalgo_gauc_abi_version() == abi.version == 1 and abi.label == "GAUC ABI"
    c_int, c_int64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    F = abi.functions
    assert F["recalgo_gauc_abi_version"] == (c_int, [])
    assert F["recalgo_gauc_state_bytes"] == F["recalgo_gauc_workspace_bytes"] == (c_int64, [c_int, c_int, c_int])
    assert F["recalgo_gauc_append"] == (c_int, [ptr, c_int, ptr, c_int, c_int, c_int, c_int, ptr, ptr])
    assert F["recalgo_gauc_finish"] == (c_int, [ptr, c_int, c_int, c_int, ptr, ptr, ptr])
    assert abi.structs["recalgo_gauc_column_t"]._fields_ == [("labels", ptr), ("predictions", ptr), ("label_step", c_int),
                                                            ("prediction_step", c_int)]
    assert ctypes.sizeof(abi.structs["recalgo_gauc_column_t"]) == 24
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RECALGO_GAUC_\w+) (0x[0-9A-Fa-f]+|\d+)", open(HEADER).read())
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_GAUC_ABI_VERSION": 1, "RECALGO_GAUC_MAX_TASKS": 8, "RECALGO_GAUC_MAX_GROUPS": MAX_G,
                                        "RECALGO_GAUC_MAX_ROWS": MAX_C, "RECALGO_GAUC_STATE_HEADER_WORDS": 8,
                                        "RECALGO_GAUC_RESULT_HEADER_WORDS": 3}
    assert (ops.GAUC_MAX_TASKS, ops.GAUC_MAX_GROUPS, ops.GAUC_MAX_ROWS) == (8, MAX_G, MAX_C)
    assert MAX_G < 2 ** 31 and MAX_C < 2 ** 31, "a group id and a log position are int32"

    # the size queries (host side): the documented layout, each limit and one past it
    shapes = [(1, 1, 1), (7, 3, 4099), (1000, 8, 12297), (70001, 1, 5), (20000, 3, 1 << 22), (MAX_G, 8, MAX_C), (257, 2, 3)]
    for G, T, C in shapes:
        assert lib.recalgo_gauc_state_bytes(G, T, C) == state_bytes(G, T, C), (G, T, C)
        assert lib.recalgo_gauc_workspace_bytes(G, T, C) == workspace_bytes(G, T, C), (G, T, C)
        assert ops.gauc_shape_ok(G, T, C)
    assert state_bytes(1, 1, 1) == 64 + 4 * 9 + 4 and state_bytes(20000, 1, 1 << 22) == 64 + 9 * (1 << 22)
    for G, T, C in [(0, 1, 1), (MAX_G + 1, 1, 1), (1, 0, 1), (1, 9, 1), (1, 1, 0), (1, 1, MAX_C + 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1)]:
        assert lib.recalgo_gauc_state_bytes(G, T, C) == 0 and lib.recalgo_gauc_workspace_bytes(G, T, C) == 0, (G, T, C)
        assert not ops.gauc_shape_ok(G, T, C)
    assert not ops.gauc_shape_ok(True, 1, 1) and not ops.gauc_shape_ok(1.0, 1, 1)

    # every refusal returns hipErrorInvalidValue through the errcheck, before any launch (fake addresses: nothing is read)
    refused_append = pytest.raises(_lib.RecalgoError, match="recalgo_gauc_append failed with hipError_t=1$")
    refused_finish = pytest.raises(_lib.RecalgoError, match="recalgo_gauc_finish failed with hipError_t=1$")

    def append(cols=({},), T=None, groups=FAKE, group_step=1, n=64, G=100, C=1000, state=FAKE):
        t = None if cols is None else _columns(abi, list(cols))
        return lib.recalgo_gauc_append(groups, group_step, t, len(cols) if T is None else T, n, G, C, state, None)

    def finish(state=FAKE, G=100, T=1, C=1000, result=FAKE, workspace=FAKE):
        return lib.recalgo_gauc_finish(state, G, T, C, result, workspace, None)
    for bad in (dict(n=0), dict(n=-1), dict(cols=[{}] * 9, T=0), dict(cols=[{}] * 9, T=9), dict(cols=[{}] * 9, T=-1), dict(G=0), dict(G=MAX_G + 1),
                dict(C=0), dict(C=MAX_C + 1), dict(groups=None), dict(cols=None, T=1), dict(state=None), dict(group_step=0),
                dict(group_step=-5)):
        with refused_append:
            append(**bad)
    for field in ("labels", "predictions"):
        with refused_append:
            append(cols=[{}, {field: None}])
        for off in (1, 2, 3):
            with refused_append:
                append(cols=[{field: FAKE + off}])
    for bad in (dict(label_step=0), dict(prediction_step=0), dict(prediction_step=-3), dict(label_step=-1)):
        with refused_append:
            append(cols=[{}, {}, bad])
    for off in (1, 2, 4, 7):
        with refused_append:
            append(groups=FAKE + off)
        with refused_append:
            append(state=FAKE + off)
        for which in ("state", "result", "workspace"):
            with refused_finish:
                finish(**{which: FAKE + off})
    for bad in (dict(G=0), dict(G=MAX_G + 1), dict(T=0), dict(T=9), dict(C=0), dict(C=MAX_C + 1), dict(state=None), dict(result=None),
                dict(workspace=None)):
        with refused_finish:
            finish(**bad)


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
    assert _abi.read_record(NAME) == {1: _abi.declaration_hash(NAME)}, "include/recalgo_gauc.abi records version 1's hash"


# ---- GroupAUCMetric against the restatement ---------------------------------------------------------------------------------------
G_ZIPF, SIZES = 1000, (4099, 4099, 4099)


def _metric(batches, G, weighting="uniform", t=0):
    from recalgorithm_amd.estimator import GroupAUCMetric
    m = GroupAUCMetric(None, None, None, G, weighting)
    for groups, labels, p in batches:
        m.groups = torch.from_numpy(groups)
        m.labels, m.predictions = torch.from_numpy(labels[:, t:t + 1]), torch.from_numpy(p[:, t:t + 1])
        m.update()
    return m


def _cat(batches, t=0):
    return (np.concatenate([b[0] for b in batches]), np.concatenate([b[1][:, t] for b in batches]), np.concatenate([b[2][:, t] for b in batches]))


@pytest.fixture(scope="module")
def zipf():
    batches = [R.batch(n, G_ZIPF, seed=s) for s, n in enumerate(SIZES)]
    return batches, R.counts(*_cat(batches), G_ZIPF)


def test_the_generated_input_has_every_kind_of_group(zipf):
    _, (num2, pos, neg, skipped) = zipf
    valid, empty, lonely = R.kinds(pos, neg)
    assert valid > 0 and empty > 0 and lonely > 0 and valid + empty + lonely == G_ZIPF and skipped > 0
    assert (pos + neg).max() > 1000, "a head that is far heavier than the rest"
    assert int((pos + neg).sum()) + skipped == sum(SIZES)


@pytest.mark.parametrize("weighting", ["uniform", "samples"])
def test_the_host_metric_equals_the_restatement(zipf, weighting):
    from recalgorithm_amd.estimator import group_auc_value
    batches, (num2, pos, neg, skipped) = zipf
    m = _metric(batches, G_ZIPF, weighting)
    got = m.result()
    assert all(a.dtype == np.int64 for a in (m.num2, m.pos, m.neg))
    assert np.array_equal(m.num2, num2) and np.array_equal(m.pos, pos) and np.array_equal(m.neg, neg) and m.skipped_rows == skipped
    want, valid = group_auc_value(num2, pos, neg, weighting)
    assert isinstance(got, float) and got == want and m.valid_groups == valid == R.kinds(pos, neg)[0], "the one shared function"
    assert abs(got - R.value(num2, pos, neg, weighting)) <= 1e-12 and 0.0 < got < 1.0
    assert m.result() == got, "result() twice"
    other = group_auc_value(num2, pos, neg, "samples" if weighting == "uniform" else "uniform")[0]
    assert other != got, "the two weightings differ on this input"


def test_each_valid_group_agrees_with_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    groups, labels, p = R.batch(12297, G_ZIPF, seed=9, edges=False)              # finite predictions, ties among them
    num2, pos, neg, _ = R.counts(groups, labels[:, 0], p[:, 0], G_ZIPF)
    y = labels[:, 0] > 0.5
    checked = 0
    for u in np.nonzero(pos * neg > 0)[0]:
        rows = groups == u
        ours = num2[u] / (2.0 * pos[u] * neg[u])
        assert abs(ours - sk.roc_auc_score(y[rows], p[rows, 0].astype(np.float64))) <= 1e-12, u
        checked += 1
    assert checked > 100


def _one_group(labels, p, G=1, groups=None):
    labels, p = np.asarray(labels, np.float32), np.asarray(p, np.float32)
    groups = np.zeros(len(p), np.int64) if groups is None else np.asarray(groups, np.int64)
    m = _metric([(groups, labels.reshape(-1, 1), p.reshape(-1, 1))], G)
    value = m.result()
    want = R.counts(groups, labels, p, G)
    assert [a.tolist() for a in (m.num2, m.pos, m.neg)] + [m.skipped_rows] == [a.tolist() for a in want[:3]] + [want[3]]
    return m, value


def test_edge_semantics_one_by_one():
    nan, inf = float("nan"), float("inf")
    # a NaN adds 0 against every partner, as a positive and as a negative
    m, v = _one_group([1, 0, 0], [nan, 0.1, 0.9])
    assert (m.num2[0], m.pos[0], m.neg[0], v) == (0, 1, 2, 0.0)
    m, v = _one_group([1, 1, 0], [0.1, 0.9, nan])
    assert (m.num2[0], v) == (0, 0.0)
    m, v = _one_group([1, 0], [nan, nan])
    assert (m.num2[0], v) == (0, 0.0)
    # +-inf order as usual, and tie with themselves
    m, v = _one_group([1, 1, 0, 0], [inf, -inf, inf, -inf])
    assert (m.num2[0], v) == (2 + 1 + 0 + 1, 0.5)
    m, v = _one_group([1, 0, 0], [inf, 3.0e38, -inf])
    assert (m.num2[0], v) == (4, 1.0)
    # -0.0 ties with 0.0
    m, v = _one_group([1, 0], [-0.0, 0.0])
    assert (m.num2[0], v) == (1, 0.5)
    m, v = _one_group([1, 0], [0.0, -0.0])
    assert (m.num2[0], v) == (1, 0.5)
    # a label of 0.5 is a negative, its float32 successor a positive
    m, v = _one_group([0.50000006, 0.5], [0.9, 0.1])
    assert (m.num2[0], m.pos[0], m.neg[0], v) == (2, 1, 1, 1.0)
    m, v = _one_group([0.5, 0.5, 1.0], [0.9, 0.1, 0.5])
    assert (m.pos[0], m.neg[0], m.num2[0], v) == (1, 2, 2, 0.5)
    # only positives, only negatives, an empty group: none of them valid, and the valid one alone is the mean
    m, v = _one_group([1, 1, 0, 0, 1, 0], [0.3, 0.4, 0.1, 0.2, 0.7, 0.6], G=5, groups=[0, 0, 1, 1, 3, 3])
    assert m.pos.tolist() == [2, 0, 0, 1, 0] and m.neg.tolist() == [0, 2, 0, 1, 0] and m.num2.tolist() == [0, 0, 0, 2, 0]
    assert (m.valid_groups, v) == (1, 1.0)
    # ids -1 and G belong to no group
    m, v = _one_group([1, 0, 1, 0], [0.9, 0.1, 0.2, 0.8], G=2, groups=[-1, 2, 1, 1])
    assert (m.skipped_rows, m.pos.tolist(), m.neg.tolist(), m.num2.tolist(), v) == (2, [0, 1], [0, 1], [0, 0], 0.0)
    # no valid group at all: 0.0, for both weightings, and for no row at all
    from recalgorithm_amd.estimator import GroupAUCMetric, group_auc_value
    m, v = _one_group([1, 0, 1], [0.5, 0.5, 0.5], G=3, groups=[0, 1, 2])
    assert (m.valid_groups, v) == (0, 0.0) and group_auc_value(m.num2, m.pos, m.neg, "samples") == (0.0, 0)
    assert GroupAUCMetric(None, None, None, 4).result() == 0.0
    # the two weightings on two valid groups of different size: (1 + 0.5) / 2 against (2 * 1 + 4 * 0.5) / 6
    m, v = _one_group([1, 0, 1, 0, 0, 0], [0.9, 0.1, 0.5, 0.5, 0.9, 0.1], G=2, groups=[0, 0, 1, 1, 1, 1])
    assert m.num2.tolist() == [2, 3] and v == 0.75
    assert group_auc_value(m.num2, m.pos, m.neg, "samples") == ((2 * 1.0 + 4 * 0.5) / 6, 2)
    for bad in (dict(weighting="mean"), dict(num_groups=0), dict(num_groups=True), dict(num_groups=2.0)):
        with pytest.raises(ValueError, match="group_auc"):
            GroupAUCMetric(None, None, None, **{"num_groups": 3, **bad})
    with pytest.raises(ValueError, match="weighting"):
        group_auc_value(m.num2, m.pos, m.neg, "mean")


# ---- evaluate() on a CPU store --------------------------------------------------------------------------------------------------
def _cpu_model_fn(features, labels, mode, params):
    """the EVAL branch of model_tail.finish_model_fn with the loss in plain torch (its loss kernel needs a GPU)"""
    from recalgorithm_amd.estimator import EstimatorSpec, metrics
    from recalgorithm_amd.model_tail import group_auc_metric_ops
    from recalgorithm_amd.variables import get_variable
    w = get_variable("w", [4, 1])
    logit = features["x"] @ w.data
    y = labels["read_comment"]
    prob = torch.sigmoid(logit)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    return EstimatorSpec(mode, loss=loss, eval_metric_ops={"eval_accuracy": metrics.accuracy(labels=y, predictions=(prob >= 0.5).float()),
                                                           "eval_auc": metrics.auc(labels=y, predictions=prob),
                                                           **group_auc_metric_ops(params, [(None, y, prob)])})


def _cpu_multitask_model_fn(features, labels, mode, params):
    from recalgorithm_amd.model_tail import group_auc_metric_ops
    from recalgorithm_amd.estimator import EstimatorSpec, metrics
    from recalgorithm_amd.variables import get_variable
    w = get_variable("w", [4, 2])
    prob = torch.sigmoid(features["x"] @ w.data)
    tasks = [(n, labels[n], prob[:, i:i + 1]) for i, n in enumerate(("read_comment", "like"))]
    ops_ = {f"eval_{n}_auc": metrics.auc(labels=y, predictions=p) for n, y, p in tasks}
    return EstimatorSpec(mode, loss=prob.mean(), eval_metric_ops={**ops_, **group_auc_metric_ops(params, tasks)})


def _cpu_batches(G=12):
    g = torch.Generator().manual_seed(5)
    out = []
    for n in (48, 48, 48, 21):
        ids = torch.randint(-1, G, (n,), generator=g)
        out.append(({"x": torch.randn(n, 4, generator=g), "userid": ids if n != 21 else ids.reshape(-1, 1)},
                    {"read_comment": (torch.rand(n, 1, generator=g) < 0.4).float(), "like": (torch.rand(n, 1, generator=g) < 0.5).float()}))
    return out


@pytest.mark.parametrize("weighting", [None, "uniform", "samples"])
def test_evaluate_on_a_cpu_store_returns_the_restatement(weighting):
    from recalgorithm_amd import estimator as E
    G, batches = 12, _cpu_batches(12)
    base = E.Estimator(_cpu_model_fn, {"learning_rate": 0.01}, E.RunConfig(device="cpu", seed=3, use_hip_graph=False))
    before = base.evaluate(lambda: iter(batches))
    assert list(before) == ["eval_accuracy", "eval_auc", "loss", "global_step"], "without the key: exactly the keys as before"
    params = {"learning_rate": 0.01, "group_auc_key": "userid", "group_auc_groups": G}
    if weighting is not None:
        params["group_auc_weighting"] = weighting
    est = E.Estimator(_cpu_model_fn, params, E.RunConfig(device="cpu", seed=3, use_hip_graph=False))
    out = est.evaluate(lambda: iter(batches))
    key = "eval_gauc" if weighting == "samples" else "eval_uauc"
    assert list(out) == ["eval_accuracy", "eval_auc", key, "loss", "global_step"]
    assert {k: v for k, v in out.items() if k != key} == before, "the other metrics are what they were"
    w = est.store.vars["w"].data
    prob = torch.cat([torch.sigmoid(f["x"] @ w) for f, _ in batches]).reshape(-1).numpy()
    ids = torch.cat([f["userid"].reshape(-1) for f, _ in batches]).numpy()
    y = torch.cat([l["read_comment"] for _, l in batches]).reshape(-1).numpy()
    num2, pos, neg, skipped = R.counts(ids, y, prob, G)
    assert R.kinds(pos, neg)[0] > 3 and skipped > 0
    assert out[key] == E.group_auc_value(num2, pos, neg, weighting or "uniform")[0]
    assert out == est.evaluate(lambda: iter(batches))
    assert est.evaluate(lambda: iter(()))  == {"loss": 0.0, "global_step": 0}


def test_the_multitask_keys_and_the_errors_of_the_tails():
    from recalgorithm_amd import estimator as E
    from recalgorithm_amd.feature_column import Ragged
    batches = _cpu_batches(12)
    params = {"group_auc_key": "userid", "group_auc_groups": 12, "group_auc_weighting": "samples"}
    out = E.Estimator(_cpu_multitask_model_fn, params, E.RunConfig(device="cpu", seed=3)).evaluate(lambda: iter(batches))
    assert list(out) == ["eval_read_comment_auc", "eval_like_auc", "eval_read_comment_gauc", "eval_like_gauc", "loss", "global_step"]
    assert out["eval_read_comment_gauc"] != out["eval_like_gauc"]

    def evaluate(params, batches=batches):
        return E.Estimator(_cpu_model_fn, {"learning_rate": 0.01, **params}, E.RunConfig(device="cpu", seed=3)).evaluate(lambda: iter(batches))
    with pytest.raises(ValueError, match="group_auc_key"):
        evaluate({"group_auc_key": "authorid", "group_auc_groups": 12})
    ragged = [({"x": f["x"], "userid": Ragged(f["userid"].reshape(-1), torch.arange(f["x"].shape[0] + 1))}, l) for f, l in batches]
    with pytest.raises(ValueError, match="group_auc_key.*Ragged"):
        evaluate({"group_auc_key": "userid", "group_auc_groups": 12}, ragged)
    with pytest.raises(ValueError, match="group_auc_key"):
        evaluate({"group_auc_key": "x", "group_auc_groups": 12})
    for bad in (None, 0, 2.5):
        with pytest.raises(ValueError, match="group_auc_groups"):
            evaluate({"group_auc_key": "userid", "group_auc_groups": bad})
    with pytest.raises(ValueError, match="weighting"):
        evaluate({"group_auc_key": "userid", "group_auc_groups": 12, "group_auc_weighting": "rows"})
    assert "eval_uauc" not in evaluate({"group_auc_key": "", "group_auc_groups": 12})


def test_the_capacity_of_run_config():
    from recalgorithm_amd import estimator as E
    assert E.RunConfig(device="cpu").group_auc_capacity == E.GROUP_AUC_CAPACITY == 1 << 22
    assert E.RunConfig(device="cpu", group_auc_capacity=1).group_auc_capacity == 1
    assert E.RunConfig(device="cpu", group_auc_capacity=MAX_C).group_auc_capacity == MAX_C
    for bad in (0, -1, MAX_C + 1, None, "auto", 2.0, True):
        with pytest.raises(ValueError, match="group_auc_capacity"):
            E.RunConfig(device="cpu", group_auc_capacity=bad)


def test_a_spec_the_accumulator_does_not_serve_stays_on_the_host_loop():
    """CPU tensors are never served; the rules for group metrics themselves (one groups tensor, one num_groups, at most 8) are
    checked before any tensor is looked at on a device"""
    from recalgorithm_amd.estimator import EstimatorSpec, EvalAccumulator, metrics
    y, p, ids = torch.zeros(4, 1), torch.zeros(4, 1), torch.zeros(4, dtype=torch.int64)
    spec = EstimatorSpec("eval", loss=torch.zeros(()), eval_metric_ops={"a": metrics.auc(y, p), "u": metrics.group_auc(y, p, ids, 3)})
    assert EvalAccumulator.serves(spec, "cuda") is False and EvalAccumulator.of(spec, "cuda") is None


def test_the_flags_and_the_params_they_fill(tmp_path):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm import _common as C
    C.define_group_auc_flags()
    vocab = tmp_path / "userid.txt"
    vocab.write_text("".join(f"u{i}\n" for i in range(37)))
    user = fc.categorical_column_with_vocabulary_file("userid", str(vocab))
    bag = fc.sequence_categorical_column_with_vocabulary_file("tags", str(vocab))
    columns = [fc.numeric_column("d"), fc.embedding_column(bag, 4), fc.embedding_column(user, 8)]
    saved = dict(flags.FLAGS._overrides)
    try:
        flags.FLAGS._parse([])
        assert flags.FLAGS.group_auc_key == "" and flags.FLAGS.group_auc_weighting == "uniform"
        assert C.group_auc_params_from_flags(columns) == {}, "off by default"
        flags.FLAGS.group_auc_key = "userid"
        assert C.group_auc_params_from_flags(columns) == {"group_auc_key": "userid", "group_auc_groups": 37, "group_auc_weighting": "uniform"}
        assert C.group_auc_params_from_flags([fc.indicator_column(user)])["group_auc_groups"] == 37
        flags.FLAGS.group_auc_weighting = "samples"
        assert C.group_auc_params_from_flags([user])["group_auc_weighting"] == "samples"
        for key in ("tags", "d", "feedid"):
            flags.FLAGS.group_auc_key = key
            with pytest.raises(ValueError, match="group_auc_key"):
                C.group_auc_params_from_flags(columns)
        flags.FLAGS._overrides.clear()
        assert flags.FLAGS._parse(["--group_auc_key=userid", "--group_auc_weighting=samples"]) == []
        assert (flags.FLAGS.group_auc_key, flags.FLAGS.group_auc_weighting) == ("userid", "samples")
        with pytest.raises(SystemExit):
            flags.FLAGS._parse(["--group_auc_weighting=rows"])
    finally:
        flags.FLAGS._parse([])
        flags.FLAGS._overrides.clear()
        flags.FLAGS._overrides.update(saved)
