"""-m gpu: the per-group AUC kernels (include/recalgo_gauc.h) and evaluate() on them.

The kernels at the C ABI against tests/gauc_ref.py's brute-force restatement; the counts are integers, so every comparison is ==:
  * n per launch in {1, 63, 64, 65, 255, 256, 257, 4099} (wave and workgroup boundaries; a workgroup of the append owns 256
    rows), three launches accumulate, T in {1, 3, 8}; labels at stride 1, predictions as column 1 of an [n, 3] matrix, the group
    id as column 2 of an [n, 5] int64 matrix whose other columns hold other ids;
  * G in {1, 2, 7, 1000, 70 001}: the scan works in tiles of 256 groups and scans the tile sums 256 at a time, so 70 001
    (274 tiles) crosses both edges; 1000 crosses the first;
  * every row in one group (the skew case, 3 x 4099 rows, timed), every row its own group (no valid group), Zipf(1.1) over 1000
    groups with all three kinds of group present; ids -1 and G mixed in; half of the predictions tied, NaN, +-inf, -0.0 among them;
  * finish, append, finish again; the log unchanged by finish; capacity C = rows, rows - 1, and a batch that starts past C;
  * every refusal leaves state and result as they were; the whole run once more under tests/redzone.py;
  * one append captured in a graph and replayed 5 times over changing inputs equals 5 eager appends.

evaluate() on DCN, DeepFM and MMoE (3 tasks) with the fixture of tests/test_gpu_metrics.py and userid as the key over a
vocabulary of 12: host loop, device metrics eager and device metrics captured return the same dict; the integer arrays equal the
restatement over the host loop's own predictions; no Metric.update() on the device path, one recalgo_metrics_update and one
recalgo_gauc_append per eager batch and none for a replay; with the key unset the dict and the launches are the earlier ones;
a group_auc_capacity below the rows raises."""
import ctypes
import time

import numpy as np
import pytest
import torch

from recalgorithm_amd import _lib, ops
from recalgorithm_amd import estimator as E
from recalgorithm_amd.io import synth
from tests import gauc_ref as R
from tests.redzone import guarded
from tests.test_gpu_metrics import B, LAST, MODELS, N_FULL, _Counting

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 4099]
_ABI = _lib.SERVING_HEADERS["recalgo_gauc.h"]
_COLUMN = _ABI.structs["recalgo_gauc_column_t"]
HDR, RES = 8, 3


class Log:
    """The three buffers of one (G, T, C) on the device and the launches over host batches (R.batch's triples)."""

    def __init__(self, dev, G, T, C, place=None, empty=None):
        self.lib, self.dev, self.G, self.T, self.C = _lib.load(), dev, G, T, C
        self.place = place or (lambda t: t.to(dev))
        empty = empty or torch.empty
        self.state = empty(self.lib.recalgo_gauc_state_bytes(G, T, C) // 8, dtype=torch.int64, device=dev)
        self.state[:HDR] = 0
        self.workspace = empty(self.lib.recalgo_gauc_workspace_bytes(G, T, C) // 8, dtype=torch.int64, device=dev)
        self.result = empty(RES + 3 * T * G, dtype=torch.int64, device=dev)
        self.keep, self.rows = [], []

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def device_batch(self, groups, labels, p):
        """-> (ids [n, 5] with the groups in column 2, [labels [n] per task], [[n, 3] with the predictions in column 1 per task])"""
        n = len(groups)
        ids = np.stack([groups + 1, np.zeros(n, np.int64), groups, np.full(n, 3), groups[::-1]], axis=1).astype(np.int64)
        mats = [np.stack([1.0 - p[:, t], p[:, t], np.full(n, 0.5)], axis=1).astype(np.float32) for t in range(self.T)]
        return self.place(torch.from_numpy(ids)), [self.place(torch.from_numpy(labels[:, t].copy())) for t in range(self.T)], \
            [self.place(torch.from_numpy(m)) for m in mats]

    def table(self, dl, dm):
        table = (_COLUMN * self.T)()
        for t in range(self.T):
            table[t].labels, table[t].predictions = dl[t].data_ptr(), dm[t][:, 1].data_ptr()
            table[t].label_step, table[t].prediction_step = 1, 3
        return table

    def append(self, groups, labels, p):
        ids, dl, dm = self.device_batch(groups, labels, p)
        self.keep += [ids, dl, dm]
        self.lib.recalgo_gauc_append(ids[:, 2].data_ptr(), 5, self.table(dl, dm), self.T, len(groups), self.G, self.C,
                                     self.state.data_ptr(), self.stream())
        self.rows.append((groups, labels, p))
        return self

    def finish(self):
        self.lib.recalgo_gauc_finish(self.state.data_ptr(), self.G, self.T, self.C, self.result.data_ptr(), self.workspace.data_ptr(),
                                     self.stream())
        torch.cuda.synchronize()
        return self.result.cpu().numpy()

    def check(self, result, first=None):
        """result against the restatement over the first `first` rows appended (default: all of them, which must have fitted)"""
        groups, labels, p = (np.concatenate([b[k] for b in self.rows]) for k in range(3))
        total = len(groups)
        first = total if first is None else first
        num2, pos, neg = result[RES:].reshape(3, self.T, self.G)
        skipped = None
        for t in range(self.T):
            w2, wp, wn, skipped = R.counts(groups[:first], labels[:first, t], p[:first, t], self.G)
            assert np.array_equal(pos[t], wp) and np.array_equal(neg[t], wn), f"task {t}: pos, neg"
            assert np.array_equal(num2[t], w2), f"task {t}: num2"
        assert result[:RES].tolist() == [skipped, total - first, first], "skipped, dropped, rows"
        return num2, pos, neg


def _batches(n, G, T, shape="zipf", rounds=3, seed=0):
    return [R.batch(n, G, T, shape=shape, seed=10 * seed + r) for r in range(rounds)]


@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_three_appends_and_a_finish(dev, n, T):
    log = Log(dev, 7, T, 3 * n)
    for b in _batches(n, 7, T, seed=1):
        log.append(*b)
    log.check(log.finish())
    assert log.state[:HDR].tolist() == [3 * n, 0, 0, 0, 0, 0, 0, 0], "cursor, dropped, the ticket back at zero"


@pytest.mark.parametrize("G", [1, 2, 7, 1000, 70001])
def test_the_number_of_groups(dev, G):
    log = Log(dev, G, 1, 3 * 4099)
    for b in _batches(4099, G, 1, seed=2):
        log.append(*b)
    num2, pos, neg = log.check(log.finish())
    assert R.kinds(pos[0], neg[0])[0] > 0
    if G == 70001:
        assert np.nonzero(pos[0] + neg[0])[0].max() >= 256 * 256, "a group behind the first 256 tiles of the scan holds rows"


def test_zipf_has_every_kind_of_group(dev):
    log = Log(dev, 1000, 3, 3 * 4099)
    for b in _batches(4099, 1000, 3, seed=0):
        log.append(*b)
    num2, pos, neg = log.check(log.finish())
    for t in range(3):
        valid, empty, lonely = R.kinds(pos[t], neg[t])
        assert valid > 0 and empty > 0 and lonely > 0, "no case silently tests nothing"
    assert (pos[0] + neg[0]).max() > 1000


def test_every_row_in_one_group(dev):
    """the skew case: one group's pair work is spread over its rows"""
    log = Log(dev, 7, 1, 3 * 4099)
    for b in _batches(4099, 7, 1, shape="one", seed=3):
        log.append(*b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = log.finish()
    seconds = time.perf_counter() - t0
    num2, pos, neg = log.check(result)
    assert R.kinds(pos[0], neg[0]) == (1, 6, 0) and pos[0][3] * neg[0][3] > 1 << 24
    print(f"finish over {3 * 4099} rows of one group: {seconds * 1e3:.2f} ms")
    assert seconds < 0.5, "well under a second"


def test_every_row_its_own_group(dev):
    log = Log(dev, 1000, 3, 257)
    log.append(*R.batch(257, 1000, 3, shape="own", seed=4))
    num2, pos, neg = log.check(log.finish())
    assert not num2.any() and R.kinds(pos[0], neg[0])[0] == 0 and (pos + neg).max() == 1


def test_finish_twice_with_an_append_between(dev):
    log = Log(dev, 1000, 3, 4 * 4099)
    a, b, c = _batches(4099, 1000, 3, seed=5)
    log.append(*a).append(*b)
    log.check(log.finish())
    before = log.state.clone()
    again = log.finish()
    assert torch.equal(log.state, before), "finish leaves the header and the log as they are"
    log.check(again)
    log.append(*c)
    log.check(log.finish())
    whole = Log(dev, 1000, 3, 4 * 4099).append(*a).append(*b).append(*c)
    assert np.array_equal(whole.finish(), log.result.cpu().numpy())


def test_capacity(dev):
    n, G, T = 257, 7, 3
    rounds = _batches(n, G, T, seed=6)
    exact = Log(dev, G, T, 3 * n)
    for b in rounds:
        exact.append(*b)
    exact.check(exact.finish())
    short = Log(dev, G, T, 3 * n - 1)
    for b in rounds:
        short.append(*b)
    short.check(short.finish(), first=3 * n - 1)
    assert short.state[:3].tolist() == [3 * n, 1, 0]
    # a batch that starts past C drops all of its rows and writes nothing
    small = Log(dev, G, T, n + 5)
    small.append(*rounds[0]).append(*rounds[1])
    torch.cuda.synchronize()
    before = small.state.clone()
    small.append(*rounds[2])
    torch.cuda.synchronize()
    assert small.state[:3].tolist() == [3 * n, 2 * n - 5, 0] and torch.equal(small.state[HDR:], before[HDR:])
    small.check(small.finish(), first=n + 5)


def test_refusals_leave_state_and_result_untouched(dev):
    n, G, T, C = 65, 7, 3, 300
    log = Log(dev, G, T, C)
    log.append(*R.batch(n, G, T, seed=7))
    log.finish()
    state, result = log.state.clone(), log.result.clone()
    ids, dl, dm = log.device_batch(*R.batch(n, G, T, seed=8))
    refused = pytest.raises(_lib.RecalgoError, match="failed with hipError_t=1$")
    g, st, res, ws = ids[:, 2].data_ptr(), log.state.data_ptr(), log.result.data_ptr(), log.workspace.data_ptr()

    def append(groups=g, stride=5, table=True, T=T, n=n, G=G, C=C, state=st, **column):
        t = log.table(dl, dm) if table else None
        for k, v in column.items():
            setattr(t[1], k, v)
        with refused:
            log.lib.recalgo_gauc_append(groups, stride, t, T, n, G, C, state, log.stream())

    def finish(state=st, G=G, T=T, C=C, result=res, workspace=ws):
        with refused:
            log.lib.recalgo_gauc_finish(state, G, T, C, result, workspace, log.stream())
    for bad in (dict(n=0), dict(n=-1), dict(T=0), dict(T=9), dict(G=0), dict(G=ops.GAUC_MAX_GROUPS + 1), dict(C=0), dict(C=ops.GAUC_MAX_ROWS + 1),
                dict(groups=None), dict(table=False), dict(state=None), dict(stride=0), dict(labels=None), dict(predictions=None),
                dict(label_step=0), dict(prediction_step=-3), dict(labels=dl[1].data_ptr() + 2), dict(predictions=dm[1].data_ptr() + 1),
                dict(groups=g + 4), dict(state=st + 4)):
        append(**bad)
    for bad in (dict(G=0), dict(G=ops.GAUC_MAX_GROUPS + 1), dict(T=0), dict(T=9), dict(C=0), dict(C=ops.GAUC_MAX_ROWS + 1), dict(state=None),
                dict(result=None), dict(workspace=None), dict(state=st + 4), dict(result=res + 4), dict(workspace=ws + 4)):
        finish(**bad)
    torch.cuda.synchronize()
    assert torch.equal(log.state, state) and torch.equal(log.result, result)


@pytest.mark.parametrize("n,G,T", [(4099, 1000, 3), (65, 70001, 8)], ids=["zipf", "wide"])
def test_guarded(dev, n, G, T):
    """every input and the three buffers between 0xFF redzones, the buffers themselves poisoned: the counts are right, the redzones
    and the inputs untouched"""
    with guarded() as g:
        log = Log(dev, G, T, 3 * n + 1, place=lambda t: g.input(t, dev), empty=torch.empty)
        for b in _batches(n, G, T, seed=9):
            log.append(*b)
        result = log.finish()
        assert {"recalgo_gauc_append", "recalgo_gauc_finish"} <= g.launched and sum(r.kind == "empty" for r in g.records) == 3
    log.check(result)


def test_a_captured_append_replayed(dev):
    n, G, T = 257, 7, 3
    rounds = _batches(n, G, T, rounds=5, seed=10)
    eager = Log(dev, G, T, 5 * n)
    for b in rounds:
        eager.append(*b)
    want = eager.finish()
    log = Log(dev, G, T, 5 * n)
    ids, dl, dm = log.device_batch(*rounds[0])
    table = log.table(dl, dm)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        log.lib.recalgo_gauc_append(ids[:, 2].data_ptr(), 5, table, T, n, G, log.C, log.state.data_ptr(), log.stream())
    assert log.state[:HDR].tolist() == [0] * HDR, "capturing appends nothing"
    for b in rounds:
        new_ids, new_dl, new_dm = log.device_batch(*b)
        ids.copy_(new_ids)
        for t in range(T):
            dl[t].copy_(new_dl[t])
            dm[t].copy_(new_dm[t])
        graph.replay()
        log.rows.append(b)
    torch.cuda.synchronize()
    got = log.finish()
    log.check(got)
    assert np.array_equal(got, want) and log.state[:3].tolist() == [5 * n, 0, 0]


def test_the_ops_entries_are_those_launches(dev):
    """the Python entries on the model's tensors: [B, 1] column views of a [B, T] matrix, the ids as a column of the id matrix"""
    n, G, T = 300, 1000, 3
    st = ops.gauc_state(G, T, 2 * n, dev)
    assert (st.G, st.T, st.C) == (G, T, 2 * n) and st.state[:HDR].tolist() == [0] * HDR
    log = Log(dev, G, T, 2 * n)
    for b in _batches(n, G, T, rounds=2, seed=11):
        groups, labels, p = b
        ids = torch.from_numpy(np.stack([groups, groups + 1], axis=1)).to(dev)
        dl, dp = torch.from_numpy(labels).to(dev), torch.from_numpy(p).to(dev)
        ops.gauc_append(st, ids[:, 0], [(dl[:, t:t + 1], dp[:, t:t + 1]) for t in range(T)])
        log.append(*b)
    skipped, dropped, rows, num2, pos, neg = ops.gauc_counts(ops.gauc_finish(st), G, T)
    want = log.finish()
    assert [skipped, dropped, rows] == want[:RES].tolist() and np.array_equal(np.stack([num2, pos, neg]).reshape(-1), want[RES:])
    log.check(want)
    with pytest.raises(TypeError):
        ops.gauc_append(st, ids[:, 0].int(), [(dl[:, t:t + 1], dp[:, t:t + 1]) for t in range(T)])
    with pytest.raises(ValueError):
        ops.gauc_append(st, ids[:, 0], [(dl[:, :1], dp[:, :1])])
    with pytest.raises(ValueError):
        ops.gauc_state(G, 9, 10, dev)


# ---- evaluate() -----------------------------------------------------------------------------------------------------------------
USERS = 12
_shared = {}


def _instances(monkeypatch):
    """every GroupAUCMetric whose result() runs from here on, in order"""
    seen, real = [], E.GroupAUCMetric.result
    monkeypatch.setattr(E.GroupAUCMetric, "result", lambda self: (seen.append(self), real(self))[1])
    return seen


def _setup(name, dev):
    """(estimator with userid as the group key after three training steps, the six EVAL batches, the host loop's result, its
    group metrics, the task names): built once per model"""
    if name not in _shared:
        model_fn, params, spec, extra = MODELS[name](dev)
        spec.vocabs[spec.names.index("userid")] = USERS          # (the table keeps its rows: ids 0 .. 11 and -1 are valid for it)
        params = dict(params, group_auc_key="userid", group_auc_groups=USERS)
        est = E.Estimator(model_fn, params, E.RunConfig(device=dev, seed=3, use_hip_graph=False, device_metrics=False))
        sizes = [B] * N_FULL + [LAST]
        batches = [synth.device_features(spec, b, dev, batch_index=i, extra_labels=extra)[:2] for i, b in enumerate(sizes)]
        train = synth.device_features(spec, 256, dev, batch_index=50, extra_labels=extra)[:2]
        est.build(*train)
        for _ in range(3):
            est.train_step(*train)
        with pytest.MonkeyPatch.context() as mp:
            seen = _instances(mp)
            want = est.evaluate(lambda: iter(batches))
        tasks = ["read_comment"] + list(extra)
        keys = ["eval_uauc"] if not extra else [f"eval_{t}_uauc" for t in tasks]
        assert len(want) == 2 + 3 * len(tasks) and [k for k in want if k.endswith("uauc")] == keys and len(seen) == len(tasks)
        assert all(np.isfinite(v) for v in want.values())
        _shared[name] = (est, batches, want, seen, keys)
    return _shared[name]


def _evaluate(est, batches, monkeypatch, **run):
    """evaluate() under `run`, with Metric.update() forbidden -> (result, its group metrics, calls per entry)"""
    def forbidden(self):
        raise AssertionError("Metric.update() ran under device_metrics=True")
    for cls in (E.AUCMetric, E.AccuracyMetric, E.GroupAUCMetric):
        monkeypatch.setattr(cls, "update", forbidden)
    seen = _instances(monkeypatch)
    lib = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    for k, v in run.items():
        monkeypatch.setattr(est.config, k, v)
    out = est.evaluate(lambda: iter(batches))
    return out, seen, {k: lib.calls.get(k, 0) for k in ("recalgo_metrics_update", "recalgo_gauc_append", "recalgo_gauc_finish")}


@pytest.mark.parametrize("name", list(MODELS))
def test_the_host_loop_counts_are_the_restatement(dev, name):
    est, batches, want, host, keys = _setup(name, dev)
    for m, key in zip(host, keys):
        groups, y, p = (np.concatenate(c) for c in zip(*m._rows))
        assert len(groups) == B * N_FULL + LAST and p.dtype == np.float32
        num2, pos, neg, skipped = R.counts(groups, y.astype(np.float32), p, USERS)
        assert np.array_equal(m.num2, num2) and np.array_equal(m.pos, pos) and np.array_equal(m.neg, neg) and m.skipped_rows == skipped
        assert R.kinds(pos, neg)[0] >= 3 and skipped > 0 and m.valid_groups == R.kinds(pos, neg)[0]
        assert want[key] == E.group_auc_value(num2, pos, neg, "uniform")[0] and 0.0 <= want[key] <= 1.0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("name", list(MODELS))
def test_device_metrics_return_the_host_loops_dict(dev, name, graph, monkeypatch):
    est, batches, want, host, keys = _setup(name, dev)
    got, seen, calls = _evaluate(est, batches, monkeypatch, device_metrics=True, use_hip_graph=graph)
    assert got == want and list(got) == list(want)
    for m, h in zip(seen, host):
        assert np.array_equal(m.num2, h.num2) and np.array_equal(m.pos, h.pos) and np.array_equal(m.neg, h.neg)
        assert (m.skipped_rows, m.valid_groups) == (h.skipped_rows, h.valid_groups) and not m._rows
    # captured: batches 1 and 2 eager, batch 3 captured (one call, recorded) and replayed, 4 and 5 replays, the batch of 37 eager
    per_batch = 4 if graph else N_FULL + 1
    assert calls == {"recalgo_metrics_update": per_batch, "recalgo_gauc_append": per_batch, "recalgo_gauc_finish": 1}


@pytest.mark.parametrize("name", list(MODELS))
def test_with_the_key_unset_nothing_changes(dev, name, monkeypatch):
    est, batches, want, host, keys = _setup(name, dev)
    monkeypatch.setitem(est.params, "group_auc_key", "")
    plain = est.evaluate(lambda: iter(batches))
    assert plain == {k: v for k, v in want.items() if k not in keys} and len(plain) == len(want) - len(keys)
    for graph, per_batch in ((False, N_FULL + 1), (True, 4)):
        with pytest.MonkeyPatch.context() as mp:
            got, seen, calls = _evaluate(est, batches, mp, device_metrics=True, use_hip_graph=graph)
        assert got == plain and list(got) == list(plain) and seen == []
        assert calls == {"recalgo_metrics_update": per_batch, "recalgo_gauc_append": 0, "recalgo_gauc_finish": 0}


def test_a_capacity_below_the_rows_raises(dev, monkeypatch):
    est, batches, want, host, keys = _setup("dcn", dev)
    rows = B * N_FULL + LAST
    with pytest.raises(RuntimeError, match=f"group_auc_capacity = {rows - 57} rows, and 57 more rows were dropped"):
        _evaluate(est, batches, monkeypatch, device_metrics=True, use_hip_graph=True, group_auc_capacity=rows - 57)
    monkeypatch.undo()
    with pytest.MonkeyPatch.context() as mp:
        got, _, _ = _evaluate(est, batches, mp, device_metrics=True, use_hip_graph=False, group_auc_capacity=rows)
    assert got == want, "a capacity of exactly the rows serves them all"
