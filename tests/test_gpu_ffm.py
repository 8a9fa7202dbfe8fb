"""-m gpu: FFM's field-aware term as one kernel each way (include/recalgo_ffm.h, csrc/ffm.hip, ops.ffm_interaction) and what
follows from it — FFM's step over the reference's columns (six single-valued fields and the multi-hot manual_tag_list) is captured
and served from graphs.

  1. ops.ffm_bag_distinct against tests/ffm_ref.py, exact;
  2. the op against tests/ffm_ref.py at the bar tests/test_gpu_siblings.py::test_ffm_pairs holds the composed op to: the fp64
     restatement, ref32 from the fp32 one, reduced=True for `out`; gradients as the rows the scatter's sources receive and, through
     sparse.materialize_grads, as table gradients;
  3. strict equalities: g[b] * row bit for bit, zero rows for dropped entries, two runs, a padded Ragged;
  4. PREDICT between training steps reads lagging rows through the deferred view;
  5. once more under tests/redzone.py's guarded, poisoned allocations;
  6. dispatch;
  7. model_ffm on the golden's columns: captured TRAIN steps == eager steps bit for bit, captured EVAL == the host loop;
  8. serving from graphs."""
import numpy as np
import pytest
import torch

from recalgorithm_amd import export as E
from recalgorithm_amd import ops, sparse
from recalgorithm_amd.estimator import Estimator, RunConfig
from recalgorithm_amd.feature_column import Ragged
from recalgorithm_amd.variables import EmbeddingArena, VariableStore, use_store
from tests import ffm_ref as R
from tests import golden_util as GU
from tests import redzone
from tests.test_gpu_ragged import ORDER, _assert_same_run, _model, _nnz, _on_device, _steps, _to
from tests.test_gpu_serving import _same, exported, golden_records
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu


# ---- 1. the de-duplication ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 257])
def test_bag_distinct(dev, B):
    for seed in range(5 if B == 1 else 1):                       # (B = 1: one bag of every kind)
        values, offsets = R.make_bags(B, 9, seed=seed)
        nnz = len(values)
        for capacity in (nnz, nnz + 1, (nnz + 255) // 256 * 256 + 3):
            v = R.pad(values, capacity)
            want = R.distinct(v, offsets)
            got = ops.ffm_bag_distinct(torch.from_numpy(v).to(dev), torch.from_numpy(offsets).to(dev))
            assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.int32]
            for g, w, what in zip(got, want, ("values", "valid", "distinct")):
                assert np.array_equal(g.cpu().numpy(), w), (what, B, capacity)
            assert (got[0][nnz:] == -1).all() and (got[0].cpu().numpy()[:nnz][want[0][:nnz] < 0] == -1).all()
    kinds = R.distinct(*R.make_bags(5, 9, seed=0))
    assert kinds[1].tolist()[:4] == [0, 0, 3, 4] and kinds[2].tolist()[:4] == [0, 0, 1, 2] and kinds[1][4] == 70


# ---- the op on a problem of tests/ffm_ref.py --------------------------------------------------------------------------------------------
def _setup(dev, p, capacity=None, place=None):
    """-> (store, arena, table names, ids on the device, {field: Ragged on the device})"""
    place = place or (lambda t: t.to(dev))
    store = VariableStore(dev)
    store.opt_state = None
    arena = store.arenas["emb"] = EmbeddingArena("emb", p["K"], dev, seed=1)
    names = [f"t{i}" for i in range(p["F"])]
    for n, t in zip(names, p["tables"]):
        arena.add_table(n, t.shape[0] * t.shape[1], torch.from_numpy(t.reshape(-1, p["K"]).copy()))
    arena.materialize()
    ids = place(torch.from_numpy(p["ids"])) if p["single"] else None
    bags = {}
    for i, (values, offsets) in p["bags"].items():
        v = values if capacity is None else R.pad(values, capacity[i])
        bags[i] = Ragged(place(torch.from_numpy(v)), place(torch.from_numpy(offsets)))
    return store, arena, names, ids, bags


def _run(dev, p, fused=True, capacity=None, train=True, place=None):
    """-> (out [B] on the host, sources' gradient tensors [d_single, d_bag ...] or None, table gradients [F] or None)"""
    store, arena, names, ids, bags = _setup(dev, p, capacity, place)
    place = place or (lambda t: t.to(dev))
    with use_store(store):
        sparse.new_forward(store)
        if not train:
            with torch.no_grad():
                return ops.ffm_interaction(store, ids, bags, arena, names, p["vocab"], p["F"], p["K"], fused=fused).cpu().reshape(-1), None, None
        with torch.enable_grad():
            out = ops.ffm_interaction(store, ids, bags, arena, names, p["vocab"], p["F"], p["K"], fused=fused)
            out.backward(place(torch.from_numpy(p["g"])).reshape(-1, 1))
        srcs = [s.g.detach().cpu().clone() for s in sparse.plan_of(arena).sources if s.g is not None]
        sparse.materialize_grads(store)
        grads = [arena.grad[arena.tables[n][0]:arena.tables[n][0] + arena.tables[n][1]].cpu().reshape(t.shape)
                 for n, t in zip(names, p["tables"])]
        sparse.new_forward(store)
    return out.detach().cpu().reshape(-1), srcs, grads


SHAPES = [(1, 2, 4), (5, 3, 4), (5, 7, 8), (130, 7, 4), (5, 32, 4), (3, 4, 64), (33, 26, 16)]
BAG_FIELDS = {"none": lambda F: (), "first": lambda F: (0,), "middle": lambda F: (F // 2,), "last": lambda F: (F - 1,),
              "two adjacent": lambda F: (F // 2 - 1 if F > 2 else 0, F // 2 if F > 2 else 1)}


def _check(dev, p, **kw):
    out, srcs, grads = _run(dev, p, **kw)
    assert_close(out, torch.from_numpy(R.out(p)), what="ffm fused fwd", reduced=True, ref32=torch.from_numpy(R.out(p, np.float32)))
    (d1, db), (d1_32, db_32) = R.grad_rows(p), R.grad_rows(p, np.float32)
    want = ([d1] if p["single"] else []) + [db[i] for i in sorted(db) if len(db[i])]
    want32 = ([d1_32] if p["single"] else []) + [db_32[i] for i in sorted(db) if len(db[i])]
    assert len(srcs) == len(want), "ONE source for the single-valued requests, one per bag field"
    for k, (got, w, w32) in enumerate(zip(srcs, want, want32)):
        n = w.shape[0]
        assert_close(got[:n], torch.from_numpy(w), what=f"ffm fused bwd: rows of source {k}", ref32=torch.from_numpy(w32))
        assert not got[n:].any(), "the rows of a padded tail are zeros"
    for i, (got, w, w32) in enumerate(zip(grads, R.table_grads(p), R.table_grads(p, np.float32))):
        assert_close(got, torch.from_numpy(w), what=f"ffm fused bwd: table {i}", reduced=True, ref32=torch.from_numpy(w32))
    return out, srcs, grads


@pytest.mark.parametrize("where", list(BAG_FIELDS))
@pytest.mark.parametrize("B,F,K", SHAPES)
def test_the_op_against_the_reference(dev, B, F, K, where):
    p = R.problem(B, F, K, BAG_FIELDS[where](F), seed=3)
    assert p["ids"] is None or B == 1 or (p["ids"] < 0).any(), "OOV ids in the single-valued fields"
    _check(dev, p)


def test_every_field_a_bag(dev):
    _check(dev, R.problem(5, 3, 4, (0, 1, 2), seed=1))
    _check(dev, R.problem(9, 4, 8, (0, 1, 2, 3), seed=2))


# ---- 3. strict equalities -----------------------------------------------------------------------------------------------------------
def test_strict_equalities(dev):
    p = R.problem(33, 7, 8, (2, 3), seed=5)
    B, F, K = p["B"], p["F"], p["K"]
    out, srcs, grads = _run(dev, p)
    # a single-valued request whose partner is single-valued: g[b] * row, one fp32 product — recalgo_ffm_pairs_bwd's value too
    d1 = srcs[0].numpy().reshape(B, len(p["single"]), F - 1, K)
    v32 = R.rows(p, np.float32)
    checked = 0
    for c, a in enumerate(p["single"]):
        for s in range(F - 1):
            pa, ps = R.partner(a, s)
            if pa in p["bags"]:
                continue
            want = p["g"][:, None] * v32[:, pa, ps]
            assert np.array_equal(d1[:, c, s].view(np.uint32), want.astype(np.float32).view(np.uint32)), (a, s)
            checked += 1
    assert checked == len(p["single"]) * (F - 1 - 2)
    # rows of dropped bag entries are exactly zero
    for k, i in enumerate(sorted(p["bags"])):
        kept = R.distinct(*p["bags"][i])[0]
        rows = srcs[1 + k].numpy()
        assert (kept < 0).any() and not rows[kept < 0].any() and rows[kept >= 0].any(axis=1).all()
    # two runs: identical bits
    again = _run(dev, p)
    assert_bit_exact(again[0], out, "second run: out")
    for a, b in zip(again[1] + again[2], srcs + grads):
        assert_bit_exact(a, b, "second run: gradients")
    # a padded Ragged: the bits of the unpadded one
    caps = {i: len(v) + 1 + 260 * k for k, (i, (v, _)) in enumerate(sorted(p["bags"].items()))}
    wide = _run(dev, p, capacity=caps)
    assert_bit_exact(wide[0], out, "padded: out")
    assert_bit_exact(wide[1][0], srcs[0], "padded: single-valued rows")
    for k, i in enumerate(sorted(p["bags"])):
        n = len(p["bags"][i][0])
        assert wide[1][1 + k].shape[0] == caps[i] and not wide[1][1 + k][n:].any()
        assert_bit_exact(wide[1][1 + k][:n], srcs[1 + k], "padded: bag rows")
    for a, b in zip(wide[2], grads):
        assert_bit_exact(a, b, "padded: table gradients")
    # PREDICT (no source, no view on a fresh arena) gives the TRAIN forward's bits; the composed path agrees at the parity bar
    assert_bit_exact(_run(dev, p, train=False)[0], out, "no_grad forward")
    composed = _run(dev, p, fused=False)
    assert_close(composed[0], torch.from_numpy(R.out(p)), what="composed fwd", reduced=True, ref32=torch.from_numpy(R.out(p, np.float32)))
    for a, b in zip(composed[2], R.table_grads(p)):
        assert_close(a, torch.from_numpy(b), what="composed table gradients", reduced=True)


# ---- 5. guarded, poisoned allocations --------------------------------------------------------------------------------------------------
def test_under_guarded_poisoned_allocations(dev):
    """every output is allocated 0xFF-poisoned between redzones: a piece the kernels skipped would be NaN, a store past the end
    of the rows of a bag's capacity would hit a redzone"""
    with redzone.guarded() as guard:
        place = lambda t: guard.input(t, dev)
        for shape, bags, caps in (((5, 7, 8), (6,), None), ((33, 26, 16), (), None), ((130, 7, 4), (2, 3), {2: 1027, 3: 600})):
            p = R.problem(*shape, bags, seed=7)
            _check(dev, p, capacity=caps, place=place)
        values, offsets = R.make_bags(257, 9, seed=1)
        v = R.pad(values, len(values) + 3)
        got = ops.ffm_bag_distinct(place(torch.from_numpy(v)), place(torch.from_numpy(offsets)))
        for g, w in zip(got, R.distinct(v, offsets)):
            assert np.array_equal(g.cpu().numpy(), w)
    assert {"recalgo_ffm_fwd", "recalgo_ffm_bwd", "recalgo_ffm_bag_distinct"} <= guard.launched


# ---- 6. dispatch ------------------------------------------------------------------------------------------------------------------------
def test_dispatch(dev, monkeypatch):
    calls = []
    real = ops._FfmFn.apply
    monkeypatch.setattr(ops._FfmFn, "apply", lambda *a: calls.append(1) or real(*a))
    for (B, F, K), bags, fused_by_default in (((48, 7, 4), (6,), True), ((5, 7, 6), (6,), False), ((3, 33, 4), (), False)):
        p = R.problem(B, F, K, bags, seed=2)
        del calls[:]
        out = _run(dev, p, fused=None)[0]
        assert bool(calls) == fused_by_default, (B, F, K)
        assert_close(out, torch.from_numpy(R.out(p)), what="fused=None", reduced=True, ref32=torch.from_numpy(R.out(p, np.float32)))
        if not fused_by_default:
            with pytest.raises(ValueError, match="the kernels serve 2 <= F <= 32, K % 4 == 0 with 4 <= K <= 64 and at most 4 bag fields"):
                _run(dev, p, fused=True)
        del calls[:]
        _run(dev, p, fused=False)
        assert not calls
    # a frozen setting of the all-single-valued default does not touch a call with a bag field
    monkeypatch.setattr(ops, "FFM_FUSED_ALL_SINGLE", False)
    del calls[:]
    _run(dev, R.problem(5, 7, 4, (6,), seed=2), fused=None)
    assert calls
    del calls[:]
    _run(dev, R.problem(5, 7, 4, (), seed=2), fused=None)
    assert not calls
    _run(dev, R.problem(5, 7, 4, (), seed=2), fused=True)
    assert calls


# ---- 7. model_ffm on the golden's columns: captured steps ---------------------------------------------------------------------------------
def _ffm_model(tmp_path_factory):
    """tests/test_gpu_ragged.py's model and batches; the golden rows hold at most four tags, which fit any capacity that serves
    the cut batches, so batch 3 is the golden rows with every bag written out twice: it overflows, and every id of it repeats"""
    model_fn, params, batches = _model("model_ffm", tmp_path_factory)
    feats, labels = batches[3]
    tags = feats["manual_tag_list"]
    o, v = tags.offsets.numpy(), tags.values.numpy()
    twice = [np.concatenate([v[o[i]:o[i + 1]]] * 2) for i in range(48)]
    offsets = np.zeros(49, np.int64)
    offsets[1:] = np.cumsum([len(b) for b in twice])
    doubled = dict(feats, manual_tag_list=Ragged(torch.from_numpy(np.concatenate(twice).astype(np.int64)), torch.from_numpy(offsets)))
    return model_fn, params, batches[:3] + [(doubled, labels)]


def _ffm_capacity(batches):
    """values per example of manual_tag_list: what the three cut batches need; batch 3 does not fit"""
    key = "manual_tag_list"
    caps = {key: -(-max(_nnz(b)[key] for b in batches[:3]) // 48)}
    assert [set(_nnz(b)) for b in batches] == [{key}] * 4
    assert [_nnz(b)[key] <= 48 * caps[key] for b in batches] == [True, True, True, False], (caps, [_nnz(b) for b in batches])
    return caps


def test_captured_steps_are_the_eager_steps(dev, tmp_path_factory):
    model_fn, params, batches = _ffm_model(tmp_path_factory)
    caps = _ffm_capacity(batches)
    sequence = [batches[i] for i in ORDER]
    eager = _steps(dev, model_fn, params, sequence, _on_device(dev), use_hip_graph=True, ragged_capacity=None)
    assert eager[0].graph_replays == 0 and eager[0].capture_refused is None
    graphed = _steps(dev, model_fn, params, sequence, _on_device(dev), use_hip_graph=True, ragged_capacity=caps)
    est = graphed[0]
    assert est.capture_refused is None
    assert est.ragged_overflows == 1
    assert est.graph_replays == 8 - 2 - 1 - 1, "two eager warm-up steps, the capture, the batch that overflowed"
    _assert_same_run(graphed, eager, f"model_ffm, ragged_capacity={caps}")
    # the composed path says why it cannot be captured, and computes the same model
    composed = _steps(dev, model_fn, dict(params, ffm_fused=False), sequence[:4], _on_device(dev), use_hip_graph=True, ragged_capacity=caps)
    assert composed[0].graph_replays == 0 and "_distinct_bags" in composed[0].capture_refused
    for a, b in zip(composed[1], eager[1][:4]):
        assert_close(a, b, what="composed against fused: loss")


def test_evaluate_with_the_captured_step_is_the_host_loop(dev, tmp_path_factory):
    model_fn, params, batches = _ffm_model(tmp_path_factory)
    caps = _ffm_capacity(batches)
    sequence = [_to(batches[i], dev) for i in (0, 1, 2, 0, 1, 3)]
    results = {}
    for name, run in (("host loop", dict(device_metrics=False, use_hip_graph=False)),
                      ("device, captured", dict(device_metrics=True, use_hip_graph=True, ragged_capacity=caps))):
        est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, **run))
        est.build(*sequence[0])
        for b in sequence[:2]:
            est.train_step(*b)
        results[name] = est.evaluate(lambda: iter(sequence))
        if name == "device, captured":
            assert est.graph_replays == 6 - 2 - 1 - 1 and est.ragged_overflows == 1 and est.capture_refused is None
    want = results["host loop"]
    assert {"loss", "global_step"} <= set(want) and 0.0 < want["loss"]
    assert results["device, captured"] == want and list(results["device, captured"]) == list(want)


# ---- 4. the deferred view -----------------------------------------------------------------------------------------------------------------
def test_predict_between_training_steps_reads_current_rows(dev, monkeypatch):
    """Three TF1-Adam steps on rotating batches over tables large enough that the sweep (1/32 of the arena per step) leaves the
    rows of the first batch behind the step counter: PREDICT on that batch reads them through the deferred view, as of now."""
    monkeypatch.setenv("RECALGO_ADAM_SWEEP_PERIOD", "32")
    B, F, K, vocab = 64, 4, 8, 3000
    store = VariableStore(dev)
    store.opt_state = {"step": torch.zeros(1, dtype=torch.int64, device=dev), "lr_t": torch.zeros(1, device=dev)}
    arena = store.arenas["emb"] = EmbeddingArena("emb", K, dev, seed=1)
    names = [f"t{i}" for i in range(F)]
    for n in names:
        arena.add_table(n, (F - 1) * vocab)
    arena.materialize()
    gen = torch.Generator().manual_seed(9)

    def batch(seed):
        ids = torch.randint(0, vocab, (B, F - 1), generator=gen)
        ids[torch.rand(B, F - 1, generator=gen) < 0.05] = -1
        values, offsets = R.make_bags(B, vocab, seed)
        return ids.to(dev), {F - 1: Ragged(torch.from_numpy(values).to(dev), torch.from_numpy(offsets).to(dev))}
    batches = [batch(i) for i in range(3)]

    def call(ids, bags, fused):
        return ops.ffm_interaction(store, ids, bags, arena, names, [vocab] * F, F, K, fused=fused)
    with use_store(store):
        for ids, bags in batches:
            store.begin_call()
            with torch.enable_grad():
                call(ids, bags, True).backward(torch.randn(B, 1, generator=gen).to(dev))
            store.opt_state["step"] += 1
            sparse.apply(arena, False, store.opt_state["step"], 0.01, 0.9, 0.999, 1e-8)
        plan = sparse.plan_of(arena)
        lagging = lambda: (plan.last_step > 0) & (int(store.opt_state["step"]) - plan.last_step > 0)
        assert int(store.opt_state["step"]) == 3 and bool(lagging().any()), "the test must meet rows that lag"

        def predict(fused):
            store.begin_call()
            with torch.no_grad():
                return call(*batches[0], fused).cpu().clone()
        before, composed = predict(True), predict(False)
        sparse.sync_store(store)
        assert not bool(lagging().any())
        after = predict(True)
    assert_bit_exact(after, before, "fused PREDICT through the deferred view against the swept tables")
    assert float(before.abs().max()) > 0
    assert_close(before, composed, what="fused PREDICT against composed PREDICT", reduced=True)


# ---- 8. serving -----------------------------------------------------------------------------------------------------------------------------
def test_model_ffm_is_served_from_graphs(dev, tmp_path):
    _, _, model_fn, params, export_dir = exported(dev, "model_ffm", tmp_path)
    records = golden_records()
    model = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=(16, 64), ragged_capacity=4)
    got = model.serve(records)
    assert model.compiled_buckets == [16, 64] and model.graphs_dropped_by is None and model.ragged_overflows == 0
    assert model.ragged_keys() == ["manual_tag_list"]
    _same(got, model.predict(records), "model_ffm: served from the graphs against predict")
    for lo, n in ((0, 1), (47, 1), (0, 17), (31, 17)):
        _same(model.serve(records[lo:lo + n]), {k: v[lo:lo + n] for k, v in got.items()}, f"rows {lo}..{lo + n - 1} as a request of their own")
    # a bag over the capacity is served eagerly: a capacity of two values per row, a bucket of one row, the row of four tags
    tags = GU.string_batch()[0]["manual_tag_list"]
    long = next(i for i, r in enumerate(tags) if len(r) == 4)
    small = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=(1,), ragged_capacity=2)
    _same(small.serve([records[long]]), {k: v[long:long + 1] for k, v in got.items()}, "the row of four tags alone")
    assert small.ragged_overflows == 1 and small.compiled_buckets == [1]
