"""-m gpu: recalgo_scatter_prepare_feed (include/recalgo_feed.h) — the scatter's `prepare` launch that also moves a captured
step's batch into the graph's static input span — and the captured step that uses it (estimator.GraphedTrainStep's head).

ABI: two identical copies of an arena's state (weights, Adam moments, last_step with rows that lag 1 .. P + 1 steps and rows never
touched, the lr ring, a plan workspace); (a) recalgo_copy_bytes(dst, src) then the existing entry on the ids in dst, (b) the new
entry on the ids in src with the feed as part of its launch.  Everything the launches write is compared bit for bit, dst byte
for byte, with guard bytes on both sides of dst.  Model level: tiny DCN / DeepFM steps captured with the head and without."""
import ctypes

import pytest
import torch

from recalgorithm_amd import _lib, estimator, ops, sparse as sp
from recalgorithm_amd.estimator import DeviceBatch, GraphedTrainStep, _byte_span, _tree_tensors
from recalgorithm_amd.io import synth

pytestmark = pytest.mark.gpu

P_SWEEP, T_NOW, GUARD = 6, 20, 64
COUNT, CATCHUP, SWEEP = sp.PREPARE_COUNT, sp.PREPARE_CATCHUP, sp.PREPARE_SWEEP
FLAGS = {"count": COUNT, "count+catchup": COUNT | CATCHUP, "count+catchup+sweep": COUNT | CATCHUP | SWEEP}
# (B, F, K, rows, phase of the spans inside their allocations, bytes behind the labels): a partial tile of 256, one field, the
# bench's width; a byte head (phase 8) and lengths that are no multiple of 16
SHAPES = [(300, 3, 4, 700, 0, 3), (257, 1, 16, 300, 8, 0), (64, 26, 16, 2000, 0, 5)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ids(gen, B, F, rows):
    ids = torch.randint(0, rows, (B, F), generator=gen)
    # a two-valued field: heavy duplicates (where it is the only field, every second example keeps its own row)
    two = 5 + torch.randint(0, 2, (B,), generator=gen)
    ids[:, 0] = two if F > 1 else torch.where(torch.arange(B) % 2 == 0, two, ids[:, 0])
    ids[torch.rand(B, F, generator=gen) < 0.05] = -1
    return ids


class Arena:
    """(w, m, v, last_step, lr ring) of `rows` rows of K floats: a third of the rows never touched (last_step 0), the others
    valid for a step in [T - (P + 1), T]."""

    def __init__(self, gen, rows, K, dev):
        self.rows, self.K = rows, K
        last = T_NOW - torch.randint(0, P_SWEEP + 2, (rows,), generator=gen)
        last[torch.rand(rows, generator=gen) < 0.33] = 0
        ring = torch.zeros(sp.LR_RING)
        for t in range(1, T_NOW + 1):
            ring[t % sp.LR_RING] = 0.001 * (1.0 + 0.01 * t)
        self.t = {"w": torch.randn(rows, K, generator=gen), "m": torch.randn(rows, K, generator=gen) * 0.01,
                  "v": torch.rand(rows, K, generator=gen) * 1e-3 + 1e-6, "last_step": last.to(torch.int32), "lr_ring": ring}
        self.t = {k: v.to(dev) for k, v in self.t.items()}
        self.d = sp._CDeferred(*(self.t[k].data_ptr() for k in ("w", "m", "v", "last_step", "lr_ring")), 0.9, 0.999, 1e-8)


class Setup:
    """One copy of everything a launch reads and writes, built from a seed (two Setups of one seed are identical)."""

    def __init__(self, dev, shape, n_sources, companion, seed):
        B, F, K, rows, phase, extra = shape
        lib = _lib.load()
        gen = torch.Generator().manual_seed(seed)
        self.K, self.rows = K, rows
        mats = [_ids(gen, B, F if i == 0 else 2, rows) for i in range(n_sources)]
        labels = torch.rand(B, generator=gen)
        pieces = [m.contiguous().view(-1).view(torch.uint8) for m in mats] + [labels.view(torch.uint8)]
        pieces.append(torch.randint(0, 256, (extra,), generator=gen, dtype=torch.uint8))
        span = torch.cat(pieces)
        self.nbytes = span.numel()
        self.id_offs = [sum(p.numel() for p in pieces[:i]) for i in range(n_sources)]          # (multiples of 8)
        self.want = span.to(dev)
        # the caller's span and the static span, each at `phase` inside an allocation of its own; guards around the static one
        self.src_all = torch.zeros(phase + self.nbytes, dtype=torch.uint8, device=dev)
        self.src = self.src_all[phase:]
        self.src.copy_(self.want)
        self.dst_all = torch.full((GUARD + phase + self.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.dst = self.dst_all[GUARD + phase:GUARD + phase + self.nbytes]
        assert self.src.data_ptr() % 16 == phase == self.dst.data_ptr() % 16
        self.main = Arena(gen, rows, K, dev)
        self.comp = Arena(gen, rows, 1, dev) if companion else None
        self.shapes = [(B, m.shape[1]) for m in mats]
        slots = [int(lib.recalgo_scatter_source_slots(b, f, 0)) for b, f in self.shapes]
        self.firsts = [sum(slots[:i]) for i in range(n_sources)]
        self.cap = max((sum(slots) + 255) // 256 * 256, 256)
        self.nb = int(lib.recalgo_scatter_plan_buckets_log2(self.cap))
        self.header = int(lib.recalgo_scatter_plan_header_bytes(self.nb))
        self.ws = torch.zeros(int(lib.recalgo_scatter_plan_workspace_bytes(self.cap, self.nb, K)), dtype=torch.uint8, device=dev)
        self.step = torch.full((1,), T_NOW, dtype=torch.int64, device=dev)

    def sources(self, base: torch.Tensor):
        """the recalgo_scatter_source_t array with the ids read from the span `base`"""
        return (sp._CSource * len(self.shapes))(*[sp._CSource(base.data_ptr() + o, None, None, 0, b, f, None, 0, 0, self.K, None, None, None)
                                                   for o, (b, f) in zip(self.id_offs, self.shapes)])

    def old_entry(self, flags):
        lib, n = _lib.load(), len(self.shapes)
        arr = self.sources(self.dst)
        if n == 1:
            lib.recalgo_scatter_prepare(arr, self.K, _p(self.ws), self.cap, self.nb, 0, flags, ctypes.byref(self.main.d),
                                        None if self.comp is None else ctypes.byref(self.comp.d), self.rows,
                                        0 if self.comp is None else self.rows, P_SWEEP, _p(self.step), 0, _st())
        else:
            lib.recalgo_scatter_prepare_multi(arr, n, (ctypes.c_int64 * n)(*self.firsts), self.K, _p(self.ws), self.cap, self.nb, flags,
                                              ctypes.byref(self.main.d), self.rows, P_SWEEP, _p(self.step), 0, _st())

    def new_entry(self, flags, ids_in, feed_dst, feed_src, feed_bytes):
        n = len(self.shapes)
        _lib.load().recalgo_scatter_prepare_feed(
            self.sources(ids_in), n, (ctypes.c_int64 * n)(*self.firsts), self.K, _p(self.ws), self.cap, self.nb, flags,
            ctypes.byref(self.main.d), None if self.comp is None else ctypes.byref(self.comp.d), self.rows,
            0 if self.comp is None else self.rows, P_SWEEP, _p(self.step), 0, feed_dst, feed_src, feed_bytes, _st())

    def written(self):
        torch.cuda.synchronize()
        out = {"plan header (bucket totals)": self.ws[:self.header].cpu()}
        for name, ar in (("main", self.main), ("companion", self.comp)):
            if ar is not None:
                out.update({f"{name} {k}": v.cpu() for k, v in ar.t.items()})
        return out

    def check_dst(self, what):
        got = self.dst_all.cpu()
        lo = self.dst.data_ptr() - self.dst_all.data_ptr()
        assert torch.equal(got[lo:lo + self.nbytes], self.want.cpu()), f"{what}: the static span is not the caller's, byte for byte"
        assert bool((got[:lo] == 0xA5).all()) and bool((got[lo + self.nbytes:] == 0xA5).all()), f"{what}: a guard byte of dst changed"


def _same(a, b, what):
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k].view(torch.uint8) if a[k].dtype != torch.uint8 else a[k],
                                           b[k].view(torch.uint8) if b[k].dtype != torch.uint8 else b[k])]
    assert not bad, f"{what}: {bad} differ"


VARIANTS = {"one source": (1, False), "two sources": (2, False), "companion": (1, True)}


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{s[0]}-F{s[1]}-K{s[2]}" for s in SHAPES])
def test_the_feed_launch_is_the_copy_and_the_existing_entry(dev, shape, variant, flags):
    n_sources, companion = VARIANTS[variant]
    seed = 1000 * SHAPES.index(shape) + 10 * list(VARIANTS).index(variant) + list(FLAGS).index(flags)
    a, b = (Setup(dev, shape, n_sources, companion, seed) for _ in range(2))
    what = f"{variant}, {flags}, (B, F, K) = {shape[:3]}, {a.nbytes} bytes at phase {shape[4]}"
    # something must lag, something must be untouched, or the catch-up and the sweep have nothing to show
    last = a.main.t["last_step"]
    assert int((last == 0).sum()) > 0 and int(((last > 0) & (last < T_NOW)).sum()) > 0 and int(last.min()) >= 0
    assert a.nbytes % 16 != 0 or shape[5] == 0
    before = a.written()
    # (a) the copy launch, then the existing entry on the static span
    ops.copy_bytes(a.dst, a.src)
    a.old_entry(FLAGS[flags])
    # (b) one launch: ids from the caller's span, the copy by workgroups of the same grid
    b.new_entry(FLAGS[flags], b.src, _p(b.dst), _p(b.src), b.nbytes)
    wa, wb = a.written(), b.written()
    a.check_dst(what + " (copy_bytes)")
    b.check_dst(what)
    _same(wa, wb, what)
    assert torch.equal(b.src.cpu(), b.want.cpu()), f"{what}: the caller's span was written"
    changed = [k for k in wa if not torch.equal(wa[k], before[k])]
    assert "plan header (bucket totals)" in changed, f"{what}: nothing was counted"
    if FLAGS[flags] & CATCHUP:
        assert {"main w", "main m", "main v", "main last_step"} <= set(changed), f"{what}: no row was caught up ({changed})"
        if companion:
            assert "companion last_step" in changed, f"{what}: no companion row was caught up"
    else:
        assert changed == ["plan header (bucket totals)"], f"{what}: {changed} changed without CATCHUP / SWEEP"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("feed", ["no source", "dst is src", "no bytes"])
def test_without_a_copy_the_launch_is_the_existing_entry(dev, variant, feed):
    """feed_src NULL, feed_dst == feed_src and feed_bytes 0: nothing is copied (the guards AND the span between them keep their
    fill), and what the launch writes is what the existing entry writes."""
    n_sources, companion = VARIANTS[variant]
    shape = SHAPES[0]
    flags = COUNT | CATCHUP | SWEEP
    a, b = (Setup(dev, shape, n_sources, companion, 77 + list(VARIANTS).index(variant)) for _ in range(2))
    a.dst.copy_(a.src)
    a.old_entry(flags)
    if feed == "no source":
        b.new_entry(flags, b.src, _p(b.dst), None, b.nbytes)
    elif feed == "dst is src":
        b.new_entry(flags, b.src, _p(b.src), _p(b.src), b.nbytes)
    else:
        b.new_entry(flags, b.src, _p(b.dst), _p(b.src), 0)
    _same(a.written(), b.written(), f"{variant}, {feed}")
    assert bool((b.dst_all == 0xA5).all()), f"{variant}, {feed}: the static span was written"
    assert torch.equal(b.src.cpu(), b.want.cpu())


def test_refused_feeds_launch_nothing(dev):
    """Another 16-byte phase, partially overlapping ranges, a negative size: an error code, `_supported` says no, and neither the
    state nor the spans change (the checks are host code in front of the launch)."""
    s = Setup(dev, SHAPES[0], 1, False, 5)
    lib = _lib.load()
    before, dst_before = s.written(), s.dst_all.clone()
    over = s.src_all[16:]                                               # overlaps src from above
    for what, d, r, n in (("phase", s.dst.data_ptr() + 4, s.src.data_ptr(), s.nbytes - 4), ("overlap", over.data_ptr(), s.src.data_ptr(), 64),
                          ("negative", s.dst.data_ptr(), s.src.data_ptr(), -16)):
        assert lib.recalgo_scatter_prepare_feed_supported(d, r, n) == 0, what
        with pytest.raises(_lib.RecalgoError, match="hipError_t=1"):
            s.new_entry(COUNT | CATCHUP | SWEEP, s.src, ctypes.c_void_p(d), ctypes.c_void_p(r), n)
    assert lib.recalgo_scatter_prepare_feed_supported(s.dst.data_ptr(), s.src.data_ptr(), s.nbytes) == 1
    _same(before, s.written(), "after the refused calls")
    assert torch.equal(dst_before, s.dst_all) and torch.equal(s.src.cpu(), s.want.cpu())


# ---- in the captured step ---------------------------------------------------------------------------------------------------------
B_MODEL = 300


def _estimator(model, dev):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.estimator import Estimator, RunConfig
    spec = synth.SynthSpec(n_fields=4 if model == "dcn" else 3, max_vocab=300, seed=5)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    hidden = ["32", "16"]
    if model == "dcn":
        from recalgorithm_amd.algorithm.DCN.dcn import dcn_model_fn as model_fn
        params = {"category_feature_columns": [fc.embedding_column(c, 16) for c in cats], "dense_feature_columns": [],
                  "hidden_units": hidden, "num_cross_layer": 3, "learning_rate": 0.005}
    else:
        from recalgorithm_amd.algorithm.DeepFM.deepfm import deepfm_model_fn as model_fn
        cats = sorted(cats, key=lambda c: c.key)
        params = {"first_order_feature_columns": [fc.indicator_column(c) for c in cats],
                  "second_order_feature_columns": [fc.embedding_column(c, 4) for c in cats],
                  "hidden_units": hidden, "dropout_rate": 0.0, "batch_norm": True, "learning_rate": 0.005}
    est = Estimator(model_fn, params, RunConfig(device=dev))
    batches = [synth.device_features(spec, B_MODEL, dev, batch_index=i)[:2] for i in range(3)]
    est.build(*batches[0])
    return est, batches


def _state(est, losses):
    torch.cuda.synchronize()
    out = {f"loss of call {i}": l.cpu() for i, l in enumerate(losses)}
    out.update({f"var {k}": v.detach().cpu().clone() for k, v in est.store.named_arrays().items()})
    for n, ar in est.store.arenas.items():
        out[f"arena {n}.m"], out[f"arena {n}.v"] = ar.m.cpu().clone(), ar.v.cpu().clone()
    out["flat_m"], out["flat_v"] = est.store.flat_m.cpu().clone(), est.store.flat_v.cpu().clone()
    out["step counter"] = est.store.opt_state["step"].cpu().clone()
    return out


def _as_device_batch(f, l):
    """the batch as Estimator._to_device_one_copy hands it out: a DeviceBatch whose device_span covers the id matrix and the labels
    behind it, with the layout signature of a native-reader batch of these columns (Estimator._packed_host_batch)"""
    tensors = [t for _, t in _tree_tensors(f, "f")] + [t for _, t in _tree_tensors(l, "l")]
    st = tensors[0].untyped_storage()
    assert all(t.untyped_storage().data_ptr() == st.data_ptr() for t in tensors)
    hi = max(_byte_span(t)[1] for t in tensors)
    buf = torch.empty(0, dtype=torch.uint8, device=tensors[0].device).set_(st, 0, (hi,), (1,))
    feats = DeviceBatch(f)
    B = tensors[0].shape[0]
    assert hi == 8 * B * len(f) + 4 * B * len(l)
    sig = ("ids+labels", int(hi), int(B), tuple(f), tuple(l), tuple(tuple(v.shape) for v in l.values()))
    feats.device_span = (buf, sig, (dict(f), l))
    return feats, l


def _host_batch(f, l, packed):
    """the batch on the host: plain column tensors, or a native-reader batch (PackedBatch: columns of ONE [B, F] matrix)"""
    from recalgorithm_amd.io.native import PackedBatch
    labels = {k: v.cpu() for k, v in l.items()}
    if not packed:
        return {k: v.cpu() for k, v in f.items()}, labels
    keys = list(f)
    mat = torch.stack([f[k].cpu() for k in keys], 1).contiguous()
    feats = PackedBatch({k: mat[:, j] for j, k in enumerate(keys)})
    feats.packed_ids = (mat, keys)
    return feats, labels


@pytest.fixture
def switch(monkeypatch):
    before = estimator.FEED_IN_PREPARE
    copies = []
    real = ops.copy_bytes
    monkeypatch.setattr(ops, "copy_bytes", lambda dst, src: (copies.append(dst.numel()), real(dst, src))[1])
    yield copies
    estimator.FEED_IN_PREPARE = before


def _captured_run(model, dev, on, layout, copies):
    estimator.FEED_IN_PREPARE = on
    est, batches = _estimator(model, dev)
    if layout == "device batch":
        batches = [_as_device_batch(*b) for b in batches]
    kept = [[t.clone() for _, t in _tree_tensors({"f": dict(b[0]), "l": b[1]}, "b")] for b in batches]
    g = GraphedTrainStep(est.train_step, *batches[0], warmup=1)
    assert (g._span_plan is not None) == (layout == "device batch")
    assert (g._head is not None) == on, f"{model}: the step's first prepare launch was {'not ' if on else ''}taken as its head"
    del copies[:]
    # six replays over three rotating device batches (one-span loads), one replay of the inputs as they stand
    losses = [g(*batches[i % 3]).clone() for i in range(6)] + [g().clone()]
    counters = {"head_launches": g.head_launches, "fused_feeds": g.fused_feeds, "copy launches": len(copies)}
    # a batch whose columns are separately allocated: per-tensor copies, the head runs without a feed
    f, l = batches[1]
    fused = g.fused_feeds
    losses.append(g({k: v.clone() for k, v in f.items()}, {k: v.clone() for k, v in l.items()}).clone())
    assert g.fused_feeds == fused, "a per-tensor load was fed through the head"
    # the host path of the training loop: a reader batch of the captured layout goes straight into the static span (the head runs
    # without a feed); plain host columns go through _to_device and the device load
    fused = g.fused_feeds
    if layout == "device batch":
        g.load(*batches[0])                             # a load that no replay follows: the host batch below replaces it
    losses.append(est.feed_step(g, *_host_batch(*batches[2], packed=layout == "device batch")).clone())
    assert layout != "device batch" or g.fused_feeds == fused
    assert g.head_launches == (9 if on else 0)
    state = _state(est, losses)
    # the caller's batches were read, never written
    assert all(torch.equal(t, k) for b, kp in zip(batches, kept) for (_, t), k in zip(_tree_tensors({"f": dict(b[0]), "l": b[1]}, "b"), kp))
    return state, counters


@pytest.mark.parametrize("layout", ["views of one allocation", "device batch"])
@pytest.mark.parametrize("model", ["dcn", "deepfm"])
def test_captured_steps_are_the_same_with_the_batch_fed_by_the_head(dev, model, layout, switch):
    off, c_off = _captured_run(model, dev, False, layout, switch)
    on, c_on = _captured_run(model, dev, True, layout, switch)
    assert c_off == {"head_launches": 0, "fused_feeds": 0, "copy launches": 6}, c_off
    # every span load rode in the head's launch; no copy launch was issued for any of them
    assert c_on == {"head_launches": 7, "fused_feeds": 6, "copy launches": 0}, c_on
    assert int(off["step counter"]) == 1 + 9
    assert all(bool(torch.isfinite(v).all()) for k, v in off.items() if k.startswith("loss"))
    assert len({float(off[f"loss of call {i}"]) for i in range(3)}) == 3, "the three batches give three losses"
    assert on.keys() == off.keys()
    bad = [k for k in off if not torch.equal(off[k], on[k])]
    assert not bad, f"{model}, {layout}: with the head the run differs in {bad[:8]} ({len(bad)} in all)"


def test_a_step_whose_first_lookup_is_ragged_takes_no_head(dev, switch):
    """DIN: the first prepare launch of the step carries the history's ragged lookup — not eligible; the step is captured whole,
    the load is the copy launch, and the results are those of the switch off."""
    import bench
    runs = {}
    for on in (False, True):
        estimator.FEED_IN_PREPARE = on
        est, spec, _, _, _ = bench.build_estimator(bench.parse_args(["--model", "din", "--batch", "256", "--fields", "8", "--max-vocab", "500"]), dev)
        batches = [synth.device_features(spec, 256, dev, batch_index=i)[:2] for i in range(3)]
        g = GraphedTrainStep(est.train_step, *batches[0], warmup=1)
        assert g._head is None
        losses = [g(*batches[i % 3]).clone() for i in range(4)]
        assert g.head_launches == 0 and g.fused_feeds == 0
        runs[on] = _state(est, losses)
    bad = [k for k in runs[False] if not torch.equal(runs[False][k], runs[True][k])]
    assert not bad, f"din: {bad[:8]} differ ({len(bad)} in all)"
