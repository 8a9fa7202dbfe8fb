"""-m gpu: the one launch that ends every training step, recalgo_adam_tf1_step / recalgo_adam_tf1_step_plans (csrc/tail.hip,
adam_tf1_step_kernel), driven at the C ABI (include/recalgo.h) with the test's own buffers, live lists, counters and plan-scan
records.

Two references.  BIT-EXACT: the same state run through the separate entries on copies of the buffers -
recalgo_adam_tf1_advance, recalgo_adam_tf1_dense with its lr_t_dev, one recalgo_adam_tf1_list per arena and, where the rows
outside the list have g = m = v = 0, recalgo_adam_tf1_dense over the whole [rows * K] arena - compared after each of three
steps.  ABSOLUTE: oracle.ref_ops.adam_tf1_step in float64 at tests.util.assert_close's default tolerance, with the inputs of
test_gpu_kernels.test_adam_tf1 (randn, a third of g exactly zero); LazyAdam against ref_ops.lazy_adam_step at the rtol of
test_gpu_sparse.test_lazy_adam_matches_tf_lazy_adam.

A live list is a shuffled ("first touch") permutation of ALL rows of the arena plus a device count: the slots behind the count
hold valid rows that are not in the set, so a kernel that reads past the count gives wrong numbers, never a wild address.

The arms of the launch and the smallest shape that reaches each:

| arm                                                        | shape                                                            |
|------------------------------------------------------------|------------------------------------------------------------------|
| dense: scalar tail only                                    | n = 1, 3                                                         |
| dense: one float4 word, no tail / 3-float tail             | n = 4 / 7                                                        |
| dense: second workgroup / with tail                        | n = 1025 / 2053                                                  |
| dense: the 4096-workgroup cap, second grid-stride pass     | n = 4_197_379 (cap: 4_194_304 floats; 3-float tail)              |
| dense: inert word skipped (g = m = v = 0, one g = -0.0)    | every fifth float4 word of n >= 8                                |
| lr_t from step_dev, advance = 0 / 1, the arrival ticket    | 298 workgroups, step_dev from 0, 1, 9, 999, 10^6                 |
| the launch with nothing to do (n = 0, no live arena)       | one workgroup that only takes its ticket                         |
| arena routing, descriptors 0..3, a max_rows = 0 descriptor | K = (16, 12, 6, 256) beside n = 2053                             |
| float4 arm, shift (K / 4 = 1, 2, 16, 64 lanes per row)     | K = 4, 8, 64, 256 at 130..300 rows                               |
| float4 arm, division (K / 4 not a power of two)            | K = 12, 260                                                      |
| scalar arm (K % 4 != 0), any base alignment                | K = 1, 2, 6                                                      |
| the 2048-workgroup cap of an arena                         | K = 64 x 33_000 rows (float4), K = 6 x 90_000 rows (scalar)      |
| lazy vote over the K / 4 lanes of a row                    | K = 4, 16, 64, 256; the gradient in the row's LAST float4 only   |
| plan scan: counters in registers / re-read                 | nb_log2 = 8, 10, 12 (1, 4, 16 per thread) / 13 (32)              |
| plan scan behind other workgroups (scan_first > 0)         | beside n = 2053 and two arenas                                   |
| refusals (hipErrorInvalidValue, nothing written)           | advance without a ticket, lazy K = 1, 6, 12, 260, 512, a base 4 bytes off |

Every test is a thin wrapper over a helper (dev, ...), so that test_cases_under_the_redzone_guard can run the helpers again
between 0xFF fences."""
import ctypes

import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from oracle import ref_ops
from recalgorithm_amd import _lib
from tests.redzone import guarded
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

_Arena, _Scan = _lib.STRUCTS["recalgo_adam_arena_t"], _lib.STRUCTS["recalgo_plan_scan_t"]
LR, B1, B2, EPS = 0.005, 0.9, 0.999, 1e-8
LAZY_RTOL = 2e-5                                   # (test_lazy_adam_matches_tf_lazy_adam)
REFUSED = r"failed with hipError_t=1$"             # hipErrorInvalidValue

DENSE_N = (1, 3, 4, 7, 1025, 2053, 4_197_379)
STEP_STARTS = (0, 1, 9, 999, 10 ** 6)
MIXED_K = (16, 12, 6, 256)
ARM_ROWS = {4: 300, 8: 257, 64: 130, 256: 131, 12: 211, 260: 133, 1: 300, 2: 259, 6: 173}
LAZY_K = (4, 16, 64, 256)
LAZY_REFUSED_K = (1, 6, 12, 260, 512)
SCAN_KINDS = ("zero", "equal", "random")


def L():
    return _lib.load()               # (looked up per call: under redzone.guarded() it is the recording proxy)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _third_zero(gen, *shape):
    g = torch.randn(*shape, generator=gen)
    g.view(-1)[::3] = 0.0
    return g


def _place(t, dev, shift=0):
    """A flat device copy of `t` whose first element lies `shift` floats behind a 16-byte aligned base."""
    flat = t.reshape(-1)
    if not shift:
        return flat.clone().to(dev)
    out = torch.cat([torch.full((shift,), -7777.0), flat]).to(dev)[shift:]
    assert out.data_ptr() % 16 == 4 * shift
    return out


# ---- what one launch sees, on the host --------------------------------------------------------------------------------------------
class Dense:
    """The flat dense buffer: p randn, m = v = 0 at the start.  Every fifth float4 word (from word 1) is inert - g = m = v = 0 in
    every step - and one float of word 1 has g = -0.0.  g: randn with a third exactly zero, except in the n % 4 tail."""

    def __init__(self, n, seed=0, shift=0):
        self.n, self.shift = n, shift
        self.gen = torch.Generator().manual_seed(n * 31 + seed)
        self.p, self.m, self.v = torch.randn(n, generator=self.gen), torch.zeros(n), torch.zeros(n)
        words = torch.zeros(n // 4, 4, dtype=torch.bool)
        words[1::5] = True
        self.inert = torch.cat([words.view(-1), torch.zeros(n % 4, dtype=torch.bool)])
        self.neg0 = 6 if n >= 8 else None

    def grad(self, s):
        g = _third_zero(self.gen, self.n) * s
        tail = self.n % 4
        if tail:                                      # (no zero there: with m = v = 0 a tail element nobody updates would pass)
            g[self.n - tail:] = (torch.rand(tail, generator=self.gen) + 0.5) * s
        g[self.inert] = 0.0
        if self.neg0 is not None:
            g[self.neg0] = -0.0
        return g


class ArenaSpec:
    """One arena [rows, K] with a shuffled list of all its rows, of which the first `count` are live.
    plain: m = v = 0 at the start and g = 0 outside the live rows (the invariant of the product: the dense update of the whole
           arena is the same thing);
    decoy: every row has non-zero g, m and v; only the live rows may move;
    lazy:  every row has non-zero m and v; in a step a live row has either g = 0 (it must keep p, m, v) or a gradient in ONE
           element of its last float4 (the whole row moves)."""

    def __init__(self, K, rows, count, lazy=0, decoy=False, seed=0, max_rows=None, shift=0):
        self.K, self.rows, self.count, self.lazy, self.decoy, self.shift = K, rows, count, lazy, decoy, shift
        self.max_rows = rows if max_rows is None else max_rows
        self.gen = gen = torch.Generator().manual_seed((K * 1009 + rows) * 31 + seed)
        self.p = torch.randn(rows, K, generator=gen)
        self.list = torch.randperm(rows, generator=gen).to(torch.int32)
        warm = decoy or lazy
        self.m = torch.randn(rows, K, generator=gen) * 0.1 if warm else torch.zeros(rows, K)
        self.v = torch.rand(rows, K, generator=gen) * 0.01 + 1e-4 if warm else torch.zeros(rows, K)
        self.invariant = not warm and not shift and self.max_rows > 0
        self.moved = self.live

    @property
    def live(self):
        return self.list[:self.count].long()

    def grad(self, s):
        """This step's gradient [rows, K]; self.moved: the rows the step must move, in list order."""
        g, live = torch.zeros(self.rows, self.K), self.live
        if self.lazy:
            self.moved = live[(torch.arange(self.count) + s) % 2 == 0]
            g[self.moved, self.K - 1 - (s % 4 if self.K >= 4 else 0)] = (torch.rand(self.moved.numel(), generator=self.gen) + 0.5) * s
        else:
            self.moved = live
            g[live] = _third_zero(self.gen, self.count, self.K) * s
        if self.decoy:
            others = self.list[self.count:].long()
            g[others] = torch.randn(others.numel(), self.K, generator=self.gen) + 3.0
        return g


class ScanSpec:
    """A fabricated plan: bucket b's count at word b << cs of `total` (the words between hold a large number), offs and sched
    0xFF bytes before every launch."""

    def __init__(self, dev, nb_log2, cs, kind, seed=0):
        self.nb_log2, self.cs, self.kind = nb_log2, cs, kind
        nb = 1 << nb_log2
        gen = torch.Generator().manual_seed(nb * 7 + cs + seed)
        if kind == "zero":
            c = torch.zeros(nb, dtype=torch.int64)
        elif kind == "equal":
            c = torch.full((nb,), 37, dtype=torch.int64)
        else:
            c = torch.randint(0, 60, (nb,), generator=gen)
            c[torch.randperm(nb, generator=gen)[:5]] = 5000 + torch.arange(5)
        self.counts = c
        words = torch.full((nb << cs,), 1_000_003, dtype=torch.int64)
        words[torch.arange(nb) << cs] = c
        self.words = words.to(torch.int32)
        self.total = self.words.to(dev)
        self.offs = torch.full((nb,), -1, dtype=torch.int32, device=dev)
        self.sched = torch.full((nb, 4), -1, dtype=torch.int32, device=dev)
        self.heavy_min = 2 * (int(c.sum()) >> nb_log2) + 64
        assert (kind == "random") == bool((c >= self.heavy_min).any()), "the fabricated totals"

    def record(self):
        return _Scan(self.total.data_ptr(), self.offs.data_ptr(), self.sched.data_ptr(), self.cs, self.nb_log2)

    def reset(self):
        self.offs.fill_(-1)
        self.sched.fill_(-1)

    def check(self, what):
        c, nb = self.counts, self.counts.numel()
        want = torch.cumsum(c, 0) - c
        assert torch.equal(self.offs.cpu().long(), want), f"{what}: offs is not the exclusive prefix sum of the counts"
        sch = self.sched.cpu().long()
        b = sch[:, 0]
        assert torch.equal(torch.sort(b).values, torch.arange(nb)), f"{what}: sched is not a permutation of the buckets"
        assert torch.equal(sch[:, 1], want[b]) and torch.equal(sch[:, 2], c[b]) and not bool(sch[:, 3].any()), \
            f"{what}: a sched record is not (b, offs[b], count[b], 0)"
        heavy = c[b] >= self.heavy_min
        nh = int(heavy.sum())
        assert bool(heavy[:nh].all()) and not bool(heavy[nh:].any()), f"{what}: the heavy buckets do not come first"
        assert_bit_exact(self.total, self.words, f"{what}: the counters")


class World:
    """One device copy of everything the launch reads and writes."""

    def __init__(self, dev, dense, specs, t0=0):
        z = torch.zeros
        self.d = None if dense is None else [_place(t, dev, dense.shift) for t in (dense.p, z(dense.n), dense.m, dense.v)]
        self.a = [[_place(t, dev, s.shift) for t in (s.p, z(s.rows, s.K), s.m, s.v)] for s in specs]
        self.lists = [s.list.clone().to(dev) for s in specs]
        self.counts = [torch.tensor([s.count], dtype=torch.int32).to(dev) for s in specs]
        self.step = torch.full((1,), t0, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lr_t = torch.zeros(1, device=dev)

    def set_grads(self, gd, ga):
        if self.d is not None:
            self.d[1].copy_(gd)
        for bufs, g in zip(self.a, ga):
            bufs[1].copy_(g.reshape(-1))

    def set_list(self, j, rows):
        """(the reference of a lazy arena: a list of exactly the rows with a non-zero gradient)"""
        if rows.numel():
            self.lists[j][:rows.numel()].copy_(rows.to(torch.int32))
        self.counts[j].fill_(rows.numel())

    def tensors(self):
        out = {"step": self.step, "ticket": self.ticket}
        for nm, t in zip("pgmv", self.d or ()):
            out[f"dense {nm}"] = t
        for j, bufs in enumerate(self.a):
            for nm, t in zip("pgmv", bufs):
                out[f"arena {j} {nm}"] = t
        return out

    def snapshot(self):
        return {k: t.clone() for k, t in self.tensors().items()}

    def assert_unchanged(self, snap, what):
        for k, t in self.tensors().items():
            assert_bit_exact(t, snap[k], f"{what}: {k} after the refused call")


def _launch_fused(w, dense, specs, advance, zero_grad, scans=(), ticket=True, nonlazy=False):
    lib = L()
    arr = None
    if specs:
        arr = (_Arena * len(specs))()
        for j, (s, bufs) in enumerate(zip(specs, w.a)):
            arr[j] = _Arena(*[b.data_ptr() for b in bufs], w.lists[j].data_ptr(), w.counts[j].data_ptr(), s.max_rows, s.K,
                            0 if nonlazy else s.lazy)
    d = w.d or [None] * 4
    args = (P(d[0]), P(d[1]), P(d[2]), P(d[3]), 0 if dense is None else dense.n, arr, len(specs), P(w.step),
            P(w.ticket) if ticket else None, advance, LR, B1, B2, EPS, zero_grad)
    if scans:
        recs = (_Scan * len(scans))(*[c.record() for c in scans])
        return lib.recalgo_adam_tf1_step_plans(*args, recs, len(scans), _stream())
    return lib.recalgo_adam_tf1_step(*args, _stream())


def _launch_separate(w, dense, specs, advance, zero_grad):
    """recalgo_adam_tf1_advance (on a counter put back by one where the launch under test does not advance), then
    recalgo_adam_tf1_dense and one recalgo_adam_tf1_list per arena with its lr_t_dev."""
    lib = L()
    if not advance:
        w.step.sub_(1)
    lib.recalgo_adam_tf1_advance(P(w.step), LR, B1, B2, P(w.lr_t), _stream())
    if w.d is not None:
        lib.recalgo_adam_tf1_dense(*map(P, w.d), dense.n, 0.0, P(w.lr_t), B1, B2, EPS, zero_grad, _stream())
    for j, (s, bufs) in enumerate(zip(specs, w.a)):
        lib.recalgo_adam_tf1_list(*map(P, bufs), P(w.lists[j]), P(w.counts[j]), s.max_rows, s.K, 0.0, P(w.lr_t), B1, B2, EPS,
                                  zero_grad, _stream())


def _launch_whole(w, specs, lr_t, zero_grad):
    """recalgo_adam_tf1_dense over the whole arena, where the rows outside the list have g = m = v = 0."""
    for s, bufs in zip(specs, w.a):
        if s.invariant:
            L().recalgo_adam_tf1_dense(*map(P, bufs), s.rows * s.K, 0.0, P(lr_t), B1, B2, EPS, zero_grad, _stream())


class Ref64:
    def __init__(self, dense, specs):
        self.d = None if dense is None else [t.double() for t in (dense.p, dense.m, dense.v)]
        self.a = [[t.double() for t in (s.p, s.m, s.v)] for s in specs]

    def step(self, t, specs, gd, ga):
        if self.d is not None:
            ref_ops.adam_tf1_step(self.d[0], gd.double(), self.d[1], self.d[2], t, LR, B1, B2, EPS)
        for s, (p, m, v), g in zip(specs, self.a, ga):
            rows = s.moved
            if s.max_rows <= 0 or rows.numel() == 0:
                continue
            if s.lazy:
                ref_ops.lazy_adam_step(p, rows, g[rows].double(), m, v, t, LR, B1, B2, EPS)
            else:
                pl, ml, vl = p[rows], m[rows], v[rows]
                ref_ops.adam_tf1_step(pl, g[rows].double(), ml, vl, t, LR, B1, B2, EPS)
                p[rows], m[rows], v[rows] = pl, ml, vl


def _run(dev, n, specs, *, steps=3, zero_grad=1, advance=1, t0=0, scans=(), absolute=True, reference="separate", seed=0,
         dense_shift=0, what=""):
    """`steps` launches of the fused entry from step counter t0 against both references; after each: the counter and the ticket,
    p / g / m / v of the dense buffer and of every arena bit for bit, the scans.  reference "nonlazy": the bit-exact reference of
    the arenas is the fused launch itself with lazy = 0 and a list of exactly the rows with a non-zero gradient."""
    dense = Dense(n, seed, dense_shift) if n else None
    fused, sep, whole = World(dev, dense, specs, t0), World(dev, dense, specs, t0), World(dev, None, specs, t0)
    ref = Ref64(dense, specs) if absolute else None
    gd, ga = None, []
    for s in range(1, steps + 1):
        t, tag = t0 + s, f"{what} step {s}"
        gd, ga = dense.grad(s) if dense else None, [sp.grad(s) for sp in specs]
        for w in (fused, sep, whole):
            w.set_grads(gd, ga)
        for j, sp in enumerate(specs):
            if sp.lazy:
                sep.set_list(j, sp.moved)
        if not advance:
            fused.step.fill_(t)
            sep.step.fill_(t)
        for c in scans:
            c.reset()
        assert _launch_fused(fused, dense, specs, advance, zero_grad, scans) == 0
        if reference == "nonlazy":
            assert _launch_fused(sep, dense, specs, advance, zero_grad, nonlazy=True) == 0
        else:
            _launch_separate(sep, dense, specs, advance, zero_grad)
            _launch_whole(whole, specs, sep.lr_t, zero_grad)
        assert int(fused.step.cpu()) == t, f"{tag}: step_dev is {int(fused.step.cpu())}, not {t} (advance = {advance})"
        assert int(fused.ticket.cpu()) == 0, f"{tag}: the ticket reads {int(fused.ticket.cpu())} after the call"
        assert int(sep.step.cpu()) == t
        got, want = fused.tensors(), sep.tensors()
        for k in got:
            assert_bit_exact(got[k], want[k], f"{tag}: {k}, one launch vs the separate entries")
        if reference != "nonlazy":
            for j, sp in enumerate(specs):
                if sp.invariant:
                    for nm, a, b in zip("pgmv", fused.a[j], whole.a[j]):
                        assert_bit_exact(a, b, f"{tag}: arena {j} {nm} vs the dense update of the whole arena")
        if dense is not None:
            if zero_grad:
                assert not bool(fused.d[1].cpu().ne(0).any()), f"{tag}: zero_grad left a gradient in the dense buffer"
            else:
                assert_bit_exact(fused.d[1], gd, f"{tag}: dense g with zero_grad = 0")
        for j, sp in enumerate(specs):
            g = fused.a[j][1].cpu().view(sp.rows, sp.K)
            if sp.max_rows <= 0 or not zero_grad:
                assert_bit_exact(g, ga[j], f"{tag}: arena {j} g (zero_grad = {zero_grad}, max_rows = {sp.max_rows})")
            else:
                assert not bool(g[sp.live].ne(0).any()), f"{tag}: zero_grad left a gradient in a live row of arena {j}"
        for i, c in enumerate(scans):
            c.check(f"{tag}: scan {i}")
        if ref is not None:
            ref.step(t, specs, gd, ga)
    if ref is not None:
        if ref.d is not None:
            for nm, a, b in zip("pmv", (fused.d[0], fused.d[2], fused.d[3]), ref.d):
                assert_close(a, b, what=f"{what}: dense {nm}")
        for j, sp in enumerate(specs):
            bufs = fused.a[j]
            for nm, a, b in zip("pmv", (bufs[0], bufs[2], bufs[3]), ref.a[j]):
                assert_close(a, b, what=f"{what}: arena {j} (K = {sp.K}) {nm}", **({"rtol": LAZY_RTOL} if sp.lazy else {}))
    if dense is not None and bool(dense.inert.any()):
        assert_bit_exact(fused.d[0].cpu()[dense.inert], dense.p[dense.inert], f"{what}: p of the inert words")
    for j, sp in enumerate(specs):
        still = torch.ones(sp.rows, dtype=torch.bool)
        if sp.max_rows > 0:
            still[sp.live] = False                      # (a lazy arena's live rows all move in one step or the other)
        host = (sp.p, ga[j], sp.m, sp.v)
        for nm, a, b in zip("pgmv", fused.a[j], host):
            assert_bit_exact(a.cpu().view(sp.rows, sp.K)[still], b[still], f"{what}: arena {j} {nm} of the rows outside the list")
    return fused


def _refused(dev, n, specs, *, advance=1, ticket=True, dense_shift=0, what=""):
    """The call returns hipErrorInvalidValue; every buffer, the counter and the ticket keep their bits."""
    dense = Dense(n, 0, dense_shift) if n else None
    w = World(dev, dense, specs, 7)
    w.set_grads(dense.grad(1) if dense else None, [sp.grad(1) for sp in specs])
    snap = w.snapshot()
    with pytest.raises(_lib.RecalgoError, match=REFUSED):
        _launch_fused(w, dense, specs, advance, 1, ticket=ticket)
    torch.cuda.synchronize()
    w.assert_unchanged(snap, what)


# ---- a. the dense buffer alone ----------------------------------------------------------------------------------------------------
def _dense_case(dev, n, zero_grad):
    _run(dev, n, [], zero_grad=zero_grad, advance=0, what=f"dense n = {n}, zero_grad = {zero_grad}")


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("n", DENSE_N)
def test_dense_buffer_alone(dev, n, zero_grad):
    _dense_case(dev, n, zero_grad)


# ---- b. the step counter and the ticket -------------------------------------------------------------------------------------------
def _counter_case(dev, t0, advance):
    """293 dense and 5 arena workgroups, five eager calls in a row."""
    _run(dev, 300_001, [ArenaSpec(16, 300, 300)], steps=5, advance=advance, t0=t0, what=f"counter from {t0}, advance = {advance}")


@pytest.mark.parametrize("t0", STEP_STARTS)
def test_advance_1_moves_the_counter_by_one_per_call_and_rearms_the_ticket(dev, t0):
    _counter_case(dev, t0, 1)


def test_advance_0_reads_the_counter_and_leaves_it(dev):
    _counter_case(dev, 9, 0)


def _no_ticket_case(dev):
    _refused(dev, 2053, [ArenaSpec(16, 130, 65)], advance=1, ticket=False, what="advance = 1 without a ticket")
    # advance = 0 needs none
    dense = Dense(7)
    w = World(dev, dense, [], 3)
    w.set_grads(dense.grad(1), [])
    assert _launch_fused(w, dense, [], 0, 1, ticket=False) == 0
    assert int(w.step.cpu()) == 3


def test_advance_1_without_a_ticket_is_refused(dev):
    _no_ticket_case(dev)


def _empty_specs():
    return {"no arenas": [], "max_rows 0 only": [ArenaSpec(16, 8, 5, max_rows=0), ArenaSpec(6, 8, 8, max_rows=0)]}


def _empty_case(dev, which, advance):
    """n = 0 and no arena with rows: one workgroup with nothing to update.  (Before the arena branch asked for n_arenas > 0 it read
    the count of a padding descriptor through a null pointer: found by reading, never run.)"""
    if which == "one scan":
        specs, scans = [], [ScanSpec(dev, 10, 4, "random")]
    else:
        specs, scans = _empty_specs()[which], []
    _run(dev, 0, specs, advance=advance, t0=41, scans=scans, what=f"empty launch ({which}), advance = {advance}")


@pytest.mark.parametrize("advance", [0, 1])
@pytest.mark.parametrize("which", ["no arenas", "max_rows 0 only", "one scan"])
def test_launch_with_nothing_to_update(dev, which, advance):
    _empty_case(dev, which, advance)


def test_graph_replay_with_growing_live_lists(dev):
    """One captured launch (n = 5000, K = 16 and K = 6 arenas, one scan, advance = 1), one eager launch first, replayed 10 times
    with new gradients and a growing live_count in the static buffers; after each replay bit for bit the eager sequence of the
    separate entries."""
    t0, n = 5, 5000
    dense = Dense(n)
    specs = [ArenaSpec(16, 300, 20), ArenaSpec(6, 257, 20)]
    scan = ScanSpec(dev, 10, 4, "random")
    fused, sep = World(dev, dense, specs, t0), World(dev, dense, specs, t0)

    def feed(s):
        for j, sp in enumerate(specs):
            sp.count = min(sp.rows, 20 * s)
            for w in (fused, sep):
                w.counts[j].fill_(sp.count)
        gd, ga = dense.grad(s), [sp.grad(s) for sp in specs]
        for w in (fused, sep):
            w.set_grads(gd, ga)
        scan.reset()

    def compare(s):
        torch.cuda.synchronize()
        _launch_separate(sep, dense, specs, 1, 1)
        got, want = fused.tensors(), sep.tensors()
        for k in got:
            assert_bit_exact(got[k], want[k], f"graph, launch {s}: {k}")
        scan.check(f"graph, launch {s}")

    feed(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _launch_fused(fused, dense, specs, 1, 1, [scan]) == 0
    torch.cuda.current_stream().wait_stream(side)
    compare(1)
    graph = torch.cuda.CUDAGraph()
    feed(2)
    with torch.cuda.graph(graph):
        assert _launch_fused(fused, dense, specs, 1, 1, [scan]) == 0
    for it in range(10):
        graph.replay()
        compare(2 + it)
        feed(3 + it)
    assert int(fused.step.cpu()) == t0 + 1 + 10 and int(fused.ticket.cpu()) == 0


# ---- c. arenas --------------------------------------------------------------------------------------------------------------------
def _mixed_specs(hole):
    specs = [ArenaSpec(K, ARM_ROWS.get(K, 140), ARM_ROWS.get(K, 140) // 2 + 1, seed=j) for j, K in enumerate(MIXED_K)]
    if hole:
        specs[1] = ArenaSpec(12, 8, 5, max_rows=0)
    return specs


def _mixed_case(dev, hole):
    _run(dev, 2053, _mixed_specs(hole), advance=0, t0=2, what=f"four arenas K = {MIXED_K}" + (", max_rows = 0 in position 1" if hole else ""))


@pytest.mark.parametrize("hole", [0, 1], ids=["four-live", "max_rows-0-in-position-1"])
def test_four_arenas_of_different_widths_beside_the_dense_buffer(dev, hole):
    _mixed_case(dev, hole)


LIVE = ("none", "one", "all", "half")


def _counts(rows):
    return {"none": 0, "one": 1, "all": rows, "half": rows // 2 + 1}


def _width_case(dev, K, live):
    rows = ARM_ROWS[K]
    _run(dev, 0, [ArenaSpec(K, rows, _counts(rows)[live])], advance=0, t0=1, what=f"arena K = {K}, {rows} rows, {live} live")


@pytest.mark.parametrize("live", LIVE)
@pytest.mark.parametrize("K", sorted(ARM_ROWS))
def test_arena_width_arms(dev, K, live):
    _width_case(dev, K, live)


CAPS = [(64, 33_000), (6, 90_000)]


def _cap_case(dev, K, rows):
    _run(dev, 0, [ArenaSpec(K, rows, rows)], advance=0, t0=1, what=f"arena K = {K}, {rows} rows, all live (2048-workgroup cap)")


@pytest.mark.parametrize("K,rows", CAPS)
def test_arena_beyond_the_workgroup_cap(dev, K, rows):
    _cap_case(dev, K, rows)


def _decoy_case(dev, K):
    rows = 260
    _run(dev, 1025, [ArenaSpec(K, rows, rows // 2, decoy=True)], what=f"decoy rows, K = {K}")


@pytest.mark.parametrize("K", [16, 12, 6])
def test_rows_behind_the_count_are_not_touched(dev, K):
    """The rows in the list's slots behind live_count have non-zero g, m and v and keep them, and p, bit for bit."""
    _decoy_case(dev, K)


def _scalar_arm_any_base_case(dev):
    _run(dev, 7, [ArenaSpec(6, 173, 90, shift=1), ArenaSpec(1, 300, 151, shift=3)], what="scalar arm at a base 4 / 12 bytes off")


def test_scalar_arm_takes_any_base(dev):
    _scalar_arm_any_base_case(dev)


# ---- d. lazy ----------------------------------------------------------------------------------------------------------------------
def _lazy_case(dev, K):
    rows = 200
    for reference in ("nonlazy", "separate"):
        _run(dev, 0, [ArenaSpec(K, rows, rows // 2 + 1, lazy=1)], reference=reference, what=f"lazy K = {K} ({reference})")


@pytest.mark.parametrize("K", LAZY_K)
def test_lazy_rows_vote_as_a_whole(dev, K):
    _lazy_case(dev, K)


def _lazy_beside_plain_case(dev):
    _run(dev, 1025, [ArenaSpec(16, 200, 101, lazy=1), ArenaSpec(16, 200, 101, seed=1), ArenaSpec(64, 130, 66, lazy=1)],
         what="lazy and plain arenas in one launch")


def test_lazy_and_plain_arenas_in_one_launch(dev):
    _lazy_beside_plain_case(dev)


def _lazy_refused_case(dev, K):
    _refused(dev, 1025, [ArenaSpec(16, 130, 65), ArenaSpec(K, 40, 20, lazy=1)], advance=1, what=f"lazy K = {K}")


@pytest.mark.parametrize("K", LAZY_REFUSED_K)
def test_lazy_widths_that_cannot_vote_per_row_are_refused(dev, K):
    _lazy_refused_case(dev, K)


# ---- e. plan-scan riders ----------------------------------------------------------------------------------------------------------
SCAN_SHAPES = [(nb_log2, cs) for nb_log2 in (8, 10, 12, 13) for cs in (0, 4)]


def _scan_case(dev, nb_log2, cs, kind):
    what = f"scan nb_log2 = {nb_log2}, counter_shift = {cs}, {kind}"
    alone = ScanSpec(dev, nb_log2, cs, kind)
    _run(dev, 0, [], advance=1, t0=3, steps=1, scans=[alone], what=what + " alone")
    rider = ScanSpec(dev, nb_log2, cs, kind)
    _run(dev, 2053, [ArenaSpec(16, 300, 151), ArenaSpec(6, 173, 90)], advance=1, t0=3, steps=1, scans=[rider], what=what + " riding")
    assert_bit_exact(rider.offs, alone.offs, what + ": offs alone vs riding")
    assert_bit_exact(rider.sched, alone.sched, what + ": sched alone vs riding")


@pytest.mark.parametrize("kind", SCAN_KINDS)
@pytest.mark.parametrize("nb_log2,cs", SCAN_SHAPES)
def test_plan_scan_alone_and_behind_other_workgroups(dev, nb_log2, cs, kind):
    _scan_case(dev, nb_log2, cs, kind)


def _scans_beside_case(dev, n_scans):
    shapes = [(10, 4, "random"), (8, 0, "equal"), (13, 0, "random"), (12, 4, "zero")][:n_scans]
    scans = [ScanSpec(dev, *sh, seed=i) for i, sh in enumerate(shapes)]
    _run(dev, 2053, [ArenaSpec(16, 300, 151), ArenaSpec(6, 173, 90)], advance=1, t0=0, scans=scans, what=f"{n_scans} scans riding")


@pytest.mark.parametrize("n_scans", [1, 4])
def test_scans_beside_dense_and_arenas_three_calls(dev, n_scans):
    _scans_beside_case(dev, n_scans)


# ---- alignment --------------------------------------------------------------------------------------------------------------------
def _unaligned_case(dev):
    """A base 4 bytes off a 16-byte boundary is refused wherever the entry would load float4s, and nothing is written."""
    lib = L()
    _refused(dev, 1025, [], advance=0, dense_shift=1, what="shifted dense buffer")
    _refused(dev, 1025, [ArenaSpec(6, 40, 20), ArenaSpec(16, 130, 65, shift=1)], advance=1, what="shifted K = 16 arena")
    _refused(dev, 0, [ArenaSpec(12, 130, 65, shift=1)], advance=0, what="shifted K = 12 arena")
    rows, K = 130, 16
    sp = ArenaSpec(K, rows, 65, decoy=True, shift=1)
    w = World(dev, None, [sp], 7)
    w.set_grads(None, [sp.grad(1)])
    w.lr_t.fill_(0.001)
    snap = w.snapshot()
    live = torch.ones(rows + 2, dtype=torch.uint8, device=dev)
    bufs = w.a[0]
    with pytest.raises(_lib.RecalgoError, match=REFUSED):
        lib.recalgo_adam_tf1_dense(*map(P, bufs), rows * K, 0.0, P(w.lr_t), B1, B2, EPS, 1, _stream())
    with pytest.raises(_lib.RecalgoError, match=REFUSED):
        lib.recalgo_adam_tf1_rows(*map(P, bufs), P(live), rows, K, 0.0, P(w.lr_t), B1, B2, EPS, 1, _stream())
    with pytest.raises(_lib.RecalgoError, match=REFUSED):
        lib.recalgo_adam_tf1_list(*map(P, bufs), P(w.lists[0]), P(w.counts[0]), rows, K, 0.0, P(w.lr_t), B1, B2, EPS, 1, _stream())
    torch.cuda.synchronize()
    w.assert_unchanged(snap, "shifted base at the separate entries")


def test_a_base_that_is_not_16_byte_aligned_is_refused(dev):
    _unaligned_case(dev)


# ---- f. once more behind fences, and a sweep --------------------------------------------------------------------------------------
def test_cases_under_the_redzone_guard(dev):
    """tests/test_gpu_redzone.py cannot list a new module.  Every helper above except the graph capture once more inside guarded():
    each buffer comes from Tensor.to, torch.full or torch.zeros, so it lies between 0xFF fences of its own."""
    groups = [
        lambda: [_dense_case(dev, n, z) for n in DENSE_N for z in (0, 1)],
        lambda: [_counter_case(dev, t0, 1) for t0 in STEP_STARTS] + [_counter_case(dev, 9, 0), _no_ticket_case(dev)] +
                [_empty_case(dev, w, a) for w in ("no arenas", "max_rows 0 only", "one scan") for a in (0, 1)],
        lambda: [_mixed_case(dev, h) for h in (0, 1)] + [_width_case(dev, K, c) for K in sorted(ARM_ROWS) for c in LIVE],
        lambda: [_cap_case(dev, K, rows) for K, rows in CAPS] + [_decoy_case(dev, K) for K in (16, 12, 6)] +
                [_scalar_arm_any_base_case(dev)],
        lambda: [_lazy_case(dev, K) for K in LAZY_K] + [_lazy_beside_plain_case(dev)] +
                [_lazy_refused_case(dev, K) for K in LAZY_REFUSED_K],
        lambda: [_scan_case(dev, nb, cs, kind) for nb, cs in SCAN_SHAPES for kind in SCAN_KINDS] +
                [_scans_beside_case(dev, k) for k in (1, 4)] + [_unaligned_case(dev)],
    ]
    launched = set()
    for run in groups:                               # (a guard per group: its buffers are released with it)
        with guarded() as g:
            run()
            assert g.records, "the buffers were not allocated under the guard"
            launched |= g.launched
    assert {"recalgo_adam_tf1_step", "recalgo_adam_tf1_step_plans", "recalgo_adam_tf1_advance", "recalgo_adam_tf1_dense",
            "recalgo_adam_tf1_list"} <= launched


# (the SWEEP settings of tests/test_gpu_dense_abi.py)
SWEEP = settings(max_examples=25, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
_arena_st = st.tuples(st.sampled_from(sorted(ARM_ROWS)), st.floats(0.0, 1.0), st.booleans())
_scan_st = st.tuples(st.sampled_from((8, 10, 12, 13)), st.sampled_from((0, 4)), st.sampled_from(SCAN_KINDS))


@SWEEP
@given(n=st.integers(0, 5000), arenas=st.lists(_arena_st, max_size=4), zero_grad=st.sampled_from((0, 1)), advance=st.sampled_from((0, 1)),
       scans=st.lists(_scan_st, max_size=2))
def test_any_launch_against_the_separate_entries(dev, n, arenas, zero_grad, advance, scans):
    specs = []
    for j, (K, frac, lazy) in enumerate(arenas):
        rows = ARM_ROWS[K]
        specs.append(ArenaSpec(K, rows, int(round(frac * rows)), lazy=int(lazy and K in (4, 8, 64, 256)), seed=j))
    _run(dev, n, specs, zero_grad=zero_grad, advance=advance, t0=1, scans=[ScanSpec(dev, *s, seed=i) for i, s in enumerate(scans)],
         absolute=False, what=f"sweep n = {n}, arenas = {arenas}, zero_grad = {zero_grad}, advance = {advance}, scans = {scans}")
