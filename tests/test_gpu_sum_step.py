"""-m gpu: recalgo_adam_tf1_sum_step (csrc/tail.hip, sums_adam_tf1_step_kernel) — the step's deferred gradient sums and the dense
optimizer update as one launch — against the two launches it replaces, bit for bit:

    path A   recalgo_dense_bwd_weights_reduce(jobs, sums, step_dev), then recalgo_adam_tf1_step_plans(advance = 0)
    path B   recalgo_adam_tf1_sum_step(advance = 1) over the same jobs

Both paths own a copy of one flat p / g / m / v buffer that holds several "layers"; recalgo_dense_bwd_weights(defer = 1) leaves
real slabs in each path's workspaces.  What is compared after each of two consecutive steps, with torch.equal: p, m, v, the
gradient buffer, the loss-like value outside the buffer and the step counter.

| arm of the launch                                                    | how it is reached                                         |
|----------------------------------------------------------------------|-----------------------------------------------------------|
| float4 sums, two splits / more than two                              | (200, 64, 64) / (4096, 64, 64)                            |
| one float per thread, N odd, outputs at odd offsets of the buffer    | (200, 20, 13), dw one float behind a 16-byte boundary     |
| tall sums with / without the 8-wide unrolled body                    | 512 partial rows x 7 columns / 3 rows x 5 columns         |
| a sum whose output is no gradient (the loss value): only summed      | 512 rows x 1 column into a tensor of its own              |
| elements no job writes: whole words, words cut by a job's output     | the gaps between the layers, g random there               |
| inert words (g = m = v = 0) inside a job's output and outside        | zero columns of the upstream gradient / of the partials   |
| no jobs; n = 0 with one plan scan                                    | against recalgo_adam_tf1_step_plans(advance = 1)          |
| refusals: output outside the buffer, overlapping outputs, side in it | recalgo_adam_tf1_sum_step_supported == 0, nothing written |

In the step (AdamOptimizer.apply_gradients): DCN and DeepFM (BatchNorm) at B = 256, 4 fields x emb 16, hidden 64,32,16 — eager
and captured, ops.sum_step_enabled on and off: four runs of three steps, bit-equal, and ops.sum_step_stats shows that the
one launch ran where the switch is on."""
import ctypes

import pytest
import torch

from recalgorithm_amd import _lib, ops
from tests.test_gpu_adam_step_abi import ScanSpec

pytestmark = pytest.mark.gpu

_Split, _ColSum, _Arena, _Scan = (_lib.STRUCTS[n] for n in ("recalgo_dense_split_t", "recalgo_colsum_t", "recalgo_adam_arena_t",
                                                            "recalgo_plan_scan_t"))
LR, B1, B2, EPS = 0.005, 0.9, 0.999, 1e-8


def _ticket(dev):
    return torch.zeros(ops.sum_step_ticket_ints(), dtype=torch.int32, device=dev)


def _armed(ticket):
    """The arrival words (the first 9 of the buffer's 11 lines) read zero; behind them the launch keeps the next step's lr_t."""
    return not bool(ticket.cpu()[: ticket.numel() // 11 * 9].any())

REFUSED = r"failed with hipError_t=1$"             # hipErrorInvalidValue

LAYERS = [(200, 64, 64), (200, 20, 13), (4096, 64, 64)]
TALL = [(512, 7), (3, 5)]                          # (partial rows, columns)


def L():
    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _up4(i):
    return (i + 3) // 4 * 4


class Layout:
    """Where every output lies in the flat buffer: per layer dw then dbias (the scalar layer one float behind a 16-byte boundary,
    its dbias right behind its dw), then the tall sums' outputs; 6-9 floats of gap in front of each, and a 5-float tail."""

    def __init__(self):
        at, self.dw, self.db, self.tall = 8, [], [], []
        for M, K, N in LAYERS:
            vec = N % 4 == 0
            at = _up4(at) + (0 if vec else 1)
            self.dw.append(at)
            at += K * N
            at = _up4(at) if vec else at
            self.db.append(at)
            at += N + 6
        for rows, cols in TALL:
            at += 3
            self.tall.append(at)
            at += cols + 6
        self.n = at + 5
        covered = torch.zeros(self.n, dtype=torch.bool)
        for (M, K, N), a, b in zip(LAYERS, self.dw, self.db):
            covered[a:a + K * N] = True
            covered[b:b + N] = True
        for (rows, cols), a in zip(TALL, self.tall):
            covered[a:a + cols] = True
        self.covered = covered


class Inputs:
    """Host inputs of one step: x, gy per layer (columns 4..7 of gy zero: whole inert words of dw and of dbias), the partial rows
    of the tall sums (column 1 zero), the gradient of the elements no job writes (every third word zero)."""

    def __init__(self, lay, step, seed):
        gen = torch.Generator().manual_seed(1000 * seed + step)
        self.x, self.gy = [], []
        for M, K, N in LAYERS:
            self.x.append(torch.randn(M, K, generator=gen))
            gy = torch.randn(M, N, generator=gen) * (0.1 * step)
            gy[:, 4:8] = 0.0
            self.gy.append(gy)
        self.partials = []
        for rows, cols in TALL:
            part = torch.randn(rows, cols + 2, generator=gen)          # (column 0: not summed; the last one: the "loss")
            part[:, 2] = 0.0
            self.partials.append(part)
        g = torch.randn(lay.n, generator=gen)
        g.view(-1)[: lay.n // 12 * 12].view(-1, 12)[:, 8:] = 0.0
        self.g_rest = g


class Side:
    """One path's device state."""

    def __init__(self, dev, lay, seed, jobs=True):
        gen = torch.Generator().manual_seed(seed)
        self.lay, self.dev = lay, dev
        p, m, v = torch.randn(lay.n, generator=gen), torch.randn(lay.n, generator=gen) * 0.1, torch.rand(lay.n, generator=gen) * 0.01
        # inert words: the zero columns of the layers' gradients and of the tall sums, a third of the rest
        z = torch.zeros(lay.n, dtype=torch.bool)
        for (M, K, N), a, b in zip(LAYERS, lay.dw, lay.db):
            cols = torch.zeros(K, N, dtype=torch.bool)
            cols[:, 4:8] = True
            z[a:a + K * N] = cols.view(-1)
            z[b + 4:b + 8] = True
        for (rows, cols), a in zip(TALL, lay.tall):
            z[a + 1] = True
        rest = torch.zeros(lay.n // 12 * 12, dtype=torch.bool).view(-1, 12)
        rest[:, 8:] = True
        z[: rest.numel()] |= rest.view(-1) & ~lay.covered[: rest.numel()]
        m[z], v[z] = 0.0, 0.0
        self.p, self.m, self.v = p.to(dev), m.to(dev), v.to(dev)
        self.g = torch.full((lay.n,), float("nan"), device=dev)
        self.loss = torch.full((1,), float("nan"), device=dev)
        self.step = torch.full((1,), 7, dtype=torch.int64, device=dev)
        self.ticket = _ticket(dev)
        self.ws = []
        if jobs:
            for M, K, N in LAYERS:
                nbytes = int(L().recalgo_dense_bwd_weights_workspace_bytes(M, K, N))
                self.ws.append(torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dev))
        assert all(t.data_ptr() % 16 == 0 for t in (self.p, self.g, self.m, self.v))

    def feed(self, inp):
        """This step's gradient where no job writes, and the deferred work of the backward pass: the slabs, the partial rows."""
        lay = self.lay
        g = torch.where(lay.covered, torch.full((lay.n,), float("nan")), inp.g_rest)     # (a job's output: NaN until it is summed)
        self.g.copy_(g)
        self.keep = [[t.to(self.dev) for t in ts] for ts in (inp.x, inp.gy, inp.partials)]
        xs, gys, _ = self.keep
        for (M, K, N), x, gy, ws, a, b in zip(LAYERS, xs, gys, self.ws, lay.dw, lay.db):
            dw, db = self.g[a:a + K * N], self.g[b:b + N]
            L().recalgo_dense_bwd_weights(P(x), K, P(gy), N, None, M, K, N, P(dw), P(db), P(ws), 1, _stream())

    def job_arrays(self, side_in_sums):
        lay = self.lay
        jobs = (_Split * len(LAYERS))()
        for i, ((M, K, N), ws, a, b) in enumerate(zip(LAYERS, self.ws, lay.dw, lay.db)):
            jobs[i] = _Split(M, K, N, ws.data_ptr(), self.g[a:].data_ptr(), self.g[b:].data_ptr())
        parts = self.keep[2]
        cs = [_ColSum(part[:, 1:].data_ptr(), self.g[a:].data_ptr(), rows, cols + 2, cols)
              for (rows, cols), part, a in zip(TALL, parts, lay.tall)]
        loss = [_ColSum(parts[0][:, TALL[0][1] + 1:].data_ptr(), self.loss.data_ptr(), TALL[0][0], TALL[0][1] + 2, 1)]
        if side_in_sums:
            cs, loss = cs + loss, []
        return jobs, (_ColSum * max(len(cs), 1))(*cs), len(cs), (_ColSum * max(len(loss), 1))(*loss), len(loss)

    def tensors(self):
        return {"p": self.p, "g": self.g, "m": self.m, "v": self.v, "loss": self.loss, "step": self.step}


def _two_launches(s, zero_grad, jobs=True, scans=()):
    recs = (_Scan * len(scans))(*[c.record() for c in scans]) if scans else None
    if jobs:
        ja, cs, ncs, _, _ = s.job_arrays(side_in_sums=True)
        L().recalgo_dense_bwd_weights_reduce(ja, len(LAYERS), cs, ncs, P(s.step), _stream())
    else:
        L().recalgo_dense_bwd_weights_reduce((_Split * 1)(), 0, (_ColSum * 1)(), 0, P(s.step), _stream())
    n = s.p.numel()
    L().recalgo_adam_tf1_step_plans(P(s.p) if n else None, P(s.g) if n else None, P(s.m) if n else None, P(s.v) if n else None, n,
                                    None, 0, P(s.step), None, 0, LR, B1, B2, EPS, zero_grad, recs, len(scans), _stream())


def _one_launch(s, zero_grad, jobs=True, scans=()):
    recs = (_Scan * len(scans))(*[c.record() for c in scans]) if scans else None
    if jobs:
        ja, cs, ncs, side, nside = s.job_arrays(side_in_sums=False)
        nj = len(LAYERS)
        assert L().recalgo_adam_tf1_sum_step_supported(P(s.g), s.p.numel(), ja, nj, cs, ncs, side, nside) == 1
    else:
        ja, cs, side, nj, ncs, nside = None, None, None, 0, 0, 0
    n = s.p.numel()
    L().recalgo_adam_tf1_sum_step(P(s.p) if n else None, P(s.g) if n else None, P(s.m) if n else None, P(s.v) if n else None, n,
                                  None, 0, P(s.step), P(s.ticket), 1, LR, B1, B2, EPS, zero_grad, recs, len(scans),
                                  ja, nj, cs, ncs, side, nside, _stream())


def _assert_equal(a, b, what):
    torch.cuda.synchronize()
    ta, tb = a.tensors(), b.tensors()
    for k in ta:
        x, y = ta[k].cpu(), tb[k].cpu()
        assert not torch.isnan(x.float()).any(), f"{what}: {k} of the two launches holds a NaN (an element nobody wrote)"
        assert torch.equal(x, y), f"{what}: {k} differs ({int((x != y).sum())} of {x.numel()} elements)"


@pytest.mark.parametrize("zero_grad", [0, 1])
def test_one_launch_equals_sum_then_step_bit_for_bit(dev, zero_grad):
    """Tests 1 and 2 of the issue: every summation path, covered and uncovered elements, inert words, two consecutive steps."""
    lay = Layout()
    a, b = Side(dev, lay, 3), Side(dev, lay, 3)
    splits = [int(L().recalgo_dense_bwd_weights_workspace_bytes(M, K, N)) // (4 * ((K * N + N + 3) // 4 * 4)) for M, K, N in LAYERS]
    print("splits per layer:", dict(zip(LAYERS, splits)))
    assert max(splits) > 2 and min(splits) >= 2, f"the layers no longer leave slabs / more than two of them: {splits}"
    for step in (1, 2):
        inp = Inputs(lay, step, seed=zero_grad)
        a.feed(inp)
        b.feed(inp)
        _two_launches(a, zero_grad)
        _one_launch(b, zero_grad)
        _assert_equal(a, b, f"zero_grad = {zero_grad}, step {step}")
        assert int(b.step.cpu()) == 7 + step and _armed(b.ticket)
        g = b.g.cpu()
        if zero_grad:
            assert not bool(g.ne(0).any()), "zero_grad left a gradient behind"
        else:
            assert bool(g[lay.covered].ne(0).any()) and torch.equal(g[~lay.covered], inp.g_rest[~lay.covered])
    # the inert words were there, and were skipped: their moments are still zero, the others have moved
    m = b.m.cpu()
    assert bool((m == 0).any()) and bool((m[lay.covered] != 0).any())


@pytest.mark.parametrize("zero_grad", [0, 1])
def test_no_jobs_is_the_plain_optimizer_launch(dev, zero_grad):
    lay = Layout()
    a, b = Side(dev, lay, 5, jobs=False), Side(dev, lay, 5, jobs=False)
    for step in (1, 2):
        g = Inputs(lay, step, seed=9).g_rest
        a.g.copy_(g)
        b.g.copy_(g)
        _two_launches(a, zero_grad, jobs=False)
        _one_launch(b, zero_grad, jobs=False)
        a.loss.zero_()
        b.loss.zero_()
        _assert_equal(a, b, f"no jobs, zero_grad = {zero_grad}, step {step}")


def test_empty_launch_with_one_scan_still_scans_and_advances(dev):
    class Empty:
        def __init__(self):
            self.p = self.g = self.m = self.v = torch.zeros(0, device=dev)
            self.step = torch.full((1,), 41, dtype=torch.int64, device=dev)
            self.ticket = _ticket(dev)
    for t in (1, 2):
        s, scan = Empty(), ScanSpec(dev, 10, 4, "random")
        s.step.fill_(40 + t)
        _one_launch(s, 1, jobs=False, scans=[scan])
        torch.cuda.synchronize()
        assert int(s.step.cpu()) == 41 + t and _armed(s.ticket)
        scan.check(f"empty launch {t}")


def test_jobs_the_launch_cannot_serve_are_refused(dev):
    lay = Layout()
    s = Side(dev, lay, 11)
    s.feed(Inputs(lay, 1, seed=2))
    n = lay.n
    ja, cs, ncs, side, nside = s.job_arrays(side_in_sums=False)
    outside = torch.full((64 * 64 + 64,), float("nan"), device=dev)

    def variants():
        # a. a gradient sum whose output lies outside the flat buffer (the loss among the gradient sums)
        yield "loss among the gradient sums", s.job_arrays(side_in_sums=True)
        # b. a layer whose dw lies outside
        jb = (_Split * len(LAYERS))(*ja)
        jb[0] = _Split(*LAYERS[0], s.ws[0].data_ptr(), outside.data_ptr(), outside[64 * 64:].data_ptr())
        yield "dw outside", (jb, cs, ncs, side, nside)
        # c. an output that straddles the end of the buffer
        c2 = (_ColSum * ncs)(*cs)
        c2[1] = _ColSum(cs[1].partials, s.g[n - 2:].data_ptr(), cs[1].rows, cs[1].row_stride, cs[1].n)
        yield "output across the end", (ja, c2, ncs, side, nside)
        # d. two overlapping outputs
        c3 = (_ColSum * ncs)(*cs)
        c3[1] = _ColSum(cs[1].partials, cs[0].out + 8, cs[1].rows, cs[1].row_stride, cs[1].n)
        yield "overlapping outputs", (ja, c3, ncs, side, nside)
        # e. a side sum inside the buffer
        s2 = (_ColSum * 1)(_ColSum(side[0].partials, s.g[2:].data_ptr(), side[0].rows, side[0].row_stride, 1))
        yield "side sum inside the buffer", (ja, cs, ncs, s2, 1)
        # f. more jobs than the table holds
        many = (_ColSum * 40)(*[_ColSum(cs[1].partials, s.g[4 * i:].data_ptr(), 3, cs[1].row_stride, 1) for i in range(40)])
        yield "40 jobs", ((_Split * 1)(), many, 40, side, nside)

    snap = {k: t.clone() for k, t in s.tensors().items()}
    for what, (j, c, nc, sd, nsd) in variants():
        nj = 0 if what == "40 jobs" else len(LAYERS)
        assert L().recalgo_adam_tf1_sum_step_supported(P(s.g), n, j, nj, c, nc, sd, nsd) == 0, what
        with pytest.raises(_lib.RecalgoError, match=REFUSED):
            L().recalgo_adam_tf1_sum_step(P(s.p), P(s.g), P(s.m), P(s.v), n, None, 0, P(s.step), P(s.ticket), 1, LR, B1, B2, EPS, 1,
                                          None, 0, j, nj, c, nc, sd, nsd, _stream())
    torch.cuda.synchronize()
    for k, t in s.tensors().items():
        x, y = t.cpu(), snap[k].cpu()
        assert torch.equal(torch.nan_to_num(x.float(), nan=-1.0), torch.nan_to_num(y.float(), nan=-1.0)), f"{k} after the refused calls"
    assert not bool(s.ticket.cpu().any()), "the ticket buffer after the refused calls"
    assert L().recalgo_adam_tf1_sum_step_supported(P(s.g), n, ja, len(LAYERS), cs, ncs, side, nside) == 1


# ---- in the step --------------------------------------------------------------------------------------------------------------------
def _estimator(model, dev):
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.estimator import Estimator, RunConfig
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=4, max_vocab=300, seed=5)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)]
    hidden = ["64", "32", "16"]
    if model == "dcn":
        from recalgorithm_amd.algorithm.DCN.dcn import dcn_model_fn as model_fn
        params = {"category_feature_columns": [fc.embedding_column(c, 16) for c in cats], "dense_feature_columns": [],
                  "hidden_units": hidden, "num_cross_layer": 3, "learning_rate": 0.005}
    else:
        from recalgorithm_amd.algorithm.DeepFM.deepfm import deepfm_model_fn as model_fn
        cats = sorted(cats, key=lambda c: c.key)
        params = {"first_order_feature_columns": [fc.indicator_column(c) for c in cats],
                  "second_order_feature_columns": [fc.embedding_column(c, 16) for c in cats],
                  "hidden_units": hidden, "dropout_rate": 0.0, "batch_norm": True, "learning_rate": 0.005}
    est = Estimator(model_fn, params, RunConfig(device=dev))
    batches = [synth.device_features(spec, 256, dev, batch_index=i)[:2] for i in range(3)]
    est.build(*batches[0])
    return est, batches


def _state(est, losses):
    torch.cuda.synchronize()
    out = {f"loss of step {i}": l.cpu() for i, l in enumerate(losses)}
    out.update({f"var {k}": v.detach().cpu().clone() for k, v in est.store.named_arrays().items()})
    for n, ar in est.store.arenas.items():
        out[f"arena {n}.m"], out[f"arena {n}.v"] = ar.m.cpu().clone(), ar.v.cpu().clone()
    out["flat_m"], out["flat_v"] = est.store.flat_m.cpu().clone(), est.store.flat_v.cpu().clone()
    out["flat_grad"] = est.store.flat_grad.cpu().clone()
    out["step counter"] = est.store.opt_state["step"].cpu().clone()
    return out


def _three_steps(model, dev, captured):
    from recalgorithm_amd.estimator import GraphedTrainStep
    est, batches = _estimator(model, dev)
    if captured:                                        # one eager warm-up step, the capture, two replays
        g = GraphedTrainStep(est.train_step, *batches[0], warmup=1)
        losses = [g(*batches[i]).clone() for i in (1, 2)]
    else:
        losses = [est.train_step(*batches[i]).clone() for i in range(3)][1:]
    return _state(est, losses)


@pytest.fixture
def switch():
    before = ops.sum_step_enabled
    yield
    ops.sum_step_enabled = before


@pytest.mark.parametrize("model", ["dcn", "deepfm"])
def test_training_steps_are_the_same_with_and_without_the_one_launch(dev, model, switch):
    runs = {}
    for on in (False, True):
        for captured in (False, True):
            ops.sum_step_enabled = on
            before = dict(ops.sum_step_stats)
            runs[on, captured] = _three_steps(model, dev, captured)
            ran = ops.sum_step_stats["fused"] - before["fused"]
            # eager: three steps; captured: the warm-up step and the capture
            assert ran == (0 if not on else (2 if captured else 3)), f"{model}, switch {on}, captured {captured}: {ran} fused launches"
            assert ops.sum_step_stats["refused"] == before["refused"], f"{model}: the entry refused the step's jobs"
    ref = runs[False, False]
    assert int(ref["step counter"]) == 3
    for key, got in runs.items():
        assert got.keys() == ref.keys()
        bad = [k for k in ref if not torch.equal(ref[k], got[k])]
        assert not bad, f"{model}: (switch, captured) = {key} differs from the eager two-launch run in {bad[:8]} ({len(bad)} in all)"


def test_refused_jobs_fall_back_to_the_two_launches(dev, switch, monkeypatch):
    """Two outputs overlap (a column sum queued twice) / a layer's dw lies outside the flat buffer: apply_gradients runs the sum
    launch and the optimizer launch, with the result of a run that never tried the one launch."""
    ops.sum_step_enabled = False
    ref = _three_steps("dcn", dev, False)
    ops.sum_step_enabled = True
    take = ops.take_dense_splits
    for what in ("overlap", "outside"):
        def tampered(what=what):
            dense, colsums = take()
            if what == "overlap":
                inside = [c for c in colsums if c[4] > 1]
                return dense, colsums + [inside[0]]
            M, K, N, ws, dw, dbias = next(d for d in dense if L().recalgo_dense_bwd_weights_workspace_bytes(*d[:3]) > 0)
            extra = torch.empty(K * N + N, device=dw.device)
            return dense + [(M, K, N, ws, extra[:K * N].view(K, N), extra[K * N:])], colsums
        monkeypatch.setattr(ops, "take_dense_splits", tampered)
        before = dict(ops.sum_step_stats)
        got = _three_steps("dcn", dev, False)
        monkeypatch.setattr(ops, "take_dense_splits", take)
        assert ops.sum_step_stats["fused"] == before["fused"] and ops.sum_step_stats["refused"] == before["refused"] + 3, what
        bad = [k for k in ref if not torch.equal(ref[k], got[k])]
        assert not bad, f"{what}: the fallback differs from the two launches in {bad[:8]}"
