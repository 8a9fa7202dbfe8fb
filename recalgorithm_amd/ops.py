"""Torch-tensor level wrappers around the C-ABI (include/recalgo.h).

PyTorch is plumbing here: device memory, the current HIP stream, and autograd to chain the
activation gradients between the hand-written kernels.  All arithmetic of the hot path runs in
librecalgo_hip.so; there is no CPU or eager fallback — tensors must live on a HIP device.

Parameter gradients are written by the kernels directly into `Variable.grad` /
`EmbeddingArena.grad` (see variables.py); the autograd Functions return None for them.
"""
from __future__ import annotations

import ctypes
from typing import Callable, NamedTuple, Optional, Tuple

import torch
from torch.autograd import Function

from . import _lib, sparse
from .variables import EmbeddingArena, Variable, VariableStore

_C = _lib.CONSTANTS                          # the RECALGO_* #defines of include/recalgo.h
_ACT = {"prelu": _C["RECALGO_ACT_PRELU"], "dice": _C["RECALGO_ACT_DICE"]}
_ACT_NONE = _C["RECALGO_ACT_NONE"]
# the structs of include/recalgo.h (ctypes classes derived from the header, fields in its order)
_Live, _ColSum, _DenseSplit = (_lib.STRUCTS[n] for n in ("recalgo_live_t", "recalgo_colsum_t", "recalgo_dense_split_t"))
_CDrop, _AdamArena = _lib.STRUCTS["recalgo_dropout_t"], _lib.STRUCTS["recalgo_adam_arena_t"]


def _lib_():
    return _lib.load()


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t: torch.Tensor):
    if not t.is_cuda:
        raise _lib.RecalgoError(
            "recalgo ops run only on a HIP device (no CPU fallback); got a CPU tensor")
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def copy_bytes(dst: torch.Tensor, src: torch.Tensor) -> None:
    """dst <- src for two contiguous device tensors of the same byte length on one device (recalgo_copy_bytes)."""
    n = dst.numel() * dst.element_size()
    if n != src.numel() * src.element_size() or not dst.is_contiguous() or not src.is_contiguous() or dst.device != src.device:
        raise ValueError("copy_bytes: contiguous tensors of equal byte length on one device")
    _lib_().recalgo_copy_bytes(_p(dst), _p(src), n, _stream(dst))


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")


_ws_cache = {}


# Work a training step leaves for a later launch of the same step: what each entry holds, who fills it, who drains it.  The
# first two are drained inside the forward / backward that filled them; the rest by the optimizer's nn.apply_parked_grads
# -> flush_dense_splits().  A step whose backward stopped with an exception is never drained: discard_step_work() drops all
# of it when the next forward begins.
_lazy_gathers: list = []     # (out, ids, arena, row_base): embedding_gather inside gather_feeds_cross; taken by cross_stack,
#                              or launched by flush_lazy_gathers()
_cross_rider = None          # (cross node, g): the CrossNet backward the fused tail hands over early (defer_cross_rider); taken
#                              by the next deferred dense_bwd without a GradJoin, or cleared by the node's own backward
_wgrad_rider = None          # (x, g, dw, dbias): the fused tail's weight gradient (defer_wgrad_rider); taken by the next deferred
#                              dense_bwd over the same batch, or launched on its own by launch_wgrad_rider() (flush, next rider)
_dense_pending = []          # (M, K, N, ws, dw, dbias): split reductions of dense_bwd / dense_bwd_weights(defer=True)
_colsum_pending = []         # (partials, element offset, rows, row_stride, n, out): plain column sums of partial rows
_dlogit_partials = {}        # dlogit.data_ptr() -> (partials, column, rows, row_stride, B): the loss tail's sums of
#                              d(loss)/d(logit), read by colsum_of_dlogit
_parked_l2 = []              # (variable, scale, g): nn.l2_regularization's backward; added by nn.apply_parked_grads


def discard_step_work() -> None:
    """Drop the deferred work of a step that never reached its drain.  Launches nothing: nobody reads the outputs of a
    dropped gather or sum (VariableStore.begin_call: a model_fn invocation starts)."""
    global _wgrad_rider, _cross_rider
    _lazy_gathers.clear()
    _wgrad_rider = _cross_rider = None
    _dense_pending.clear()
    _colsum_pending.clear()
    _dlogit_partials.clear()
    _parked_l2.clear()
    _bst_shared.clear()


def anchor_store(anchor):
    """The VariableStore whose autograd anchor was passed to a lookup (its optimizer state holds the step counter the
    deferred-Adam catch-up needs)."""
    return getattr(anchor, "_recalgo_store", None)


def _flush(arena) -> None:
    """Row-sharded deployment (parallel.py): the kernel scattered into a staged gradient; send it
    to the rows' owners now."""
    f = getattr(arena, "flush_grad", None)
    if f is not None:
        f()


def mark_live_rows(arena, ids: torch.Tensor, row_base: Optional[torch.Tensor], F: int) -> None:
    """Record the rows a scatter has just touched in the arena's live-row list (first touch only)."""
    if not getattr(arena, "tracks_live_rows", False):
        return
    live, lst, cnt = arena.live_state()
    _lib_().recalgo_mark_live_rows(_p(ids), _p(row_base), ids.numel(), int(F), _p(live), _p(lst), _p(cnt), _stream(ids))


def _live(arena, row_offset: int = 0):
    """recalgo_live_t* of the arena's live-row bookkeeping (the scatter kernels mark the rows they flush), or None
    for arenas without it (row-sharded staging buffers: their owners mark on receipt)."""
    if not getattr(arena, "tracks_live_rows", False):
        return None
    live, lst, cnt = arena.live_state()
    return ctypes.byref(_Live(live.data_ptr(), lst.data_ptr(), cnt.data_ptr(), int(row_offset)))


def scatter_rows_sorted(arena, rows: torch.Tensor, vals: torch.Tensor) -> None:
    """arena.grad[rows[i], :] += vals[i, :] (rows < 0 skipped), deterministically (stable sort + ordered segment sums); the
    rows join the live list.  Only for an arena that is NOT on the owner-computes path while its partner in a fused lookup is
    (DeepFM's two arenas, one of them frozen or of an unsupported width)."""
    rows = rows.reshape(-1).contiguous()
    vals = vals.reshape(rows.numel(), -1).contiguous()
    srt, perm = torch.sort(rows, stable=True)
    _lib_().recalgo_scatter_rows_sorted(_p(srt), _p(perm), _p(vals), rows.numel(), vals.shape[1], _p(arena.grad), _stream(vals))
    mark_live_rows(arena, rows, None, 1)


def _staged(arena, rows: torch.Tensor, store=None):
    """(plan, staged arena, identity ids [M]) for a row-sharded arena, or None when the arena is local.  `store`: the
    owner side of the exchange joins the shard's owner-computes plan (sparse.py) when the call is a TRAIN forward."""
    sd = getattr(arena, "sharding", None)
    if sd is None:
        return None
    from . import parallel
    if store is not None and getattr(store, "data_dependent", None) is None and rows.dim() == 1:
        # (a bag or a history looked up in a row-sharded arena: the exchange plan is made from the batch's rows)
        store.data_dependent = "a row-sharded arena stages a ragged lookup's rows per batch (ops._staged)"
    plan = sd.plan(rows)
    return plan, parallel.StagedArena(plan, arena, store, torch.is_grad_enabled()), plan.staged_ids(rows, rows.shape)


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Per-device grow-only scratch (allocated outside graph capture on first use)."""
    key = (device.type, device.index)
    w = _ws_cache.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = w
    return w


def _contig(t: Optional[torch.Tensor]):
    """t itself where it is contiguous (or None), else a contiguous copy"""
    return t if t is None or t.is_contiguous() else t.contiguous()


# ---- Parameters of a fused layer: Variable or tensor --------------------------------------------------------------------------
# The one statement of the convention of bst_attention, bst_ffn, afm_attention, autoint_layer, dcnv2_layer, flen_interaction,
# dien_gru and dien_evolve.  Each parameter is a Variable or a plain tensor; an optional one (AutoInt's wres, DCN-V2's gate) may
# be None.  The kernel writes a Variable's gradient into Variable.grad, OVERWRITING it, and autograd receives None for it; a
# tensor's gradient goes to a new buffer that autograd receives.  The wrapper calls
#     Fn.apply(anchor, inputs.., flags.., params, *_param_tail(params))
# `anchor` (VariableStore.anchor | None) makes the node differentiable when every parameter is a Variable; autograd does not look
# into the list `params`, so the tail shows it the tensors.  forward: ts, vs = _split_params(params).  backward: outs =
# _grad_buffers(ts, vs), the launch, return _param_returns(ctx, {position among forward's arguments: input gradient}, outs, vs).
def _split_params(params):
    """-> (the tensors the kernels read, the Variables | None), each as long as params; an absent parameter is None in both"""
    return [p.data if isinstance(p, Variable) else p for p in params], [p if isinstance(p, Variable) else None for p in params]


def _param_tail(params):
    """the `*tensors` of Function.apply: params with None where it holds a Variable (or nothing)"""
    return [None if isinstance(p, Variable) else p for p in params]


def _grad_buffers(ts, vs):
    """per parameter, the buffer the kernel writes its gradient to: Variable.grad, a new tensor, None for an absent one"""
    return [v.grad if v is not None else t if t is None else torch.empty_like(t) for t, v in zip(ts, vs)]


def _param_returns(ctx, input_grads: dict, outs, vs) -> tuple:
    """What backward returns, one slot per argument of forward (ctx.needs_input_grad counts them; the last len(vs) are the tail):
    None before the tail except the input_grads that are needed; in the tail a tensor parameter's buffer, None for a Variable."""
    need = ctx.needs_input_grad
    head = [None] * (len(need) - len(vs))
    for i, g in input_grads.items():
        if need[i]:
            head[i] = g
    return (*head, *[None if v is not None else o for o, v in zip(outs, vs)])


def _check_param_shapes(what: str, ts, shapes, names, chk: bool = False) -> None:
    """Every present parameter has its shape, else ValueError; chk: each goes through _chk (float32, contiguous) first."""
    for t, shape, name in zip(ts, shapes, names):
        if t is not None and chk:
            _chk(t, torch.float32, f"{what}: {name}")
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {shape}")


def _check_fp32_on_device(what: str, ts, names) -> None:
    """Every present tensor is contiguous float32 on the HIP device of the first one (the layer's input), else ValueError."""
    for t, name in zip(ts, names):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.device != ts[0].device):
            owner = names[0] + ("'" if names[0].endswith("s") else "'s")
            raise ValueError(f"{what}: {name} must be a contiguous float32 tensor on {owner} device, got {t.dtype} on {t.device}"
                             f"{', not contiguous' * (not t.is_contiguous())}")


# =============================================================================================
# K1: embedding gather
# =============================================================================================
# A gather whose output the cross network consumes next (DCN, dcn.py:152-160) is not launched: CrossNet's forward kernel
# fetches the rows itself and writes x0 on the way (recalgo_gather_cross_fwd).  `gather_feeds_cross` is the model's promise;
# anything that is still pending when another consumer could read the tensor is launched by flush_lazy_gathers().
LAZY_GATHER = True                           # module hook (tests / A-B): False = every gather is its own launch
_lazy_gather_on = False
_lazy_hit = False


class gather_feeds_cross:
    """with ops.gather_feeds_cross() as lz: x = fc.input_layer(...); lz.keep(x) — the single-launch gathers issued inside stay
    pending only if exactly one was issued and `x` IS its output (one width, no bags, no concat); else they run now."""

    def __enter__(self):
        global _lazy_gather_on
        self._prev, _lazy_gather_on = _lazy_gather_on, bool(LAZY_GATHER)
        self._kept = False
        return self

    def keep(self, x) -> None:
        self._kept = (len(_lazy_gathers) == 1 and isinstance(x, torch.Tensor) and _lazy_gathers[0][0] is x)

    def __exit__(self, *exc):
        global _lazy_gather_on
        _lazy_gather_on = self._prev
        if not self._kept:
            flush_lazy_gathers()
        return False


def flush_lazy_gathers() -> None:
    while _lazy_gathers:
        out, ids, arena, row_base = _lazy_gathers.pop()
        out._recalgo_lazy_gather = None
        B, F = ids.shape
        _lib_().recalgo_embedding_gather_fwd(_p(ids), _p(arena.weight), _p(row_base), B, F, arena.K, _p(out), F * arena.K, 0,
                                             _stream(ids))


def _take_lazy_gather(x0: torch.Tensor):
    """The pending gather whose output is x0 (-> (ids, arena, row_base)), or None; any OTHER pending gather is launched."""
    lz = getattr(x0, "_recalgo_lazy_gather", None)
    if lz is not None:
        for i, ent in enumerate(_lazy_gathers):
            if ent[0] is x0:
                _lazy_gathers.pop(i)
                break
        x0._recalgo_lazy_gather = None
    flush_lazy_gathers()
    return lz


class _GatherFn(Function):
    @staticmethod
    def forward(ctx, anchor, ids, arena: EmbeddingArena, row_base, training=False, lazy_ok=False):
        B, F = ids.shape
        K = arena.K
        out = torch.empty(B, F * K, device=ids.device, dtype=torch.float32)
        # owner-computes scatter (sparse.py): the lookup joins the arena's plan; deferred-Adam rows are caught up first
        ctx.src = sparse.begin_lookup(arena, anchor_store(anchor), ids, None, row_base, 0, B, F, training, can_defer=True)
        # deferred Adam: a registered (TRAIN) lookup's rows were just caught up; any other lookup reads lagging rows as of now
        dv, stp = sparse.view_for(ctx.src, arena, anchor_store(anchor))
        ctx.arena, ctx.ids, ctx.row_base = arena, ids, row_base
        # (lazy_ok: only the plain lookup of embedding_gather() may be left to its consumer — not the staged rows of a sharded arena)
        batched = ctx.src is not None and getattr(ctx.src, "deferred", False)       # (sparse.batch_lookups: prepare work pending)
        ctx.lazy = (lazy_ok and _lazy_gather_on and not batched and dv is None and K % 4 == 0 and F * K <= 1024
                    and ids.is_contiguous())
        if ctx.lazy:
            global _lazy_hit
            _lazy_hit = True                 # (embedding_gather() hangs the pending launch on the tensor autograd hands out)
            return out

        def launch():
            _lib_().recalgo_embedding_gather_fwd_deferred(
                _p(ids), _p(arena.weight), _p(row_base), B, F, K, _p(out), F * K, 0, dv, stp, 0, _stream(ids))
        if batched:
            # behind the block's one `prepare` launch (the rows it catches up are read here); a plain lookup: it may share its
            # launch with the block's other plain lookups
            job = (0, ids, row_base, arena.weight, B, F, K, out, F * K, 0, None) if (dv is None and ids.is_contiguous()) else None
            sparse.defer_launch(launch, job)
        else:
            launch()
        return out

    @staticmethod
    def backward(ctx, g):
        ids, arena = ctx.ids, ctx.arena
        B, F = ids.shape
        if ctx.src is not None:
            ctx.src.set_grad(g)              # summed per row (and applied) by the optimizer's recalgo_scatter_apply
            return None, None, None, None, None, None
        g = g.contiguous()
        _lib_().recalgo_embedding_gather_bwd(_p(ids), _p(g), _p(ctx.row_base), B, F, arena.K, F * arena.K, 0, _p(arena.grad),
                                             _live(arena), _stream(ids))
        _flush(arena)
        return None, None, None, None, None, None


def embedding_gather(store: VariableStore, ids: torch.Tensor, arena: EmbeddingArena,
                     row_base: torch.Tensor) -> torch.Tensor:
    """ids [B,F] int64 (id<0 = OOV) -> [B, F*K]; gradient scattered into arena.grad."""
    _chk(ids, torch.int64, "ids")
    _chk(row_base, torch.int64, "row_base")
    if getattr(arena, "sharding", None) is not None:
        from . import parallel
        _, staged, ident = _staged(arena, parallel.global_rows(ids, row_base), store)
        return _GatherFn.apply(store.anchor, ident.reshape(ids.shape), staged, torch.zeros_like(row_base), False)
    global _lazy_hit, _lazy_gather_on
    _lazy_hit = False
    if _lazy_gather_on and _lazy_gathers:
        # a SECOND gather inside gather_feeds_cross(): the outputs are about to be combined by somebody else (input_layer's
        # per-column path + torch.cat), so neither can be x0 of the cross kernel — launch the pending one, go eager from here on
        flush_lazy_gathers()
        _lazy_gather_on = False
    out = _GatherFn.apply(store.anchor, ids, arena, row_base, torch.is_grad_enabled(), True)
    if _lazy_hit:
        _lazy_hit = False
        out._recalgo_lazy_gather = (ids, arena, row_base)
        _lazy_gathers.append((out, ids, arena, row_base))
    return out


class _BagMeanFn(Function):
    @staticmethod
    def forward(ctx, anchor, values, offsets, arena: EmbeddingArena, table_name, training=False):
        B = offsets.numel() - 1
        K = arena.K
        table = arena.table_view(table_name)
        out = torch.empty(B, K, device=values.device, dtype=torch.float32)
        ctx.src = None
        if table_name != "__staged__" and values.numel():
            # one request per bag entry; its gradient row (g[bag] / count) is expanded in the backward
            ctx.src = sparse.begin_lookup(arena, anchor_store(anchor), values, None, None, arena.tables[table_name][0],
                                          values.numel(), 1, training)
        dv, stp = (None, None) if table_name == "__staged__" else sparse.view_for(ctx.src, arena, anchor_store(anchor))
        rb0 = 0 if table_name == "__staged__" else arena.tables[table_name][0]
        _lib_().recalgo_embedding_bag_mean_fwd_deferred(
            _p(values), _p(offsets), _p(table), B, K, _p(out), K, 0, dv, rb0, stp, 0, _stream(offsets))
        ctx.args = (values, offsets, arena, table_name)
        return out

    @staticmethod
    def backward(ctx, g):
        values, offsets, arena, table_name = ctx.args
        B = offsets.numel() - 1
        rb, vocab = arena.tables[table_name]
        g = g.contiguous()
        if ctx.src is not None:
            # one request per bag entry: its gradient row g[bag] / count, one launch, the bag found on the device (no host
            # synchronisation: a step with a bag lookup captures into a hipGraph)
            ctx.src.set_grad(bag_mean_grad_rows(values, offsets, g))
            return None, None, None, None, None, None
        gt = arena.grad[rb:rb + vocab]
        _lib_().recalgo_embedding_bag_mean_bwd(
            _p(values), _p(offsets), _p(g), B, arena.K, arena.K, 0, _p(gt), _live(arena, rb), _stream(offsets))
        _flush(arena)
        return None, None, None, None, None, None


def bag_mean_grad_rows(values: torch.Tensor, offsets: torch.Tensor, g: torch.Tensor, g_col: int = 0, K: Optional[int] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rows [len(values), K]: rows[j] = g[bag of j, g_col : g_col + K] / (valid values of that bag) for an entry j below
    offsets[-1] with values[j] >= 0, zeros for every other row — OOV entries and the -1 tail of a padded Ragged
    (recalgo_bag_mean_grad_rows, include/recalgo_ragged.h).  g: [B, >= g_col + K] fp32 with a contiguous last dimension."""
    _chk(values, torch.int64, "values")
    _chk(offsets, torch.int64, "offsets")
    B = offsets.numel() - 1
    if g.dtype != torch.float32 or g.dim() != 2 or g.shape[0] != B or (g.shape[1] > 1 and g.stride(1) != 1):
        raise ValueError(f"bag_mean_grad_rows: g must be fp32 [B = {B}, C] with a contiguous last dimension, got {tuple(g.shape)} {g.dtype}")
    K = g.shape[1] - g_col if K is None else int(K)
    stride = int(g.stride(0)) if B > 1 else int(g.shape[1])
    rows = torch.empty(values.numel(), K, device=values.device, dtype=torch.float32) if out is None else out
    if out is not None:
        _chk(out, torch.float32, "out")
        if tuple(out.shape) != (values.numel(), K):
            raise ValueError("bag_mean_grad_rows: out must be [len(values), K]")
    _lib_().recalgo_bag_mean_grad_rows(_p(values), _p(offsets), B, values.numel(), _p(g), stride, int(g_col), K, _p(rows),
                                       _stream(offsets))
    return rows


def ragged_pad(values: torch.Tensor, capacity: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [capacity]: `values` followed by -1 up to the capacity, one launch (recalgo_ragged_pad); `out`: an existing
    buffer of that size — a captured step's static `values`."""
    _chk(values, torch.int64, "values")
    n, capacity = values.numel(), int(capacity)
    if n > capacity:
        raise ValueError(f"ragged_pad: {n} values do not fit a capacity of {capacity}")
    dst = torch.empty(capacity, device=values.device, dtype=torch.int64) if out is None else out
    if out is not None:
        _chk(out, torch.int64, "out")
        if out.numel() != capacity or out.device != values.device:
            raise ValueError("ragged_pad: out must hold exactly `capacity` int64 values on the device of `values`")
    _lib_().recalgo_ragged_pad(_p(values) if n else None, n, _p(dst), capacity, _stream(dst))
    return dst


def embedding_bag_mean(store, values, offsets, arena, table_name) -> torch.Tensor:
    _chk(values, torch.int64, "values")
    _chk(offsets, torch.int64, "offsets")
    if getattr(arena, "sharding", None) is not None:
        rows = torch.where(values >= 0, values + arena.tables[table_name][0], torch.full_like(values, -1))
        _, staged, ident = _staged(arena, rows, store)
        return _BagMeanFn.apply(store.anchor, ident, offsets, staged, "__staged__", False)
    return _BagMeanFn.apply(store.anchor, values, offsets, arena, table_name, torch.is_grad_enabled())


class _SeqGatherFn(Function):
    @staticmethod
    def forward(ctx, anchor, values, offsets, arena: EmbeddingArena, table_name, T, training=False):
        B = offsets.numel() - 1
        K = arena.K
        table = arena.table_view(table_name)
        out = torch.empty(B, T, K, device=offsets.device, dtype=torch.float32)
        seq_len = torch.empty(B, device=offsets.device, dtype=torch.int32)
        ctx.src = None
        if table_name != "__staged__":
            ctx.src = sparse.begin_lookup(arena, anchor_store(anchor), values, offsets, None, arena.tables[table_name][0], B, T, training,
                                          can_defer=True)
        dv, stp = (None, None) if table_name == "__staged__" else sparse.view_for(ctx.src, arena, anchor_store(anchor))
        rb0 = 0 if table_name == "__staged__" else arena.tables[table_name][0]

        def launch():
            _lib_().recalgo_sequence_gather_fwd_deferred(
                _p(values), _p(offsets), _p(table), B, T, K, _p(out), _p(seq_len), dv, rb0, stp, 0, _stream(offsets))
        if ctx.src is not None and getattr(ctx.src, "deferred", False):
            # (sparse.batch_lookups: behind the block's one `prepare` launch, possibly sharing ONE forward launch)
            job = (1, values, offsets, table, B, T, K, out, 0, 0, seq_len) if (dv is None and values.is_contiguous()) else None
            sparse.defer_launch(launch, job)
        else:
            launch()
        ctx.args = (values, offsets, arena, table_name, T)
        ctx.mark_non_differentiable(seq_len)
        ctx.set_materialize_grads(False)      # (else autograd fills a zero "gradient" for seq_len: one launch per lookup and step)
        return out, seq_len

    @staticmethod
    def backward(ctx, g, _gl):
        values, offsets, arena, table_name, T = ctx.args
        B = offsets.numel() - 1
        rb, vocab = arena.tables[table_name]
        if g is None:                          # (the sequence output was not used)
            return None, None, None, None, None, None, None
        if ctx.src is not None:
            ctx.src.set_grad(g)              # (no `arena.grad` access here: reading it would sum the pending sources now)
            return None, None, None, None, None, None, None
        g = g.contiguous()
        gt = arena.grad[rb:rb + vocab]
        _lib_().recalgo_sequence_gather_bwd(
            _p(values), _p(offsets), _p(g), B, T, arena.K, _p(gt), _live(arena, rb), _stream(offsets))
        _flush(arena)
        return None, None, None, None, None, None, None


def sequence_gather(store, values, offsets, arena, table_name, T) -> Tuple[torch.Tensor, torch.Tensor]:
    _chk(values, torch.int64, "values")
    _chk(offsets, torch.int64, "offsets")
    if getattr(arena, "sharding", None) is not None:
        rows = torch.where(values >= 0, values + arena.tables[table_name][0], torch.full_like(values, -1))
        _, staged, ident = _staged(arena, rows, store)
        return _SeqGatherFn.apply(store.anchor, ident, offsets, staged, "__staged__", int(T), False)
    return _SeqGatherFn.apply(store.anchor, values, offsets, arena, table_name, int(T), torch.is_grad_enabled())


# =============================================================================================
# K1+K2+K3: DeepFM sparse path
# =============================================================================================
class _DeepFMSparseFn(Function):
    @staticmethod
    def forward(ctx, anchor, ids, arena: EmbeddingArena, w1: EmbeddingArena, bias: Variable, row_base, training=False):
        B, F = ids.shape
        K = arena.K
        emb = torch.empty(B, F * K, device=ids.device, dtype=torch.float32)
        fm1 = torch.empty(B, 1, device=ids.device, dtype=torch.float32)
        fm2 = torch.empty(B, 1, device=ids.device, dtype=torch.float32)
        fsum = torch.empty(B, K, device=ids.device, dtype=torch.float32)
        st = anchor_store(anchor)
        # the first-order arena is looked up with the same requests: it rides on the embedding arena's plan
        ctx.src, ctx.src1 = sparse.begin_lookup_pair(arena, w1, st, ids, row_base, B, F, training)
        dv, stp = sparse.view_for(ctx.src, arena, st)
        dv1, stp1 = sparse.view_for(ctx.src1, w1, st)
        _lib_().recalgo_deepfm_sparse_fwd_deferred(
            _p(ids), _p(arena.weight), _p(w1.weight), _p(bias.data), _p(row_base), B, F, K,
            _p(emb), _p(fm1), _p(fm2), _p(fsum), dv, dv1, stp if stp is not None else stp1, 0, _stream(ids))
        ctx.args = (ids, arena, w1, bias, row_base)
        ctx.save_for_backward(emb, fsum)
        ctx.set_materialize_grads(False)      # (FwFM never uses fm2: no zero "gradient" is filled for it, one launch less)
        return emb, fm1, fm2

    @staticmethod
    def backward(ctx, g_emb, g_fm1, g_fm2):
        ids, arena, w1, bias, row_base = ctx.args
        emb, fsum = ctx.saved_tensors
        B, F = ids.shape
        no_fm2 = g_fm2 is None
        g_emb = emb.new_zeros(B, F * arena.K) if g_emb is None else g_emb.contiguous()
        g_fm1 = emb.new_zeros(B, 1) if g_fm1 is None else g_fm1.contiguous()
        g_fm2 = (emb.new_zeros(B, 1) if ctx.src is None else None) if no_fm2 else g_fm2.contiguous()
        if ctx.src is not None or ctx.src1 is not None:
            # owner-computes path (sparse.py).  The second-order term's gradient g_emb + g_fm2 * (S - e) (Appendix D "FM2") is
            # the EPILOGUE of the embedding lookup's source: `place` / `apply` form it on load — no [B, F, K] tensor, no
            # elementwise launches.  An arena that is NOT on the owner path (frozen, or an unsupported width) while the
            # other one is keeps the deterministic sorted scatter for itself.
            K = arena.K
            rows = None
            if ctx.src is not None:
                ctx.src.set_grad(g_emb, fm=None if no_fm2 else (g_fm2.reshape(B), fsum, emb))
            elif getattr(arena, "trainable", True):
                rows = torch.where(ids >= 0, ids + row_base.unsqueeze(0), torch.full_like(ids, -1))
                e3, s3 = emb.reshape(B, F, K), fsum.reshape(B, 1, K)
                scatter_rows_sorted(arena, rows, torch.addcmul(g_emb.reshape(B, F, K), g_fm2.reshape(B, 1, 1), s3 - e3))
                _flush(arena)
            if ctx.src1 is not None:
                ctx.src1.set_grad(g_fm1.reshape(B, 1), fmul=0)      # every field of example b adds g_fm1[b] to its w1 row
            elif getattr(w1, "trainable", True):
                if rows is None:
                    rows = torch.where(ids >= 0, ids + row_base.unsqueeze(0), torch.full_like(ids, -1))
                scatter_rows_sorted(w1, rows, g_fm1.reshape(B, 1, 1).expand(B, F, 1))
                _flush(w1)
            if not colsum_of_dlogit(g_fm1, bias.grad.view(1)):      # (TRAIN step: a job of the step's deferred-sum launch)
                torch.sum(g_fm1, dim=0, out=bias.grad.view(1))
            return None, None, None, None, None, None, None
        _lib_().recalgo_deepfm_sparse_bwd(_p(ids), _p(emb), _p(fsum), _p(g_emb), _p(g_fm1), _p(g_fm2), _p(row_base), B, F, arena.K,
                                          _p(arena.grad), _p(w1.grad), _live(arena), _live(w1), _stream(ids))
        _flush(arena)
        _flush(w1)
        torch.sum(g_fm1, dim=0, out=bias.grad.view(1))
        return None, None, None, None, None, None, None


def deepfm_sparse(store, ids, arena, w1_arena, bias, row_base):
    """-> (deep_input [B,F*K], fm_first_order_logit [B,1], fm_second_order_logit [B,1])."""
    _chk(ids, torch.int64, "ids")
    if getattr(arena, "sharding", None) is not None:
        # the first-order arena mirrors the embedding arena's row layout: one exchange plan, two fetches
        from . import parallel
        plan, staged, ident = _staged(arena, parallel.global_rows(ids, row_base), store)
        staged_w1 = parallel.StagedArena(plan, w1_arena, store, torch.is_grad_enabled())
        return _DeepFMSparseFn.apply(store.anchor, ident.reshape(ids.shape), staged, staged_w1, bias,
                                     torch.zeros_like(row_base), False)
    return _DeepFMSparseFn.apply(store.anchor, ids, arena, w1_arena, bias, row_base, torch.is_grad_enabled())


# =============================================================================================
# K4: CrossNet
# =============================================================================================
def _pad4(t: torch.Tensor) -> torch.Tensor:
    """Zero-pad the last dimension to a multiple of 4 (the CrossNet kernels move float4s; the
    reference's default DCN input is d = 82).  Zero columns of x0 / w / b are inert: they add
    nothing to x_l . w_l and produce zero output columns."""
    pad = (-t.shape[-1]) % 4
    return t if pad == 0 else torch.nn.functional.pad(t, (0, pad))


class _CrossFn(Function):
    @staticmethod
    def forward(ctx, anchor, x0, w: Variable, b: Variable, grad_join):
        # w.data, b.data: [L, d].  grad_join: nn.GradJoin shared with the other consumer of x0 (or None).
        ctx.grad_join = grad_join
        B, d = x0.shape
        L = w.data.shape[0]
        lz = _take_lazy_gather(x0)           # x0 not gathered yet (ops.gather_feeds_cross): this kernel fetches the rows itself
        x0p, wp, bp = _pad4(x0), _pad4(w.data.reshape(L, d)), _pad4(b.data.reshape(L, d))
        dp = x0p.shape[1]
        out = torch.empty(B, dp, device=x0.device, dtype=torch.float32)
        if lz is not None and dp == d and x0.is_contiguous():
            ids, arena, row_base = lz
            _lib_().recalgo_gather_cross_fwd(_p(ids), _p(arena.weight), _p(row_base), B, ids.shape[1], arena.K, _p(wp), _p(bp), L,
                                             _p(x0), d, _p(out), dp, _stream(x0))
        else:
            if lz is not None:               # (cannot be fused after all: the plain gather first)
                ids, arena, row_base = lz
                _lib_().recalgo_embedding_gather_fwd(_p(ids), _p(arena.weight), _p(row_base), B, ids.shape[1], arena.K, _p(x0),
                                                     ids.shape[1] * arena.K, 0, _stream(ids))
                x0p = _pad4(x0)
            _lib_().recalgo_cross_fwd(_p(x0p), dp, _p(wp), _p(bp), B, dp, L, _p(out), dp, _stream(x0))
        ctx.vars = (w, b)
        ctx.d = d
        ctx.save_for_backward(x0p)
        return out if dp == d else out[:, :d]

    @staticmethod
    def backward(ctx, g):
        global _cross_rider
        w, b = ctx.vars
        (x0p,) = ctx.saved_tensors
        B, dp = x0p.shape
        d = ctx.d
        L = w.data.shape[0]
        if _cross_rider is not None and _cross_rider[0] is ctx:
            _cross_rider = None                                           # (nobody gave it a ride: computed here, as always)
        early, ctx.early = getattr(ctx, "early", None), None
        stale_dx = None
        if early is not None:
            # this backward already ran as a rider of a dense layer's launch (dense_bwd), on the gradient the fused tail produced
            eg, edx, jobs, used = early
            if eg.data_ptr() == g.data_ptr() and eg.shape == g.shape and eg.stride() == g.stride():
                if used():
                    return None, None, None, None, None          # ... and the MLP's first layer added dx0 to its own input gradient
                extra = ctx.grad_join.take() if ctx.grad_join is not None else None
                return None, (edx if extra is None else edx + extra.reshape(edx.shape)), None, None, None
            # the cross output had another consumer after all (autograd summed into a different tensor): the early result is
            # void — its deferred column sums are withdrawn, the backward runs here on the full gradient, and what the MLP's first
            # layer may already have added is taken back out
            for j in jobs:
                if any(j is e for e in _colsum_pending):
                    _colsum_pending[:] = [e for e in _colsum_pending if e is not j]
            stale_dx = edx if used() else None
        g = _pad4(g).contiguous()
        lib = _lib_()
        # unpadded width: the column sum of the partial rows joins the step's deferred-sum launch (its own scratch: the
        # rows are read after later kernels have run)
        defer = dp == d
        nbytes = int(lib.recalgo_cross_bwd_workspace_bytes(B, dp, L))
        if defer:
            key = ("cross", x0p.device.type, x0p.device.index, B, dp, L, w.grad.data_ptr())
            ws = _dense_ws.get(key)
            if ws is None:
                ws = _dense_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x0p.device)
        else:
            ws = _workspace(nbytes, x0p.device)
        dx0 = torch.empty_like(x0p)
        if dp == d:
            wp, bp, dw, db = w.data, b.data, w.grad, b.grad
        else:
            wp, bp = _pad4(w.data.reshape(L, d)), _pad4(b.data.reshape(L, d))
            dw, db = torch.empty_like(wp), torch.empty_like(bp)
        # the gradient the MLP branch parked for x0 is added in this kernel's epilogue (no separate add launch)
        extra = ctx.grad_join.take() if ctx.grad_join is not None else None
        fused_extra = extra is not None and dp == d and extra.is_contiguous() and tuple(extra.shape) == (B, d)
        lib.recalgo_cross_bwd(_p(x0p), dp, _p(wp), _p(bp), _p(g), dp, _p(extra) if fused_extra else None, B, dp, L, _p(dx0), _p(dw),
                              _p(db), _p(ws), int(defer), _stream(x0p))
        if defer:
            rows, wsf = int(lib.recalgo_cross_bwd_partial_rows(B)), ws.view(torch.float32)
            _colsum_pending.append((wsf, 0, rows, 2 * L * dp, L * dp, dw))
            _colsum_pending.append((wsf, L * dp, rows, 2 * L * dp, L * dp, db))
        if dp != d:
            w.grad.copy_(dw[:, :d].reshape(w.grad.shape))
            b.grad.copy_(db[:, :d].reshape(b.grad.shape))
            dx0 = dx0[:, :d]
        if extra is not None and not fused_extra:
            dx0 = dx0 + extra.reshape(dx0.shape)
        if stale_dx is not None:
            dx0 = dx0 - stale_dx.reshape(dx0.shape)
        return None, dx0, None, None, None


def cross_stack(store, x0: torch.Tensor, w: Variable, b: Variable, grad_join=None) -> torch.Tensor:
    """Fused L-layer CrossNet: w, b are [L, d] block variables."""
    if store.building:
        return torch.zeros_like(x0)
    _chk(x0, torch.float32, "x0")
    out = _CrossFn.apply(store.anchor, x0, w, b, grad_join)
    if grad_join is not None and out.grad_fn is not None:
        out._recalgo_cross_node = out.grad_fn        # (the fused tail hands the branch's gradient over early: defer_cross_rider)
    return out


class _CrossLayerFn(Function):
    """The reference's un-fused signature cross_layer(x0, xl, index): xl distinct from x0."""

    @staticmethod
    def forward(ctx, anchor, x0, xl, w: Variable, b: Variable):
        B, d = x0.shape
        x0p, xlp = _pad4(x0), _pad4(xl)
        wp, bp = _pad4(w.data.reshape(1, d)), _pad4(b.data.reshape(1, d))
        dp = x0p.shape[1]
        out = torch.empty(B, dp, device=x0.device, dtype=torch.float32)
        _lib_().recalgo_cross_layer_fwd(_p(x0p), _p(xlp), dp, _p(wp), _p(bp), B, dp, _p(out), dp, _stream(x0))
        ctx.vars = (w, b)
        ctx.d = d
        ctx.save_for_backward(x0p, xlp)
        return out if dp == d else out[:, :d]

    @staticmethod
    def backward(ctx, g):
        w, b = ctx.vars
        x0p, xlp = ctx.saved_tensors
        B, dp = x0p.shape
        d = ctx.d
        g = _pad4(g).contiguous()
        lib = _lib_()
        ws = _workspace(lib.recalgo_cross_bwd_workspace_bytes(B, dp, 1), x0p.device)
        dx0, dxl = torch.empty_like(x0p), torch.empty_like(x0p)
        if dp == d:
            wp, bp, dw, db = w.data, b.data, w.grad, b.grad
        else:
            wp, bp = _pad4(w.data.reshape(1, d)), _pad4(b.data.reshape(1, d))
            dw, db = torch.empty_like(wp), torch.empty_like(bp)
        lib.recalgo_cross_layer_bwd(_p(x0p), _p(xlp), dp, _p(wp), _p(bp), _p(g), dp, B, dp, _p(dx0), _p(dxl), _p(dw), _p(db),
                                    _p(ws), _stream(x0p))
        if dp != d:
            w.grad.copy_(dw[:, :d].reshape(w.grad.shape))
            b.grad.copy_(db[:, :d].reshape(b.grad.shape))
            dx0, dxl = dx0[:, :d], dxl[:, :d]
        return None, dx0, dxl, None, None


def cross_layer(store, x0: torch.Tensor, xl: torch.Tensor, w: Variable, b: Variable) -> torch.Tensor:
    """One layer, w/b of shape (d, 1) or (d,): out = x0 * (xl . w) + b + xl."""
    if store.building:
        return torch.zeros_like(x0)
    _chk(x0, torch.float32, "x0")
    _chk(xl, torch.float32, "xl")
    return _CrossLayerFn.apply(store.anchor, x0, xl, w, b)


# =============================================================================================
# K5: CIN layer (fp32 MFMA implicit GEMM)
# =============================================================================================
class _CinFn(Function):
    """One launch-sized piece of a CIN layer: the feature maps [n0, n1) of the contribution of the previous layer's maps
    [h0, h1) (the whole layer when that is everything).  The kernels take <= 128 maps on either side per launch."""

    @staticmethod
    def forward(ctx, anchor, x0, xk, filt: Variable, h0, h1, n0, n1):
        B, m, D = x0.shape
        Hk_full = filt.data.shape[-2] // m
        N_full = filt.data.shape[-1]
        whole = (h0, h1, n0, n1) == (0, Hk_full, 0, N_full)
        if whole:
            w, xk_c = filt.data, xk
        else:
            w = filt.data.reshape(Hk_full, m, N_full)[h0:h1, :, n0:n1].reshape((h1 - h0) * m, n1 - n0).contiguous()
            xk_c = xk[:, h0:h1, :].contiguous()
        Hk, N = h1 - h0, n1 - n0
        out = torch.empty(B, N, D, device=x0.device, dtype=torch.float32)
        pool = torch.empty(B, N, device=x0.device, dtype=torch.float32)
        _lib_().recalgo_cin_layer_fwd(_p(x0), _p(xk_c), _p(w), B, m, Hk, N, D, _p(out), _p(pool), N, 0, _stream(x0))
        ctx.filt, ctx.box, ctx.whole = filt, (h0, h1, n0, n1), whole
        ctx.xk_shape = xk.shape
        ctx.save_for_backward(x0, xk_c, w)
        ctx.set_materialize_grads(False)
        return out, pool

    @staticmethod
    def backward(ctx, g_out, g_pool):
        x0, xk, w = ctx.saved_tensors
        filt = ctx.filt
        h0, h1, n0, n1 = ctx.box
        B, m, D = x0.shape
        Hk, N = h1 - h0, n1 - n0
        dx0 = torch.empty_like(x0)
        dxk = torch.empty_like(xk)
        dw = filt.grad if ctx.whole else torch.empty_like(w)
        if g_out is None and g_pool is None:
            dw.zero_()
            dx0.zero_(), dxk.zero_()
        else:
            g_out = None if g_out is None else g_out.contiguous()
            g_pool = None if g_pool is None else g_pool.contiguous()
            lib = _lib_()
            ws = _workspace(lib.recalgo_cin_layer_bwd_workspace_bytes(B, m, Hk, N, D), x0.device)
            lib.recalgo_cin_layer_bwd(_p(x0), _p(xk), _p(w), _p(g_out), _p(g_pool), N, 0, B, m, Hk, N, D, _p(dx0), 0, _p(dxk), 0,
                                      _p(dw), _p(ws), _stream(x0))
        if not ctx.whole:
            Hk_full = filt.data.shape[-2] // m
            filt.grad.reshape(Hk_full, m, filt.data.shape[-1])[h0:h1, :, n0:n1].copy_(dw.reshape(Hk, m, N))
            full = torch.zeros(ctx.xk_shape, device=x0.device, dtype=torch.float32)
            full[:, h0:h1, :] = dxk
            dxk = full
        return None, dx0, dxk, None, None, None, None, None


CIN_MAX_MAPS = 128          # feature maps per launch on either side (csrc/cin.hip)


class _CinStackFn(Function):
    """The whole CIN stack of xdeepfm.py:166-174 as ONE autograd node (every layer <= 128 maps: one launch each way per layer):
    layer i's sum-pooled maps are written by its kernel straight into their column block of p_plus (no torch.cat), the
    backward reads each layer's share of d(p_plus) in place (pool_stride / pool_col of recalgo_cin_layer_bwd: no slice
    copies), the gradient of a layer's output is the next layer's dX^k handed over as is, and dX^0 is accumulated by the
    kernels across the layers (dx0_accumulate) instead of by autograd (an elementwise launch per layer)."""

    @staticmethod
    def forward(ctx, anchor, x0, *filts):
        B, m, D = x0.shape
        lib = _lib_()
        Ns = [int(f.data.shape[-1]) for f in filts]
        p_plus = torch.empty(B, sum(Ns), device=x0.device, dtype=torch.float32)
        xs, xk, col = [], x0, 0
        for f, N in zip(filts, Ns):
            Hk = xk.shape[1]
            out = torch.empty(B, N, D, device=x0.device, dtype=torch.float32)
            lib.recalgo_cin_layer_fwd(_p(x0), _p(xk), _p(f.data), B, m, Hk, N, D, _p(out), _p(p_plus), p_plus.shape[1], col,
                                      _stream(x0))
            xs.append(out)
            xk = out
            col += N
        ctx.filts, ctx.Ns = filts, Ns
        ctx.save_for_backward(x0, *xs)
        ctx.set_materialize_grads(False)
        return (p_plus, *xs)

    @staticmethod
    def backward(ctx, g_pplus, *g_xs):
        x0, *xs = ctx.saved_tensors
        filts, Ns = ctx.filts, ctx.Ns
        B, m, D = x0.shape
        lib = _lib_()
        L = len(filts)
        if g_pplus is None and all(g is None for g in g_xs):
            for f in filts:
                f.grad.zero_()
            return (None, torch.zeros_like(x0)) + (None,) * L
        if g_pplus is not None and (g_pplus.stride(1) != 1 or g_pplus.shape[1] != sum(Ns)):
            g_pplus = g_pplus.contiguous()
        dx0 = torch.empty_like(x0)
        g_next = None                                # d(loss) / d(xs[i]) arriving from layer i + 1
        cols = [sum(Ns[:i]) for i in range(L)]
        first = True
        for i in range(L - 1, -1, -1):
            xk = x0 if i == 0 else xs[i - 1]
            Hk, N = xk.shape[1], Ns[i]
            g_out = g_next
            if g_xs[i] is not None:                  # a caller that also uses the layer's maps themselves (the reference does not)
                g_out = g_xs[i].contiguous() if g_out is None else g_out + g_xs[i]
            if g_out is None and g_pplus is None:
                filts[i].grad.zero_()
                g_next = None
                continue
            dxk = torch.empty_like(xk)
            ws = _workspace(lib.recalgo_cin_layer_bwd_workspace_bytes(B, m, Hk, N, D), x0.device)
            lib.recalgo_cin_layer_bwd(
                _p(x0), _p(xk), _p(filts[i].data), _p(g_out), _p(g_pplus), 0 if g_pplus is None else g_pplus.stride(0), cols[i],
                B, m, Hk, N, D, _p(dx0), 0 if first else 1, _p(dxk), 0, _p(filts[i].grad), _p(ws), _stream(x0))
            first = False
            g_next = dxk
        if first:
            dx0.zero_()
        elif g_next is not None:
            dx0.add_(g_next)                         # layer 1: X^k IS X^0
        return (None, dx0) + (None,) * L


def cin_stack(store, x0: torch.Tensor, filts):
    """-> (p_plus [B, sum N_i], [X^1, ..., X^L]) of the CIN stack over x0 [B, m, D] with the filters `filts` (Variables of shape
    (1, H_{i-1} m, N_i)); None when a layer is wider than one launch takes (the caller then chains ops.cin_layer)."""
    if store.building or x0.dtype != torch.float32 or not x0.is_cuda:
        return None
    Hk = x0.shape[1]
    for f in filts:
        N = int(f.data.shape[-1])
        if Hk > CIN_MAX_MAPS or N > CIN_MAX_MAPS:
            return None
        Hk = N
    res = _CinStackFn.apply(store.anchor, x0.contiguous(), *filts)
    return res[0], list(res[1:])


def cin_layer(store, x0: torch.Tensor, xk: torch.Tensor, filt: Variable):
    """x0 [B,m,D], xk [B,Hk,D], filt (1, Hk*m, N) -> (xk_1 [B,N,D], sum-pooled [B,N]).  Layers wider than the kernels'
    128 x 128 maps per launch (e.g. --cin_layer_feature_maps=200,200) are tiled: output maps in column chunks
    (concatenated), previous-layer maps in row chunks (the layer is linear in X^k: the chunks' contributions add)."""
    if store.building:
        N = filt.data.shape[-1]
        return x0.new_zeros(x0.shape[0], N, x0.shape[2]), x0.new_zeros(x0.shape[0], N)
    _chk(x0, torch.float32, "x0")
    _chk(xk, torch.float32, "xk")
    Hk, N = xk.shape[1], filt.data.shape[-1]
    if Hk <= CIN_MAX_MAPS and N <= CIN_MAX_MAPS:
        return _CinFn.apply(store.anchor, x0, xk, filt, 0, Hk, 0, N)
    hs = [(h, min(h + CIN_MAX_MAPS, Hk)) for h in range(0, Hk, CIN_MAX_MAPS)]
    ns = [(n, min(n + CIN_MAX_MAPS, N)) for n in range(0, N, CIN_MAX_MAPS)]
    outs, pools = [], []
    for n0, n1 in ns:
        o = p = None
        for h0, h1 in hs:
            oc, pc = _CinFn.apply(store.anchor, x0, xk, filt, h0, h1, n0, n1)
            o, p = (oc, pc) if o is None else (o + oc, p + pc)
        outs.append(o)
        pools.append(p)
    return torch.cat(outs, dim=1), torch.cat(pools, dim=1)


# =============================================================================================
# K9: DIN attention
# =============================================================================================
class _DinAttentionFn(Function):
    @staticmethod
    def forward(ctx, anchor, query, keys, keys_length, vs, is_softmax: bool, query_join=None):
        # vs = (f1_w, f1_b, f2_w, f2_b, f3_w, f3_b) Variables
        B, T, H = keys.shape
        out = torch.empty(B, H, device=query.device, dtype=torch.float32)
        _lib_().recalgo_din_attention_fwd(_p(query), _p(keys), _p(keys_length), *[_p(v.data) for v in vs], B, T, H, int(is_softmax),
                                          _p(out), _stream(query))
        ctx.vs, ctx.is_softmax, ctx.kl = vs, is_softmax, keys_length
        ctx.query_join = query_join
        ctx.in_step = _loss_seed is not None      # built inside Estimator.train_step: its optimizer runs the deferred sums
        ctx.save_for_backward(query, keys)
        return out

    @staticmethod
    def backward(ctx, g):
        query, keys = ctx.saved_tensors
        B, T, H = keys.shape
        vs = ctx.vs
        lib = _lib_()
        # g may be a column block of a wider gradient matrix (the fcn input's): read in place when its rows are float4s
        if not (g.dim() == 2 and g.stride(1) == 1 and g.stride(0) % 4 == 0 and g.stride(0) >= H and g.data_ptr() % 16 == 0):
            g = g.contiguous()
        # the gradient the query's other consumer parked (nn.GradJoin): added in this kernel's epilogue
        extra = ctx.query_join.take() if ctx.query_join is not None else None
        fused_extra = extra is not None and extra.dim() == 2 and tuple(extra.shape) == (B, H) and extra.stride(1) == 1
        dq, dk = torch.empty_like(query), torch.empty_like(keys)
        nbytes = int(lib.recalgo_din_attention_bwd_workspace_bytes(B, T, H))
        if ctx.in_step:
            # inside a training step: the six parameter gradients are column sums of the kernel's partial rows — jobs of the
            # step's deferred-sum launch instead of a launch of their own (the partials need a buffer of their own until then)
            key = ("din_att", query.device.type, query.device.index, B, T, H, vs[0].grad.data_ptr())
            ws = _dense_ws.get(key)
            if ws is None:
                ws = _dense_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=query.device)
            grads = [None] * 6
        else:
            ws = _workspace(nbytes, query.device)
            grads = [_p(v.grad) for v in vs]
        lib.recalgo_din_attention_bwd_joined(_p(query), _p(keys), _p(ctx.kl), *[_p(v.data) for v in vs], _p(g), g.stride(0),
                                             _p(extra) if fused_extra else None, extra.stride(0) if fused_extra else 0, B, T, H,
                                             int(ctx.is_softmax), _p(dq), _p(dk), *grads, _p(ws), _stream(query))
        if ctx.in_step:
            rows, pf = int(lib.recalgo_din_attention_bwd_partial_rows(B)), int(lib.recalgo_din_attention_bwd_partial_floats(H))
            wsf, off = ws.view(torch.float32), 0
            flat = all(vs[i + 1].grad.data_ptr() == vs[i].grad.data_ptr() + 4 * vs[i].grad.numel()
                       and vs[i + 1].grad.untyped_storage().data_ptr() == vs[0].grad.untyped_storage().data_ptr()
                       for i in range(5))
            if flat:      # the six gradients lie in the flat gradient buffer in the partial row's order: ONE job
                g0 = vs[0].grad
                out = torch.empty(0, dtype=torch.float32, device=g0.device).set_(g0.untyped_storage(), g0.storage_offset(), (pf,), (1,))
                _colsum_pending.append((wsf, 0, rows, pf, pf, out))
            else:
                for v in vs:
                    n = v.grad.numel()
                    _colsum_pending.append((wsf, off, rows, pf, n, v.grad))
                    off += n
        if extra is not None and not fused_extra:
            dq = dq + extra.reshape(dq.shape)
        return None, dq, dk, None, None, None, None


def din_attention(store, query, keys, keys_length, vs, is_softmax=False, query_join=None) -> torch.Tensor:
    """query [B,H], keys [B,T,H], keys_length [B] int32 -> [B,H].  query_join (nn.GradJoin): the query's other consumer
    parks its input gradient there and this op's backward kernel adds it to d(query)."""
    if store.building:
        return torch.zeros_like(query)
    _chk(query, torch.float32, "query")
    _chk(keys, torch.float32, "keys")
    if keys_length.dtype != torch.int32:
        keys_length = keys_length.to(torch.int32)
    return _DinAttentionFn.apply(store.anchor, query, keys, keys_length.contiguous(), tuple(vs), bool(is_softmax), query_join)


# =============================================================================================
# K7/K8: FiBiNET SENET + bilinear interaction
# =============================================================================================
BILINEAR_TYPES = {"all": _C["RECALGO_BILINEAR_ALL"], "each": _C["RECALGO_BILINEAR_EACH"],
                  "interaction": _C["RECALGO_BILINEAR_INTERACTION"]}


class _SenetFn(Function):
    @staticmethod
    def forward(ctx, anchor, emb, w1: Variable, w2: Variable):
        B, F, K = emb.shape
        Rd = w1.data.shape[1]
        v = torch.empty_like(emb)
        _lib_().recalgo_senet_fwd(_p(emb), _p(w1.data), _p(w2.data), B, F, K, Rd, _p(v), None, _stream(emb))
        ctx.vars = (w1, w2)
        ctx.save_for_backward(emb)
        return v

    @staticmethod
    def backward(ctx, g):
        w1, w2 = ctx.vars
        (emb,) = ctx.saved_tensors
        B, F, K = emb.shape
        Rd = w1.data.shape[1]
        lib = _lib_()
        g = g.contiguous()
        ws = _workspace(lib.recalgo_senet_bwd_workspace_bytes(B, F, K, Rd), emb.device)
        d = torch.empty_like(emb)
        lib.recalgo_senet_bwd(_p(emb), _p(w1.data), _p(w2.data), _p(g), B, F, K, Rd, _p(d), 0,
                              _p(w1.grad), _p(w2.grad), _p(ws), _stream(emb))
        return None, d, None, None


def senet(store, emb: torch.Tensor, w1: Variable, w2: Variable) -> torch.Tensor:
    """emb [B,F,K], w1 (F, Rd), w2 (Rd, F) -> re-weighted embeddings [B,F,K]."""
    if store.building:
        return torch.zeros_like(emb)
    _chk(emb, torch.float32, "input")
    return _SenetFn.apply(store.anchor, emb, w1, w2)


class _BilinearFn(Function):
    @staticmethod
    def forward(ctx, anchor, btype: int, x0, w0: Variable, x1, w1: Optional[Variable]):
        B, F, K = x0.shape
        nv = 1 if x1 is None else 2
        P = (F - 1) * (F - 2) // 2
        out = torch.empty(B, P, nv * K, device=x0.device, dtype=torch.float32)
        _lib_().recalgo_bilinear_fwd(_p(x0), _p(w0.data), _p(x1), None if w1 is None else _p(w1.data), B, F, K, btype, _p(out),
                                     nv * K, 0, _stream(x0))
        ctx.vars, ctx.btype, ctx.nv = (w0, w1), btype, nv
        ctx.save_for_backward(x0, x1)
        return out

    @staticmethod
    def backward(ctx, g):
        w0, w1 = ctx.vars
        x0, x1 = ctx.saved_tensors
        B, F, K = x0.shape
        nv = ctx.nv
        lib = _lib_()
        g = g.contiguous()
        ws = _workspace(lib.recalgo_bilinear_bwd_workspace_bytes(B, F, K, nv, ctx.btype), x0.device)
        dx0 = torch.empty_like(x0)
        dx1 = None if x1 is None else torch.empty_like(x1)
        lib.recalgo_bilinear_bwd(_p(x0), _p(w0.data), _p(x1), None if w1 is None else _p(w1.data), _p(g), nv * K, 0, B, F, K,
                                 ctx.btype, _p(dx0), _p(w0.grad), _p(dx1), None if w1 is None else _p(w1.grad), _p(ws), _stream(x0))
        return None, None, dx0, None, dx1, None


def bilinear_interaction(store, btype: str, x0: torch.Tensor, w0: Variable,
                         x1: Optional[torch.Tensor] = None, w1: Optional[Variable] = None) -> torch.Tensor:
    """(x_s [B,F,K], W_s) for one or two sets -> [B, (F-1)(F-2)/2, n_sets*K] (sets concatenated on
    the last axis).  For type "interaction" only the first (F-1)(F-2)/2 slices of W_s are read and
    receive gradient (the reference's zip truncation); the rest keep a zero gradient."""
    if btype not in BILINEAR_TYPES:
        raise ValueError(f"Bilinear Interaction type must be in ['all','each','interaction'], got '{btype}'")
    if store.building:
        B, F, K = x0.shape
        return x0.new_zeros(B, (F - 1) * (F - 2) // 2, (1 if x1 is None else 2) * K)
    _chk(x0, torch.float32, "input")
    if x1 is not None:
        _chk(x1, torch.float32, "input")
    return _BilinearFn.apply(store.anchor, BILINEAR_TYPES[btype], x0, w0, x1, w1)


# =============================================================================================
# K6: PNN product layer
# =============================================================================================
PNN_METHODS = {"IPNN": _C["RECALGO_PNN_IPNN"], "OPNN": _C["RECALGO_PNN_OPNN"]}


class _PnnProductFn(Function):
    """relu(emb @ linear_w + phi(emb) @ omega(product_w) + bias): feature / weight builders (csrc/pnn.hip) and
    the D-way contraction (csrc/dense.hip, fp32 MFMA: both operand pairs, the bias and the ReLU in ONE
    launch; pnn.py:139,146-181) are hand-written kernels, forward and backward."""

    @staticmethod
    def forward(ctx, anchor, emb_flat, linear_w: Variable, product_w: Variable, bias: Variable, F, K, method):
        B = emb_flat.shape[0]
        D = linear_w.data.shape[1]
        lib = _lib_()
        T = lib.recalgo_pnn_feature_count(F, K, method)
        T4 = (T + 3) // 4 * 4          # row stride of phi / row count of omega: float4-addressable GEMM operands
        st = _stream(emb_flat)
        phi = torch.empty(B, T4, device=emb_flat.device, dtype=torch.float32)      # padding columns zeroed by the kernel
        omega = _pnn_omega(product_w, T4, D)                                        # padding rows stay zero
        lib.recalgo_pnn_features_fwd(_p(emb_flat), B, F, K, method, _p(phi), T4, st)
        lib.recalgo_pnn_weights_fwd(_p(product_w.data), D, F, K, method, _p(omega), st)
        # lz + lp + bias, ReLU  (pnn.py:139,175,178,181)
        y = dense_fwd(emb_flat, linear_w.data.reshape(-1, D), bias.data.reshape(-1), True, x2=phi, w2=omega)
        ctx.vars = (linear_w, product_w, bias)
        ctx.dims = (F, K, method)
        ctx.save_for_backward(emb_flat, phi, omega, y)
        return y

    @staticmethod
    def backward(ctx, g):
        linear_w, product_w, bias = ctx.vars
        F, K, method = ctx.dims
        emb_flat, phi, omega, y = ctx.saved_tensors
        B, D = y.shape
        T4 = phi.shape[1]
        lib = _lib_()
        st = _stream(emb_flat)
        g = g.contiguous()
        # gz = g * [y > 0] is applied inside the kernels (never materialised); each operand pair's input and weight
        # gradients are one merged launch.  The omega gradient is needed right away (pnn_weights_bwd), so its split
        # sum is not deferred to the end of the step
        domega = torch.empty_like(omega)
        dphi = dense_bwd(phi, g, y, omega, domega, None)
        d_emb = dense_bwd(emb_flat, g, y, linear_w.data.reshape(-1, D), linear_w.grad.view(-1, D), bias.grad.view(-1),
                          defer=True)
        lib.recalgo_pnn_features_bwd(_p(emb_flat), _p(dphi), T4, B, F, K, method, _p(d_emb), 1, st)
        lib.recalgo_pnn_weights_bwd(_p(product_w.data), _p(domega), D, F, K, method, _p(product_w.grad), st)
        return None, d_emb, None, None, None, None, None, None


_pnn_omega_cache = {}


def _pnn_omega(product_w: Variable, T4: int, D: int) -> torch.Tensor:
    """The [T4, D] omega buffer of one product layer, allocated once (zeros): recalgo_pnn_weights_fwd rewrites its first
    T rows every step, the padding rows stay zero."""
    key = (product_w.data.data_ptr(), T4, D)
    t = _pnn_omega_cache.get(key)
    if t is None:
        if len(_pnn_omega_cache) > 16:
            _pnn_omega_cache.clear()
        t = _pnn_omega_cache[key] = torch.zeros(T4, D, device=product_w.data.device, dtype=torch.float32)
    return t


def pnn_product_layer(store, emb_flat: torch.Tensor, linear_w: Variable, product_w: Variable, bias: Variable,
                      F: int, K: int, method: str) -> torch.Tensor:
    """emb_flat [B, F*K] -> relu(lz + lp + bias) [B, D] (pnn.py:133-181)."""
    if store.building:
        return emb_flat.new_zeros(emb_flat.shape[0], linear_w.data.shape[1])
    _chk(emb_flat, torch.float32, "fields_embeddings")
    return _PnnProductFn.apply(store.anchor, emb_flat, linear_w, product_w, bias, int(F), int(K),
                               PNN_METHODS["IPNN" if method == "IPNN" else "OPNN"])


class _IpnnFeaturesFn(Function):
    """phi[b, t(i,j)] = <e_i[b], e_j[b]>, i <= j: the Gram upper triangle of the fields, diagonal included
    (`recalgo_pnn_features_*`, method IPNN)."""

    @staticmethod
    def forward(ctx, emb_flat, F, K):
        B = emb_flat.shape[0]
        lib = _lib_()
        T = lib.recalgo_pnn_feature_count(F, K, 0)
        phi = torch.empty(B, T, device=emb_flat.device, dtype=torch.float32)
        lib.recalgo_pnn_features_fwd(_p(emb_flat), B, F, K, 0, _p(phi), T, _stream(emb_flat))
        ctx.dims = (F, K)
        ctx.save_for_backward(emb_flat)
        return phi

    @staticmethod
    def backward(ctx, dphi):
        (emb_flat,) = ctx.saved_tensors
        F, K = ctx.dims
        dphi = dphi.contiguous()
        d_emb = torch.empty_like(emb_flat)
        _lib_().recalgo_pnn_features_bwd(_p(emb_flat), _p(dphi), dphi.shape[1], emb_flat.shape[0], F, K, 0, _p(d_emb), 0,
                                         _stream(emb_flat))
        return d_emb, None, None


class _PairKernel:
    """The one-unit head over phi whose [T, 1] kernel is the pair strengths r scattered to the off-diagonal columns of the
    Gram triangle (0 on the diagonal).  Quacks like a Variable for the fused loss tail (`data`; its gradient = the column
    sums of the tail's partial rows, delivered straight into r.grad: row i of the strict triangle is one contiguous run
    of both index spaces, so the F - 1 runs are F - 1 jobs of the step's deferred-sum launch — no select launch)."""

    def __init__(self, r: Variable, w: torch.Tensor, F: int, anchor):
        self.r, self.data, self.F, self.anchor = r, w, int(F), anchor
        self.grad = None

    def colsum_jobs(self, partials, col, rows, stride):
        F, out, jobs, at = self.F, self.r.grad.view(-1), [], 0
        for i in range(F - 1):
            n = F - 1 - i
            jobs.append((partials, col + i * F - i * (i - 1) // 2 + 1, rows, stride, n, out[at:at + n]))
            at += n
        return jobs

    def apply_head(self, parts):
        return _PairHeadFn.apply(self.anchor, parts[0], self.r, self.F)


class _PairHeadFn(Function):
    """logit[b] = sum_{i<j} r[index(i,j)] * phi[b, t(i,j)]  (FwFM second order, fwfm.py:146-158) outside a TRAIN step's
    fused tail: the one-unit head kernels (`recalgo_dense1_*`) over phi."""

    @staticmethod
    def forward(ctx, anchor, phi, r: Variable, F):
        w = _pair_vector(r, F, phi.shape[1], phi.device)
        ctx.r, ctx.F = r, F
        ctx.save_for_backward(phi, w)
        return dense1_fwd([phi], w, None)

    @staticmethod
    def backward(ctx, g):
        phi, w = ctx.saved_tensors
        dphi = torch.empty_like(phi) if ctx.needs_input_grad[1] else None
        dw = torch.empty_like(w)
        dense1_bwd([phi], w, g.contiguous(), [dphi], dw, None)
        torch.index_select(dw.reshape(-1), 0, _pair_index(ctx.F, phi.device), out=ctx.r.grad.view(-1))
        return None, dphi, None, None


def _pair_vector(r: Variable, F: int, T: int, dev) -> torch.Tensor:
    """[T, 1]: r at the off-diagonal columns of the Gram triangle, 0 on its diagonal (allocated and cleared once)."""
    w = _pair_vectors.get((r.data.data_ptr(), T))
    if w is None:
        w = _pair_vectors[(r.data.data_ptr(), T)] = torch.zeros(T, 1, device=dev, dtype=torch.float32)
    w.index_copy_(0, _pair_index(F, dev), r.data.reshape(-1, 1))
    return w


_pair_index_cache = {}
_pair_vectors = {}


def _pair_index(F: int, device) -> torch.Tensor:
    """index_from_upper_triangular(i, j, F) (reference utils.py:67-82, row-major strict upper triangle) ->
    column t(i, j) = i*F - i(i-1)/2 + (j - i) of the Gram upper triangle with diagonal (include/recalgo.h)."""
    key = (F, device)
    t = _pair_index_cache.get(key)
    if t is None:
        cols = [i * F - i * (i - 1) // 2 + (j - i) for i in range(F - 1) for j in range(i + 1, F)]
        t = _pair_index_cache[key] = torch.tensor(cols, dtype=torch.int64, device=device)
    return t


def field_pair_logit(store, emb_flat: torch.Tensor, r: Variable, F: int, K: int):
    """emb_flat [B, F*K], r [F(F-1)/2] -> [B, 1]: sum_{i<j} r[index(i,j)] <e_i, e_j> (fwfm.py:146-158).  In a TRAIN step
    the sum over the pairs is left to the fused loss tail (nn.LazyLogit: one launch for this head, the loss and the backward
    of both)."""
    if store.building:
        return emb_flat.new_zeros(emb_flat.shape[0], 1)
    _chk(emb_flat, torch.float32, "fields_embeddings")
    F, K = int(F), int(K)
    phi = _IpnnFeaturesFn.apply(emb_flat.contiguous(), F, K)
    if logit_loss_supported([phi], []):
        from .nn import LazyLogit
        return LazyLogit([(_PairKernel(r, _pair_vector(r, F, phi.shape[1], phi.device), F, store.anchor), None, [phi])])
    return _PairHeadFn.apply(store.anchor, phi, r, F)


# =============================================================================================
# sibling models: NFM bi-interaction, AFM attention pooling, FFM pair dots (csrc/siblings.hip)
# =============================================================================================
class _BiInteractionFn(Function):
    @staticmethod
    def forward(ctx, emb, F, K):
        emb = emb.contiguous()
        B = emb.shape[0]
        out = torch.empty(B, K, device=emb.device, dtype=torch.float32)
        _lib_().recalgo_bi_interaction_fwd(_p(emb), B, F, K, _p(out), _stream(emb))
        ctx.dims = (F, K)
        ctx.save_for_backward(emb)
        return out

    @staticmethod
    def backward(ctx, g):
        (emb,) = ctx.saved_tensors
        F, K = ctx.dims
        d = torch.empty_like(emb)
        _lib_().recalgo_bi_interaction_bwd(_p(emb), _p(g.contiguous()), emb.shape[0], F, K, _p(d), _stream(emb))
        return d, None, None


def bi_interaction(emb_flat: torch.Tensor, F: int, K: int) -> torch.Tensor:
    """[B, F*K] -> [B, K]: 0.5 * ((sum_f e_f)^2 - sum_f e_f^2) (nfm.py:155-167)."""
    _chk(emb_flat, torch.float32, "fields_embeddings")
    return _BiInteractionFn.apply(emb_flat, int(F), int(K))


class _AttentionPoolFn(Function):
    @staticmethod
    def forward(ctx, pairs, att):
        pairs, att = pairs.contiguous(), att.contiguous()
        B, P, K = pairs.shape
        out = torch.empty(B, K, device=pairs.device, dtype=torch.float32)
        score = torch.empty(B, P, device=pairs.device, dtype=torch.float32)
        _lib_().recalgo_attention_pool_fwd(_p(pairs), _p(att), B, P, K, _p(out), _p(score), _stream(pairs))
        ctx.save_for_backward(pairs, score)
        return out

    @staticmethod
    def backward(ctx, g):
        pairs, score = ctx.saved_tensors
        B, P, K = pairs.shape
        dp, da = torch.empty_like(pairs), torch.empty_like(score)
        _lib_().recalgo_attention_pool_bwd(_p(pairs), _p(score), _p(g.contiguous()), B, P, K, _p(dp), _p(da), _stream(pairs))
        return dp, da


def attention_pool(pairs: torch.Tensor, att: torch.Tensor) -> torch.Tensor:
    """pairs [B, P, K], att [B, P] -> sum_p softmax(att)[p] * pairs[:, p, :]  (afm.py:184-188)."""
    return _AttentionPoolFn.apply(pairs, att.reshape(pairs.shape[0], pairs.shape[1]))


class _FfmPairsFn(Function):
    @staticmethod
    def forward(ctx, x, F, K):
        x = x.contiguous()
        B = x.shape[0]
        out = torch.empty(B, 1, device=x.device, dtype=torch.float32)
        _lib_().recalgo_ffm_pairs_fwd(_p(x), B, F, K, _p(out), _stream(x))
        ctx.dims = (F, K)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        F, K = ctx.dims
        dx = torch.empty_like(x)
        _lib_().recalgo_ffm_pairs_bwd(_p(x), _p(g.contiguous()), x.shape[0], F, K, _p(dx), _stream(x))
        return dx, None, None


def ffm_pairs(x: torch.Tensor, F: int, K: int) -> torch.Tensor:
    """x [B, F*(F-1)*K] (field i in its sub-table s at [i, s]) -> [B, 1] = sum_{i<j} <x[i][j-1], x[j][i]> (ffm.py:146-160)."""
    _chk(x, torch.float32, "field-aware embeddings")
    return _FfmPairsFn.apply(x, int(F), int(K))


# ---- FFM's field-aware term without its operand tensor (csrc/ffm.hip, include/recalgo_ffm.h) --------------------------------------
_FFM = _lib.SERVING_HEADERS["recalgo_ffm.h"]
_FfmField, _FfmBagC = _FFM.structs["recalgo_ffm_field_t"], _FFM.structs["recalgo_ffm_bag_t"]
# fused=None with every field single-valued: the kernels, or the composed gather -> ffm_pairs chain.  Set from
# scripts/bench_ffm.py (profiles/ffm_bench.json); with a bag field the kernels are the default either way: they are what makes the
# step capturable.
FFM_FUSED_ALL_SINGLE = True


class FfmBag(NamedTuple):
    """A bag field as ffm_bag_distinct left it: `values` de-duplicated ([capacity], dropped entries -1), the Ragged's `offsets`,
    valid [B] int32 (entries with an id >= 0, a repeated id counted every time) and distinct [B] int32 (kept entries)."""
    values: torch.Tensor
    offsets: torch.Tensor
    valid: torch.Tensor
    distinct: torch.Tensor


def ffm_supported(F: int, K: int, n_bags: int) -> bool:
    return bool(_lib_().recalgo_ffm_supported(int(F), int(K), int(n_bags)))


def ffm_bag_distinct(values: torch.Tensor, offsets: torch.Tensor):
    """-> (values, valid, distinct) of recalgo_ffm_bag_distinct: the DISTINCT ids of every bag (utils.py:49-64
    `to_sparse_tensor`) in place — an entry keeps its id when no earlier entry of its bag holds it, every other entry (a repeated
    id, an OOV entry, the -1 tail of a padded Ragged) becomes -1 — and the two counts per bag.  One launch, shapes fixed by the
    inputs' shapes alone, nothing read back."""
    _chk(values, torch.int64, "ffm_bag_distinct: values")
    _chk(offsets, torch.int64, "ffm_bag_distinct: offsets")
    B = offsets.numel() - 1
    if B < 1 or values.dim() != 1:
        raise ValueError("ffm_bag_distinct: values [n] and offsets [B + 1] with B >= 1")
    out = torch.empty_like(values)
    valid = torch.empty(B, dtype=torch.int32, device=offsets.device)
    distinct = torch.empty(B, dtype=torch.int32, device=offsets.device)
    _lib_().recalgo_ffm_bag_distinct(_p(values) if values.numel() else None, _p(offsets), B, values.numel(),
                                     _p(out) if values.numel() else None, _p(valid), _p(distinct), _stream(offsets))
    return out, valid, distinct


def ffm_distinct_bags_composed(values: torch.Tensor, offsets: torch.Tensor):
    """-> (values, offsets) of the bags' DISTINCT valid ids, ascending per bag (utils.py:49-64), by torch.unique: the composed
    path's form.  Its shapes depend on the data and it reads two values back: a model that comes here is not captured."""
    from . import feature_column as fc
    fc.data_dependent("FFM: the distinct ids of a bag (_distinct_bags) have a data-dependent count")
    vals, offs = values, offsets
    B = offs.numel() - 1
    bag = torch.repeat_interleave(torch.arange(B, device=vals.device), offs[1:] - offs[:-1])
    vals = vals[:bag.numel()]                                    # (a padded Ragged: the -1 tail belongs to no bag)
    ok = vals >= 0
    key = bag[ok] * (int(vals.max().item()) + 2 if vals.numel() else 1) + vals[ok]
    uniq = torch.unique(key)                                     # sorted
    mult = int(vals.max().item()) + 2 if vals.numel() else 1
    ub, uv = torch.div(uniq, mult, rounding_mode="floor"), uniq % mult
    counts = torch.zeros(B, dtype=torch.int64, device=vals.device).index_add_(0, ub, torch.ones_like(ub))
    new_offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=vals.device), counts.cumsum(0)])
    return uv.contiguous(), new_offs


def ffm_fused_serves(arena, F: int, K: int, n_bags: int, fused: Optional[bool] = None) -> bool:
    """Whether ffm_interaction(.., fused) takes the kernels for a call in the current grad mode: a HIP device, a local arena, a
    shape inside recalgo_ffm_supported and, when training a trainable arena, the owner-computes plan (sparse.py).  fused=None
    asks for them wherever they serve (every field single-valued: where they were measured not to lose, FFM_FUSED_ALL_SINGLE);
    fused=True raises where they do not serve; fused=False never takes them."""
    if fused is False:
        return False
    why = None
    if arena.weight is None or not arena.weight.is_cuda:
        why = "the arena is not on a HIP device"
    elif getattr(arena, "sharding", None) is not None or type(arena) is not EmbeddingArena:
        why = "the arena is row-sharded"
    elif arena.K != int(K) or not ffm_supported(F, K, n_bags):
        c = _FFM.constants
        why = (f"the kernels serve {c['RECALGO_FFM_MIN_F']} <= F <= {c['RECALGO_FFM_MAX_F']}, K % 4 == 0 with {c['RECALGO_FFM_MIN_K']} "
               f"<= K <= {c['RECALGO_FFM_MAX_K']} and at most {c['RECALGO_FFM_MAX_BAGS']} bag fields; got F={F} K={K} bags={n_bags}")
    elif torch.is_grad_enabled() and getattr(arena, "trainable", True) and not (sparse.scatter_mode() == "owner" and sparse._supported(arena)):
        why = "training needs the arena on the owner-computes plan"
    if why is None:
        return True if (fused or n_bags) else bool(FFM_FUSED_ALL_SINGLE)
    if fused:
        raise ValueError(f"ffm_interaction(fused=True): {why}")
    return False


class _FfmFn(Function):
    """include/recalgo_ffm.h recalgo_ffm_fwd / recalgo_ffm_bwd.  ids [B, n_single]; desc = (fields array, single-valued row bases
    [n_single (F - 1)], per bag its row bases [F - 1], F, K); bags = [FfmBag] in the order of the fields.  Nothing is saved: the
    backward fetches the rows again."""

    @staticmethod
    def forward(ctx, anchor, ids, arena: EmbeddingArena, desc, bags, training=False):
        fields, rbv, rb_bags, F, K = desc
        B = ids.shape[0] if ids is not None else bags[0].offsets.numel() - 1
        ns = F - len(bags)
        dev = arena.weight.device
        st = anchor_store(anchor)
        out = torch.empty(B, 1, device=dev, dtype=torch.float32)
        # owner-computes scatter (sparse.py): ONE source for the single-valued requests — the id matrix against F - 1 row bases
        # per field — and ONE per bag field — its entries against the field's F - 1 row bases
        ctx.src, ctx.bag_srcs = None, []
        registered = bool(training) and getattr(arena, "trainable", True)       # (ffm_fused_serves: then the arena is on the plan)
        if registered and ns:
            # (contiguous() before the reshape: with ONE single-valued field the expanded matrix reshapes to a stride-0 VIEW, and
            # the scatter indexes its ids as a dense [B, n_single (F - 1)] matrix)
            idv = ids.unsqueeze(2).expand(B, ns, F - 1).contiguous().view(B, -1)
            ctx.src = sparse.begin_lookup(arena, st, idv, None, rbv, 0, B, ns * (F - 1), True)
        if registered:
            for bg, rb in zip(bags, rb_bags):
                cap = bg.values.numel()
                bid = bg.values.unsqueeze(1).expand(cap, F - 1).contiguous()
                ctx.bag_srcs.append(sparse.begin_lookup(arena, st, bid, None, rb, 0, cap, F - 1, True) if cap else None)
        # deferred Adam: registered lookups' rows were just caught up; any other call reads lagging rows as of now
        dv, stp = (None, None) if registered else sparse.deferred_view(arena, st)
        ctx.cbags = _ffm_bag_array(bags, None)
        _lib_().recalgo_ffm_fwd(_p(ids), fields, ctx.cbags, len(bags), _p(arena.weight), B, F, K, _p(out), dv, stp, 0, _stream(out))
        ctx.args = (ids, arena, desc, bags, B, registered)
        return out

    @staticmethod
    def backward(ctx, g):
        ids, arena, (fields, _rbv, _rbb, F, K), bags, B, registered = ctx.args
        if not registered:                   # (a frozen arena: nobody takes the rows)
            return None, None, None, None, None, None
        ns = F - len(bags)
        W = (F - 1) * K
        g = _contig(g.reshape(B))
        d_single = torch.empty(B, ns * W, device=g.device, dtype=torch.float32) if ns else None
        d_bags = [torch.empty(bg.values.numel(), W, device=g.device, dtype=torch.float32) for bg in bags]
        cbags = _ffm_bag_array(bags, d_bags)
        _lib_().recalgo_ffm_bwd(_p(g), _p(ids), fields, cbags, len(bags), _p(arena.weight), B, F, K, _p(d_single), _stream(g))
        if ctx.src is not None:
            ctx.src.set_grad(d_single)       # summed per row (and applied) by the optimizer's recalgo_scatter_apply
        for src, d in zip(ctx.bag_srcs, d_bags):
            if src is not None:
                src.set_grad(d)
        return None, None, None, None, None, None


def _ffm_bag_array(bags, d_rows):
    if not bags:
        return None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    return (_FfmBagC * len(bags))(*[_FfmBagC(ptr(bg.values), bg.offsets.data_ptr(), bg.distinct.data_ptr(), bg.values.numel(),
                                            None if d_rows is None else ptr(d_rows[k])) for k, bg in enumerate(bags)])


def ffm_interaction(store, ids: Optional[torch.Tensor], bags, arena: EmbeddingArena, tables, vocab, F: int, K: int,
                    fused: Optional[bool] = None) -> torch.Tensor:
    """FFM's second-order term (ffm.py:146-160): [B, 1] = sum over the pairs i < j of <v_i[j - 1], v_j[i]>, v_i[s] the row of
    field i in its sub-table s — view s of the arena table tables[i], an (F - 1, vocab[i], K) variable.
      ids     [B, n_single] int64: the ids of the single-valued fields, in field order (id < 0: OOV, a zero row); None when
              every field is a bag
      bags    {field index: Ragged | FfmBag}: the multi-valued fields; such a field's row is the mean over the bag's DISTINCT
              valid ids (utils.py:49-64)
    fused (ffm_fused_serves): the kernels of csrc/ffm.hip — one launch each way that fetches the rows itself; the scatter gets ONE
    source for the single-valued requests and one per bag field, and nothing on the way synchronises or has a data-dependent
    shape — or (False) the composition gather / F - 1 bag means per bag field -> cat -> ffm_pairs."""
    F, K = int(F), int(K)
    bags = dict(bags or {})
    single = [i for i in range(F) if i not in bags]
    if len(tables) != F or len(vocab) != F or not all(0 <= i < F for i in bags) or (ids is None) != (not single):
        raise ValueError("ffm_interaction: F tables and vocabulary sizes, bag fields inside [0, F), ids for the single-valued fields")
    if single:
        _chk(ids, torch.int64, "ffm_interaction: ids")
        if ids.dim() != 2 or ids.shape[1] != len(single) or ids.shape[0] == 0:
            raise ValueError(f"ffm_interaction: ids must be a non-empty [B, {len(single)}] matrix, got {tuple(ids.shape)}")
    dev = arena.weight.device
    if ffm_fused_serves(arena, F, K, len(bags), fused):
        key = (arena.name, "ffm_fused", tuple(tables), tuple(int(v) for v in vocab), tuple(sorted(bags)))
        desc = store._rb_cache.get(key)
        if desc is None:
            base = [arena.tables[t][0] for t in tables]
            order = sorted(bags)
            fields = (_FfmField * F)(*[_FfmField(base[i], int(vocab[i]), order.index(i) if i in bags else -1) for i in range(F)])
            views = lambda i: [base[i] + s * int(vocab[i]) for s in range(F - 1)]
            rbv = torch.tensor([r for i in single for r in views(i)], dtype=torch.int64, device=dev)
            rb_bags = [torch.tensor(views(i), dtype=torch.int64, device=dev) for i in order]
            desc = store._rb_cache[key] = (fields, rbv, rb_bags, F, K)
        blist = []
        for i in sorted(bags):
            bg = bags[i]
            if not isinstance(bg, FfmBag):
                kept, valid, distinct = ffm_bag_distinct(bg.values, bg.offsets)
                bg = FfmBag(kept, bg.offsets, valid, distinct)
            blist.append(bg)
        return _FfmFn.apply(store.anchor, ids, arena, desc, blist, torch.is_grad_enabled())
    # ---- the composed path: X [B, F, F-1, K] in memory -----------------------------------------------------------------------------
    B = ids.shape[0] if single else next(iter(bags.values())).offsets.numel() - 1
    if single:
        # view s of field i's (F-1, V, K) variable starts at arena row base_i + s * V_i: the F - 1 lookups of a field are the
        # SAME id against F - 1 row bases (OOV stays -1), so the id matrix is one expanding copy, not 5 launches per field
        key = (arena.name, "ffm_views", tuple(single))
        rbv = store._rb_cache.get(key)
        if rbv is None:
            rbv = store._rb_cache[key] = torch.tensor([arena.tables[tables[i]][0] + s * int(vocab[i]) for i in single for s in range(F - 1)],
                                                      dtype=torch.int64, device=dev)
        idv = ids.unsqueeze(2).expand(B, len(single), F - 1).contiguous().view(B, -1)
        got = embedding_gather(store, idv, arena, rbv)                                                # (B, n_single*(F-1)*K)
    if len(single) == F:
        X = got                                                  # all fields single-valued: the gather output IS X
    else:
        # runs of consecutive single-valued fields are one slice of the gather output each; a multi-valued field is F-1
        # bag-mean lookups over its distinct ids
        blocks, i, W = [], 0, (F - 1) * K
        while i < F:
            if i in bags:
                if isinstance(bags[i], FfmBag):
                    raise ValueError("ffm_interaction: the composed path takes a bag field as a Ragged")
                dvals, doffs = ffm_distinct_bags_composed(bags[i].values, bags[i].offsets)
                blocks += [embedding_bag_mean(store, torch.where(dvals >= 0, dvals + s * int(vocab[i]), dvals), doffs, arena, tables[i])
                           for s in range(F - 1)]
                i += 1
            else:
                j = i
                while j < F and j not in bags:
                    j += 1
                a = single.index(i)
                blocks.append(got[:, a * W:(a + j - i) * W])
                i = j
        X = torch.cat(blocks, dim=1).contiguous()                # (B, F*(F-1)*K)
    return ffm_pairs(X, F, K)


# =============================================================================================
# context-MLP glue (csrc/mlp.hip): dense backward epilogue, BatchNorm training
# =============================================================================================
def _mat(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or not t.is_cuda:
        raise ValueError(f"{name}: expected a row-major fp32 device matrix, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return t


def bn_partial_rows(rows: int) -> int:
    return int(_lib_().recalgo_batchnorm_partial_rows(int(rows)))


def dense_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], relu: bool,
              x2: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
              bn_partials: Optional[torch.Tensor] = None, drop: Optional["DropSpec"] = None) -> torch.Tensor:
    """act(x @ w (+ x2 @ w2) + bias) on the fp32 matrix cores (include/recalgo.h recalgo_dense_fwd).  bn_partials
    [bn_partial_rows(M), 2 N]: the launch also leaves the per-tile batch moments of the result there, for the BatchNorm
    layer that consumes it (batchnorm_train_fwd(..., partials=)).  drop: the dropout behind the layer rides in the
    epilogue — y, and the moments, are those of the dropped tensor."""
    x, w = _mat(x, "x"), _mat(w, "w")
    M, K = x.shape
    N = w.shape[1]
    if w.shape[0] != K or w.stride(0) != N:
        raise ValueError("dense_fwd: w must be a contiguous [K, N] matrix")
    if x2 is not None:
        x2, w2 = _mat(x2, "x2"), _mat(w2, "w2")
        if w2.shape != (x2.shape[1], N) or w2.stride(0) != N or x2.shape[0] != M:
            raise ValueError("dense_fwd: second operand pair does not match")
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    if bn_partials is not None and (tuple(bn_partials.shape) != (bn_partial_rows(M), 2 * N) or not bn_partials.is_contiguous()):
        raise ValueError("dense_fwd: bn_partials must be a contiguous [bn_partial_rows(M), 2 N] tensor")
    if drop is not None:
        drop.check_mask((M, N))
    cd, _keep = _cdrop(drop)
    _lib_().recalgo_dense_fwd(
        _p(x), x.stride(0), _p(w), K, _p(x2), 0 if x2 is None else x2.stride(0), _p(w2), 0 if x2 is None else x2.shape[1],
        _p(bias), M, N, int(relu), _ACT_NONE, None, None, _p(y), N, _p(bn_partials), cd, _stream(x))
    return y


def dense_fwd_act(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], kind: int, alpha: torch.Tensor,
                  bn_partials: torch.Tensor):
    """z = x @ w + bias, y = prelu | dice (z, alpha) and the per-tile batch moments of y in ONE launch
    (recalgo_dense_fwd): the forward of DIN's dense -> activation -> batch_norm layers up to the BatchNorm merge.
    -> (z, y)"""
    x, w = _mat(x, "x"), _mat(w, "w")
    M, K = x.shape
    N = w.shape[1]
    if w.shape[0] != K or w.stride(0) != N:
        raise ValueError("dense_fwd_act: w must be a contiguous [K, N] matrix")
    if tuple(bn_partials.shape) != (bn_partial_rows(M), 2 * N) or not bn_partials.is_contiguous():
        raise ValueError("dense_fwd_act: bn_partials must be a contiguous [bn_partial_rows(M), 2 N] tensor")
    z = torch.empty(M, N, device=x.device, dtype=torch.float32)
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    _lib_().recalgo_dense_fwd(_p(x), x.stride(0), _p(w), K, None, 0, None, 0, _p(bias), M, N, 0, int(kind), _p(alpha), _p(z), _p(y),
                              N, _p(bn_partials), None, _stream(x))
    return z, y


def dense_bwd_input(g: torch.Tensor, y_mask: Optional[torch.Tensor], w: torch.Tensor, c_in: Optional[torch.Tensor] = None,
                    beta: float = 0.0, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """dx = (g * [y_mask > 0]) @ w^T (+ beta * c_in); y_mask contiguous with g's layout (recalgo_dense_bwd_input)."""
    g, w = _mat(g, "g"), _mat(w, "w")
    M, N = g.shape
    K = w.shape[0]
    if w.shape[1] != N or w.stride(0) != N:
        raise ValueError("dense_bwd_input: w must be a contiguous [K, N] matrix")
    if y_mask is not None and (y_mask.shape != g.shape or y_mask.stride() != g.stride()):
        raise ValueError("dense_bwd_input: y_mask must have g's layout")
    dx = out if out is not None else torch.empty(M, K, device=g.device, dtype=torch.float32)
    _lib_().recalgo_dense_bwd_input(_p(g), g.stride(0), _p(y_mask), _p(w), M, N, K, _p(c_in), 0 if c_in is None else c_in.stride(0),
                                    float(beta), _p(dx), dx.stride(0), int(accumulate), _stream(g))
    return dx


_dense_ws = {}


def dense_bwd_weights(x: torch.Tensor, g: torch.Tensor, y_mask: Optional[torch.Tensor], dw: torch.Tensor,
                      dbias: Optional[torch.Tensor], defer: bool = False) -> None:
    """dw = x^T (g * [y_mask > 0]), dbias = colsum(g * [y_mask > 0]) (recalgo_dense_bwd_weights; deterministic).
    `defer`: the fixed-order sum of the batch-split partials is left to `flush_dense_splits()` (one launch for all
    the layers of a backward pass; the optimizer and `named_grads` call it) — dw / dbias are valid only after it."""
    x, g = _mat(x, "x"), _mat(g, "g")
    M, K = x.shape
    N = g.shape[1]
    if g.shape[0] != M or tuple(dw.shape) != (K, N) or not dw.is_contiguous():
        raise ValueError("dense_bwd_weights: shape mismatch")
    if y_mask is not None and (y_mask.shape != g.shape or y_mask.stride() != g.stride()):
        raise ValueError("dense_bwd_weights: y_mask must have g's layout")
    lib = _lib_()
    if M == 0:
        dw.zero_()
        if dbias is not None:
            dbias.zero_()
        return
    # own scratch per weight tensor: a deferred reduction reads it after later layers have run
    nbytes = int(lib.recalgo_dense_bwd_weights_workspace_bytes(M, K, N))
    key = (x.device.type, x.device.index, M, K, N, dw.data_ptr() if defer else 0)
    ws = _dense_ws.get(key)
    if ws is None:
        ws = _dense_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    defer = bool(defer and nbytes > 0)
    lib.recalgo_dense_bwd_weights(_p(x), x.stride(0), _p(g), g.stride(0), _p(y_mask), M, K, N, _p(dw), _p(dbias),
                                  _p(ws), int(defer), _stream(x))
    if defer:
        _dense_pending.append((M, K, N, ws, dw, dbias))


def dense_bwd(x: torch.Tensor, g: torch.Tensor, y_mask: Optional[torch.Tensor], w: torch.Tensor, dw: torch.Tensor,
              dbias: Optional[torch.Tensor], c_in: Optional[torch.Tensor] = None, beta: float = 0.0,
              defer: bool = False, bn=None, premask: Optional[torch.Tensor] = None, cross_rider: bool = True) -> torch.Tensor:
    """Both gradients of a dense layer in one launch (recalgo_dense_bwd): returns dx = (g * [y_mask > 0]) @ w^T
    (+ beta * c_in); dw / dbias as dense_bwd_weights (valid after flush_dense_splits() when `defer`).
    premask [M, K] (rows contiguous): dx is zeroed where premask <= 0 (before the beta * c_in term) — x itself when x is the
    ReLU output of the layer below, whose backward then needs no mask (nn.ReluSource).
    bn = (bn_x [M, K] contiguous, mean [K], rstd [K], partials [bn_partial_rows(M), 2 K]): x is the output of a training-mode
    BatchNorm over bn_x — the launch also leaves the sums that BatchNorm's backward starts with."""
    global _cross_rider
    x, g, w = _mat(x, "x"), _mat(g, "g"), _mat(w, "w")
    M, K = x.shape
    N = g.shape[1]
    if M == 0:
        dense_bwd_weights(x, g, y_mask, dw, dbias)
        return torch.zeros(0, K, device=g.device, dtype=torch.float32)
    if g.shape[0] != M or tuple(dw.shape) != (K, N) or not dw.is_contiguous() or tuple(w.shape) != (K, N) or w.stride(0) != N:
        raise ValueError("dense_bwd: shape mismatch")
    if y_mask is not None and (y_mask.shape != g.shape or y_mask.stride() != g.stride()):
        raise ValueError("dense_bwd: y_mask must have g's layout")
    lib = _lib_()
    nbytes = int(lib.recalgo_dense_bwd_weights_workspace_bytes(M, K, N))
    key = (x.device.type, x.device.index, M, K, N, dw.data_ptr() if defer else 0)
    ws = _dense_ws.get(key)
    if ws is None:
        ws = _dense_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    defer = bool(defer and nbytes > 0)
    dx = torch.empty(M, K, device=g.device, dtype=torch.float32)
    bnp = (None, None, None, None)
    if bn is not None:
        bx, bmean, brstd, bpart = bn
        if (tuple(bx.shape) != (M, K) or not bx.is_contiguous() or bmean.numel() != K or brstd.numel() != K
                or tuple(bpart.shape) != (bn_partial_rows(M), 2 * K) or not bpart.is_contiguous()):
            raise ValueError("dense_bwd: bn = (x [M, K], mean [K], rstd [K], partials [bn_partial_rows(M), 2 K])")
        bnp = (_p(bx), _p(bmean), _p(brstd), _p(bpart))
    if premask is not None and (tuple(premask.shape) != (M, K) or premask.stride(1) != 1 or premask.dtype != torch.float32):
        raise ValueError("dense_bwd: premask must be [M, K] fp32 with contiguous rows")
    # the layer's own arguments of recalgo_dense_bwd, which recalgo_dense_bwd_rider starts with
    main = (_p(x), x.stride(0), _p(g), g.stride(0), _p(y_mask), _p(w), M, K, N, _p(c_in), 0 if c_in is None else c_in.stride(0),
            float(beta), _p(dx), K, _p(dw), _p(dbias), _p(ws), int(defer), *bnp, _p(premask),
            0 if premask is None else premask.stride(0))
    rider = _take_wgrad_rider(M, x.device) if defer else None
    crider = _take_cross_rider(M, x.device) if (defer and cross_rider and y_mask is None) else None
    if rider is not None or crider is not None:
        rx, rg, rdw, rdb = rider if rider is not None else (None, None, None, None)
        rK, rN = (rx.shape[1], rg.shape[1]) if rider is not None else (0, 0)
        if lib.recalgo_dense_bwd_rider_supported(_p(x), x.stride(0), _p(g), g.stride(0), _p(y_mask), _p(w), M, K, N, _p(dx), K,
                                                 _p(rx), 0 if rx is None else rx.stride(0), _p(rg), 0 if rg is None else rg.stride(0),
                                                 rK, rN):
            rws = _wgrad_workspace(rx.device, M, rK, rN, rdw) if rider is not None else None
            cargs, cdone = (None, 0, None, None, None, 0, 0, 0, None, None), None
            if crider is not None:
                cargs, cdone = _cross_rider_args(*crider)
            lib.recalgo_dense_bwd_rider(*main, _p(rx), 0 if rx is None else rx.stride(0), _p(rg), 0 if rg is None else rg.stride(0),
                                        rK, rN, _p(rdw), _p(rdb), _p(rws), *cargs, _stream(x))
            _dense_pending.append((M, K, N, ws, dw, dbias))
            if rider is not None:
                rider_stats["wgrad"] += 1
                if int(lib.recalgo_dense_bwd_weights_workspace_bytes(M, rK, rN)) > 0:
                    _dense_pending.append((M, rK, rN, rws, rdw, rdb))
            if cdone is not None:
                rider_stats["cross"] += 1
                cdone()
            return dx
        if rider is not None:
            dense_bwd_weights(rx, rg, None, rdw, rdb, defer=True)          # (not on the vectorised tile paths: a launch of its own)
        if crider is not None:
            _cross_rider = crider                                          # (left to the cross node's own backward)
    lib.recalgo_dense_bwd(*main, _stream(x))
    if defer:
        _dense_pending.append((M, K, N, ws, dw, dbias))
    return dx


# A weight gradient waiting for a launch to ride in (recalgo_dense_bwd_rider): the fused tail's backward leaves it (its layer's
# operands are ready, the layer below runs its merged backward next).
def defer_wgrad_rider(x: torch.Tensor, g: torch.Tensor, dw: torch.Tensor, dbias: Optional[torch.Tensor]) -> None:
    global _wgrad_rider
    launch_wgrad_rider()
    _wgrad_rider = (_mat(x, "x"), _mat(g, "g"), dw, dbias)


def _take_wgrad_rider(M: int, device):
    global _wgrad_rider
    r = _wgrad_rider
    if r is None or r[0].shape[0] != M or r[0].device != device or r[3] is None or not r[2].is_contiguous():
        return None
    _wgrad_rider = None
    return r


def launch_wgrad_rider() -> None:
    global _wgrad_rider
    if _wgrad_rider is not None:
        (rx, rg, rdw, rdb), _wgrad_rider = _wgrad_rider, None
        dense_bwd_weights(rx, rg, None, rdw, rdb, defer=True)


# The CrossNet backward waiting for a ride (recalgo_dense_bwd_rider's c_* arguments): the fused tail's backward produces the
# cross branch's upstream gradient long before autograd runs the cross node (created first, it runs last); the layer that
# shares x0 with the cross network needs the result, so only a dense_bwd WITHOUT a GradJoin of its own takes it.
rider_stats = {"wgrad": 0, "cross": 0}       # launches that carried a rider (tests / bench read it)


def defer_cross_rider(node, g: torch.Tensor) -> None:
    """node: the _CrossFn node of the cross output whose gradient g [B, d] the caller has just produced."""
    global _cross_rider
    _cross_rider = None
    if getattr(node, "grad_join", None) is None or not cross_riders_enabled:
        return
    w, _ = node.vars
    L = int(w.data.shape[0])
    if (g.dim() == 2 and g.is_contiguous() and g.dtype == torch.float32 and g.shape[1] == node.d and node.d % 4 == 0
            and g.data_ptr() % 16 == 0 and _lib_().recalgo_dense_bwd_cross_rider_supported(int(node.d), L)):
        _cross_rider = (node, g)


cross_riders_enabled = True


def _take_cross_rider(M: int, device):
    global _cross_rider
    r = _cross_rider
    if r is None or r[1].shape[0] != M or r[1].device != device:
        return None
    _cross_rider = None
    return r


def _cross_rider_args(node, g):
    """-> (the c_* arguments of recalgo_dense_bwd_rider, what to do once the launch is out)"""
    lib = _lib_()
    w, b = node.vars
    (x0p,) = node.saved_tensors
    B, dp = x0p.shape
    L = int(w.data.shape[0])
    key = ("cross", x0p.device.type, x0p.device.index, B, dp, L, w.grad.data_ptr())
    ws = _dense_ws.get(key)
    if ws is None:
        ws = _dense_ws[key] = torch.empty(max(int(lib.recalgo_cross_bwd_workspace_bytes(B, dp, L)), 16), dtype=torch.uint8,
                                          device=x0p.device)
    dx0 = torch.empty_like(x0p)
    join = node.grad_join

    def done():
        rows, wsf = int(lib.recalgo_cross_bwd_partial_rows(B)), ws.view(torch.float32)
        jobs = [(wsf, 0, rows, 2 * L * dp, L * dp, w.grad), (wsf, L * dp, rows, 2 * L * dp, L * dp, b.grad)]
        _colsum_pending.extend(jobs)
        join.early_dx, join.early_used = dx0, False
        node.early = (g, dx0, jobs, lambda: join.early_used)
    return (_p(x0p), dp, _p(w.data), _p(b.data), _p(g), g.stride(0), dp, L, _p(dx0), _p(ws)), done


def _wgrad_workspace(device, M, K, N, dw):
    nbytes = int(_lib_().recalgo_dense_bwd_weights_workspace_bytes(M, K, N))
    key = (device.type, device.index, M, K, N, dw.data_ptr())
    ws = _dense_ws.get(key)
    if ws is None:
        ws = _dense_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return ws


def flush_dense_splits(step_dev: Optional[torch.Tensor] = None) -> None:
    """Finish every deferred sum of the step in ONE launch: the weight-gradient split reductions of `dense`, the column
    sums the loss tail left behind, and (`step_dev`, the optimizer's int64 step counter) the step increment — the
    optimizer kernel that follows then only reads the counter."""
    _launch_dense_splits(*take_dense_splits(), step_dev)


def take_dense_splits():
    """The hand-over form of flush_dense_splits: everything it does but the launch -> (the _dense_pending entries, the
    _colsum_pending entries) of the step, for a launch that hosts the sums (adam_tf1_sum_step_) or, where that one refuses,
    for _launch_dense_splits."""
    launch_wgrad_rider()
    _dlogit_partials.clear()                 # (keyed by an address: no entry may outlive its step's deferred-sum launch)
    dense, colsums = list(_dense_pending), list(_colsum_pending)
    _dense_pending.clear()
    _colsum_pending.clear()
    return dense, colsums


def _split_job_arrays(dense, colsums):
    jobs = (_DenseSplit * max(len(dense), 1))()
    for i, (M, K, N, ws, dw, dbias) in enumerate(dense):
        jobs[i] = _DenseSplit(M, K, N, ws.data_ptr(), dw.data_ptr(), 0 if dbias is None else dbias.data_ptr())
    sums = (_ColSum * max(len(colsums), 1))()
    for i, (part, off, rows, stride, n, out) in enumerate(colsums):
        sums[i] = _ColSum(part.data_ptr() + 4 * off, out.data_ptr(), rows, stride, n)
    return jobs, sums


def _launch_dense_splits(dense, colsums, step_dev: Optional[torch.Tensor]) -> None:
    if not dense and not colsums and step_dev is None:
        return
    jobs, sums = _split_job_arrays(dense, colsums)
    dev_t = dense[0][4] if dense else (colsums[0][0] if colsums else step_dev)
    _lib_().recalgo_dense_bwd_weights_reduce(jobs, len(dense), sums, len(colsums), _p(step_dev), _stream(dev_t))


def mlp_width_supported(C: int) -> bool:
    return bool(_lib_().recalgo_mlp_width_supported(int(C)))


def relu_bwd_bias_(g: torch.Tensor, y: Optional[torch.Tensor], dbias: torch.Tensor) -> torch.Tensor:
    """g2 = g * [y > 0] (g itself when y is None), dbias[:] = colsum(g2); -> g2.  g, y [rows, C]."""
    rows, C = g.shape
    lib = _lib_()
    ws = _workspace(lib.recalgo_relu_bwd_bias_workspace_bytes(rows, C), g.device)
    g2 = None if y is None else torch.empty_like(g)
    lib.recalgo_relu_bwd_bias(_p(g), _p(y), rows, C, _p(g2), _p(dbias), _p(ws), _stream(g))
    return g if y is None else g2


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def dense1_supported(parts) -> bool:
    """The one-unit head kernel takes 1..4 contiguous fp32 [B, w] device tensors with one B."""
    return (1 <= len(parts) <= 4 and all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
                                         and t.shape[0] == parts[0].shape[0] and t.shape[1] >= 1 for t in parts))


def dense1_fwd(parts, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """[B, 1] = concat(parts, -1) @ w + bias without the concat (include/recalgo.h recalgo_dense1_fwd)."""
    import ctypes
    B = parts[0].shape[0]
    widths = (ctypes.c_int * len(parts))(*[int(t.shape[1]) for t in parts])
    out = torch.empty(B, 1, dtype=torch.float32, device=parts[0].device)
    _lib_().recalgo_dense1_fwd(_ptr_array(parts), widths, len(parts), B, _p(w), _p(bias), _p(out), _stream(out))
    return out


def dense1_bwd(parts, w: torch.Tensor, g: torch.Tensor, dxs, dw: torch.Tensor, dbias: Optional[torch.Tensor]) -> None:
    import ctypes
    B, C = parts[0].shape[0], sum(int(t.shape[1]) for t in parts)
    lib = _lib_()
    widths = (ctypes.c_int * len(parts))(*[int(t.shape[1]) for t in parts])
    ws = _workspace(lib.recalgo_dense1_bwd_workspace_bytes(B, C), g.device)
    lib.recalgo_dense1_bwd(_ptr_array(parts), widths, len(parts), B, _p(w), _p(g), _ptr_array(dxs), _p(dw), _p(dbias),
                           _p(ws), _stream(g))


def batchnorm_train_fwd(x, gamma, beta, moving_mean, moving_var, momentum: float, eps: float, partials=None,
                        out_drop: Optional["DropSpec"] = None):
    """Per-tile moments, then merge + apply.  partials: the per-tile moments of x when its producer has already left them
    (dense_fwd(bn_partials=)): ONE launch instead of two.  out_drop: the dropout BEHIND the BatchNorm rides in the store."""
    rows, C = x.shape
    lib = _lib_()
    y = torch.empty_like(x)
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    rstd = torch.empty(C, device=x.device, dtype=torch.float32)
    if out_drop is not None:
        out_drop.check_mask((rows, C))
    if partials is None:
        partials = _workspace(bn_partial_rows(rows) * 2 * C * 4, x.device)
        lib.recalgo_batchnorm_moments(_p(x), rows, C, _p(partials), _stream(x))
    cd, _keep = _cdrop(out_drop)
    lib.recalgo_batchnorm_apply(_p(x), _p(gamma), _p(beta), _p(partials), 1, rows, C, eps, momentum, _p(moving_mean),
                                _p(moving_var), _p(y), _p(mean), _p(rstd), cd, _stream(x))
    return y, mean, rstd


def batchnorm_train_bwd_act(x, gamma, mean, rstd, g, dgamma, dbeta, kind: int, z, alpha, dalpha, defer: bool,
                            sums=None, g_drop: Optional["DropSpec"] = None) -> torch.Tensor:
    """BatchNorm backward continued through the per-channel activation x = act(z, alpha) (recalgo_batchnorm_train_bwd):
    -> dL/dz; dgamma / dbeta / dalpha are overwritten (`defer`: dalpha by the step's deferred-sum launch).  g_drop: the
    BatchNorm's output went through a dropout — g is read as g * keep / (1 - rate) (sums of the un-dropped g are of no use)."""
    rows, C = x.shape
    lib = _lib_()
    nbytes = int(lib.recalgo_batchnorm_bwd_workspace_bytes(rows, C))
    dz = torch.empty_like(x)
    if defer:
        key = ("bn_act", x.device.type, x.device.index, rows, C, dalpha.data_ptr())
        ws = _dense_ws.get(key)
        if ws is None:
            ws = _dense_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    else:
        ws = _workspace(nbytes, x.device)
    cd, _keep = _cdrop(g_drop)
    lib.recalgo_batchnorm_train_bwd(_p(x), _p(gamma), _p(mean), _p(rstd), _p(g), None if g_drop is not None else _p(sums),
                                    rows, C, int(kind), _p(z), _p(alpha), _p(dz), _p(dgamma), _p(dbeta),
                                    None if defer else _p(dalpha), _p(ws), 0, 1.0, cd, _stream(x))
    if defer:
        nb = bn_partial_rows(rows)
        _colsum_pending.append((ws.view(torch.float32), nb * 2 * C, nb, C, C, dalpha))
    return dz


_syncbn_rows_checked = set()


def _syncbn_check_rows(rows: int, world: int, all_gather, device) -> None:
    """The Sync-BatchNorm kernels weigh every rank's tiles by the LOCAL row count: every rank must hold the same number of
    examples (weak scaling with drop_remainder; a ragged last batch would give wrong global statistics, or a hang when the
    tile counts differ).  Checked once per batch size (one tiny all_gather), outside a capture."""
    key = (int(rows), int(world))
    if key in _syncbn_rows_checked or (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
        return
    got = torch.empty(world, 1, device=device, dtype=torch.float32)
    all_gather(got, torch.full((1,), float(rows), device=device))
    if not bool((got == float(rows)).all()):
        raise ValueError(f"sync_batch_norm: every rank must hold the same number of examples per step (this rank: {rows}, "
                         f"ranks: {got.reshape(-1).tolist()}); drop the ragged last batch")
    _syncbn_rows_checked.add(key)


def batchnorm_sync_fwd(x, gamma, beta, moving_mean, moving_var, momentum: float, eps: float, sync):
    """Sync-BatchNorm forward (include/recalgo.h "Sync-BatchNorm building blocks"): per-tile moments -> all_gather of the
    partial rows over the data-parallel group -> merge + apply.  sync = (world, rank, all_gather(out [world, n], in [n])).
    Every rank must hold the same number of rows (checked once per batch size)."""
    world, _, all_gather = sync
    rows, C = x.shape
    _syncbn_check_rows(rows, world, all_gather, x.device)
    lib = _lib_()
    nb = int(lib.recalgo_batchnorm_partial_rows(rows))
    local = torch.empty(nb * 2 * C, device=x.device, dtype=torch.float32)
    lib.recalgo_batchnorm_moments(_p(x), rows, C, _p(local), _stream(x))
    parts = torch.empty(world, nb * 2 * C, device=x.device, dtype=torch.float32)
    all_gather(parts, local)
    y = torch.empty_like(x)
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    rstd = torch.empty(C, device=x.device, dtype=torch.float32)
    lib.recalgo_batchnorm_apply(_p(x), _p(gamma), _p(beta), _p(parts), world, rows, C, eps, momentum,
                                _p(moving_mean), _p(moving_var), _p(y), _p(mean), _p(rstd), None, _stream(x))
    return y, mean, rstd


def batchnorm_sync_bwd(x, gamma, mean, rstd, g, dgamma, dbeta, sync) -> torch.Tensor:
    world, rank, all_gather = sync
    rows, C = x.shape
    lib = _lib_()
    nb = int(lib.recalgo_batchnorm_partial_rows(rows))
    local = torch.empty(nb * 2 * C, device=x.device, dtype=torch.float32)
    lib.recalgo_batchnorm_bwd_sums(_p(x), _p(mean), _p(rstd), _p(g), rows, C, _p(local), _stream(x))
    parts = torch.empty(world, nb * 2 * C, device=x.device, dtype=torch.float32)
    all_gather(parts, local)
    dx = torch.empty_like(x)
    lib.recalgo_batchnorm_bwd_apply(_p(x), _p(gamma), _p(mean), _p(rstd), _p(g), _p(parts), world, rank, rows, C,
                                    _p(dx), _p(dgamma), _p(dbeta), 0, _stream(x))
    return dx


def batchnorm_train_bwd(x, gamma, mean, rstd, g, dgamma, dbeta, sums=None, relu_x: bool = False, relu_scale: float = 1.0,
                        g_drop: Optional["DropSpec"] = None) -> torch.Tensor:
    """sums [bn_partial_rows(rows), 2 C]: the per-tile (colsum g | colsum g * xhat) rows when g's producer has left them
    (dense_bwd(bn=)): ONE launch (merge + apply) instead of two.  relu_x: x is a ReLU output — dx is zeroed where x <= 0
    (the producing dense layer then needs no mask: nn.ReluSource); relu_scale = 1 / (1 - rate) when x also went through a
    dropout in front of this BatchNorm (dense(relu) -> dropout -> batch_norm).  g_drop: a dropout BEHIND this BatchNorm."""
    rows, C = x.shape
    lib = _lib_()
    dx = torch.empty_like(x)
    if sums is not None and relu_scale == 1.0 and g_drop is None:
        lib.recalgo_batchnorm_bwd_apply(_p(x), _p(gamma), _p(mean), _p(rstd), _p(g), _p(sums), 1, 0, rows, C, _p(dx),
                                        _p(dgamma), _p(dbeta), int(relu_x), _stream(x))
        return dx
    ws = _workspace(lib.recalgo_batchnorm_bwd_workspace_bytes(rows, C), x.device)
    cd, _keep = _cdrop(g_drop)
    lib.recalgo_batchnorm_train_bwd(_p(x), _p(gamma), _p(mean), _p(rstd), _p(g), None if g_drop is not None else _p(sums),
                                    rows, C, _ACT_NONE, None, None, _p(dx), _p(dgamma), _p(dbeta), None, _p(ws), int(relu_x),
                                    float(relu_scale), cd, _stream(x))
    return dx


# =============================================================================================
# a14: loss tail
# =============================================================================================
# The gradient the training loop seeds the loss with (1, or 1/world under data parallelism) is known
# before the forward runs: inside `loss_seed(c)` the loss kernel bakes c into dlogit and the backward
# hands dlogit on unchanged — no ones_like fill, no scaling launch.  The caller promises to seed
# loss.backward() with exactly c (Estimator.train_step does).
_loss_seed: Optional[float] = None


class loss_seed:
    def __init__(self, c: float):
        self.c = float(c)

    def __enter__(self):
        global _loss_seed
        self.prev, _loss_seed = _loss_seed, self.c
        return self

    def __exit__(self, *exc):
        global _loss_seed
        _loss_seed = self.prev
        return False


class _SigmoidCEFn(Function):
    @staticmethod
    def forward(ctx, logits, labels):
        ctx.set_materialize_grads(False)      # no zero tensor for the (non-differentiable) probabilities
        ctx.seed = _loss_seed
        B = logits.numel()
        lg = logits.contiguous().view(-1)
        lb = labels.contiguous().view(-1).to(torch.float32)
        prob = torch.empty_like(lg)
        loss = torch.empty(1, device=lg.device, dtype=torch.float32)
        dlogit = torch.empty_like(lg)
        _lib_().recalgo_sigmoid_ce_fwd_bwd(
            _p(lg), _p(lb), B, 1.0 if ctx.seed is None else ctx.seed, _p(prob), _p(loss), _p(dlogit), _stream(lg))
        ctx.save_for_backward(dlogit)
        ctx.shape = logits.shape
        ctx.mark_non_differentiable(prob)
        return loss.view(()), prob.view(logits.shape)

    @staticmethod
    def backward(ctx, gloss, _gprob):
        (dlogit,) = ctx.saved_tensors
        if gloss is None:
            return None, None
        if ctx.seed is not None:
            return dlogit.view(ctx.shape), None
        return (dlogit * gloss).view(ctx.shape), None


def sigmoid_cross_entropy(logits: torch.Tensor, labels: torch.Tensor):
    """-> (mean loss scalar, probabilities)."""
    return _SigmoidCEFn.apply(logits, labels)


class _LogitLossFn(Function):
    """TRAIN-step tail in one launch (include/recalgo.h recalgo_logit_loss_fwd_bwd): one-unit head(s) + sigmoid-CE +
    their backward.  Requires the loss-gradient seed to be known (ops.loss_seed): the gradients are produced by the
    forward launch, the backward only hands them out.  The loss VALUE and the head's weight / bias gradients are
    column sums of per-workgroup partials, finished by the step's deferred-sum launch (flush_dense_splits)."""

    @staticmethod
    def forward(ctx, anchor, labels, heads, bias, n_addends, loss_addend, *tensors):
        # heads: [(kernel Variable, n_parts)]; tensors = parts of all heads (in order) + the addend tensors [B, 1]
        ctx.set_materialize_grads(False)
        lib = _lib_()
        n_parts = sum(n for _, n in heads)
        parts, addends = list(tensors[:n_parts]), list(tensors[n_parts:])
        B = parts[0].shape[0]
        dev = parts[0].device
        widths = [int(t.shape[1]) for t in parts]
        C = sum(widths)
        ws_w, i = [], 0
        for kernel, n in heads:                      # weight slice of every part inside its head's (sum w, 1) kernel
            off = 0
            for t in parts[i:i + n]:
                ws_w.append(kernel.data.reshape(-1)[off:off + t.shape[1]])
                off += t.shape[1]
            i += n
        rows = int(lib.recalgo_logit_loss_partial_rows(B))
        partials = torch.empty(rows, C + 2, device=dev, dtype=torch.float32)
        logit = torch.empty(B, 1, device=dev, dtype=torch.float32)
        prob, dlogit = torch.empty_like(logit), torch.empty_like(logit)
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        need = ctx.needs_input_grad[6:6 + n_parts]
        dxs = [torch.empty_like(t) if nd else None for t, nd in zip(parts, need)]
        # a part that IS the ReLU output of a dense layer gets its gradient already masked (nn.ReluSource)
        # (not one that also went through a fused dropout: the mask here does not scale — its producer masks and scales itself)
        srcs = [getattr(t, "_recalgo_relu_src", None) if (nd and getattr(t, "_recalgo_relu_scale", 1.0) == 1.0) else None
                for t, nd in zip(parts, need)]
        relu_flags = (ctypes.c_int * n_parts)(*[int(sr is not None) for sr in srcs])
        lb = labels.contiguous().view(-1).to(torch.float32)
        wi = (ctypes.c_int * n_parts)(*widths)
        lib.recalgo_logit_loss_fwd_bwd(_ptr_array(parts), _ptr_array(ws_w), wi, n_parts, None if bias is None else _p(bias.data),
                                       _p(addends[0].contiguous().view(-1)) if n_addends > 0 else None,
                                       _p(addends[1].contiguous().view(-1)) if n_addends > 1 else None, _p(lb), _p(loss_addend), B,
                                       float(_loss_seed), _p(logit), _p(prob), _p(dlogit), _ptr_array(dxs), relu_flags,
                                       _p(partials), _stream(logit))
        for sr, dxp in zip(srcs, dxs):
            if sr is not None:
                sr.premasked = dxp
        # deferred column sums: dw of every head (contiguous columns of the partial rows), d bias, the loss value
        col, i = 0, 0
        for kernel, n in heads:
            wsum = sum(widths[i:i + n])
            if hasattr(kernel, "colsum_jobs"):           # (a derived kernel delivers its gradient itself: ops._PairKernel)
                _colsum_pending.extend(kernel.colsum_jobs(partials, col, rows, C + 2))
            else:
                _colsum_pending.append((partials, col, rows, C + 2, wsum, kernel.grad))
            col += wsum
            i += n
        if bias is not None:
            _colsum_pending.append((partials, C, rows, C + 2, 1, bias.grad))
        _colsum_pending.append((partials, C + 1, rows, C + 2, 1, loss))
        _dlogit_partials.clear()                     # sum_b dlogit[b] = column C of the partial rows (colsum_of_dlogit)
        _dlogit_partials[dlogit.data_ptr()] = (partials, C, rows, C + 2, B)
        ctx.dxs, ctx.dlogit, ctx.n_addends = dxs, dlogit, n_addends
        ctx.mark_non_differentiable(prob, logit)
        return loss.view(()), prob, logit

    @staticmethod
    def backward(ctx, gloss, _gprob, _glogit):
        if gloss is None:
            return (None,) * (6 + len(ctx.dxs) + ctx.n_addends)
        # the seed was baked into dlogit / dx by the forward launch (the caller promises to seed backward with it)
        return (None, None, None, None, None, None, *ctx.dxs, *([ctx.dlogit] * ctx.n_addends))


class _TailDenseHeadFn(Function):
    """The last hidden layer + the one-unit head + sigmoid-CE + the backward of all three down to the layer's input, in ONE
    launch (include/recalgo.h recalgo_tail_dense_head_fwd_bwd; DCN's tail, dcn.py:166-172).  As _LogitLossFn: the loss-gradient
    seed is known, the forward launch produces the gradients, the backward hands them out — and launches the layer's weight
    gradient (a batch reduction: its own launch, split partials summed by the step's deferred-sum launch)."""

    @staticmethod
    def forward(ctx, anchor, labels, head_kernel, head_bias, w3, b3, side_first, loss_addend, h2, side):
        ctx.set_materialize_grads(False)
        lib = _lib_()
        B, K2 = h2.shape
        N3 = int(w3.data.shape[1])
        Cs = 0 if side is None else int(side.shape[1])
        C = Cs + N3
        dev = h2.device
        hk = head_kernel.data.reshape(-1)
        w_side, w_h3 = (hk[:Cs], hk[Cs:]) if side_first else (hk[N3:], hk[:N3])
        rows = int(lib.recalgo_tail_partial_rows(B))
        partials = torch.empty(rows, C + 2, device=dev, dtype=torch.float32)
        logit = torch.empty(B, 1, device=dev, dtype=torch.float32)
        prob, dlogit = torch.empty_like(logit), torch.empty_like(logit)
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        d_side = torch.empty_like(side) if (side is not None and ctx.needs_input_grad[9]) else None
        dz3 = torch.empty(B, N3, device=dev, dtype=torch.float32)
        dh2 = torch.empty_like(h2)
        lb = labels.contiguous().view(-1).to(torch.float32)
        lib.recalgo_tail_dense_head_fwd_bwd(
            _p(h2), K2, _p(w3.data), _p(b3.data), N3, _p(side), Cs, int(bool(side_first)), _p(w_side) if Cs else None, _p(w_h3),
            None if head_bias is None else _p(head_bias.data), _p(lb), _p(loss_addend), B, float(_loss_seed), _p(logit), _p(prob),
            _p(dlogit), _p(d_side), _p(dz3), _p(dh2), _p(partials), _stream(logit))
        src = getattr(h2, "_recalgo_relu_src", None)
        if src is not None:
            src.premasked = dh2                        # masked with h2 > 0 by the kernel: the producing layer skips its own mask
        if hasattr(head_kernel, "colsum_jobs"):
            _colsum_pending.extend(head_kernel.colsum_jobs(partials, 0, rows, C + 2))
        else:
            _colsum_pending.append((partials, 0, rows, C + 2, C, head_kernel.grad))
        if head_bias is not None:
            _colsum_pending.append((partials, C, rows, C + 2, 1, head_bias.grad))
        _colsum_pending.append((partials, C + 1, rows, C + 2, 1, loss))
        _dlogit_partials.clear()
        _dlogit_partials[dlogit.data_ptr()] = (partials, C, rows, C + 2, B)
        ctx.h2, ctx.dz3, ctx.dh2, ctx.d_side, ctx.vars = h2, dz3, dh2, d_side, (w3, b3)
        ctx.cross_node = getattr(side, "_recalgo_cross_node", None) if side is not None else None
        ctx.mark_non_differentiable(prob, logit)
        return loss.view(()), prob, logit

    @staticmethod
    def backward(ctx, gloss, _gprob, _glogit):
        if gloss is None:
            return (None,) * 10
        w3, b3 = ctx.vars
        # (rides in the launch of the layer below's backward, which autograd runs next: ops.dense_bwd picks it up)
        defer_wgrad_rider(ctx.h2, ctx.dz3, w3.grad, b3.grad)
        if ctx.cross_node is not None and ctx.d_side is not None:
            # ... and so does the backward of the cross network `side` came out of: autograd would run that node last
            defer_cross_rider(ctx.cross_node, ctx.d_side)
        return (None, None, None, None, None, None, None, None, ctx.dh2, ctx.d_side)


def tail_dense_head_supported(h2, units: int, side) -> bool:
    """recalgo_tail_dense_head_fwd_bwd serves this last-hidden-layer / head pair (inside a training step whose loss seed is known)."""
    if _loss_seed is None or not torch.is_grad_enabled():
        return False
    for t in (h2, side):
        if t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
                and t.data_ptr() % 16 == 0):
            return False
    if side is not None and side.shape[0] != h2.shape[0]:
        return False
    return bool(_lib_().recalgo_tail_dense_head_supported(int(h2.shape[1]), int(units), 0 if side is None else int(side.shape[1])))


def tail_dense_head(store, labels, head_kernel, head_bias, w3, b3, h2, side, side_first: bool,
                    loss_addend: Optional[torch.Tensor] = None):
    """-> (mean sigmoid-CE loss (+ loss_addend), probabilities [B, 1], logit [B, 1]) of
    logit = dense1(concat([side, relu(h2 w3 + b3)]) in the given order) + head_bias."""
    if loss_addend is not None:
        loss_addend = loss_addend.detach().reshape(1).to(torch.float32)
    return _TailDenseHeadFn.apply(store.anchor, labels, head_kernel, head_bias, w3, b3, bool(side_first), loss_addend, h2, side)


class _ConcatSumsqFn(Function):
    """torch.cat(parts, -1) with sum(out^2) * scale as a detached by-product (one launch, include/recalgo.h
    recalgo_concat_sumsq); the gradient of a part is its column block of the output's gradient."""

    @staticmethod
    def forward(ctx, scale, joins, *parts):
        lib = _lib_()
        ctx.joins = joins or {}
        parts = [t.contiguous() for t in parts]
        B = parts[0].shape[0]
        widths = [int(t.shape[1]) for t in parts]
        dev = parts[0].device
        out = torch.empty(B, sum(widths), device=dev, dtype=torch.float32)
        val = torch.empty(1, device=dev, dtype=torch.float32)
        key = ("concat_sumsq", dev.type, dev.index, B)
        ws = _dense_ws.get(key)
        if ws is None:
            ws = _dense_ws[key] = torch.zeros(int(lib.recalgo_concat_sumsq_workspace_bytes(B)), dtype=torch.uint8, device=dev)
        wi = (ctypes.c_int * len(parts))(*widths)
        lib.recalgo_concat_sumsq(_ptr_array(parts), wi, len(parts), B, _p(out), float(scale), _p(val), _p(ws), _stream(out))
        ctx.widths = widths
        ctx.mark_non_differentiable(val)
        ctx.set_materialize_grads(False)      # (else autograd fills a zero "gradient" for val: one launch per step)
        return out, val

    @staticmethod
    def backward(ctx, g, _gv):
        if g is None:
            return (None, None) + (None,) * len(ctx.widths)
        outs, off = [], 0
        for i, w in enumerate(ctx.widths):
            gi = g[:, off:off + w]
            join = ctx.joins.get(i)
            # (a part with a second consumer whose backward kernel adds this block itself: parked, not returned)
            outs.append(None if join is not None and join.park(gi) else gi)
            off += w
        return (None, None, *outs)


def concat_sumsq(parts, scale: float, joins=None):
    """-> (concat(parts, -1) [B, C], scale * sum(concat^2) as a detached [1] tensor); 1..4 fp32 [B, w] device tensors.
    joins {part index: nn.GradJoin}: that part's gradient block is parked for its other consumer's backward kernel."""
    return _ConcatSumsqFn.apply(float(scale), joins, *parts)


def colsum_of_dlogit(g: torch.Tensor, out: torch.Tensor) -> bool:
    """out[0] = sum_b g[b] as ONE MORE JOB of the step's deferred-sum launch, when g is the d(loss)/d(logit) vector the fused
    loss tail produced (a logit addend's gradient, e.g. DeepFM's first-order logit -> its bias): the tail's partial rows
    already hold the per-workgroup sums.  False: g is something else — the caller sums it itself."""
    e = _dlogit_partials.get(g.data_ptr())
    if e is None or g.numel() != e[4] or not g.is_contiguous():
        return False
    _colsum_pending.append((e[0], e[1], e[2], e[3], 1, out))
    return True


def logit_loss_supported(parts, addends) -> bool:
    return (_loss_seed is not None and torch.is_grad_enabled() and dense1_supported(parts) and len(addends) <= 2
            and sum(int(t.shape[1]) for t in parts) <= 4096          # the kernel keeps an [8, C] tile + the weights in LDS
            and all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 1 for t in addends))


def logit_loss(store, labels: torch.Tensor, heads, bias, parts, addends, loss_addend: Optional[torch.Tensor] = None):
    """-> (mean sigmoid-CE loss (+ loss_addend, a detached device scalar), probabilities [B,1], logit [B,1]) of
    logit = sum_heads dense1(parts) + bias + addends."""
    if loss_addend is not None:
        loss_addend = loss_addend.detach().reshape(1).to(torch.float32)
    return _LogitLossFn.apply(store.anchor, labels, heads, bias, len(addends), loss_addend, *parts, *addends)


# =============================================================================================
# MMoE (csrc/mmoe.hip): softmax gates + expert mix, the multi-task loss tail
# =============================================================================================
GATE_MIX_MAX = _C["RECALGO_GATE_MIX_MAX"]


def _colsum_now(jobs, device_tensor: torch.Tensor) -> None:
    """The fixed-order column sums of `jobs` (entries as in _colsum_pending) in a launch of their own."""
    sums = (_ColSum * len(jobs))()
    for i, (part, off, rows, stride, n, out) in enumerate(jobs):
        sums[i] = _ColSum(part.data_ptr() + 4 * off, out.data_ptr(), rows, stride, n)
    _lib_().recalgo_dense_bwd_weights_reduce((_DenseSplit * 1)(), 0, sums, len(jobs), None, _stream(device_tensor))


class _MixEntry(NamedTuple):
    """What differs between the two gate-mix ops (`gate_mix`: csrc/mmoe.hip, include/recalgo.h; `cgc_mix`: csrc/cgc.hip,
    include/recalgo_cgc.h) around their one autograd Function and their one argument check."""
    op: str                     # the public op's name: the prefix of every error text
    fwd: str                    # the forward entry point
    bwd: str                    # the backward entry point
    partial_rows: Callable      # (lib, B, In, n_total) -> rows of the backward's gate-kernel partials
    has_sum_outputs: bool       # the ABI carries `sum_outputs` (after H, in both entries)
    skip_unused_backward: bool  # a backward whose upstream gradients are all None launches nothing
    strict_gates: bool          # the argument check also refuses G < 1 and a gate kernel that is not 2-d


_GATE_MIX = _MixEntry("gate_mix", "recalgo_gate_mix_fwd", "recalgo_gate_mix_bwd",
                      lambda lib, B, In, n_total: lib.recalgo_gate_mix_partial_rows(B), False, False, False)
_CGC_MIX = _MixEntry("cgc_mix", "recalgo_cgc_fwd", "recalgo_cgc_bwd",
                     lambda lib, B, In, n_total: lib.recalgo_cgc_partial_rows(B, In, n_total), True, True, True)


class GateMixSpec:
    """What `_MixFn` needs besides its tensors: the gate kernels (Variables: the gradient goes to Variable.grad
    through the step's deferred column sums; tensors: returned by backward), the selection table, whether the experts are ReLU
    outputs whose gradient the op masks, where the gates' share of d x goes (x_grad_sink.first instead of autograd),
    (`cgc_mix` only) whether the G outputs are summed into one, and which of the two ops' entry points serve it."""

    def __init__(self, kernels, selection, relu_sources, x_grad_sink, sum_outputs: bool = False, entry: _MixEntry = _GATE_MIX):
        self.kernels, self.selection, self.relu_sources, self.x_grad_sink = kernels, selection, relu_sources, x_grad_sink
        self.sum_outputs, self.entry = bool(sum_outputs), entry
        self.n_sel = (ctypes.c_int * len(selection))(*[len(s) for s in selection])
        flat = [int(e) for s in selection for e in s]
        self.sel = (ctypes.c_int * len(flat))(*flat)
        self.n_total = len(flat)


def _mix_backward_tail(spec: GateMixSpec, ws, need_w, partials, rows, x, dx, dex):
    """What the backward of both gate-mix ops does once its kernel has run (-> the Function's return tuple): hands the masked
    expert gradients to the experts' ReluSources, turns the [rows, In * n_total] partial rows into the gate kernels' gradients
    (Variables: jobs of the step's deferred column sums; tensors: a fixed-order sum launched now) and offers d x to the sink."""
    if spec.relu_sources is not None:
        for src, d in zip(spec.relu_sources, dex):
            src.premasked = d                # (nn.ReluSource: the expert layers' backward then runs without mask loads)
    In, stride = x.shape[1], x.shape[1] * spec.n_total
    dws, now, off = [], [], 0
    for k, w, nd in zip(spec.kernels, ws, need_w):
        n = In * w.shape[1]
        if isinstance(k, Variable):
            _colsum_pending.append((partials, off, rows, stride, n, k.grad))
            dws.append(None)
        elif nd:
            dw = torch.empty_like(w)
            now.append((partials, off, rows, stride, n, dw))
            dws.append(dw)
        else:
            dws.append(None)
        off += n
    if now:
        _colsum_now(now, x)
    if dx is not None and spec.x_grad_sink is not None and spec.x_grad_sink.offer(dx):
        dx = None                            # (the other consumers of x add it in their input-gradient epilogue)
    return (None, None, dx, *dex, *dws)


class _MixFn(Function):
    """The softmax gates + expert mix of either op (spec.entry): include/recalgo.h recalgo_gate_mix_fwd / recalgo_gate_mix_bwd,
    G outputs [B, H]; include/recalgo_cgc.h recalgo_cgc_fwd / recalgo_cgc_bwd, G outputs or their sum as ONE (spec.sum_outputs)."""

    @staticmethod
    def forward(ctx, anchor, spec: GateMixSpec, x, *tensors):
        ctx.set_materialize_grads(False)     # a gate nobody differentiates: NULL upstream gradient, no zero tensor
        G = len(spec.kernels)
        experts, gate_ts = tensors[:len(tensors) - G], tensors[len(tensors) - G:]
        ws = [k.data if isinstance(k, Variable) else t for k, t in zip(spec.kernels, gate_ts)]
        B, In = x.shape
        E, H = len(experts), experts[0].shape[1]
        outs = [torch.empty(B, H, device=x.device, dtype=torch.float32) for _ in range(1 if spec.sum_outputs else G)]
        p = torch.empty(B, spec.n_total, device=x.device, dtype=torch.float32)
        summed = (int(spec.sum_outputs),) if spec.entry.has_sum_outputs else ()
        getattr(_lib_(), spec.entry.fwd)(_p(x), x.stride(0), _ptr_array(ws), spec.n_sel, spec.sel, _ptr_array(experts),
                                         B, In, E, G, H, *summed, _ptr_array(outs), _p(p), _stream(x))
        ctx.spec, ctx.ws, ctx.E = spec, ws, E
        ctx.save_for_backward(x, p, *experts)
        ctx.mark_non_differentiable(p)
        return (*outs, p)

    @staticmethod
    def backward(ctx, *grads):
        spec, ws, E = ctx.spec, ctx.ws, ctx.E
        x, p, *experts = ctx.saved_tensors
        G = len(ws)
        M = 1 if spec.sum_outputs else G
        gs = [_contig(g) for g in grads[:M]]
        if spec.entry.skip_unused_backward and all(g is None for g in gs):
            return (None,) * (3 + E + G)
        B, In = x.shape
        H = experts[0].shape[1]
        lib = _lib_()
        need_x = ctx.needs_input_grad[2]
        need_e = ctx.needs_input_grad[3:3 + E]
        dx = torch.empty(B, In, device=x.device, dtype=torch.float32) if need_x else None
        dex = [torch.empty_like(t) if nd else None for t, nd in zip(experts, need_e)]
        rows = int(spec.entry.partial_rows(lib, B, In, spec.n_total))
        partials = torch.empty(rows, In * spec.n_total, device=x.device, dtype=torch.float32)
        relu = spec.relu_sources is not None
        summed = (int(spec.sum_outputs),) if spec.entry.has_sum_outputs else ()
        getattr(lib, spec.entry.bwd)(_p(x), x.stride(0), _ptr_array(ws), spec.n_sel, spec.sel, _ptr_array(experts), _p(p),
                                     _ptr_array(gs), B, In, E, G, H, *summed, int(relu), _ptr_array(dex), _p(dx), In,
                                     _p(partials), _stream(x))
        return _mix_backward_tail(spec, ws, ctx.needs_input_grad[3 + E:], partials, rows, x, dx, dex)


def _mix_check(entry: _MixEntry, x, gate_kernels, experts, selection) -> int:
    """The shape checks both ops make before they ask their `_supported` query (-> H): ValueError, prefixed by the op's name."""
    op, E, G = entry.op, len(experts), len(gate_kernels)
    ws = [k.data if isinstance(k, Variable) else k for k in gate_kernels]
    if x.dim() != 2 or (entry.strict_gates and G < 1) or len(selection) != G or \
            any((entry.strict_gates and w.dim() != 2) or tuple(w.shape) != (x.shape[1], len(s)) for w, s in zip(ws, selection)):
        raise ValueError(f"{op}: one [In, n_g] gate kernel per selection row")
    if any(len(s) < 1 for s in selection) or any(e < 0 or e >= E for s in selection for e in s):
        raise ValueError(f"{op}: every gate selects at least one expert, indices in [0, E)")
    if E < 1 or any(t.dim() != 2 or t.shape != experts[0].shape or t.shape[0] != x.shape[0] for t in experts):
        raise ValueError(f"{op}: experts must be E same-shaped [B, H] tensors")
    return experts[0].shape[1]


def _mix_launch(entry: _MixEntry, x, gate_kernels, experts, selection, sum_outputs, x_grad_sink, anchor):
    """What both ops do once the shapes are inside their kernel's limits -> (outputs, gate probabilities)."""
    if x.shape[0] == 0:
        raise NotImplementedError(f"{entry.op}: empty batch")
    x = _mat(x, "x")
    for k in gate_kernels:
        _chk(k.data if isinstance(k, Variable) else k, torch.float32, "gate kernel")
    srcs = [getattr(t, "_recalgo_relu_src", None) if getattr(t, "_recalgo_relu_scale", 1.0) == 1.0 else None for t in experts]
    srcs = srcs if all(s is not None for s in srcs) else None
    experts = [_mat(_contig(t), "expert") for t in experts]
    spec = GateMixSpec(gate_kernels, selection, srcs, x_grad_sink, sum_outputs=sum_outputs, entry=entry)
    gate_ts = [None if isinstance(k, Variable) else k for k in gate_kernels]
    *outs, p = _MixFn.apply(anchor, spec, x, *experts, *gate_ts)
    return outs, p


def gate_mix_supported(In: int, E: int, G: int, H: int, n_total: int) -> bool:
    return bool(_lib_().recalgo_gate_mix_supported(int(In), int(E), int(G), int(H), int(n_total)))


def gate_mix(x: torch.Tensor, gate_kernels, experts, selection=None, x_grad_sink=None, anchor=None, return_gates: bool = False):
    """MMoE / CGC block behind the expert layers (mmoe.py:208-232): for every gate g,
        out_g = sum_j softmax(x @ gate_kernels[g])[:, j, None] * experts[selection[g][j]]
    x [B, In]; gate_kernels: G bias-free [In, n_g] kernels (Variables or tensors); experts: E [B, H] tensors;
    selection[g]: the n_g expert indices gate g mixes (default: every gate over all E experts, MMoE).
    -> the G outputs [B, H] (and the gate probabilities [B, sum n_g] with return_gates).
    Experts that carry an nn.ReluSource (outputs of ReLU expert layers) get their gradient already masked.
    x_grad_sink: an nn.InputGradChain shared with the other consumers of x — the gates' share of d x is handed to it instead
    of to autograd.  Outside the kernel's limits (recalgo_gate_mix_supported): NotImplementedError."""
    gate_kernels, experts = list(gate_kernels), list(experts)
    E, G = len(experts), len(gate_kernels)
    selection = [list(range(E)) for _ in range(G)] if selection is None else [list(s) for s in selection]
    H = _mix_check(_GATE_MIX, x, gate_kernels, experts, selection)
    n_total = sum(len(s) for s in selection)
    if max(len(s) for s in selection) > GATE_MIX_MAX or not gate_mix_supported(x.shape[1], E, G, H, n_total):
        raise NotImplementedError(
            f"gate_mix serves H % 4 == 0, E, G, n_g <= {GATE_MIX_MAX}, In <= 512 and In * (sum n_g | 1) <= 4096; got In={x.shape[1]} "
            f"E={E} G={G} H={H} sum n_g={n_total}")
    outs, p = _mix_launch(_GATE_MIX, x, gate_kernels, experts, selection, False, x_grad_sink, anchor)
    return (outs, p) if return_gates else outs


# =============================================================================================
# PLE (csrc/cgc.hip, include/recalgo_cgc.h): the CGC block — wide softmax gates + expert mix, optionally summed
# =============================================================================================
_CC = _lib.HEADERS["recalgo_cgc.h"].constants                 # the RECALGO_CGC_* #defines of include/recalgo_cgc.h
CGC_MAX_EXPERTS = _CC["RECALGO_CGC_MAX_EXPERTS"]
CGC_MAX_GATES = _CC["RECALGO_CGC_MAX_GATES"]
# include/recalgo_wide.h (the op itself lives in wide.py)
_CW = _lib.HEADERS["recalgo_wide.h"].constants
WIDE_HASH_KEY, WIDE_MAX_BUCKETS = _CW["RECALGO_WIDE_HASH_KEY"], _CW["RECALGO_WIDE_MAX_BUCKETS"]


def cgc_supported(In: int, E: int, G: int, H: int, n_total: int, n_max: int) -> bool:
    return bool(_lib_().recalgo_cgc_supported(int(In), int(E), int(G), int(H), int(n_total), int(n_max)))


def cgc_mix(x: torch.Tensor, gate_kernels, experts, selection, sum_outputs: bool = False, x_grad_sink=None, anchor=None,
            return_gates: bool = False):
    """PLE's CGC block (extraction_network.py:25-85, ple.py:185-226) at sizes beyond `gate_mix`: for every gate g,
        out_g = sum_j softmax(x @ gate_kernels[g])[:, j, None] * experts[selection[g][j]]
    x [B, In]; gate_kernels: G bias-free [In, n_g] kernels (Variables or tensors); experts: E [B, H] tensors;
    selection[g]: the n_g expert indices gate g mixes (duplicates allowed).
    -> the G outputs [B, H]; with sum_outputs ONE tensor, their sum (the tf.add_n an extraction network returns) — and the
    gate probabilities [B, sum n_g] with return_gates.
    Experts that carry an nn.ReluSource get their gradient already masked; x_grad_sink as in `gate_mix`.
    Malformed tables: ValueError.  Outside the kernel's limits (recalgo_cgc_supported) or an empty batch: NotImplementedError."""
    gate_kernels, experts = list(gate_kernels), list(experts)
    E, G = len(experts), len(gate_kernels)
    selection = [list(s) for s in selection]
    H = _mix_check(_CGC_MIX, x, gate_kernels, experts, selection)
    n_total, n_max = sum(len(s) for s in selection), max(len(s) for s in selection)
    if not cgc_supported(x.shape[1], E, G, H, n_total, n_max):
        raise NotImplementedError(
            f"cgc_mix serves H % 4 == 0, E <= {CGC_MAX_EXPERTS}, G <= {CGC_MAX_GATES}, n_g <= {CGC_MAX_EXPERTS}, In <= 512 and "
            f"In * (sum n_g | 1) <= 20480; got In={x.shape[1]} E={E} G={G} H={H} sum n_g={n_total} max n_g={n_max}")
    outs, p = _mix_launch(_CGC_MIX, x, gate_kernels, experts, selection, sum_outputs, x_grad_sink, anchor)
    outs = outs[0] if sum_outputs else outs
    return (outs, p) if return_gates else outs


class _MultiTaskCEFn(Function):
    """include/recalgo.h recalgo_multitask_sigmoid_ce_fwd_bwd: T sigmoid-CE tails and their sum in one launch."""

    @staticmethod
    def forward(ctx, labels, *logits):
        ctx.set_materialize_grads(False)
        ctx.seed = _loss_seed
        T, B = len(logits), logits[0].numel()
        lgs = [t.contiguous().view(-1) for t in logits]
        lbs = [t.contiguous().view(-1).to(torch.float32) for t in labels]
        dev = lgs[0].device
        prob = torch.empty(B, T, device=dev, dtype=torch.float32)
        losses = torch.empty(T, device=dev, dtype=torch.float32)
        total = torch.empty(1, device=dev, dtype=torch.float32)
        dlogit = torch.empty(T, B, device=dev, dtype=torch.float32)
        _lib_().recalgo_multitask_sigmoid_ce_fwd_bwd(_ptr_array(lgs), _ptr_array(lbs), T, B, 1.0 if ctx.seed is None else ctx.seed,
                                                     _p(prob), _p(losses), _p(total), _p(dlogit), _stream(lgs[0]))
        ctx.save_for_backward(dlogit)
        ctx.shapes = [t.shape for t in logits]
        ctx.mark_non_differentiable(prob)
        return total.view(()), losses, prob

    @staticmethod
    def backward(ctx, gtotal, glosses, _gprob):
        (dlogit,) = ctx.saved_tensors
        if gtotal is None and glosses is None:
            return (None,) * (1 + len(ctx.shapes))
        if ctx.seed is not None and glosses is None:
            return (None, *[dlogit[t].view(s) for t, s in enumerate(ctx.shapes)])     # (the seed is baked in: ops.loss_seed)
        out = []
        for t, s in enumerate(ctx.shapes):
            g = glosses[t] if glosses is not None else 0.0
            g = g + gtotal if gtotal is not None else g
            out.append((dlogit[t] * g).view(s))
        return (None, *out)


def multitask_sigmoid_cross_entropy(logits, labels):
    """T logits [B, 1] and T labels -> (sum of the tasks' mean sigmoid-CE (scalar), the T task losses [T], probabilities
    [B, T]); mmoe.py:235,247-249.  Every task's loss is `sigmoid_cross_entropy`'s value bit for bit."""
    logits, labels = list(logits), list(labels)
    if not 1 <= len(logits) <= GATE_MIX_MAX or len(labels) != len(logits):
        raise NotImplementedError(f"multitask_sigmoid_cross_entropy: 1..{GATE_MIX_MAX} tasks, one label tensor each")
    if any(t.numel() != logits[0].numel() for t in logits + labels) or logits[0].numel() == 0:
        raise ValueError("multitask_sigmoid_cross_entropy: T logits and T labels of one batch size")
    for t in logits:
        if t.dtype != torch.float32:
            raise TypeError("multitask_sigmoid_cross_entropy: fp32 logits")
        _stream(t)
    return _MultiTaskCEFn.apply(labels, *logits)


# =============================================================================================
# ESMM (csrc/esmm.hip, include/recalgo_esmm.h): the click loss and the entire-space click-and-conversion loss, one launch
# =============================================================================================
ESMM_MAX_ROWS = _lib.SERVING_HEADERS["recalgo_esmm.h"].constants["RECALGO_ESMM_MAX_ROWS"]


class _EsmmLossFn(Function):
    """include/recalgo_esmm.h recalgo_esmm_loss_fwd_bwd: both losses, their sum, the three probabilities and both logit
    gradients in one launch.  The header delivers each logit's gradient of the SUM, so only `total` is differentiable."""

    @staticmethod
    def forward(ctx, want, click, conversion, ctr_logit, cvr_logit):
        # want: a logit requires grad and grad mode is on, as esmm_loss saw it (inside forward grad mode is always off)
        ctx.set_materialize_grads(False)
        ctx.seed = _loss_seed
        B = ctr_logit.numel()
        a, b = ctr_logit.contiguous().view(-1), cvr_logit.contiguous().view(-1)
        y, c = (t.contiguous().view(-1).to(torch.float32) for t in (click, conversion))
        dev = a.device
        prob = torch.empty(B, 3, device=dev, dtype=torch.float32)
        losses = torch.empty(2, device=dev, dtype=torch.float32)
        total = torch.empty(1, device=dev, dtype=torch.float32)
        da, db = (torch.empty_like(a), torch.empty_like(b)) if want else (None, None)
        _lib_().recalgo_esmm_loss_fwd_bwd(_p(a), _p(b), _p(y), _p(c), B, 1.0 if ctx.seed is None else ctx.seed, _p(prob), _p(losses),
                                          _p(total), _p(da), _p(db), _stream(a))
        if want:
            ctx.save_for_backward(da, db)
        ctx.shapes = (ctr_logit.shape, cvr_logit.shape)
        ctx.mark_non_differentiable(losses, prob)
        return total.view(()), losses, prob

    @staticmethod
    def backward(ctx, gtotal, _glosses, _gprob):
        if gtotal is None or not ctx.saved_tensors:
            return None, None, None, None, None
        grads = ctx.saved_tensors
        if ctx.seed is None:
            grads = [d * gtotal for d in grads]                                       # (the seed is baked in otherwise: ops.loss_seed)
        return (None, None, None, *[d.view(s) if need else None for d, s, need in zip(grads, ctx.shapes, ctx.needs_input_grad[3:])])


def esmm_loss(ctr_logit: torch.Tensor, cvr_logit: torch.Tensor, click: torch.Tensor, conversion: torch.Tensor):
    """ESMM's loss over all impressions: L_ctr = mean sigmoid-CE(ctr_logit, click) — `sigmoid_cross_entropy`'s value bit for bit —
    plus L_ctcvr = mean CE(sigmoid(ctr_logit) sigmoid(cvr_logit), click * conversion), evaluated in logit space
    (include/recalgo_esmm.h).  Four tensors of B values -> (total (scalar, differentiable in both logits), the two losses [2],
    probabilities [B, 3]: pCTR, pCVR, pCTCVR)."""
    n = ctr_logit.numel()
    if any(t.numel() != n for t in (cvr_logit, click, conversion)) or n == 0:
        raise ValueError("esmm_loss: two logits and two labels of one batch size, at least one row")
    if n > ESMM_MAX_ROWS:
        raise NotImplementedError(f"esmm_loss: at most {ESMM_MAX_ROWS} rows")
    if ctr_logit.dtype != torch.float32 or cvr_logit.dtype != torch.float32:
        raise TypeError("esmm_loss: fp32 logits")
    _stream(ctr_logit), _stream(cvr_logit)
    want =torch.is_grad_enabled() and (ctr_logit.requires_grad or cvr_logit.requires_grad)
    return _EsmmLossFn.apply(want, click, conversion, ctr_logit, cvr_logit)


# =============================================================================================
# a12: PReLU / Dice
# =============================================================================================
class _ActFn(Function):
    @staticmethod
    def forward(ctx, anchor, x, alpha: Variable, kind: int):
        x = x.contiguous()
        rows, C = x.shape
        y = torch.empty_like(x)
        _lib_().recalgo_activation_fwd(_p(x), _p(alpha.data), rows, C, kind, _p(y), _stream(x))
        ctx.alpha, ctx.kind = alpha, kind
        ctx.in_step = _loss_seed is not None      # built inside Estimator.train_step: its optimizer runs the deferred sums
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        rows, C = x.shape
        lib = _lib_()
        gy = gy.contiguous()
        dx = torch.empty_like(x)
        nbytes = int(lib.recalgo_activation_bwd_workspace_bytes(rows, C))
        if ctx.in_step:
            # inside a training step: d(alpha) = column sum of the partial rows, a job of the step's deferred-sum launch
            key = ("act", x.device.type, x.device.index, rows, C, ctx.alpha.grad.data_ptr())
            ws = _dense_ws.get(key)
            if ws is None:
                ws = _dense_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
            lib.recalgo_activation_bwd(_p(x), _p(ctx.alpha.data), _p(gy), rows, C, ctx.kind, _p(dx), None, _p(ws), _stream(x))
            _colsum_pending.append((ws.view(torch.float32), 0, int(lib.recalgo_activation_bwd_partial_rows(rows, C)), C, C,
                                    ctx.alpha.grad))
            return None, dx, None, None
        ws = _workspace(nbytes, x.device)
        lib.recalgo_activation_bwd(_p(x), _p(ctx.alpha.data), _p(gy), rows, C, ctx.kind, _p(dx),
                                   _p(ctx.alpha.grad), _p(ws), _stream(x))
        return None, dx, None, None


def activation(store, x: torch.Tensor, alpha: Variable, kind: str) -> torch.Tensor:
    if store.building:
        return torch.zeros_like(x)
    return _ActFn.apply(store.anchor, x, alpha, _ACT[kind])


# =============================================================================================
# tf.layers.dropout (training mode)
# =============================================================================================
class DropSpec:
    """One training-mode tf.layers.dropout call: rate, and where its keep decisions come from — an explicit mask (parity
    tests replay the reference run's), or the counter-based hash of csrc/dropout.h keyed by (seed, call, device step counter)."""
    __slots__ = ("rate", "mask", "seed", "call", "step")

    def __init__(self, rate: float, mask: Optional[torch.Tensor], seed: int, call: int, step: Optional[torch.Tensor]):
        self.rate, self.mask, self.seed, self.call, self.step = float(rate), mask, int(seed) & 0x7FFFFFFF, int(call), step

    @property
    def scale(self) -> float:
        return 1.0 / (1.0 - self.rate)

    def check_mask(self, shape) -> None:
        if self.mask is not None and (tuple(self.mask.shape) != tuple(shape) or self.mask.dtype != torch.float32
                                      or not self.mask.is_contiguous()):
            raise ValueError("dropout: the explicit keep mask must be a contiguous fp32 tensor of the dropped tensor's shape")


def _cdrop(d: Optional["DropSpec"]):
    """-> (byref argument or None, keep-alive)"""
    if d is None:
        return None, None
    c = _CDrop(d.rate, None if d.mask is None else d.mask.data_ptr(), d.seed, d.call, None if d.step is None else d.step.data_ptr())
    return ctypes.byref(c), c


def _dropout_launch(x: torch.Tensor, d: DropSpec) -> torch.Tensor:
    y = torch.empty_like(x)
    _lib_().recalgo_dropout_fwd(_p(x), x.numel(), d.rate, _p(d.mask), d.seed, d.call, _p(d.step), _p(y), _stream(x))
    return y


class _DropoutFn(Function):
    @staticmethod
    def forward(ctx, x, d: DropSpec):
        ctx.d = d
        return _dropout_launch(x.contiguous(), d)

    @staticmethod
    def backward(ctx, g):
        # the gradient of the keep-mask scale is the same scale: the same map with the same key
        return _dropout_launch(g.contiguous(), ctx.d), None


def dropout(x: torch.Tensor, d: DropSpec) -> torch.Tensor:
    """y = x * keep / (1 - rate) as its own launch each way (a dropout no neighbouring kernel can absorb)."""
    _chk(x, torch.float32, "x")
    if d.mask is not None and (d.mask.shape != x.shape or d.mask.dtype != torch.float32 or not d.mask.is_contiguous()):
        raise ValueError("dropout: the explicit keep mask must be a contiguous fp32 tensor of x's shape")
    return _DropoutFn.apply(x, d)


def dropout_keep_mask(shape, d: DropSpec, device) -> torch.Tensor:
    """The keep mask (1 / 0) the hash of `d` stands for at the CURRENT value of the step counter."""
    out = torch.empty(*shape, dtype=torch.float32, device=device)
    _lib_().recalgo_dropout_keep_mask(out.numel(), d.rate, d.seed, d.call, _p(d.step), _p(out), _stream(out))
    return out


# =============================================================================================
# a15: TF1 Adam
# =============================================================================================
def adam_tf1_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int,
              lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
              zero_grad: bool = True, lr_t_dev: Optional[torch.Tensor] = None) -> None:
    """In-place dense TF1 Adam over flat fp32 buffers (step is 1-based).  With `lr_t_dev`
    (a 1-element device tensor maintained by adam_tf1_advance_) the launch is hipGraph
    replayable."""
    import math
    import struct
    # TF keeps lr/beta1/beta2 as float32 scalars: round them first (1 - f32(0.999) != 0.001)
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]
    lr_, b1_, b2_ = f32(lr), f32(beta1), f32(beta2)
    lr_t = 0.0 if lr_t_dev is not None else \
        lr_ * math.sqrt(1.0 - b2_ ** step) / (1.0 - b1_ ** step)
    _lib_().recalgo_adam_tf1_dense(_p(p), _p(g), _p(m), _p(v), p.numel(), lr_t, _p(lr_t_dev), beta1, beta2, eps, int(zero_grad),
                                   _stream(p))


def adam_tf1_rows_(weight: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                   row_live: torch.Tensor, lr_t_dev: torch.Tensor, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, zero_grad: bool = True) -> None:
    """TF1 dense Adam over an embedding arena [rows, K] that skips rows no batch has touched yet
    (exactly the identity for them); row_live [rows] uint8 is maintained by the kernel."""
    rows, K = weight.shape
    _lib_().recalgo_adam_tf1_rows(_p(weight), _p(grad), _p(m), _p(v), _p(row_live), rows, K, 0.0, _p(lr_t_dev), beta1, beta2, eps,
                                  int(zero_grad), _stream(weight))


def adam_tf1_list_(arena, lr_t_dev: torch.Tensor, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                   zero_grad: bool = True) -> None:
    """TF1 dense Adam applied to the arena's live rows only (identity elsewhere: bit-identical to
    the dense pass)."""
    _, lst, cnt = arena.live_state()
    rows, K = arena.weight.shape
    _lib_().recalgo_adam_tf1_list(_p(arena.weight), _p(arena.grad), _p(arena.m), _p(arena.v), _p(lst), _p(cnt), rows, K, 0.0,
                                  _p(lr_t_dev), beta1, beta2, eps, int(zero_grad), _stream(arena.weight))


def adam_tf1_advance_(step_dev: torch.Tensor, lr_t_dev: torch.Tensor, lr: float,
                      beta1: float = 0.9, beta2: float = 0.999) -> None:
    """step_dev (int64[1]) += 1; lr_t_dev (float[1]) = lr*sqrt(1-b2^t)/(1-b1^t), on device."""
    _lib_().recalgo_adam_tf1_advance(_p(step_dev), lr, beta1, beta2, _p(lr_t_dev), _stream(step_dev))


def adam_tf1_step_(flat, flat_grad, flat_m, flat_v, arenas, step_dev: torch.Tensor, ticket_dev: Optional[torch.Tensor],
                   lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, zero_grad: bool = True,
                   advance: bool = False, lazy: bool = False, plan_scans=()) -> None:
    """ONE launch: TF1 Adam over the flat dense buffer and over the live rows of every arena, lr_t derived on the device
    from step_dev (already advanced unless `advance`; include/recalgo.h recalgo_adam_tf1_step).  plan_scans: the
    recalgo_plan_scan_t records (sparse.plan_scan_record) of the scatter plans whose `apply` follows — their bucket-total
    prefix scans ride on this launch (recalgo_adam_tf1_step_plans)."""
    lib = _lib_()
    n = 0 if flat is None else flat.numel()
    for i in range(0, max(len(arenas), 1), 4):
        chunk = arenas[i:i + 4]
        arr = (_AdamArena * max(len(chunk), 1))()
        for j, a in enumerate(chunk):
            _, lst, cnt = a.live_state()
            rows, K = a.weight.shape
            arr[j] = _AdamArena(a.weight.data_ptr(), a.grad.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), lst.data_ptr(),
                                cnt.data_ptr(), rows, K, int(lazy))
        first = i == 0
        if not first:
            raise NotImplementedError("more than 4 embedding arenas in one model")
        scans = None
        if plan_scans:
            scans = (type(plan_scans[0]) * len(plan_scans))(*plan_scans)
        lib.recalgo_adam_tf1_step_plans(_p(flat) if n else None, _p(flat_grad) if n else None, _p(flat_m) if n else None,
                                        _p(flat_v) if n else None, n, arr, len(chunk), _p(step_dev), _p(ticket_dev), int(advance),
                                        lr, beta1, beta2, eps, int(zero_grad), scans, len(plan_scans), _stream(step_dev))


# The step's deferred sums inside the optimizer launch (recalgo_adam_tf1_sum_step): off -> the two launches, always
sum_step_enabled = True
sum_step_stats = {"fused": 0, "refused": 0}       # optimizer steps that ran as the one launch / that the entry refused


def sum_step_ticket_ints() -> int:
    """Length of the zeroed int32 tensor the launch keeps its arrival ticket in (adam_tf1_sum_step_'s ticket_dev)."""
    return int(_lib_().recalgo_adam_tf1_sum_step_workspace_bytes()) // 4


def adam_tf1_sum_step_(flat, flat_grad, flat_m, flat_v, arenas, step_dev: torch.Tensor, ticket_dev: torch.Tensor, lr: float,
                       beta1: float, beta2: float, eps: float, dense, colsums, lazy: bool = False, plan_scans=()) -> bool:
    """flush_dense_splits(step_dev) + adam_tf1_step_(.., zero_grad=True) as ONE launch (include/recalgo_sumstep.h
    recalgo_adam_tf1_sum_step), bit-identical to the two.  dense, colsums: take_dense_splits().  -> False, nothing launched,
    where the entry cannot serve the jobs (the caller runs the two launches)."""
    lib = _lib_()
    n = 0 if flat is None else flat.numel()
    if len(arenas) > 4:
        return False
    g0 = flat_grad.data_ptr() if n else 0
    g1 = g0 + 4 * n
    # a column sum whose output is no part of the flat gradient buffer (the loss value) is only summed
    side = [c for c in colsums if c[5].data_ptr() + 4 * c[4] <= g0 or c[5].data_ptr() >= g1]
    grads = [c for c in colsums if not any(c is e for e in side)]
    jobs, sums = _split_job_arrays(dense, grads)
    _, side_sums = _split_job_arrays((), side)
    gp = _p(flat_grad) if n else None
    if not lib.recalgo_adam_tf1_sum_step_supported(gp, n, jobs, len(dense), sums, len(grads), side_sums, len(side)):
        sum_step_stats["refused"] += 1
        return False
    arr = (_AdamArena * max(len(arenas), 1))()
    for j, a in enumerate(arenas):
        _, lst, cnt = a.live_state()
        rows, K = a.weight.shape
        arr[j] = _AdamArena(a.weight.data_ptr(), a.grad.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), lst.data_ptr(),
                            cnt.data_ptr(), rows, K, int(lazy))
    scans = (type(plan_scans[0]) * len(plan_scans))(*plan_scans) if plan_scans else None
    lib.recalgo_adam_tf1_sum_step(_p(flat) if n else None, gp, _p(flat_m) if n else None, _p(flat_v) if n else None, n, arr,
                                  len(arenas), _p(step_dev), _p(ticket_dev), 1, lr, beta1, beta2, eps, 1, scans, len(plan_scans),
                                  jobs, len(dense), sums, len(grads), side_sums, len(side), _stream(step_dev))
    sum_step_stats["fused"] += 1
    return True


# =============================================================================================
# BST (csrc/bst.hip, include/recalgo_bst.h): the transformer block — attention + LayerNorm, FFN + LayerNorm (+ pooling)
# =============================================================================================
_CB = _lib.HEADERS["recalgo_bst.h"].constants                 # the RECALGO_BST_* #defines of include/recalgo_bst.h
BST_MAX_T, BST_MAX_D, BST_MAX_HEADS = _CB["RECALGO_BST_MAX_T"], _CB["RECALGO_BST_MAX_D"], _CB["RECALGO_BST_MAX_HEADS"]
_bst_shared = {}             # id(Variable) -> how many blocks of the running step read it (position_embedding: every block
#                              adds it again); the block whose backward runs first overwrites its gradient, the others add


def bst_supported(T: int, d: int, H: int) -> bool:
    return bool(_lib_().recalgo_bst_supported(int(T), int(d), int(H)))


class _BstAttnFn(Function):
    """include/recalgo_bst.h recalgo_bst_attn_fwd / recalgo_bst_attn_bwd; params = (pos, w_q, w_k, w_v, w_o, gamma, beta) ("Parameters
    of a fused layer" above).  `pos` alone is not written by the kernel: its gradient is the table's first T rows."""

    @staticmethod
    def forward(ctx, anchor, x, keys_length, heads, differentiated, params, *tensors):
        ts, vs = _split_params(params)
        B, T, d = x.shape
        n1 = torch.empty(B, T, d, device=x.device, dtype=torch.float32)
        _lib_().recalgo_bst_attn_fwd(_p(x), *[_p(t) for t in ts[:1]], _p(keys_length), *[_p(t) for t in ts[1:]], B, T, d, heads,
                                     _p(n1), None, _stream(x))
        ctx.ts, ctx.vs, ctx.heads, ctx.order = ts, vs, heads, 0
        if vs[0] is not None and differentiated:         # (the caller's grad mode: inside a Function's forward it is always off)
            ctx.order = _bst_shared[id(vs[0])] = _bst_shared.get(id(vs[0]), 0) + 1
        ctx.save_for_backward(x, keys_length)
        return n1

    @staticmethod
    def backward(ctx, g):
        ts, vs, H = ctx.ts, ctx.vs, ctx.heads
        x, keys_length = ctx.saved_tensors
        B, T, d = x.shape
        g = _contig(g)
        lib = _lib_()
        dx = torch.empty_like(x)
        dpos = torch.empty(T, d, device=x.device, dtype=torch.float32)
        outs = _grad_buffers(ts[1:], vs[1:])             # dw_q, dw_k, dw_v, dw_o, dgamma, dbeta
        ws = _workspace(int(lib.recalgo_bst_attn_bwd_workspace_bytes(B, T, d, H)), x.device)
        lib.recalgo_bst_attn_bwd(_p(x), _p(ts[0]), _p(keys_length), *[_p(t) for t in ts[1:6]], _p(g), B, T, d, H, _p(dx), _p(dpos),
                                 *[_p(o) for o in outs], _p(ws), _stream(x))
        pos_v = vs[0]
        if pos_v is not None:
            # the table is [max_length, d], the kernel's gradient its first T rows; shared by every block of the model
            first = ctx.order == _bst_shared.get(id(pos_v), ctx.order)
            if first:
                pos_v.grad.zero_()
                pos_v.grad[:T].copy_(dpos)
            else:
                pos_v.grad[:T].add_(dpos)
            if ctx.order <= 1:
                _bst_shared.pop(id(pos_v), None)
            dpos_ret = None
        else:
            dpos_ret = torch.zeros_like(ts[0])
            dpos_ret[:T].copy_(dpos)
        return _param_returns(ctx, {1: dx}, [dpos_ret] + outs, vs)


class _BstFfnFn(Function):
    """include/recalgo_bst.h recalgo_bst_ffn_fwd / recalgo_bst_ffn_bwd; params = (ffn_w, ffn_b, gamma, beta) ("Parameters of a
    fused layer" above).  -> (out | None, pool | None)."""

    @staticmethod
    def forward(ctx, anchor, n1, mean_pool, want_out, want_pool, params, *tensors):
        ctx.set_materialize_grads(False)
        ts, vs = _split_params(params)
        B, T, d = n1.shape
        out = torch.empty(B, T, d, device=n1.device, dtype=torch.float32) if want_out else None
        pool = torch.empty(B, d, device=n1.device, dtype=torch.float32) if want_pool else None
        _lib_().recalgo_bst_ffn_fwd(_p(n1), *[_p(t) for t in ts], B, T, d, int(mean_pool), _p(out), _p(pool), None, _stream(n1))
        ctx.ts, ctx.vs, ctx.mean_pool = ts, vs, int(mean_pool)
        ctx.save_for_backward(n1)
        return out, pool

    @staticmethod
    def backward(ctx, g_out, g_pool):
        ts, vs = ctx.ts, ctx.vs
        (n1,) = ctx.saved_tensors
        if g_out is None and g_pool is None:
            return (None,) * len(ctx.needs_input_grad)
        B, T, d = n1.shape
        g_out, g_pool = _contig(g_out), _contig(g_pool)
        lib = _lib_()
        dn1 = torch.empty_like(n1)
        outs = _grad_buffers(ts, vs)                     # dw, db, dgamma, dbeta
        ws = _workspace(int(lib.recalgo_bst_ffn_bwd_workspace_bytes(B, d)), n1.device)
        lib.recalgo_bst_ffn_bwd(_p(n1), *[_p(t) for t in ts[:3]], _p(g_out), _p(g_pool), B, T, d, ctx.mean_pool, _p(dn1),
                                *[_p(o) for o in outs], _p(ws), _stream(n1))
        return _param_returns(ctx, {1: dn1}, outs, vs)


def _bst_check(x, T, d, H, ts, shapes, what):
    if not bst_supported(T, d, H):
        raise ValueError(f"{what}: the BST kernels serve 1 <= T <= {BST_MAX_T}, d in (4, 8, 12, 16) and 1 <= heads <= "
                         f"{BST_MAX_HEADS}; got T={T} d={d} heads={H} (there is no fallback)")
    if x.shape[0] == 0:
        raise ValueError(f"{what}: empty batch")
    names = ("pos", "w_q", "w_k", "w_v", "w_o", "gamma", "beta") if len(shapes) == 7 else ("ffn_w", "ffn_b", "gamma", "beta")
    if names[0] == "pos" and ts[0].dim() == 2 and ts[0].shape[0] >= T and ts[0].shape[1] == d:
        shapes = [tuple(ts[0].shape)] + shapes[1:]       # (the table may be longer than T: its first T rows are read)
    _check_param_shapes(what, ts, shapes, names, chk=True)


def bst_attention(x: torch.Tensor, keys_length: torch.Tensor, pos, w_q, w_k, w_v, w_o, gamma, beta, anchor=None) -> torch.Tensor:
    """The attention half of a BST block (transformer_layer.py:27-72): LayerNorm(concat_h(softmax(Q_h K_h^T / sqrt(d) + mask)
    V_h) w_o + Xp) with Xp = x + pos[:T], Q and K from Xp, V from x; the mask is on the QUERY rows >= keys_length.
    x [B, T, d]; keys_length integer [B]; pos [>= T, d]; w_q / w_k / w_v [H, d, d]; w_o [H d, d]; gamma, beta [d] — Variables
    (gradient to Variable.grad; a `pos` Variable shared by several blocks gets their sum) or tensors.  Unsupported sizes:
    ValueError, there is no fallback."""
    if x.dim() != 3:
        raise ValueError("bst_attention: x must be [B, T, d]")
    B, T, d = x.shape
    params = [pos, w_q, w_k, w_v, w_o, gamma, beta]
    ts, _ = _split_params(params)
    H = int(ts[1].shape[0]) if ts[1].dim() == 3 else 0
    _bst_check(x, T, d, H, ts, [(T, d), (H, d, d), (H, d, d), (H, d, d), (H * d, d), (d,), (d,)], "bst_attention")
    _chk(x, torch.float32, "bst_attention: x")
    keys_length = keys_length.reshape(-1).to(torch.int32).contiguous()
    if keys_length.numel() != B:
        raise ValueError("bst_attention: one keys_length per example")
    return _BstAttnFn.apply(anchor, x, keys_length, H, torch.is_grad_enabled(), params, *_param_tail(params))


def bst_ffn(n1: torch.Tensor, ffn_w, ffn_b, gamma, beta, pool: Optional[str] = None, want_out: bool = True, anchor=None):
    """The FFN half of a BST block (transformer_layer.py:74-81): out = LayerNorm(leakyrelu(n1 W + b) + n1) -> (out, pooled):
    pooled = out summed (pool="sum") or averaged (pool="mean") over ALL T rows, None without `pool`; out is None with
    want_out=False."""
    if n1.dim() != 3 or pool not in (None, "sum", "mean") or not (want_out or pool):
        raise ValueError("bst_ffn: n1 must be [B, T, d], pool one of None, 'sum', 'mean', and some output wanted")
    B, T, d = n1.shape
    params = [ffn_w, ffn_b, gamma, beta]
    _bst_check(n1, T, d, 1, _split_params(params)[0], [(d, d), (d,), (d,), (d,)], "bst_ffn")
    _chk(n1, torch.float32, "bst_ffn: n1")
    return _BstFfnFn.apply(anchor, n1, pool == "mean", bool(want_out), pool is not None, params, *_param_tail(params))


# =============================================================================================
# DeepCrossing (csrc/residual.hip, include/recalgo_res.h): the stack of residual units, one kernel each way
# =============================================================================================
_CR = _lib.HEADERS["recalgo_res.h"].constants                 # the RECALGO_RES_* #defines of include/recalgo_res.h
RES_MAX_D, RES_MAX_H, RES_MAX_UNITS = _CR["RECALGO_RES_MAX_D"], _CR["RECALGO_RES_MAX_H"], _CR["RECALGO_RES_MAX_UNITS"]


def residual_supported(D: int, H: int, L: int) -> bool:
    return bool(_lib_().recalgo_res_supported(int(D), int(H), int(L)))


class _ResidualStackFn(Function):
    """include/recalgo_res.h recalgo_res_stack_fwd / recalgo_res_stack_bwd; the four parameter gradients of a unit are batch
    sums over what the backward kernel wrote: two launches of the dense engine's weight gradient per unit."""

    @staticmethod
    def forward(ctx, anchor, x, w0s, b0s, w1s, b1s, differentiated):
        B, D = x.shape
        L, H = len(w0s), int(w0s[0].data.shape[1])
        tables = [_ptr_array([v.data for v in vs]) for vs in (w0s, b0s, w1s, b1s)]
        save = bool(differentiated)          # (the caller's grad mode: inside a Function's forward it is always off)
        hs = torch.empty(L, B, H, device=x.device, dtype=torch.float32) if save else None
        ys = torch.empty((L, B, D) if save else (B, D), device=x.device, dtype=torch.float32)
        _lib_().recalgo_res_stack_fwd(_p(x), *tables, B, D, H, L, int(save), _p(hs), _p(ys), _stream(x))
        if not save:
            return ys
        ctx.vars = (w0s, b0s, w1s, b1s)
        ctx.in_step = _loss_seed is not None      # built inside Estimator.train_step: its optimizer runs the deferred sums
        ctx.save_for_backward(x, hs, ys)
        return ys[L - 1]

    @staticmethod
    def backward(ctx, g):
        w0s, b0s, w1s, b1s = ctx.vars
        x, hs, ys = ctx.saved_tensors
        L, B, D = ys.shape
        H = hs.shape[2]
        g = _contig(g)
        dzs, dhs, dx = torch.empty_like(ys), torch.empty_like(hs), torch.empty_like(x)
        _lib_().recalgo_res_stack_bwd(_p(g), _p(hs), _p(ys), _ptr_array([v.data for v in w0s]), _ptr_array([v.data for v in w1s]),
                                      B, D, H, L, _p(dzs), _p(dhs), _p(dx), _stream(x))
        for l in range(L):
            dense_bwd_weights(x if l == 0 else ys[l - 1], dhs[l], None, w0s[l].grad, b0s[l].grad, defer=ctx.in_step)
            dense_bwd_weights(hs[l], dzs[l], None, w1s[l].grad, b1s[l].grad, defer=ctx.in_step)
        return (None, dx if ctx.needs_input_grad[1] else None, None, None, None, None, None)


def residual_stack(x: torch.Tensor, w0s, b0s, w1s, b1s, anchor=None) -> torch.Tensor:
    """DeepCrossing's residual units (residual_unit.py:4-22) chained: x_{l+1} = relu(x_l + relu(x_l W0_l + b0_l) W1_l + b1_l)
    for the L units of the four lists of Variables (W0_l [D, H], b0_l [H], W1_l [H, D], b1_l [D]); x [B, D] -> [B, D].
    With grad enabled the forward keeps every unit's two activations and the backward is one launch plus two weight-gradient
    launches per unit (gradients to Variable.grad; inside a training step their sums join the step's deferred reduction,
    flush_dense_splits).  Sizes the kernels do not serve (residual_supported): ValueError — nn.residual_stack composes those
    from dense layers."""
    if x.dim() != 2 or x.shape[0] == 0:
        raise ValueError("residual_stack: x must be a non-empty [B, D] matrix")
    _chk(x, torch.float32, "residual_stack: x")
    B, D = x.shape
    L = len(w0s)
    H = int(w0s[0].data.shape[1]) if L and w0s[0].data.dim() == 2 else 0
    if not (len(b0s) == len(w1s) == len(b1s) == L) or not residual_supported(D, H, L):
        raise ValueError(f"residual_stack: the kernels serve 1 <= D <= {RES_MAX_D}, 16 <= H <= {RES_MAX_H} with H % 16 == 0 and "
                         f"1 <= units <= {RES_MAX_UNITS}; got D={D} H={H} units={L}")
    for vs, shape, name in ((w0s, (D, H), "W0"), (b0s, (H,), "b0"), (w1s, (H, D), "W1"), (b1s, (D,), "b1")):
        for v in vs:
            _chk(v.data, torch.float32, f"residual_stack: {name}")
            if tuple(v.data.shape) != shape:
                raise ValueError(f"residual_stack: {name} has shape {tuple(v.data.shape)}, expected {shape}")
    return _ResidualStackFn.apply(anchor, x, tuple(w0s), tuple(b0s), tuple(w1s), tuple(b1s), torch.is_grad_enabled())


# =============================================================================================
# AFM (csrc/afm.hip, include/recalgo_afm.h): the attention network over the pair products, one kernel each way
# =============================================================================================
def afm_supported(F: int, K: int, t: int) -> bool:
    return bool(_lib_().recalgo_afm_supported(int(F), int(K), int(t)))


class _AfmAttentionFn(Function):
    """include/recalgo_afm.h recalgo_afm_attention_fwd / recalgo_afm_attention_bwd; params = (w, b, h) ("Parameters of a fused
    layer" above).  Saved: the fields and the pre-softmax scores [B, P]."""

    @staticmethod
    def forward(ctx, anchor, fields, F, K, differentiated, params, *tensors):
        ts, vs = _split_params(params)
        B, t = fields.shape[0], int(ts[0].shape[1])
        out = torch.empty(B, K, device=fields.device, dtype=torch.float32)
        # (the caller's grad mode: inside a Function's forward it is always off; PREDICT / EVAL keep no scores)
        scores = torch.empty(B, F * (F - 1) // 2, device=fields.device, dtype=torch.float32) if differentiated else None
        _lib_().recalgo_afm_attention_fwd(_p(fields), *[_p(x) for x in ts], B, F, K, t, _p(out), _p(scores), _stream(fields))
        if differentiated:
            ctx.ts, ctx.vs, ctx.F, ctx.K = ts, vs, F, K
            ctx.save_for_backward(fields, scores)
        return out

    @staticmethod
    def backward(ctx, g):
        ts, vs, F, K = ctx.ts, ctx.vs, ctx.F, ctx.K
        fields, scores = ctx.saved_tensors
        B, t = fields.shape[0], int(ts[0].shape[1])
        g = _contig(g)
        lib = _lib_()
        d_fields = torch.empty_like(fields)
        outs = _grad_buffers(ts, vs)                     # dw, db, dh
        ws = _workspace(int(lib.recalgo_afm_bwd_workspace_bytes(B, F, K, t)), fields.device)
        lib.recalgo_afm_attention_bwd(_p(g), _p(fields), *[_p(x) for x in ts], _p(scores), B, F, K, t, _p(d_fields),
                                      *[_p(o) for o in outs], _p(ws), _stream(fields))
        return _param_returns(ctx, {1: d_fields}, outs, vs)


def afm_attention(fields: torch.Tensor, F: int, K: int, w, b, h, anchor=None) -> torch.Tensor:
    """AFM's attention network (afm.py:162-188) as one launch each way: fields [B, F * K] (contiguous fp32 on the device) ->
    sum_p softmax_p(relu(pair_p @ w + b) @ h) * pair_p over the pairs p = (i < j) of the F field rows, [B, K].  w [K, t],
    b [t], h [t, 1] or [t] — Variables (gradient to Variable.grad, overwritten) or tensors.  With grad enabled the forward
    keeps the fields and the [B, P] scores; the backward is one launch and the fixed-order sum of its partial rows.  Shapes
    the kernels do not serve (afm_supported): ValueError, there is no fallback here (nn.afm_attention owns the composed chain)."""
    F, K = int(F), int(K)
    params = [w, b, h]
    ts, _ = _split_params(params)
    t = int(ts[0].shape[1]) if ts[0].dim() == 2 else 0
    if not afm_supported(F, K, t):
        raise ValueError(f"afm_attention: the kernels serve 2 <= F <= 64, K % 4 == 0 with 4 <= K <= 32 and t % 16 == 0 with "
                         f"16 <= t <= 256; got F={F} K={K} t={t} (there is no fallback)")
    if fields.dim() != 2 or fields.shape[0] == 0 or fields.shape[1] != F * K:
        raise ValueError(f"afm_attention: fields must be a non-empty [B, F * K = {F * K}] matrix, got {tuple(fields.shape)}")
    _chk(fields, torch.float32, "afm_attention: fields")
    for x, n, name in zip(ts, (K * t, t, t), ("w", "b", "h")):
        _chk(x, torch.float32, f"afm_attention: {name}")
        if x.numel() != n or (name == "w" and tuple(x.shape) != (K, t)):
            raise ValueError(f"afm_attention: {name} has shape {tuple(x.shape)}")
    return _AfmAttentionFn.apply(anchor, fields, F, K, torch.is_grad_enabled(), params, *_param_tail(params))


# =============================================================================================
# AutoInt (csrc/autoint.hip, include/recalgo_autoint.h): one interacting layer — multi-head self-attention over the fields
# =============================================================================================
_CAI = _lib.SERVING_HEADERS["recalgo_autoint.h"].constants    # the RECALGO_AUTOINT_* #defines of include/recalgo_autoint.h


def autoint_supported(F: int, D: int, A: int, H: int) -> bool:
    return bool(_lib_().recalgo_autoint_supported(int(F), int(D), int(A), int(H)))


class _AutoIntLayerFn(Function):
    """include/recalgo_autoint.h recalgo_autoint_layer_fwd / recalgo_autoint_layer_bwd; params = (wq, wk, wv, wres | None)
    ("Parameters of a fused layer" above).  Saved: x and y (the backward recomputes everything between them)."""

    @staticmethod
    def forward(ctx, anchor, x, F, differentiated, params, *tensors):
        ts, vs = _split_params(params)
        B, (H, D, A) = x.shape[0], ts[0].shape
        y = torch.empty(B, F * H * A, device=x.device, dtype=torch.float32)
        _lib_().recalgo_autoint_layer_fwd(_p(x), *[_p(t) for t in ts], B, F, D, A, H, _p(y), _stream(x))
        if differentiated:               # (the caller's grad mode: inside a Function's forward it is always off)
            ctx.ts, ctx.vs, ctx.F = ts, vs, F
            ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, g):
        ts, vs, F = ctx.ts, ctx.vs, ctx.F
        x, y = ctx.saved_tensors
        B, (H, D, A) = x.shape[0], ts[0].shape
        g = _contig(g)
        lib = _lib_()
        dx = torch.empty_like(x)
        outs = _grad_buffers(ts, vs)                     # dwq, dwk, dwv, dwres | None
        ws = _workspace(int(lib.recalgo_autoint_bwd_workspace_bytes(B, F, D, A, H, int(ts[3] is not None))), x.device)
        lib.recalgo_autoint_layer_bwd(_p(g), _p(x), _p(y), *[_p(t) for t in ts], B, F, D, A, H, _p(dx), *[_p(o) for o in outs],
                                      _p(ws), _stream(x))
        return _param_returns(ctx, {1: dx}, outs, vs)


def autoint_layer(x: torch.Tensor, F: int, wq, wk, wv, wres=None, anchor=None) -> torch.Tensor:
    """One AutoInt interacting layer (include/recalgo_autoint.h) as one launch each way: x [B, F * D] (contiguous fp32 on the
    device), wq, wk, wv [H, D, A] and the optional residual projection wres [D, H * A] -> relu(concat_h softmax(Q_h K_h^T) V_h
    + x Wres), [B, F * H * A] with head-major columns.  Each parameter is a Variable (gradient to Variable.grad, overwritten) or
    a tensor.  With grad enabled the forward keeps x and y, nothing else; the backward is one launch and the fixed-order sum of
    its partial rows.  Shapes the kernels do not serve (autoint_supported): ValueError — there is no fallback."""
    F = int(F)
    params = [wq, wk, wv, wres]
    ts, _ = _split_params(params)
    if ts[0].dim() != 3:
        raise ValueError(f"autoint_layer: wq must be [H, D, A], got {tuple(ts[0].shape)}")
    H, D, A = (int(v) for v in ts[0].shape)
    if not autoint_supported(F, D, A, H):
        raise ValueError(f"autoint_layer: the kernels serve {_CAI['RECALGO_AUTOINT_MIN_F']} <= F <= {_CAI['RECALGO_AUTOINT_MAX_F']}, "
                         f"D % 4 == 0 with {_CAI['RECALGO_AUTOINT_MIN_D']} <= D <= {_CAI['RECALGO_AUTOINT_MAX_D']}, A % 4 == 0 with "
                         f"{_CAI['RECALGO_AUTOINT_MIN_A']} <= A <= {_CAI['RECALGO_AUTOINT_MAX_A']} and 1 <= H <= "
                         f"{_CAI['RECALGO_AUTOINT_MAX_H']} with H * A <= {_CAI['RECALGO_AUTOINT_MAX_HA']}; got F={F} D={D} A={A} H={H} "
                         f"(there is no fallback)")
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] != F * D:
        raise ValueError(f"autoint_layer: x must be a non-empty [B, F * D = {F * D}] matrix, got {tuple(x.shape)}")
    names = ("wq", "wk", "wv", "wres")
    _check_param_shapes("autoint_layer", ts, ((H, D, A), (H, D, A), (H, D, A), (D, H * A)), names)
    _check_fp32_on_device("autoint_layer", [x] + ts, ("x",) + names)
    return _AutoIntLayerFn.apply(anchor, x, F, torch.is_grad_enabled(), params, *_param_tail(params))


# =============================================================================================
# DCN-V2 (csrc/dcnv2.hip, include/recalgo_dcnv2.h): one cross layer — the mixture of low-rank experts with a softmax gate
# =============================================================================================
_CDX = _lib.SERVING_HEADERS["recalgo_dcnv2.h"].constants      # the RECALGO_DCNV2_* #defines of include/recalgo_dcnv2.h


def dcnv2_supported(D: int, r: int, E: int) -> bool:
    return bool(_lib_().recalgo_dcnv2_supported(int(D), int(r), int(E)))


class _Dcnv2LayerFn(Function):
    """include/recalgo_dcnv2.h recalgo_dcnv2_layer_fwd / recalgo_dcnv2_layer_bwd; params = (V, C, U, gate | None, bias) ("Parameters
    of a fused layer" above).  Saved: x0 and xl (the backward recomputes everything from them).  `same`: xl IS x0 (a stack's
    first layer) — x0 is passed once and receives dx0 + dxl."""

    @staticmethod
    def forward(ctx, anchor, x0, xl, differentiated, params, *tensors):
        same = xl is None
        xl = x0 if same else xl
        ts, vs = _split_params(params)
        B, (E, D, r) = x0.shape[0], ts[0].shape
        y = torch.empty_like(x0)
        _lib_().recalgo_dcnv2_layer_fwd(_p(x0), _p(xl), *[_p(t) for t in ts], B, D, r, E, _p(y), _stream(x0))
        if differentiated:               # (the caller's grad mode: inside a Function's forward it is always off)
            ctx.ts, ctx.vs, ctx.same = ts, vs, same
            ctx.save_for_backward(x0, xl)
        return y

    @staticmethod
    def backward(ctx, g):
        ts, vs, same = ctx.ts, ctx.vs, ctx.same
        x0, xl = ctx.saved_tensors
        B, (E, D, r) = x0.shape[0], ts[0].shape
        g = _contig(g)
        lib = _lib_()
        dx0, dxl = torch.empty_like(x0), torch.empty_like(xl)
        outs = _grad_buffers(ts, vs)                     # dV, dC, dU, dgate | None, dbias
        ws = _workspace(int(lib.recalgo_dcnv2_bwd_workspace_bytes(B, D, r, E)), x0.device)
        lib.recalgo_dcnv2_layer_bwd(_p(g), _p(x0), _p(xl), *[_p(t) for t in ts], B, D, r, E, _p(dx0), _p(dxl),
                                    *[_p(o) for o in outs], _p(ws), _stream(x0))
        if same:
            return _param_returns(ctx, {1: dx0.add_(dxl)} if ctx.needs_input_grad[1] else {}, outs, vs)
        return _param_returns(ctx, {1: dx0, 2: dxl}, outs, vs)


def dcnv2_layer(x0: torch.Tensor, xl: torch.Tensor, V, C, U, gate, bias, anchor=None) -> torch.Tensor:
    """One DCN-V2 cross layer (include/recalgo_dcnv2.h), the mixture of E low-rank experts, as one entry each way: x0, xl
    [B, D] (contiguous fp32 on the device; xl may BE x0, a stack's first layer), V, U [E, D, r], C [E, r, r], gate [E, D] (None
    with E == 1: the plain low-rank layer) and bias [D] -> x0 * sum_e p_e (tanh(tanh(xl V_e) C_e) U_e^T + bias) + xl with
    p = softmax(xl gate^T).  Each parameter is a Variable (gradient to Variable.grad, overwritten) or a tensor.  With grad enabled
    the forward keeps x0 and xl, nothing else; the backward recomputes from them and sums its partial rows in fixed order.
    Shapes the kernels do not serve (dcnv2_supported): ValueError — the composed layer is nn.cross_mix_layer(fused=False)."""
    params = [V, C, U, gate, bias]
    ts, _ = _split_params(params)
    if ts[0].dim() != 3:
        raise ValueError(f"dcnv2_layer: V must be [E, D, r], got {tuple(ts[0].shape)}")
    E, D, r = (int(v) for v in ts[0].shape)
    if not dcnv2_supported(D, r, E):
        raise ValueError(f"dcnv2_layer: the kernels serve {_CDX['RECALGO_DCNV2_MIN_D']} <= D <= {_CDX['RECALGO_DCNV2_MAX_D']}, "
                         f"r % 4 == 0 with {_CDX['RECALGO_DCNV2_MIN_R']} <= r <= {_CDX['RECALGO_DCNV2_MAX_R']} and 1 <= E <= "
                         f"{_CDX['RECALGO_DCNV2_MAX_E']}; got D={D} r={r} E={E} (nn.cross_mix_layer(fused=False) is the composed layer)")
    if gate is None and E != 1:
        raise ValueError(f"dcnv2_layer: only a single expert runs without a gate, got E={E}")
    if x0.dim() != 2 or x0.shape[0] == 0 or x0.shape[1] != D or tuple(xl.shape) != tuple(x0.shape):
        raise ValueError(f"dcnv2_layer: x0 and xl must be non-empty [B, D = {D}] matrices, got {tuple(x0.shape)} and {tuple(xl.shape)}")
    names = ("V", "C", "U", "gate", "bias")
    _check_param_shapes("dcnv2_layer", ts, ((E, D, r), (E, r, r), (E, D, r), (E, D), (D,)), names)
    _check_fp32_on_device("dcnv2_layer", [x0, xl] + ts, ("x0", "xl") + names)
    return _Dcnv2LayerFn.apply(anchor, x0, None if xl is x0 else xl, torch.is_grad_enabled(), params, *_param_tail(params))


# =============================================================================================
# FLEN (csrc/flen.hip, include/recalgo_flen.h): the field-wise bi-interaction with Dicefactor
# =============================================================================================
_CFL = _lib.SERVING_HEADERS["recalgo_flen.h"].constants       # the RECALGO_FLEN_* #defines of include/recalgo_flen.h


def flen_supported(F: int, M: int, K: int) -> bool:
    return bool(_lib_().recalgo_flen_supported(int(F), int(M), int(K)))


def _flen_groups(group_of):
    """-> the HOST int32 array the entries read at launch time"""
    return (ctypes.c_int32 * len(group_of))(*group_of)


class _FlenFn(Function):
    """include/recalgo_flen.h recalgo_flen_fwd / recalgo_flen_bwd; params = (r_mf, r_fm, bias) ("Parameters of a fused layer"
    above).  Saved: x alone (the backward recomputes e and q, and the Dicefactor mask from its key)."""

    @staticmethod
    def forward(ctx, anchor, x, F, group_of, dice, differentiated, params, *tensors):
        ts, vs = _split_params(params)
        B, M, K = x.shape[0], ts[1].shape[0], ts[2].shape[0]
        e = torch.empty(B, M * K, device=x.device, dtype=torch.float32)
        h = torch.empty(B, K, device=x.device, dtype=torch.float32)
        groups = _flen_groups(group_of)
        cd, keep = _cdrop(dice)
        _lib_().recalgo_flen_fwd(_p(x), ctypes.cast(groups, ctypes.c_void_p), _p(ts[0]), _p(ts[1]), _p(ts[2]), cd, B, F, M, K,
                                 _p(e), _p(h), _stream(x))
        del keep
        if differentiated:               # (the caller's grad mode: inside a Function's forward it is always off)
            ctx.ts, ctx.vs, ctx.F, ctx.group_of, ctx.dice = ts, vs, F, group_of, dice
            ctx.save_for_backward(x)
        return e, h

    @staticmethod
    def backward(ctx, g_e, g_h):         # (the gradient of an output nobody used arrives as zeros)
        ts, vs, F = ctx.ts, ctx.vs, ctx.F
        x, = ctx.saved_tensors
        B, M, K = x.shape[0], ts[1].shape[0], ts[2].shape[0]
        g_e, g_h = _contig(g_e), _contig(g_h)
        lib = _lib_()
        dx = torch.empty_like(x)
        outs = _grad_buffers(ts, vs)                     # dr_mf, dr_fm, dbias
        groups = _flen_groups(ctx.group_of)
        cd, keep = _cdrop(ctx.dice)
        ws = _workspace(int(lib.recalgo_flen_bwd_workspace_bytes(B, F, M, K)), x.device)
        lib.recalgo_flen_bwd(_p(g_e), _p(g_h), _p(x), ctypes.cast(groups, ctypes.c_void_p), _p(ts[0]), _p(ts[1]), cd, B, F, M, K,
                             _p(dx), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(ws), _stream(x))
        del keep
        return _param_returns(ctx, {1: dx}, outs, vs)


def flen_interaction(fields: torch.Tensor, F: int, group_of, r_mf, r_fm, bias, dice: Optional["DropSpec"] = None, anchor=None):
    """FLEN's field-wise bi-interaction (include/recalgo_flen.h) as one launch each way: fields [B, F * K] (contiguous fp32 on
    the device), group_of the F group indices in [0, M), r_mf [M (M - 1) / 2], r_fm [M] and bias [K] -> (e [B, M * K], the
    field-wise embeddings, h [B, K], the MF term across the groups plus the FM term inside each).  `dice`: the DropSpec of
    Dicefactor over the [B, P + M, K] path components (None: none).  Each parameter is a Variable (gradient to Variable.grad,
    overwritten) or a tensor.  With grad enabled the forward keeps `fields`, nothing else; the backward is one launch and the
    fixed-order sum of its partial rows.  Shapes the kernels do not serve (flen_supported), an empty group or a group index
    outside [0, M): ValueError — the composed arithmetic is nn.field_wise_bi_interaction(fused=False)."""
    F = int(F)
    group_of = tuple(int(g) for g in group_of)
    params = [r_mf, r_fm, bias]
    ts, _ = _split_params(params)
    if ts[1].dim() != 1 or ts[2].dim() != 1:
        raise ValueError(f"flen_interaction: r_fm must be [M] and bias [K], got {tuple(ts[1].shape)} and {tuple(ts[2].shape)}")
    M, K = int(ts[1].shape[0]), int(ts[2].shape[0])
    P = M * (M - 1) // 2
    if not flen_supported(F, M, K):
        raise ValueError(f"flen_interaction: the kernels serve {_CFL['RECALGO_FLEN_MIN_F']} <= F <= {_CFL['RECALGO_FLEN_MAX_F']}, "
                         f"{_CFL['RECALGO_FLEN_MIN_M']} <= M <= min(F, {_CFL['RECALGO_FLEN_MAX_M']}) and K % 4 == 0 with "
                         f"{_CFL['RECALGO_FLEN_MIN_K']} <= K <= {_CFL['RECALGO_FLEN_MAX_K']}; got F={F} M={M} K={K} "
                         f"(nn.field_wise_bi_interaction(fused=False) is the composed arithmetic)")
    if len(group_of) != F or set(group_of) != set(range(M)):
        raise ValueError(f"flen_interaction: group_of must map the F={F} fields onto every one of the M={M} groups, got {group_of}")
    if fields.dim() != 2 or fields.shape[0] == 0 or fields.shape[1] != F * K:
        raise ValueError(f"flen_interaction: fields must be a non-empty [B, F * K = {F * K}] matrix, got {tuple(fields.shape)}")
    names = ("r_mf", "r_fm", "bias")
    _check_param_shapes("flen_interaction", ts, ((P,), (M,), (K,)), names)
    _check_fp32_on_device("flen_interaction", [fields] + ts, ("fields",) + names)
    if dice is not None:
        if not 0.0 < dice.rate < 1.0:
            raise ValueError(f"flen_interaction: the Dicefactor rate must lie in (0, 1), got {dice.rate}")
        if fields.shape[0] * (P + M) * K >= 1 << 32:
            raise ValueError("flen_interaction: Dicefactor indexes B (P + M) K < 2^32 path components")
        dice.check_mask((fields.shape[0], P + M, K))
    return _FlenFn.apply(anchor, fields, F, group_of, dice, torch.is_grad_enabled(), params, *_param_tail(params))


class _VariableLeafFn(Function):
    """A Variable as a leaf of a chain composed from torch ops: forward gives its data, backward OVERWRITES Variable.grad (the
    convention of every parameter-owning op here; a variable is read once per step)."""

    @staticmethod
    def forward(ctx, anchor, var):
        ctx.var = var
        return var.data.view_as(var.data)

    @staticmethod
    def backward(ctx, g):
        ctx.var.grad.copy_(g)
        return None, None


def variable_leaf(var, anchor) -> torch.Tensor:
    return _VariableLeafFn.apply(anchor, var) if isinstance(var, Variable) else var


# =============================================================================================
# DIEN (csrc/dien.hip, include/recalgo_dien.h): the GRU recurrence; attention + the AGRU / AUGRU recurrence
# =============================================================================================
_CD = _lib.MORE_HEADERS["recalgo_dien.h"].constants           # the RECALGO_DIEN_* #defines of include/recalgo_dien.h
DIEN_MAX_T, DIEN_MAX_NA, DIEN_MAX_NH = _CD["RECALGO_DIEN_MAX_T"], _CD["RECALGO_DIEN_MAX_NA"], _CD["RECALGO_DIEN_MAX_NH"]
DIEN_MODES = {"AGRU": _CD["RECALGO_DIEN_MODE_AGRU"], "AUGRU": _CD["RECALGO_DIEN_MODE_AUGRU"]}


def dien_supported(T: int, na: int, nh: int) -> bool:
    return bool(_lib_().recalgo_dien_supported(int(T), int(na), int(nh)))


class _DienGruFn(Function):
    """include/recalgo_dien.h recalgo_dien_gru_fwd / recalgo_dien_gru_bwd; params = (Wg, bg, Wc, bc) ("Parameters of a fused
    layer" above)."""

    @staticmethod
    def forward(ctx, anchor, x, lengths, params, *tensors):
        ts, vs = _split_params(params)
        B, T, na = x.shape
        nh = ts[3].shape[0]
        h = torch.empty(B, T, nh, device=x.device, dtype=torch.float32)
        _lib_().recalgo_dien_gru_fwd(_p(x), _p(lengths), *[_p(t) for t in ts], B, T, na, nh, _p(h), _stream(x))
        ctx.ts, ctx.vs, ctx.lengths = ts, vs, lengths
        ctx.save_for_backward(x, h)
        return h

    @staticmethod
    def backward(ctx, g):
        ts, vs, lengths = ctx.ts, ctx.vs, ctx.lengths
        x, h = ctx.saved_tensors
        B, T, na = x.shape
        nh = h.shape[2]
        g = _contig(g)
        lib = _lib_()
        dx = torch.empty_like(x)
        outs = _grad_buffers(ts, vs)                     # dWg, dbg, dWc, dbc
        ws = _workspace(int(lib.recalgo_dien_gru_bwd_workspace_bytes(B, na, nh)), x.device)
        lib.recalgo_dien_gru_bwd(_p(x), _p(lengths), _p(h), *[_p(t) for t in ts], _p(g), B, T, na, nh, _p(dx),
                                 *[_p(o) for o in outs], _p(ws), _stream(x))
        return _param_returns(ctx, {1: dx}, outs, vs)


class _DienEvolveFn(Function):
    """include/recalgo_dien.h recalgo_dien_evolve_fwd / recalgo_dien_evolve_bwd; params = (w_att, Wg, bg, Wc, bc) ("Parameters of
    a fused layer" above).  -> (final, att, states); only `final` is differentiable."""

    @staticmethod
    def forward(ctx, anchor, h, target, lengths, mode, params, *tensors):
        ts, vs = _split_params(params)
        B, T, nh = h.shape
        na = target.shape[1]
        att = torch.empty(B, T, device=h.device, dtype=torch.float32)
        states = torch.empty(B, T, nh, device=h.device, dtype=torch.float32)
        final = torch.empty(B, nh, device=h.device, dtype=torch.float32)
        _lib_().recalgo_dien_evolve_fwd(_p(h), _p(target), _p(lengths), *[_p(t) for t in ts], B, T, na, nh, mode, _p(att),
                                        _p(states), _p(final), _stream(h))
        ctx.ts, ctx.vs, ctx.mode, ctx.lengths = ts, vs, mode, lengths
        ctx.save_for_backward(h, target, att, states)
        ctx.mark_non_differentiable(att, states)
        return final, att, states

    @staticmethod
    def backward(ctx, g_final, _g_att, _g_states):
        ts, vs, lengths = ctx.ts, ctx.vs, ctx.lengths
        h, target, att, states = ctx.saved_tensors
        B, T, nh = h.shape
        na = target.shape[1]
        g_final = _contig(g_final)
        lib = _lib_()
        dh, dtarget = torch.empty_like(h), torch.empty_like(target)
        outs = _grad_buffers(ts, vs)                     # dw_att, dWg, dbg, dWc, dbc
        ws = _workspace(int(lib.recalgo_dien_evolve_bwd_workspace_bytes(B, na, nh)), h.device)
        lib.recalgo_dien_evolve_bwd(_p(h), _p(target), _p(lengths), *[_p(t) for t in ts], _p(att), _p(states), _p(g_final), B, T,
                                    na, nh, ctx.mode, _p(dh), _p(dtarget), *[_p(o) for o in outs], _p(ws), _stream(h))
        return _param_returns(ctx, {1: dh, 2: dtarget}, outs, vs)


def _dien_check(what, B, T, na, nh, params, shapes, names):
    if not dien_supported(T, na, nh):
        raise ValueError(f"{what}: the DIEN kernels serve 1 <= T <= {DIEN_MAX_T}, an input width in (4, 8, 12, 16) up to "
                         f"{DIEN_MAX_NA} and a state width in (4, 8, 12, 16) up to {DIEN_MAX_NH}; got T={T} na={na} nh={nh} "
                         "(there is no fallback)")
    if B == 0:
        raise ValueError(f"{what}: empty batch")
    _check_param_shapes(what, _split_params(params)[0], shapes, names, chk=True)


def _dien_lengths(lengths, B, what):
    if lengths is None:
        return None
    lengths = lengths.reshape(-1).to(torch.int32).contiguous()
    if lengths.numel() != B:
        raise ValueError(f"{what}: one length per example")
    return lengths


def dien_gru(x: torch.Tensor, lengths: Optional[torch.Tensor], Wg, bg, Wc, bc, anchor=None) -> torch.Tensor:
    """dynamic_rnn over TF 1.14's GRUCell from a zero state (dien.py:196-203): x [B, T, na] -> h [B, T, nh]; with `lengths`
    (integer [B]) the rows t >= L of h are zero, without it all T steps run.  Wg [na + nh, 2 nh], bg [2 nh], Wc [na + nh, nh],
    bc [nh]: Variables (gradient to Variable.grad) or tensors.  Unsupported sizes: ValueError, there is no fallback."""
    if x.dim() != 3:
        raise ValueError("dien_gru: x must be [B, T, na]")
    B, T, na = x.shape
    params = [Wg, bg, Wc, bc]
    bc_t = bc.data if isinstance(bc, Variable) else bc
    nh = int(bc_t.shape[0]) if bc_t.dim() == 1 else 0
    _dien_check("dien_gru", B, T, na, nh, params, [(na + nh, 2 * nh), (2 * nh,), (na + nh, nh), (nh,)], ("Wg", "bg", "Wc", "bc"))
    _chk(x, torch.float32, "dien_gru: x")
    return _DienGruFn.apply(anchor, x, _dien_lengths(lengths, B, "dien_gru"), params, *_param_tail(params))


def dien_evolve(h: torch.Tensor, target: torch.Tensor, lengths: torch.Tensor, w_att, Wg, bg, Wc, bc, mode: str = "AGRU",
                anchor=None):
    """DIEN's interest evolution (dien.py:205-229) -> (final [B, nh], att [B, T], states [B, T, nh]): att = softmax over all T
    of h[b, t] . (w_att target_b) with the entries t >= L replaced by -2^32, then the AGRU / AUGRU recurrence over the rows of
    h with those weights; final is the state after step L - 1.  h [B, T, nh], target [B, na], lengths integer [B],
    w_att [nh, na], the cell's Wg [2 nh, 2 nh], bg [2 nh], Wc [2 nh, nh], bc [nh].  Only `final` carries a gradient."""
    if h.dim() != 3 or target.dim() != 2 or target.shape[0] != h.shape[0] or mode not in DIEN_MODES:
        raise ValueError("dien_evolve: h must be [B, T, nh], target [B, na] and mode one of " + ", ".join(DIEN_MODES))
    B, T, nh = h.shape
    na = target.shape[1]
    params = [w_att, Wg, bg, Wc, bc]
    _dien_check("dien_evolve", B, T, na, nh, params, [(nh, na), (2 * nh, 2 * nh), (2 * nh,), (2 * nh, nh), (nh,)],
                ("w_att", "Wg", "bg", "Wc", "bc"))
    _chk(h, torch.float32, "dien_evolve: h")
    _chk(target, torch.float32, "dien_evolve: target")
    if lengths is None:
        raise ValueError("dien_evolve: lengths are required")
    return _DienEvolveFn.apply(anchor, h, target, _dien_lengths(lengths, B, "dien_evolve"), DIEN_MODES[mode], params,
                               *_param_tail(params))


# =============================================================================================
# Serving (csrc/serve.hip, include/recalgo_serve.h): the inference tower of a small request, one launch
# =============================================================================================
_CS = _lib.SERVING_HEADERS["recalgo_serve.h"].constants       # the RECALGO_SERVE_* #defines of include/recalgo_serve.h
SERVE_MAX_LAYERS, SERVE_MAX_IN, SERVE_MAX_UNITS = (_CS["RECALGO_SERVE_MAX_LAYERS"], _CS["RECALGO_SERVE_MAX_IN"],
                                                   _CS["RECALGO_SERVE_MAX_UNITS"])


def serve_tower_supported(K0: int, units) -> bool:
    units = [int(u) for u in units]
    return bool(_lib_().recalgo_serve_tower_supported(int(K0), (ctypes.c_int * max(len(units), 1))(*units), len(units)))


def serve_tower(x: torch.Tensor, layers, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """include/recalgo_serve.h recalgo_serve_tower_fwd: h <- fmaf(relu?(h W + b), scale, shift) layer after layer, one launch.
    x [B, K0] fp32 contiguous; layers: [(W [K, units], b [units] | None, scale [units] | None, shift [units] | None, relu)].
    Inference only (no autograd node).  Shapes the kernel does not serve: ValueError — there is no fallback here; the caller
    (nn.LazyTower) asks serve_tower_supported first and runs the per-layer kernels otherwise."""
    if x.dim() != 2 or x.shape[0] == 0:
        raise ValueError("serve_tower: x must be a non-empty [B, K0] matrix")
    _chk(x, torch.float32, "serve_tower: x")
    B, K = int(x.shape[0]), int(x.shape[1])
    units, relu_bits = [], 0
    for l, (w, b, scale, shift, relu) in enumerate(layers):
        if w.dim() != 2 or int(w.shape[0]) != (units[-1] if units else K):
            raise ValueError(f"serve_tower: layer {l}'s kernel is {tuple(w.shape)}, its input has {units[-1] if units else K} columns")
        n = int(w.shape[1])
        for t, name in ((w, "kernel"), (b, "bias"), (scale, "scale"), (shift, "shift")):
            if t is not None:
                _chk(t, torch.float32, f"serve_tower: layer {l} {name}")
                if t.device != x.device or (t is not w and tuple(t.shape) != (n,)):
                    raise ValueError(f"serve_tower: layer {l} {name} must be a [{n}] tensor on {x.device}")
        if (scale is None) != (shift is None):
            raise ValueError(f"serve_tower: layer {l} has a scale without a shift (or the reverse)")
        units.append(n)
        relu_bits |= int(bool(relu)) << l
    if not serve_tower_supported(K, units):
        raise ValueError(f"serve_tower: the kernel serves 1 .. {SERVE_MAX_LAYERS} layers, 1 <= K0 <= {SERVE_MAX_IN} and widths of "
                         f"16 .. {SERVE_MAX_UNITS} that are multiples of 16; got K0={K} units={units}")
    if out is None:
        out = torch.empty(B, units[-1], device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, units[-1]) or out.device != x.device:
        raise ValueError("serve_tower: out must be [B, units[-1]] on x's device")
    else:
        _chk(out, torch.float32, "serve_tower: out")
    tables = [_ptr_array([ly[i] for ly in layers]) for i in range(4)]
    _lib_().recalgo_serve_tower_fwd(_p(x), *tables, (ctypes.c_int * len(units))(*units), len(units), relu_bits, B, K, _p(out),
                                    _stream(x))
    return out


# =============================================================================================
# Evaluation (csrc/metrics.hip, include/recalgo_metrics.h): every streaming metric of an EVAL batch and the loss sum, one launch
# =============================================================================================
_MH = _lib.SERVING_HEADERS["recalgo_metrics.h"]
_CM = _MH.constants                                            # the RECALGO_METRICS_* #defines of include/recalgo_metrics.h
_MetricsSlot = _MH.structs["recalgo_metrics_slot_t"]
METRICS_MAX_SLOTS, METRICS_MAX_THRESHOLDS = _CM["RECALGO_METRICS_MAX_SLOTS"], _CM["RECALGO_METRICS_MAX_THRESHOLDS"]
METRICS_KINDS = {"auc": _CM["RECALGO_METRICS_AUC"], "accuracy": _CM["RECALGO_METRICS_ACCURACY"]}


def metrics_element_stride(t: torch.Tensor) -> Optional[int]:
    """The element stride at which the kernel walks t's numel() values in order, None when there is no single one: a contiguous
    tensor (1), or one whose values lie along one dimension (a [B, 1] column view of a [B, T] matrix: T)."""
    long_dims = [int(st) for d, st in zip(t.shape, t.stride()) if d > 1]
    if not long_dims:
        return 1
    if len(long_dims) == 1:
        return long_dims[0] if long_dims[0] >= 1 else None
    if t.is_contiguous():
        return 1
    return None


def metrics_slot_table(slots):
    """slots: [("auc", labels, predictions, thresholds) | ("accuracy", labels, predictions)] -> (the ctypes table of
    recalgo_metrics_slot_t, word offset of each slot's counters in the state buffer, the buffer's size in 64-bit words)."""
    table = (_MetricsSlot * max(len(slots), 1))()
    first, word = [], 2
    for i, (kind, labels, predictions, *th) in enumerate(slots):
        s = table[i]
        s.kind = METRICS_KINDS[kind]
        s.labels, s.predictions = labels.data_ptr(), predictions.data_ptr()
        s.label_stride, s.prediction_stride = metrics_element_stride(labels) or 0, metrics_element_stride(predictions) or 0
        if kind == "auc":
            s.thresholds, s.num_thresholds = th[0].data_ptr(), int(th[0].numel())
        first.append(word)
        word += 2 * (s.num_thresholds + 1) if kind == "auc" else 2
    nbytes = int(_lib_().recalgo_metrics_state_bytes(table, len(slots)))
    if nbytes != 8 * word:
        raise ValueError(f"metrics: 1 .. {METRICS_MAX_SLOTS} slots, an AUC slot with 2 .. {METRICS_MAX_THRESHOLDS} thresholds")
    return table, first, word


def metrics_update(slots, loss: Optional[torch.Tensor], state: torch.Tensor) -> None:
    """include/recalgo_metrics.h recalgo_metrics_update: one launch adds a batch to `state` (int64 words, laid out as
    metrics_slot_table says, zeroed by the caller before the first batch) — per AUC slot hist[labels > 0.5][#{j : p > th[j]}],
    per accuracy slot (labels == predictions).sum() and the row count, and `loss` (fp32 scalar on the device, or None) into the
    double loss sum with one more batch counted.  Every tensor is fp32 on state's device; labels and predictions of a slot have the
    same number of elements, the same in every slot, at one element stride each (metrics_element_stride)."""
    n = int(slots[0][1].numel()) if slots else 0
    for kind, labels, predictions, *th in slots:
        for t, name in ((labels, "labels"), (predictions, "predictions")) + (((th[0], "thresholds"),) if kind == "auc" else ()):
            if t.dtype != torch.float32 or t.device != state.device:
                raise TypeError(f"metrics_update: {kind} {name} must be float32 on {state.device}")
        if labels.numel() != n or predictions.numel() != n or metrics_element_stride(labels) is None \
                or metrics_element_stride(predictions) is None or (kind == "auc" and not th[0].is_contiguous()):
            raise ValueError(f"metrics_update: {kind} labels and predictions must hold the batch's {n} values at one element stride")
    table, _, words = metrics_slot_table(slots)
    if state.dtype != torch.int64 or not state.is_contiguous() or state.numel() != words:
        raise ValueError(f"metrics_update: state must be a contiguous int64 tensor of {words} words")
    if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1 or loss.device != state.device):
        raise TypeError(f"metrics_update: loss must be one float32 value on {state.device}")
    _lib_().recalgo_metrics_update(table, len(slots), _p(loss), n, _p(state), _stream(state))


# The same metrics over the rows a mask selects (include/recalgo_maskmetrics.h): one launch for masked and unmasked slots together
_MaskMetricsSlot = _lib.SERVING_HEADERS["recalgo_maskmetrics.h"].structs["recalgo_maskmetrics_slot_t"]


def maskmetrics_update(slots, loss: Optional[torch.Tensor], state: torch.Tensor) -> None:
    """include/recalgo_maskmetrics.h recalgo_maskmetrics_update: `metrics_update` with one more element per slot tuple, a mask
    (fp32 on state's device, the batch's n values at one element stride) or None: ("auc", labels, predictions, thresholds, mask) |
    ("accuracy", labels, predictions, mask).  A row of a slot takes part iff the slot's mask is None or mask[i] > 0.5 (a NaN: no
    part); an accuracy slot counts the rows that take part.  The state buffer is metrics_slot_table's, word for word."""
    n = int(slots[0][1].numel()) if slots else 0
    for slot in slots:
        kind, labels, predictions, *th = slot[:-1]
        named = ((labels, "labels"), (predictions, "predictions")) + (((th[0], "thresholds"),) if kind == "auc" else ()) \
            + (((slot[-1], "mask"),) if slot[-1] is not None else ())
        for t, name in named:
            if t.dtype != torch.float32 or t.device != state.device:
                raise TypeError(f"maskmetrics_update: {kind} {name} must be float32 on {state.device}")
        if any(t.numel() != n or metrics_element_stride(t) is None for t, name in named if name != "thresholds") \
                or (kind == "auc" and not th[0].is_contiguous()):
            raise ValueError(f"maskmetrics_update: {kind} labels, predictions and mask must hold the batch's {n} values at one element stride")
    _, _, words = metrics_slot_table([s[:-1] for s in slots])
    table = (_MaskMetricsSlot * max(len(slots), 1))()
    for s, (kind, labels, predictions, *th, mask) in zip(table, slots):
        s.kind = METRICS_KINDS[kind]
        s.labels, s.predictions = labels.data_ptr(), predictions.data_ptr()
        s.label_step, s.prediction_step = metrics_element_stride(labels), metrics_element_stride(predictions)
        if kind == "auc":
            s.thresholds, s.num_thresholds = th[0].data_ptr(), int(th[0].numel())
        if mask is not None:
            s.mask, s.mask_step = mask.data_ptr(), metrics_element_stride(mask)
    if state.dtype != torch.int64 or not state.is_contiguous() or state.numel() != words:
        raise ValueError(f"maskmetrics_update: state must be a contiguous int64 tensor of {words} words")
    if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1 or loss.device != state.device):
        raise TypeError(f"maskmetrics_update: loss must be one float32 value on {state.device}")
    _lib_().recalgo_maskmetrics_update(table, len(slots), _p(loss), n, _p(state), _stream(state))


# =============================================================================================
# Per-group AUC (csrc/gauc.hip, include/recalgo_gauc.h): uAUC / GAUC as integer pair counts per group — one append launch per
# batch into a row log on the device, and a finish (count, scan, place, pairs) once per evaluation
# =============================================================================================
_GH = _lib.SERVING_HEADERS["recalgo_gauc.h"]
_CG = _GH.constants                                            # the RECALGO_GAUC_* #defines of include/recalgo_gauc.h
_GaucColumn = _GH.structs["recalgo_gauc_column_t"]
GAUC_MAX_TASKS, GAUC_MAX_GROUPS, GAUC_MAX_ROWS = _CG["RECALGO_GAUC_MAX_TASKS"], _CG["RECALGO_GAUC_MAX_GROUPS"], _CG["RECALGO_GAUC_MAX_ROWS"]
GAUC_STATE_HEADER_WORDS, GAUC_RESULT_HEADER_WORDS = _CG["RECALGO_GAUC_STATE_HEADER_WORDS"], _CG["RECALGO_GAUC_RESULT_HEADER_WORDS"]


def gauc_shape_ok(num_groups, tasks, capacity) -> bool:
    """What the header's launches accept (decided without loading the library)"""
    ints = all(isinstance(v, int) and not isinstance(v, bool) for v in (num_groups, tasks, capacity))
    return ints and 1 <= tasks <= GAUC_MAX_TASKS and 1 <= num_groups <= GAUC_MAX_GROUPS and 1 <= capacity <= GAUC_MAX_ROWS


class GaucState:
    """The three caller-owned buffers of include/recalgo_gauc.h for (num_groups, tasks, capacity), as int64 tensors:
    .state (header zeroed: no row yet), .result [3 + 3 T G] and .workspace."""

    def __init__(self, num_groups: int, tasks: int, capacity: int, device):
        if not gauc_shape_ok(num_groups, tasks, capacity):
            raise ValueError(f"gauc_state: 1 .. {GAUC_MAX_TASKS} tasks, 1 .. {GAUC_MAX_GROUPS} groups and a capacity of 1 .. "
                             f"{GAUC_MAX_ROWS} rows; got {tasks}, {num_groups}, {capacity}")
        self.G, self.T, self.C = num_groups, tasks, capacity
        lib = _lib_()
        sb, wb = int(lib.recalgo_gauc_state_bytes(self.G, self.T, self.C)), int(lib.recalgo_gauc_workspace_bytes(self.G, self.T, self.C))
        self.state = torch.empty(sb // 8, dtype=torch.int64, device=device)
        self.state[:GAUC_STATE_HEADER_WORDS].zero_()
        self.workspace = torch.empty(wb // 8, dtype=torch.int64, device=device)
        self.result = torch.empty(GAUC_RESULT_HEADER_WORDS + 3 * self.T * self.G, dtype=torch.int64, device=device)


def gauc_state(num_groups: int, tasks: int, capacity: int, device) -> GaucState:
    return GaucState(num_groups, tasks, capacity, device)


def gauc_append(st: GaucState, groups: torch.Tensor, columns) -> None:
    """recalgo_gauc_append: one launch logs a batch behind the rows `st` already holds.  groups: int64 ids, one per row, at one
    element stride (a [B] column view of a packed [B, F] id matrix is fine); columns: st.T pairs (labels, predictions) of fp32
    tensors with as many elements, each at one element stride.  No allocation, no read-back: capturable."""
    n = int(groups.numel())
    gs = metrics_element_stride(groups)
    if groups.dtype != torch.int64 or groups.device != st.state.device or gs is None:
        raise TypeError(f"gauc_append: groups must be int64 on {st.state.device} at one element stride")
    if len(columns) != st.T:
        raise ValueError(f"gauc_append: {len(columns)} columns for a state of {st.T} tasks")
    table = (_GaucColumn * st.T)()
    for c, (labels, predictions) in zip(table, columns):
        for t, name in ((labels, "labels"), (predictions, "predictions")):
            if t.dtype != torch.float32 or t.device != st.state.device:
                raise TypeError(f"gauc_append: {name} must be float32 on {st.state.device}")
        c.label_step, c.prediction_step = metrics_element_stride(labels) or 0, metrics_element_stride(predictions) or 0
        if labels.numel() != n or predictions.numel() != n or not c.label_step or not c.prediction_step:
            raise ValueError(f"gauc_append: labels and predictions must hold the batch's {n} values at one element stride")
        c.labels, c.predictions = labels.data_ptr(), predictions.data_ptr()
    _lib_().recalgo_gauc_append(_p(groups), gs, table, st.T, n, st.G, st.C, _p(st.state), _stream(st.state))


def gauc_finish(st: GaucState) -> torch.Tensor:
    """recalgo_gauc_finish over every row appended so far -> st.result on the device (gauc_counts reads a host copy of it).  The
    log is left as it is: more rows may follow, and another finish then counts all of them."""
    _lib_().recalgo_gauc_finish(_p(st.state), st.G, st.T, st.C, _p(st.result), _p(st.workspace), _stream(st.state))
    return st.result


def gauc_counts(result: torch.Tensor, num_groups: int, tasks: int):
    """A host copy of a result buffer -> (skipped, dropped, rows, num2 [T, G], pos [T, G], neg [T, G]) as ints and int64 arrays"""
    r = result.cpu().numpy()
    h = GAUC_RESULT_HEADER_WORDS
    num2, pos, neg = r[h:].reshape(3, tasks, num_groups)
    return int(r[0]), int(r[1]), int(r[2]), num2, pos, neg
