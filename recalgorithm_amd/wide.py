"""The wide part of Wide&Deep on the device (include/recalgo_wide.h, csrc/wide.hip): host-side state and the autograd
Function of `tf.layers.dense(fc.input_layer(features, [indicator_column(crossed_column([a, b], H))]), 1)`.

The [B, H] multi-hot never exists.  The forward hashes every (example, tag) request to its bucket, keeps the buckets in a
workspace of FIXED capacity (the length of the bag's value tensor: nothing is sized by the batch's request count, so the
step captures into a hipGraph) and writes the logit.  The backward only keeps d loss / d logit; the optimizer
(estimator.FtrlOptimizer) then runs the plan (count -> place -> rank) and the per-bucket ordered sum fused with FTRL.  Whoever
reads the kernel's gradient before that (tests, variables.named_grads) gets it summed into Variable.grad first
(materialize_grads), and the FTRL launch clears it again: the dense Adam launch that sweeps the store's flat buffer afterwards
sees g = 0 on the wide variables, whose Adam moments therefore stay 0 — the identity.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch
from torch.autograd import Function

from . import _lib
from .variables import Variable, VariableStore

_C = _lib.HEADERS["recalgo_wide.h"].constants
HASH_KEY = _C["RECALGO_WIDE_HASH_KEY"]
MAX_BUCKETS = _C["RECALGO_WIDE_MAX_BUCKETS"]
APPLY_FTRL, APPLY_GRAD = _C["RECALGO_WIDE_APPLY_FTRL"], _C["RECALGO_WIDE_APPLY_GRAD"]


NO_DATA_PARALLEL = ("a model with a crossed wide column (nn.crossed_indicator_dense, trained by FtrlOptimizer) runs on one GPU: "
                    "its FTRL update consumes the LOCAL gradient of the touched buckets, which attach_data_parallel would "
                    "have to all-reduce first")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t: torch.Tensor):
    if not t.is_cuda:
        raise _lib.RecalgoError("recalgo ops run only on a HIP device (no CPU fallback); got a CPU tensor")
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _capturing(device) -> bool:
    return torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing()


class WideState:
    """Everything one crossed wide layer keeps between launches: the per-bucket counts / segment starts (persistent, zero
    between steps), the request workspace, the pending d loss / d logit of the step, and the FTRL slots."""

    def __init__(self, kernel: Variable, bias: Optional[Variable], hash_bucket_size: int, hash_key: int):
        self.kernel, self.bias = kernel, bias
        self.H, self.hash_key = int(hash_bucket_size), int(hash_key)
        self.table = None            # int32 [2 * H]: count, start
        self.ws, self.capacity = None, 0     # the TRAIN forward's request workspace, the capacity it is laid out for
        self.ws_infer, self.capacity_infer = None, 0
        self.counted = False         # the last forward counted its requests and nothing has returned the counts to zero yet
        self.dlogit = None           # the step's d loss / d wide_logit [B, 1] (set by the backward)
        self.planned = False         # recalgo_wide_cross_plan ran for self.dlogit
        self.grad_materialized = False
        self.slots: Dict[str, torch.Tensor] = {}      # "<var name>/Ftrl" (accum), "<var name>/Ftrl_1" (linear)
        self.ftrl_steps = 0          # FTRL steps applied so far (host side: the first one also zeroes the untouched buckets)

    def _reset_counts(self) -> None:
        if self.counted:
            _lib.load().recalgo_wide_cross_reset(_p(self.ws), _p(self.table), self.capacity, _stream(self.ws))
        self.counted = self.planned = self.grad_materialized = False
        self.dlogit = None

    def prepare(self, capacity: int, device, count: bool) -> torch.Tensor:
        """-> the request workspace of a forward of `capacity` requests.  A counting (TRAIN) forward owns `self.ws` until its
        FTRL apply: a counted step that never reached it is undone first (its counts return to zero).  Any other forward
        (PREDICT / EVAL, possibly between a TRAIN forward and its apply) writes its buckets to a buffer of its own."""
        lib = _lib.load()
        if self.table is None:
            self.table = torch.zeros(int(lib.recalgo_wide_state_workspace_bytes(self.H)) // 4, dtype=torch.int32, device=device)
        need = int(lib.recalgo_wide_workspace_bytes(int(capacity)))
        which = "ws" if count else "ws_infer"
        if count:
            self._reset_counts()
            self.capacity = int(capacity)
        else:
            self.capacity_infer = int(capacity)
        buf = getattr(self, which)
        if buf is None or buf.numel() < need:
            if _capturing(device):
                raise RuntimeError("wide layer: its workspace must exist before the step is captured (run one eager step first)")
            buf = torch.empty(need, dtype=torch.uint8, device=device)
            setattr(self, which, buf)
        return buf

    def last_requests(self, training: bool = True):
        """-> (example int32 [n], bucket int32 [n]) of the last TRAIN (or other) forward, read back from its workspace (one
        host synchronisation: tests and tools)."""
        ws, cap = (self.ws, self.capacity) if training else (self.ws_infer, self.capacity_infer)
        words = ws[:16 + 8 * cap].view(torch.int32)
        n = int(words[0])
        return words[4 + cap:4 + cap + n].clone(), words[4:4 + n].clone()

    def ensure_slots(self, initial_accumulator_value: float) -> None:
        if self.slots:
            return
        if _capturing(self.kernel.data.device):
            raise RuntimeError("FtrlOptimizer: its slots must exist before the step is captured (run one eager step first)")
        for v in (self.kernel, self.bias):
            if v is not None:
                self.slots[v.name + "/Ftrl"] = torch.full_like(v.data, float(initial_accumulator_value))
                self.slots[v.name + "/Ftrl_1"] = torch.zeros_like(v.data)

    # -- the backward's plan, the gradient, the update ------------------------------------------------------------------------
    def _plan(self) -> None:
        if not self.planned:
            _lib.load().recalgo_wide_cross_plan(_p(self.ws), _p(self.table), self.capacity, self.H, _p(self.dlogit),
                                                _stream(self.dlogit))
            self.planned = True

    def _apply(self, mode, lr=1.0, l1=0.0, l2=0.0, zero_untouched=False) -> None:
        k, b, s = self.kernel, self.bias, self.slots
        ftrl = mode == APPLY_FTRL
        kg = k.grad if (mode == APPLY_GRAD or self.grad_materialized) else None
        _lib.load().recalgo_wide_cross_apply(
            _p(self.ws), _p(self.table), self.capacity, self.H, mode, _p(k.data), _p(kg),
            _p(s[k.name + "/Ftrl"]) if ftrl else None, _p(s[k.name + "/Ftrl_1"]) if ftrl else None,
            _p(b.data) if (ftrl and b is not None) else None, _p(b.grad) if (ftrl and b is not None) else None,
            _p(s[b.name + "/Ftrl"]) if (ftrl and b is not None) else None,
            _p(s[b.name + "/Ftrl_1"]) if (ftrl and b is not None) else None,
            float(lr), float(l1), float(l2), int(bool(zero_untouched)), _stream(k.data))

    def materialize_grad(self) -> None:
        """kernel.grad[j] = the ordered sum of bucket j's requests (buckets without a request keep their 0)."""
        if self.dlogit is None or self.grad_materialized:
            return
        self._plan()
        self._apply(APPLY_GRAD)
        self.grad_materialized = True

    def apply_ftrl(self, lr: float, l1: float, l2: float, initial_accumulator_value: float) -> None:
        if self.dlogit is None:
            raise RuntimeError(f"FtrlOptimizer: no gradient reached {self.kernel.name} in this step")
        self.ensure_slots(initial_accumulator_value)
        first = self.ftrl_steps == 0
        if first and _capturing(self.kernel.data.device):
            raise RuntimeError("FtrlOptimizer: the first step zeroes every bucket the batch did not touch, once: it cannot be "
                               "part of a captured graph (run one eager step first)")
        self._plan()
        self._apply(APPLY_FTRL, lr, l1, l2, zero_untouched=first)
        self.ftrl_steps += 1
        self.counted = self.planned = self.grad_materialized = False
        self.dlogit = None


def states(store: VariableStore) -> Dict[str, WideState]:
    """kernel variable name -> WideState of every crossed wide layer of the store"""
    return store.__dict__.setdefault("wide_states", {})


def state_of(store: VariableStore, var: Variable) -> Optional[WideState]:
    for st in states(store).values():
        if var is st.kernel or var is st.bias:
            return st
    return None


def materialize_grads(store: VariableStore) -> None:
    for st in states(store).values():
        st.materialize_grad()


class _WideCrossFn(Function):
    @staticmethod
    def forward(ctx, anchor, st: WideState, user_ids, tag_values, tag_offsets, training):
        lib = _lib.load()
        B = int(user_ids.shape[0])
        dev = user_ids.device
        if tag_offsets is not None and tag_values.numel() == 0:
            tag_values = torch.full((1,), -1, dtype=torch.int64, device=dev)       # (every bag is empty: never read)
        capacity = int(tag_values.numel())
        ws = st.prepare(capacity, dev, count=bool(training))
        out = torch.empty(B, 1, device=dev, dtype=torch.float32)
        dense_tags = tag_offsets is None
        lib.recalgo_wide_cross_fwd(_p(user_ids), int(user_ids.stride(0)), _p(tag_values), _p(tag_offsets),
                                   int(tag_values.stride(0)) if dense_tags else 1, B, capacity, st.H, st.hash_key,
                                   _p(st.kernel.data), None if st.bias is None else _p(st.bias.data), _p(ws),
                                   _p(st.table) if training else None, _p(out), _stream(out))
        st.counted = bool(training) or st.counted
        ctx.st = st
        return out

    @staticmethod
    def backward(ctx, g):
        st = ctx.st
        if g is None:
            return None, None, None, None, None, None
        g = g.contiguous()
        st.dlogit = g
        st.planned = st.grad_materialized = False
        if st.bias is not None:
            from . import ops
            if not ops.colsum_of_dlogit(g, st.bias.grad.view(1)):      # (TRAIN step: a job of the step's deferred-sum launch)
                torch.sum(g, dim=0, out=st.bias.grad.view(1))
        return None, None, None, None, None, None


def cross_logit(store: VariableStore, st: WideState, user_ids: torch.Tensor, tag_values: torch.Tensor,
                tag_offsets: Optional[torch.Tensor], training: bool = True) -> torch.Tensor:
    """-> wide_logit [B, 1] = bias + sum over the example's (user, tag) requests of kernel[bucket].  tag_offsets None: one
    tag per example (tag_values [B]).  `training`: the step's backward and FTRL apply follow (the requests are counted)."""
    for t, name in ((user_ids, "user ids"), (tag_values, "tag values"), (tag_offsets, "tag offsets")):
        if t is not None and (t.dtype != torch.int64 or t.dim() != 1):
            raise TypeError(f"wide cross: {name} must be a 1-D int64 tensor")
    if user_ids.shape[0] < 1:
        raise NotImplementedError("wide cross: empty batch")
    if tag_offsets is not None:
        if not (tag_values.is_contiguous() and tag_offsets.is_contiguous()) or tag_offsets.numel() != user_ids.shape[0] + 1:
            raise ValueError("wide cross: contiguous bag values and B + 1 contiguous offsets")
    elif tag_values.shape[0] != user_ids.shape[0]:
        raise ValueError("wide cross: one tag per example needs as many tags as examples")
    return _WideCrossFn.apply(store.anchor, st, user_ids, tag_values, tag_offsets,
                              bool(training) and torch.is_grad_enabled())
