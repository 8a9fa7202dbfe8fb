"""tf.layers.{dense, batch_normalization, dropout} look-alikes for the mirrored model_fns.

These are the "context" MLP of the models.  `dense` runs on the hand-written fp32-MFMA
kernels of csrc/dense.hip (bias + ReLU fused in the forward, the ReLU mask and the bias gradient fused in the
backward); layers wider than DENSE_MAX_K inputs (FiBiNET's 9600 -> 512) run on hipBLASLt through torch.  Parameter
gradients are written straight into the flat gradient buffer (variables.py).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function

from .variables import Variable, current_store, glorot_uniform, ones, zeros


def _hip(x: torch.Tensor, C: int) -> bool:
    """The fused HIP glue kernels serve contiguous fp32 device tensors of a supported width."""
    from . import ops
    return x.is_cuda and x.dtype == torch.float32 and ops.mlp_width_supported(C)


DENSE_MAX_K = 4096
FUSED_TAIL = True           # dense(last_hidden=True) may hand the layer to the fused layer + head + loss kernel (tests switch it off to compare)


def _mfma_dense(in_features: int = 0) -> bool:
    """The hand-written fp32-MFMA kernels with fused epilogues (csrc/dense.hip) serve layers of up to DENSE_MAX_K input
    features.  Wider layers are plain large GEMMs whose gradient tiles have short reductions (FiBiNET's 9600 -> 512: 150
    column tiles of 16 chunks each): the per-tile prologue / epilogue of the 64 x 64 engine then costs 25 % — the step is
    1.546 ms on it against 1.342 ms with the library kernels (round 5, same box; round 2: 1.57 vs 1.42) — those go to
    hipBLASLt through torch."""
    return in_features <= DENSE_MAX_K


class GradJoin:
    """A tensor consumed by two branches (DCN's x0 feeds the cross network and the MLP, dcn.py:157-166) receives the
    SUM of the two input gradients — in autograd an extra elementwise launch.  With a GradJoin shared by the two ops,
    the branch whose backward runs first (`dense`: it is created later in the forward) parks its input gradient here
    instead of returning it, and the other branch's backward kernel adds it in its own epilogue
    (`recalgo_cross_bwd`'s g_x0_extra) and returns the total.  If the order is ever the other way round, or the
    consumer cannot take it, both gradients are returned normally and autograd adds them."""

    def __init__(self):
        self.pending: Optional[torch.Tensor] = None
        self.consumer_done = False
        # the OTHER direction (ops.defer_cross_rider): the cross network's backward already ran — as a rider of an upper dense
        # layer's launch — and left its dx0 here; the MLP's first layer adds it in its input-gradient epilogue (beta * C, beta = 1)
        self.early_dx: Optional[torch.Tensor] = None
        self.early_used = False

    def take_early(self) -> Optional[torch.Tensor]:
        t, self.early_dx = self.early_dx, None
        if t is not None:
            self.early_used = True
        return t

    def park(self, dx: torch.Tensor) -> bool:
        if self.consumer_done or self.pending is not None:
            return False
        self.pending = dx
        return True

    def take(self) -> Optional[torch.Tensor]:
        t, self.pending, self.consumer_done = self.pending, None, True
        return t


class BNLink:
    """A training-mode BatchNorm whose output feeds a dense layer (tf.layers.batch_normalization -> tf.layers.dense): the
    dense layer's backward kernel can leave the two column sums BatchNorm's backward starts with (ops.dense_bwd(bn=)).  The
    BatchNorm attaches a BNLink to its output tensor; a dense layer that finds one on its input fills `sums` in its backward
    and records which gradient tensor they belong to; the BatchNorm's backward uses them only if that IS the gradient it is
    given (another consumer of the BatchNorm output, or anything in between, makes autograd hand over a different tensor)."""

    def __init__(self, x, mean, rstd):
        self.x, self.mean, self.rstd = x, mean, rstd
        self.sums, self.grad_ptr = None, 0

    def new_sums(self) -> torch.Tensor:
        from . import ops
        rows, C = self.x.shape
        self.sums = torch.empty(ops.bn_partial_rows(rows), 2 * C, device=self.x.device, dtype=torch.float32)
        return self.sums

    def take(self, g: torch.Tensor):
        sums, self.sums = self.sums, None
        return sums if (sums is not None and g.data_ptr() == self.grad_ptr and g.is_contiguous()) else None


def _attach_link(out: torch.Tensor) -> torch.Tensor:
    """the BNLink the node's forward made (ctx.link), hung on the output tensor for the consumer to find"""
    link = getattr(out.grad_fn, "link", None) if out.grad_fn is not None else None
    if link is not None:
        out._recalgo_bn_link = link
    return out


def _bn_link_of(x: torch.Tensor):
    link = getattr(x, "_recalgo_bn_link", None)
    return link if (link is not None and x.dim() == 2 and x.is_contiguous() and tuple(x.shape) == tuple(link.x.shape)) else None


class ReluSource:
    """Rides on the output tensor of a tf.layers.dense(..., relu) (`_recalgo_relu_src`).  A consumer whose backward kernel can
    mask its input gradient with that tensor itself — the next dense layer (recalgo_dense_bwd dx_relu_mask), the fused
    loss tail (recalgo_logit_loss_fwd_bwd relu_parts) — does so and leaves the gradient tensor here; the producing layer's
    backward skips its own mask (the mask loads of both of its GEMMs) when the gradient autograd hands it IS that tensor.
    Any other consumer of the activation makes autograd sum into a new tensor (the reference held here keeps the engine from
    accumulating in place): the pointer differs and the mask is applied as before — idempotent on the pre-masked share."""
    __slots__ = ("premasked",)

    def __init__(self):
        self.premasked = None

    def take(self, g: torch.Tensor) -> bool:
        pm, self.premasked = self.premasked, None
        return pm is not None and pm.data_ptr() == g.data_ptr() and pm.shape == g.shape and pm.stride() == g.stride()


class _DenseFn(Function):
    @staticmethod
    def forward(ctx, anchor, x, kernel: Variable, bias: Optional[Variable], relu: bool, input_l2: float = 0.0,
                grad_join: Optional[GradJoin] = None, bn_partials: Optional[torch.Tensor] = None,
                relu_src: Optional[ReluSource] = None, drop=None):
        ctx.input_l2 = float(input_l2)
        ctx.drop_scale = 1.0 if drop is None else float(drop.scale)
        ctx.grad_join = grad_join
        ctx.bn_link = _bn_link_of(x)
        ctx.relu_src = relu_src
        ctx.x_relu_src = getattr(x, "_recalgo_relu_src", None) if (x.dim() == 2 and x.is_contiguous()) else None
        if getattr(x, "_recalgo_relu_scale", 1.0) != 1.0:
            ctx.x_relu_src = None              # (only the BatchNorm backward scales while it masks: the producer does it itself)
        x2 = x.reshape(-1, x.shape[-1])
        ctx.hip = x2.is_cuda and x2.dtype == torch.float32 and _mfma_dense(x2.shape[1])
        if ctx.hip:
            from . import ops
            if x2.stride(1) != 1:
                x2 = x2.contiguous()
            # GEMM + bias + ReLU in one launch
            # (drop: the tf.layers.dropout behind the layer applied by the epilogue — y IS the dropped tensor, y > 0 <=> relu > 0 and kept)
            y = ops.dense_fwd(x2, kernel.data, None if bias is None else bias.data, relu, bn_partials=bn_partials, drop=drop)
        elif drop is not None:
            raise ValueError("dense(drop=): only with the hand-written kernels (the caller checks nn.dense_drop_supported)")
        elif bias is not None and relu and x2.is_cuda:
            y = torch._addmm_activation(bias.data, x2, kernel.data)     # GEMM + bias + ReLU epilogue (hipBLASLt)
        else:
            y = torch.addmm(bias.data, x2, kernel.data) if bias is not None else x2 @ kernel.data
            if relu:
                y = torch.relu_(y)
        ctx.vars = (kernel, bias)
        ctx.relu = relu
        ctx.xshape = x.shape
        ctx.save_for_backward(x2, y if relu else None)
        return y.view(*x.shape[:-1], kernel.data.shape[1])

    @staticmethod
    def backward(ctx, g):
        from . import ops
        kernel, bias = ctx.vars
        x2, y = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        if ctx.hip:
            if g2.stride(1) != 1 or (y is not None and g2.stride() != y.stride()):
                g2 = g2.contiguous()
            # the ReLU mask rides on the staging of g in both GEMMs, the bias gradient on the weight-gradient one; the
            # split partials of the weight gradient are summed by ONE launch per backward pass (ops.flush_dense_splits)
            mask = y if ctx.relu else None
            if mask is not None and ctx.relu_src is not None and ctx.relu_src.take(g2):
                mask = None                        # the consumer's backward kernel masked (and, behind a fused dropout, scaled) its dx with y already
            elif ctx.drop_scale != 1.0:
                g2 = g2 * ctx.drop_scale           # (no consumer did it: d/d relu of relu * keep / (1 - rate), the keep part is the mask y > 0)
            db = None if bias is None else bias.grad
            if ctx.needs_input_grad[1]:
                # input and weight gradient in ONE launch
                link = ctx.bn_link if ctx.grad_join is None else None
                src = ctx.x_relu_src if ctx.grad_join is None else None
                c_in, beta = (x2, ctx.input_l2) if ctx.input_l2 else (None, 0.0)
                early = None
                if ctx.grad_join is not None and c_in is None and ctx.grad_join.early_dx is not None:
                    e = ctx.grad_join.early_dx
                    if tuple(e.shape) == tuple(x2.shape) and e.is_contiguous():
                        early = ctx.grad_join.take_early()       # the other consumer's input gradient, already computed: dx += it
                        c_in, beta = early, 1.0
                dx = ops.dense_bwd(x2, g2, mask, kernel.data, kernel.grad, db, c_in=c_in, beta=beta, defer=True,
                                   bn=None if link is None else (link.x, link.mean, link.rstd, link.new_sums()),
                                   premask=None if src is None else x2, cross_rider=ctx.grad_join is None).view(ctx.xshape)
                if src is not None:
                    src.premasked = dx             # x is the ReLU output of the layer below: its gradient is masked here
                if link is not None:
                    link.grad_ptr = dx.data_ptr()
                if ctx.grad_join is not None and early is None and ctx.grad_join.park(dx):
                    dx = None                      # added by the other consumer of x in its backward kernel
                return None, dx, None, None, None, None, None, None, None, None
            # (no input gradient wanted: the first layer over a non-differentiable input.  Tried in round 2: the weight
            # gradient on a second stream beside the dgrad chain — DCN 0.319 vs 0.268 ms; removed)
            ops.dense_bwd_weights(x2, g2, mask, kernel.grad, db, defer=True)
            return None, None, None, None, None, None, None, None, None, None
        if not g2.is_contiguous():
            g2 = g2.contiguous()
        if bias is not None and _hip(g2, g2.shape[1]):
            # one fused pass: ReLU mask + bias gradient (csrc/mlp.hip)
            g2 = ops.relu_bwd_bias_(g2, y if ctx.relu else None, bias.grad)
        else:
            if ctx.relu:
                g2 = g2 * (y > 0)
            if bias is not None:
                torch.sum(g2, dim=0, out=bias.grad)
        torch.mm(x2.t(), g2, out=kernel.grad)
        if ctx.input_l2:
            # d/dx of the activity regulariser (input_l2 / 2) * sum(x^2) rides on the GEMM as its beta * C term
            dx = torch.addmm(x2, g2, kernel.data.t(), beta=ctx.input_l2)
        else:
            dx = g2 @ kernel.data.t()
        return None, dx.view(ctx.xshape), None, None, None, None, None, None, None, None


class _Dense1Fn(Function):
    """tf.layers.dense(tf.concat(parts, -1), 1): one fused pass each way (csrc/mlp.hip dense1_*)."""

    @staticmethod
    def forward(ctx, anchor, kernel: Variable, bias: Optional[Variable], *parts):
        from . import ops
        ctx.vars = (kernel, bias)
        ctx.save_for_backward(*parts)
        return ops.dense1_fwd(parts, kernel.data, None if bias is None else bias.data)

    @staticmethod
    def backward(ctx, g):
        from . import ops
        kernel, bias = ctx.vars
        parts = ctx.saved_tensors
        dxs = [torch.empty_like(t) if need else None for t, need in zip(parts, ctx.needs_input_grad[3:])]
        ops.dense1_bwd(parts, kernel.data, g.contiguous(), dxs, kernel.grad, None if bias is None else bias.grad)
        return (None, None, None, *dxs)


class LazyDense:
    """`tf.layers.dense(x, units, relu)` — the LAST hidden layer of a TRAIN step — not evaluated yet: when its only consumer
    turns out to be the one-unit head in front of the loss (dcn.py:166-172), model_tail.finish_model_fn runs layer, head, loss and
    their backward as ONE kernel (ops.tail_dense_head).  Any other use goes through `materialize()`: the layer as `dense` runs it."""

    def __init__(self, x, kernel: Variable, bias: Variable, grad_join=None):
        self.x, self.kernel, self.bias, self.grad_join = x, kernel, bias, grad_join
        self._out = None

    @property
    def shape(self):
        return (*self.x.shape[:-1], int(self.kernel.data.shape[1]))

    def dim(self):
        return self.x.dim()

    @property
    def is_cuda(self):
        return self.x.is_cuda

    def materialize(self) -> torch.Tensor:
        if self._out is None:
            store = current_store()
            src = ReluSource()
            self._out = _DenseFn.apply(store.anchor, self.x, self.kernel, self.bias, True, 0.0, self.grad_join, None, src, None)
            self._out._recalgo_relu_src = src
        return self._out


def _resolved(t):
    return t.materialize() if isinstance(t, (LazyDense, LazyTower)) else t


# ServingModel.compile's switch (VariableStore.serving) routes the hidden stack of a PREDICT graph into ONE launch (ops.serve_tower)
# for request buckets of at most this many rows: the largest measured bucket at which the compiled graph with the fused tower
# is no slower than the compiled graph on the per-layer kernels (profiles/serving_bench.json, DESIGN.md §5 "Serving").
SERVE_TOWER_MAX_ROWS = 4096
# ...and only where the tower folds at least one BatchNorm.  A plain dense(relu) stack (DCN's) is three launches of the dense
# engine, which the same measurement has FASTER than the tower at every size (0.044 against 0.058 ms of device time per request
# at n = 1): such a stack is collected all the same — whether a BatchNorm follows is known only at the end — and then runs
# on the per-layer kernels, the launches it would have had without the switch.  True: plain stacks take the tower too (tests, the bench).
SERVE_TOWER_PLAIN_STACKS = False


class ServingPlan:
    """What ServingModel.compile hangs on VariableStore.serving while it captures a bucket: the row limit of the fused tower
    for this bucket and the BatchNorm folds, computed once per export: {<scope>/gamma: (scale, shift)} at `epsilon`.
    `tower_launches` counts the ops.serve_tower launches made under this plan (warm-up calls and the capture)."""

    def __init__(self, max_rows: int, folds: dict, epsilon: float):
        self.max_rows, self.folds, self.epsilon = int(max_rows), folds, float(epsilon)
        self.tower_launches = 0


class LazyTower:
    """Consecutive `dense(relu) -> [dropout = identity] -> [batch_normalization(training=False)]` layers of a PREDICT graph under
    the serving switch, not evaluated yet: whatever consumes the stack (the one-unit head, a concat) gets it from ONE launch
    (ops.serve_tower, include/recalgo_serve.h) instead of one or two launches per layer.  LazyDense is the precedent.
    A tower is a value: a layer or a fold added gives a NEW tower over the same input and the same first layers, so a model_fn
    that keeps a hidden layer's output beside the next layer's holds two different stacks, each evaluated when used."""

    def __init__(self, x: torch.Tensor, layers=(), plan=None):
        self.x, self.plan = x, plan
        self.layers = tuple(layers)           # ((kernel Variable, bias Variable | None, scale | None, shift | None), ..)
        self._out = None

    @property
    def shape(self):
        return (self.x.shape[0], int(self.layers[-1][0].data.shape[1]))

    def dim(self):
        return 2

    @property
    def is_cuda(self):
        return True

    def units(self):
        return [int(ly[0].data.shape[1]) for ly in self.layers]

    def with_layer(self, kernel: Variable, bias: Optional[Variable]) -> "LazyTower":
        return LazyTower(self.x, self.layers + ((kernel, bias, None, None),), self.plan)

    def with_fold(self, scale: torch.Tensor, shift: torch.Tensor) -> "LazyTower":
        """the tower whose last layer's epilogue applies a BatchNorm's (scale, shift)"""
        kernel, bias, _, _ = self.layers[-1]
        return LazyTower(self.x, self.layers[:-1] + ((kernel, bias, scale, shift),), self.plan)

    def materialize(self) -> torch.Tensor:
        if self._out is None:
            from . import ops
            if SERVE_TOWER_PLAIN_STACKS or any(ly[2] is not None for ly in self.layers):
                self._out = ops.serve_tower(self.x, [(k.data, None if b is None else b.data, sc, sh, True) for k, b, sc, sh in self.layers])
                if self.plan is not None:
                    self.plan.tower_launches += 1
            else:                             # no BatchNorm to fold: the layers as `dense` runs them
                out, store = self.x, current_store()
                for kernel, bias, _, _ in self.layers:
                    out = _DenseFn.apply(store.anchor, out, kernel, bias, True, 0.0, None, None, ReluSource(), None)
                self._out = out
        return self._out


def _serving_tower(store, x, units: int):
    """The LazyTower a relu layer of `units` columns over x extends (an empty one over a plain tensor), or None: the serving
    switch is on (a PREDICT capture of ServingModel.compile), the bucket is small enough, and the kernel serves the stack
    with this layer added."""
    plan = getattr(store, "serving", None)
    if plan is None or store.building or torch.is_grad_enabled():
        return None
    from . import ops
    if isinstance(x, LazyTower):
        if x._out is None:
            ok = len(x.layers) < ops.SERVE_MAX_LAYERS and ops.serve_tower_supported(x.x.shape[1], x.units() + [units])
            return x if ok else None
        x = x._out                            # (already evaluated for another consumer: a new tower starts at its output)
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            and 1 <= x.shape[0] <= plan.max_rows and x.data_ptr() % 4 == 0 and ops.serve_tower_supported(x.shape[1], [units])):
        return None
    return LazyTower(x, (), plan)


class LazyConcat:
    """`tf.concat(values, axis=-1)` whose consumer is a one-unit `dense`: the head kernel reads the
    parts in place, so the [B, sum(widths)] copy (and the two slice copies of its gradient) never
    happen.  Any other use goes through `materialize()`."""

    def __init__(self, values):
        self.parts = list(values)

    @property
    def shape(self):
        return (*self.parts[0].shape[:-1], sum(int(t.shape[-1]) for t in self.parts))

    def materialize(self) -> torch.Tensor:
        return torch.cat([_resolved(t) for t in self.parts], dim=-1)


class LazyLogit:
    """`tf.layers.dense(x, 1)` (and sums of such heads and of [B, 1] tensors) whose consumer is the loss of a TRAIN
    step: model_tail.finish_model_fn hands the un-evaluated sum to ONE kernel that computes the logit, the
    probabilities, the loss and the whole backward of this tail (ops.logit_loss).  Any other use goes through
    `materialize()`, i.e. the separate head kernel."""

    def __init__(self, heads=(), tensors=()):
        self.heads = list(heads)          # [(kernel Variable, bias Variable | None, [parts])]
        self.tensors = list(tensors)      # [B, 1] addends

    @property
    def shape(self):
        B = (self.heads[0][2][0] if self.heads else self.tensors[0]).shape[0]
        return (B, 1)

    def __add__(self, other):
        if isinstance(other, LazyLogit):
            return LazyLogit(self.heads + other.heads, self.tensors + other.tensors)
        if isinstance(other, torch.Tensor):
            return LazyLogit(self.heads, self.tensors + [other])
        return NotImplemented

    __radd__ = __add__

    def tail(self):
        """(side part | None, LazyDense, side_first) when this is ONE head over [side, last hidden layer] (either order) with
        nothing else added and the fused layer + head + loss kernel serves the shapes; else None."""
        from . import ops
        if len(self.heads) != 1 or self.tensors:
            return None
        kernel, _, parts = self.heads[0]
        lazies = [i for i, t in enumerate(parts) if isinstance(t, LazyDense)]
        if len(lazies) != 1 or len(parts) > 2 or hasattr(kernel, "apply_head"):
            return None
        ld = parts[lazies[0]]
        side = parts[1 - lazies[0]] if len(parts) == 2 else None
        if not ops.tail_dense_head_supported(ld.x, ld.shape[-1], side):
            return None
        return side, ld, lazies[0] == 1

    def resolve(self):
        """the un-evaluated last hidden layer (LazyDense), if any, run as an ordinary dense layer"""
        self.heads = [(k, b, [_resolved(t) for t in ps]) for k, b, ps in self.heads]
        return self

    def fusable(self) -> bool:
        from . import ops
        self.resolve()
        parts = [t for _, _, ps in self.heads for t in ps]
        return (len(self.heads) >= 1 and sum(b is not None for _, b, _ in self.heads) <= 1
                and ops.logit_loss_supported(parts, self.tensors))

    def materialize(self) -> torch.Tensor:
        store = current_store()
        out = None
        for kernel, bias, parts in self.resolve().heads:
            t = kernel.apply_head(parts) if hasattr(kernel, "apply_head") else _Dense1Fn.apply(store.anchor, kernel, bias, *parts)
            out = t if out is None else out + t
        for t in self.tensors:
            out = t if out is None else out + t
        return out


def concat(values, axis: int = -1):
    """tf.concat along the last axis; lazy (see LazyConcat) when every value is a 2-D device tensor."""
    values = [t.materialize() if isinstance(t, LazyTower) else t for t in values]
    if axis in (-1, values[0].dim() - 1) and len(values) <= 4 and all(t.dim() == 2 and t.is_cuda for t in values):
        return LazyConcat(values)
    return torch.cat([_resolved(t) for t in values], dim=axis)


def dense_drop_supported(x, units: int) -> bool:
    """dense(drop=) — the dropout behind a ReLU layer applied by the layer's own epilogue — is served for what the hand-written
    forward kernel serves: a 2-D fp32 device tensor of up to DENSE_MAX_K features, outside Sync-BatchNorm."""
    store = current_store()
    return (not store.building and isinstance(x, torch.Tensor) and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32
            and _mfma_dense(x.shape[1]) and int(units) % 4 == 0 and x.shape[0] * int(units) < (1 << 32)
            and getattr(getattr(store.anchor, "_recalgo_store", None), "sync_bn", None) is None)


def dense(x, units, activation: Optional[str] = None,
          use_bias: bool = True, name: Optional[str] = None, input_l2: float = 0.0,
          grad_join: Optional[GradJoin] = None, bn_stats: bool = False, drop=None, last_hidden: bool = False) -> torch.Tensor:
    """tf.layers.dense(x, units, activation=None|relu, use_bias, name).  `units` may be a
    str (the reference passes FLAGS.hidden_units.split(','), deepfm.py:286; quirk B-2).
    Variables: <scope>/<name>/kernel (glorot-uniform), <scope>/<name>/bias (zeros).
    `input_l2` = c (not a TF argument): the caller adds the loss term (c / 2) * sum(x^2) as a VALUE only
    (`l2_value`) and this layer adds its gradient c * x to the input gradient inside the dgrad GEMM
    (beta * C epilogue) — c must already contain the loss-gradient seed (ops.loss_seed).
    `bn_stats` (not a TF argument): a training-mode tf.layers.batch_normalization consumes this layer's output next (the
    dense -> [dropout] -> batch_norm order of deepfm.py:207-211): the GEMM's epilogue leaves the batch moments of its tiles
    and `batch_normalization` runs without a moments pass of its own (it finds them attached to the tensor it is given —
    a dropout in between makes a new tensor, and the BatchNorm layer computes its own moments as before).
    `last_hidden` (not a TF argument): this ReLU layer's output goes to the one-unit head in front of the loss (dcn.py:166-172);
    in a TRAIN step it is returned un-evaluated (LazyDense) for the fused layer + head + loss kernel."""
    store = current_store()
    units = int(units)
    if isinstance(x, LazyDense):
        x = x.materialize()
    name = name or store.auto_name("dense")
    with store.variable_scope(name):
        kernel = store.get_variable("kernel", (x.shape[-1], units), glorot_uniform)
        bias = store.get_variable("bias", (units,), zeros) if use_bias else None
    if activation not in (None, "relu"):
        raise ValueError(f"unsupported activation {activation}")
    if getattr(store, "serving", None) is not None or isinstance(x, LazyTower):
        tower = _serving_tower(store, x, units) if (activation == "relu" and input_l2 == 0.0 and not bn_stats and drop is None) else None
        if tower is not None:                 # a PREDICT capture of ServingModel.compile: the layer joins the one-launch tower
            return tower.with_layer(kernel, bias)
        x = _resolved(x)
    parts = x.parts if isinstance(x, LazyConcat) else [x]
    if units == 1 and activation is None:
        from . import ops
        parts = [t if (isinstance(t, LazyDense) or t.is_contiguous()) else t.contiguous() for t in parts]
        if any(isinstance(t, LazyDense) for t in parts):
            lazy = LazyLogit([(kernel, bias, parts)])
            if not store.building and lazy.tail() is not None:
                return lazy                                   # TRAIN step: layer + head + loss + their backward in one launch
            parts = lazy.resolve().heads[0][2]
        if ops.dense1_supported(parts):
            if ops.logit_loss_supported(parts, []) and not store.building:
                return LazyLogit([(kernel, bias, parts)])     # TRAIN step: evaluated together with the loss
            return _Dense1Fn.apply(store.anchor, kernel, bias, *parts)
        x = LazyConcat(parts) if isinstance(x, LazyConcat) else parts[0]
    if isinstance(x, LazyConcat):
        x = x.materialize()
    if (last_hidden and FUSED_TAIL and activation == "relu" and use_bias and not store.building and input_l2 == 0.0 and not bn_stats and drop is None
            and grad_join is None and isinstance(x, torch.Tensor) and getattr(x, "_recalgo_relu_src", None) is not None
            and getattr(x, "_recalgo_relu_scale", 1.0) == 1.0):
        from . import ops
        if ops.tail_dense_head_supported(x, units, None):
            return LazyDense(x, kernel, bias, grad_join)
    bn_part = None
    if (bn_stats and not store.building and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and units % 4 == 0
            and _mfma_dense(x.shape[1]) and getattr(getattr(store.anchor, "_recalgo_store", None), "sync_bn", None) is None):
        from . import ops
        bn_part = torch.empty(ops.bn_partial_rows(x.shape[0]), 2 * units, device=x.device, dtype=torch.float32)
    if drop is not None and (activation != "relu" or not dense_drop_supported(x, units)):
        raise ValueError("dense(drop=) needs activation='relu' and nn.dense_drop_supported(x, units)")
    relu_src = ReluSource() if (activation == "relu" and not store.building) else None
    out = _DenseFn.apply(store.anchor, x, kernel, bias, activation == "relu", input_l2, grad_join, bn_part, relu_src, drop)
    if bn_part is not None:
        out._recalgo_bn_partials = bn_part
    if relu_src is not None:
        out._recalgo_relu_src = relu_src
        if drop is not None:
            out._recalgo_relu_scale = float(drop.scale)      # (a consumer that masks its dx with this tensor also scales it)
    return out


def crossed_indicator_dense(features, feature_columns, units=1, name: Optional[str] = None, training: bool = False) -> torch.Tensor:
    """tf.layers.dense(fc.input_layer(features, [fc.indicator_column(fc.crossed_column([a, b], H))]), 1, name=name)
    (the reference's algorithm/WideAndDeep/wide_and_deep.py:208-210) as ONE launch that never builds the [B, H] multi-hot
    (wide.py, csrc/wide.hip).  Same scopes and variables as the two calls: the input layer takes its auto name (it owns no
    variable), the layer owns <scope>/<name>/kernel (H, 1) glorot-uniform and <scope>/<name>/bias (1,) zeros.  `training`:
    a TRAIN step — the requests are counted for the backward's plan; the kernel's gradient never becomes a dense tensor
    unless somebody reads it, and estimator.FtrlOptimizer updates the touched buckets in place."""
    from . import feature_column as fc
    from . import wide
    store = current_store()
    cols = list(feature_columns)
    if len(cols) != 1 or not fc.is_crossed_indicator(cols[0]) or int(units) != 1:
        raise NotImplementedError("crossed_indicator_dense: ONE indicator column over a crossed column, one unit")
    crossed = cols[0].categorical_column
    if getattr(store, "shard_at_build", None) is not None or getattr(store, "sync_bn", None) is not None:
        raise NotImplementedError(wide.NO_DATA_PARALLEL)
    store.auto_name("input_layer")
    name = name or store.auto_name("dense")
    with store.variable_scope(name):
        kernel = store.get_variable("kernel", (crossed.hash_bucket_size, 1), glorot_uniform)
        bias = store.get_variable("bias", (1,), zeros)
    B = fc._batch_size(features, crossed.keys[0])
    st = wide.states(store).get(kernel.name)
    if st is None:           # (made on the registration pass: a checkpoint restored right after it finds the layer)
        st = wide.states(store)[kernel.name] = wide.WideState(kernel, bias, crossed.hash_bucket_size, crossed.hash_key)
    if store.building:
        return torch.zeros(B, 1, device=store.device)
    users, tags, offsets = crossed.requests(features, store.device)
    return wide.cross_logit(store, st, users, tags, offsets, training=training)


def dense_relu_dropout_bn(x, units, dropout_rate, batch_norm: bool, training: bool) -> torch.Tensor:
    """One hidden layer of the DeepFM / PNN / FiBiNET / NFM MLPs (/root/reference algorithm/DeepFM/deepfm.py:207-211):
        net = tf.layers.dense(net, unit, activation=tf.nn.relu)
        if "dropout_rate" in params and 0.0 < params["dropout_rate"] < 1.0: net = tf.layers.dropout(net, rate, training=...)
        if params["batch_norm"]: net = tf.layers.batch_normalization(net, training=...)
    Same variables, scopes and arithmetic as the three calls.  In a training step with both the dropout and the BatchNorm on,
    the dropout costs no launch: the dense layer's epilogue applies it (and leaves the BatchNorm's tile moments of the DROPPED
    tensor), and the BatchNorm's backward — which masks its input gradient with that tensor anyway — scales it by 1 / (1 - rate)."""
    rate = float(dropout_rate) if dropout_rate is not None else 0.0
    drop_on = bool(training) and 0.0 < rate < 1.0
    if drop_on and batch_norm and isinstance(x, torch.Tensor) and dense_drop_supported(x, units):
        d = drop_spec((x.shape[0], int(units)), rate, x.device)
        net = dense(x, units, activation="relu", bn_stats=True, drop=d)
        return batch_normalization(net, training=True)
    net = dense(x, units, activation="relu", bn_stats=bool(batch_norm) and bool(training) and not drop_on)
    if 0.0 < rate < 1.0:
        net = dropout(net, rate, training=training)
    if batch_norm:
        net = batch_normalization(net, training=training)
    return net


class InputGradChain:
    """A tensor that feeds the MMoE gates AND the E expert layers (mmoe.py:197-215) receives the sum of 1 + E input
    gradients.  Shared by `gate_mix` and `expert_layers`: the gates' backward (it runs first: it consumes the experts)
    offers its share here instead of returning it, and the expert layers add theirs one after the other through the beta * C
    epilogue of their input-gradient GEMM (ops.dense_bwd c_in) and return the total — no elementwise add launches.  Made per
    model_fn invocation, so an abandoned backward leaves nothing behind.
    An offer is accepted only when a consumer that WILL return the input gradient has registered in its forward
    (`expert_layers` over an input that needs a gradient, called before `gate_mix`): otherwise the gates return their share to
    autograd as any op does, and nothing can be dropped."""

    def __init__(self):
        self.first: Optional[torch.Tensor] = None
        self.closed = False
        self.consumers = 0

    def register_consumer(self) -> None:
        self.consumers += 1

    def offer(self, dx: torch.Tensor) -> bool:
        if self.consumers == 0 or self.closed or self.first is not None:
            return False
        self.first = dx
        return True

    def take(self) -> Optional[torch.Tensor]:
        t, self.first, self.closed = self.first, None, True
        return t


class _ExpertsFn(Function):
    """E sibling tf.layers.dense(x, units, relu) over ONE input as one autograd node: E GEMM launches each way; the input
    gradients are chained through the dgrad GEMM's beta * C term, starting with what the InputGradChain holds."""

    @staticmethod
    def forward(ctx, anchor, x, chain: Optional[InputGradChain], srcs, *kb):
        from . import ops
        ctx.set_materialize_grads(False)
        x2 = x if x.stride(1) == 1 else x.contiguous()
        ks, bs = kb[0::2], kb[1::2]
        ys = [ops.dense_fwd(x2, k.data, b.data, True) for k, b in zip(ks, bs)]
        ctx.vars, ctx.chain, ctx.srcs = (ks, bs), chain, srcs
        if chain is not None and ctx.needs_input_grad[1]:
            chain.register_consumer()        # (this node's backward returns d x: it takes what the chain holds)
        else:
            ctx.chain = None
        ctx.save_for_backward(x2, *ys)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gs):
        from . import ops
        x2, *ys = ctx.saved_tensors
        ks, bs = ctx.vars
        need_x = ctx.needs_input_grad[1]
        dx = ctx.chain.take() if ctx.chain is not None else None
        if dx is not None and (tuple(dx.shape) != tuple(x2.shape) or dx.stride(1) != 1):
            raise ValueError("expert_layers: the chained input gradient does not have the input's shape")
        for k, b, y, g, src in zip(ks, bs, ys, gs, ctx.srcs):
            if g is None:
                continue
            g2 = ops._contig(g)
            mask = None if src.take(g2) else y       # (ops.gate_mix masked the gradient it wrote: nn.ReluSource)
            if need_x:
                dx = ops.dense_bwd(x2, g2, mask, k.data, k.grad, b.grad, c_in=dx, beta=0.0 if dx is None else 1.0, defer=True,
                                   cross_rider=False)
            else:
                ops.dense_bwd_weights(x2, g2, mask, k.grad, b.grad, defer=True)
        return (None, dx if need_x else None, None, None) + (None,) * (2 * len(ks))


def expert_layers(x: torch.Tensor, units, num_experts: int, chain: Optional[InputGradChain] = None, names=None):
    """[tf.layers.dense(x, units, activation=tf.nn.relu, name=f"expert_{i}") for i in range(num_experts)] (mmoe.py:199-202):
    variables <scope>/expert_<i>/{kernel,bias}, or <scope>/<names[i]>/{kernel,bias} when `names` lists the num_experts layer
    names (PLE's shared_expert_<j> / task_specific_expert_<task>_<j>: ONE call — one autograd node, one input-gradient chain —
    over all the experts of a block).  -> the list of expert outputs [B, units]."""
    store = current_store()
    units = int(units)
    names = [f"expert_{i}" for i in range(int(num_experts))] if names is None else [str(n) for n in names]
    if len(names) != int(num_experts) or len(set(names)) != len(names):
        raise ValueError("expert_layers: `names` must list num_experts distinct layer names")
    kb = []
    for name in names:
        with store.variable_scope(name):
            kb.append(store.get_variable("kernel", (x.shape[-1], units), glorot_uniform))
            kb.append(store.get_variable("bias", (units,), zeros))
    if store.building:
        return [x.new_zeros(x.shape[0], units) for _ in range(int(num_experts))]
    if not (x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and _mfma_dense(x.shape[1])):
        raise NotImplementedError("expert_layers: a 2-D fp32 device input of up to DENSE_MAX_K features")
    srcs = [ReluSource() for _ in range(int(num_experts))]
    outs = list(_ExpertsFn.apply(store.anchor, x, chain, srcs, *kb))
    for o, src in zip(outs, srcs):
        o._recalgo_relu_src = src
    return outs


def gate_mix(x: torch.Tensor, experts, num_gates: int, selection=None, chain: Optional[InputGradChain] = None):
    """The `gates` scope and the per-task mix of mmoe.py:208-232: num_gates bias-free softmax gates
    tf.layers.dense(x, n_g, activation=tf.nn.softmax, use_bias=False, name=f"gate_{i}") and, per gate,
    tf.squeeze(tf.matmul(experts, gate[..., None], transpose_a=True), -1) — one kernel each way (ops.gate_mix).
    Variables: <scope>/gate_<i>/kernel.  -> (the num_gates mixed tensors [B, H], the gate probabilities [B, sum n_g])."""
    from . import ops
    store = current_store()
    experts = list(experts)
    E = len(experts)
    selection = [list(range(E)) for _ in range(int(num_gates))] if selection is None else [list(s) for s in selection]
    kernels = []
    for i, sel in enumerate(selection):
        with store.variable_scope(f"gate_{i}"):
            kernels.append(store.get_variable("kernel", (x.shape[-1], len(sel)), glorot_uniform))
    if store.building:
        return [torch.zeros_like(experts[0]) for _ in selection], x.new_zeros(x.shape[0], sum(len(s) for s in selection))
    return ops.gate_mix(x if x.stride(-1) == 1 else x.contiguous(), kernels, experts, selection, x_grad_sink=chain,
                        anchor=store.anchor, return_gates=True)


def cgc_layer(x: torch.Tensor, experts, gate_names, selection, sum_outputs: bool = False,
              chain: Optional[InputGradChain] = None):
    """The gates and the mix of a PLE "customized gate control" block (extraction_network.py:55-85, ple.py:215-226): per
    named gate tf.layers.dense(x, n_g, activation=tf.nn.softmax, use_bias=False, name=<gate_name>) over the experts
    selection[g], mixed by tf.matmul(experts, gate[..., None], transpose_a=True) — one kernel each way (ops.cgc_mix).
    Variables: <scope>/<gate_name>/kernel (a gate name may carry a scope of its own: "task_gate_final/gate_final_like").
    -> the per-gate mixed tensors [B, H]; with sum_outputs their tf.add_n as ONE tensor."""
    from . import ops
    store = current_store()
    experts, selection = list(experts), [list(s) for s in selection]
    if len(gate_names) != len(selection):
        raise ValueError("cgc_layer: one gate name per selection row")
    kernels = []
    for name, sel in zip(gate_names, selection):
        with store.variable_scope(name):
            kernels.append(store.get_variable("kernel", (x.shape[-1], len(sel)), glorot_uniform))
    if store.building:
        return torch.zeros_like(experts[0]) if sum_outputs else [torch.zeros_like(experts[0]) for _ in selection]
    return ops.cgc_mix(x if x.stride(-1) == 1 else x.contiguous(), kernels, experts, selection, sum_outputs=sum_outputs,
                       x_grad_sink=chain, anchor=store.anchor)


def dense_with(x: torch.Tensor, kernel: Variable, bias: Optional[Variable] = None, relu: bool = False) -> torch.Tensor:
    """tf.matmul(x, kernel) (+ bias) (+ relu) on variables the model created itself with tf.get_variable (AFM's attention
    network, afm.py:168-190): the same kernels as `dense` (one-unit outputs go through the head kernel)."""
    store = current_store()
    if kernel.data.shape[1] == 1 and not relu:
        from . import ops
        xc = ops._contig(x)
        if ops.dense1_supported([xc]):
            return _Dense1Fn.apply(store.anchor, kernel, bias, xc)
    return _DenseFn.apply(store.anchor, x, kernel, bias, relu, 0.0, None)


def l2_value(x: torch.Tensor, half_coeff: float) -> torch.Tensor:
    """half_coeff * sum(x^2) as a detached scalar (its gradient is taken care of by `dense(input_l2=)`)."""
    with torch.no_grad():
        v = x.reshape(-1)
        return torch.dot(v, v) * half_coeff


class _BatchNormTrainFn(Function):
    @staticmethod
    def forward(ctx, anchor, x, gamma: Variable, beta: Variable, mmean: Variable, mvar: Variable,
                momentum: float, eps: float, partials: Optional[torch.Tensor] = None):
        ctx.vars = (gamma, beta)
        ctx.hip = x.dim() == 2 and x.is_contiguous() and _hip(x, x.shape[1])
        ctx.x_relu_src = getattr(x, "_recalgo_relu_src", None) if ctx.hip else None
        ctx.x_relu_scale = float(getattr(x, "_recalgo_relu_scale", 1.0)) if ctx.x_relu_src is not None else 1.0
        # Sync-BatchNorm (parallel.attach_data_parallel(sync_batch_norm=True)): statistics over the GLOBAL batch
        ctx.sync = getattr(getattr(anchor, "_recalgo_store", None), "sync_bn", None)
        if ctx.sync is not None and not ctx.hip:
            raise NotImplementedError("sync_batch_norm needs the HIP BatchNorm kernels (2-D contiguous input, C % 4 == 0)")
        if ctx.hip:
            from . import ops
            if ctx.sync is not None:
                y, mean, rstd = ops.batchnorm_sync_fwd(x, gamma.data, beta.data, mmean.data, mvar.data, momentum, eps, ctx.sync)
            else:
                y, mean, rstd = ops.batchnorm_train_fwd(x, gamma.data, beta.data, mmean.data, mvar.data, momentum, eps,
                                                        partials=partials)
                ctx.link = BNLink(x, mean, rstd)       # (attached to the output by batch_normalization())
            ctx.save_for_backward(x, mean, rstd)
            return y
        mean = x.mean(dim=0)
        xc = x - mean
        var = (xc * xc).mean(dim=0)            # biased, tf.nn.moments
        rstd = torch.rsqrt(var + eps)
        xhat = xc * rstd
        y = xhat * gamma.data + beta.data
        # moving stats: assign_moving_average, decay = momentum (TF default 0.99)
        mmean.data.mul_(momentum).add_(mean, alpha=1 - momentum)
        mvar.data.mul_(momentum).add_(var, alpha=1 - momentum)
        ctx.save_for_backward(xhat, rstd)
        return y

    @staticmethod
    def backward(ctx, g):
        gamma, beta = ctx.vars
        if ctx.hip:
            from . import ops
            x, mean, rstd = ctx.saved_tensors
            if ctx.sync is not None:
                dx = ops.batchnorm_sync_bwd(x, gamma.data, mean, rstd, g.contiguous(), gamma.grad, beta.grad, ctx.sync)
            else:
                # x is the ReLU output of a dense layer: this kernel masks the gradient it writes (it reads x anyway) and that
                # layer's backward runs without mask loads (ReluSource)
                src = ctx.x_relu_src
                dx = ops.batchnorm_train_bwd(x, gamma.data, mean, rstd, g.contiguous(), gamma.grad, beta.grad,
                                             sums=ctx.link.take(g), relu_x=src is not None, relu_scale=ctx.x_relu_scale)
                if src is not None:
                    src.premasked = dx
            return None, dx, None, None, None, None, None, None, None, None
        xhat, rstd = ctx.saved_tensors
        B = g.shape[0]
        dbeta = g.sum(dim=0)
        dgamma = (g * xhat).sum(dim=0)
        gamma.grad.copy_(dgamma)
        beta.grad.copy_(dbeta)
        dx = (gamma.data * rstd / B) * (B * g - dbeta - xhat * dgamma)
        return None, dx, None, None, None, None, None, None, None, None


class _BatchNormInferFn(Function):
    @staticmethod
    def forward(ctx, x, scale, shift):
        ctx.save_for_backward(scale)
        return x * scale + shift

    @staticmethod
    def backward(ctx, g):
        (scale,) = ctx.saved_tensors
        return g * scale, None, None


BN_EPSILON = 1e-3        # tf.layers.batch_normalization's default, which every model_fn here leaves alone


def fold_batch_norm(gamma: torch.Tensor, beta: torch.Tensor, moving_mean: torch.Tensor, moving_variance: torch.Tensor,
                    epsilon: float = BN_EPSILON):
    """BatchNorm inference as one multiply-add per column -> (scale, shift): y = x * scale + shift with
    scale = gamma * rsqrt(moving_variance + epsilon), shift = beta - moving_mean * scale.  Pure: any dtype, any device."""
    scale = torch.rsqrt(moving_variance + epsilon) * gamma
    return scale, beta - moving_mean * scale


def batch_normalization(x: torch.Tensor, training: bool = False,
                        momentum: float = 0.99, epsilon: float = BN_EPSILON,
                        name: Optional[str] = None) -> torch.Tensor:
    """tf.layers.batch_normalization on (B, C)."""
    store = current_store()
    name = name or store.auto_name("batch_normalization")
    C = x.shape[-1]
    with store.variable_scope(name):
        gamma = store.get_variable("gamma", (C,), ones)
        beta = store.get_variable("beta", (C,), zeros)
        mmean = store.get_variable("moving_mean", (C,), zeros, trainable=False)
        mvar = store.get_variable("moving_variance", (C,), ones, trainable=False)
    if isinstance(x, LazyTower):
        plan = getattr(store, "serving", None)
        fold = plan.folds.get(gamma.name) if (plan is not None and not training and plan.epsilon == epsilon) else None
        if fold is not None and x._out is None and x.layers[-1][2] is None:
            return x.with_fold(*fold)         # the last layer's epilogue applies it
        x = x.materialize()
    if training:
        # (batch moments left behind by the producing dense layer's epilogue, see dense(bn_stats=))
        pre = getattr(x, "_recalgo_bn_partials", None) if (x.dim() == 2 and x.is_contiguous()) else None
        return _attach_link(_BatchNormTrainFn.apply(store.anchor, x, gamma, beta, mmean, mvar, momentum, epsilon, pre))
    return _BatchNormInferFn.apply(x, *fold_batch_norm(gamma.data, beta.data, mmean.data, mvar.data, epsilon))


class _DenseActBNFn(Function):
    """dense -> prelu | dice -> batch_normalization(training=True) as five launches instead of nine: the GEMM's epilogue applies
    the activation and leaves the BatchNorm tile moments (ops.dense_fwd_act), the BatchNorm backward continues through the
    activation (ops.batchnorm_train_bwd_act); same arithmetic per element as the three layers one after the other."""

    @staticmethod
    def forward(ctx, anchor, x, kernel: Variable, bias: Variable, alpha: Variable, kind: int, gamma: Variable, beta: Variable,
                mmean: Variable, mvar: Variable, momentum: float, eps: float, input_l2: float, drop=None):
        from . import ops
        x2 = x if x.stride(1) == 1 else x.contiguous()
        M, N = x2.shape[0], kernel.data.shape[1]
        partials = torch.empty(ops.bn_partial_rows(M), 2 * N, device=x.device, dtype=torch.float32)
        z, y = ops.dense_fwd_act(x2, kernel.data, bias.data, kind, alpha.data, partials)
        # drop: the tf.layers.dropout BEHIND the BatchNorm (din.py:233-236) rides in the BatchNorm's store, and in the loads of its backward
        out, mean, rstd = ops.batchnorm_train_fwd(y, gamma.data, beta.data, mmean.data, mvar.data, momentum, eps, partials=partials,
                                                  out_drop=drop)
        ctx.drop = drop
        # (the next dense layer's backward may leave this BN's sums, see _attach_link — not behind a dropout: they would be sums of
        # the un-dropped gradient)
        ctx.link = BNLink(y, mean, rstd) if drop is None else None
        ctx.in_link = _bn_link_of(x)                                 # (... and this one's those of the BatchNorm before it)
        ctx.vars, ctx.kind, ctx.input_l2 = (kernel, bias, alpha, gamma, beta), kind, float(input_l2)
        ctx.in_step = ops._loss_seed is not None      # Estimator.train_step: its optimizer runs the deferred column sums
        ctx.save_for_backward(x2, z, y, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import ops
        kernel, bias, alpha, gamma, beta = ctx.vars
        x2, z, y, mean, rstd = ctx.saved_tensors
        dz = ops.batchnorm_train_bwd_act(y, gamma.data, mean, rstd, g.contiguous(), gamma.grad, beta.grad, ctx.kind, z, alpha.data,
                                         alpha.grad, defer=ctx.in_step, sums=None if ctx.link is None else ctx.link.take(g),
                                         g_drop=ctx.drop)
        dx = None
        if ctx.needs_input_grad[1]:
            link = ctx.in_link
            dx = ops.dense_bwd(x2, dz, None, kernel.data, kernel.grad, bias.grad, c_in=x2 if ctx.input_l2 else None,
                               beta=ctx.input_l2, defer=True,
                               bn=None if link is None else (link.x, link.mean, link.rstd, link.new_sums()))
            if link is not None:
                link.grad_ptr = dx.data_ptr()
        else:
            ops.dense_bwd_weights(x2, dz, None, kernel.grad, bias.grad, defer=True)
        return (None, dx) + (None,) * 12


def dense_activation_bn(x: torch.Tensor, units, kind: str, act_name, batch_norm: bool, training: bool,
                        input_l2: float = 0.0, momentum: float = 0.99, epsilon: float = 1e-3, dropout_rate=None) -> torch.Tensor:
    """One hidden layer of DIN's `fcn` scope (/root/reference algorithm/DIN/din.py:227-236):
        net = tf.layers.dense(net, units, activation=None); net = dice | prelu (net, name=act_name)
        if batch_norm: net = tf.layers.batch_normalization(net, training=training)
        if "dropout_rate" in params and 0.0 < rate < 1.0: net = tf.layers.dropout(net, rate, training=training)   (dropout_rate=)
    Variables, scopes and arithmetic are those of the calls; in a training step on the GPU they run as ONE autograd node
    (_DenseActBNFn: the dropout in the BatchNorm's store and in the loads of its backward), otherwise as the separate layers."""
    rate = float(dropout_rate) if dropout_rate is not None else 0.0
    drop_on = bool(training) and 0.0 < rate < 1.0
    from . import ops
    store = current_store()
    units = int(units)
    dname = store.auto_name("dense")
    fused = bool(batch_norm and training and not store.building and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32
                 and units % 4 == 0 and _mfma_dense(x.shape[1]) and torch.is_grad_enabled()
                 and getattr(getattr(store.anchor, "_recalgo_store", None), "sync_bn", None) is None)
    if not fused:
        net = dense(x, units, activation=None, name=dname, input_l2=input_l2)
        alpha = store.get_variable(f"{kind}_alpha_{act_name}", (units,), ones)
        net = ops.activation(store, net, alpha, kind)
        net = batch_normalization(net, training=training, momentum=momentum, epsilon=epsilon) if batch_norm else net
        return dropout(net, rate, training=training) if 0.0 < rate < 1.0 else net
    with store.variable_scope(dname):
        kernel = store.get_variable("kernel", (x.shape[-1], units), glorot_uniform)
        bias = store.get_variable("bias", (units,), zeros)
    alpha = store.get_variable(f"{kind}_alpha_{act_name}", (units,), ones)
    with store.variable_scope(store.auto_name("batch_normalization")):
        gamma = store.get_variable("gamma", (units,), ones)
        beta = store.get_variable("beta", (units,), zeros)
        mmean = store.get_variable("moving_mean", (units,), zeros, trainable=False)
        mvar = store.get_variable("moving_variance", (units,), ones, trainable=False)
    d = drop_spec((x.shape[0], units), rate, x.device) if (drop_on and x.shape[0] * units < (1 << 32)) else None
    out = _attach_link(_DenseActBNFn.apply(store.anchor, x, kernel, bias, alpha, ops._ACT[kind], gamma, beta, mmean, mvar, momentum,
                                           epsilon, input_l2, d))
    return dropout(out, rate, training=training) if (drop_on and d is None) else out


DROPOUT_KEEP_MASKS: list = []      # test hook: keep masks consumed (FIFO) by the next training-mode dropout calls
DROPOUT_SPECS: list = []           # test hook: when not None, every training-mode dropout call appends its ops.DropSpec


def drop_spec(x_shape, rate: float, device):
    """The ops.DropSpec of the next training-mode dropout call of the current model_fn invocation: an injected keep mask
    (DROPOUT_KEEP_MASKS), else the hash stream (store seed + rank, call index, the optimizer's device step counter)."""
    from . import ops
    store = current_store()
    call = store._drop_calls
    store._drop_calls += 1
    mask = None
    if DROPOUT_KEEP_MASKS:
        mask = DROPOUT_KEEP_MASKS.pop(0).to(device=device, dtype=torch.float32).reshape(tuple(x_shape)).contiguous()
    rank = 0                       # (data parallel: every rank drops its own slice of the global batch with its own stream)
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            rank = dist.get_rank()
    except Exception:
        pass
    d = ops.DropSpec(rate, mask, store.seed * 1000003 + 7919 * rank, call, store.ensure_opt_state()["step"])
    if DROPOUT_SPECS is not None:
        DROPOUT_SPECS.append(d)
        del DROPOUT_SPECS[:-64]
    return d


def dropout(x: torch.Tensor, rate: float, training: bool = False) -> torch.Tensor:
    """tf.layers.dropout: keep prob 1-rate, scaled by 1/(1-rate); identity when not training.  TF's random stream
    cannot be reproduced: parity tests inject the keep mask the golden recorded through DROPOUT_KEEP_MASKS; otherwise the
    keep decisions are the counter-based hash of csrc/dropout.h (a new mask per optimizer step, also under hipGraph replay)."""
    if not training or rate <= 0.0:
        return x
    store = current_store()
    if store.building:
        return x
    from . import ops
    return ops.dropout(x, drop_spec(x.shape, rate, x.device))


class _L2RegFn(Function):
    @staticmethod
    def forward(ctx, anchor, scale: float, variables):
        ctx.scale, ctx.vars = scale, variables
        return sum((v.data * v.data).sum() for v in variables) * (0.5 * scale)

    @staticmethod
    def backward(ctx, g):
        # runs before the kernels that OVERWRITE these variables' grads?  No: the parameter-owning
        # ops overwrite .grad during their own backward, in autograd order.  To be order independent
        # the regulariser's contribution is parked and added by `apply_parked_grads` (called by the
        # optimizer before the update).
        from . import ops
        ops._parked_l2.extend((v, ctx.scale, g) for v in ctx.vars)
        return None, None, None


def apply_parked_grads(step_dev=None):
    """Finish the gradients that backward left parked (called once per step, after backward, by the optimizer and by
    `variables.named_grads`): the deferred weight-gradient split sums of `dense` (ops.flush_dense_splits), then
    grad += scale * g * w for every parked l2 term."""
    from . import ops
    ops.flush_dense_splits(step_dev)
    while ops._parked_l2:
        v, scale, g = ops._parked_l2.pop()
        v.grad.add_(v.data * (scale * g))


def l2_regularization(scale: float, variables) -> torch.Tensor:
    """sum_v tf.contrib.layers.l2_regularizer(scale)(v) = scale * sum(v^2) / 2."""
    return _L2RegFn.apply(current_store().anchor, float(scale), tuple(variables))


def bst_transformer(queries: torch.Tensor, keys_length: torch.Tensor, heads: int, index: int, max_length: int,
                    pool: Optional[str] = None):
    """algorithm/BST/transformer_layer.py bst_transformer(queries, queries, queries, keys_length, heads, index, max_length) on
    the two fused kernels of csrc/bst.hip per direction.  Variables under the caller's scope, the reference's names:
    position_embedding [max_length, d] (ONE table for every block of the scope: each block adds it again, its gradient is the
    sum over the blocks), w_q_<index> / w_k_<index> / w_v_<index> [heads, d, d], w_o_<index> [heads * d, d] (glorot-uniform,
    tf.get_variable's default), LayerNorm[_n]/{gamma, beta} twice (tf.contrib.layers.layer_norm's auto names: ones, zeros),
    dense[_n]/{kernel, bias} (tf.layers.dense).
    queries [B, T, d] (row 0 the target, padded rows zero), keys_length [B] = history length + 1.
    pool=None -> the block's output [B, T, d], to chain into the next block; pool='sum' | 'mean' -> [B, d], the reduction over
    ALL T rows (bst.py:195-198) fused into the block's last kernel.  Sizes the kernels do not serve raise ValueError."""
    from . import ops
    store = current_store()
    B, T, d = queries.shape
    heads, max_length = int(heads), int(max_length)
    if T > max_length:
        raise ValueError(f"bst_transformer: {T} rows but position_embedding has max_length={max_length}")
    pos = store.get_variable("position_embedding", (max_length, d), glorot_uniform)
    w_q, w_k, w_v = (store.get_variable(f"w_{n}_{index}", (heads, d, d), glorot_uniform) for n in ("q", "k", "v"))
    w_o = store.get_variable(f"w_o_{index}", (heads * d, d), glorot_uniform)

    def layer_norm_variables():
        with store.variable_scope(store.auto_name("LayerNorm")):
            return store.get_variable("gamma", (d,), ones), store.get_variable("beta", (d,), zeros)
    norm1 = layer_norm_variables()               # (creation order of transformer_layer.py:72-79: LayerNorm, dense, LayerNorm_1)
    with store.variable_scope(store.auto_name("dense")):
        ffn_w = store.get_variable("kernel", (d, d), glorot_uniform)
        ffn_b = store.get_variable("bias", (d,), zeros)
    norms = [norm1, layer_norm_variables()]
    if pool not in (None, "sum", "mean"):
        raise ValueError(f"bst_transformer: pool={pool!r}")
    if not ops.bst_supported(T, d, heads):
        raise ValueError(f"bst_transformer: T={T} d={d} heads={heads} is outside what the BST kernels serve (1 <= T <= "
                         f"{ops.BST_MAX_T}, d in (4, 8, 12, 16), heads <= {ops.BST_MAX_HEADS}); there is no fallback")
    if store.building:
        return queries.new_zeros((B, T, d) if pool is None else (B, d))
    n1 = ops.bst_attention(ops._contig(queries), keys_length, pos, w_q, w_k, w_v, w_o, *norms[0], anchor=store.anchor)
    out, pooled = ops.bst_ffn(n1, ffn_w, ffn_b, *norms[1], pool=pool, want_out=pool is None, anchor=store.anchor)
    return out if pool is None else pooled


def _gru_cell_variables(store, nx: int, nh: int):
    """TF 1.14 GRUCell's four variables under the current scope: gates/{kernel [nx + nh, 2 nh], bias = 1},
    candidate/{kernel [nx + nh, nh], bias = 0}, kernels glorot-uniform (the variable scope's default initializer)."""
    with store.variable_scope("gates"):
        wg, bg = store.get_variable("kernel", (nx + nh, 2 * nh), glorot_uniform), store.get_variable("bias", (2 * nh,), ones)
    with store.variable_scope("candidate"):
        wc, bc = store.get_variable("kernel", (nx + nh, nh), glorot_uniform), store.get_variable("bias", (nh,), zeros)
    return wg, bg, wc, bc


def _dien_served(what: str, T: int, na: int, nh: int):
    from . import ops
    if not ops.dien_supported(T, na, nh):
        raise ValueError(f"{what}: T={T} na={na} nh={nh} is outside what the DIEN kernels serve (1 <= T <= {ops.DIEN_MAX_T}, an "
                         f"input width in (4, 8, 12, 16), a state width in (4, 8, 12, 16)); there is no fallback")


def dien_gru(inputs: torch.Tensor, sequence_length: Optional[torch.Tensor], num_units: int) -> torch.Tensor:
    """dynamic_rnn(GRUCell(num_units), inputs) of algorithm/DIEN/dien.py:202 on csrc/dien.hip: inputs [B, T, na] -> the
    outputs [B, T, nh], rows t >= sequence_length zero (None: all T steps run, as the reference calls it).  Variables under the
    caller's scope, TF's names: rnn/gru_cell/{gates, candidate}/{kernel, bias}."""
    from . import ops
    store = current_store()
    B, T, na = inputs.shape
    nh = int(num_units)
    with store.variable_scope("rnn"), store.variable_scope("gru_cell"):
        cell = _gru_cell_variables(store, na, nh)
    _dien_served("dien_gru", T, na, nh)
    if store.building:
        return inputs.new_zeros((B, T, nh))
    return ops.dien_gru(ops._contig(inputs), sequence_length, *cell, anchor=store.anchor)


def dien_evolve(h: torch.Tensor, target: torch.Tensor, sequence_length: torch.Tensor, custom_gru_type: str = "AGRU",
                return_states: bool = False):
    """algorithm/DIEN/dien.py:205-229 as one launch each way: the attention of `target` [B, na] over the rows of h [B, T, nh]
    (scores past sequence_length replaced by -2^32, softmax over all T) and dynamic_rnn(AGRUCell | AUGRUCell, h, scores,
    sequence_length) -> (final state [B, nh], attention scores [B, T]), with return_states also the cell's outputs [B, T, nh]
    (neither the scores nor the outputs carry a gradient).  Variables under the caller's scope:
    attention_project_matrix [nh, na], and rnn/{gates, candidate}/{kernel, bias} — the custom cells override __call__, so
    there is no cell-name scope, and the second dynamic_rnn re-enters the scope `rnn`."""
    from . import ops
    store = current_store()
    B, T, nh = h.shape
    na = int(target.shape[1])
    if custom_gru_type not in ops.DIEN_MODES:
        raise ValueError(f"dien_evolve: custom_gru_type={custom_gru_type!r}, expected one of {sorted(ops.DIEN_MODES)}")
    w_att = store.get_variable("attention_project_matrix", (nh, na), glorot_uniform)
    with store.variable_scope("rnn"):
        cell = _gru_cell_variables(store, nh, nh)
    _dien_served("dien_evolve", T, na, nh)
    if store.building:
        outs = (h.new_zeros((B, nh)), h.new_zeros((B, T)), h.new_zeros((B, T, nh)))
    else:
        outs = ops.dien_evolve(ops._contig(h), ops._contig(target), sequence_length, w_att, *cell, mode=custom_gru_type, anchor=store.anchor)
    return outs if return_states else outs[:2]


# ---- fused=: a layer on its fused kernels (True), composed from other ops (False), or whichever its default says (None) -----------
def _fp32_matrix_on_device(x) -> bool:
    """an fp32 2-D device tensor: what the kernels of every layer with a fused= argument read"""
    return isinstance(x, torch.Tensor) and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32


def _resolve_fused(fused: Optional[bool], served: bool, default: bool, refusal: Optional[str]) -> bool:
    """A layer's fused= argument -> whether this call runs the kernels.  served: whether they serve this call; default: what
    None picks; refusal: the ValueError of fused=True where they do not serve (None: the op itself refuses)."""
    if fused is None:
        return bool(default)
    if fused and not served and refusal is not None:
        raise ValueError(refusal)
    return bool(fused)


# From this width on nn.residual_stack runs the composed dense layers by default; below it the fused kernels of
# csrc/residual.hip.  The choice is a function of the shape alone (residual_fused_default): one path trains, evaluates and serves
# a model.  scripts/bench_deepcrossing.py (profiles/deepcrossing_bench.json, B = 4096, H = 128; DESIGN.md §5 "DeepCrossing
# residual stack"), fused against composed, forward + backward with the weight gradients, 1 unit / 3 units:
#   D = 82: 0.94 x / 1.03 x      D = 128: 0.80 x / 0.89 x      D = 256: 0.71 x / 0.76 x      D = 432: 0.63 x / 0.68 x
# At the measured widths from 128 on the composed layers are faster at both depths and are the default.  At D = 82, the
# reference's width, the two are within 6 % of each other and the fused path is the default because it is the one that meets the
# strict parity rule on both committed goldens (the composed layers leave 28 elements of one kernel gradient of the three-unit
# golden outside it, limit 24).  Widths between 82 and 128 were not measured; they go with 82.
RESIDUAL_COMPOSED_FROM_D = 128


def residual_fused_default(D: int, H: int, L: int) -> bool:
    """Whether residual_stack(fused=None) runs a [*, D] stack of L units of internal width H on the fused kernels."""
    from . import ops
    return L >= 1 and D < RESIDUAL_COMPOSED_FROM_D and ops.residual_supported(D, H, L)


def residual_stack(x: torch.Tensor, internal_dim: int, num_units: int, first_index: int = 0,
                   fused: Optional[bool] = None) -> torch.Tensor:
    """algorithm/DeepCrossing/deepcrossing.py:154-157: `num_units` residual units (residual_unit.py:4-22) chained,
        h = tf.layers.dense(x, internal_dim, name="dense_<i>_0", activation=relu)
        x = relu(x + tf.layers.dense(h, D, name="dense_<i>_1"))                      i = first_index, first_index + 1, ..
    Variables under the caller's scope, the reference's names: dense_<i>_0/{kernel [D, internal_dim], bias},
    dense_<i>_1/{kernel [internal_dim, D], bias} (glorot-uniform, zeros); both paths own the same ones.
    fused=None (not a reference argument): the whole stack as ONE launch each way (ops.residual_stack) where
    residual_fused_default(D, internal_dim, num_units) says so, else the same arithmetic as two `dense` layers and an
    add + ReLU per unit (internal_dim % 16 != 0, wide stacks, more than 8 units, a CPU tensor).  fused=True / False: that
    path; True where csrc/residual.hip does not serve the sizes is a ValueError."""
    from . import ops
    store = current_store()
    D, H, L = int(x.shape[-1]), int(internal_dim), int(num_units)
    on_device = store.device.type == "cuda" and (x.dim() == 2 if store.building else _fp32_matrix_on_device(x))
    fused = _resolve_fused(fused, on_device and L >= 1 and ops.residual_supported(D, H, L), on_device and residual_fused_default(D, H, L),
                           f"residual_stack(fused=True): the kernels do not serve D={D} H={H} units={L} on {store.device}")
    if not fused:
        for i in range(first_index, first_index + L):
            h = dense(x, H, activation="relu", name=f"dense_{i}_0")
            x = torch.relu(x + dense(h, D, activation=None, name=f"dense_{i}_1"))
        return x
    params = ([], [], [], [])                # W0, b0, W1, b1 of every unit, created in the reference's order
    for i in range(first_index, first_index + L):
        for j, shape in enumerate(((D, H), (H, D))):
            with store.variable_scope(f"dense_{i}_{j}"):
                params[2 * j].append(store.get_variable("kernel", shape, glorot_uniform))
                params[2 * j + 1].append(store.get_variable("bias", shape[1:], zeros))
    if store.building:
        return torch.zeros_like(x)
    return ops.residual_stack(ops._contig(x), *params, anchor=store.anchor)


def residual_unit(x: torch.Tensor, internal_dim: int, index: int, fused: Optional[bool] = None) -> torch.Tensor:
    """One residual unit (residual_unit.py:4-22) with the variables dense_<index>_0 / dense_<index>_1: the one-unit stack."""
    return residual_stack(x, internal_dim, 1, first_index=index, fused=fused)


# ---- AFM's attention network (afm.py:162-188) ------------------------------------------------------------------------------------
_afm_identity = {}


def _afm_identity_weight(K: int, device) -> Variable:
    """W = I for the bilinear kernel (a constant: its 'gradient' buffer is scratch)."""
    key = (K, str(device))
    v = _afm_identity.get(key)
    if v is None:
        v = _afm_identity[key] = Variable("afm/identity", torch.eye(K, device=device))
    return v


def afm_fused_served(fields: torch.Tensor, F: int, K: int, t: int) -> bool:
    """Whether afm_attention(fused=True) has a kernel for these fields: an fp32 [B >= 1, F * K] device tensor of a served shape."""
    from . import ops
    return _fp32_matrix_on_device(fields) and fields.shape[0] >= 1 and fields.shape[1] == F * K and ops.afm_supported(F, K, t)


def afm_fused_default(fields: torch.Tensor, F: int, K: int, t: int) -> bool:
    """Whether afm_attention(fused=None) runs the fused kernels: wherever they serve the shape."""
    return afm_fused_served(fields, F, K, t)


def afm_attention(fields: torch.Tensor, F: int, K: int, w: Variable, b: Variable, h: Variable,
                  fused: Optional[bool] = None) -> torch.Tensor:
    """algorithm/AFM/afm.py:162-188: the pair products e_i * e_j (i < j, row-major over the strict upper triangle) of the F field
    embeddings of fields [B, F * K], their attention scores relu(pairs @ w + b) @ h, the softmax over the pairs and the weighted
    sum -> [B, K].  w [K, t], b [t], h [t, 1] are the model's own variables.
    fused (not a reference argument; the model: params["afm_fused"]), in the manner of residual_stack.  False runs the
    composed chain — the FiBiNET bilinear kernel with W = I on the fields plus one zero field (that kernel pairs
    `combinations(range(F' - 1), 2)`, quirk B-3), the fp32-MFMA dense kernel on [B * P, K], the one-unit head and
    ops.attention_pool.  True runs ops.afm_attention, one launch each way (csrc/afm.hip), where afm_fused_served says so: an
    fp32 device tensor and 2 <= F <= 64, K % 4 == 0 with 4 <= K <= 32, t % 16 == 0 with 16 <= t <= 256 (a non-contiguous
    `fields` is copied first); anywhere else True is a ValueError.  None picks the kernel wherever True would succeed
    (afm_fused_default; the measurement: DESIGN.md §5 "AFM attention").
    tests/afm_ref.py is the float64 restatement both paths answer to."""
    from . import ops
    store = current_store()
    F, K = int(F), int(K)
    t = int(w.data.shape[1])
    served = afm_fused_served(fields, F, K, t)                                    # (= afm_fused_default)
    if _resolve_fused(fused, served, served, f"afm_attention(fused=True): no fused kernel serves F={F} K={K} t={t} on {fields.device}"):
        return ops.afm_attention(ops._contig(fields), F, K, w, b, h, anchor=store.anchor)
    B, P = fields.shape[0], F * (F - 1) // 2
    # pair Hadamard products over all F fields: the bilinear kernel pairs the first F' - 1 of F' fields -> one zero field
    padded = torch.cat([fields, fields.new_zeros(B, K)], dim=1).reshape(B, F + 1, K)
    pairs = ops.bilinear_interaction(store, "all", padded.contiguous(), _afm_identity_weight(K, fields.device))   # (B, P, K)
    att = dense_with(pairs.reshape(B * P, K), w, b, relu=True)                   # relu(pairs @ w + b)   (B*P, t)
    att = dense_with(att, h, None, relu=False)                                    # @ h                   (B*P, 1)
    return ops.attention_pool(pairs, att.reshape(B, P))                           # softmax over pairs, weighted sum (B, K)


# ---- AutoInt's interacting layer (Song et al., CIKM 2019, eqs. 5-8) -------------------------------------------------------------------
def interacting_layer(x: torch.Tensor, F: int, att_embedding_size: int, head_num: int, use_res: bool, index: int) -> torch.Tensor:
    """One interacting layer over the F field rows of x [B, F * D]: multi-head self-attention over the fields, unscaled, with the
    optional residual projection and a ReLU -> [B, F * head_num * att_embedding_size], head-major columns (the arithmetic:
    include/recalgo_autoint.h; tests/autoint_ref.py is its float64 restatement).  Variables under the caller's scope, default
    glorot-uniform: interacting_layer_<index>_w_query, _w_key, _w_value [head_num, D, att_embedding_size] and, with use_res,
    _w_res [D, head_num * att_embedding_size].  One launch each way (ops.autoint_layer); sizes csrc/autoint.hip does not
    serve are a ValueError — there is no composed path."""
    from . import ops
    store = current_store()
    F, A, H = int(F), int(att_embedding_size), int(head_num)
    if x.dim() != 2 or F < 1 or x.shape[1] % F:
        raise ValueError(f"interacting_layer: x must be [B, F * D] with F = {F}, got {tuple(x.shape)}")
    D = int(x.shape[1]) // F
    ws = [store.get_variable(f"interacting_layer_{index}_w_{n}", (H, D, A)) for n in ("query", "key", "value")]
    w_res = store.get_variable(f"interacting_layer_{index}_w_res", (D, H * A)) if use_res else None
    if store.building:
        return x.new_zeros(x.shape[0], F * H * A)
    return ops.autoint_layer(ops._contig(x), F, *ws, w_res, anchor=store.anchor)


# ---- DCN-V2's cross layer (Wang et al., WWW 2021, eq. 4) ---------------------------------------------------------------------------------
def cross_mix_fused_default(x0: torch.Tensor, low_rank: int, num_experts: int) -> bool:
    """What cross_mix_layer(fused=None) picks: the kernels wherever they serve the tensor and the shape (csrc/dcnv2.hip; the
    measurement: DESIGN.md §5 "DCN-V2 cross layer")."""
    from . import ops
    return _fp32_matrix_on_device(x0) and ops.dcnv2_supported(int(x0.shape[1]), int(low_rank), int(num_experts))


def cross_mix_layer(x0: torch.Tensor, xl: torch.Tensor, low_rank: int, num_experts: int, index: int, fused=None) -> torch.Tensor:
    """One DCN-V2 cross layer, the mixture of `num_experts` low-rank experts of rank `low_rank` with a softmax gate over xl (the
    arithmetic: include/recalgo_dcnv2.h; tests/dcnv2_ref.py is its float64 restatement):
        x0 * sum_e p_e (tanh(tanh(xl V_e) C_e) U_e^T + bias) + xl,   p = softmax_e(xl . gate_e)
    Variables under the caller's scope: cross_layer_<index>/V, U [E, D, r], C [E, r, r], gate [E, D] (default glorot-uniform) and
    bias [D] (zeros).  fused (not a paper argument), in the manner of residual_stack: True runs ops.dcnv2_layer, one entry each way
    (csrc/dcnv2.hip), and is a ValueError where the kernels do not serve the shape; False runs the layer composed from torch ops —
    the path the bench compares against, and the one for shapes outside the kernels' domain; None takes the kernels wherever True
    would succeed (cross_mix_fused_default)."""
    from . import ops
    store = current_store()
    D, r, E = int(x0.shape[-1]), int(low_rank), int(num_experts)
    with store.variable_scope(f"cross_layer_{index}"):
        V, C, U = store.get_variable("V", (E, D, r)), store.get_variable("C", (E, r, r)), store.get_variable("U", (E, D, r))
        gate = store.get_variable("gate", (E, D))
        bias = store.get_variable("bias", (D,), zeros)
    if store.building:
        return torch.zeros_like(x0)
    default = cross_mix_fused_default(x0, r, E)
    if _resolve_fused(fused, default, default, None):        # (True on a shape the kernels do not serve: ops.dcnv2_layer refuses)
        same = xl is x0
        x0 = ops._contig(x0)
        return ops.dcnv2_layer(x0, x0 if same else ops._contig(xl), V, C, U, gate, bias, anchor=store.anchor)
    Vt, Ct, Ut, gt, bt = (ops.variable_leaf(v, store.anchor) for v in (V, C, U, gate, bias))
    v = torch.tanh(torch.einsum("bd,edr->ber", xl, Vt))
    c = torch.tanh(torch.einsum("ber,ers->bes", v, Ct))
    u = torch.einsum("ber,edr->bed", c, Ut) + bt
    p = torch.softmax(xl @ gt.t(), dim=-1)
    return x0 * torch.einsum("be,bed->bd", p, u) + xl


def cross_mix_network(x0: torch.Tensor, num_cross_layer: int, low_rank: int, num_experts: int, fused=None) -> torch.Tensor:
    """x_{l+1} = cross_mix_layer(x0, x_l, l) for l = 0 .. num_cross_layer - 1, x_0 = x0: one entry each way per layer."""
    xl = x0
    for i in range(int(num_cross_layer)):
        xl = cross_mix_layer(x0, xl, low_rank, num_experts, i, fused=fused)
    return xl


# ---- FLEN's field-wise bi-interaction with Dicefactor (Chen et al., arXiv 1911.04690) -----------------------------------------------
def flen_fused_default(fields: torch.Tensor, F: int, M: int, K: int) -> bool:
    """What field_wise_bi_interaction(fused=None) picks: the kernels wherever they serve the tensor and the shape (csrc/flen.hip;
    the measurement: DESIGN.md §5 "FLEN field-wise bi-interaction" — they were the faster path at every measured shape class)."""
    from . import ops
    return _fp32_matrix_on_device(fields) and ops.flen_supported(int(F), int(M), int(K))


_flen_index_cache: dict = {}


def _flen_indices(group_of: tuple, M: int, device):
    """the composed path's index tensors — each group's fields, the pairs' first and second groups — made once per (grouping,
    device): a captured step's replays find them on the device"""
    from itertools import combinations
    key = (group_of, str(device))
    if key not in _flen_index_cache:
        members = [torch.tensor([f for f, g in enumerate(group_of) if g == m], device=device) for m in range(M)]
        first, second = (torch.tensor(ix, device=device) for ix in zip(*combinations(range(M), 2)))
        _flen_index_cache[key] = (members, first, second)
    return _flen_index_cache[key]


def field_wise_bi_interaction(fields: torch.Tensor, group_of, dice_rate: float = 0.0, training: bool = False, fused=None):
    """FLEN's field-wise bi-interaction over the F = len(group_of) field rows of fields [B, F * K]; group_of[f] in [0, M) is
    field f's group and every group holds a field (the arithmetic: include/recalgo_flen.h; tests/flen_ref.py is its float64
    restatement) -> (e [B, M * K], h [B, K]):
        e_m = sum of group m's rows      h = bias + sum_{i<j} r_mf[p] c_p e_i e_j + sum_m r_fm[m] c_{P+m} (e_m^2 - sum x_f^2)
    Variables under the caller's scope: r_mf [M (M - 1) / 2] (ones), r_fm [M] (0.5) and bias [K] (zeros).  Dicefactor: when
    training with dice_rate > 0 the [B, P + M, K] path components are dropped like any other dropout of the model_fn (drop_spec:
    the next call of the hash stream, or the next injected keep mask) and scaled by 1 / (1 - rate); EVAL and PREDICT apply none.
    fused (not a paper argument), as in cross_mix_layer: True runs ops.flen_interaction, one launch each way, and is a ValueError
    where the kernels do not serve; False runs the arithmetic composed from torch ops — the path the bench compares against, and
    the one outside the kernels' domain; None takes the kernels wherever True would succeed (flen_fused_default)."""
    from . import ops
    from .variables import constant
    store = current_store()
    group_of = tuple(int(g) for g in group_of)
    F = len(group_of)
    M = max(group_of) + 1 if group_of else 0
    if F < 2 or M < 2 or set(group_of) != set(range(M)):
        raise ValueError(f"field_wise_bi_interaction: group_of must map at least two fields onto every one of M >= 2 groups "
                         f"0 .. M - 1, got {group_of}")
    if fields.dim() != 2 or fields.shape[1] % F:
        raise ValueError(f"field_wise_bi_interaction: fields must be [B, F * K] with F = {F}, got {tuple(fields.shape)}")
    B, K = int(fields.shape[0]), int(fields.shape[1]) // F
    P = M * (M - 1) // 2
    r_mf = store.get_variable("r_mf", (P,), ones)
    r_fm = store.get_variable("r_fm", (M,), constant(0.5))
    bias = store.get_variable("bias", (K,), zeros)
    if store.building:
        return fields.new_zeros(B, M * K), fields.new_zeros(B, K)
    served = flen_fused_default(fields, F, M, K)
    fused = _resolve_fused(fused, served, served,
                           f"field_wise_bi_interaction(fused=True): no fused kernel serves F={F} M={M} K={K} on {fields.device}")
    dice = drop_spec((B, P + M, K), float(dice_rate), fields.device) if (training and dice_rate and dice_rate > 0.0) else None
    if fused:
        return ops.flen_interaction(ops._contig(fields), F, group_of, r_mf, r_fm, bias, dice=dice, anchor=store.anchor)
    mf_w, fm_w, b = (ops.variable_leaf(v, store.anchor) for v in (r_mf, r_fm, bias))
    x = fields.reshape(B, F, K)
    members, first, second = _flen_indices(group_of, M, fields.device)
    e = torch.stack([x.index_select(1, idx).sum(1) for idx in members], dim=1)                          # [B, M, K]
    q = torch.stack([x.index_select(1, idx).square().sum(1) for idx in members], dim=1)
    paths = torch.cat([mf_w[:, None] * (e.index_select(1, first) * e.index_select(1, second)), fm_w[:, None] * (e * e - q)], dim=1)
    if dice is not None:
        keep = dice.mask if dice.mask is not None else ops.dropout_keep_mask((B, P + M, K), dice, fields.device)
        paths = paths * (keep * dice.scale)
    return e.reshape(B, M * K), b + paths.sum(1)
