"""The dense ABI of include/recalgo.h (recalgo_dense_fwd / _bwd_input / _bwd_weights / _bwd / _bwd_weights_reduce) stated once in
plain torch on the CPU, written from the header's comments.  `dtype` is the arithmetic: float64 is the reference, float32
the same statement in the reference's own rounding (the `ref32` of tests/util.assert_close).  Nothing here but
colsum_fixed_order, the restatement of the fixed summation order, follows the order in which a kernel adds;
tests/test_dense_ref_host.py checks these functions against torch.autograd.

Tile rows: the BatchNorm partial rows are per 64 consecutive examples (recalgo_batchnorm_partial_rows(M) = ceil(M / 64))."""
import torch

TILE = 64
PRELU, DICE = 0, 1          # RECALGO_ACT_PRELU, RECALGO_ACT_DICE
DICE_EPS = 1e-3


def partial_rows(M):
    return (M + TILE - 1) // TILE


def _tiles(t):
    return [t[r:r + TILE] for r in range(0, t.shape[0], TILE)]


def activation(z, act_kind, alpha):
    """PReLU: max(0, z) + alpha * min(0, z).  Dice: p = sigmoid(z / sqrt(1 + 1e-3)), z * p + alpha * z * (1 - p)."""
    if act_kind == PRELU:
        return z.clamp(min=0) + alpha * z.clamp(max=0)
    if act_kind == DICE:
        p = torch.sigmoid(z / (1.0 + DICE_EPS) ** 0.5)
        return z * p + alpha * z * (1 - p)
    raise ValueError(act_kind)


def fwd(x, w, x2=None, w2=None, bias=None, relu=False, act_kind=None, alpha=None, drop_keep=None, drop_rate=0.0,
        dtype=torch.float64):
    """-> (z, y, bn_partials): z = x w (+ x2 w2) + bias, y = act(z) (ReLU | PReLU | Dice | none), then the training-mode dropout
    y * keep / (1 - rate); bn_partials [ceil(M / 64)][2 N]: per 64-row tile of y the column means, then the sums of squared
    deviations from the tile's mean."""
    c = lambda t: None if t is None else t.to(dtype)
    x, w, x2, w2, bias, alpha, drop_keep = c(x), c(w), c(x2), c(w2), c(bias), c(alpha), c(drop_keep)
    z = x @ w
    if x2 is not None:
        z = z + x2 @ w2
    if bias is not None:
        z = z + bias
    if act_kind is not None:
        assert not relu
        y = activation(z, act_kind, alpha)
    else:
        y = torch.relu(z) if relu else z
    if drop_keep is not None:
        y = y * drop_keep * torch.tensor(1.0 / (1.0 - drop_rate), dtype=dtype)
    parts = []
    for t in _tiles(y):
        mean = t.mean(0)
        parts.append(torch.cat([mean, ((t - mean) ** 2).sum(0)]))
    bn_partials = torch.stack(parts) if parts else y.new_zeros(0, 2 * y.shape[1])
    return z, y, bn_partials


def bwd(x, g, y_mask, w, c_in=None, beta=0.0, dx_relu_mask=None, bn_x=None, bn_mean=None, bn_rstd=None, dtype=torch.float64):
    """-> (dx, dw, dbias, bn_partials):
        gm = g * [y_mask > 0]
        dx = (gm w^T) * [dx_relu_mask > 0] + beta * c_in          (the mask on the product only)
        dw = x^T gm,  dbias = colsum(gm)
        bn_partials [ceil(M / 64)][2 K]: per 64-row tile colsum(dx) and colsum(dx * xhat), xhat = (bn_x - bn_mean) * bn_rstd
    (None when bn_x is None)."""
    c = lambda t: None if t is None else t.to(dtype)
    x, g, w, c_in, bn_x, bn_mean, bn_rstd = c(x), c(g), c(w), c(c_in), c(bn_x), c(bn_mean), c(bn_rstd)
    gm = g if y_mask is None else g * (y_mask > 0).to(dtype)
    dx = gm @ w.t()
    if dx_relu_mask is not None:
        dx = dx * (dx_relu_mask > 0).to(dtype)
    if c_in is not None:
        dx = dx + torch.tensor(beta, dtype=torch.float32).to(dtype) * c_in
    dw = x.t() @ gm
    dbias = gm.sum(0)
    bn_partials = None
    if bn_x is not None:
        xhat = (bn_x - bn_mean) * bn_rstd
        bn_partials = torch.stack([torch.cat([d.sum(0), (d * h).sum(0)]) for d, h in zip(_tiles(dx), _tiles(xhat))])
    return dx, dw, dbias, bn_partials


def colsum(partials, rows, row_stride, n, dtype=torch.float64):
    """recalgo_colsum_t: out[i] = sum_{r < rows} partials[r * row_stride + i], i < n; `partials` flat."""
    p = partials.reshape(-1).to(dtype)
    return torch.as_strided(p, (rows, n), (row_stride, 1)).sum(0)


GROUPS = 16


def colsum_fixed_order(partials, rows, row_stride, n):
    """The ONE order in which the library adds partial rows (csrc/slab_sum.h, sum_tall), restated in fp32 on the CPU: for each
    g < 16 the rows g, g + 16, g + 32, .. are added in row order starting from 0.0f, then the sixteen group sums are added in
    group order starting from 0.0f.  Every add is one IEEE fp32 addition, so a kernel that keeps the order returns these bits.
    (Unlike the functions above, this one does follow the kernels' order: it is the statement of the determinism contract.)"""
    p = partials.detach().cpu().reshape(-1)
    assert p.dtype == torch.float32
    m = torch.as_strided(p, (rows, n), (row_stride, 1))
    out = torch.zeros(n, dtype=torch.float32)
    for g in range(GROUPS):
        acc = torch.zeros(n, dtype=torch.float32)
        for r in range(g, rows, GROUPS):
            acc = acc + m[r]
        out = out + acc
    return out
