"""tests/dense_ref.py is right: its backward is torch.autograd of its forward (with a ReLU below the layer, and with a
BatchNorm below it), its tile partials add up to the whole-batch definitions, and the option tables of
tests/test_gpu_dense_abi.py cover every pair of option values.  No GPU."""
import itertools

import pytest
import torch

from tests import dense_ref as R

TOL = 1e-12


def _close(a, b, what):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape, what
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= TOL * scale, f"{what}: {float((a - b).abs().max()):.3g}"


def _inputs(M, K, N, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    return dict(u=r(M, K), w=r(K, N) / K ** 0.5, b=r(N) * 0.1, up=r(M, N), c=r(M, K), gamma=torch.rand(K, generator=gen, dtype=torch.float64) + 0.5,
                shift=r(K))


@pytest.mark.parametrize("M,K,N", [(1, 4, 4), (64, 8, 8), (65, 33, 50), (130, 84, 68), (300, 100, 52)])
@pytest.mark.parametrize("relu", [False, True])
def test_bwd_is_autograd_of_fwd_over_a_relu(M, K, N, relu):
    """x = relu(u): the layer is called with dx_relu_mask = x and returns dL/du; the beta * c_in term is the gradient of
    beta * <c_in, u>, which does not pass through the ReLU: it is added after the mask."""
    t = _inputs(M, K, N, M + K + N)
    u, w, b = (t[k].clone().requires_grad_(True) for k in ("u", "w", "b"))
    x = torch.relu(u)
    z, y, _ = R.fwd(x, w, bias=b, relu=relu)
    beta = 0.25
    ((y * t["up"]).sum() + beta * (t["c"] * u).sum()).backward()
    dx, dw, db, part = R.bwd(x.detach(), t["up"], y.detach() if relu else None, w.detach(), c_in=t["c"], beta=beta,
                             dx_relu_mask=x.detach())
    assert part is None
    _close(dx, u.grad, "dx")
    _close(dw, w.grad, "dw")
    _close(db, b.grad, "dbias")
    # without the options: plain dL/dx
    x2 = t["u"].clone().requires_grad_(True)
    _, y2, _ = R.fwd(x2, t["w"], bias=t["b"], relu=relu)
    (y2 * t["up"]).sum().backward()
    dx2 = R.bwd(x2.detach(), t["up"], y2.detach() if relu else None, t["w"])[0]
    _close(dx2, x2.grad, "dx, no options")


@pytest.mark.parametrize("M,K,N", [(1, 4, 4), (64, 8, 8), (65, 33, 50), (130, 84, 68), (300, 100, 52)])
def test_bwd_partials_are_the_sums_a_batchnorm_below_starts_with(M, K, N):
    """x = xhat * gamma + shift, xhat = (bn_x - mean) * rstd with the batch statistics held fixed: d(shift) = colsum(dx),
    d(gamma) = colsum(dx * xhat) — the tile partials of bwd, added over the tiles."""
    t = _inputs(M, K, N, 3 * M + K)
    bn_x = t["u"]
    mean = bn_x.mean(0)
    rstd = 1.0 / (bn_x.var(0, unbiased=False) + 1e-3).sqrt()
    gamma, shift, w = (t[k].clone().requires_grad_(True) for k in ("gamma", "shift", "w"))
    xhat = (bn_x - mean) * rstd
    x = xhat * gamma + shift
    _, y, _ = R.fwd(x, w, bias=t["b"], relu=True)
    (y * t["up"]).sum().backward()
    dx, dw, db, part = R.bwd(x.detach(), t["up"], y.detach(), w.detach(), bn_x=bn_x, bn_mean=mean, bn_rstd=rstd)
    assert part.shape == (R.partial_rows(M), 2 * K)
    _close(part[:, :K].sum(0), shift.grad, "colsum(dx) over the tiles")
    _close(part[:, K:].sum(0), gamma.grad, "colsum(dx * xhat) over the tiles")
    _close(part[:, :K].sum(0), dx.sum(0), "colsum(dx)")
    _close(dw, w.grad, "dw")
    # ... and through the whole BatchNorm: dL/d(bn_x) from those two sums is autograd's
    bx = bn_x.clone().requires_grad_(True)
    mu = bx.mean(0)
    rs = 1.0 / (((bx - mu) ** 2).mean(0) + 1e-3).sqrt()
    xx = (bx - mu) * rs * t["gamma"] + t["shift"]
    _, yy, _ = R.fwd(xx, t["w"], bias=t["b"], relu=True)
    (yy * t["up"]).sum().backward()
    dbeta, dgamma = part[:, :K].sum(0), part[:, K:].sum(0)
    dbx = t["gamma"] * rstd / M * (M * dx - dbeta - xhat * dgamma)
    _close(dbx, bx.grad, "BatchNorm backward from the partial rows")


@pytest.mark.parametrize("M,N", [(1, 4), (64, 8), (65, 50), (300, 52), (1025, 36)])
@pytest.mark.parametrize("act", [None, R.PRELU, R.DICE])
def test_fwd_partials_merge_to_the_batch_moments(M, N, act):
    """Chan's merge of the per-tile (mean, M2) rows gives the batch mean and sum of squared deviations of y."""
    K = 12
    t = _inputs(M, K, N, M + N)
    alpha = torch.rand(N, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 0.5 + 0.1
    z, y, part = R.fwd(t["u"], t["w"], bias=t["b"], relu=act is None, act_kind=act, alpha=alpha)
    assert part.shape == (R.partial_rows(M), 2 * N)
    n, mean, m2 = 0, torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for i in range(part.shape[0]):
        nb = min(R.TILE, M - i * R.TILE)
        d = part[i, :N] - mean
        mean = mean + d * nb / (n + nb)
        m2 = m2 + part[i, N:] + d * d * n * nb / (n + nb)
        n += nb
    assert n == M
    _close(mean, y.mean(0), "merged mean")
    _close(m2, ((y - y.mean(0)) ** 2).sum(0), "merged M2")
    _close(z, t["u"] @ t["w"] + t["b"], "z")
    if act == R.PRELU:
        _close(y, torch.nn.functional.prelu(z, alpha), "PReLU")
    if act == R.DICE:
        p = torch.sigmoid(z / 1.001 ** 0.5)
        _close(y, p * z + (1 - p) * alpha * z, "Dice")


def test_fwd_second_pair_dropout_and_colsum():
    t = _inputs(70, 9, 10, 5)
    gen = torch.Generator().manual_seed(2)
    x2, w2 = torch.randn(70, 5, generator=gen, dtype=torch.float64), torch.randn(5, 10, generator=gen, dtype=torch.float64)
    keep = (torch.rand(70, 10, generator=gen) > 0.3).double()
    z, y, _ = R.fwd(t["u"], t["w"], x2, w2, t["b"], relu=True, drop_keep=keep, drop_rate=0.3)
    _close(z, torch.cat([t["u"], x2], 1) @ torch.cat([t["w"], w2], 0) + t["b"], "two operand pairs")
    _close(y, torch.relu(z) * keep / 0.7, "dropout behind the ReLU")
    flat = torch.randn(17 * 13 + 5, generator=gen, dtype=torch.float64)
    want = sum(flat[r * 13:r * 13 + 10] for r in range(17))
    _close(R.colsum(flat, 17, 13, 10), want, "colsum")
    z32, y32, p32 = R.fwd(t["u"], t["w"], bias=t["b"], dtype=torch.float32)
    assert z32.dtype == y32.dtype == p32.dtype == torch.float32
    assert all(o.dtype == torch.float32 for o in R.bwd(t["u"], t["up"], None, t["w"], dtype=torch.float32)[:3])


@pytest.mark.parametrize("rows,stride,n", [(1, 5, 5), (3, 7, 4), (16, 9, 9), (17, 13, 10), (261, 40, 33)])
def test_colsum_fixed_order_is_the_column_sum(rows, stride, n):
    """Within fp32 rounding of the float64 colsum: `rows` - 1 additions per column at most, each off by at most half an ulp of
    a partial sum no larger than the column's sum of magnitudes A: |error| <= (rows - 1) * 2^-24 * A."""
    gen = torch.Generator().manual_seed(rows * 100 + n)
    flat = torch.randn(rows * stride + 3, generator=gen)
    got = R.colsum_fixed_order(flat, rows, stride, n)
    assert got.dtype == torch.float32 and got.shape == (n,)
    want = R.colsum(flat, rows, stride, n)
    bound = (rows - 1) * 2.0 ** -24 * R.colsum(flat.abs(), rows, stride, n)
    assert bool(((got.double() - want).abs() <= bound).all()), float(((got.double() - want).abs() - bound).max())
    if rows == 1:
        assert torch.equal(got, flat[:n])


def test_colsum_fixed_order_is_not_the_row_order():
    """Rows 0 and 16 (both group 0) hold +1e8 and -1e8, rows 1..15 hold 1: group 0 cancels exactly and the fifteen ones
    survive, 15.0f.  In plain row order every 1 is absorbed by 1e8 (ulp 8) and the sum is 0.0f.  A second column has the pair
    in rows 0 and 1 (groups 0 and 1): there row order is exact, and the group order loses row 16's 1 to row 0's 1e8."""
    rows = 17
    m = torch.ones(rows, 2)
    m[0, 0], m[16, 0] = 1e8, -1e8
    m[0, 1], m[1, 1] = 1e8, -1e8
    got = R.colsum_fixed_order(m.reshape(-1), rows, 2, 2)
    plain = torch.zeros(2)
    for r in range(rows):
        plain = plain + m[r]
    assert got.tolist() == [15.0, 14.0] and plain.tolist() == [0.0, 15.0]
    assert R.colsum(m.reshape(-1), rows, 2, 2).tolist() == [15.0, 15.0]


# ---- the option tables of tests/test_gpu_dense_abi.py -----------------------------------------------------------------------
def _uncovered(axes, rows, valid):
    """The pairs of values of two axes that some legal call has (a pair no legal call has is ruled out by a REQUIRE of the
    header) and no row of the table has."""
    names = list(axes)
    pairs = lambda r: {(a, r[a], b, r[b]) for a, b in itertools.combinations(names, 2)}
    legal = set()
    for full in itertools.product(*axes.values()):
        r = dict(zip(names, full))
        if valid(r):
            legal |= pairs(r)
    have = set().union(*(pairs(r) for r in rows))
    return sorted(legal - have, key=repr)


def test_option_tables_cover_every_pair():
    from tests import test_gpu_dense_abi as T
    for axes, rows, valid in ((T.BWD_AXES, T.BWD_ROWS, T.bwd_row_valid), (T.FWD_AXES, T.FWD_ROWS, T.fwd_row_valid)):
        rows = [dict(zip(axes, r)) for r in rows]
        for r in rows:
            assert all(r[a] in axes[a] for a in axes) and valid(r), r
        assert _uncovered(axes, rows, valid) == []
    assert set(T.BWD_AXES["shape"]) == set(T.FWD_AXES["shape"]) == {(300, 100, 52), (65, 84, 50), (1025, 128, 36), (130, 33, 68)}
