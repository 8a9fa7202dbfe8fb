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
