"""The inference tower of include/recalgo_serve.h restated in torch.

    tower64(x, layers)   float64, plain matrix products: the oracle of tests/test_gpu_serve_tower.py
    tower32(x, layers)   float32 in the ORDER the header states, term by term: two fmaf chains per dot product (chain 0 starts at
                         the bias), groups of 16 k alternating between them, inside a group k = 16 g + 4 q + x for x, then q;
                         z = c0 + c1; relu; fmaf(a, scale, shift).  The `ref32` of assert_close.
    fold(gamma, beta, moving_mean, moving_variance, epsilon)   the BatchNorm fold the caller of the kernel computes

layers: [(W [K, N], b [N] | None, scale [N] | None, shift [N] | None, relu)] of float64 tensors.  An fp32 fmaf is evaluated as
float64(a) * float64(b) + float64(c) rounded to float32: the product of two fp32 numbers is exact in float64, so the only
departure from a hardware fmaf is the double rounding of the sum, one case in ~2^29.
"""
import torch


def fold(gamma, beta, moving_mean, moving_variance, epsilon):
    scale = gamma * torch.rsqrt(moving_variance + epsilon)
    return scale, beta - moving_mean * scale


def tower64(x, layers):
    h = x.double()
    for w, b, scale, shift, relu in layers:
        z = h @ w.double()
        if b is not None:
            z = z + b.double()
        a = torch.relu(z) if relu else z
        h = a * scale.double() + shift.double() if scale is not None else a
    return h


def _fmaf(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def tower32(x, layers):
    h = x.float()
    for w, b, scale, shift, relu in layers:
        w = w.float()
        K, N = w.shape
        chains = [(b.float() if b is not None else torch.zeros(N)).expand(h.shape[0], N).clone(), torch.zeros(h.shape[0], N)]
        for g in range((K + 15) // 16):
            c = chains[g % 2]
            for x_ in range(4):
                for q in range(4):
                    k = 16 * g + 4 * q + x_
                    if k < K:                    # (the terms past K are exact zeros)
                        c = _fmaf(h[:, k:k + 1], w[k:k + 1, :], c)
            chains[g % 2] = c
        z = chains[0] + chains[1]
        a = torch.relu(z) if relu else z
        h = _fmaf(a, scale.float(), shift.float()) if scale is not None else a
    return h


def random_tower(B, K0, units, relu_bits, scale_layers, nobias_layers, seed):
    """-> (x [B, K0], layers) in float64, every value exactly representable in float32.  Weights ~ glorot, BatchNorm statistics
    as a trained model has them (variance around 1, mean and beta of the activations' size)."""
    g = torch.Generator().manual_seed(seed)
    r32 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()          # noqa: E731
    x = r32(B, K0)
    layers, K = [], K0
    for l, N in enumerate(units):
        w = (r32(K, N) * (2.0 / (K + N)) ** 0.5).float().double()
        b = None if l in nobias_layers else (0.1 * r32(N)).float().double()
        scale = shift = None
        if l in scale_layers:
            gamma, beta, mean = 1 + 0.2 * r32(N), 0.1 * r32(N), 0.3 * r32(N)
            var = (0.5 + torch.rand(N, generator=g, dtype=torch.float64))
            scale, shift = (t.float().double() for t in fold(gamma, beta, mean, var, 1e-3))
        layers.append((w, b, scale, shift, bool((relu_bits >> l) & 1)))
        K = N
    return x, layers
