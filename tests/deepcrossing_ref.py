"""DeepCrossing restated in torch, dtype-parametric: float64 is the oracle of the tests, float32 their `ref32` (the reference
arithmetic's own rounding).  The bare residual stack (algorithm/DeepCrossing/residual_unit.py:4-22), its backward from GIVEN
masks (what include/recalgo_res.h's backward entry computes: nothing is recomputed), and the whole model
(deepcrossing.py:131-178)."""
import math

import torch


def stack_forward(x, w0s, b0s, w1s, b1s):
    """-> (hs [L, B, H], ys [L, B, D]): h_l = relu(x_l W0_l + b0_l), ys[l] = x_{l+1} = relu(x_l + (h_l W1_l + b1_l))"""
    hs, ys = [], []
    for w0, b0, w1, b1 in zip(w0s, b0s, w1s, b1s):
        h = torch.relu(x @ w0 + b0)
        x = torch.relu(x + (h @ w1 + b1))
        hs.append(h)
        ys.append(x)
    return torch.stack(hs), torch.stack(ys)


def stack_backward(g, hs, ys, w0s, w1s):
    """The backward with the masks READ from hs / ys -> (dzs [L, B, D], dhs [L, B, H], dx):
    dz_l = g_{l+1} [ys[l] > 0], dh_l = (dz_l W1_l^T) [hs[l] > 0], g_l = dz_l + dh_l W0_l^T"""
    L = len(w0s)
    dzs, dhs = [None] * L, [None] * L
    zero = torch.zeros((), dtype=g.dtype)
    for l in range(L - 1, -1, -1):
        dz = torch.where(ys[l] > 0, g, zero)
        dh = torch.where(hs[l] > 0, dz @ w1s[l].t(), zero)
        g = dz + dh @ w0s[l].t()
        dzs[l], dhs[l] = dz, dh
    return torch.stack(dzs), torch.stack(dhs), g


def weight_grads(x, hs, ys, dzs, dhs):
    """-> [(dW0_l, db0_l, dW1_l, db1_l)]: the batch sums the caller of the backward entry forms"""
    out = []
    for l in range(len(hs)):
        xl = x if l == 0 else ys[l - 1]
        out.append((xl.t() @ dhs[l], dhs[l].sum(dim=0), hs[l].t() @ dzs[l], dzs[l].sum(dim=0)))
    return out


def random_stack(B, D, H, L, seed, dtype=torch.float64):
    """Inputs of a stack: values that are float32 numbers, held in `dtype`; glorot-sized kernels, biases and inputs of order 1
    (both ReLUs see both signs).  -> {x, g, w0, b0, w1, b1} (the last four: lists of L)"""
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return ((torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1) * scale).to(torch.float32).to(dtype)
    lim = math.sqrt(6.0 / (D + H))
    return {"x": rnd(B, D), "g": rnd(B, D),
            "w0": [rnd(D, H, scale=lim) for _ in range(L)], "b0": [rnd(H, scale=0.2) for _ in range(L)],
            "w1": [rnd(H, D, scale=lim) for _ in range(L)], "b1": [rnd(D, scale=0.2) for _ in range(L)]}


def cast(case, dtype):
    return {k: ([t.to(dtype) for t in v] if isinstance(v, list) else v.to(dtype)) for k, v in case.items()}


def stack_variables(P, L, scope="residual_module"):
    """the four parameter lists of the stack from the model's variables (the reference's names)"""
    return ([P[f"{scope}/dense_{i}_0/kernel"] for i in range(L)], [P[f"{scope}/dense_{i}_0/bias"] for i in range(L)],
            [P[f"{scope}/dense_{i}_1/kernel"] for i in range(L)], [P[f"{scope}/dense_{i}_1/bias"] for i in range(L)])


def model_input(P, feats, params):
    """concat_all of deepcrossing.py:144-152"""
    from oracle import ref_models as M
    dense_in = M.input_layer(P, feats, params["dense_feature_columns"], "dense_input/input_layer")
    category = M.input_layer(P, feats, params["category_feature_columns"], "category_input/input_layer", {})
    return torch.cat([dense_in, category], dim=-1)


def relu_margins(P, feats, params):
    """Per ReLU of the stack (2 L of them, unit by unit): min |pre-activation| / max |pre-activation| over the batch."""
    x = model_input(P, feats, params)
    out = []
    for w0, b0, w1, b1 in zip(*stack_variables(P, int(params["residual_network_num"]))):
        z0 = x @ w0 + b0
        h = torch.relu(z0)
        z1 = x + (h @ w1 + b1)
        x = torch.relu(z1)
        out += [float(z0.abs().min() / z0.abs().max()), float(z1.abs().min() / z1.abs().max())]
    return out


def deepcrossing(P, feats, labels, params, training=False):
    """deepcrossing.py:131-178 on the variables P (the reference's names) -> {"logit", "prob", and with labels "loss"}"""
    from oracle import ref_models as M
    from oracle import ref_ops as O
    x = model_input(P, feats, params)
    L = int(params["residual_network_num"])
    if L:
        x = stack_forward(x, *stack_variables(P, L))[1][-1]
    logit = O.dense(x, P["dense/kernel"], P["dense/bias"])
    return M._tail(logit, None if labels is None else labels["read_comment"])
