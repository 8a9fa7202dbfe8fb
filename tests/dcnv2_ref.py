"""DCN-V2's cross layer, the mixture of low-rank experts (include/recalgo_dcnv2.h; Wang et al., WWW 2021, eq. 4) restated in
torch, differentiated by autograd, in float64 (the yardstick) or float32 (the arithmetic's own rounding); results are computed
once per case and shared.  The upstream zoo has no DCN-V2 file, so this restatement is the reference.  Also the header's backward
formulas written out, and the whole model as a function of named variables (algorithm/DCNV2/dcnv2.py's graph) for the step
tests."""
import functools

import torch

NAMES = ("y", "dx0", "dxl", "dV", "dC", "dU", "dgate", "dbias")
REDUCED = ("dV", "dC", "dU", "dgate", "dbias")

# (B, D, r, E): the shapes of the GPU parity tests (tests/test_gpu_dcnv2.py)
SHAPES = [(1, 4, 4, 1),           # the smallest of everything
          (17, 5, 4, 2),          # D not a multiple of 4, a partial example tile
          (33, 82, 8, 2),         # the width of the dataset's columns
          (19, 416, 32, 4),       # the benchmark shape on few rows
          (5, 512, 64, 4),        # every limit at once
          (67, 20, 64, 3)]        # r > D
LARGE_GATE = dict(B=67, D=20, r=8, E=3, gate_scale=400.0)          # scores reach +-1000
SATURATED = dict(B=67, D=20, r=8, E=3, v_scale=40.0)              # |xl V| above 20 in most places


def layer(x0, xl, V, C, U, gate, bias, parts=False):
    """x0, xl [B, D]; V, U [E, D, r]; C [E, r, r]; gate [E, D] or None (E == 1: p = 1); bias [D] -> y [B, D]"""
    v = torch.tanh(torch.einsum("bd,edr->ber", xl, V))
    c = torch.tanh(torch.einsum("ber,ers->bes", v, C))
    u = torch.einsum("ber,edr->bed", c, U) + bias
    if gate is None:
        assert V.shape[0] == 1
        s = xl.new_zeros(xl.shape[0], 1)
        p = torch.ones_like(s)
    else:
        s = xl @ gate.t()
        p = torch.softmax(s, dim=-1)
    y = x0 * torch.einsum("be,bed->bd", p, u) + xl
    return (y, v, c, u, s, p) if parts else y


def inputs(B, D, r, E, gated=True, seed=0, gate_scale=1.0, v_scale=1.0):
    """The float32 inputs of a case on the host: x0, xl, the weights (gate None without one) and the output gradient g."""
    gen = torch.Generator().manual_seed(100000 * E + 1000 * D + 10 * r + 7919 * seed + B)
    rnd = lambda *s: torch.randn(*s, generator=gen)                  # noqa: E731
    out = {"x0": rnd(B, D), "xl": rnd(B, D), "V": rnd(E, D, r) * (v_scale / D ** 0.5), "C": rnd(E, r, r) / r ** 0.5,
           "U": rnd(E, D, r) / r ** 0.5}
    gate = rnd(E, D) * (gate_scale / D ** 0.5)                       # (drawn either way: the other tensors do not depend on `gated`)
    out["gate"] = gate if gated else None
    out["bias"] = rnd(D) * 0.5
    out["g"] = rnd(B, D)
    return out


def reference(x, dtype, same=False):
    """the layer and its autograd gradients on the inputs `x` in `dtype`; same: xl IS x0 (x["xl"] is not read) and dx0 holds the
    whole gradient"""
    v = {k: (None if t is None else t.clone().to(dtype).requires_grad_(k != "g")) for k, t in x.items()}
    xl = v["x0"] if same else v["xl"]
    y, _, _, _, s, p = layer(v["x0"], xl, v["V"], v["C"], v["U"], v["gate"], v["bias"], parts=True)
    y.backward(v["g"])
    out = {"y": y.detach(), "dx0": v["x0"].grad, "dxl": None if same else v["xl"].grad, "dV": v["V"].grad, "dC": v["C"].grad,
           "dU": v["U"].grad, "dgate": None if v["gate"] is None else v["gate"].grad, "dbias": v["bias"].grad,
           "s": s.detach(), "p": p.detach()}
    return out


@functools.lru_cache(maxsize=None)
def case(B, D, r, E, gated=True, seed=0, gate_scale=1.0, v_scale=1.0, same=False):
    """-> (inputs, ref64, ref32).  Cached: treat as read-only."""
    x = inputs(B, D, r, E, gated, seed, gate_scale, v_scale)
    return x, reference(x, torch.float64, same), reference(x, torch.float32, same)


def names_of(x, same=False):
    """the outputs a case has: without a gate there is no dgate, with xl = x0 no dxl"""
    return [n for n in NAMES if (n != "dgate" or x["gate"] is not None) and (n != "dxl" or not same)]


def backward_by_hand(x, g):
    """The header's backward formulas written out (no autograd), in the dtype of x -> {dx0, dxl, dV, dC, dU, dgate, dbias}"""
    x0, xl, V, C, U, gate, bias = (x[k] for k in ("x0", "xl", "V", "C", "U", "gate", "bias"))
    _, v, c, u, _, p = layer(x0, xl, V, C, U, gate, bias, parts=True)
    m = torch.einsum("be,bed->bd", p, u)
    q = g * x0
    dp = torch.einsum("bd,bed->be", q, u)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    du = p.unsqueeze(-1) * q.unsqueeze(1)                                    # [B, E, D]
    dcpre = torch.einsum("bed,edr->ber", du, U) * (1 - c * c)
    dvpre = torch.einsum("bes,ers->ber", dcpre, C) * (1 - v * v)
    out = {"dx0": g * m, "dbias": q.sum(0), "dU": torch.einsum("bed,ber->edr", du, c), "dC": torch.einsum("ber,bes->ers", v, dcpre),
           "dV": torch.einsum("bd,ber->edr", xl, dvpre), "dgate": None}
    dxl = g + torch.einsum("ber,edr->bd", dvpre, V)
    if gate is not None:
        dxl = dxl + ds @ gate
        out["dgate"] = ds.t() @ xl
    out["dxl"] = dxl
    return out


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def cross_mix(P, x0, L, scope="cross_part"):
    xl = x0
    for i in range(L):
        w = [P[f"{scope}/cross_layer_{i}/{n}"] for n in ("V", "C", "U", "gate", "bias")]
        xl = layer(x0, xl, *w)
    return xl


def cross_matrix(P, x0, L, scope="cross_part"):
    xl = x0
    for i in range(L):
        xl = x0 * (xl @ P[f"{scope}/cross_layer_{i}/matrix/kernel"] + P[f"{scope}/cross_layer_{i}/matrix/bias"]) + xl
    return xl


def dcnv2(P, feats, labels, params, training=False):
    """algorithm/DCNV2/dcnv2.py's graph on the variables P -> {"logit", "prob", and with labels "loss"}"""
    from oracle import ref_models as M
    from oracle import ref_ops as O
    cat = M.input_layer(P, feats, params["category_feature_columns"], "category_input/input_layer", {})
    dense_cols = params.get("dense_feature_columns") or []
    x0 = torch.cat([M.input_layer(P, feats, dense_cols, "dense_input/input_layer"), cat], dim=-1) if dense_cols else cat
    L = int(params["num_cross_layer"])
    cross = cross_mix(P, x0, L) if params.get("cross_parameterization", "mix") == "mix" else cross_matrix(P, x0, L)
    stacked = params.get("structure", "parallel") == "stacked"
    dnn = M._mlp(P, cross if stacked else x0, "dnn_part", [f"dnn_dense_{i}" for i in range(len(params["hidden_units"]))])
    output = dnn if stacked else torch.cat([cross, dnn], dim=-1)
    logit = O.dense(output, P["output_part/dense/kernel"], P["output_part/dense/bias"])
    return M._tail(logit, None if labels is None else labels["read_comment"])
