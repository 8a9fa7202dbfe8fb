"""AutoInt's interacting layer (include/recalgo_autoint.h; Song et al., CIKM 2019, eqs. 5-8) restated in torch, differentiated by
autograd, in float64 (the yardstick) or float32 (the arithmetic's own rounding); results are computed once per case and shared.
The upstream zoo has no AutoInt file, so this restatement is the reference.  Also the whole model as a function of named
variables (algorithm/AutoInt/autoint.py's graph) for the step tests."""
import functools

import torch

NAMES = ("y", "dx", "dwq", "dwk", "dwv", "dwres")
REDUCED = ("dwq", "dwk", "dwv", "dwres")

# (B, F, D, A, H, res): the shapes of the GPU parity tests (tests/test_gpu_autoint.py); tests/test_autoint_host.py holds the
# float32 restatement alone to the same bound on every one of them
SHAPES = [(1, 2, 4, 4, 1, True),          # the smallest of everything
          (5, 3, 8, 4, 3, True),          # H A = 12, three heads
          (3, 16, 8, 8, 2, True),         # F exactly one tile
          (3, 17, 12, 8, 2, True),        # one row into the second tile, D = 12
          (130, 7, 8, 8, 2, True),        # the dataset's shape; B does not fill its last workgroup
          (67, 7, 16, 8, 2, True),        # a later layer of the default stack
          (67, 9, 16, 8, 2, False),       # no residual term
          (33, 26, 16, 8, 2, True),       # the benchmark shape
          (9, 26, 16, 32, 2, True),       # the paper's first layer
          (5, 26, 64, 32, 2, True),       # the paper's later layers
          (3, 64, 8, 4, 4, True),         # F and H at their limits
          (3, 33, 4, 32, 1, True)]        # A at its limit
LARGE = dict(B=67, F=9, D=16, A=8, H=2, res=True, x_scale=3.0, qk_scale=3.0)      # scores reach +-1600


def layer(x, wq, wk, wv, wres=None, return_scores=False):
    """x [B, F, D], wq / wk / wv [H, D, A], wres [D, H A] or None -> y [B, F, H A] (head-major columns)"""
    B, F, _ = x.shape
    H, _, A = wq.shape
    q, k, v = (torch.einsum("bfd,hda->bhfa", x, w) for w in (wq, wk, wv))
    s = q @ k.transpose(-1, -2)                                      # [B, H, F, F], no scaling
    p = torch.softmax(s, dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B, F, H * A)
    if wres is not None:
        o = o + x @ wres
    y = torch.relu(o)
    return (y, s, p) if return_scores else y


def inputs(B, F, D, A, H, res=True, seed=0, x_scale=1.0, qk_scale=1.0):
    """The float32 inputs of a case on the host: x [B, F, D], wq, wk, wv, wres (None without the residual term) and the output
    gradient g [B, F, H A]."""
    gen = torch.Generator().manual_seed(100000 * F + 1000 * D + 10 * A + H + 7919 * seed + B)
    rnd = lambda *s: torch.randn(*s, generator=gen)                  # noqa: E731
    out = {"x": rnd(B, F, D) * x_scale, "wq": rnd(H, D, A) * (qk_scale / D ** 0.5), "wk": rnd(H, D, A) * (qk_scale / D ** 0.5),
           "wv": rnd(H, D, A) / D ** 0.5}
    wres = rnd(D, H * A) / D ** 0.5                                  # (drawn either way: the other tensors do not depend on `res`)
    out["wres"] = wres if res else None
    out["g"] = rnd(B, F, H * A)
    return out


def reference(x, dtype):
    """the layer and its autograd gradients on the inputs `x` in `dtype` -> {y, dx, dwq, dwk, dwv, dwres (None without), s, p}"""
    v = {k: (None if t is None else t.clone().to(dtype).requires_grad_(k != "g")) for k, t in x.items()}
    y, s, p = layer(v["x"], v["wq"], v["wk"], v["wv"], v["wres"], return_scores=True)
    y.backward(v["g"])
    return {"y": y.detach(), "dx": v["x"].grad, "dwq": v["wq"].grad, "dwk": v["wk"].grad, "dwv": v["wv"].grad,
            "dwres": None if v["wres"] is None else v["wres"].grad, "s": s.detach(), "p": p.detach()}


@functools.lru_cache(maxsize=None)
def case(B, F, D, A, H, res=True, seed=0, x_scale=1.0, qk_scale=1.0):
    """-> (inputs, ref64, ref32).  Cached: treat as read-only."""
    x = inputs(B, F, D, A, H, res, seed, x_scale, qk_scale)
    return x, reference(x, torch.float64), reference(x, torch.float32)


def names_of(x):
    """the outputs a case has: without the residual term there is no dwres"""
    return [n for n in NAMES if n != "dwres" or x["wres"] is not None]


def backward_by_hand(x, g):
    """The header's backward formulas written out (no autograd), in the dtype of x -> {dx, dwq, dwk, dwv, dwres}"""
    xs, wq, wk, wv, wres = x["x"], x["wq"], x["wk"], x["wv"], x["wres"]
    B, F, D = xs.shape
    H, _, A = wq.shape
    y, s, p = layer(xs, wq, wk, wv, wres, return_scores=True)
    dz = g * (y > 0).to(g.dtype)                                     # [B, F, H A]
    dzh = dz.reshape(B, F, H, A).permute(0, 2, 1, 3)                 # [B, H, F, A]
    q, k, v = (torch.einsum("bfd,hda->bhfa", xs, w) for w in (wq, wk, wv))
    dv = p.transpose(-1, -2) @ dzh
    dp = dzh @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dq, dk = ds @ k, ds.transpose(-1, -2) @ q
    dx = sum(torch.einsum("bhfa,hda->bfd", d, w) for d, w in ((dq, wq), (dk, wk), (dv, wv)))
    out = {"dwq": torch.einsum("bfd,bhfa->hda", xs, dq), "dwk": torch.einsum("bfd,bhfa->hda", xs, dk),
           "dwv": torch.einsum("bfd,bhfa->hda", xs, dv), "dwres": None}
    if wres is not None:
        dx = dx + dz @ wres.t()
        out["dwres"] = torch.einsum("bfd,bfc->dc", xs, dz)
    out["dx"] = dx
    return out


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def layer_variables(P, i, use_res, scope="interacting_part"):
    w = [P[f"{scope}/interacting_layer_{i}_w_{n}"] for n in ("query", "key", "value")]
    return w + [P[f"{scope}/interacting_layer_{i}_w_res"] if use_res else None]


def autoint(P, feats, labels, params, training=False, bn_state=None):
    """algorithm/AutoInt/autoint.py's graph on the variables P -> {"logit", "prob", and with labels "loss"}"""
    from oracle import ref_models as M
    from oracle import ref_ops as O
    dense_in = M.input_layer(P, feats, params["dense_feature_columns"], "dense_input/input_layer")
    logit = O.dense(dense_in, P["dense_input/dense_logit/kernel"], P["dense_input/dense_logit/bias"])
    cols = params["category_feature_columns"]
    parts = [M.input_layer(P, feats, [c], "interacting_part/input_layer" + ("" if i == 0 else f"_{i}"), {})
             for i, c in enumerate(cols)]                            # one input_layer per column, list order
    fields = torch.cat(parts, dim=1)
    B, F = fields.shape[0], len(cols)
    x = fields.reshape(B, F, -1)
    for i in range(int(params["num_interacting_layers"])):
        x = layer(x, *layer_variables(P, i, bool(params["use_residual"])))
    logit = logit + O.dense(x.reshape(B, -1), P["prediction_part/autoint_logit/kernel"], P["prediction_part/autoint_logit/bias"])
    hidden = [int(u) for u in params.get("hidden_units") or []]
    if hidden:
        net = fields
        for i, _ in enumerate(hidden):
            sfx = "" if i == 0 else f"_{i}"
            net = M._mlp(P, net, "deep_part", [f"dense{sfx}"])
            if params.get("batch_norm"):
                net = M._bn(P, net, f"deep_part/batch_normalization{sfx}", training, bn_state)
        logit = logit + O.dense(net, P["deep_part/deep_logit/kernel"], P["deep_part/deep_logit/bias"])
    return M._tail(logit, None if labels is None else labels["read_comment"])
