"""BST's transformer block (algorithm/BST/transformer_layer.py:6-81, bst.py:183-198) restated in torch, dtype-generic: the
float64 run is what the GPU tests compare the kernels against, the float32 run the reference arithmetic's own rounding
(`ref32=` of tests/util.assert_close).  Never imported by the product path.

What is restated, and where it is easy to go wrong:
  * Xp = X + position_embedding[0:T]; Q and K are projected from Xp, V from X; the residual is Xp;
  * scores = Q_h K_h^T / float32(sqrt(d)): a division by the fp32 value;
  * the mask is on the QUERY axis: float32(-2**32 + 1) = -4294967296.0 is added to whole rows i >= keys_length.  In fp32 the
    add absorbs every |s| < 128, so such a row's softmax is exactly uniform and the add's gradient (the identity) still
    reaches Q and K.  The float64 run models that fp32 step, not float64 arithmetic: `s + (c - s).detach()` on those rows
    (a straight-through constant);
  * tf.contrib.layers.layer_norm defaults: begin_norm_axis=1 (moments per example over the whole [T, d] block, padded rows
    included), begin_params_axis=-1 (gamma, beta of shape [d]), variance epsilon 1e-12, tf.nn.moments /
    tf.nn.batch_normalization arithmetic.  No TensorFlow exists where this was written to confirm these defaults: they
    are restated from the TF 1.15 sources of tensorflow/contrib/layers/python/layers/layers.py;
  * leakyrelu(x) = 0.505 x + 0.495 |x| (algorithm/BST/leakyrelu.py); pooling over ALL T rows.
"""
import math

import torch

MASK_ADD = -4294967296.0        # float32(-2 ** 32 + 1)
LN_EPS = 1e-12


def layer_norm(x, gamma, beta, eps=LN_EPS):
    """x [B, T, d]; moments over (T, d) per example; gamma, beta [d]"""
    mean = x.mean(dim=(1, 2), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(1, 2), keepdim=True)
    inv = torch.rsqrt(var + eps) * gamma
    return x * inv + (beta - mean * inv)


def masked_rows(keys_length, T):
    """[B, 1, T, 1] bool: the query rows >= keys_length (clamped to [0, T])"""
    kl = keys_length.reshape(-1).to(torch.int64).clamp(0, T)
    return (torch.arange(T)[None, :] >= kl[:, None])[:, None, :, None]


def add_mask(s, keys_length):
    """s [B, H, T, T] + the query-row mask: the literal add in float32, its straight-through model in any other dtype"""
    rows = masked_rows(keys_length, s.shape[-1])
    if s.dtype == torch.float32:
        return s + rows.to(s.dtype) * torch.tensor(MASK_ADD, dtype=torch.float32)
    # the straight-through constant s + (c - s).detach(), written so that the VALUE is exactly c also in float64 (c - s is
    # rounded at the magnitude of c, 1e-6 absolute: s + (c - s) would leave the rows unequal at that level)
    return torch.where(rows, MASK_ADD + (s - s.detach()), s)


def probabilities(x, keys_length, pos, w_q, w_k):
    """-> (softmax [B, H, T, T], Q, K)"""
    T, d = x.shape[1], x.shape[2]
    xp = x + pos[:T]
    q = torch.einsum("bik,hkj->bhij", xp, w_q)
    k = torch.einsum("bik,hkj->bhij", xp, w_k)
    scale = torch.tensor(math.sqrt(d), dtype=torch.float32).to(x.dtype)
    s = add_mask(q @ k.transpose(-1, -2) / scale, keys_length)
    return torch.softmax(s, dim=-1), q, k


def attention(x, keys_length, pos, w_q, w_k, w_v, w_o, gamma, beta):
    """n1 [B, T, d] = LayerNorm(concat_heads(softmax(scores + mask) V) w_o + Xp)"""
    B, T, d = x.shape
    H = w_q.shape[0]
    p, _, _ = probabilities(x, keys_length, pos, w_q, w_k)
    v = torch.einsum("bik,hkj->bhij", x, w_v)
    heads = (p @ v).permute(0, 2, 1, 3).reshape(B, T, H * d)
    return layer_norm(heads @ w_o + (x + pos[:T]), gamma, beta)


def leakyrelu(x):
    return 0.505 * x + 0.495 * x.abs()


def ffn(n1, w, b, gamma, beta):
    """out [B, T, d] = LayerNorm(leakyrelu(n1 W + b) + n1)"""
    return layer_norm(leakyrelu(n1 @ w + b) + n1, gamma, beta)


def pool(out, method):
    return out.sum(dim=1) if method == "sum" else out.mean(dim=1)


def block(x, keys_length, P, index, ln_first):
    """One bst_transformer call on the variables P (names without the scope): w_q_<i>, .., LayerNorm*, dense*"""
    def suffix(base, n):
        return base if n == 0 else f"{base}_{n}"
    ln1, ln2, dn = suffix("LayerNorm", ln_first), suffix("LayerNorm", ln_first + 1), suffix("dense", index)
    n1 = attention(x, keys_length, P["position_embedding"], P[f"w_q_{index}"], P[f"w_k_{index}"], P[f"w_v_{index}"],
                   P[f"w_o_{index}"], P[f"{ln1}/gamma"], P[f"{ln1}/beta"])
    return ffn(n1, P[f"{dn}/kernel"], P[f"{dn}/bias"], P[f"{ln2}/gamma"], P[f"{ln2}/beta"])


def transformer_part(x, keys_length, P, blocks, pooling):
    """bst.py:183-198 on P = the variables of scope transformer_part (names without the scope)"""
    out = x
    for i in range(blocks):
        out = block(out, keys_length, P, i, 2 * i)
    return pool(out, pooling)


# ---- inputs for the kernel tests ---------------------------------------------------------------------------------------------
def random_case(B, T, d, H, seed, dtype=torch.float64):
    """Inputs of one block with |scores| well below 128 and no constant [T, d] block; keys_length mixes 0, 1, T, values above
    T and random ones; padded rows of x are zero, as sequence_input_layer leaves them."""
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return ((torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1) * scale).to(torch.float32).to(dtype)
    kl = torch.randint(0, T + 1, (B,), generator=gen, dtype=torch.int64)
    for i, v in enumerate((0, 1, T, T + 3, 2 * T + 1)):
        if i < B:
            kl[(i * 7) % B] = v
    if B == 1:
        kl[0] = max(T - 1, 1)
    x = rnd(B, T, d)
    x = x * (torch.arange(T)[None, :, None] < kl.clamp(0, T)[:, None, None]).to(dtype)
    lim = math.sqrt(6.0 / (2 * d))
    case = {"x": x, "keys_length": kl.to(torch.int32), "pos": rnd(T + 2, d, scale=0.5),
            "w_q": rnd(H, d, d, scale=lim), "w_k": rnd(H, d, d, scale=lim), "w_v": rnd(H, d, d, scale=lim),
            "w_o": rnd(H * d, d, scale=math.sqrt(6.0 / (H * d + d))), "gamma": 1.0 + rnd(d, scale=0.3), "beta": rnd(d, scale=0.3),
            "ffn_w": rnd(d, d, scale=lim), "ffn_b": rnd(d, scale=0.2), "gamma2": 1.0 + rnd(d, scale=0.3), "beta2": rnd(d, scale=0.3),
            "g_n1": rnd(B, T, d), "g_out": rnd(B, T, d), "g_pool": rnd(B, d)}
    return case


ATTN_PARAMS = ("pos", "w_q", "w_k", "w_v", "w_o", "gamma", "beta")
FFN_PARAMS = ("ffn_w", "ffn_b", "gamma2", "beta2")


def attention_reference(case, dtype):
    """-> {n1, dx, d<param>}: the attention half and its gradients for the upstream gradient case["g_n1"], in `dtype`"""
    c = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in case.items()}
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("x",) + ATTN_PARAMS}
    n1 = attention(leaves["x"], c["keys_length"], *[leaves[k] for k in ATTN_PARAMS])
    n1.backward(c["g_n1"])
    out = {"n1": n1.detach()}
    out.update({"d" + k: leaves[k].grad for k in leaves})
    return out


def ffn_reference(case, n1, dtype, pooling, use_out=True, use_pool=True):
    """-> {out, pool, dn1, d<param>} of the FFN half on `n1`, the loss being <out, g_out> (use_out) + <pool, g_pool> (use_pool)"""
    c = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in case.items()}
    leaves = {k: c[k].clone().requires_grad_(True) for k in FFN_PARAMS}
    n1 = n1.to(dtype).clone().requires_grad_(True)
    out = ffn(n1, *[leaves[k] for k in FFN_PARAMS])
    pl = pool(out, pooling)
    loss = (out * c["g_out"]).sum() * (1.0 if use_out else 0.0) + (pl * c["g_pool"]).sum() * (1.0 if use_pool else 0.0)
    loss.backward()
    res = {"out": out.detach(), "pool": pl.detach(), "dn1": n1.grad}
    res.update({"d" + k: leaves[k].grad for k in leaves})
    return res


# ---- the whole model ---------------------------------------------------------------------------------------------------------------
def bst(P, feats, labels, params, training=False, dropout_masks=None, bn_state=None):
    """algorithm/BST/bst.py:151-226 on the variables P (the reference's names); feats: ids by key, a multi-valued key as
    (values, offsets).  The tower is dense (no activation) -> BatchNorm -> dropout per hidden unit (:204-209).
    -> {"logit", "prob", and with labels "loss"}"""
    from oracle import ref_models as M
    from oracle import ref_ops as O
    masks = list(dropout_masks or [])
    reg = {}
    dense_in = M.input_layer(P, feats, params["dense_feature_columns"], "dense_input/input_layer")
    category = M.input_layer(P, feats, params["category_feature_columns"], "category_input/input_layer", reg)
    tcol, scol = params["target_feedid_feature_columns"][0], params["sequence_feature_columns"][0]
    table = P[reg.setdefault(tcol.shared_name, M.table_name(tcol, "target_input/sequence_input_layer"))]
    tid = feats[tcol.key]
    if isinstance(tid, tuple):               # a sequence column over a single-valued key: one id per example
        assert bool((tid[1][1:] - tid[1][:-1] == 1).all())
        tid = tid[0]
    target = O.embedding_lookup_single(tid.reshape(-1), table)
    vals, offs = feats[scol.key]
    static_T = int(params["sequence_max_length"]) if params.get("static_sequence_length") else None
    seq, seq_len = O.sequence_lookup(vals, offs, table, static_T)
    x = torch.cat([target[:, None, :], seq], dim=1)
    scope = "transformer_part/"
    pooled = transformer_part(x, seq_len + 1, {k[len(scope):]: v for k, v in P.items() if k.startswith(scope)},
                              int(params["num_transformer_block"]), params["pooling_method"])
    net = torch.cat([dense_in, category, pooled], dim=-1)
    n = len(params["hidden_units"])
    for i in range(n):
        dn = "dense" if i == 0 else f"dense_{i}"
        net = O.dense(net, P[f"dnn_part/{dn}/kernel"], P[f"dnn_part/{dn}/bias"])
        if params["batch_norm"]:
            bn = "batch_normalization" if i == 0 else f"batch_normalization_{i}"
            net = M._bn(P, net, f"dnn_part/{bn}", training, bn_state)
        net = M._dropout(net, params, training, masks)
    dn = "dense" if n == 0 else f"dense_{n}"
    logit = O.dense(net, P[f"dnn_part/{dn}/kernel"], P[f"dnn_part/{dn}/bias"])
    return M._tail(logit, None if labels is None else labels["read_comment"])
