"""Restatements the Wide&Deep tests compare against — TEST INFRASTRUCTURE ONLY: the product path never imports this file.

  * the crossed column's hash (TF 1.14 sparse_cross_op.cc HashCrosser over int64 inputs with core/platform/fingerprint.h
    FingerprintCat64, as include/recalgo_wide.h states it) twice: on Python integers and on numpy uint64;
  * tf.train.FtrlOptimizer's ApplyFtrl with its defaults (initial_accumulator_value 0.1, l1 = l2 = 0, lr_power -0.5), dense
    and sparse (touched buckets + the step-1 zeroing);
  * the reference's Wide&Deep forward (algorithm/WideAndDeep/wide_and_deep.py:194-240) for (variables by TF name, encoded
    features, labels, params), in the style of tests/ple_ref.py.  Run in float64 it is the reference the GPU tests compare
    against (pinned to the goldens by tests/test_wdl_host.py); run in float32 it is their `ref32` guard.

None of this was checked against TensorFlow (there is none where the project is authored): the hash and FTRL are written
from knowledge of the TF sources named above."""
import numpy as np
import torch

from oracle import ref_models as M
from oracle import ref_ops as R

HASH_KEY = 0xDECAFCAFFE
K_MUL = 0xc6a4a7935bd1e995
MASK = (1 << 64) - 1
FTRL_INITIAL_ACCUMULATOR = 0.1

# (u, t) -> full hash: the issue's known answers, computed with Python integers
KNOWN_ANSWERS = {(0, 0): 7883058887674371304, (1, 2): 5036120653031601357, (12345, 67): 11264971086424720464,
                 (-1, 3): 8470749512028849339, (7, -1): 3850899422564833121, (2147483647, 349): 4482412670132046439}


# ---- the hash, on Python integers ---------------------------------------------------------------------------------------
def _shift_mix(v):
    return v ^ (v >> 47)


def cat64_py(a, b):
    r = a ^ K_MUL
    r ^= (_shift_mix((b * K_MUL) & MASK) * K_MUL) & MASK
    r = (r * K_MUL) & MASK
    r = (_shift_mix(r) * K_MUL) & MASK
    return _shift_mix(r)


def cross_hash_py(u, t, hash_key=HASH_KEY):
    """ids are crossed as their int64 value: -1 is 0xFFFFFFFFFFFFFFFF"""
    return cat64_py(cat64_py(hash_key & MASK, int(u) & MASK), int(t) & MASK)


# ---- the hash, on numpy uint64 (wrapping arithmetic) ----------------------------------------------------------------------
def cat64_np(a, b):
    k = np.uint64(K_MUL)
    s = np.uint64(47)
    with np.errstate(over="ignore"):
        r = a ^ k
        m = b * k
        r = r ^ ((m ^ (m >> s)) * k)
        r = r * k
        r = (r ^ (r >> s)) * k
        return r ^ (r >> s)


def cross_hash_np(u, t, hash_key=HASH_KEY):
    u = np.asarray(u, dtype=np.int64).astype(np.uint64)
    t = np.asarray(t, dtype=np.int64).astype(np.uint64)
    return cat64_np(cat64_np(np.full_like(u, np.uint64(hash_key)), u), t)


def requests(user_ids, values, offsets):
    """-> (example [n], user [n], tag [n]) int64 arrays: one request per (example, entry of its bag), in bag order"""
    user_ids, values, offsets = (np.asarray(x, dtype=np.int64) for x in (user_ids, values, offsets))
    lens = offsets[1:] - offsets[:-1]
    ex = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    n = int(offsets[-1])
    return ex, user_ids[ex], values[:n]


def buckets(user_ids, values, offsets, hash_bucket_size, hash_key=HASH_KEY):
    """-> (example [n] int64, bucket [n] int64)"""
    ex, u, t = requests(user_ids, values, offsets)
    return ex, (cross_hash_np(u, t, hash_key) % np.uint64(hash_bucket_size)).astype(np.int64)


# ---- FTRL -------------------------------------------------------------------------------------------------------------------
def ftrl_dense(var, accum, linear, g, lr, l1=0.0, l2=0.0):
    """TF's ApplyFtrl (lr_power = -0.5) on whole tensors, out of place -> (var, accum, linear)"""
    new_accum = accum + g * g
    linear = linear + g - (new_accum.sqrt() - accum.sqrt()) / lr * var
    quad = new_accum.sqrt() / lr + 2 * l2
    var = torch.where(linear.abs() > l1, (torch.sign(linear) * l1 - linear) / quad, torch.zeros_like(linear))
    return var, new_accum, linear


def ftrl_sparse(var, accum, linear, touched, g_touched, lr, first_step, l1=0.0, l2=0.0):
    """What the library does: the update of the `touched` buckets (int64 indices, unique; g_touched their gradients), and on
    the first step the zeroing of every other bucket.  Out of place -> (var, accum, linear)."""
    var, accum, linear = var.clone(), accum.clone(), linear.clone()
    if first_step:
        keep = torch.zeros_like(var, dtype=torch.bool)
        keep[touched] = True
        var = torch.where(keep, var, torch.zeros_like(var))
    v, a, l = ftrl_dense(var[touched], accum[touched], linear[touched], g_touched, lr, l1, l2)
    var[touched], accum[touched], linear[touched] = v, a, l
    return var, accum, linear


# ---- the wide part and the model -------------------------------------------------------------------------------------------
def wide_logit(kernel, bias, user_ids, values, offsets, hash_bucket_size, hash_key=HASH_KEY):
    """tf.layers.dense(indicator(crossed), 1): bias + the sum of kernel[bucket] over the example's requests -> [B, 1]"""
    ex, bk = buckets(user_ids, values, offsets, hash_bucket_size, hash_key)
    B = len(np.asarray(offsets)) - 1
    out = torch.zeros(B, dtype=kernel.dtype)
    if len(bk):
        out = out.index_add(0, torch.from_numpy(ex), kernel.reshape(-1)[torch.from_numpy(bk)])
    return (out + (bias.reshape(()) if bias is not None else 0.0)).reshape(B, 1)


WIDE_KERNEL = "wide_part/wide_part_variables/kernel"
WIDE_BIAS = "wide_part/wide_part_variables/bias"


def wide_and_deep(P, feats, labels, params, training=False, dropout_masks=None):
    """-> {"wide_logit", "deep_logit", "logit", "prob", and with labels "loss"}; feats: ids by key, a multi-valued key as
    (values, offsets); dense(relu) -> dropout -> BN per hidden unit (wide_and_deep.py:216-221)."""
    masks = list(dropout_masks or [])
    crossed = params["wide_part_feature_columns"][0].categorical_column
    ukey, tkey = [c.key for c in crossed.keys]
    tv, to = feats[tkey]
    wl = wide_logit(P[WIDE_KERNEL], P[WIDE_BIAS], feats[ukey], tv, to, crossed.hash_bucket_size)
    net = M.input_layer(P, feats, params["deep_part_feature_columns"], "deep_part/input_layer", {})
    for k in range(len(params["hidden_units"])):
        dn = "dense" if k == 0 else f"dense_{k}"
        bn = "batch_normalization" if k == 0 else f"batch_normalization_{k}"
        net = R.dense(net, P[f"deep_part/{dn}/kernel"], P[f"deep_part/{dn}/bias"], relu=True)
        net = M._dropout(net, params, training, masks)
        if params.get("batch_norm"):
            net = R.batch_norm(net, P[f"deep_part/{bn}/gamma"], P[f"deep_part/{bn}/beta"], P[f"deep_part/{bn}/moving_mean"],
                               P[f"deep_part/{bn}/moving_variance"], training)
    k = len(params["hidden_units"])
    dl = R.dense(net, P[f"deep_part/dense_{k}/kernel" if k else "deep_part/dense/kernel"],
                 P[f"deep_part/dense_{k}/bias" if k else "deep_part/dense/bias"])
    logit = wl + dl
    out = {"wide_logit": wl, "deep_logit": dl, "logit": logit, "prob": torch.sigmoid(logit)}
    if labels is not None:
        out["loss"] = R.ce_loss(labels["read_comment"], logit)
    return out


def encode(params, sfeats):
    """string features -> the restatement's feature batch (ids; (values, offsets) for multi-valued keys), through the
    mirror's own columns; the crossed column's base columns included"""
    from recalgorithm_amd.feature_column import CrossedColumn, NumericColumn, Ragged
    feats, cats = {}, []
    for c in list(params["wide_part_feature_columns"]) + list(params["deep_part_feature_columns"]):
        if isinstance(c, NumericColumn):
            feats[c.key] = sfeats[c.key].double()
        elif isinstance(c.categorical_column, CrossedColumn):
            cats += list(c.categorical_column.keys)
        else:
            cats.append(c.categorical_column)
    for cat in cats:
        x = cat.ids({cat.key: sfeats[cat.key]}, torch.device("cpu"))
        feats[cat.key] = (x.values, x.offsets) if isinstance(x, Ragged) else x
    return feats
