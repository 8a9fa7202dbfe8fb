"""DIEN's interest module (algorithm/DIEN/dien.py:196-229, custom_grucell.py, rnn.py:201-219) restated in torch,
dtype-generic: the float64 run is what the GPU tests compare the kernels against, the float32 run the reference arithmetic's
own rounding (`ref32=` of tests/util.assert_close), and the whole model (`dien`) on the oracle's input layers and dense
epilogues.  Never imported by the product path, and imports nothing from it.

What is restated, and where it is easy to go wrong:
  * the cell is TF 1.14's GRUCell: ONE gates product [x, h] Wg + bg split into r (first nh columns) and u (last nh), and the
    reset gate applied BEFORE the candidate's product, c = tanh([x, r * h] Wc + bc) — torch.nn.GRU applies it after;
  * GRU: h' = u h + (1 - u) c.  AGRU: h' = (1 - a) h + a c (u unused).  AUGRU: u' = (1 - a) u, h' = u' h + (1 - u') c;
  * dynamic_rnn's sequence_length: for t >= L the state is copied through and the output row is zero; L is clamped to [0, T];
  * the scores s[b, t] = h[b, t] . (w_att target_b) are REPLACED (tf.where) by float32(-2**32 + 1) for t >= L, the softmax
    runs over all T entries: a replaced entry's weight is exactly 0, an example with L = 0 gets the uniform 1 / T;
  * the second recurrence runs over the rows of h with a_t = att[b, t] and starts from a zero state; `final` is the state
    after step L - 1.
"""
import math

import torch

MASK_VALUE = -4294967296.0        # float32(-2 ** 32 + 1)
GRU, AGRU, AUGRU = 0, 1, 2
CELL_PARAMS = ("Wg", "bg", "Wc", "bc")


def cell(x_t, h, Wg, bg, Wc, bc, mode=GRU, a_t=None):
    """One step: x_t [B, nx], h [B, nh], a_t [B, 1] for modes 1 and 2 -> h' [B, nh]"""
    nh = h.shape[1]
    gates = torch.sigmoid(torch.cat([x_t, h], dim=1) @ Wg + bg)
    r, u = gates[:, :nh], gates[:, nh:]
    c = torch.tanh(torch.cat([x_t, r * h], dim=1) @ Wc + bc)
    if mode == GRU:
        return u * h + (1 - u) * c
    if mode == AGRU:
        return (1 - a_t) * h + a_t * c
    u = (1 - a_t) * u
    return u * h + (1 - u) * c


def recurrence(x, lengths, Wg, bg, Wc, bc, mode=GRU, att=None):
    """dynamic_rnn from a zero state: x [B, T, nx], lengths int [B] or None (all T steps) -> (outputs [B, T, nh], final state)"""
    B, T, _ = x.shape
    nh = bc.shape[0]
    h = x.new_zeros(B, nh)
    # (lengths=None takes the same path with L = T: the same autograd graph, so that gradients are summed in the same order)
    L = torch.full((B,), T, dtype=torch.int64) if lengths is None else lengths.reshape(-1).to(torch.int64).clamp(0, T)
    live = torch.arange(T)[None, :] < L[:, None]
    outs = []
    for t in range(T):
        new = cell(x[:, t], h, Wg, bg, Wc, bc, mode, None if att is None else att[:, t:t + 1])
        m = live[:, t:t + 1]
        h = torch.where(m, new, h)
        outs.append(torch.where(m, new, torch.zeros_like(new)))
    return torch.stack(outs, dim=1), h


def gru(x, lengths, Wg, bg, Wc, bc):
    """h [B, T, nh]"""
    return recurrence(x, lengths, Wg, bg, Wc, bc)[0]


def attention(h, target, lengths, w_att):
    """att [B, T] = softmax over all T of h . (w_att target), the entries t >= L replaced by MASK_VALUE"""
    T = h.shape[1]
    e = target @ w_att.t()                                         # [B, nh]
    s = h[:, :, 0] * e[:, None, 0]                                 # (term by term: the same order whatever T is)
    for j in range(1, h.shape[2]):
        s = s + h[:, :, j] * e[:, None, j]
    dead = torch.arange(T)[None, :] >= lengths.reshape(-1).to(torch.int64).clamp(0, T)[:, None]
    s = torch.where(dead, torch.full_like(s, MASK_VALUE), s)
    # softmax with its sum taken entry by entry: a replaced entry adds an exact 0, so padding T changes no bit of the result
    # (torch.softmax's vectorized sum associates the same entries differently for another T)
    ex = torch.exp(s - s.max(dim=1, keepdim=True).values)
    total = ex[:, 0]
    for t in range(1, T):
        total = total + ex[:, t]
    return ex / total[:, None]


def evolve(h, target, lengths, w_att, Wg, bg, Wc, bc, mode):
    """-> (att [B, T], states [B, T, nh], final [B, nh])"""
    att = attention(h, target, lengths, w_att)
    states, final = recurrence(h, lengths, Wg, bg, Wc, bc, mode, att)
    return att, states, final


# ---- inputs for the kernel tests ---------------------------------------------------------------------------------------------
def random_case(B, T, na, nh, mode, seed, dtype=torch.float64):
    """Inputs of both entry pairs.  The lengths start T, 1, 0 (so every case with B >= 3 holds all three; B = 1 holds T),
    then one above T and random ones.  Every value is an fp32 number.  `h_in`, the evolve pair's input, has zero rows past
    L, as the first recurrence leaves them.  The gru pair's cell reads `x` (Wg, .. of an na-wide input), the evolve pair's
    cell reads h_in (eWg, .. of an nh-wide input)."""
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return ((torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1) * scale).to(torch.float32).to(dtype)
    L = torch.randint(0, T + 1, (B,), generator=gen, dtype=torch.int64)
    for i, v in enumerate((T, 1, 0, T + 3)):
        if i < B:
            L[i] = v
    live = (torch.arange(T)[None, :, None] < L.clamp(0, T)[:, None, None]).to(dtype)

    def glorot(rows, cols):
        return rnd(rows, cols, scale=math.sqrt(6.0 / (rows + cols)))
    return {"mode": mode, "x": rnd(B, T, na), "lengths": L.to(torch.int32), "g_h": rnd(B, T, nh),
            "Wg": glorot(na + nh, 2 * nh), "bg": 1.0 + rnd(2 * nh, scale=0.2), "Wc": glorot(na + nh, nh), "bc": rnd(nh, scale=0.2),
            "h_in": rnd(B, T, nh) * live, "target": rnd(B, na), "w_att": glorot(nh, na), "g_final": rnd(B, nh),
            "eWg": glorot(2 * nh, 2 * nh), "ebg": 1.0 + rnd(2 * nh, scale=0.2), "eWc": glorot(2 * nh, nh), "ebc": rnd(nh, scale=0.2)}


def _leaves(case, names, dtype):
    return {k: case[k].to(dtype).clone().requires_grad_(True) for k in names}


def gru_reference(case, dtype, with_lengths=True):
    """{h, dx, dWg, dbg, dWc, dbc} of loss = sum(h * g_h)"""
    p = _leaves(case, ("x",) + CELL_PARAMS, dtype)
    h = gru(p["x"], case["lengths"] if with_lengths else None, *[p[k] for k in CELL_PARAMS])
    (h * case["g_h"].to(dtype)).sum().backward()
    return {"h": h.detach(), **{"d" + k: v.grad for k, v in p.items()}}


def evolve_reference(case, dtype):
    """{att, states, final, dh, dtarget, dw_att, dWg, dbg, dWc, dbc} of loss = sum(final * g_final)"""
    names = {"h_in": "h", "target": "target", "w_att": "w_att", "eWg": "Wg", "ebg": "bg", "eWc": "Wc", "ebc": "bc"}
    p = _leaves(case, tuple(names), dtype)
    att, states, final = evolve(p["h_in"], p["target"], case["lengths"], p["w_att"], p["eWg"], p["ebg"], p["eWc"], p["ebc"],
                                case["mode"])
    (final * case["g_final"].to(dtype)).sum().backward()
    out = {"att": att.detach(), "states": states.detach(), "final": final.detach()}
    out.update({"d" + names[k]: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()})
    return out


# ---- the whole model ---------------------------------------------------------------------------------------------------------------
def dien(P, feats, labels, params, training=False, dropout_masks=None, bn_state=None, first_gru_lengths=True, pad_to=None):
    """algorithm/DIEN/dien.py:166-254 on the variables P (the reference's names); feats: ids by key, a multi-valued key as
    (values, offsets).  The fcn stack lives INSIDE seq_encoder: dense -> dice | prelu -> BatchNorm -> dropout per hidden unit.
    first_gru_lengths=False runs the first GRU over all T rows, as the reference calls it; pad_to: a static T (the product's
    sequence_max_length) instead of the batch's longest history.  -> {"logit", "prob", and with labels "loss"}"""
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
    seq, seq_len = O.sequence_lookup(vals, offs, table, pad_to)
    s = "seq_encoder/"
    h = gru(seq, seq_len if first_gru_lengths else None, *[P[f"{s}rnn/gru_cell/{n}"] for n in
                                                           ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")])
    mode = AUGRU if params["custom_gru_type"] == "AUGRU" else AGRU
    _, _, final = evolve(h, target, seq_len, P[f"{s}attention_project_matrix"], P[f"{s}rnn/gates/kernel"], P[f"{s}rnn/gates/bias"],
                         P[f"{s}rnn/candidate/kernel"], P[f"{s}rnn/candidate/bias"], mode)
    net = torch.cat([dense_in, category, target, final], dim=-1)
    n = len(params["hidden_units"])
    for i in range(n):
        dn = "dense" if i == 0 else f"dense_{i}"
        net = O.dense(net, P[f"{s}fcn/{dn}/kernel"], P[f"{s}fcn/{dn}/bias"])
        if params["activation"] == "dice":
            net = O.dice(net, P[f"{s}fcn/dice_alpha_{i + 1}"])
        else:
            net = O.prelu(net, P[f"{s}fcn/prelu_alpha_{i + 1}"])
        if params["batch_norm"]:
            bn = "batch_normalization" if i == 0 else f"batch_normalization_{i}"
            net = M._bn(P, net, f"{s}fcn/{bn}", training, bn_state)
        net = M._dropout(net, params, training, masks)
    dn = "dense" if n == 0 else f"dense_{n}"
    logit = O.dense(net, P[f"{s}fcn/{dn}/kernel"], P[f"{s}fcn/{dn}/bias"])
    return M._tail(logit, None if labels is None else labels["read_comment"])


# ---- three LazyAdam steps of the model --------------------------------------------------------------------------------------------
TABLE_KEYS = ("userid", "device", "authorid", "bgm_song_id", "bgm_singer_id", "manual_tag_list")


def touched_rows(name, feats):
    """The rows of embedding table `name` that a batch's IndexedSlices hold: every id the batch looks up there (OOV dropped).
    The shared table is read through the target feed and through the history."""
    keys = ("feedid", "his_read_comment_7d_seq") if "shared_embedding" in name else \
        [k for k in TABLE_KEYS if f"/{k}_embedding/" in name]
    ids = []
    for k in keys:
        v = feats[k]
        ids.append((v[0] if isinstance(v, tuple) else v).reshape(-1).to(torch.int64))
    ids = torch.cat(ids)
    return torch.unique(ids[ids >= 0])


def lazy_adam_trajectory(start, batches, params, lr, dtype=torch.float64, lazy=True, masks=None):
    """`len(batches)` training steps of `dien` from the variables `start` with tf.contrib.opt.LazyAdamOptimizer (dien.py:328):
    oracle.ref_ops.lazy_adam_step on the rows of each embedding table the step's batch touches, adam_tf1_step on every dense
    variable, BatchNorm's moving statistics by assign_moving_average(0.99); lazy=False: tf.train.AdamOptimizer on everything.
    batches: [(feats, labels)].  -> the dict tests/trajectory_ref.bounds reads: loss, grad, v (per step), final, trainable, and
    `touched` [step][table] -> rows."""
    from oracle import ref_ops as O
    P = {k: v.clone().to(dtype) for k, v in start.items()}
    m = {k: torch.zeros_like(v) for k, v in P.items()}
    v_ = {k: torch.zeros_like(v) for k, v in P.items()}
    out = {"loss": [], "grad": [], "v": [], "touched": [], "moving": []}
    for step, (feats, labels) in enumerate(batches, start=1):
        for k, p in P.items():
            p.grad = None
            p.requires_grad_("/moving_" not in k)
        bn = {}
        feats = {k: (x.to(dtype) if isinstance(x, torch.Tensor) and x.is_floating_point() else x) for k, x in feats.items()}
        kw = {"dropout_masks": [x.to(dtype) for x in masks[step - 1]]} if masks and masks[step - 1] else {}
        res = dien(P, feats, {k: y.to(dtype) for k, y in labels.items()}, params, training=True, bn_state=bn, **kw)
        res["loss"].backward()
        out["loss"].append(res["loss"].detach().clone())
        grads = {n: p.grad.detach().clone() for n, p in P.items() if p.grad is not None}
        touched = {}
        with torch.no_grad():
            for n, g in grads.items():
                if lazy and n.endswith("embedding_weights"):
                    rows = touched[n] = touched_rows(n, feats)
                    O.lazy_adam_step(P[n], rows, g[rows], m[n], v_[n], step, lr)
                else:
                    O.adam_tf1_step(P[n], g, m[n], v_[n], step, lr)
            for scope, (mean, var) in bn.items():
                P[f"{scope}/moving_mean"].mul_(0.99).add_(mean, alpha=0.01)
                P[f"{scope}/moving_variance"].mul_(0.99).add_(var, alpha=0.01)
        out["grad"].append(grads)
        out["v"].append({n: v_[n].clone() for n in grads})
        out["touched"].append(touched)
        out["moving"].append({n: p.detach().clone() for n, p in P.items() if "/moving_" in n and "dice_bn" not in n})
    out["final"] = {n: p.detach().clone() for n, p in P.items()}
    out["trainable"] = sorted({n for g in out["grad"] for n in g})
    return out
