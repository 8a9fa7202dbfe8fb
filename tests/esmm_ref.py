"""Restatement of ESMM (Ma et al., SIGIR 2018) for the tests: the loss tail of include/recalgo_esmm.h, the masked metric counts of
include/recalgo_maskmetrics.h by brute force, and the model of algorithm/ESMM/esmm.py built as tests/mmoe_ref.py builds MMoE's
towers.  TEST INFRASTRUCTURE ONLY: the product path never imports it.  Run in float64 it is the reference the GPU tests compare
against; the same code in float32 is their `ref32` guard (tests/test_esmm_host.py holds it inside assert_close on the host)."""
import functools
import itertools

import numpy as np
import torch

from tests import metrics_ref as MR

EDGE_LOGITS = (-30.0, -8.0, -1.5, 0.0, 0.75, 8.0, 30.0)
ROW_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4099)
NAMES = ("losses", "total", "prob", "d_ctr_logit", "d_cvr_logit")
REDUCED = ("losses", "total")


def sp(x):
    """softplus: max(x, 0) + log1p(exp(-|x|)) — the same values written branch by branch, so that autograd's derivative at
    x == 0 is sigmoid(0) = 0.5 (through max and abs it would be the subgradients 1 and 0: 1.0)"""
    return torch.where(x >= 0, x + torch.log1p(torch.exp(-x)), torch.log1p(torch.exp(x)))


def sigmoid2(x):
    """sigmoid in the two-branch form of csrc/sigmoid_ce.h"""
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def loss_terms(a, b, y, c):
    """the header's arithmetic in the dtype of a -> (L_ctr, L_ctcvr, prob [B, 3], the per-row second term)"""
    z = y * c
    # max(a, 0) - a y + log1p(exp(-|a|)), branch by branch for the same reason as sp
    l_ctr = torch.where(a >= 0, a - a * y + torch.log1p(torch.exp(-a)), -a * y + torch.log1p(torch.exp(a))).mean()
    log_p = -sp(-a) - sp(-b)
    terms = torch.stack([-a, -b, -a - b], dim=1)
    m = terms.max(dim=1).values
    lam = m + torch.log(torch.exp(terms - m[:, None]).sum(dim=1))
    log_1mp = lam + log_p
    rows = -z * log_p - (1 - z) * log_1mp
    p_ctr, p_cvr = sigmoid2(a), sigmoid2(b)
    return l_ctr, rows.mean(), torch.stack([p_ctr, p_cvr, p_ctr * p_cvr], dim=1), rows


def loss(a, b, y, c, dtype=torch.float64, grad_scale=1.0):
    """-> {losses [2], total, prob [B, 3], rows [B], d_ctr_logit [B], d_cvr_logit [B]} in `dtype`, the gradients by autograd"""
    a, b = (t.detach().to(dtype).reshape(-1).clone().requires_grad_(True) for t in (a, b))
    y, c = (t.detach().to(dtype).reshape(-1) for t in (y, c))
    l_ctr, l_ctcvr, prob, rows = loss_terms(a, b, y, c)
    total = l_ctr + l_ctcvr
    da, db = torch.autograd.grad(total * grad_scale, [a, b])
    return {"losses": torch.stack([l_ctr, l_ctcvr]).detach(), "total": total.detach(), "prob": prob.detach(), "rows": rows.detach(),
            "d_ctr_logit": da, "d_cvr_logit": db}


def gradients_by_hand(a, b, y, c):
    """the header's gradient formulas of the second term, written out (no autograd) -> (dl/da, dl/db) per row"""
    z = y * c
    terms = torch.stack([-a, -b, -a - b], dim=1)
    m = terms.max(dim=1).values
    lam = m + torch.log(torch.exp(terms - m[:, None]).sum(dim=1))
    return ((1 - z) * torch.exp(-sp(a) - lam) - z * torch.exp(-sp(a)), (1 - z) * torch.exp(-sp(b) - lam) - z * torch.exp(-sp(b)))


def probability_space_rows(a, b, y, c):
    """what the kernel is NOT: the second term composed from probabilities, -z log p - (1 - z) log(1 - p), in the dtype of a"""
    p = torch.sigmoid(a) * torch.sigmoid(b)
    z = y * c
    return -z * torch.log(p) - (1 - z) * torch.log(1 - p)


@functools.lru_cache(maxsize=None)
def inputs(B, seed=0, sigma=3.0):
    """(a, b, y, c) float32 [B]: logits N(0, sigma), click 30 %, conversion 40 % drawn independently (conversions without a click
    exist).  Cached: treat as read-only."""
    g = torch.Generator().manual_seed(1000 * seed + B)
    a, b = sigma * torch.randn(B, generator=g), sigma * torch.randn(B, generator=g)
    y, c = (torch.rand(B, generator=g) < 0.3).float(), (torch.rand(B, generator=g) < 0.4).float()
    return a, b, y, c


@functools.lru_cache(maxsize=None)
def edge_grid():
    """the 196 rows EDGE_LOGITS^2 x {0, 1}^2 as (a, b, y, c) float32.  Cached: treat as read-only."""
    rows = list(itertools.product(EDGE_LOGITS, EDGE_LOGITS, (0.0, 1.0), (0.0, 1.0)))
    a, b, y, c = (torch.tensor(col, dtype=torch.float32) for col in zip(*rows))
    return a, b, y, c


@functools.lru_cache(maxsize=None)
def case(B, seed=0):
    """-> (inputs, ref64, ref32) of the random case, or of the edge grid for B == "grid".  Cached: treat as read-only."""
    v = edge_grid() if B == "grid" else inputs(B, seed)
    return v, loss(*v, dtype=torch.float64), loss(*v, dtype=torch.float32)


# ---- masked metric counts by brute force ------------------------------------------------------------------------------------------
def takes_part(mask, n):
    """bool [n]: mask None — every row; else mask > 0.5 in float32 (a NaN: no part)"""
    if mask is None:
        return np.ones(n, bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, np.float32).reshape(-1) > np.float32(0.5)


def masked_hist(labels, p, th, mask):
    """[2, N + 1] int64, row by row"""
    labels, p, th = (np.asarray(t, np.float32).reshape(-1) for t in (labels, p, th))
    part = takes_part(mask, len(p))
    h = np.zeros((2, len(th) + 1), np.int64)
    for i in range(len(p)):
        if part[i]:
            with np.errstate(invalid="ignore"):
                h[int(labels[i] > np.float32(0.5)), int((p[i] > th).sum())] += 1
    return h


def masked_accuracy(labels, p, mask):
    """(correct, total) over the rows that take part"""
    labels, p = (np.asarray(t, np.float32).reshape(-1) for t in (labels, p))
    part = takes_part(mask, len(p))
    return int(((labels == p) & part).sum()), int(part.sum())


def mask_kinds(n, seed):
    """name -> float32 [n]: all ones, all zeros, 30 % ones, and one holding NaN, 0.5, its float32 successor and other non-0/1 values"""
    rng = np.random.default_rng([seed, n])
    odd = np.array([np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 1.0, 0.0, -1.0, 2.0, np.inf, -np.inf], np.float32)
    return {"ones": np.ones(n, np.float32), "zeros": np.zeros(n, np.float32), "30 %": (rng.random(n) < 0.3).astype(np.float32),
            "nan": odd[rng.integers(0, len(odd), size=n)]}


thresholds = MR.thresholds


# ---- the model --------------------------------------------------------------------------------------------------------------------
def esmm(P, feats, labels, params, training=False, dropout_masks=None, bn_state=None):
    """algorithm/ESMM/esmm.py's graph on the variables P -> {"logits": {ctr, cvr}, "probs": {ctr, cvr, ctcvr}, and with labels
    "losses": {ctr, ctcvr}, "loss": their sum}.  Tower order dense(relu) -> dropout -> BN, the auto names running on across the two
    towers in one `tower` scope; training-mode dropout takes its keep masks from `dropout_masks` (call order)."""
    from oracle import ref_models as M
    from oracle import ref_ops as R
    masks = list(dropout_masks or [])
    dense_in = M.input_layer(P, feats, params["dense_feature_columns"], "dense_input/input_layer")
    cat = M.input_layer(P, feats, params["category_feature_columns"], "category_input/input_layer", {})
    x = torch.cat([dense_in, cat], dim=-1)
    k, logits = 0, {}
    for task in ("ctr", "cvr"):
        net = x
        for _ in params["hidden_units"]:
            dn = "dense" if k == 0 else f"dense_{k}"
            bn = "batch_normalization" if k == 0 else f"batch_normalization_{k}"
            net = R.dense(net, P[f"tower/{dn}/kernel"], P[f"tower/{dn}/bias"], relu=True)
            net = M._dropout(net, params, training, masks)
            if params.get("batch_norm"):
                net = M._bn(P, net, f"tower/{bn}", training, bn_state)
            k += 1
        logits[task] = R.dense(net, P[f"tower/tower_{task}_logit/kernel"], P[f"tower/tower_{task}_logit/bias"])
    p_ctr, p_cvr = torch.sigmoid(logits["ctr"]), torch.sigmoid(logits["cvr"])
    out = {"logits": logits, "probs": {"ctr": p_ctr, "cvr": p_cvr, "ctcvr": p_ctr * p_cvr}}
    if labels is not None:
        y, c = (labels[params[n]].reshape(-1).to(x.dtype) for n in ("ctr_task_name", "cvr_task_name"))
        l_ctr, l_ctcvr, _, _ = loss_terms(logits["ctr"].reshape(-1), logits["cvr"].reshape(-1), y, c)
        out["losses"] = {"ctr": l_ctr, "ctcvr": l_ctcvr}
        out["loss"] = l_ctr + l_ctcvr
    return out
