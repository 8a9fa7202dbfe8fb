"""numpy restatement of include/recalgo_ragged.h, and the cases its tests share.

    pad(values, capacity)                       recalgo_ragged_pad
    grad_rows(values, offsets, g, g_col, K)     recalgo_bag_mean_grad_rows: rows [len(values), K]
    composition(values, offsets, g)             the torch composition the kernel replaces (what _BagMeanFn.backward ran before
                                                it), on whatever device the tensors live on

np.float32 / np.float32 is the IEEE fp32 division the header states, element by element."""
import numpy as np
import torch


def pad(values: np.ndarray, capacity: int) -> np.ndarray:
    out = np.full(capacity, -1, np.int64)
    out[:len(values)] = values
    return out


def grad_rows(values: np.ndarray, offsets: np.ndarray, g: np.ndarray, g_col: int = 0, K: int = None) -> np.ndarray:
    B, capacity = len(offsets) - 1, len(values)
    K = g.shape[1] - g_col if K is None else K
    rows = np.zeros((capacity, K), np.float32)
    nnz = min(int(offsets[B]), capacity) if B else 0
    for b in range(B):
        lo, hi = int(offsets[b]), min(int(offsets[b + 1]), nnz)
        cnt = np.float32(max(int((values[lo:hi] >= 0).sum()), 1))
        for j in range(lo, hi):
            if values[j] >= 0:
                rows[j] = g[b, g_col:g_col + K].astype(np.float32) / cnt
    return rows


def composition(values: torch.Tensor, offsets: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """rows of the torch composition: searchsorted / arange / index_add_ / clamp / gather / div.  Defined for every entry (an
    entry with an id < 0 and the tail of a padded buffer get a row too: the scatter skipped them by their id)."""
    B = offsets.numel() - 1
    bag = torch.searchsorted(offsets[1:], torch.arange(values.numel(), device=values.device), right=True).clamp_(max=B - 1)
    cnt = torch.zeros(B, device=values.device).index_add_(0, bag, (values >= 0).float()).clamp_(min=1.0)
    return g[bag] / cnt[bag].unsqueeze(1)


def valid_rows(values: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """bool [len(values)]: the entries whose row carries a gradient (below offsets[-1], id >= 0)"""
    ok = values >= 0
    ok[int(offsets[-1]):] = False
    return ok


def bags(B: int, seed: int = 0, vocab: int = 50):
    """-> (values int64 [nnz], offsets int64 [B + 1]) of B bags that hold, wherever B allows: an empty bag, a bag of OOV ids
    only, a bag of one value, a bag of nine values, duplicate ids within a bag, OOV ids among valid ones; the rest random
    lengths 0 .. 5."""
    rng = np.random.default_rng([seed, B])
    fixed = [[], [-1, -1, -1], [7], [3, 3, 9, -1, 9, 3, 11, 12, 13], [5, 5]]
    out = []
    for b in range(B):
        if B >= 5 and b < len(fixed):
            out.append(fixed[b])
        elif B < 5 and b == 0:
            out.append(fixed[3])                 # (B == 1: the bag of nine with duplicates and an OOV id)
        else:
            n = int(rng.integers(0, 6))
            v = rng.integers(0, vocab, n)
            v[rng.random(n) < 0.15] = -1
            out.append(list(v))
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum([len(x) for x in out])
    values = np.array([i for x in out for i in x], np.int64)
    return values, offsets
