"""numpy restatement of FFM's field-aware second-order term (/root/reference algorithm/FFM/ffm.py:146-160) over ids, bags and
tables — what include/recalgo_ffm.h's kernels compute without the operand tensor — and of the de-duplication of a bag
(utils.py:49-64 `to_sparse_tensor`) as plain Python.

    field i owns F - 1 sub-tables [V_i, K]: tables[i] is [F - 1, V_i, K]
    v[b, i, s]   = tables[i][s, id]                      single-valued field, 0 for an id < 0
                 = mean over the bag's distinct ids      bag field, 0 for a bag without a valid id
    out[b]       = sum over i < j of <v[b, i, j - 1], v[b, j, i]>
    gradient row of request (b, a, s) = g[b] * v[b, partner(a, s)], partner = (s + 1, a) when s >= a, else (s, a - 1); for a
    kept bag entry divided by the bag's distinct count, for a dropped one zero.

Every function takes `dtype`: float64 is the reference, float32 the same arithmetic as the reference's own number format
(`ref32` of tests.util.assert_close)."""
import numpy as np


# ---- bags -------------------------------------------------------------------------------------------------------------------------
def distinct(values, offsets):
    """-> (out_values [n], valid [B], distinct [B]): entry j below offsets[B] keeps its id when it is >= 0 and no earlier entry of
    its bag holds it; every other entry — a repeated id, an OOV entry, the tail of a padded Ragged — becomes -1."""
    values, offsets = [int(v) for v in values], [int(o) for o in offsets]
    out = [-1] * len(values)
    valid, kept = [], []
    for b in range(len(offsets) - 1):
        seen = []
        n_valid = 0
        for j in range(offsets[b], offsets[b + 1]):
            if values[j] < 0:
                continue
            n_valid += 1
            if values[j] not in seen:
                seen.append(values[j])
                out[j] = values[j]
        valid.append(n_valid)
        kept.append(len(seen))
    return np.array(out, np.int64).reshape(-1), np.array(valid, np.int32), np.array(kept, np.int32)


def pad(values, capacity):
    out = np.full(capacity, -1, np.int64)
    out[:len(values)] = values
    return out


def make_bags(B, vocab, seed):
    """B bags over [0, vocab) whose first kinds are fixed: an empty bag, an all-OOV one, one id three times, duplicates around an
    OOV entry, 70 values (longer than a wave); the rest hold 0 .. 5 values with repeats and OOV entries."""
    rng = np.random.default_rng([B, vocab, seed])
    fixed = [[], [-1, -1], [3 % vocab] * 3, [1 % vocab, -1, 1 % vocab, 2 % vocab, -1, 2 % vocab],
             list(rng.integers(0, vocab, 70))]
    bags = []
    for b in range(B):
        if b < len(fixed):
            bags.append(fixed[(b + seed) % len(fixed)] if B < len(fixed) else fixed[b])
        else:
            n = int(rng.integers(0, 6))
            bag = rng.integers(0, vocab, n)
            bag[rng.random(n) < 0.15] = -1
            if n >= 2 and rng.random() < 0.4:
                bag[n - 1] = bag[0]
            bags.append(list(bag))
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum([len(b) for b in bags])
    values = np.array([v for b in bags for v in b], np.int64).reshape(-1)
    return values, offsets


# ---- a problem ----------------------------------------------------------------------------------------------------------------------
def problem(B, F, K, bag_fields=(), seed=0, oov=0.1):
    """ids [B, n_single] (-1: OOV), bags {field: (values, offsets)}, tables [F] of [F - 1, V_i, K] float32, vocab [F], g [B]"""
    rng = np.random.default_rng([B, F, K, seed, len(bag_fields)])
    vocab = [int(v) for v in rng.integers(3, 12, F)]
    tables = [rng.standard_normal((F - 1, v, K)).astype(np.float32) for v in vocab]
    single = [i for i in range(F) if i not in bag_fields]
    ids = np.stack([rng.integers(0, vocab[i], B) for i in single], 1).astype(np.int64) if single else None
    if single:
        ids[rng.random(ids.shape) < oov] = -1
        if B > 1:
            ids[rng.integers(B), rng.integers(len(single))] = -1             # (at least one OOV id, whatever the draw)
    bags = {i: make_bags(B, vocab[i], seed + i) for i in bag_fields}
    g = rng.standard_normal(B).astype(np.float32)
    return dict(B=B, F=F, K=K, vocab=vocab, tables=tables, single=single, ids=ids, bags=bags, g=g)


def rows(p, dtype=np.float64):
    """v [B, F, F - 1, K]"""
    B, F, K = p["B"], p["F"], p["K"]
    v = np.zeros((B, F, F - 1, K), dtype)
    for c, i in enumerate(p["single"]):
        t = p["tables"][i].astype(dtype)
        for b in range(B):
            if p["ids"][b, c] >= 0:
                v[b, i] = t[:, p["ids"][b, c]]
    for i, (values, offsets) in p["bags"].items():
        t = p["tables"][i].astype(dtype)
        kept, _, n = distinct(values, offsets)
        for b in range(B):
            acc = np.zeros((F - 1, K), dtype)
            for j in range(int(offsets[b]), int(offsets[b + 1])):        # (bag order; the reference sums ascending: an fp32 reordering)
                if kept[j] >= 0:
                    acc = acc + t[:, kept[j]]
            if n[b]:
                v[b, i] = acc / dtype(n[b])
    return v


def out(p, dtype=np.float64):
    """[B]: ffm.py:146-160, the pairs in the reference's loop order"""
    v = rows(p, dtype)
    F = p["F"]
    acc = np.zeros(p["B"], dtype)
    for i in range(F - 1):
        for j in range(i + 1, F):
            acc = acc + (v[:, i, j - 1] * v[:, j, i]).sum(-1, dtype=dtype)
    return acc


def partner(a, s):
    return (s + 1, a) if s >= a else (s, a - 1)


def grad_rows(p, dtype=np.float64, capacity=None):
    """-> (d_single [B, n_single (F - 1) K] or None, {field: d_rows [capacity, (F - 1) K]}): the rows the scatter's sources get"""
    v = rows(p, dtype)
    B, F, K = p["B"], p["F"], p["K"]
    g = p["g"].astype(dtype)
    d = np.zeros((B, F, F - 1, K), dtype)                  # g[b] * partner row, per (field, sub-table)
    for a in range(F):
        for s in range(F - 1):
            pa, ps = partner(a, s)
            d[:, a, s] = g[:, None] * v[:, pa, ps]
    d_single = d[:, p["single"]].reshape(B, -1) if p["single"] else None
    d_bags = {}
    for i, (values, offsets) in p["bags"].items():
        kept, _, n = distinct(values, offsets)
        cap = len(values) if capacity is None else capacity[i]
        r = np.zeros((cap, F - 1, K), dtype)
        for b in range(B):
            for j in range(int(offsets[b]), int(offsets[b + 1])):
                if kept[j] >= 0:
                    r[j] = (g[b] / dtype(n[b])) * v[b].reshape(F, F - 1, K)[[partner(i, s)[0] for s in range(F - 1)],
                                                                           [partner(i, s)[1] for s in range(F - 1)]]
        d_bags[i] = r.reshape(cap, -1)
    return d_single, d_bags


def table_grads(p, dtype=np.float64):
    """[F] of [F - 1, V_i, K]: the request rows summed per table row"""
    d_single, d_bags = grad_rows(p, dtype)
    B, F, K = p["B"], p["F"], p["K"]
    grads = [np.zeros(t.shape, dtype) for t in p["tables"]]
    for c, i in enumerate(p["single"]):
        r = d_single.reshape(B, len(p["single"]), F - 1, K)[:, c]
        for b in range(B):
            if p["ids"][b, c] >= 0:
                grads[i][:, p["ids"][b, c]] += r[b]
    for i, (values, offsets) in p["bags"].items():
        kept = distinct(values, offsets)[0]
        r = d_bags[i].reshape(len(values), F - 1, K)
        for j in range(int(offsets[-1])):
            if kept[j] >= 0:
                grads[i][:, kept[j]] += r[j]
    return grads
