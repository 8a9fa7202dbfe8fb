"""The bin rule of include/recalgo_metrics.h restated in numpy, the edge inputs of its tests, and the state buffer's layout.

    bin(p) = #{j : p > th[j]}   compared in float32; a NaN compares false everywhere: bin 0
    hist[y][bin] += 1           y = label > 0.5

No device, no product code: tests/test_metrics_host.py holds it against AUCMetric.update, tests/test_gpu_metrics.py holds the
kernel against the same host classes."""
import numpy as np
import torch

AUC, ACCURACY = 0, 1


def thresholds(N: int) -> np.ndarray:
    """tf.metrics.auc's thresholds as estimator.AUCMetric builds them, float32"""
    eps = 1e-7
    return np.array([0.0 - eps] + [(i + 1) * 1.0 / (N - 1) for i in range(N - 2)] + [1.0 + eps], dtype=np.float32)


def bins(p: np.ndarray, th: np.ndarray) -> np.ndarray:
    p, th = np.asarray(p, np.float32).reshape(-1), np.asarray(th, np.float32)
    with np.errstate(invalid="ignore"):
        return (p[:, None] > th[None, :]).sum(1)


def hist(labels: np.ndarray, p: np.ndarray, th: np.ndarray) -> np.ndarray:
    """[2, N + 1] int64"""
    with np.errstate(invalid="ignore"):
        y = (np.asarray(labels, np.float32).reshape(-1) > np.float32(0.5)).astype(np.int64)
    h = np.zeros((2, len(th) + 1), np.int64)
    np.add.at(h, (y, bins(p, th)), 1)
    return h


def edge_predictions(th: np.ndarray) -> np.ndarray:
    """every threshold, its float32 neighbours on both sides, the ends of [0, 1] and beyond, the non-finite values"""
    th = np.asarray(th, np.float32)
    special = np.array([0.0, 1.0, -0.0, -0.25, -3.0, 1.5, 7.0, np.nan, np.inf, -np.inf, 0.5, np.nextafter(np.float32(0.5), np.float32(0))],
                       dtype=np.float32)
    return np.concatenate([th, np.nextafter(th, np.float32(-np.inf)), np.nextafter(th, np.float32(np.inf)), special]).astype(np.float32)


EDGE_LABELS = np.array([0.0, 1.0, 0.5, 0.50000006], dtype=np.float32)      # 0.5 itself is a negative; the next float32 is not
assert EDGE_LABELS[3] > np.float32(0.5) and EDGE_LABELS[3] == np.nextafter(np.float32(0.5), np.float32(1))


def batch(n: int, th: np.ndarray, seed: int):
    """(labels [n], predictions [n]) float32: the edge predictions (all of them once n allows it) among uniform draws from
    [-0.1, 1.1), in a seeded order; the edge labels in rotation."""
    rng = np.random.default_rng([seed, n, len(th)])
    edge = edge_predictions(th)
    fill = rng.uniform(-0.1, 1.1, size=max(n - len(edge), 0)).astype(np.float32)
    p = rng.permutation(np.concatenate([edge, fill]))[:n]
    labels = EDGE_LABELS[rng.integers(0, 4, size=n)]
    return labels.astype(np.float32), p.astype(np.float32)


def state_words(slots) -> int:
    """slots: [(AUC, N) | (ACCURACY, None)] -> 64-bit words of the state buffer: loss_sum, batches, then each slot's counters"""
    return 2 + sum(2 * (N + 1) if kind == AUC else 2 for kind, N in slots)


def slot_offsets(slots):
    out, w = [], 2
    for kind, N in slots:
        out.append(w)
        w += 2 * (N + 1) if kind == AUC else 2
    return out


def host_counts(m):
    """an AUCMetric's tp / fp / fn / tn as one [4, N] float64 tensor"""
    return torch.stack([m.tp, m.fp, m.fn, m.tn])
