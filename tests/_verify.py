"""An explicit-order numpy restatement of the pair verification kernels (cpg_amd/csrc/verify_kernels.hip), for the tests.

row_sum is numpy's float32 pairwise summation written out (blocks of at most 128 elements summed by eight accumulators, a recursive
split at n/2 - (n/2 % 8) above 128, the block's rest added in order, the result added to the identity 0); tests/test_verify_host.py
pins it to np.sum and np.linalg.norm.  distance, sweep and roc restate the reference's utils/metrics.py (distance,
calculate_roc, calculate_accuracy) with explicit loops; they never import cpg_amd.
"""
import math

import numpy as np

F32 = np.float32


def _pw(x):
    m = x.shape[1]
    if m < 8:
        res = np.zeros(x.shape[0], F32)
        for i in range(m):
            res = res + x[:, i]
        return res
    if m <= 128:
        r = [x[:, j].copy() for j in range(8)]
        i = 8
        while i < m - m % 8:
            for j in range(8):
                r[j] = r[j] + x[:, i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(m - m % 8, m):
            res = res + x[:, i]
        return res
    n2 = m // 2
    n2 -= n2 % 8
    return _pw(x[:, :n2]) + _pw(x[:, n2:])


def row_sum(x):
    """np.sum(x, axis=1) of a float32 [n][d] matrix, element for element in numpy's order."""
    x = np.asarray(x, F32)
    return np.zeros(x.shape[0], F32) + _pw(x)


def cosine(e1, e2):
    """dot / (|e1| * |e2|) in float32, as utils/metrics.py:18-20 computes it."""
    e1, e2 = np.asarray(e1, F32), np.asarray(e2, F32)
    dot = row_sum(e1 * e2)
    norm = np.sqrt(row_sum(e1 * e1)) * np.sqrt(row_sum(e2 * e2))
    with np.errstate(invalid='ignore', divide='ignore'):
        return dot / norm


def distance(e1, e2, metric):
    """Metric 0 exactly as the reference; metric 1 with the arccos taken in fp64 and rounded once (the kernel's arccos)."""
    if metric == 0:
        d = np.asarray(e1, F32) - np.asarray(e2, F32)
        return row_sum(d * d)
    sim = cosine(e1, e2)
    c = sim.copy()
    c[c < 0] = 0                        # NaN stays NaN, as np.clip
    c[c > 1] = 1
    return np.arccos(c.astype(np.float64)).astype(F32) * F32(4) / F32(math.pi)


def folds(n, nfolds):
    """sklearn's KFold(nfolds, shuffle=False) test ranges."""
    q, r = divmod(n, nfolds)
    out, at = [], 0
    for f in range(nfolds):
        size = q + (1 if f < r else 0)
        out.append((at, at + size))
        at += size
    return out


def sweep(dist, issame, thr, nfolds):
    """counts[F][T][4] = {tp, fp, tn, fn} of every fold's test pairs, and every fold's first best train threshold index."""
    dist = np.asarray(dist, F32)
    issame = np.asarray(issame).astype(bool)
    thr = np.asarray(thr, np.float64)
    n, T = len(dist), len(thr)
    counts = np.zeros((nfolds, T, 4), np.int64)
    best = np.zeros(nfolds, np.int64)
    pred = dist.astype(np.float64)[None, :] < thr[:, None]                  # [T][n]
    for f, (lo, hi) in enumerate(folds(n, nfolds)):
        test = np.zeros(n, bool)
        test[lo:hi] = True
        for part, out in ((test, 'test'), (~test, 'train')):
            p, s = pred[:, part], issame[part]
            tp = (p & s).sum(1)
            fp = (p & ~s).sum(1)
            tn = (~p & ~s).sum(1)
            fn = (~p & s).sum(1)
            if out == 'test':
                counts[f] = np.stack([tp, fp, tn, fn], 1)
            else:
                acc = tp + tn
                b = 0
                for t in range(T):
                    if acc[t] > acc[b]:
                        b = t
                best[f] = b
    return counts, best


def roc(counts, best):
    """(tpr, fpr, accuracy) from the counts with calculate_accuracy's expressions (utils/metrics.py:63-74), folds averaged with np.mean."""
    F, T, _ = counts.shape
    tprs = np.zeros((F, T))
    fprs = np.zeros((F, T))
    accuracy = np.zeros(F)
    for f in range(F):
        for t in range(T):
            tp, fp, tn, fn = (int(v) for v in counts[f, t])
            tprs[f, t] = 0 if (tp + fn == 0) else float(tp) / float(tp + fn)
            fprs[f, t] = 0 if (fp + tn == 0) else float(fp) / float(fp + tn)
        tp, fp, tn, fn = (int(v) for v in counts[f, best[f]])
        accuracy[f] = float(tp + tn) / (tp + fp + tn + fn)
    return np.mean(tprs, 0), np.mean(fprs, 0), accuracy


def adversarial_rows(rng, n, d):
    """Rows whose float32 sum depends on the order: wide magnitudes, cancellations, many ulp-sized terms."""
    x = rng.standard_normal((n, d)).astype(F32)
    scale = (F32(2) ** rng.integers(-20, 20, (n, d))).astype(F32)
    x = x * scale
    k = rng.integers(0, d, n)
    x[np.arange(n), k] = F32(1e8) * np.sign(rng.standard_normal(n)).astype(F32)
    j = rng.integers(0, d, n)
    x[np.arange(n), j] = -x[np.arange(n), k]
    return x
