"""An explicit-order numpy restatement of the subtract_mean and VAL@FAR half of pair verification (cpg_amd/csrc/verify_kernels.hip:
cpg_pair_fold_mean, cpg_pair_distance_centred, cpg_pair_sweep_folds, cpg_pair_val_table, cpg_pair_val_at), beside tests/_verify.py.

col_mean is numpy's float32 np.mean(axis=0) of a C-contiguous matrix written out: the sum starts from the identity 0 and takes the
rows one after another -- except for a matrix of one column, whose rows are one contiguous run that numpy sums pairwise (_verify's
row_sum) -- then one division by float32(rows); tests/test_verify_val_host.py pins it to np.mean.  The rest restates the reference's
utils/metrics.py (calculate_roc and calculate_val with subtract_mean, calculate_val_far) and SciPy's slinear interp1d with explicit
loops; nothing here imports cpg_amd or scipy.
"""
import numpy as np

import _verify as V

F32 = V.F32


def col_mean(x):
    """np.mean(x, axis=0) of a C-contiguous float32 [m][d] matrix, element for element in numpy's order."""
    x = np.asarray(x, F32)
    m, d = x.shape
    with np.errstate(all='ignore'):
        if d == 1:
            s = V.row_sum(np.ascontiguousarray(x.T))
        else:
            s = np.zeros(d, F32)
            for i in range(m):
                s = s + x[i]
        return s / F32(m)


def fold_means(e1, e2, nfolds):
    """[F][d]: the mean of [e1[train]; e2[train]] for every fold's training pairs (utils/metrics.py:46)."""
    e1, e2 = np.asarray(e1, F32), np.asarray(e2, F32)
    n = e1.shape[0]
    out = np.zeros((nfolds, e1.shape[1]), F32)
    for f, (lo, hi) in enumerate(V.folds(n, nfolds)):
        train = np.r_[0:lo, hi:n]
        out[f] = col_mean(np.concatenate([e1[train], e2[train]]))
    return out


def centred(e, mean):
    with np.errstate(all='ignore'):
        return np.asarray(e, F32) - np.asarray(mean, F32)


def centred_distance(e1, e2, means, metric):
    """[F][n]: distance(e1 - mean_f, e2 - mean_f) with _verify's distance (metric 1: the kernel's fp64 arccos)."""
    with np.errstate(all='ignore'):
        return np.stack([V.distance(centred(e1, m), centred(e2, m), metric) for m in means])


def centred_cosine(e1, e2, means):
    with np.errstate(all='ignore'):
        return np.stack([V.cosine(centred(e1, m), centred(e2, m)) for m in means])


def rows(dist, nfolds):
    dist = np.asarray(dist, F32)
    return dist if dist.ndim == 2 else np.broadcast_to(dist, (nfolds, len(dist)))


def sweep_folds(dist, issame, thr, nfolds):
    """_verify.sweep where fold f measures with row f of dist."""
    dist = rows(dist, nfolds)
    counts = np.zeros((nfolds, len(thr), 4), np.int64)
    best = np.zeros(nfolds, np.int64)
    for f in range(nfolds):
        c, b = V.sweep(dist[f], issame, thr, nfolds)
        counts[f], best[f] = c[f], b[f]
    return counts, best


def val_table(dist, issame, thr, nfolds):
    """table[F][T][2] = {true accepts, false accepts} of every fold's TRAIN pairs at every threshold; totals[F][2] = {n_same, n_diff}."""
    dist = rows(dist, nfolds)
    issame = np.asarray(issame).astype(bool)
    thr = np.asarray(thr, np.float64)
    n = dist.shape[1]
    table = np.zeros((nfolds, len(thr), 2), np.int64)
    totals = np.zeros((nfolds, 2), np.int64)
    for f, (lo, hi) in enumerate(V.folds(n, nfolds)):
        train = np.r_[0:lo, hi:n]
        d, s = dist[f, train].astype(np.float64), issame[train]
        with np.errstate(invalid='ignore'):
            pred = d[None, :] < thr[:, None]
        table[f, :, 0] = (pred & s).sum(1)
        table[f, :, 1] = (pred & ~s).sum(1)
        totals[f] = s.sum(), (~s).sum()
    return table, totals


def _test_counts(row, issame, lo, hi, threshold):
    d, s = row[lo:hi].astype(np.float64), issame[lo:hi]
    with np.errstate(invalid='ignore'):
        pred = d < np.float64(threshold)
    return (pred & s).sum(), (pred & ~s).sum(), s.sum(), (~s).sum()


def val_at(dist, issame, thr_per_fold, nfolds):
    """out[F][4] = {true accepts, false accepts, n_same, n_diff} of every fold's TEST pairs at that fold's threshold."""
    dist = rows(dist, nfolds)
    issame = np.asarray(issame).astype(bool)
    out = np.zeros((nfolds, 4), np.int64)
    for f, (lo, hi) in enumerate(V.folds(dist.shape[1], nfolds)):
        out[f] = _test_counts(dist[f], issame, lo, hi, thr_per_fold[f])
    return out


def ratio(accepts, total):
    """calculate_val_far's float(accepts) / float(total) (utils/metrics.py:120-121)."""
    return float(int(accepts)) / float(int(total))


def slinear(x, y, x_new):
    """scipy.interpolate.interp1d(x, y, kind='slinear')(x_new) as SciPy 1.15 computes it: a stable sort by x, ValueError for a
    repeated x or an x_new outside the range, else the degree-1 B-spline by de Boor's recurrence."""
    x = [float(v) for v in x]
    y = [float(v) for v in y]
    if len(x) < 2:
        raise ValueError('x and y arrays must have at least 2 entries')
    order = sorted(range(len(x)), key=lambda k: x[k])            # Python's sort is stable
    x, y = [x[k] for k in order], [y[k] for k in order]
    if any(x[k] == x[k + 1] for k in range(len(x) - 1)):
        raise ValueError('Expect x to not have duplicates')
    x_new = float(x_new)
    if x_new < x[0] or x_new > x[-1]:
        raise ValueError('A value (%r) in x_new is outside the interpolation range [%r, %r].' % (x_new, x[0], x[-1]))
    i = 0
    while i < len(x) - 2 and x[i + 1] <= x_new:
        i += 1
    w = 1.0 / (x[i + 1] - x[i])
    h0 = 0.0 + w * (x[i + 1] - x_new)
    h1 = w * (x_new - x[i])
    return (0.0 + y[i] * h0) + y[i + 1] * h1


def calculate_val(thr, dist, issame, far_target, nfolds):
    """utils/metrics.py:77-111 given the folds' distances: (val_mean, val_std, far_mean); raises what the reference raises, fold by
    fold in its order (a set without a "same" or a "different" pair: ZeroDivisionError; the interpolation: ValueError)."""
    thr = np.asarray(thr, np.float64)
    dist = rows(dist, nfolds)
    issame = np.asarray(issame).astype(bool)
    table, totals = val_table(dist, issame, thr, nfolds)
    val, far = np.zeros(nfolds), np.zeros(nfolds)
    for f, (lo, hi) in enumerate(V.folds(dist.shape[1], nfolds)):
        far_train = np.zeros(len(thr))
        for t in range(len(thr)):
            ratio(table[f, t, 0], totals[f, 0])                   # the reference forms val_train too, first
            far_train[t] = ratio(table[f, t, 1], totals[f, 1])
        threshold = slinear(far_train, thr, far_target) if np.max(far_train) >= far_target else 0.0
        ta, fa, n_same, n_diff = _test_counts(dist[f], issame, lo, hi, threshold)
        val[f], far[f] = ratio(ta, n_same), ratio(fa, n_diff)
    return np.mean(val), np.std(val), np.mean(far)


def fv_evaluate(e1, e2, issame, nfolds=10, metric=0, subtract_mean=False):
    """utils/metrics.py:125-153 with both of its tables."""
    e1, e2 = np.asarray(e1, F32), np.asarray(e2, F32)
    dist = centred_distance(e1, e2, fold_means(e1, e2, nfolds), metric) if subtract_mean else V.distance(e1, e2, metric)
    counts, best = sweep_folds(dist, issame, np.arange(0, 4, 0.01), nfolds)
    tpr, fpr, acc = V.roc(counts, best)
    return (tpr, fpr, acc) + calculate_val(np.arange(0, 4, 0.001), dist, issame, 1e-3, nfolds)
