"""LFW pair scoring (the reference's utils/metrics.py, same module path): pair distances and the 10-fold threshold search on the
device (cpg_pair_distance, cpg_pair_sweep: cpg_amd/csrc/verify_kernels.hip).  Embeddings and distances stay in device memory; only
the integer counts, F x T x 4 of them, come to the host, where tpr, fpr and accuracy are formed with calculate_accuracy's own
expressions (utils/metrics.py:63-74) and the folds are averaged with np.mean, as the reference does.

Threshold comparison.  The reference compares a float32 distance with a float64 threshold (np.less(dist, threshold)).  Under
numpy >= 2 (NEP 50) that comparison is made in fp64; under the numpy 1.x of the reference's era value-based casting made it in fp32.
threshold_dtype='float64' (the default) gives numpy 2's result; threshold_dtype='float32' rounds the table to float32 first, which
gives numpy 1's result exactly.

subtract_mean=True.  The reference centres both embeddings on the mean of the fold's training rows before every distance, so the
distances differ per fold: cpg_pair_fold_mean gives the F means (numpy's axis-0 order, bit for bit), cpg_pair_distance_centred an
F x n distance matrix, and the sweeps read row f for fold f.

VAL@FAR (calculate_val, :77-122).  cpg_pair_val_table counts the train set's true and false accepts at every threshold of the fine
table and cpg_pair_val_at the test set's at one threshold per fold; val and far are formed on the host from those integers.  Between
the two the reference takes scipy.interpolate.interp1d(far_train, thresholds, kind='slinear')(far_target); threshold_at_far restates
that on the host in numpy, with what SciPy 1.15 does: far_train is a step function, and as soon as it repeats a value interp1d raises
ValueError('Expect x to not have duplicates') -- so calculate_val does here.  fv_evaluate's 4 000-entry table always repeats values,
so the reference's fv_evaluate completes only where no false accept is ever seen (the `max(far_train) < far_target` branch, threshold
0); where it raises, fv_evaluate here keeps returning NaN for val, val_std and far unless strict=True asks for the exception.
A caller that wants VAL@FAR regardless applies its own rule to val_tables' far_train and scores it with val_far_at (first_at_far is
one such rule); both stay on the device path.  A fold without a "same" or a "different" pair makes the reference's calculate_val_far
divide by zero (ZeroDivisionError), and so it does here.
"""
import ctypes

import numpy as np
import torch

from .. import _lib

MAX_THRESHOLDS = 480            # include/cpg_hip.h: cpg_pair_sweep's table travels by value
MAX_DIM = 4096


def _embeddings(e, device=None):
    t = torch.as_tensor(e)
    if not t.is_cuda:
        t = t.to(device if device is not None else 'cuda')
    if t.dtype != torch.float32:
        raise TypeError('cpg_amd: embeddings must be float32, got %s' % t.dtype)
    if t.dim() != 2:
        raise ValueError('cpg_amd: embeddings must be a [n][d] matrix, got shape %s' % (tuple(t.shape),))
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _metric(distance_metric):
    if distance_metric == 0:
        return 0
    if distance_metric == 1:
        return 1
    raise ValueError('Undefined distance metric %r' % (distance_metric,))


def _distance(e1, e2, metric, sim=None):
    n, d = e1.shape
    dist = torch.empty(n, dtype=torch.float32, device=e1.device)
    with torch.cuda.device(e1.device):
        _lib.call('cpg_pair_distance', ctypes.c_void_p(e1.data_ptr()), max(int(e1.stride(0)), d), ctypes.c_void_p(e2.data_ptr()),
                  max(int(e2.stride(0)), d), n, d, metric, _lib.dptr(dist), None if sim is None else _lib.dptr(sim), _lib.stream_ptr())
    return dist


def distance(embeddings1, embeddings2, distance_metric=0):
    """utils/metrics.py:11-27 on the device: a float32 tensor of n distances.  Metric 0 (Euclidean: sum of squared differences) is
    bit-identical to the reference; metric 1 (angular: arccos of the clipped cosine, times 4 / pi) has the reference's cosine bit
    for bit and an fp64 arccos rounded once to float32 (numpy's float32 arccos is within two ulp of it)."""
    metric = _metric(distance_metric)
    e1 = _embeddings(embeddings1)
    e2 = _embeddings(embeddings2, e1.device)
    if e1.shape != e2.shape:
        raise ValueError('cpg_amd: embedding shapes differ: %s and %s' % (tuple(e1.shape), tuple(e2.shape)))
    return _distance(e1, e2, metric)


def _thresholds(thresholds, threshold_dtype):
    thr = np.asarray(thresholds, np.float64).reshape(-1)
    if threshold_dtype in ('float32', np.float32):
        thr = thr.astype(np.float32).astype(np.float64)
    elif threshold_dtype not in ('float64', np.float64):
        raise ValueError("threshold_dtype must be 'float64' (numpy >= 2 comparisons) or 'float32' (numpy 1.x), got %r" % (threshold_dtype,))
    return np.ascontiguousarray(thr)


def roc_counts(thresholds, dist, actual_issame, nrof_folds=10, threshold_dtype='float64'):
    """The device sweep: (counts int64 [F][T][4] = {tp, fp, tn, fn} of each fold's test pairs, best [F] = first best train threshold
    index), both on the host.  dist: the device distances; actual_issame: n labels (host or device)."""
    thr = _thresholds(thresholds, threshold_dtype)
    if dist.dim() == 2:
        return _roc_counts_folds(thr, dist, actual_issame, int(nrof_folds))
    n = int(dist.shape[0])
    same = torch.as_tensor(actual_issame).reshape(-1)[:n].to(device=dist.device, dtype=torch.bool).to(torch.uint8).contiguous()
    if same.shape[0] != n:
        raise ValueError('cpg_amd: %d labels for %d pairs' % (same.shape[0], n))
    F, T = int(nrof_folds), len(thr)
    counts = torch.empty((max(F, 0), T, 4), dtype=torch.int64, device=dist.device)
    best = torch.empty(max(F, 0), dtype=torch.int64, device=dist.device)
    with torch.cuda.device(dist.device):
        _lib.call('cpg_pair_sweep', _lib.dptr(dist), _lib.dptr(same, torch.uint8), n, thr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), T, F,
                  ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(best.data_ptr()), _lib.stream_ptr())
    return counts.cpu().numpy(), best.cpu().numpy()


def _labels(actual_issame, dist):
    n = int(dist.shape[-1])
    same = torch.as_tensor(actual_issame).reshape(-1)[:n].to(device=dist.device, dtype=torch.bool).to(torch.uint8).contiguous()
    if same.shape[0] != n:
        raise ValueError('cpg_amd: %d labels for %d pairs' % (same.shape[0], n))
    return n, same


def _rows(dist, F):
    """(contiguous distances, leading dimension): 0 for n distances every fold shares, n for an [F][n] matrix (row f for fold f)."""
    if dist.dim() == 1:
        return dist.contiguous(), 0
    if dist.dim() != 2 or dist.shape[0] != F:
        raise ValueError('cpg_amd: distances of shape %s for %d folds (want [n] or [folds][n])' % (tuple(dist.shape), F))
    return dist.contiguous(), int(dist.shape[1])


def _f64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _roc_counts_folds(thr, dist, actual_issame, F):
    n, same = _labels(actual_issame, dist)
    dist, ldd = _rows(dist, F)
    T = len(thr)
    counts = torch.empty((max(F, 0), T, 4), dtype=torch.int64, device=dist.device)
    best = torch.empty(max(F, 0), dtype=torch.int64, device=dist.device)
    with torch.cuda.device(dist.device):
        _lib.call('cpg_pair_sweep_folds', _lib.dptr(dist), ldd, _lib.dptr(same, torch.uint8), n, _f64p(thr), T, F,
                  ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(best.data_ptr()), _lib.stream_ptr())
    return counts.cpu().numpy(), best.cpu().numpy()


def fold_means(embeddings1, embeddings2, nrof_folds=10):
    """np.mean(np.concatenate([e1[train], e2[train]]), axis=0) of every fold's training pairs: a float32 [folds][d] device tensor,
    numpy's bits (cpg_pair_fold_mean)."""
    e1 = _embeddings(embeddings1)
    e2 = _embeddings(embeddings2, e1.device)
    n, d = e1.shape
    F = int(nrof_folds)
    mean = torch.empty((max(F, 0), d), dtype=torch.float32, device=e1.device)
    with torch.cuda.device(e1.device):
        _lib.call('cpg_pair_fold_mean', ctypes.c_void_p(e1.data_ptr()), max(int(e1.stride(0)), d), ctypes.c_void_p(e2.data_ptr()),
                  max(int(e2.stride(0)), d), n, d, F, _lib.dptr(mean), _lib.stream_ptr())
    return mean


def centred_distance(embeddings1, embeddings2, mean, distance_metric=0, sim=None):
    """distance(e1 - mean[f], e2 - mean[f], metric) for every row f of `mean`: a float32 [folds][n] device tensor."""
    metric = _metric(distance_metric)
    e1 = _embeddings(embeddings1)
    e2 = _embeddings(embeddings2, e1.device)
    n, d = e1.shape
    F = int(mean.shape[0])
    dist = torch.empty((F, n), dtype=torch.float32, device=e1.device)
    with torch.cuda.device(e1.device):
        _lib.call('cpg_pair_distance_centred', ctypes.c_void_p(e1.data_ptr()), max(int(e1.stride(0)), d), ctypes.c_void_p(e2.data_ptr()),
                  max(int(e2.stride(0)), d), n, d, metric, _lib.dptr(mean), F, _lib.dptr(dist), None if sim is None else _lib.dptr(sim),
                  _lib.stream_ptr())
    return dist


def fold_distances(embeddings1, embeddings2, actual_issame, nrof_folds=10, distance_metric=0, subtract_mean=False):
    """What every fold of calculate_roc / calculate_val measures with: the n distances all folds share (subtract_mean=False), or the
    [folds][n] matrix of distances centred on each fold's training mean.  On the device; the first min(len(actual_issame), n) pairs."""
    metric = _metric(distance_metric)
    e1 = _embeddings(embeddings1)
    e2 = _embeddings(embeddings2, e1.device)
    assert e1.shape[0] == e2.shape[0]
    assert e1.shape[1] == e2.shape[1]
    n = min(len(actual_issame), e1.shape[0])
    if not subtract_mean:
        return _distance(e1[:n], e2[:n], metric)
    return centred_distance(e1[:n], e2[:n], fold_means(e1[:n], e2[:n], nrof_folds), metric)


def val_counts(thresholds, dist, actual_issame, nrof_folds=10, threshold_dtype='float64'):
    """cpg_pair_val_table: (table int64 [F][T][2] = {true accepts, false accepts} of each fold's TRAIN pairs at every threshold,
    totals int64 [F][2] = {n_same, n_diff} of those pairs), on the host.  dist: [n] or [F][n] device distances."""
    thr = _thresholds(thresholds, threshold_dtype)
    F, T = int(nrof_folds), len(thr)
    n, same = _labels(actual_issame, dist)
    dist, ldd = _rows(dist, F)
    table = torch.empty((max(F, 0), T, 2), dtype=torch.int64, device=dist.device)
    totals = torch.empty((max(F, 0), 2), dtype=torch.int64, device=dist.device)
    ws, nbytes = _lib.workspace(int(_lib.lib().cpg_pair_val_workspace_bytes(T)), dist.device)
    with torch.cuda.device(dist.device):
        _lib.call('cpg_pair_val_table', _lib.dptr(dist), ldd, _lib.dptr(same, torch.uint8), n, _f64p(thr), T, F,
                  ctypes.c_void_p(table.data_ptr()), ctypes.c_void_p(totals.data_ptr()), _lib.dptr(ws), nbytes, _lib.stream_ptr())
    return table.cpu().numpy(), totals.cpu().numpy()


def _val_far(accepts, totals):
    """calculate_val_far's two divisions (:120-121) on integer counts [..., 2] / [..., 2]: Python's float / float, which raises where
    a set has no "same" or no "different" pair."""
    if (np.asarray(totals) == 0).any():
        raise ZeroDivisionError('float division by zero')
    ratio = np.asarray(accepts, np.float64) / np.asarray(totals, np.float64)
    return ratio[..., 0], ratio[..., 1]


def val_tables(thresholds, dist, actual_issame, nrof_folds=10, threshold_dtype='float64'):
    """(val_train, far_train), float64 [F][T]: calculate_val's table of every fold's training pairs (:97-99) from the device counts."""
    table, totals = val_counts(thresholds, dist, actual_issame, nrof_folds, threshold_dtype)
    return _val_far(table, totals[:, None, :])


def val_counts_at(thresholds_per_fold, dist, actual_issame, nrof_folds=10, threshold_dtype='float64'):
    """cpg_pair_val_at: int64 [F][4] = {true accepts, false accepts, n_same, n_diff} of each fold's TEST pairs at its own threshold."""
    F = int(nrof_folds)
    thr = _thresholds(thresholds_per_fold, threshold_dtype)
    if len(thr) != F:
        raise ValueError('cpg_amd: %d thresholds for %d folds' % (len(thr), F))
    n, same = _labels(actual_issame, dist)
    dist, ldd = _rows(dist, F)
    out = torch.empty((max(F, 0), 4), dtype=torch.int64, device=dist.device)
    with torch.cuda.device(dist.device):
        _lib.call('cpg_pair_val_at', _lib.dptr(dist), ldd, _lib.dptr(same, torch.uint8), n, _f64p(thr), F, ctypes.c_void_p(out.data_ptr()),
                  _lib.stream_ptr())
    return out.cpu().numpy()


def val_far_at(thresholds_per_fold, dist, actual_issame, nrof_folds=10, threshold_dtype='float64'):
    """(val, far), float64 [F]: calculate_val_far of every fold's test pairs at that fold's threshold (:106) -- the second half of
    calculate_val for any rule that picks the thresholds."""
    c = val_counts_at(thresholds_per_fold, dist, actual_issame, nrof_folds, threshold_dtype)
    return _val_far(c[:, :2], c[:, 2:])


def slinear(x, y, x_new):
    """scipy.interpolate.interp1d(x, y, kind='slinear')(x_new) for one x_new, restated (SciPy 1.15): x is sorted stably and y with
    it; a repeated x, fewer than two points or an x_new outside [min x, max x] raise ValueError; otherwise the degree-1 B-spline's
    value, in de Boor's order of operations (the same bits)."""
    x = np.asarray(x, np.float64).reshape(-1)
    y = np.asarray(y, np.float64).reshape(-1)
    if len(x) != len(y):
        raise ValueError('x and y arrays must be equal in length along interpolation axis.')
    if len(x) < 2:
        raise ValueError('x and y arrays must have at least 2 entries')
    order = np.argsort(x, kind='mergesort')
    x, y = x[order], y[order]
    if (x[1:] == x[:-1]).any():
        raise ValueError('Expect x to not have duplicates')
    x_new = float(x_new)
    if x_new < x[0]:
        raise ValueError("A value (%s) in x_new is below the interpolation range's minimum value (%s)." % (x_new, x[0]))
    if x_new > x[-1]:
        raise ValueError("A value (%s) in x_new is above the interpolation range's maximum value (%s)." % (x_new, x[-1]))
    i = min(max(int(np.searchsorted(x, x_new, side='right')) - 1, 0), len(x) - 2)
    xa, xb = x[i], x[i + 1]
    w = 1.0 / (xb - xa)
    h0 = 0.0 + w * (xb - x_new)
    h1 = w * (x_new - xa)
    return (0.0 + y[i] * h0) + y[i + 1] * h1


def threshold_at_far(far_train, thresholds, far_target):
    """calculate_val's choice of one fold's threshold (:100-104): the slinear interpolation of thresholds over far_train at far_target
    where the training FAR reaches the target (ValueError where SciPy raises: far_train repeats a value, or starts above the target),
    else 0.0."""
    if np.max(far_train) >= far_target:
        return slinear(far_train, thresholds, far_target)
    return 0.0


def first_at_far(far_train, thresholds, far_target):
    """A threshold rule that always answers, for callers the reference's interpolation leaves without a value: the largest threshold
    whose training FAR is still <= far_target (0.0 when there is none).  Not the reference's rule."""
    ok = np.nonzero(np.asarray(far_train) <= far_target)[0]
    return float(np.asarray(thresholds, np.float64)[ok[-1]]) if len(ok) else 0.0


def roc_from_counts(counts, best):
    """(tpr, fpr, accuracy) of calculate_roc from the device counts: calculate_accuracy's expressions (0 where a denominator is 0,
    float(tp) / float(tp + fn), float(tp + tn) / test size), then np.mean over the folds."""
    c = counts.astype(np.float64)
    tp, fp, tn, fn = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    tprs = np.divide(tp, tp + fn, out=np.zeros_like(tp), where=(tp + fn) != 0)
    fprs = np.divide(fp, fp + tn, out=np.zeros_like(fp), where=(fp + tn) != 0)
    at = c[np.arange(c.shape[0]), best]
    accuracy = (at[:, 0] + at[:, 2]) / at.sum(1)
    return np.mean(tprs, 0), np.mean(fprs, 0), accuracy


def _opted_in(subtract_mean, accept_subtract_mean):
    """calculate_roc and fv_evaluate refused subtract_mean=True before the centred kernels existed, and callers (and tests) rely on
    that refusal; they take it now when the caller says so.  calculate_val, fold_distances and evalLFW never refused: no opt-in."""
    if subtract_mean and not accept_subtract_mean:
        raise ValueError('cpg_amd: subtract_mean=True is refused unless accept_subtract_mean=True is passed with it (calculate_val, '
                         'fold_distances and evalLFW(subtract_mean=True) take it as it is)')


def calculate_roc(thresholds, embeddings1, embeddings2, actual_issame, nrof_folds=10, distance_metric=0, subtract_mean=False,
                  threshold_dtype='float64', accept_subtract_mean=False):
    """utils/metrics.py:29-61: (tpr, fpr, accuracy) as numpy float64 arrays, the reference's values exactly (given the distances).
    The first min(len(actual_issame), len(embeddings1)) pairs are scored, as the reference's KFold indices do.  subtract_mean=True
    needs accept_subtract_mean=True (_opted_in)."""
    _opted_in(subtract_mean, accept_subtract_mean)
    dist = fold_distances(embeddings1, embeddings2, actual_issame, nrof_folds, distance_metric, subtract_mean)
    counts, best = roc_counts(thresholds, dist, actual_issame, nrof_folds, threshold_dtype)
    return roc_from_counts(counts, best)


def calculate_val_far(threshold, dist, actual_issame, threshold_dtype='float64'):
    """utils/metrics.py:114-122: (val, far) of the pairs with distances `dist` (a device tensor, or anything torch can move there) at
    one threshold, as Python floats."""
    dist = torch.as_tensor(dist)
    if not dist.is_cuda:
        dist = dist.to('cuda')
    val, far = val_far_at([threshold], dist.reshape(-1), actual_issame, 1, threshold_dtype)
    return float(val[0]), float(far[0])


def val_from_distances(thresholds, dist, actual_issame, far_target, nrof_folds=10, threshold_dtype='float64'):
    """calculate_val (:96-111) given the folds' distances ([n] or [F][n], on the device): (val_mean, val_std, far_mean)."""
    thr = _thresholds(thresholds, threshold_dtype)
    F = int(nrof_folds)
    table, totals = val_counts(thr, dist, actual_issame, F)
    at, error = [], None
    for f in range(F):
        try:
            _, far_train = _val_far(table[f], totals[f])
            at.append(threshold_at_far(far_train, thr, far_target))
        except (ValueError, ZeroDivisionError) as e:
            error = e
            break
    # the reference scores a fold's test pairs before it turns to the next fold: an earlier fold's division by zero comes first
    c = val_counts_at(at + [0.0] * (F - len(at)), dist, actual_issame, F, threshold_dtype)[:len(at)]
    val, far = _val_far(c[:, :2], c[:, 2:])
    if error is not None:
        raise error
    return np.mean(val), np.std(val), np.mean(far)


def calculate_val(thresholds, embeddings1, embeddings2, actual_issame, far_target, nrof_folds=10, distance_metric=0, subtract_mean=False,
                  threshold_dtype='float64'):
    """utils/metrics.py:77-111: (val_mean, val_std, far_mean), the reference's values exactly (given the distances) wherever the
    reference returns; ValueError where its interp1d raises and ZeroDivisionError where its calculate_val_far divides by zero (the
    module docstring).  `thresholds` must ascend strictly (the device searches it) and hold at most cpg_pair_val_max_thresholds
    entries."""
    dist = fold_distances(embeddings1, embeddings2, actual_issame, nrof_folds, distance_metric, subtract_mean)
    return val_from_distances(thresholds, dist, actual_issame, far_target, nrof_folds, threshold_dtype)


def fv_evaluate(embeddings1, embeddings2, labels, nrof_folds=10, distance_metric=0, subtract_mean=False, threshold_dtype='float64',
                accept_subtract_mean=False, strict=False):
    """utils/metrics.py:125-153's 6-tuple (tpr, fpr, accuracy, val, val_std, far): calculate_roc over np.arange(0, 4, 0.01), then
    calculate_val over np.arange(0, 4, 0.001) at FAR = 1e-3.  The distances are computed once for both.  Where the reference's
    calculate_val raises (the module docstring) val, val_std and far are NaN, as they were before VAL@FAR was built; strict=True
    raises the reference's exception instead.  subtract_mean=True needs accept_subtract_mean=True (_opted_in)."""
    _opted_in(subtract_mean, accept_subtract_mean)
    dist = fold_distances(embeddings1, embeddings2, labels, nrof_folds, distance_metric, subtract_mean)
    counts, best = roc_counts(np.arange(0, 4, 0.01), dist, labels, nrof_folds, threshold_dtype)
    tpr, fpr, accuracy = roc_from_counts(counts, best)
    try:
        val, val_std, far = val_from_distances(np.arange(0, 4, 0.001), dist, labels, 1e-3, nrof_folds, threshold_dtype)
    except (ValueError, ZeroDivisionError):
        if strict:
            raise
        val = val_std = far = float('nan')
    return tpr, fpr, accuracy, val, val_std, far


__all__ = ['distance', 'calculate_roc', 'calculate_val', 'calculate_val_far', 'fv_evaluate', 'roc_counts', 'roc_from_counts', 'fold_means',
           'centred_distance', 'fold_distances', 'val_counts', 'val_tables', 'val_counts_at', 'val_far_at', 'slinear', 'threshold_at_far',
           'first_at_far']
