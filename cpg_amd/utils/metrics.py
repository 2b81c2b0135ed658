"""LFW pair scoring (the reference's utils/metrics.py, same module path): pair distances and the 10-fold threshold search on the
device (cpg_pair_distance, cpg_pair_sweep: cpg_amd/csrc/verify_kernels.hip).  Embeddings and distances stay in device memory; only
the integer counts, F x T x 4 of them, come to the host, where tpr, fpr and accuracy are formed with calculate_accuracy's own
expressions (utils/metrics.py:63-74) and the folds are averaged with np.mean, as the reference does.

Threshold comparison.  The reference compares a float32 distance with a float64 threshold (np.less(dist, threshold)).  Under
numpy >= 2 (NEP 50) that comparison is made in fp64; under the numpy 1.x of the reference's era value-based casting made it in fp32.
threshold_dtype='float64' (the default) gives numpy 2's result; threshold_dtype='float32' rounds the table to float32 first, which
gives numpy 1's result exactly.

Not built: calculate_val (VAL@FAR, :77-111) -- evalLFW discards it, and the reference's own interp1d(far_train, thresholds) raises
on current SciPy because far_train repeats 0.0; fv_evaluate returns NaN for val, val_std and far.  subtract_mean=True is refused.
"""
import ctypes
import math

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


def calculate_roc(thresholds, embeddings1, embeddings2, actual_issame, nrof_folds=10, distance_metric=0, subtract_mean=False,
                  threshold_dtype='float64'):
    """utils/metrics.py:29-61: (tpr, fpr, accuracy) as numpy float64 arrays, the reference's values exactly (given the distances).
    The first min(len(actual_issame), len(embeddings1)) pairs are scored, as the reference's KFold indices do."""
    if subtract_mean:
        raise ValueError('cpg_amd: subtract_mean=True is not supported (evalLFW uses subtract_mean=False)')
    metric = _metric(distance_metric)
    e1 = _embeddings(embeddings1)
    e2 = _embeddings(embeddings2, e1.device)
    assert e1.shape[0] == e2.shape[0]
    assert e1.shape[1] == e2.shape[1]
    n = min(len(actual_issame), e1.shape[0])
    dist = _distance(e1[:n], e2[:n], metric)
    counts, best = roc_counts(thresholds, dist, actual_issame, nrof_folds, threshold_dtype)
    return roc_from_counts(counts, best)


def fv_evaluate(embeddings1, embeddings2, labels, nrof_folds=10, distance_metric=0, subtract_mean=False, threshold_dtype='float64'):
    """utils/metrics.py:114-154's 6-tuple (tpr, fpr, accuracy, val, val_std, far) over the reference's thresholds np.arange(0, 4, 0.01).
    VAL@FAR (calculate_val) is not built: val, val_std and far are NaN (see the module docstring)."""
    thresholds = np.arange(0, 4, 0.01)
    tpr, fpr, accuracy = calculate_roc(thresholds, embeddings1, embeddings2, labels, nrof_folds=nrof_folds, distance_metric=distance_metric,
                                       subtract_mean=subtract_mean, threshold_dtype=threshold_dtype)
    return tpr, fpr, accuracy, math.nan, math.nan, math.nan


__all__ = ['distance', 'calculate_roc', 'fv_evaluate', 'roc_counts', 'roc_from_counts']
