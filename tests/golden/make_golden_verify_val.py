#!/usr/bin/env python3
"""Generate tests/golden/verify_val.npz by RUNNING the reference's LFW scoring with subtract_mean and VAL@FAR (utils/metrics.py:
calculate_roc(subtract_mean=True), calculate_val, fv_evaluate).

Like make_golden_verify.py this imports ivclab/CPG from /root/reference (present only in the build container) with the container's
numpy, SciPy and scikit-learn; nothing of its source travels, the fixture holds arrays only.  Re-run with

    python tests/golden/make_golden_verify_val.py

What the probe of the reference showed (SciPy 1.15): interp1d(far_train, thresholds, kind='slinear') raises ValueError('Expect x to
not have duplicates') as soon as far_train repeats a value, and ValueError when far_target lies below far_train[0]; fv_evaluate's
4 000-entry table always repeats values, so fv_evaluate completes only on the `max(far_train) < far_target` branch (threshold 0).
A test or train set without a "same" or a "different" pair makes calculate_val_far raise ZeroDivisionError.  An outcome that is an
exception is recorded by its class name.

Cases (embeddings are float16 values, used as float32; `folds` is nrof_folds):
  * uneven   23 x 9,   10 folds: ragged folds; a short ascending table on which far_train is strictly increasing in every fold, so
                       the interpolation returns a value.
  * lfw      600 x 129, 10 folds: both metrics; fv_evaluate raises (repeated far_train).
  * single   10 x 1,   10 folds: one pair per fold, so every test fold lacks a label: calculate_roc's guarded ratios give 0,
                       calculate_val divides by zero.
  * nonfinite 40 x 8,  10 folds: NaN, +Inf and -Inf embeddings (the means of the folds that train on them are not finite either).
  * apart    60 x 8,   10 folds: every "different" pair is further apart than the last threshold: fv_evaluate completes (threshold 0).
  * ties     40 x 4,    5 folds: multiples of 1/2 and 64 training rows, so means, differences and squares are exact and centred
                       metric-0 distances sit exactly on thresholds of np.arange(0, 4, 0.01) and of the case's own short table.
For every case and metric: the F fold means, the centred distances of every fold, calculate_roc(subtract_mean=True) over
np.arange(0, 4, 0.01), calculate_val over the case's own table and FAR target with subtract_mean False and True, and (10 folds)
fv_evaluate with subtract_mean False and True.  No metric-1 distance lies within 1e-6 (four float32 ulp at 2, the largest angular
distance) of a threshold of np.arange(0, 4, 0.01) or of a short table, so an arccos ulp cannot move a count; over the 4 000-entry
table every metric-1 outcome is an exception that no single count decides (a repeated far_train), or every distance is NaN (checked
below).
"""
import os
import sys
import warnings

import numpy as np

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
warnings.filterwarnings('ignore')

THR_ROC = np.arange(0, 4, 0.01)
THR_VAL = np.arange(0, 4, 0.001)


def _pairs(rng, n, d, scale=None):
    scale = np.sqrt(1.0 / d) if scale is None else scale
    e1 = rng.standard_normal((n, d)) * scale
    sigma = rng.uniform(0.05, 1.6, n)
    e2 = e1 + rng.standard_normal((n, d)) * (scale * sigma)[:, None]
    same = sigma + rng.normal(0, 0.3, n) < 0.8
    return e1.astype(np.float16), e2.astype(np.float16), same


def _folds(n, F):
    from sklearn.model_selection import KFold
    return list(KFold(n_splits=F, shuffle=False).split(np.arange(n)))


def _fold_dists(M, f1, f2, F, metric):
    means, dists = [], []
    for train, _ in _folds(len(f1), F):
        mean = np.mean(np.concatenate([f1[train], f2[train]]), axis=0)
        means.append(mean)
        dists.append(M.distance(f1 - mean, f2 - mean, metric))
    return np.stack(means).astype(np.float32), np.stack(dists).astype(np.float32)


def _clear(dist, tables, eps=1e-6):
    x = dist.astype(np.float64).reshape(-1, 1)
    ok = np.ones(x.shape[0], bool)
    for thr in tables:
        ok &= np.abs(x - thr[None, :]).min(1) > eps
    return bool((np.isnan(x[:, 0]) | ok).all())


def _outcome(fn, size):
    try:
        return np.asarray(fn(), np.float64).reshape(size), ''
    except (ValueError, ZeroDivisionError) as e:
        return np.full(size, np.nan), type(e).__name__


def main():
    from utils import metrics as M
    rng = np.random.default_rng(20261021)
    cases = []

    # uneven: labels alternate (every test fold has both), and the 11 "different" pairs lie 4 / 4 / 3 in the three bins of a short
    # table, so that far_train is strictly increasing whichever fold (at most two of them) is left out
    table = np.array([0.0, 1.0, 2.0, 3.5])
    same = np.arange(23) % 2 == 0
    target = np.where(same, rng.uniform(0.05, 0.5, 23), 0.0)
    target[~same] = rng.permutation([0.2, 0.4, 0.6, 0.8, 1.2, 1.4, 1.6, 1.8, 2.3, 2.7, 3.1])
    e1 = rng.standard_normal((23, 9)) / 3
    u = rng.standard_normal((23, 9))
    e2 = e1 + u / np.linalg.norm(u, axis=1, keepdims=True) * np.sqrt(target)[:, None]
    e1, e2 = e1.astype(np.float16), e2.astype(np.float16)
    for sm in (False, True):                        # the reference completes: the interpolation returns a value in every fold
        M.calculate_val(table, e1.astype(np.float32), e2.astype(np.float32), same, 0.3, nrof_folds=10, distance_metric=0, subtract_mean=sm)
    cases.append(('uneven', e1, e2, same, 10, (0, 1), table, 0.3))

    for _ in range(200):                            # redrawn until no metric-1 distance of any fold sits on a threshold
        e1, e2, same = _pairs(rng, 600, 129)
        f1, f2 = e1.astype(np.float32), e2.astype(np.float32)
        if _clear(_fold_dists(M, f1, f2, 10, 1)[1], [THR_ROC]) and _clear(M.distance(f1, f2, 1), [THR_ROC]):
            break
    cases.append(('lfw', e1, e2, same, 10, (0, 1), THR_VAL, 1e-3))

    # a FAR target no table reaches: no interpolation, threshold 0, and then the division by the test fold's missing label
    e1, e2, same = _pairs(rng, 10, 1, 0.7)
    cases.append(('single', e1, e2, same, 10, (0,), table, 2.0))

    for _ in range(200):
        e1, e2, same = _pairs(rng, 40, 8)
        e1[3, 2], e2[17, 0], e1[29, 5], e2[29, 5] = np.nan, np.inf, -np.inf, np.inf
        f1, f2 = e1.astype(np.float32), e2.astype(np.float32)
        both = all(same[test].any() and not same[test].all() for _, test in _folds(40, 10))
        if both and _clear(_fold_dists(M, f1, f2, 10, 1)[1], [THR_ROC, table]) and _clear(M.distance(f1, f2, 1), [THR_ROC, table]):
            break
    cases.append(('nonfinite', e1, e2, same, 10, (0, 1), table, 0.3))

    # apart: "different" pairs are opposite points of a sphere of radius 1.25 (squared distance 6.25 > every threshold), "same" close
    e1 = rng.standard_normal((60, 8))
    e1 = (1.25 * e1 / np.linalg.norm(e1, axis=1, keepdims=True)).astype(np.float16)
    same = rng.random(60) < 0.5
    e2 = np.where(same[:, None], e1.astype(np.float64) + rng.standard_normal((60, 8)) * 0.15, -e1.astype(np.float64)).astype(np.float16)
    cases.append(('apart', e1, e2, same, 10, (0,), THR_VAL, 1e-3))

    # ties: multiples of 1/2; the pairs differ by patterns whose squares sum to 0, 0.25, 0.5, 1, 1.25, 2, 3
    # (drawn until far_train is strictly increasing over a table of exactly those values in every fold: the interpolation answers)
    tie_table = np.array([0.0, 0.25, 0.5, 1.0, 1.25, 2.0, 3.0, 3.5])
    pats = [(), (0.5,), (0.5, 0.5), (1.0,), (0.5, 1.0), (1.0, 1.0), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5, 0.5)]
    for _ in range(2000):
        e1 = (rng.integers(-2, 3, (40, 4)) * 0.5).astype(np.float16)
        e2 = e1.copy()
        for i in range(40):
            pat = pats[int(rng.integers(0, len(pats)))]
            for c, v in zip(rng.choice(4, len(pat), replace=False), pat):
                e2[i, c] = e1[i, c] + np.float16(v)
        same = rng.random(40) < 0.4
        try:
            M.calculate_val(tie_table, e1.astype(np.float32), e2.astype(np.float32), same, 0.3, nrof_folds=5, distance_metric=0,
                            subtract_mean=True)
            break
        except (ValueError, ZeroDivisionError):
            continue
    else:
        raise SystemExit('ties: no draw on which the interpolation returns a value')
    cases.append(('ties', e1, e2, same, 5, (0,), tie_table, 0.3))

    out = {'cases': np.array([c[0] for c in cases])}
    for tag, e1, e2, same, F, metrics, vtable, target in cases:
        f1, f2 = e1.astype(np.float32), e2.astype(np.float32)
        out.update({tag + '_e1': e1, tag + '_e2': e2, tag + '_issame': same, tag + '_folds': np.array(F), tag + '_metrics': np.array(metrics),
                    tag + '_val_thr': vtable, tag + '_far_target': np.array(target)})
        for metric in metrics:
            key = '%s_m%d_' % (tag, metric)
            means, dists = _fold_dists(M, f1, f2, F, metric)
            plain = M.distance(f1, f2, metric).astype(np.float32)
            if metric == 1:
                tables = [THR_ROC] + ([vtable] if len(vtable) < 100 else [])
                assert _clear(dists, tables) and _clear(plain, tables), tag
            if tag == 'ties':
                on = np.isin(dists.astype(np.float64), THR_ROC) & np.isin(dists.astype(np.float64), vtable)
                assert on.all() and np.array_equal(dists, np.broadcast_to(plain, dists.shape)), tag
            out[tag + '_mean'] = means
            out[key + 'dist'] = dists
            tpr, fpr, acc = M.calculate_roc(THR_ROC, f1, f2, same, nrof_folds=F, distance_metric=metric, subtract_mean=True)
            out[key + 'tpr'], out[key + 'fpr'], out[key + 'acc'] = tpr, fpr, acc
            for sm in (0, 1):
                out[key + 'val_sm%d' % sm], out[key + 'val_sm%d_raises' % sm] = _outcome(
                    lambda: M.calculate_val(vtable, f1, f2, same, target, nrof_folds=F, distance_metric=metric, subtract_mean=bool(sm)), 3)
                if F == 10:
                    try:
                        res = M.fv_evaluate(f1, f2, same, nrof_folds=F, distance_metric=metric, subtract_mean=bool(sm))
                        for name, v in zip(('tpr', 'fpr', 'acc', 'val', 'val_std', 'far'), res):
                            out[key + 'fv_sm%d_%s' % (sm, name)] = np.asarray(v, np.float64)
                        raised = ''
                    except (ValueError, ZeroDivisionError) as e:
                        raised = type(e).__name__
                    out[key + 'fv_sm%d_raises' % sm] = np.array(raised)
                    assert metric == 0 or raised or (sm and np.isnan(dists).all()), tag
                assert metric == 0 or len(vtable) < 100 or out[key + 'val_sm%d_raises' % sm] or (sm and np.isnan(dists).all()), tag
            print(tag, metric, 'val', [str(out[key + 'val_sm%d_raises' % s]) or out[key + 'val_sm%d' % s] for s in (0, 1)],
                  'fv', [str(out.get(key + 'fv_sm%d_raises' % s)) for s in (0, 1)])
    # what the interpolation itself returns, apart from the scoring: (x, y, x_new) -> value or the exception's class
    from scipy import interpolate
    xs, ys, ts, vals, errs = [], [], [], [], []
    for k in range(64):
        n = int(rng.integers(2, 9))
        x = np.cumsum(rng.integers(0 if k % 8 == 0 else 1, 4, n)) / 27.0
        y = np.sort(rng.random(n) * 4)
        t = [x[0], x[-1], x[int(rng.integers(0, n))], x[0] + (x[-1] - x[0]) * rng.random(), x[0] - 0.01, x[-1] + 0.01][k % 6]
        try:
            v, err = float(interpolate.interp1d(x, y, kind='slinear')(t)), ''
        except ValueError as e:
            v, err = np.nan, type(e).__name__
        xs.append(np.pad(x, (0, 8 - n), constant_values=np.nan))
        ys.append(np.pad(y, (0, 8 - n), constant_values=np.nan))
        ts.append(t), vals.append(v), errs.append(err)
    out.update(interp_x=np.array(xs), interp_y=np.array(ys), interp_t=np.array(ts), interp_value=np.array(vals), interp_raises=np.array(errs))
    import scipy
    out['numpy_version'], out['scipy_version'] = np.array(np.__version__), np.array(scipy.__version__)
    path = os.path.join(OUT, 'verify_val.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
