"""Pair verification on the host: the explicit-order restatement (tests/_verify.py) against numpy and the reference's fixture, and the
library's refusals of bad sweep / distance arguments, which happen before anything touches the device."""
import ctypes

import numpy as np
import pytest

import _verify as V

DIMS = [1, 3, 7, 8, 9, 15, 16, 17, 64, 100, 127, 128, 129, 130, 255, 256, 300, 511, 512, 513, 1000, 2047, 4096]


@pytest.mark.parametrize('d', DIMS)
def test_row_sum_is_numpys_pairwise_order(d):
    rng = np.random.default_rng(1000 + d)
    x = V.adversarial_rows(rng, 300, d)
    assert np.array_equal(V.row_sum(x).view(np.uint32), np.sum(x, axis=1).view(np.uint32))
    assert np.array_equal(np.sqrt(V.row_sum(x * x)).view(np.uint32), np.linalg.norm(x, axis=1).view(np.uint32))
    y = V.adversarial_rows(rng, 300, d)
    assert np.array_equal(V.row_sum(x * y).view(np.uint32), np.sum(np.multiply(x, y), axis=1).view(np.uint32))


def test_a_first_element_start_is_a_different_order():
    """What the restatement pins is not vacuous: starting the sum from the first element instead of the identity changes rows."""
    rng = np.random.default_rng(7)
    x = V.adversarial_rows(rng, 300, 300)
    first = x[:, 0] + V._pw(x[:, 1:])
    assert not np.array_equal(first.view(np.uint32), np.sum(x, axis=1).view(np.uint32))


def _sets(fx):
    for tag in ('a', 'b', 'c'):
        yield tag, fx[tag + '_e1'].astype(np.float32), fx[tag + '_e2'].astype(np.float32), fx[tag + '_issame']


def test_restatement_matches_the_reference_fixture(golden):
    fx = golden('verify_roc')
    for tag, e1, e2, same in _sets(fx):
        for metric in ((0, 1) if tag != 'c' else (0,)):
            want = fx['%s_dist%d' % (tag, metric)]
            got = V.distance(e1, e2, metric)
            if metric == 0:
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tag
            else:
                assert np.array_equal(np.isnan(got), np.isnan(want))
                ok = ~np.isnan(want)
                assert np.abs(got[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32)).max() <= 2, tag
            for tt in ('64', '32'):
                counts, best = V.sweep(got, same, fx['thr' + tt].astype(np.float64), 10)
                for name, val in zip(('tpr', 'fpr', 'acc'), V.roc(counts, best)):
                    assert np.array_equal(val, fx['%s_m%d_t%s_%s' % (tag, metric, tt, name)]), (tag, metric, tt, name)
    # set c is where numpy 1 (fp32 comparison) and numpy 2 (fp64) disagree
    assert not np.array_equal(fx['c_m0_t64_tpr'], fx['c_m0_t32_tpr'])


def _lib():
    from cpg_amd import _lib as L
    return L, L.lib()


def _sweep(n, thr, nfolds):
    L, h = _lib()
    thr = np.ascontiguousarray(thr, np.float64)
    rc = h.cpg_pair_sweep(None, None, n, thr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(thr), nfolds, None, None, None)
    return rc, h.cpg_last_error().decode()


@pytest.mark.parametrize('case,n,thr,nfolds,text', [
    ('descending', 100, [0.0, 0.2, 0.1], 10, 'not strictly ascending at entry 2'),
    ('repeated', 100, [0.0, 0.1, 0.1], 10, 'not strictly ascending at entry 2'),
    ('nan_first', 100, [np.nan, 0.1], 10, 'not strictly ascending at entry 0'),
    ('nan_inside', 100, [0.0, np.nan, 0.3], 10, 'not strictly ascending at entry 1'),
    ('one_fold', 100, [0.0, 0.1], 1, 'nfolds must be at least 2'),
    ('fewer_pairs_than_folds', 9, [0.0, 0.1], 10, '9 pairs for 10 folds'),
    ('no_thresholds', 100, [], 10, '0 thresholds'),
    ('too_many_thresholds', 100, np.arange(0, 4, 0.001), 10, '4000 thresholds'),
])
def test_sweep_refuses_bad_arguments_on_the_host(case, n, thr, nfolds, text):
    L, _ = _lib()
    rc, err = _sweep(n, thr, nfolds)
    assert rc == L.CPG_E_INVALID and text in err, (case, rc, err)


def test_sweep_reaches_the_pointer_check_with_good_arguments():
    """A valid table, fold count and pair count pass every argument check: the call then stops at the NULL device pointers."""
    L, _ = _lib()
    rc, err = _sweep(100, np.arange(0, 4, 0.01), 10)
    assert rc == L.CPG_E_INVALID and 'null distances' in err


@pytest.mark.parametrize('d,lda,metric,text', [(0, 0, 0, 'width 0'), (4097, 4097, 0, 'width 4097'), (8, 8, 2, 'metric must be 0'),
                                                (8, 7, 1, 'leading dimensions 7')])
def test_distance_refuses_bad_arguments_on_the_host(d, lda, metric, text):
    L, h = _lib()
    rc = h.cpg_pair_distance(None, lda, None, max(d, 1), 5, d, metric, None, None, None)
    assert rc == L.CPG_E_INVALID and text in h.cpg_last_error().decode()
    assert h.cpg_pair_distance(None, 8, None, 8, 0, 8, 0, None, None, None) == L.CPG_OK          # no pairs: nothing to launch


def test_subtract_mean_and_unknown_options_are_refused():
    from cpg_amd.utils import metrics
    e = np.zeros((12, 4), np.float32)
    with pytest.raises(ValueError, match='subtract_mean'):
        metrics.calculate_roc(np.arange(0, 4, 0.01), e, e, np.zeros(12, bool), subtract_mean=True)
    with pytest.raises(ValueError, match='subtract_mean'):
        metrics.fv_evaluate(e, e, np.zeros(12, bool), subtract_mean=True)
    with pytest.raises(ValueError, match='Undefined distance metric'):
        metrics.distance(e, e, 2)
    with pytest.raises(ValueError, match='threshold_dtype'):
        metrics._thresholds([0.0, 0.5], 'float16')
    thr = metrics._thresholds(np.arange(0, 4, 0.01), 'float32')
    assert thr.dtype == np.float64 and np.array_equal(thr, np.arange(0, 4, 0.01).astype(np.float32).astype(np.float64))
