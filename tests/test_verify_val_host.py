"""subtract_mean and VAL@FAR on the host: the explicit-order restatement (tests/_verify_val.py) against numpy and against what the
reference itself returned or raised (tests/golden/verify_val.npz), the product's host half (the interpolation, the ratios), and the
library's refusals of bad arguments, which happen before anything touches the device."""
import ctypes

import numpy as np
import pytest

import _verify as V
import _verify_val as W

F32 = np.float32
ROWS = [1, 2, 7, 8, 9, 127, 128, 129, 1025]
THR_ROC = np.arange(0, 4, 0.01)


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _same(got, want):
    """Bit for bit, a NaN being any NaN (its sign and payload are not arithmetic)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def _adversarial_columns(rng, m, d):
    """Columns whose float32 sum depends on the order: wide magnitudes, a cancelling pair of 1e8, denormals; then columns with NaN,
    +Inf, -Inf, both infinities and -0.0 only."""
    x = (rng.standard_normal((m, d)) * 2.0 ** rng.integers(-20, 20, (m, d))).astype(F32)
    x[rng.random((m, d)) < 0.1] = F32(1e-42)
    if m >= 2:
        k, j = rng.integers(0, m, d), rng.integers(0, m, d)
        x[k, np.arange(d)] = 1e8
        x[j, np.arange(d)] = -x[k, np.arange(d)]
    special = [np.nan, np.inf, -np.inf]
    for c in range(min(d, 5)):
        if c < 3:
            x[rng.integers(0, m), c] = special[c]
        elif c == 3 and m >= 2:
            x[0, c], x[m - 1, c] = np.inf, -np.inf
        elif c == 4:
            x[:, c] = -0.0
    return x


@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('d', [1, 2, 3, 8, 9, 129])
def test_col_mean_is_numpys_axis0_order(m, d):
    rng = np.random.default_rng(m * 1000 + d)
    for trial in range(3):
        x = _adversarial_columns(rng, m, d) if trial else (rng.standard_normal((m, d)) * 1e3).astype(F32)
        with np.errstate(all='ignore'):
            want = np.mean(x, axis=0)
        got = W.col_mean(x)
        assert want.dtype == F32 and _same(got, want), (m, d, trial)


def test_other_orders_are_different_orders():
    """What col_mean pins is not vacuous: pairwise blocks over the rows of a wide matrix, or rows in order for one column, change bits."""
    rng = np.random.default_rng(3)
    x = _adversarial_columns(rng, 1025, 9)[:, 5:]
    pairwise = V.row_sum(np.ascontiguousarray(x.T)) / F32(1025)
    assert not _same(pairwise, np.mean(x, axis=0))
    cols = rng.standard_normal((1025, 16)).astype(F32)
    in_order = np.zeros(16, F32)
    for i in range(1025):
        in_order = in_order + cols[i]
    alone = np.array([np.mean(np.ascontiguousarray(cols[:, c:c + 1]), axis=0)[0] for c in range(16)])
    assert not _same(in_order / F32(1025), alone)


def _cases(fx):
    for tag in fx['cases']:
        tag = str(tag)
        yield (tag, fx[tag + '_e1'].astype(F32), fx[tag + '_e2'].astype(F32), fx[tag + '_issame'], int(fx[tag + '_folds']),
               [int(m) for m in fx[tag + '_metrics']], fx[tag + '_val_thr'], float(fx[tag + '_far_target']))


def _outcome(fn):
    try:
        return fn(), ''
    except (ValueError, ZeroDivisionError) as e:
        return None, type(e).__name__


def test_restatement_matches_the_reference_fixture(golden):
    fx = golden('verify_val')
    seen = set()
    for tag, e1, e2, same, F, metrics, vthr, target in _cases(fx):
        means = W.fold_means(e1, e2, F)
        assert _same(means, fx[tag + '_mean']), tag
        for metric in metrics:
            key = '%s_m%d_' % (tag, metric)
            dist, want = W.centred_distance(e1, e2, means, metric), fx[key + 'dist']
            if metric == 0:
                assert _same(dist, want), key
            else:
                # numpy's float32 arccos and the kernel's fp64 one differ by ulps; the fixture keeps every metric-1 distance 1e-6
                # away from the thresholds it is scored on, so agreement within that leaves every count where it is
                ok = ~np.isnan(want)
                assert np.array_equal(np.isnan(dist), ~ok) and (not ok.any() or np.abs(dist[ok].astype(np.float64) - want[ok]).max() < 1e-6), key
            counts, best = W.sweep_folds(dist, same, THR_ROC, F)
            for name, val in zip(('tpr', 'fpr', 'acc'), V.roc(counts, best)):
                assert np.array_equal(val, fx[key + name]), (key, name)
            for sm, d in ((0, V.distance(e1, e2, metric)), (1, dist)):
                got, raised = _outcome(lambda: W.calculate_val(vthr, d, same, target, F))
                assert raised == str(fx[key + 'val_sm%d_raises' % sm]), (key, sm, raised)
                seen.add(('val', raised))
                if not raised:
                    assert np.array_equal(np.array(got), fx[key + 'val_sm%d' % sm]), (key, sm)
                if F == 10:
                    got, raised = _outcome(lambda: W.fv_evaluate(e1, e2, same, F, metric, bool(sm)))
                    assert raised == str(fx[key + 'fv_sm%d_raises' % sm]), (key, sm, raised)
                    seen.add(('fv', raised))
                    for name, val in zip(('tpr', 'fpr', 'acc', 'val', 'val_std', 'far'), got or ()):
                        assert np.array_equal(np.asarray(val), fx[key + 'fv_sm%d_%s' % (sm, name)]), (key, sm, name)
    # the fixture shows every outcome: a value from the interpolation, the threshold-0 branch, and both of the reference's errors
    assert seen >= {('val', ''), ('val', 'ValueError'), ('val', 'ZeroDivisionError'), ('fv', ''), ('fv', 'ValueError')}
    assert fx['uneven_m0_val_sm1'][2] > 0 and fx['apart_m0_fv_sm1_far'] == 0


def _interp_cases(fx):
    for x, y, t, v, err in zip(fx['interp_x'], fx['interp_y'], fx['interp_t'], fx['interp_value'], fx['interp_raises']):
        keep = ~np.isnan(x)
        yield x[keep], y[keep], float(t), float(v), str(err)


def test_slinear_restatements_match_scipys_recorded_results(golden):
    from cpg_amd.utils import metrics
    fx = golden('verify_val')
    outcomes = set()
    for x, y, t, v, err in _interp_cases(fx):
        for fn in (W.slinear, metrics.slinear):
            got, raised = _outcome(lambda: fn(x, y, t))
            assert raised == err and (err or float(got) == v), (fn.__module__, x, t, got, v, raised, err)
        outcomes.add(err)
    assert outcomes == {'', 'ValueError'}


def test_threshold_rules_and_ratios_on_the_host():
    from cpg_amd.utils import metrics
    thr = np.array([0.0, 1.0, 2.0, 3.5])
    assert metrics.threshold_at_far(np.array([0.0, 0.0, 0.0, 0.0]), thr, 1e-3) == 0.0           # max(far_train) < far_target
    assert metrics.threshold_at_far(np.array([0.0, 0.25, 0.5, 1.0]), thr, 0.25) == 1.0
    assert metrics.threshold_at_far(np.array([0.0, 0.25, 0.5, 1.0]), thr, 0.3) == W.slinear([0.0, 0.25, 0.5, 1.0], thr, 0.3)
    with pytest.raises(ValueError, match='duplicates'):
        metrics.threshold_at_far(np.array([0.0, 0.0, 0.5, 1.0]), thr, 0.25)
    with pytest.raises(ValueError, match='below'):
        metrics.threshold_at_far(np.array([0.1, 0.25, 0.5, 1.0]), thr, 0.05)
    assert metrics.first_at_far(np.array([0.0, 0.0, 0.5, 1.0]), thr, 0.25) == 1.0
    assert metrics.first_at_far(np.array([0.3, 0.4, 0.5, 1.0]), thr, 0.25) == 0.0
    val, far = metrics._val_far(np.array([[1, 2], [3, 0]]), np.array([[3, 7], [3, 7]]))
    assert val.tolist() == [1 / 3, 1.0] and far.tolist() == [2 / 7, 0.0]
    with pytest.raises(ZeroDivisionError):
        metrics._val_far(np.array([[0, 0]]), np.array([[0, 5]]))


def _lib():
    from cpg_amd import _lib as L
    return L, L.lib()


def _f64(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def test_val_planners_answer_on_the_host():
    L, h = _lib()
    top = h.cpg_pair_val_max_thresholds()
    assert top >= 4000                                              # fv_evaluate's np.arange(0, 4, 0.001) fits
    assert 8 * (top + 1) + 8 * 256 <= 64 * 1024 < 8 * (top + 2) + 8 * 256       # two int histograms of n_thr + 1, the scan's carries
    assert h.cpg_pair_val_workspace_bytes(4000) == 32000 and h.cpg_pair_val_workspace_bytes(top) == 8 * top
    assert h.cpg_pair_val_workspace_bytes(0) == 0 and h.cpg_pair_val_workspace_bytes(top + 1) == 0


@pytest.mark.parametrize('case,n,thr,nfolds,ldd,text', [
    ('too_long', 100, 'top+1', 10, 0, 'thresholds outside'),
    ('none', 100, [], 10, 0, '0 thresholds'),
    ('descending', 100, [0.0, 0.2, 0.1], 10, 0, 'not strictly ascending at entry 2'),
    ('nan', 100, [0.0, np.nan], 10, 0, 'not strictly ascending at entry 1'),
    ('one_fold', 100, [0.0, 0.1], 1, 0, 'nfolds must be at least 2'),
    ('few_pairs', 9, [0.0, 0.1], 10, 0, '9 pairs for 10 folds'),
    ('short_rows', 100, [0.0, 0.1], 10, 99, 'leading dimension 99'),
    ('good', 100, np.arange(0, 4, 0.001), 10, 100, 'null distances'),
])
def test_val_table_refuses_bad_arguments_on_the_host(case, n, thr, nfolds, ldd, text):
    L, h = _lib()
    if isinstance(thr, str):
        thr = np.arange(h.cpg_pair_val_max_thresholds() + 1) * 1e-4
    thr, p = _f64(thr)
    rc = h.cpg_pair_val_table(None, ldd, None, n, p, len(thr), nfolds, None, None, None, 0, None)
    assert rc == L.CPG_E_INVALID and text in h.cpg_last_error().decode(), (case, h.cpg_last_error())


def test_the_other_new_entry_points_refuse_bad_arguments_on_the_host():
    L, h = _lib()
    thr, p = _f64(np.arange(0, 4, 0.01))

    def refused(rc, text):
        return rc == L.CPG_E_INVALID and text in h.cpg_last_error().decode()

    assert refused(h.cpg_pair_fold_mean(None, 8, None, 8, 100, 8, 1, None, None), 'nfolds must be at least 2')
    assert refused(h.cpg_pair_fold_mean(None, 8, None, 8, 5, 8, 10, None, None), '5 pairs for 10 folds')
    assert refused(h.cpg_pair_fold_mean(None, 7, None, 8, 100, 8, 10, None, None), 'leading dimensions 7')
    assert refused(h.cpg_pair_fold_mean(None, 8, None, 8, 100, 8, 10, None, None), 'null embeddings')
    assert refused(h.cpg_pair_distance_centred(None, 8, None, 8, 5, 8, 2, None, 10, None, None, None), 'metric must be 0')
    assert refused(h.cpg_pair_distance_centred(None, 8, None, 8, 5, 8, 0, None, 0, None, None, None), '0 folds outside')
    assert refused(h.cpg_pair_distance_centred(None, 8, None, 8, 5, 8, 0, None, 10, None, None, None), 'null embeddings, means')
    assert h.cpg_pair_distance_centred(None, 8, None, 8, 0, 8, 0, None, 10, None, None, None) == L.CPG_OK     # no pairs: no launch
    assert refused(h.cpg_pair_sweep_folds(None, 99, None, 100, p, len(thr), 10, None, None, None), 'leading dimension 99')
    assert refused(h.cpg_pair_sweep_folds(None, 100, None, 100, p, 481, 10, None, None, None), '481 thresholds')
    assert refused(h.cpg_pair_sweep_folds(None, 100, None, 100, p, len(thr), 10, None, None, None), 'null distances')
    assert refused(h.cpg_pair_val_at(None, 0, None, 100, p, 0, None, None), 'nfolds must be at least 1')
    assert refused(h.cpg_pair_val_at(None, 50, None, 100, p, 10, None, None), 'leading dimension 50')
    assert refused(h.cpg_pair_val_at(None, 0, None, 100, None, 10, None, None), 'null threshold table')
    assert refused(h.cpg_pair_val_at(None, 0, None, 100, p, 10, None, None), 'null distances')
