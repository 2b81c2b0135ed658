"""subtract_mean and VAL@FAR on the GPU: cpg_pair_fold_mean, cpg_pair_distance_centred, cpg_pair_sweep_folds, cpg_pair_val_table
and cpg_pair_val_at against the explicit-order restatement (tests/_verify_val.py), and calculate_roc / calculate_val / fv_evaluate
against what the reference returned or raised (tests/golden/verify_val.npz).  Every output and workspace lies between guard bands."""
import ctypes

import numpy as np
import pytest
import torch

import _guarded as G
import _verify as V
import _verify_val as W

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
THR_ROC = np.arange(0, 4, 0.01)
THR_VAL = np.arange(0, 4, 0.001)
GUARDED = ('cpg_amd.utils.metrics',)


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _same(got, want):
    """Bit for bit, a NaN being any NaN (its sign and payload are not arithmetic)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32))


def _embeddings(rng, n, d, special):
    """Order-sensitive rows scaled so that metric-0 distances spread over the thresholds; special: a NaN, a +Inf, a -Inf and a zero
    row among the pairs (each in another fold where there are enough pairs)."""
    e1 = V.adversarial_rows(rng, n, d) if d >= 4 else rng.standard_normal((n, d)).astype(F32)
    e1 = e1 / np.maximum(1.0, np.abs(e1).max(1, keepdims=True)).astype(F32) * F32(1.0 / np.sqrt(d))
    sigma = rng.uniform(0.05, 1.6, n).astype(F32)
    e2 = (e1 + rng.standard_normal((n, d)).astype(F32) * (sigma / F32(np.sqrt(d)))[:, None]).astype(F32)
    if special:
        e1[n // 3, 0] = np.nan
        e2[n // 2, d - 1] = np.inf
        e1[n - 2, d // 2] = -np.inf
        e2[1] = 0
    return e1, e2, sigma < 0.8


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _check_folds(e1, e2, same, F):
    """Every kernel against the restatement for one set of pairs; returns nothing, asserts everything."""
    from cpg_amd.utils import metrics
    n, d = e1.shape
    with G.guarding(GUARDED) as ledger:
        a, b = G.frozen_copy(_dev(e1)), G.frozen_copy(_dev(e2))
        # the means: numpy's bits (NaN and Inf columns included)
        mean = metrics.fold_means(a, b, F)
        want_mean = W.fold_means(e1, e2, F)
        assert _same(mean.cpu().numpy(), want_mean)
        for metric in (0, 1):
            sim = G.guarded((F, n), torch.float32, DEV) if metric == 1 else None
            dist = metrics.centred_distance(a, b, mean, metric, sim=sim)
            got, want = dist.cpu().numpy(), W.centred_distance(e1, e2, want_mean, metric)
            if metric == 0:
                assert _same(got, want)
            else:
                # the cosine of the centred rows bit for bit, the arccos within 2 ulp of float32(acos_fp64(cosine)) * 4 / pi
                got_sim, want_sim = sim.cpu().numpy(), W.centred_cosine(e1, e2, want_mean)
                ok = ~np.isnan(want_sim)
                assert np.array_equal(np.isnan(got_sim), ~ok) and _same(got_sim[ok], want_sim[ok])
                assert np.array_equal(np.isnan(got), np.isnan(want))
                ok = ~np.isnan(want)
                assert not ok.any() or _ulps(got[ok], want[ok]).max() <= 2
            # the sweeps measure with the DEVICE's distances: integer counts, bit-exact given those
            counts, best = metrics.roc_counts(THR_ROC, dist, same, F)
            want_c, want_b = W.sweep_folds(got, same, THR_ROC, F)
            assert np.array_equal(counts, want_c) and np.array_equal(best, want_b)
            for thr in (THR_VAL, np.array([0.0, 0.5, 1.0, 3.0])):
                for rows_, ref in ((dist, got), (dist[F - 1], got[F - 1])):           # a matrix, and one row every fold shares
                    table, totals = metrics.val_counts(thr, rows_, same, F)
                    want_t, want_n = W.val_table(ref, same, thr, F)
                    assert np.array_equal(table, want_t) and np.array_equal(totals, want_n)
            # one threshold per fold: 0, NaN, beyond every distance, Inf, and from there on the fold's own first distance (a tie)
            at = np.resize(np.array([0.0, np.nan, 4.0, np.inf, 0.5]), F)
            for f, (lo, _) in enumerate(V.folds(n, F)):
                if f >= 4 and np.isfinite(got[f, lo]):
                    at[f] = got[f, lo]
            assert np.array_equal(metrics.val_counts_at(at, dist, same, F), W.val_at(got, same, at, F))
            assert np.array_equal(metrics.val_counts_at(at, dist[0], same, F), W.val_at(got[0], same, at, F))
        ledger.verify()
        assert ledger.workspaces >= 4 and ledger.intercepted >= 20


@pytest.mark.parametrize('n,F,d', [(n, 10, d) for n in (10, 23, 600) for d in (1, 8, 9, 128, 129, 512)]
                         + [(23, 2, 1), (23, 2, 129), (301, 7, 1), (301, 7, 129)])
def test_kernels_match_the_restatement(n, F, d):
    rng = np.random.default_rng(n * 7919 + d * 31 + F)
    e1, e2, same = _embeddings(rng, n, d, special=False)
    _check_folds(e1, e2, same, F)


@pytest.mark.parametrize('n,d', [(23, 1), (40, 9), (600, 129)])
def test_kernels_match_the_restatement_with_nan_and_inf(n, d):
    rng = np.random.default_rng(n + d)
    e1, e2, same = _embeddings(rng, n, d, special=True)
    _check_folds(e1, e2, same, 10)


def test_a_strided_view_and_a_long_column():
    """Leading dimensions above the width (a column slice of a wider matrix), and d == 1 with enough rows for numpy's pairwise
    split of the one contiguous column (2 x 540 rows: blocks of 128 and a recursion three deep)."""
    from cpg_amd.utils import metrics
    rng = np.random.default_rng(77)
    wide1, wide2 = (V.adversarial_rows(rng, 600, 12) for _ in range(2))
    for lo, hi in ((3, 4), (2, 11)):
        e1, e2 = np.ascontiguousarray(wide1[:, lo:hi]), np.ascontiguousarray(wide2[:, lo:hi])
        with G.guarding(GUARDED) as ledger:
            a, b = G.frozen_copy(_dev(wide1))[:, lo:hi], G.frozen_copy(_dev(wide2))[:, lo:hi]
            assert a.stride(0) == 12
            mean = metrics.fold_means(a, b, 10)
            want = W.fold_means(e1, e2, 10)
            assert _same(mean.cpu().numpy(), want)
            dist = metrics.centred_distance(a, b, mean, 0)
            assert _same(dist.cpu().numpy(), W.centred_distance(e1, e2, want, 0))
            ledger.verify()


def test_distances_on_a_threshold_and_one_label_folds(golden):
    """Centred metric-0 distances that ARE thresholds (the fixture's `ties`: exact means, differences and squares), and test folds
    without a "same" or without a "different" pair (`single`: one pair a fold)."""
    from cpg_amd.utils import metrics
    fx = golden('verify_val')
    for tag, F in (('ties', 5), ('single', 10)):
        e1, e2, same = fx[tag + '_e1'].astype(F32), fx[tag + '_e2'].astype(F32), fx[tag + '_issame']
        with G.guarding(GUARDED) as ledger:
            dist = metrics.fold_distances(_dev(e1), _dev(e2), same, F, 0, True)
            got = dist.cpu().numpy()
            assert _same(got, fx[tag + '_m0_dist'])
            if tag == 'ties':
                assert np.isin(got.astype(np.float64), THR_ROC).all()
            for thr in (THR_ROC, fx[tag + '_val_thr']):
                table, totals = metrics.val_counts(thr, dist, same, F)
                want_t, want_n = W.val_table(got, same, thr, F)
                assert np.array_equal(table, want_t) and np.array_equal(totals, want_n)
            at = np.resize(np.array([0.25, 1.0, 0.0, 3.0, 0.5]), F)
            c = metrics.val_counts_at(at, dist, same, F)
            assert np.array_equal(c, W.val_at(got, same, at, F))
            if tag == 'single':
                assert ((c[:, 2] == 0) | (c[:, 3] == 0)).all()
                with pytest.raises(ZeroDivisionError):
                    metrics.val_far_at(at, dist, same, F)
            ledger.verify()


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


def test_scoring_matches_the_reference_fixture(golden):
    """calculate_roc(subtract_mean=True), calculate_val and fv_evaluate: the reference's values where it returns, its exception's
    class where it raises (fv_evaluate: under strict=True; by default NaN for val, val_std and far there, as before).  On the parent
    commit subtract_mean=True could not be scored at all and fv_evaluate's last three values were always NaN."""
    from cpg_amd.utils import metrics
    fx = golden('verify_val')
    for tag, e1, e2, same, F, mets, vthr, target in _cases(fx):
        with G.guarding(GUARDED) as ledger:
            a, b = G.frozen_copy(_dev(e1)), G.frozen_copy(_dev(e2))
            assert _same(metrics.fold_means(a, b, F).cpu().numpy(), fx[tag + '_mean']), tag
            for metric in mets:
                key = '%s_m%d_' % (tag, metric)
                res = metrics.calculate_roc(THR_ROC, a, b, same, nrof_folds=F, distance_metric=metric, subtract_mean=True,
                                            accept_subtract_mean=True)
                for name, val in zip(('tpr', 'fpr', 'acc'), res):
                    assert val.dtype == np.float64 and np.array_equal(val, fx[key + name]), (key, name)
                for sm in (0, 1):
                    got, raised = _outcome(lambda: metrics.calculate_val(vthr, a, b, same, target, nrof_folds=F, distance_metric=metric,
                                                                         subtract_mean=bool(sm)))
                    assert raised == str(fx[key + 'val_sm%d_raises' % sm]), (key, sm, raised)
                    if not raised:
                        assert np.array_equal(np.array(got), fx[key + 'val_sm%d' % sm]), (key, sm, got)
                    if F != 10:
                        continue
                    kw = dict(nrof_folds=F, distance_metric=metric, subtract_mean=bool(sm), accept_subtract_mean=bool(sm))
                    got, raised = _outcome(lambda: metrics.fv_evaluate(a, b, same, strict=True, **kw))
                    assert raised == str(fx[key + 'fv_sm%d_raises' % sm]), (key, sm, raised)
                    lenient = metrics.fv_evaluate(a, b, same, **kw)
                    assert len(lenient) == 6
                    if raised:
                        assert all(np.isnan(v) for v in lenient[3:])
                        assert np.array_equal(lenient[2], fx[key + 'acc'] if sm else metrics.calculate_roc(THR_ROC, a, b, same, F, metric)[2])
                    else:
                        for name, val, same_val in zip(('tpr', 'fpr', 'acc', 'val', 'val_std', 'far'), got, lenient):
                            assert np.array_equal(np.asarray(val), fx[key + 'fv_sm%d_%s' % (sm, name)]), (key, sm, name)
                            assert np.array_equal(np.asarray(same_val), np.asarray(val))
            ledger.verify()


def test_calculate_val_far_and_the_public_tables(golden):
    from cpg_amd.utils import metrics
    fx = golden('verify_val')
    e1, e2, same = fx['lfw_e1'].astype(F32), fx['lfw_e2'].astype(F32), fx['lfw_issame']
    with G.guarding(GUARDED) as ledger:
        dist = metrics.fold_distances(_dev(e1), _dev(e2), same, 10, 0, True)
        got = dist.cpu().numpy()
        val_train, far_train = metrics.val_tables(THR_VAL, dist, same, 10)
        table, totals = W.val_table(got, same, THR_VAL, 10)
        assert val_train.shape == far_train.shape == (10, 4000)
        assert np.array_equal(val_train, table[..., 0] / totals[:, None, 0]) and np.array_equal(far_train, table[..., 1] / totals[:, None, 1])
        # the reference's rule has no answer here (far_train repeats values); a caller's own rule is scored on the device all the same
        with pytest.raises(ValueError, match='duplicates'):
            metrics.threshold_at_far(far_train[0], THR_VAL, 1e-3)
        at = [metrics.first_at_far(f, THR_VAL, 1e-3) for f in far_train]
        val, far = metrics.val_far_at(at, dist, same, 10)
        c = W.val_at(got, same, at, 10)
        assert np.array_equal(val, c[:, 0] / c[:, 2]) and np.array_equal(far, c[:, 1] / c[:, 3]) and 0 < val.mean() < 1
        # calculate_val_far on one set of distances, as the reference's (threshold, dist, actual_issame)
        v, f = metrics.calculate_val_far(1.0, dist[0], same)
        pred = got[0].astype(np.float64) < 1.0
        assert (v, f) == (float((pred & same).sum()) / float(same.sum()), float((pred & ~same).sum()) / float((~same).sum()))
        ledger.verify()


def test_default_scoring_is_unchanged(golden):
    """calculate_roc(subtract_mean=False) and a Manager's default score_pairs give the existing entry points' bits on verify_roc.npz;
    full=True adds VAL@FAR without moving them."""
    from cpg_amd import _lib
    from cpg_amd.utils import metrics
    from cpg_amd.utils.manager import ManagerBase
    fx = golden('verify_roc')
    e1, e2, same = (fx['b_e1'].astype(F32), fx['b_e2'].astype(F32), fx['b_issame'])
    a, b = _dev(e1), _dev(e2)
    n, d = e1.shape
    dist = torch.empty(n, device=DEV)
    _lib.call('cpg_pair_distance', _lib.dptr(a), d, _lib.dptr(b), d, n, d, 1, _lib.dptr(dist), None, _lib.stream_ptr())
    thr = np.ascontiguousarray(THR_ROC)
    counts = torch.empty((10, 400, 4), dtype=torch.int64, device=DEV)
    best = torch.empty(10, dtype=torch.int64, device=DEV)
    lab = torch.from_numpy(same.astype(np.uint8)).to(DEV)
    _lib.call('cpg_pair_sweep', _lib.dptr(dist), _lib.dptr(lab, torch.uint8), n, thr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 400, 10,
              ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(best.data_ptr()), _lib.stream_ptr())
    want = metrics.roc_from_counts(counts.cpu().numpy(), best.cpu().numpy())
    got = metrics.calculate_roc(THR_ROC, a, b, same, distance_metric=1)
    for g, w, name in zip(got, want, ('tpr', 'fpr', 'acc')):
        assert np.array_equal(g, w) and np.array_equal(g, fx['b_m1_t64_' + name])
    assert torch.equal(metrics.fold_distances(a, b, same, 10, 1, False).view(torch.int32), dist.view(torch.int32))

    class Mgr(ManagerBase):
        def __init__(self):
            self.args = type('A', (), {})()
            self.last_stats, self.last_lfw, self.progress = {}, None, False
    mgr = Mgr()
    batches = [(a[:200], b[:200], same[:200]), (a[200:], b[200:], same[200:])]
    acc = mgr.score_pairs(batches)
    assert acc == np.mean(want[2]) and set(mgr.last_lfw) == {'tpr', 'fpr', 'accuracy'} and np.array_equal(mgr.last_lfw['accuracy'], want[2])
    assert mgr.score_pairs(batches, full=True) == acc
    full = mgr.last_lfw
    assert np.array_equal(full['accuracy'], want[2]) and full['far_train'].shape == (10, 4000)
    assert np.isnan(full['val']) and 'duplicates' in full['val_error'] and 0 < full['val_first'] <= 1 and 0 <= full['far_first'] < 1
    centred = mgr.score_pairs(batches, full=True, subtract_mean=True)
    with pytest.raises(ValueError, match='accept_subtract_mean'):        # the refusal of a bare subtract_mean=True stays
        metrics.calculate_roc(THR_ROC, a, b, same, distance_metric=1, subtract_mean=True)
    res = metrics.calculate_roc(THR_ROC, a, b, same, distance_metric=1, subtract_mean=True, accept_subtract_mean=True)
    assert centred == np.mean(res[2]) and np.array_equal(mgr.last_lfw['tpr'], res[0])
