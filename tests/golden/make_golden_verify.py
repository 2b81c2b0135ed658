#!/usr/bin/env python3
"""Generate tests/golden/verify_roc.npz by RUNNING the reference's LFW scoring (utils/metrics.py: distance, calculate_roc).

Like make_golden.py this imports ivclab/CPG from /root/reference (present only in the build container); nothing of its source
travels, the fixture holds arrays only.  fv_evaluate is not called: its calculate_val raises on current SciPy (interp1d over a FAR
curve that repeats 0.0).  Re-run with

    python tests/golden/make_golden_verify.py

Two embedding sets, pair counts not divisible by 10 (ragged KFold folds):
  * a: 1203 pairs x 64, with exact metric-0 ties (distances equal to a threshold of the table, checked below);
  * b: 311 pairs x 512, with a zero row (metric 1: NaN distance) -- 512 = four numpy summation blocks;
  * c: 53 pairs x 3 (metric 0 only), distances equal to float32-rounded thresholds, where numpy 1 and numpy 2 disagree.
Embeddings are float16 values (stored as float16, used as float32) so that the file stays small.  For each set and metric: the
reference's distances and calculate_roc's (tpr, fpr, accuracy) over np.arange(0, 4, 0.01), and over that table rounded to float32
(the numpy 1.x comparison).  No metric-1 distance lies within 1e-5 of a threshold of either table, so an arccos ulp cannot move a
count.
"""
import os
import sys
import warnings

import numpy as np

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
warnings.filterwarnings('ignore')


def _pairs(rng, n, d, scale):
    """e2 = e1 + noise of a per-pair size; the label says whether the noise was small."""
    e1 = rng.standard_normal((n, d)) * scale
    sigma = rng.uniform(0.05, 1.6, n)
    e2 = e1 + rng.standard_normal((n, d)) * (scale * sigma)[:, None]
    same = sigma + rng.normal(0, 0.3, n) < 0.8
    return e1.astype(np.float16), e2.astype(np.float16), same


def _far_from(dist, tables, eps=1e-5):
    x = dist.astype(np.float64)[:, None]
    far = np.ones(len(dist), bool)
    for thr in tables:
        far &= np.abs(x - thr[None, :]).min(1) > eps
    return np.isnan(dist) | far


def main():
    from utils import metrics as M
    thr64 = np.arange(0, 4, 0.01)
    thr32 = thr64.astype(np.float32)
    tables = [thr64, thr32.astype(np.float64)]
    rng = np.random.default_rng(20261016)
    out = {'thr64': thr64, 'thr32': thr32}
    for tag, n, d in (('a', 1203, 64), ('b', 311, 512)):
        scale = np.sqrt(1.0 / d)                    # metric-0 distances spread over [0, ~4)
        e1, e2, same = _pairs(rng, n, d, scale)
        if tag == 'a':
            # exact metric-0 ties: the pair differs in a few coordinates by powers of two whose squares sum to a table value
            ties = rng.choice(n, 60, replace=False)
            for k, i in enumerate(ties):
                e2[i] = e1[i]
                pat = [(), (0.5,), (1.0,), (0.5, 0.5), (0.5, 0.5, 0.5, 0.5), (1.0, 1.0), (1.0, 1.0, 1.0), (0.5, 1.0)][k % 8]
                cols = rng.choice(d, len(pat), replace=False)
                for c, v in zip(cols, pat):
                    e1[i, c], e2[i, c] = 0, v
        else:
            e1[7] = 0                                # |a| = 0: metric 1 gives NaN
        # metric 1: redraw pairs until no distance sits within 1e-5 of a threshold
        for _ in range(100):
            d1 = M.distance(e1.astype(np.float32), e2.astype(np.float32), 1)
            bad = ~_far_from(d1, tables)
            if not bad.any():
                break
            for i in np.nonzero(bad)[0]:
                noise = rng.standard_normal(d).astype(np.float32) * np.float32(scale * 0.01)
                if tag == 'a' and i in ties:        # keep the metric-0 tie: move both rows alike where they agree
                    eq = e1[i] == e2[i]
                    e1[i, eq] = e2[i, eq] = (e1[i, eq].astype(np.float32) + noise[eq]).astype(np.float16)
                else:
                    e2[i] = (e2[i].astype(np.float32) + noise).astype(np.float16)
        else:
            raise SystemExit('could not separate the metric-1 distances from the thresholds')
        f1, f2 = e1.astype(np.float32), e2.astype(np.float32)
        out[tag + '_e1'], out[tag + '_e2'], out[tag + '_issame'] = e1, e2, same
        for metric in (0, 1):
            dist = M.distance(f1, f2, metric).astype(np.float32)
            if metric == 1:
                assert _far_from(dist, tables).all()
                assert tag != 'b' or np.isnan(dist[7])
            elif tag == 'a':
                on = np.isin(dist[ties].astype(np.float64), thr64) & np.isin(dist[ties].astype(np.float64), thr32.astype(np.float64))
                assert on.all(), on.sum()                # ties by construction: 0, 0.25, 0.5, 1, 1.25, 2, 3 are entries of both tables
            out['%s_dist%d' % (tag, metric)] = dist
            for tt, thr in (('64', thr64), ('32', thr32)):
                tpr, fpr, acc = M.calculate_roc(thr, f1, f2, same, nrof_folds=10, distance_metric=metric, subtract_mean=False)
                out['%s_m%d_t%s_tpr' % (tag, metric, tt)] = tpr
                out['%s_m%d_t%s_fpr' % (tag, metric, tt)] = fpr
                out['%s_m%d_t%s_acc' % (tag, metric, tt)] = acc
    # c: 53 pairs x 3 (float32) whose metric-0 distance IS float32(thr[k]) for thresholds that float32 rounds down -- predicted "same"
    # at thr[k] under numpy 2's fp64 comparison, not under numpy 1's fp32 one: the two tables give different counts
    ks = [k for k in range(1, 400) if np.float64(thr32[k]) < thr64[k]]
    e1, e2, ks_hit = [], [], []
    for k in ks:
        target = thr32[k]
        bits = np.float32(np.sqrt(np.float64(target))).view(np.int32)
        for off in range(-32, 33):                  # float32 neighbours of the square root
            cand = np.int32(bits + off).view(np.float32)
            if np.float32(cand * cand) == target:
                e1.append([0, 0, 0])
                e2.append([0, cand, 0])
                ks_hit.append(k)
                break
        if len(e1) == 53:
            break
    f1, f2 = np.array(e1, np.float32), np.array(e2, np.float32)
    same = rng.random(len(f1)) < 0.5
    dist = M.distance(f1, f2, 0).astype(np.float32)
    assert len(f1) == 53 and np.array_equal(dist, thr32[ks_hit])
    out.update(c_e1=f1, c_e2=f2, c_issame=same, c_dist0=dist)
    for tt, thr in (('64', thr64), ('32', thr32)):
        tpr, fpr, acc = M.calculate_roc(thr, f1, f2, same, nrof_folds=10, distance_metric=0, subtract_mean=False)
        out['c_m0_t%s_tpr' % tt], out['c_m0_t%s_fpr' % tt], out['c_m0_t%s_acc' % tt] = tpr, fpr, acc
    assert not np.array_equal(out['c_m0_t64_tpr'], out['c_m0_t32_tpr'])
    out['numpy_version'] = np.array(np.__version__)
    path = os.path.join(OUT, 'verify_roc.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
