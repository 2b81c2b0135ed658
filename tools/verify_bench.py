#!/usr/bin/env python3
"""Cost of LFW pair scoring (cpg_amd/utils/metrics.py, cpg_amd/csrc/verify_kernels.hip) on one MI355X, and of the host computation it
replaces.

  device  6 000 pairs x 512 (LFW's size): cpg_pair_distance (metric 1, what evalLFW uses) and cpg_pair_sweep (10 folds x 400
          thresholds), each in HIP events over --reps launches; and a whole calculate_roc call (both kernels, the counts' copy to the
          host, tpr / fpr / accuracy), device-synchronised wall clock.
  host    the same scoring the reference's way: numpy distance (np.sum, np.linalg.norm, np.arccos), then for every fold the
          400 + 400 calculate_accuracy calls of calculate_roc on the train and test slices.
  fv      the whole of fv_evaluate's work at the same size, subtract_mean False and True: the folds' distances (with the means and
          the centred F x n distance matrix when subtract_mean), calculate_roc's sweep over 400 thresholds and calculate_val's over
          4 000, the thresholds at FAR = 1e-3 and the test folds' val / far.  The reference's own interpolation raises on such a
          table (far_train repeats values), so both sides pick the thresholds with first_at_far's rule.  Device: every new kernel in
          HIP events, and the whole call in device-synchronised wall clock.  Host: the reference's loops in numpy, as `host` above.
  evallfw Manager.evalLFW of a width-1.0 SphereNet-20 over 6 000 PairLoader pairs drawn from a synthetic 12 000-image store at
          112 x 112, batch 256: embeddings, scoring, logging -- device-synchronised wall clock.

Synthetic data: the cost depends on the sizes only.  Prints one JSON object, writes it to --out and a summary to --md.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PAIRS, DIM, FOLDS = 6000, 512, 10


def _pairs(rng, n=N_PAIRS, d=DIM):
    e1 = rng.standard_normal((n, d)).astype(np.float32)
    sigma = rng.uniform(0.2, 2.0, n).astype(np.float32)
    e2 = (e1 + rng.standard_normal((n, d)).astype(np.float32) * sigma[:, None]).astype(np.float32)
    return e1, e2, sigma < 1.0


def part_device(reps):
    import ctypes
    import torch
    from cpg_amd import _lib
    from cpg_amd.utils import metrics
    rng = np.random.default_rng(1)
    e1, e2, same = _pairs(rng)
    a, b = torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda()
    thr = np.arange(0, 4, 0.01)
    dist = torch.empty(N_PAIRS, device='cuda')
    lab = torch.from_numpy(same.astype(np.uint8)).cuda()
    counts = torch.empty((FOLDS, len(thr), 4), dtype=torch.int64, device='cuda')
    best = torch.empty(FOLDS, dtype=torch.int64, device='cuda')
    h = _lib.lib()
    thr_p = thr.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def dist_call():
        _lib.check('cpg_pair_distance', h.cpg_pair_distance(_lib.dptr(a), DIM, _lib.dptr(b), DIM, N_PAIRS, DIM, 1, _lib.dptr(dist), None,
                                                            _lib.stream_ptr()))

    def sweep_call():
        _lib.check('cpg_pair_sweep', h.cpg_pair_sweep(_lib.dptr(dist), _lib.dptr(lab, torch.uint8), N_PAIRS, thr_p, len(thr), FOLDS,
                                                      ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(best.data_ptr()),
                                                      _lib.stream_ptr()))

    def events(fn):
        for _ in range(5):
            fn()
        out = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            out.append(s.elapsed_time(e))
        return out

    t_dist = events(dist_call)
    t_sweep = events(sweep_call)
    walls = []
    for i in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metrics.calculate_roc(thr, a, b, same, nrof_folds=FOLDS, distance_metric=1)
        torch.cuda.synchronize()
        if i >= 3:
            walls.append((time.perf_counter() - t0) * 1e3)
    med = lambda v: float(np.median(v))
    return {'pairs': N_PAIRS, 'dim': DIM, 'folds': FOLDS, 'thresholds': len(thr), 'reps': reps,
            'distance_kernel_ms_median': med(t_dist), 'distance_kernel_ms_min': float(min(t_dist)),
            'sweep_kernel_ms_median': med(t_sweep), 'sweep_kernel_ms_min': float(min(t_sweep)),
            'kernels_ms_median': med(t_dist) + med(t_sweep),
            'calculate_roc_wall_ms_median': med(walls), 'calculate_roc_wall_ms_min': float(min(walls)),
            'device': torch.cuda.get_device_name(0)}


def _device_fv(metrics, a, b, same, subtract_mean):
    thr = np.arange(0, 4, 0.001)
    dist = metrics.fold_distances(a, b, same, FOLDS, 1, subtract_mean)
    roc = metrics.roc_from_counts(*metrics.roc_counts(np.arange(0, 4, 0.01), dist, same, FOLDS))
    _, far_train = metrics.val_tables(thr, dist, same, FOLDS)
    val, far = metrics.val_far_at([metrics.first_at_far(f, thr, 1e-3) for f in far_train], dist, same, FOLDS)
    return roc + (np.mean(val), np.std(val), np.mean(far))


def part_fv(reps, host_reps):
    import ctypes
    import torch
    from cpg_amd import _lib
    from cpg_amd.utils import metrics
    rng = np.random.default_rng(1)
    e1, e2, same = _pairs(rng)
    a, b = torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda()
    lab = torch.from_numpy(same.astype(np.uint8)).cuda()
    h = _lib.lib()
    sp, i64 = _lib.stream_ptr, lambda t: ctypes.c_void_p(t.data_ptr())
    thr_roc, thr_val = np.arange(0, 4, 0.01), np.arange(0, 4, 0.001)
    p_roc, p_val = (t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for t in (thr_roc, thr_val))
    mean = torch.empty((FOLDS, DIM), device='cuda')
    dist = torch.empty((FOLDS, N_PAIRS), device='cuda')
    counts = torch.empty((FOLDS, 400, 4), dtype=torch.int64, device='cuda')
    best = torch.empty(FOLDS, dtype=torch.int64, device='cuda')
    table = torch.empty((FOLDS, 4000, 2), dtype=torch.int64, device='cuda')
    totals = torch.empty((FOLDS, 2), dtype=torch.int64, device='cuda')
    out = torch.empty((FOLDS, 4), dtype=torch.int64, device='cuda')
    ws, nbytes = _lib.workspace(int(h.cpg_pair_val_workspace_bytes(4000)), 'cuda')
    at = np.full(FOLDS, 0.9)
    p_at = at.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    calls = {
        'fold_mean': lambda: h.cpg_pair_fold_mean(_lib.dptr(a), DIM, _lib.dptr(b), DIM, N_PAIRS, DIM, FOLDS, _lib.dptr(mean), sp()),
        'distance_centred': lambda: h.cpg_pair_distance_centred(_lib.dptr(a), DIM, _lib.dptr(b), DIM, N_PAIRS, DIM, 1, _lib.dptr(mean), FOLDS,
                                                                _lib.dptr(dist), None, sp()),
        'sweep_folds': lambda: h.cpg_pair_sweep_folds(_lib.dptr(dist), N_PAIRS, _lib.dptr(lab, torch.uint8), N_PAIRS, p_roc, 400, FOLDS,
                                                      i64(counts), i64(best), sp()),
        'val_table_rows': lambda: h.cpg_pair_val_table(_lib.dptr(dist), N_PAIRS, _lib.dptr(lab, torch.uint8), N_PAIRS, p_val, 4000, FOLDS,
                                                       i64(table), i64(totals), _lib.dptr(ws), nbytes, sp()),
        'val_table_shared': lambda: h.cpg_pair_val_table(_lib.dptr(dist), 0, _lib.dptr(lab, torch.uint8), N_PAIRS, p_val, 4000, FOLDS,
                                                         i64(table), i64(totals), _lib.dptr(ws), nbytes, sp()),
        'val_at': lambda: h.cpg_pair_val_at(_lib.dptr(dist), N_PAIRS, _lib.dptr(lab, torch.uint8), N_PAIRS, p_at, FOLDS, i64(out), sp()),
    }
    rec = {'pairs': N_PAIRS, 'dim': DIM, 'folds': FOLDS, 'reps': reps, 'host_reps': host_reps, 'kernels_ms': {}}
    for name, fn in calls.items():
        ts = []
        for i in range(reps + 5):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            _lib.check(name, fn())
            e.record()
            e.synchronize()
            if i >= 5:
                ts.append(s.elapsed_time(e))
        rec['kernels_ms'][name] = {'median': float(np.median(ts)), 'min': float(min(ts))}
    for sm in (False, True):
        walls = []
        for i in range(reps + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = _device_fv(metrics, a, b, same, sm)
            torch.cuda.synchronize()
            if i >= 3:
                walls.append((time.perf_counter() - t0) * 1e3)
        hosts = []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            want = _host_fv(e1, e2, same, sm)
            hosts.append((time.perf_counter() - t0) * 1e3)
        key = 'subtract_mean' if sm else 'plain'
        rec[key] = {'device_wall_ms_median': float(np.median(walls)), 'device_wall_ms_min': float(min(walls)),
                    'host_wall_ms_median': float(np.median(hosts)), 'host_wall_ms_min': float(min(hosts)),
                    'device_accuracy': float(np.mean(got[2])), 'host_accuracy': float(np.mean(want[2])),
                    'device_val': float(got[3]), 'host_val': float(want[3])}
    rec['numpy'], rec['threads'] = np.__version__, os.environ.get('OMP_NUM_THREADS')
    return rec


def _host_accuracy(threshold, dist, issame):
    predict = np.less(dist, threshold)
    tp = np.sum(np.logical_and(predict, issame))
    fp = np.sum(np.logical_and(predict, np.logical_not(issame)))
    tn = np.sum(np.logical_and(np.logical_not(predict), np.logical_not(issame)))
    fn = np.sum(np.logical_and(np.logical_not(predict), issame))
    tpr = 0 if (tp + fn == 0) else float(tp) / float(tp + fn)
    fpr = 0 if (fp + tn == 0) else float(fp) / float(fp + tn)
    return tpr, fpr, float(tp + tn) / dist.size


def _host_roc(thr, e1, e2, issame):
    dot = np.sum(np.multiply(e1, e2), axis=1)
    norm = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    dist = np.arccos(np.clip(dot / norm, 0, 1)) * 4 / math.pi
    n, T = len(issame), len(thr)
    tprs, fprs, acc = np.zeros((FOLDS, T)), np.zeros((FOLDS, T)), np.zeros(FOLDS)
    q, r = divmod(n, FOLDS)
    at = 0
    for f in range(FOLDS):
        size = q + (1 if f < r else 0)
        test = np.arange(at, at + size)
        train = np.concatenate([np.arange(0, at), np.arange(at + size, n)])
        at += size
        acc_train = np.array([_host_accuracy(t, dist[train], issame[train])[2] for t in thr])
        b = int(np.argmax(acc_train))
        for i, t in enumerate(thr):
            tprs[f, i], fprs[f, i], _ = _host_accuracy(t, dist[test], issame[test])
        acc[f] = _host_accuracy(thr[b], dist[test], issame[test])[2]
    return np.mean(tprs, 0), np.mean(fprs, 0), acc


def _host_distance(e1, e2):
    dot = np.sum(np.multiply(e1, e2), axis=1)
    norm = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    return np.arccos(np.clip(dot / norm, 0, 1)) * 4 / math.pi


def _host_val_far(threshold, dist, issame):
    predict = np.less(dist, threshold)
    ta = np.sum(np.logical_and(predict, issame))
    fa = np.sum(np.logical_and(predict, np.logical_not(issame)))
    return float(ta) / float(np.sum(issame)), float(fa) / float(np.sum(np.logical_not(issame)))


def _host_fv(e1, e2, issame, subtract_mean):
    """fv_evaluate the reference's way (calculate_roc, then calculate_val, each with its own distances per fold), the threshold at
    the FAR target by first_at_far's rule."""
    thr_roc, thr_val = np.arange(0, 4, 0.01), np.arange(0, 4, 0.001)
    n = len(issame)
    tprs, fprs, acc = np.zeros((FOLDS, 400)), np.zeros((FOLDS, 400)), np.zeros(FOLDS)
    val, far = np.zeros(FOLDS), np.zeros(FOLDS)
    q, r = divmod(n, FOLDS)
    for which in ('roc', 'val'):
        at = 0
        for f in range(FOLDS):
            size = q + (1 if f < r else 0)
            test = np.arange(at, at + size)
            train = np.concatenate([np.arange(0, at), np.arange(at + size, n)])
            at += size
            mean = np.mean(np.concatenate([e1[train], e2[train]]), axis=0) if subtract_mean else 0.0
            dist = _host_distance(e1 - mean, e2 - mean)
            if which == 'roc':
                acc_train = np.array([_host_accuracy(t, dist[train], issame[train])[2] for t in thr_roc])
                b = int(np.argmax(acc_train))
                for i, t in enumerate(thr_roc):
                    tprs[f, i], fprs[f, i], _ = _host_accuracy(t, dist[test], issame[test])
                acc[f] = _host_accuracy(thr_roc[b], dist[test], issame[test])[2]
            else:
                far_train = np.array([_host_val_far(t, dist[train], issame[train])[1] for t in thr_val])
                ok = np.nonzero(far_train <= 1e-3)[0]
                val[f], far[f] = _host_val_far(thr_val[ok[-1]] if len(ok) else 0.0, dist[test], issame[test])
    return np.mean(tprs, 0), np.mean(fprs, 0), acc, np.mean(val), np.std(val), np.mean(far)


def part_host(reps):
    rng = np.random.default_rng(1)
    e1, e2, same = _pairs(rng)
    thr = np.arange(0, 4, 0.01)
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _host_roc(thr, e1, e2, same)
        walls.append((time.perf_counter() - t0) * 1e3)
    return {'pairs': N_PAIRS, 'dim': DIM, 'reps': reps, 'wall_ms_median': float(np.median(walls)), 'wall_ms_min': float(min(walls)),
            'numpy': np.__version__, 'threads': os.environ.get('OMP_NUM_THREADS')}


def part_evallfw(reps, batch):
    import torch
    import cpg_amd.models as M
    from cpg_amd import data as D
    from cpg_amd.driver import default_args
    from cpg_amd.models import layers as nl
    from cpg_amd.utils.manager import Manager
    rng = np.random.default_rng(2)
    n_img = 2 * N_PAIRS
    block = rng.integers(0, 256, (n_img, 112, 112, 3), dtype=np.uint8)
    store = D.ImageStore.from_arrays(list(block), np.zeros(n_img, np.int64), 'cuda')
    del block
    pairs = [(2 * i, 2 * i + 1, bool(i % 2)) for i in range(N_PAIRS)]
    loader = D.PairLoader(store, pairs, batch)
    torch.manual_seed(1)
    net = M.spherenet20(dataset_history=[], dataset2num_classes={}, network_width_multiplier=1.0, shared_layer_info={})
    net.add_dataset('face_verification', 10572)
    net.set_dataset('face_verification')
    net = net.cuda()
    masks = {n: torch.ones(m.weight.shape, dtype=torch.uint8, device='cuda') for n, m in net.named_modules()
             if isinstance(m, (nl.SharableConv2d, nl.SharableLinear))}
    mgr = Manager(default_args(dataset='face_verification', network_width_multiplier=1.0), net, {}, masks, None, loader, 0, 1)
    walls, accs = [], []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        accs.append(float(mgr.evalLFW(0)))
        torch.cuda.synchronize()
        if i >= 1:
            walls.append((time.perf_counter() - t0) * 1e3)
    return {'images': n_img, 'pairs': N_PAIRS, 'batch': batch, 'batches': len(loader), 'reps': reps, 'wall_ms_median': float(np.median(walls)),
            'wall_ms_min': float(min(walls)), 'pairs_per_s': N_PAIRS / (float(np.median(walls)) / 1e3), 'accuracy': accs[-1]}


def _md(rec, cmd):
    d, h, e, v = rec.get('device'), rec.get('host'), rec.get('evallfw'), rec.get('fv')
    out = ['# LFW pair scoring: device kernels, the host computation they replace, and a whole evalLFW (`tools/verify_bench.py`)', '',
           'One MI355X, one process.  Record: `verify_bench.json`, written by `%s`.  Synthetic data: the cost depends on the sizes only.' % cmd,
           '']
    if d:
        out += ['## Device scoring: %d pairs x %d, metric 1, %d folds x %d thresholds' % (d['pairs'], d['dim'], d['folds'], d['thresholds']), '',
                '| step | median ms | min ms |', '|---|---|---|',
                '| cpg_pair_distance (HIP events) | %.4f | %.4f |' % (d['distance_kernel_ms_median'], d['distance_kernel_ms_min']),
                '| cpg_pair_sweep (HIP events) | %.4f | %.4f |' % (d['sweep_kernel_ms_median'], d['sweep_kernel_ms_min']),
                '| calculate_roc, whole call (wall clock: both kernels, counts to the host, tpr / fpr / accuracy) | %.3f | %.3f |'
                % (d['calculate_roc_wall_ms_median'], d['calculate_roc_wall_ms_min']), '']
    if h:
        out += ['## Host restatement: numpy distance + the reference\'s calculate_roc loops (%s threads, numpy %s)' % (h['threads'], h['numpy']), '',
                '| step | median ms | min ms |', '|---|---|---|',
                '| distance + 10 folds x (400 train + 400 test) calculate_accuracy | %.1f | %.1f |' % (h['wall_ms_median'], h['wall_ms_min']), '']
    if v:
        out += ['## fv_evaluate\'s whole work (roc over 400 thresholds, VAL@FAR over 4 000), %d pairs x %d, metric 1, %d folds' % (v['pairs'], v['dim'], v['folds']),
                '', '| kernel (HIP events) | median ms | min ms |', '|---|---|---|']
        out += ['| cpg_pair_%s | %.4f | %.4f |' % (k, t['median'], t['min']) for k, t in v['kernels_ms'].items()]
        out += ['', '| whole call (wall clock) | device median ms | device min ms | host numpy median ms | host min ms |', '|---|---|---|---|---|']
        out += ['| subtract_mean=%s | %.3f | %.3f | %.1f | %.1f |' % (k == 'subtract_mean', v[k]['device_wall_ms_median'], v[k]['device_wall_ms_min'],
                                                                      v[k]['host_wall_ms_median'], v[k]['host_wall_ms_min']) for k in ('plain', 'subtract_mean')]
        out += ['', 'Host: the reference\'s loops in numpy %s with %s threads; both sides take each fold\'s threshold by first_at_far\'s rule (the '
                'reference\'s interpolation raises on this table).' % (v['numpy'], v['threads']), '']
    if e:
        out += ['## Manager.evalLFW: SphereNet-20 width 1.0, %d pairs from a %d-image store at 112 x 112, batch %d'
                % (e['pairs'], e['images'], e['batch']), '',
                '| | median ms | min ms | pairs/s |', '|---|---|---|---|',
                '| evalLFW (2 x %d forward_to_embeddings batches + scoring) | %.1f | %.1f | %.0f |'
                % (e['batches'], e['wall_ms_median'], e['wall_ms_min'], e['pairs_per_s']), '']
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'device', 'host', 'fv', 'evallfw'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--lfw-reps', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'verify_bench.json'))
    ap.add_argument('--md', default=os.path.join(ROOT, 'profiles', 'verify_bench.md'))
    a = ap.parse_args()
    rec = {}
    if a.part in ('all', 'device'):
        rec['device'] = part_device(a.reps)
    if a.part in ('all', 'host'):
        rec['host'] = part_host(a.host_reps)
    if a.part in ('all', 'fv'):
        rec['fv'] = part_fv(a.reps, a.host_reps)
    if a.part in ('all', 'evallfw'):
        rec['evallfw'] = part_evallfw(a.lfw_reps, a.batch)
    argv, skip = [], False
    for x in sys.argv[1:]:                          # the recorded command leaves out where the record was written
        if skip or x in ('--out', '--md') or x.startswith(('--out=', '--md=')):
            skip = x in ('--out', '--md')
            continue
        argv.append(x)
    cmd = ' '.join(['python tools/verify_bench.py'] + argv)
    rec['command'] = cmd
    text = json.dumps(rec, indent=1, default=str)
    print(text)
    for path, body in ((a.out, text + '\n'), (a.md, _md(rec, cmd) + '\n')):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                f.write(body)


if __name__ == '__main__':
    main()
