"""Pair verification on the GPU: cpg_pair_distance / cpg_pair_sweep against the explicit-order restatement (tests/_verify.py) and the
reference's fixture (tests/golden/verify_roc.npz), then Manager.evalLFW, CPGSession's face task and a two-rank run end to end."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

import _verify as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
THR = np.arange(0, 4, 0.01)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _device_distance(e1, e2, metric, lda=None):
    """cpg_pair_distance straight through the ABI (with the cosine output); lda > d runs on a column slice of a wider matrix."""
    from cpg_amd import _lib
    n, d = e1.shape
    lda = lda or d
    wide = [torch.zeros((n, lda), dtype=torch.float32, device=DEV) for _ in range(2)]
    wide[0][:, :d] = torch.from_numpy(e1)
    wide[1][:, :d] = torch.from_numpy(e2)
    dist = torch.full((n,), -7.0, device=DEV)
    sim = torch.full((n,), -7.0, device=DEV)
    rc = _lib.lib().cpg_pair_distance(ctypes.c_void_p(wide[0].data_ptr()), lda, ctypes.c_void_p(wide[1].data_ptr()), lda, n, d, metric,
                                      _lib.dptr(dist), _lib.dptr(sim), _lib.stream_ptr())
    _lib.check('cpg_pair_distance', rc)
    return dist, sim.cpu().numpy()


def _embeddings(rng, n, d, zero_rows=()):
    e1 = V.adversarial_rows(rng, n, d) if d >= 4 else rng.standard_normal((n, d)).astype(np.float32)
    # scaled so that metric-0 distances spread over the thresholds, with a few order-sensitive rows kept
    e1 = e1 / np.maximum(1.0, np.abs(e1).max(1, keepdims=True)).astype(np.float32) * np.float32(1.0 / np.sqrt(d))
    sigma = rng.uniform(0.05, 1.6, n).astype(np.float32)
    e2 = (e1 + rng.standard_normal((n, d)).astype(np.float32) * (sigma / np.float32(np.sqrt(d)))[:, None]).astype(np.float32)
    for i in zero_rows:
        e1[i] = 0
    return e1, e2, sigma < 0.8


def _check_sweep(dist_dev, same, thr=THR, nfolds=10):
    from cpg_amd.utils import metrics
    counts, best = metrics.roc_counts(thr, dist_dev, same, nfolds)
    want_c, want_b = V.sweep(dist_dev.cpu().numpy(), same, thr, nfolds)
    assert np.array_equal(counts, want_c) and np.array_equal(best, want_b)
    got = metrics.roc_from_counts(counts, best)
    for g, w in zip(got, V.roc(want_c, want_b)):
        assert g.dtype == np.float64 and np.array_equal(g, w)
    return counts


@pytest.mark.parametrize('n', [10, 13, 5999, 6000])
@pytest.mark.parametrize('d', [1, 7, 128, 129, 512, 1000])
def test_distances_and_sweep_match_the_restatement(n, d):
    rng = np.random.default_rng(n * 7919 + d)
    zero = [3, n - 1]
    e1, e2, same = _embeddings(rng, n, d, zero)
    # metric 0: bit for bit
    dist, _ = _device_distance(e1, e2, 0, lda=d + 3 if d % 2 else None)
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(V.distance(e1, e2, 0)))
    _check_sweep(dist, same)
    # metric 1: the cosine bit for bit, the arccos within 2 ulp of float32(acos_fp64(cosine)) * 4 / pi; zero rows give NaN
    dist1, sim = _device_distance(e1, e2, 1)
    want_sim = V.cosine(e1, e2)
    assert np.array_equal(np.isnan(sim), np.isnan(want_sim)) and np.isnan(sim[zero]).all()
    ok = ~np.isnan(want_sim)
    assert np.array_equal(_bits(sim[ok]), _bits(want_sim[ok]))
    got1, want1 = dist1.cpu().numpy(), V.distance(e1, e2, 1)
    assert np.isnan(got1[zero]).all() and np.array_equal(np.isnan(got1), np.isnan(want1))
    assert np.abs(got1[ok].view(np.int32).astype(np.int64) - want1[ok].view(np.int32)).max() <= 2
    counts = _check_sweep(dist1, same)
    assert (counts[..., 0] + counts[..., 1]).max() <= n                 # NaN pairs are never predicted "same"


@pytest.mark.parametrize('labels', ['all_same', 'all_different'])
def test_sweep_with_one_label_only(labels):
    rng = np.random.default_rng(5)
    e1, e2, _ = _embeddings(rng, 123, 64, zero_rows=[0])
    same = np.full(123, labels == 'all_same')
    for metric in (0, 1):
        dist, _ = _device_distance(e1, e2, metric)
        counts = _check_sweep(dist, same)
        assert (counts[..., 0 if labels == 'all_different' else 1] == 0).all()


def test_device_scoring_matches_the_reference_fixture(golden):
    from cpg_amd.utils import metrics
    fx = golden('verify_roc')
    for tag in ('a', 'b', 'c'):
        e1 = torch.from_numpy(fx[tag + '_e1'].astype(np.float32)).to(DEV)
        e2 = torch.from_numpy(fx[tag + '_e2'].astype(np.float32)).to(DEV)
        same = fx[tag + '_issame']
        for metric in ((0, 1) if tag != 'c' else (0,)):
            want = fx['%s_dist%d' % (tag, metric)]
            got = metrics.distance(e1, e2, metric)
            assert got.is_cuda and got.dtype == torch.float32
            got = got.cpu().numpy()
            if metric == 0:
                assert np.array_equal(_bits(got), _bits(want)), tag
            else:
                ok = ~np.isnan(want)
                assert np.array_equal(np.isnan(got), ~ok)
                assert np.abs(got[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32)).max() <= 2, tag
            for tt, dtype in (('64', 'float64'), ('32', 'float32')):
                res = metrics.calculate_roc(THR, e1, e2, same, nrof_folds=10, distance_metric=metric, threshold_dtype=dtype)
                for name, val in zip(('tpr', 'fpr', 'acc'), res):
                    assert np.array_equal(val, fx['%s_m%d_t%s_%s' % (tag, metric, tt, name)]), (tag, metric, tt, name)
        if tag != 'c':
            out = metrics.fv_evaluate(e1, e2, same, distance_metric=True)
            assert len(out) == 6 and np.array_equal(out[2], fx['%s_m1_t64_acc' % tag]) and all(np.isnan(v) for v in out[3:])


# ---------------------------------------------------------------------------------------------------------------- end to end
WIDTH = 0.25


def _store_and_pairs(seed=11, n_img=24, n_pairs=43):
    from cpg_amd import data as D
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 6, n_img)
    imgs = []
    for c in ids:                                                   # identity-dependent blocks, so that "same" pairs look alike
        im = rng.integers(0, 90, (112, 112, 3), dtype=np.uint8)
        im[(c * 13) % 60:(c * 13) % 60 + 40, (c * 17) % 60:(c * 17) % 60 + 40, c % 3] = 240
        imgs.append(im)
    store = D.ImageStore.from_arrays(imgs, ids, DEV)
    pairs = []
    for _ in range(n_pairs):
        a, p = rng.choice(n_img, 2, replace=False)
        pairs.append((int(a), int(p), bool(ids[a] == ids[p])))
    return store, pairs


def _spherenet(seed=1):
    import cpg_amd.models as M
    torch.manual_seed(seed)
    net = M.spherenet20(dataset_history=[], dataset2num_classes={}, network_width_multiplier=WIDTH, shared_layer_info={})
    net.add_dataset('face_verification', 6)
    net.set_dataset('face_verification')
    return net.to(DEV)


def _masks(model, rng=None):
    from cpg_amd.models import layers as nl
    out = {}
    for n, m in model.named_modules():
        if isinstance(m, (nl.SharableConv2d, nl.SharableLinear)):
            mk = torch.ones(m.weight.shape, dtype=torch.uint8, device=DEV)
            if rng is not None:                                     # some released slots: apply_mask zeroes them
                mk[torch.from_numpy(rng.random(tuple(m.weight.shape)) < 0.1).to(DEV)] = 0
            out[n] = mk
    return out


def _manager(model, masks, val_loader, train_loader=None, mode='finetune'):
    from cpg_amd.driver import default_args
    from cpg_amd.utils.manager import Manager
    args = default_args(mode=mode, dataset='face_verification', network_width_multiplier=WIDTH)
    return Manager(args, model, {}, masks, train_loader, val_loader, 0, 1)


def _restated_accuracy(embs):
    a = np.concatenate([b[0].cpu().numpy() for b in embs])
    p = np.concatenate([b[1].cpu().numpy() for b in embs])
    same = np.concatenate([np.asarray(b[2]).reshape(-1) for b in embs])
    counts, best = V.sweep(V.distance(a, p, 1), same, THR, 10)
    return V.roc(counts, best)[2]


class _Wrap(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.module = m

    def forward(self, x):
        return self.module(x)


def test_evalLFW_matches_the_restatement_and_applies_the_mask():
    from cpg_amd import data as D
    from cpg_amd.models import layers as nl
    store, pairs = _store_and_pairs()
    loader = D.PairLoader(store, pairs, 16)
    model = _Wrap(_spherenet())
    masks = _masks(model, np.random.default_rng(3))
    before = {n: m.weight.detach().clone() for n, m in model.named_modules() if isinstance(m, (nl.SharableConv2d, nl.SharableLinear))}
    mgr = _manager(model, masks, loader)
    acc = mgr.evalLFW(0)
    assert isinstance(acc, np.floating) and 0.0 <= acc <= 1.0
    assert mgr.last_stats['accuracy'] == float(acc) and mgr.last_stats['accuracy_std'] == float(np.std(mgr.last_lfw['accuracy']))
    # the weights are what validate leaves: apply_mask zeroed every released slot, nothing else moved
    for n, m in model.named_modules():
        if n in before:
            assert torch.equal(m.weight.detach(), before[n] * (masks[n] != 0).to(before[n].dtype)), n
    embs = mgr.eval_embeddings(0)                                   # the same forward again (the mask is applied already)
    want = _restated_accuracy(embs)
    assert np.array_equal(mgr.last_lfw['accuracy'], want) and acc == np.mean(want)
    # a bare model (no .module) works the same way
    bare = _manager(model.module, {k[len('module.'):]: v for k, v in masks.items()}, loader)
    assert bare.evalLFW(0) == acc


def test_face_main_call_sequence():
    """CPG_face_main.py's order of calls for the face task: the finetuning mask and evalLFW(0) (:401-404), the epoch loop's
    train + evalLFW(epoch_idx) (:412-417) and the prune run's evalLFW(start_epoch - 1) (:357-361) with start_epoch 0."""
    from cpg_amd import data as D
    from cpg_amd.utils import Optimizers
    from cpg_amd.utils.fused_sgd import MaskedSGD
    store, pairs = _store_and_pairs(seed=12)
    val = D.PairLoader(store, pairs, 16)
    train = D.DeviceLoader(store, 8, 'face_train', seed=1)
    model = _Wrap(_spherenet(seed=2))
    masks = _masks(model)
    for m in masks.values():
        m.zero_()
    manager = _manager(model, masks, val, train)
    manager.pruner.make_finetuning_mask()
    first = manager.evalLFW(0)
    opts = Optimizers()
    opts.add(MaskedSGD(list(model.parameters()), pruner=manager.pruner, lr=1e-3, momentum=0.9, nesterov=True), 1e-3)
    start_epoch = 0
    for epoch_idx in range(start_epoch, 1):
        manager.train(opts, epoch_idx, [1e-3], 0)
        avg_val_acc = manager.evalLFW(epoch_idx)
    again = manager.evalLFW(start_epoch - 1)
    assert again == avg_val_acc
    assert all(0.0 <= v <= 1.0 for v in (first, avg_val_acc))
    assert avg_val_acc == np.mean(_restated_accuracy(manager.eval_embeddings(0)))


def test_run_task_scores_a_pair_loader_like_evalLFW():
    from cpg_amd import data as D
    from cpg_amd.driver import CPGSession, default_args
    store, pairs = _store_and_pairs(seed=13)
    val = D.PairLoader(store, pairs, 16)
    sess = CPGSession('spherenet20', WIDTH, device=DEV, seed=1)
    args = default_args(network_width_multiplier=WIDTH)
    res = sess.run_task('face_verification', 6, [], val, pretrained_pass_through=True, sparsities=(), args=args)
    mgr = _manager(sess.model, sess.masks, val)
    want = mgr.evalLFW(0)
    assert res.finetune_acc == float(want) and 0.0 < want <= 1.0
    acc, embs = sess.evaluate('face_verification', val)
    assert acc == float(want) and len(embs) == len(val) and all(len(b) == 3 for b in embs)
    # a set embedding_scorer still wins; a loader of single images still reports 0.0
    sess.embedding_scorer = lambda e: 0.25
    assert sess.evaluate('face_verification', val)[0] == 0.25
    del sess.embedding_scorer
    x = torch.zeros(4, 3, 112, 112, device=DEV)
    assert sess.evaluate('face_verification', [(x, torch.zeros(4, dtype=torch.int64, device=DEV))])[0] == 0.0


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from cpg_amd import data as D
        from cpg_amd import dist as cdist
        store, pairs = _store_and_pairs(seed=14)
        model = cdist.DataParallel(_spherenet(seed=3))
        mgr = _manager(model, _masks(model), D.PairLoader(store, pairs, 16))
        acc = mgr.evalLFW(0)
        torch.cuda.synchronize()
        torch.save({'acc': float(acc), 'folds': mgr.last_lfw['accuracy']}, os.path.join(out_dir, 'lfw_rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_return_the_same_accuracy(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(os.path.join(tmp_path, 'lfw_rank0.pt'), weights_only=False)
    r1 = torch.load(os.path.join(tmp_path, 'lfw_rank1.pt'), weights_only=False)
    assert r0['acc'] == r1['acc'] and np.array_equal(r0['folds'], r1['folds']) and 0.0 <= r0['acc'] <= 1.0
