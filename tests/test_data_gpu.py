"""The data path on the GPU (cpg_amd/data.py, include/cpg_hip.h "image batches"): both kernels against the numpy restatement of
PIL / torchvision in tests/_imaging.py (itself checked against PIL in test_data_host.py), bit for bit; every preset's loader; and the
loader as a drop-in for a list of batches in Manager.train and CPGSession.run_task.  Small sizes; no PIL needed here."""
import types
import zlib

import numpy as np
import pytest
import torch

import _imaging as I
from cpg_amd import data as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CIFAR_MEAN, CIFAR_STD = (0.5071, 0.4865, 0.4409), (0.2673, 0.2564, 0.2762)     # a caller's statistics (any three values will do)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _images(rng, n, lo, hi):
    return [rng.integers(0, 256, (int(rng.integers(lo, hi)), int(rng.integers(lo, hi)), 3), dtype=np.uint8) for _ in range(n)]


def test_resample_kernel_matches_reference_on_a_ragged_batch():
    rng = np.random.default_rng(11)
    n = 220
    imgs = []
    for i in range(n):
        if i % 4 == 0:
            H, W = int(rng.integers(300, 601)), int(rng.integers(300, 601))
        else:
            H, W = int(rng.integers(1, 120)), int(rng.integers(1, 120))
        imgs.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    store = D.ImageStore.from_arrays(imgs, np.zeros(n, np.int64), DEV)
    rows, refs, off = [], [], 0
    for i, img in enumerate(imgs):
        H, W = img.shape[:2]
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        kind = i % 5
        if kind == 0:
            oh, ow = int(rng.integers(1, 12)), int(rng.integers(1, 12))           # > 8x reductions of the big sources
        elif kind == 1:
            oh, ow = int(rng.integers(150, 301)), int(rng.integers(150, 301))     # enlargements
        elif kind == 2:
            oh, ow = h, w                                                       # identity: a copy
        elif kind == 3:
            oh, ow = (h, int(rng.integers(1, 301))) if i % 2 else (int(rng.integers(1, 301)), w)    # one pass only
        else:
            oh, ow = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        rows.append((int(store.offsets[i]), H, W, y, x, h, w, off, oh, ow))
        refs.append(I.resample(img, (y, x, h, w), oh, ow))
        off += oh * ow * 3
    dst = torch.full((off + 64,), 7, dtype=torch.uint8, device=DEV)
    D.resample(store.data, store.nbytes, rows, dst, off)
    got = dst.cpu().numpy()
    bad = [i for i, r in enumerate(rows) if not np.array_equal(got[r[7]:r[7] + r[8] * r[9] * 3], refs[i].reshape(-1))]
    assert not bad, ('items that differ', bad[:10], [rows[i] for i in bad[:3]])
    assert (got[off:] == 7).all()                                               # nothing past the last item is written


def test_to_tensor_kernel_matches_torch_cpu_bits():
    rng = np.random.default_rng(5)
    imgs = _images(rng, 12, 1, 60) + [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)]
    store = D.ImageStore.from_arrays(imgs, np.arange(len(imgs)), DEV)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for out_h, out_w in ((37, 53), (32, 32), (5, 3)):
        rows = []
        for i, img in enumerate(imgs):
            H, W = img.shape[:2]
            case = i % 6
            y0, x0 = int(rng.integers(-6, H)), int(rng.integers(-6, W))
            if case == 0:
                y0, x0 = -out_h - 3, 2                                     # wholly outside: (0 - mean) / std everywhere
            if case == 1:
                y0, x0 = 0, 0
            cut = [(0, 0, 0, 0), (0, min(8, out_h), 0, min(8, out_w)), (max(0, out_h - 5), out_h, max(0, out_w - 3), out_w),
                   (out_h // 3, out_h // 2 + 1, 1, out_w), (0, out_h, 0, out_w), (2, 2, 0, out_w)][case]
            rows.append((int(store.offsets[i]), H, W, y0, x0, i % 2) + cut)
        out = torch.full((len(rows) + 1, 3, out_h, out_w), 5.0, device=DEV)
        D.to_tensor(store.data, store.nbytes, rows, out_h, out_w, mean, std, out[:len(rows)])
        got = out.cpu()
        assert (got[-1] == 5.0).all()
        for i, r in enumerate(rows):
            img = imgs[i]
            # torch-CPU arithmetic: u.float() / 255, (v - mean) / std, then the Cutout mask multiply
            u = torch.from_numpy(I.window(img, r[3], r[4], out_h, out_w, r[5])).permute(2, 0, 1)
            v = (u.float() / 255 - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
            mask = torch.ones(out_h, out_w)
            mask[r[6]:r[7], r[8]:r[9]] = 0.
            v *= mask.expand_as(v)
            assert np.array_equal(_bits(got[i].numpy()), _bits(v.numpy())), (out_h, out_w, r)
            assert np.array_equal(_bits(got[i].numpy()), _bits(I.to_tensor(img, r[3], r[4], out_h, out_w, r[5], r[6:10], mean, std)))
    # a Cutout over the whole output: zeros, -0.0 where the normalised value was negative (the bit comparison above pins which)
    z = got[4].numpy()
    assert (z == 0).all() and np.signbit(z).any()


def _store_for(preset, rng, n):
    if preset.startswith('cifar100'):
        imgs = [rng.integers(0, 256, (32, 32, 3), dtype=np.uint8) for _ in range(n)]
    elif preset.startswith('face'):
        imgs = [rng.integers(0, 256, (int(s), int(s), 3), dtype=np.uint8) for s in rng.choice([96, 112, 150], n)]
    else:
        imgs = _images(rng, n, 180, 330)
    labels = rng.integers(0, 7, n)
    return imgs, labels


@pytest.mark.parametrize('preset', sorted(D.PRESETS))
def test_every_preset_epoch_matches_reference(preset):
    rng = np.random.default_rng(zlib.crc32(preset.encode()))
    n, B = 10, 4
    imgs, labels = _store_for(preset, rng, n)
    kw = dict(mean=CIFAR_MEAN, std=CIFAR_STD) if preset.startswith('cifar100') else {}
    store = D.ImageStore.from_arrays(imgs, labels, DEV).prepared(preset)
    rule = D.PRESETS[preset].resize
    ref_imgs = [I.resize_rule(im, rule) for im in imgs] if rule is not None else imgs
    for i, im in enumerate(ref_imgs):                                 # the store's one-time resize, bit for bit
        o = int(store.offsets[i])
        assert np.array_equal(store.data[o:o + im.size].cpu().numpy(), im.reshape(-1)), i
    loader = D.DeviceLoader(store, B, preset, seed=3, **kw)
    assert len(loader) == 3
    mean, std = loader.mean, loader.std
    for epoch in range(2):
        plan = loader.plan(epoch)
        batches = list(loader)
        assert len(batches) == 3 and loader.epoch == epoch + 1
        for b, (x, y) in enumerate(batches):
            pos = np.arange(b * B, min(n, (b + 1) * B))
            rx, ry = I.batch(ref_imgs, labels, plan, pos, mean, std)
            assert x.is_cuda and x.dtype == torch.float32 and y.dtype == torch.int64 and x.is_contiguous()
            assert np.array_equal(_bits(x.cpu().numpy()), _bits(rx)), (epoch, b)
            assert np.array_equal(y.cpu().numpy(), ry)
    # rank shards of the same epoch, concatenated, are the full batches (cpg_amd.dist.shard_batch)
    full = D.DeviceLoader(store, 4, preset, seed=9, drop_last=True, **kw)
    shards = [D.DeviceLoader(store, 4, preset, seed=9, drop_last=True, rank=r, world=2, **kw) for r in range(2)]
    for (x, y), (x0, y0), (x1, y1) in zip(full, *shards):
        assert x0.shape[0] == 2 and torch.equal(torch.cat([x0, x1]), x) and torch.equal(torch.cat([y0, y1]), y)
    with pytest.raises(ValueError, match='not divisible'):
        D.DeviceLoader(store, 4, preset, world=3, **kw)
    with pytest.raises(ValueError, match='not divisible'):
        D.DeviceLoader(store, 4, preset, world=4, **kw)            # the last global batch has 2 rows


def test_pair_loader_yields_face_val_pairs():
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (112, 112, 3), dtype=np.uint8) for _ in range(5)]
    store = D.ImageStore.from_arrays(imgs, np.arange(5), DEV)
    pairs = [(0, 1, True), (2, 3, False), (4, 0, False)]
    out = list(D.PairLoader(store, pairs, 2))
    assert len(out) == 2 and [len(b[0]) for b in out] == [2, 1]
    a, p, same = out[0]
    assert same.dtype == torch.bool and same.tolist() == [True, False]
    ref = I.to_tensor(imgs[3], 0, 0, 112, 112, 0, (0, 0, 0, 0), D.FACE_MEAN, D.FACE_STD)
    assert np.array_equal(_bits(p[1].cpu().numpy()), _bits(ref))


def _vgg(seed=1):
    import torch.nn as nn
    import cpg_amd.models as M
    torch.manual_seed(seed)
    cfg = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']
    net = M.custom_vgg_cifar100(cfg, dataset_history=[], dataset2num_classes={}, network_width_multiplier=0.125, shared_layer_info={})
    net.add_dataset('t1', 5)
    net.set_dataset('t1')

    class Wrap(nn.Module):
        def __init__(self, m):
            super().__init__()
            self.module = m

        def forward(self, x):
            return self.module(x)

    return Wrap(net.to(DEV))


def _train(loader):
    from cpg_amd.models import layers as nl
    from cpg_amd.utils import Optimizers
    from cpg_amd.utils.fused_sgd import MaskedSGD
    from cpg_amd.utils.manager import Manager
    model = _vgg()
    masks = {n: torch.ones(m.weight.shape, dtype=torch.uint8, device=DEV) for n, m in model.named_modules()
             if isinstance(m, (nl.SharableConv2d, nl.SharableLinear))}
    args = types.SimpleNamespace(mode='prune', dataset='t1', finetune_again=False, target_sparsity=0.3, initial_sparsity=0.0,
                                 pruning_frequency=1, weight_decay=4e-5, network_width_multiplier=0.125, cuda=True, log_path=None,
                                 progress=False)
    mgr = Manager(args, model, {}, masks, loader, None, 0, 3)
    opts = Optimizers()
    opts.add(MaskedSGD(list(model.parameters()), pruner=mgr.pruner, lr=1e-2, momentum=0.9, nesterov=True), 1e-2)
    mgr.train(opts, 0, [1e-2], 0)
    model.eval()
    with torch.no_grad():
        probe = torch.linspace(-2, 2, 4 * 3 * 32 * 32, device=DEV).view(4, 3, 32, 32)
        logits = model(probe)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, {k: v.clone() for k, v in masks.items()}, logits


def test_device_loader_is_a_drop_in_for_manager_train():
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (32, 32, 3), dtype=np.uint8) for _ in range(24)]
    labels = rng.integers(0, 5, 24)
    store = D.ImageStore.from_arrays(imgs, labels, DEV)
    loader = D.DeviceLoader(store, 8, 'cifar100_train', seed=5, mean=CIFAR_MEAN, std=CIFAR_STD)
    plan = loader.plan(0)
    host = []
    for b in range(3):
        x, y = I.batch(imgs, labels, plan, np.arange(8 * b, 8 * b + 8), CIFAR_MEAN, CIFAR_STD)
        host.append((torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)))
    sd_a, m_a, l_a = _train(loader)
    sd_b, m_b, l_b = _train(host)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    for k in m_a:
        assert torch.equal(m_a[k], m_b[k]), k
    assert torch.equal(l_a, l_b) and torch.isfinite(l_a).all()
    assert any(int((v == 0).sum()) for v in m_a.values())              # the prune events ran


def test_run_task_over_a_tiny_store():
    from cpg_amd.driver import CPGSession, default_args
    rng = np.random.default_rng(8)
    labels = rng.integers(0, 5, 32)
    imgs = []
    for c in labels:                                            # a class-dependent bright block
        im = rng.integers(0, 120, (32, 32, 3), dtype=np.uint8)
        im[(c * 5) % 16:(c * 5) % 16 + 12, (c * 6) % 20:(c * 6) % 20 + 12, c % 3] = 250
        imgs.append(im)
    store = D.ImageStore.from_arrays(imgs, labels, DEV)
    train = D.DeviceLoader(store, 8, 'cifar100_train', mean=CIFAR_MEAN, std=CIFAR_STD)
    val = D.DeviceLoader(store, 16, 'cifar100_val', mean=CIFAR_MEAN, std=CIFAR_STD)
    sess = CPGSession('custom_vgg_cifar100', 0.125, device=DEV, seed=1)
    args = default_args(lr=5e-2, lr_mask=5e-4, pruning_frequency=1, pruning_interval=1, prune_lr=1e-2)
    res = sess.run_task('t1', 5, train, val, accuracy_goal=0.0, finetune_epochs=1, prune_epochs=1, sparsities=(0.2,), args=args,
                        min_train_acc=-1.0)
    assert set(res.ratio_to_acc) == {0.0, 0.2}
    assert all(np.isfinite(v) for v in res.ratio_to_acc.values()) and np.isfinite(res.finetune_train_acc)
    assert train.epoch >= 2                                     # every pass over the loader was a new epoch


def test_cpu_tensors_have_no_fallback():
    store = D.ImageStore.from_arrays([np.zeros((4, 4, 3), np.uint8)], [0], DEV)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        D.to_tensor(store.data.cpu(), 48, [(0, 4, 4, 0, 0, 0, 0, 0, 0, 0)], 4, 4, (0, 0, 0), (1, 1, 1), torch.empty(1, 3, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        D.to_tensor(store.data, 48, [(0, 4, 4, 0, 0, 0, 0, 0, 0, 0)], 4, 4, (0, 0, 0), (1, 1, 1), torch.empty(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        D.ImageStore(store.data.cpu(), store.labels, [0], [4], [4])
