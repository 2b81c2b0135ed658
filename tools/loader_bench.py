#!/usr/bin/env python3
"""Cost of the GPU data path (cpg_amd/data.py) on one MI355X, and the host pipeline it replaces.

  loader  images/s of every DeviceLoader preset alone (device-synchronised wall clock over whole epochs), at the reference's train
          batch (32) and the bench's (256).  Kernel time: run the same part again under
          `rocprofv3 --kernel-trace --stats -- python tools/loader_bench.py --part loader --quick` and read k_image_* there.
  ab      train-step ms of VGG16-224 (fine_grained_train preset) and SphereNet-20 (face_train preset) at batch 256 through
          Manager.train, fed from DeviceLoader (A) versus a list of resident batches (B), interleaved in blocks.
  pil     images/s of the same transforms done the reference's way: per sample PIL resize / crop, then ToTensor + Normalize (+ Cutout)
          in numpy, in a pool of --procs processes (decoded images in memory: the JPEG decode the reference also pays is left out).

Synthetic images (uniform random bytes at CUBS-like sizes for the fine-grained presets, 112 x 112 faces, 32 x 32 CIFAR): the cost
of every step is set by sizes, not by pixel values.  Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESET_SRC = {                        # (source images: n, min side, max side)
    'cifar100_train': (4096, 32, 32), 'cifar100_val': (4096, 32, 32),
    'face_train': (2048, 112, 112), 'face_val': (2048, 112, 112),
    'fine_grained_train': (768, 300, 500), 'fine_grained_val': (768, 300, 500),
    'fine_grained_train_cropped': (768, 300, 500), 'fine_grained_val_cropped': (768, 300, 500),
}
CIFAR_STATS = ((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))      # any three values: the arithmetic does not depend on them
HBM_COPY_TBS = 6.29                                       # MI355X HBM3E: measured float4 copy rate, TB/s


def _images(rng, n, lo, hi):
    return [rng.integers(0, 256, (int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1)), 3), dtype=np.uint8) for _ in range(n)]


def _sync():
    import torch
    torch.cuda.synchronize()


def part_loader(quick):
    import torch
    from cpg_amd import data as D
    rng = np.random.default_rng(0)
    out = {}
    for preset, (n, lo, hi) in PRESET_SRC.items():
        if quick:
            n = min(n, 512)
        imgs = _images(rng, n, lo, hi)
        store = D.ImageStore.from_arrays(imgs, rng.integers(0, 10, n), 'cuda').prepared(preset)
        kw = dict(mean=CIFAR_STATS[0], std=CIFAR_STATS[1]) if preset.startswith('cifar100') else {}
        res = {'images': n, 'store_bytes': store.nbytes}
        for B in (32, 256):
            loader = D.DeviceLoader(store, B, preset, seed=1, drop_last=True, **kw)
            for _ in loader:                                  # warm-up epoch
                pass
            _sync()
            epochs = 1 if quick else 3
            t0 = time.perf_counter()
            for _ in range(epochs):
                for x, y in loader:
                    pass
            _sync()
            dt = time.perf_counter() - t0
            imgs_done = epochs * len(loader) * B
            shape = tuple(x.shape[1:])
            # bytes the kernels must move per image: the fp32 output, the uint8 window it reads (+ the RandomSizedCrop staging image
            # written and read again), the crop itself (upper bound: the whole source image)
            per = 4 * 3 * shape[1] * shape[2] + 3 * shape[1] * shape[2]
            if D.PRESETS[preset].crop == 'rsc':
                per += 2 * 3 * shape[1] * shape[2] + int(np.mean(store.heights * store.widths) * 3)
            res['batch%d' % B] = {'images_per_s': imgs_done / dt, 'ms_per_batch': 1e3 * dt / (imgs_done / B), 'out_shape': shape,
                                  'bytes_per_image': per}
        out[preset] = res
        del store
        torch.cuda.empty_cache()
    return out


def _model(arch, dev):
    import cpg_amd.models as M
    import torch
    torch.manual_seed(1)
    kw = dict(dataset_history=[], dataset2num_classes={}, network_width_multiplier=1.0, shared_layer_info={})
    if arch == 'vgg16':
        net = M.custom_vgg([64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M'], **kw)
        ds, ncls = 'cubs', 200
    else:
        net = M.spherenet20(**kw)
        ds, ncls = 'face_verification', 4630
    net.add_dataset(ds, ncls)
    net.set_dataset(ds)

    class Wrap(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.module = m

        def forward(self, x):
            return self.module(x)

    return Wrap(net.to(dev)), ds, ncls


def part_ab(blocks, steps):
    import torch
    from cpg_amd import data as D
    from cpg_amd.models import layers as nl
    from cpg_amd.utils import Optimizers
    from cpg_amd.utils.fused_sgd import MaskedSGD
    from cpg_amd.utils.manager import Manager
    rng = np.random.default_rng(0)
    out = {}
    B = 256
    for arch, preset in (('vgg16', 'fine_grained_train'), ('spherenet20', 'face_train')):
        model, ds, ncls = _model(arch, 'cuda')
        n, lo, hi = PRESET_SRC[preset]
        n = B * steps
        store = D.ImageStore.from_arrays(_images(rng, n, lo, hi), rng.integers(0, ncls, n), 'cuda').prepared(preset)
        loader = D.DeviceLoader(store, B, preset, seed=1, drop_last=True)
        resident = [(x.clone(), y.clone()) for x, y in loader]
        masks = {nm: torch.ones(m.weight.shape, dtype=torch.uint8, device='cuda') for nm, m in model.named_modules()
                 if isinstance(m, (nl.SharableConv2d, nl.SharableLinear))}
        args = types.SimpleNamespace(mode='finetune', dataset=ds, finetune_again=False, target_sparsity=0.1, initial_sparsity=0.0,
                                     pruning_frequency=10, weight_decay=4e-5, network_width_multiplier=1.0, cuda=True, log_path=None,
                                     progress=False)
        mgr = Manager(args, model, {}, masks, loader, None, 0, 0)
        lr = 1e-3
        opts = Optimizers()
        opts.add(MaskedSGD(list(model.parameters()), pruner=mgr.pruner, lr=lr, momentum=0.9, nesterov=True), lr)
        times = {'device_loader': [], 'resident': []}
        for rep in range(blocks + 1):
            for name, src in (('device_loader', loader), ('resident', resident)) if rep % 2 == 0 else \
                    (('resident', resident), ('device_loader', loader)):
                mgr.train_loader = src
                _sync()
                t0 = time.perf_counter()
                mgr.train(opts, rep, [lr], 0)
                _sync()
                if rep:                                        # block 0 warms both up
                    times[name].append(1e3 * (time.perf_counter() - t0) / steps)
        out[arch] = {'preset': preset, 'batch': B, 'steps_per_block': steps, 'blocks': blocks,
                     'ms_per_step': {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v)), 'all': v}
                                     for k, v in times.items()}}
        med = out[arch]['ms_per_step']
        out[arch]['delta_ms'] = med['device_loader']['median'] - med['resident']['median']
        del mgr, opts, model, store, loader, resident
        torch.cuda.empty_cache()
    return out


# ---------------------------------------------------------------------------------------------------------- the host pipeline
_POOL_IMGS = None


def _pil_init(imgs):
    global _POOL_IMGS
    _POOL_IMGS = imgs


def _pil_work(args):
    """One sample the reference's way (utils/fine_grained_dataset.py:36-70, utils/face_dataset.py:10-25, utils/cifar100_dataset.py:7-25)."""
    from PIL import Image
    kind, i, seed = args
    r = np.random.default_rng(seed)
    img = Image.fromarray(_POOL_IMGS[i])
    if kind == 'fine_grained_train':
        w, h = img.size
        img = img.resize((256, int(256 * h / w)) if w < h else (int(256 * w / h), 256), Image.BILINEAR)     # Scale(256)
        w, h = img.size
        a = r.uniform(0.08, 1.0) * w * h                                                                     # RandomSizedCrop(224)
        ar = r.uniform(3 / 4, 4 / 3)
        cw, ch = min(w, int(round(np.sqrt(a * ar)))), min(h, int(round(np.sqrt(a / ar))))
        x0, y0 = int(r.integers(0, w - cw + 1)), int(r.integers(0, h - ch + 1))
        img = img.crop((x0, y0, x0 + cw, y0 + ch)).resize((224, 224), Image.BILINEAR)
    if r.random() < 0.5:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    u = np.asarray(img)
    if kind == 'cifar100_train':
        u = np.pad(u, ((4, 4), (4, 4), (0, 0)))
        y0, x0 = r.integers(0, 9, 2)
        u = u[y0:y0 + 32, x0:x0 + 32]
    v = u.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    v = (v - np.float32(0.45)) / np.float32(0.25)
    if kind == 'fine_grained_train':
        cy, cx = r.integers(0, 224, 2)
        v[:, max(0, cy - 8):cy + 8, max(0, cx - 8):cx + 8] *= np.float32(0)
    return v.shape


def part_pil(procs, quick):
    import multiprocessing as mp
    try:
        import PIL  # noqa: F401
    except ImportError:
        return {'error': 'PIL is not installed: not measured'}
    rng = np.random.default_rng(0)
    out = {'processes': procs}
    for kind, (n, lo, hi) in (('fine_grained_train', (256, 300, 500)), ('face_train', (256, 112, 112)), ('cifar100_train', (1024, 32, 32))):
        imgs = _images(rng, n, lo, hi)
        total = (2 if quick else 8) * n
        work = [(kind, i % n, i) for i in range(total)]
        with mp.get_context('fork').Pool(procs, initializer=_pil_init, initargs=(imgs,)) as pool:
            pool.map(_pil_work, work[:procs * 4], chunksize=4)          # warm-up
            t0 = time.perf_counter()
            pool.map(_pil_work, work, chunksize=16)
            dt = time.perf_counter() - t0
        out[kind] = {'images_per_s': total / dt, 'images': total}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'loader', 'ab', 'pil'])
    ap.add_argument('--quick', action='store_true', help='fewer images and epochs (the rocprofv3 run)')
    ap.add_argument('--blocks', type=int, default=4, help='A/B: interleaved blocks per side after one warm-up block')
    ap.add_argument('--steps', type=int, default=8, help='A/B: train steps per block')
    ap.add_argument('--procs', type=int, default=16, help='pil: worker processes (a GPU job gets 16 CPUs)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    # the options that shape the measurement; where the record is written (--out) is not part of it
    rec = {'tool': 'tools/loader_bench.py', 'options': {k: getattr(a, k) for k in ('part', 'quick', 'blocks', 'steps', 'procs')}}
    if a.part in ('all', 'pil'):                  # first: the pool forks before this process touches the GPU
        rec['pil_16cpu'] = part_pil(a.procs, a.quick)
    if a.part in ('all', 'loader', 'ab'):
        import torch
        assert torch.cuda.is_available(), 'loader_bench needs a GPU (no CPU fallback)'
        rec['device'] = torch.cuda.get_device_name(0)
    if a.part in ('all', 'loader'):
        rec['loader'] = part_loader(a.quick)
    if a.part in ('all', 'ab'):
        rec['ab_train_step'] = part_ab(a.blocks, a.steps)
    rec['hbm_copy_tb_s'] = HBM_COPY_TBS
    text = json.dumps(rec, indent=1, default=str)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
