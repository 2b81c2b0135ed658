"""Real images for the training loop: a uint8 image store resident in device memory, and loaders that build every batch on the GPU.

The reference feeds its networks through torchvision `ImageFolder` + `DataLoader` workers that decode, crop, resize and normalise
every sample in PIL on the host (utils/cifar100_dataset.py, utils/face_dataset.py, utils/fine_grained_dataset.py,
utils/LFWDataset.py).  Here a dataset is decoded ONCE into an `ImageStore` -- RGB, HWC, uint8, one flat device buffer -- and each
batch is produced by two HIP kernels (include/cpg_hip.h, "image batches"):

  * cpg_image_resample: crop, then PIL's 8-bit BILINEAR resize, bit for bit (the store's one-time Resize / Scale, and
    RandomSizedCrop's per-sample crop-and-resize);
  * cpg_image_to_tensor: RandomCrop's zero-padded window / CenterCrop, RandomHorizontalFlip, ToTensor, Normalize and Cutout in
    one pass, fp32 NCHW, element for element torchvision's CPU arithmetic.

The host only draws the random parameters (`plan_epoch`, a few numbers per image) and hands the kernels their item tables.  There is
no CPU fallback: a store or a batch that is not on a HIP device raises.

`DeviceLoader` yields `(data, target)` and `PairLoader` yields `(a, p, issame)`: the iterables `Manager.train / validate /
eval_embeddings` and `CPGSession.run_task` already take in place of the reference's `train_loader` / `val_loader`.
"""
import ctypes
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)     # utils/fine_grained_dataset.py:9-10 (the public ImageNet statistics)
IMAGENET_STD = (0.229, 0.224, 0.225)
FACE_MEAN = (0.5, 0.5, 0.5)               # utils/face_dataset.py:6-7, CPG_face_main.py:290-291
FACE_STD = (0.5, 0.5, 0.5)
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')   # torchvision's ImageFolder

_NO_CPU = ('cpg_amd.data: %s lives on %s; image batches are built by HIP kernels on the device '
           '(no CPU fallback -- give the store a HIP device)')


def _require_device(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(_NO_CPU % (what, getattr(t, 'device', type(t).__name__)))


def _items(ctype, rows):
    arr = (ctype * max(1, len(rows)))()
    for i, r in enumerate(rows):
        arr[i] = ctype(*r)
    return arr


def resample(src, src_bytes, rows, dst, dst_bytes):
    """Enqueue cpg_image_resample on the current stream.  rows: (src_off, src_h, src_w, crop_y, crop_x, crop_h, crop_w, dst_off,
    out_h, out_w) per item.  src / dst: uint8 device tensors (or None with a byte count of 0 for an empty call)."""
    lib = _lib.lib()
    items = _items(_lib.ResampleItem, rows)
    nbytes = lib.cpg_image_resample_workspace_bytes(items, len(rows))
    ws, wsb = _lib.workspace(nbytes, dst.device) if nbytes else (None, 0)
    _lib.call('cpg_image_resample', _lib.dptr(src, torch.uint8, 'image store'), int(src_bytes), items, len(rows),
              _lib.dptr(dst, torch.uint8, 'resample destination'), int(dst_bytes), _lib.dptr(ws), wsb, _lib.stream_ptr())


def to_tensor(src, src_bytes, rows, out_h, out_w, mean, std, dst):
    """Enqueue cpg_image_to_tensor: rows (src_off, src_h, src_w, y0, x0, flip, cut_y0, cut_y1, cut_x0, cut_x1) -> dst[i]."""
    items = _items(_lib.TensorItem, [tuple(r) + (0,) for r in rows])
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.call('cpg_image_to_tensor', _lib.dptr(src, torch.uint8, 'image store'), int(src_bytes), items, len(rows), int(out_h), int(out_w), m, s,
              _lib.dptr(dst, torch.float32, 'batch'), dst.numel() * 4, _lib.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------- the store
def resize_size(h, w, rule):
    """Output (h, w) of the store-wide deterministic resize.  rule: int N -> short side N, long side int(N * long / short), the
    image untouched when its short side already is N (torchvision Resize(N) / Scale(N), utils/fine_grained_dataset.py:138-151);
    (w, h) -> exactly that size (Scale((224, 224))); None -> unchanged."""
    if rule is None:
        return h, w
    if isinstance(rule, (tuple, list)):
        return int(rule[1]), int(rule[0])
    n = int(rule)
    if (w <= h and w == n) or (h <= w and h == n):
        return h, w
    if w < h:
        return int(n * h / w), n
    return n, int(n * w / h)


class ImageStore(object):
    """N RGB images (HWC uint8, sizes may differ) in one flat device buffer, with their labels.

    data: uint8 device tensor; labels: int64 device tensor (labels_host: its host copy); offsets / heights / widths: host int64
    arrays (byte offset and size of each image -- what the host validates and plans with).  paths / classes: set by from_image_folder."""

    def __init__(self, data, labels, offsets, heights, widths, paths=None, classes=None):
        _require_device(data, 'the image store')
        _require_device(labels, 'the label tensor')
        if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
            raise TypeError('cpg_amd.data: the store must be a flat contiguous uint8 tensor')
        self.data = data
        self.labels = labels.to(torch.int64)
        self.labels_host = self.labels.cpu().numpy()       # batches take their labels from here: no device gather, no host stall
        self.offsets = np.asarray(offsets, np.int64)
        self.heights = np.asarray(heights, np.int64)
        self.widths = np.asarray(widths, np.int64)
        n = len(self.offsets)
        if not (len(self.heights) == len(self.widths) == self.labels.numel() == n):
            raise ValueError('cpg_amd.data: %d offsets, %d heights, %d widths, %d labels' % (n, len(self.heights), len(self.widths),
                                                                                          self.labels.numel()))
        if n and ((self.heights < 1).any() or (self.widths < 1).any() or (self.offsets < 0).any()
                  or (self.offsets + self.heights * self.widths * 3 > data.numel()).any()):
            raise ValueError('cpg_amd.data: an image lies outside the store')
        self.paths = list(paths) if paths is not None else None
        self.classes = list(classes) if classes is not None else None

    def __len__(self):
        return len(self.offsets)

    @property
    def nbytes(self):
        """Device bytes of the pixel buffer (CUBS at short side 256 is about 1.6 GB)."""
        return self.data.numel()

    @property
    def device(self):
        return self.data.device

    @classmethod
    def from_arrays(cls, images, labels, device='cuda', paths=None, classes=None):
        """HWC uint8 numpy arrays (H x W x 3) and their integer labels; one host-to-device copy."""
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(_NO_CPU % ('the image store', dev))
        images = [np.ascontiguousarray(im) for im in images]
        for i, im in enumerate(images):
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError('cpg_amd.data: image %d must be an H x W x 3 uint8 array, got %s %s' % (i, im.dtype, im.shape))
        sizes = np.array([im.size for im in images], np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(images) else np.zeros(0, np.int64)
        flat = np.concatenate([im.reshape(-1) for im in images]) if images else np.zeros(1, np.uint8)
        data = torch.from_numpy(flat).to(dev)
        lab = torch.as_tensor(np.asarray(labels, np.int64).reshape(-1)).to(dev)
        return cls(data, lab, offsets, [im.shape[0] for im in images], [im.shape[1] for im in images], paths, classes)

    @classmethod
    def from_image_folder(cls, root, device='cuda', extensions=IMG_EXTENSIONS):
        """A store of an ImageFolder tree (load_image_folder), labels = class indices; paths and classes are kept."""
        images, labels, paths, classes = load_image_folder(root, extensions)
        return cls.from_arrays(images, labels, device, paths=paths, classes=classes)

    def resized(self, rule):
        """A new store with every image resized once on the GPU (cpg_image_resample, PIL BILINEAR): rule as in `resize_size`."""
        if rule is None:
            return self
        out = [resize_size(int(h), int(w), rule) for h, w in zip(self.heights, self.widths)]
        oh = np.array([o[0] for o in out], np.int64)
        ow = np.array([o[1] for o in out], np.int64)
        sizes = oh * ow * 3
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(self) else np.zeros(0, np.int64)
        dst = torch.empty(max(1, int(sizes.sum())), dtype=torch.uint8, device=self.device)
        rows = [(int(self.offsets[i]), int(self.heights[i]), int(self.widths[i]), 0, 0, int(self.heights[i]), int(self.widths[i]),
                 int(offsets[i]), int(oh[i]), int(ow[i])) for i in range(len(self))]
        for at in range(0, len(rows), 1024):           # bounds the workspace of one call
            resample(self.data, self.nbytes, rows[at:at + 1024], dst, dst.numel())
        return ImageStore(dst, self.labels, offsets, oh, ow, self.paths, self.classes)

    def prepared(self, preset):
        """The store resized as `preset` expects it (the table in PRESETS)."""
        return self.resized(PRESETS[preset].resize)


def load_image_folder(root, extensions=IMG_EXTENSIONS):
    """Decode an ImageFolder tree on the host, once: (HWC uint8 images, labels, paths, classes).  torchvision ImageFolder's rules:
    classes are the sorted subdirectory names of `root`, label = index of the class, files are walked in sorted order (symlinks
    followed) and kept when their lower-cased name ends in one of `extensions`; each is decoded with
    PIL.Image.open(f).convert('RGB')."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError('cpg_amd.data: reading an image folder decodes the images with PIL (Pillow), which is not installed; '
                          'decode them yourself and use ImageStore.from_arrays') from e
    paths, labels = scan_image_folder(root, extensions)
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    images = []
    for p in paths:
        with open(p, 'rb') as f:
            images.append(np.asarray(Image.open(f).convert('RGB'), dtype=np.uint8))
    return images, labels, paths, classes


def scan_image_folder(root, extensions=IMG_EXTENSIONS):
    """(paths, labels) in torchvision ImageFolder's order (make_dataset)."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError('cpg_amd.data: no class folders under %s' % root)
    ext = tuple(e.lower() for e in extensions)
    paths, labels = [], []
    for ci, c in enumerate(classes):
        for d, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
            for f in sorted(files):
                if f.lower().endswith(ext):
                    paths.append(os.path.join(d, f))
                    labels.append(ci)
    return paths, labels


# ---------------------------------------------------------------------------------------------------------------- presets
Preset = namedtuple('Preset', 'resize crop size flip cutout mean std shuffle')
# resize: the store's one-time resize (resize_size's rule); crop: None (the whole image), 'pad' (RandomCrop(size, padding=4)),
# 'center' (CenterCrop(size)), 'rsc' (RandomSizedCrop(size)); cutout: Cutout(length) or 0; mean / std: defaults (None: the caller's)
PRESETS = {
    # utils/cifar100_dataset.py:7-46 -- the per-task statistics are the caller's (mean=, std=)
    'cifar100_train': Preset(None, 'pad', 32, True, 0, None, None, True),
    'cifar100_val': Preset(None, None, None, False, 0, None, None, False),
    # utils/face_dataset.py:10-45, CPG_face_main.py:286-293 (LFW pairs: face_val)
    'face_train': Preset(112, None, None, True, 0, FACE_MEAN, FACE_STD, True),
    'face_val': Preset(112, None, None, False, 0, FACE_MEAN, FACE_STD, False),
    # utils/fine_grained_dataset.py:36-70
    'fine_grained_train': Preset(256, 'rsc', 224, True, 16, IMAGENET_MEAN, IMAGENET_STD, True),
    'fine_grained_val': Preset(256, 'center', 224, False, 0, IMAGENET_MEAN, IMAGENET_STD, False),
    # utils/fine_grained_dataset.py:73-112
    'fine_grained_train_cropped': Preset((224, 224), None, None, True, 16, IMAGENET_MEAN, IMAGENET_STD, True),
    'fine_grained_val_cropped': Preset((224, 224), None, None, False, 0, IMAGENET_MEAN, IMAGENET_STD, False),
}
PAD = 4                                   # RandomCrop(32, padding=4)

Plan = namedtuple('Plan', 'order out_h out_w crop window flip cutout')
# order: store index of every epoch position; crop: [N, 4] (y, x, h, w) RandomSizedCrop boxes or None; window: [N, 2] (y0, x0)
# top-left of the out_h x out_w window; flip: [N] 0/1; cutout: [N, 4] (y0, y1, x0, x1), all zero when the preset has none


def center_offset(size, out):
    """CenterCrop's offset int(round((size - out) / 2.)) -- Python's round, half to even."""
    return int(round((size - out) / 2.))


def random_sized_crop(rng, heights, widths):
    """RandomSizedCrop's box (torchvision 0.2.x, the version PyTorch 1.0 used), vectorised over images: up to 10 attempts of
    area * U(0.08, 1), aspect U(3/4, 4/3), w = int(round(sqrt(a * r))), h = int(round(sqrt(a / r))), swapped with p = 0.5, kept
    if it fits (a zero size is a failed attempt), then the corner uniformly; when no attempt fits, the centred min(W, H) square.
    Returns [N, 4] int64 (y, x, h, w)."""
    H = np.asarray(heights, np.float64)
    W = np.asarray(widths, np.float64)
    n = len(H)
    area = (H * W)[:, None]
    target = rng.uniform(0.08, 1.0, (n, 10)) * area
    aspect = rng.uniform(3. / 4, 4. / 3, (n, 10))
    w = np.rint(np.sqrt(target * aspect)).astype(np.int64)          # np.rint: round half to even, as Python's round
    h = np.rint(np.sqrt(target / aspect)).astype(np.int64)
    swap = rng.random((n, 10)) < 0.5
    w, h = np.where(swap, h, w), np.where(swap, w, h)
    ok = (w >= 1) & (h >= 1) & (w <= W[:, None]) & (h <= H[:, None])
    first = np.argmax(ok, axis=1)
    found = ok[np.arange(n), first]
    cw = w[np.arange(n), first]
    ch = h[np.arange(n), first]
    u = rng.random((n, 2))
    Hi, Wi = H.astype(np.int64), W.astype(np.int64)
    y = np.minimum((u[:, 0] * (Hi - ch + 1)).astype(np.int64), Hi - ch)
    x = np.minimum((u[:, 1] * (Wi - cw + 1)).astype(np.int64), Wi - cw)
    side = np.minimum(Hi, Wi)
    fy, fx = (Hi - side) // 2, (Wi - side) // 2
    return np.stack([np.where(found, y, fy), np.where(found, x, fx), np.where(found, ch, side), np.where(found, cw, side)], 1)


def plan_epoch(heights, widths, preset, epoch, seed=0, shuffle=None):
    """The host half of an epoch: the order and every per-image random parameter, drawn from a generator seeded by (seed, epoch)
    -- equal seeds give equal epochs, every epoch is reshuffled.  heights / widths: sizes of the store's images (after the preset's
    resize).  Needs no GPU."""
    p = PRESETS[preset] if isinstance(preset, str) else preset
    H = np.asarray(heights, np.int64)
    W = np.asarray(widths, np.int64)
    n = len(H)
    rng = np.random.default_rng([int(seed), int(epoch)])
    shuffle = p.shuffle if shuffle is None else shuffle
    order = rng.permutation(n).astype(np.int64) if shuffle else np.arange(n, dtype=np.int64)
    h, w = H[order], W[order]
    crop = None
    window = np.zeros((n, 2), np.int64)
    if p.crop is None:
        if n and ((h != h[0]).any() or (w != w[0]).any()):
            raise ValueError('cpg_amd.data: preset %s batches whole images, which must all have one size (found %s)'
                             % (preset, sorted(set(zip(H.tolist(), W.tolist())))[:4]))
        out_h, out_w = (int(h[0]), int(w[0])) if n else (1, 1)
    else:
        out_h = out_w = p.size
        if p.crop == 'pad':
            # RandomCrop(size, padding=4): a corner of the zero-padded image, i.e. an offset in [-4, H + 4 - size]
            if n and ((h + 2 * PAD < out_h).any() or (w + 2 * PAD < out_w).any()):
                raise ValueError('cpg_amd.data: an image is smaller than the padded crop')
            window[:, 0] = rng.integers(0, h + 2 * PAD - out_h + 1) - PAD
            window[:, 1] = rng.integers(0, w + 2 * PAD - out_w + 1) - PAD
        elif p.crop == 'center':
            window[:, 0] = [center_offset(int(v), out_h) for v in h]
            window[:, 1] = [center_offset(int(v), out_w) for v in w]
        elif p.crop == 'rsc':
            crop = random_sized_crop(rng, h, w)
        else:
            raise ValueError('cpg_amd.data: unknown crop %r' % (p.crop,))
    flip = (rng.random(n) < 0.5).astype(np.int64) if p.flip else np.zeros(n, np.int64)
    cutout = np.zeros((n, 4), np.int64)
    if p.cutout:
        half = p.cutout // 2
        cy = rng.integers(0, out_h, n)
        cx = rng.integers(0, out_w, n)
        cutout[:, 0] = np.clip(cy - half, 0, out_h)
        cutout[:, 1] = np.clip(cy + half, 0, out_h)
        cutout[:, 2] = np.clip(cx - half, 0, out_w)
        cutout[:, 3] = np.clip(cx + half, 0, out_w)
    return Plan(order, out_h, out_w, crop, window, flip, cutout)


def num_batches(n, batch_size, drop_last=False):
    """DataLoader's len(): ceil(N / B), or floor(N / B) with drop_last."""
    return n // batch_size if drop_last else (n + batch_size - 1) // batch_size


def shard_rows(n_rows, rank, world):
    """Rows [rank * n / world, (rank + 1) * n / world) of a global batch of n rows -- cpg_amd.dist.shard_batch's split, which
    refuses a batch that does not divide."""
    if n_rows % world:
        raise ValueError('global batch %d is not divisible by world size %d' % (n_rows, world))
    per = n_rows // world
    return rank * per, (rank + 1) * per


def build_batch(store, plan, positions, mean, std):
    """(fp32 NCHW batch, int64 labels) of the given epoch positions of `plan`, built on the device on the current stream."""
    _require_device(store.data, 'the image store')
    positions = np.asarray(positions, np.int64)
    idx = plan.order[positions]
    n = len(idx)
    dev = store.device
    x = torch.empty((n, 3, plan.out_h, plan.out_w), dtype=torch.float32, device=dev)
    src, src_bytes = store.data, store.nbytes
    offs, hs, ws = store.offsets[idx], store.heights[idx], store.widths[idx]
    if plan.crop is not None and n:
        # RandomSizedCrop: crop + resize into a uint8 staging batch, then the window is that whole image
        per = plan.out_h * plan.out_w * 3
        stage = torch.empty(n * per, dtype=torch.uint8, device=dev)
        c = plan.crop[positions]
        resample(src, src_bytes, [(int(offs[i]), int(hs[i]), int(ws[i]), int(c[i, 0]), int(c[i, 1]), int(c[i, 2]), int(c[i, 3]), i * per,
                                   plan.out_h, plan.out_w) for i in range(n)], stage, stage.numel())
        src, src_bytes = stage, stage.numel()
        offs = np.arange(n, dtype=np.int64) * per
        hs = np.full(n, plan.out_h, np.int64)
        ws = np.full(n, plan.out_w, np.int64)
        win = np.zeros((n, 2), np.int64)
    else:
        win = plan.window[positions]
    fl, cut = plan.flip[positions], plan.cutout[positions]
    if n:
        to_tensor(src, src_bytes, [(int(offs[i]), int(hs[i]), int(ws[i]), int(win[i, 0]), int(win[i, 1]), int(fl[i]), int(cut[i, 0]),
                                    int(cut[i, 1]), int(cut[i, 2]), int(cut[i, 3])) for i in range(n)],
                  plan.out_h, plan.out_w, mean, std, x)
    # from pinned memory, asynchronously: a copy from pageable memory would make the host wait for the previous step to finish
    y = torch.from_numpy(store.labels_host[idx]).pin_memory().to(dev, non_blocking=True)
    return x, y


def _norm(preset, mean, std):
    p = PRESETS[preset]
    mean = p.mean if mean is None else mean
    std = p.std if std is None else std
    if mean is None or std is None:
        raise ValueError('cpg_amd.data: preset %s needs the dataset\'s mean= and std=' % preset)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError('cpg_amd.data: mean and std take 3 values')
    return tuple(float(v) for v in mean), tuple(float(v) for v in std)


class DeviceLoader(object):
    """DataLoader(ImageFolder(root, transform), batch_size, shuffle) of one of the reference's loaders (PRESETS), with every batch
    built on the GPU from `store` (already resized as the preset expects: store.prepared(preset)).

    Iterating yields (fp32 NCHW device tensor, int64 device labels), fresh tensors from torch's allocator on the current stream;
    every iteration is the next epoch (set_epoch chooses one).  world > 1: this rank's rows [rank * B / world, (rank + 1) * B /
    world) of each global batch -- cpg_amd.dist.shard_batch of the full batch."""

    def __init__(self, store, batch_size, preset, shuffle=None, seed=0, drop_last=False, rank=0, world=1, mean=None, std=None):
        if preset not in PRESETS:
            raise ValueError('cpg_amd.data: unknown preset %r (one of %s)' % (preset, ', '.join(sorted(PRESETS))))
        _require_device(store.data, 'the image store')
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError('cpg_amd.data: batch_size %d, rank %d, world %d' % (batch_size, rank, world))
        self.store, self.batch_size, self.preset = store, int(batch_size), preset
        self.shuffle = PRESETS[preset].shuffle if shuffle is None else bool(shuffle)
        self.seed, self.drop_last, self.rank, self.world = int(seed), bool(drop_last), int(rank), int(world)
        self.mean, self.std = _norm(preset, mean, std)
        n = len(store)
        for b in range(len(self)):
            shard_rows(min(self.batch_size, n - b * self.batch_size), 0, self.world)     # refuse an uneven global batch now
        self.epoch = 0

    def __len__(self):
        return num_batches(len(self.store), self.batch_size, self.drop_last)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def plan(self, epoch=None):
        st = self.store
        return plan_epoch(st.heights, st.widths, self.preset, self.epoch if epoch is None else epoch, self.seed, self.shuffle)

    def __iter__(self):
        plan = self.plan()
        self.epoch += 1
        n = len(self.store)
        for b in range(len(self)):
            lo, hi = b * self.batch_size, min(n, (b + 1) * self.batch_size)
            r0, r1 = shard_rows(hi - lo, self.rank, self.world)
            yield build_batch(self.store, plan, np.arange(lo + r0, lo + r1), self.mean, self.std)


# ---------------------------------------------------------------------------------------------------------------- LFW pairs
def read_lfw_pairs(pairs_path):
    """utils/LFWDataset.py:17-23: every line after the first, split on whitespace."""
    with open(pairs_path) as f:
        return [ln.strip().split() for ln in f.readlines()[1:]]


def lfw_pair_paths(lfw_dir, pairs, file_ext='jpg'):
    """utils/LFWDataset.py:25-45: 3 fields (name, n1, n2) = same person, 4 fields (name1, n1, name2, n2) = different people; a
    pair with a missing file is skipped.  Returns ([(path0, path1, issame)], number skipped).  (Lines of any other length are
    skipped and counted too: the reference would fail on them.)"""
    out, skipped = [], 0
    for pair in pairs:
        if len(pair) == 3:
            p0 = os.path.join(lfw_dir, pair[0], pair[0] + '_' + '%04d' % int(pair[1]) + '.' + file_ext)
            p1 = os.path.join(lfw_dir, pair[0], pair[0] + '_' + '%04d' % int(pair[2]) + '.' + file_ext)
            same = True
        elif len(pair) == 4:
            p0 = os.path.join(lfw_dir, pair[0], pair[0] + '_' + '%04d' % int(pair[1]) + '.' + file_ext)
            p1 = os.path.join(lfw_dir, pair[2], pair[2] + '_' + '%04d' % int(pair[3]) + '.' + file_ext)
            same = False
        else:
            skipped += 1
            continue
        if os.path.exists(p0) and os.path.exists(p1):
            out.append((p0, p1, same))
        else:
            skipped += 1
    return out, skipped


class PairLoader(object):
    """The reference's LFW validation loader (CPG_face_main.py:286-293 over utils/LFWDataset.py): yields (a, p, issame) batches
    through the face-val transform (the store's images as they are -- store.prepared('face_val') -- ToTensor, Normalize 0.5 / 0.5).
    pairs: [(store index a, store index p, issame)] or [(path a, path p, issame)] when the store was read from an image folder.
    issame is a bool tensor on the host, as DataLoader collates it; a and p are on the device."""

    def __init__(self, store, pairs, batch_size, mean=FACE_MEAN, std=FACE_STD):
        _require_device(store.data, 'the image store')
        index = {os.path.normpath(p): i for i, p in enumerate(store.paths)} if store.paths else {}
        a, p, s = [], [], []
        for x, y, same in pairs:
            a.append(index[os.path.normpath(x)] if isinstance(x, str) else int(x))
            p.append(index[os.path.normpath(y)] if isinstance(y, str) else int(y))
            s.append(bool(same))
        self.store, self.batch_size = store, int(batch_size)
        self.a, self.p, self.issame = np.array(a, np.int64), np.array(p, np.int64), np.array(s, bool)
        self.mean, self.std = tuple(mean), tuple(std)

    @classmethod
    def from_lfw(cls, store, lfw_dir, pairs_path, batch_size, file_ext='jpg'):
        pairs, skipped = lfw_pair_paths(lfw_dir, read_lfw_pairs(pairs_path), file_ext)
        loader = cls(store, pairs, batch_size)
        loader.skipped = skipped
        return loader

    def __len__(self):
        return num_batches(len(self.a), self.batch_size)

    def __iter__(self):
        st = self.store
        for b in range(len(self)):
            sl = slice(b * self.batch_size, (b + 1) * self.batch_size)
            out = []
            for idx in (self.a[sl], self.p[sl]):
                plan = plan_epoch(st.heights[idx], st.widths[idx], 'face_val', 0)
                plan = plan._replace(order=idx)
                out.append(build_batch(st, plan, np.arange(len(idx)), self.mean, self.std)[0])
            yield out[0], out[1], torch.from_numpy(self.issame[sl].copy())


__all__ = ['ImageStore', 'DeviceLoader', 'PairLoader', 'PRESETS', 'plan_epoch', 'random_sized_crop', 'center_offset', 'resize_size',
           'num_batches', 'shard_rows', 'scan_image_folder', 'load_image_folder', 'read_lfw_pairs', 'lfw_pair_paths', 'build_batch', 'IMAGENET_MEAN',
           'IMAGENET_STD', 'FACE_MEAN', 'FACE_STD']
