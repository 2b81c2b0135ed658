"""Test reference for the data path (cpg_amd/data.py): the reference's PIL / torchvision pixel arithmetic restated in vectorised
numpy.  The product has no CPU fallback, so this lives with the tests.  Its resample is checked against PIL itself on the CPU
(tests/test_data_host.py); the GPU tests compare the kernels with it, which carries PIL exactness over without needing PIL there.
"""
import numpy as np

PRECISION_BITS = 22               # Pillow Resample.c, 8 bits per channel: 32 - 8 - 2


def _coeffs(in_size, out_size):
    """Pillow's precompute_coeffs (bilinear, box [0, in_size)) + normalize_coeffs_8bpc as a dense [out, in] int64 matrix."""
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    k = np.zeros((out_size, in_size), np.int64)
    for o in range(out_size):
        center = 0.0 + (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        x = np.arange(xmin, xmax)
        t = np.abs((x - center + 0.5) * ss)
        w = np.where(t < 1.0, 1.0 - t, 0.0)
        ww = 0.0
        for v in w:                                    # the C loop's summation order
            ww += v
        if ww != 0.0:
            w = w / ww
        k[o, xmin:xmax] = np.where(w < 0, (-0.5 + w * (1 << PRECISION_BITS)).astype(np.int64),
                                   (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64))
    return k


def _pass(img, k, axis):
    acc = np.tensordot(img.astype(np.int64), k, axes=([axis], [1]))        # the resampled axis moves last
    acc = np.moveaxis(acc, -1, axis) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample(img, crop, out_h, out_w):
    """PIL.Image.fromarray(img).crop((x, y, x + w, y + h)).resize((out_w, out_h), Image.BILINEAR) of an HWC uint8 image;
    crop = (y, x, h, w)."""
    y, x, h, w = (int(v) for v in crop)
    c = img[y:y + h, x:x + w]
    if out_w != w:
        c = _pass(c, _coeffs(w, out_w), 1)
    if out_h != h:
        c = _pass(c, _coeffs(h, out_h), 0)
    return np.ascontiguousarray(c)


def window(img, y0, x0, out_h, out_w, flip):
    """The out_h x out_w window at (y0, x0) of an HWC uint8 image, zero bytes outside it (RandomCrop's padding), columns reversed
    when flip (RandomHorizontalFlip after the crop)."""
    H, W = img.shape[:2]
    ys = np.arange(out_h) + y0
    wx = np.arange(out_w)
    if flip:
        wx = out_w - 1 - wx
    xs = wx + x0
    inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    u = img[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)]
    return np.where(inside[..., None], u, 0).astype(np.uint8)


def to_tensor(img, y0, x0, out_h, out_w, flip, cutout, mean, std):
    """Window, flip, ToTensor, Normalize, Cutout -> fp32 [3, out_h, out_w]; cutout = (y0, y1, x0, x1)."""
    u = window(img, y0, x0, out_h, out_w, flip)
    v = u.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    v = (v - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]
    cy0, cy1, cx0, cx1 = (int(c) for c in cutout)
    v[:, cy0:cy1, cx0:cx1] *= np.float32(0.0)
    return v


def batch(images, labels, plan, positions, mean, std):
    """What DeviceLoader builds for the given epoch positions of `plan` (cpg_amd.data.plan_epoch): (fp32 [n, 3, H, W], int64 [n])."""
    out = np.empty((len(positions), 3, plan.out_h, plan.out_w), np.float32)
    lab = np.empty(len(positions), np.int64)
    for r, pos in enumerate(positions):
        i = int(plan.order[pos])
        img = images[i]
        y0, x0 = (int(v) for v in plan.window[pos])
        if plan.crop is not None:
            img = resample(img, plan.crop[pos], plan.out_h, plan.out_w)
            y0 = x0 = 0
        out[r] = to_tensor(img, y0, x0, plan.out_h, plan.out_w, int(plan.flip[pos]), plan.cutout[pos], mean, std)
        lab[r] = labels[i]
    return out, lab


def resize_rule(img, rule):
    """The store's one-time resize (cpg_amd.data.resize_size) of one image."""
    from cpg_amd.data import resize_size
    h, w = img.shape[:2]
    oh, ow = resize_size(h, w, rule)
    return resample(img, (0, 0, h, w), oh, ow)
