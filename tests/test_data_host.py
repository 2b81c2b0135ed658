"""Host half of the data path (cpg_amd/data.py), no GPU: the test reference's resample against PIL, epoch planning, the
ImageFolder scan, the LFW pairs parser, and the C ABI's host-side validation of image item tables."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _imaging as I
import cpg_amd._lib as L
from cpg_amd import data as D


# ------------------------------------------------------------------------------------------------ the test reference vs PIL
def _pil_cases(rng, n):
    cases = []
    for t in range(n):
        kind = t % 5
        if kind == 0:                                   # 1-pixel edges
            H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
            oh, ow = int(rng.integers(1, 3)), int(rng.integers(1, 60))
            if t % 2:
                oh, ow = ow, oh
        elif kind == 1:                                 # reduce by more than 8x
            H, W = int(rng.integers(200, 600)), int(rng.integers(200, 600))
            oh, ow = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        elif kind == 2:                                 # enlarge by more than 8x
            H, W = int(rng.integers(1, 20)), int(rng.integers(1, 20))
            oh, ow = int(rng.integers(160, 300)), int(rng.integers(160, 300))
        else:
            H, W = int(rng.integers(1, 300)), int(rng.integers(1, 300))
            oh, ow = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        if kind == 4:                                   # identity, and one axis kept
            oh, ow = (h, w) if t % 2 else (h, int(rng.integers(1, 300)))
        cases.append((rng.integers(0, 256, (H, W, 3), dtype=np.uint8), (y, x, h, w), oh, ow))
    return cases


def test_imaging_resample_matches_pil_bit_for_bit():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(7)
    bad = []
    for n, (img, (y, x, h, w), oh, ow) in enumerate(_pil_cases(rng, 240)):
        ref = np.asarray(Image.fromarray(img).crop((x, y, x + w, y + h)).resize((ow, oh), Image.BILINEAR))
        got = I.resample(img, (y, x, h, w), oh, ow)
        if ref.shape != got.shape or (ref != got).any():
            bad.append((n, img.shape, (y, x, h, w), (oh, ow)))
    assert not bad, bad[:5]


def test_imaging_to_tensor_is_torch_cpu_arithmetic():
    """ToTensor + Normalize on torch-CPU: u.float() / 255, then (v - mean) / std; a multiply by 1/255 would differ."""
    u = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    mean, std = (0.5071, 0.4865, 0.4409), (0.2673, 0.2564, 0.2762)
    got = I.to_tensor(u, 0, 0, 16, 16, 0, (0, 0, 0, 0), mean, std)
    t = torch.from_numpy(u).permute(2, 0, 1).float().div(255)
    ref = ((t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)).numpy()
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    recip = (torch.from_numpy(u[..., 0]).float() * (1.0 / 255)).numpy()
    assert (recip != (torch.from_numpy(u[..., 0]).float() / 255).numpy()).sum() > 0


# ------------------------------------------------------------------------------------------------ plan_epoch
def test_plan_permutation_reshuffle_and_seed():
    hw = [32] * 50
    a0 = D.plan_epoch(hw, hw, 'cifar100_train', 0, seed=3)
    a1 = D.plan_epoch(hw, hw, 'cifar100_train', 1, seed=3)
    b0 = D.plan_epoch(hw, hw, 'cifar100_train', 0, seed=3)
    assert sorted(a0.order.tolist()) == list(range(50)) == sorted(a1.order.tolist())
    assert not np.array_equal(a0.order, a1.order)
    for f in ('order', 'window', 'flip', 'cutout'):
        assert np.array_equal(getattr(a0, f), getattr(b0, f)), f
    assert not np.array_equal(D.plan_epoch(hw, hw, 'cifar100_train', 0, seed=4).order, a0.order)
    assert np.array_equal(D.plan_epoch(hw, hw, 'cifar100_val', 5).order, np.arange(50))


def test_plan_parameter_ranges():
    n = 4000
    p = D.plan_epoch([32] * n, [32] * n, 'cifar100_train', 0, seed=1)
    assert (p.out_h, p.out_w) == (32, 32) and p.crop is None
    assert p.window.min() == -4 and p.window.max() == 4
    assert set(p.flip.tolist()) == {0, 1} and 0.45 < p.flip.mean() < 0.55
    assert not p.cutout.any()
    rng = np.random.default_rng(0)
    H = rng.integers(256, 700, n)
    W = rng.integers(256, 700, n)
    H[::2] = 256
    W[1::2] = 256
    p = D.plan_epoch(H, W, 'fine_grained_train', 2, seed=1)
    h, w = H[p.order], W[p.order]
    y, x, ch, cw = p.crop.T
    assert (ch >= 1).all() and (cw >= 1).all() and (y >= 0).all() and (x >= 0).all()
    assert (y + ch <= h).all() and (x + cw <= w).all()
    frac = ch * cw / (h * w)
    assert frac.min() > 0.07 and frac.max() <= 1.0
    ratio = cw / ch
    assert ratio.min() > 0.74 * 0.9 and ratio.max() < 1.34 / 0.9
    cy0, cy1, cx0, cx1 = p.cutout.T
    assert (cy0 >= 0).all() and (cy1 <= 224).all() and (cx0 >= 0).all() and (cx1 <= 224).all()
    assert (cy1 - cy0).max() == 16 and (cy1 - cy0).min() >= 8 and (cy1 > cy0).all() and (cx1 > cx0).all()
    assert ((cy0 == 0) & (cy1 < 16)).any() and ((cx1 == 224) & (cx0 > 208)).any()   # clipped at the corners
    assert 0.45 < p.flip.mean() < 0.55
    for name in ('face_train', 'fine_grained_train_cropped'):
        q = D.plan_epoch([112] * 100, [112] * 100, name, 0)
        assert q.crop is None and not q.window.any() and 0 < q.flip.sum() < 100
    assert D.plan_epoch([224] * 100, [224] * 100, 'fine_grained_train_cropped', 0).cutout.any()
    assert not D.plan_epoch([112] * 9, [112] * 9, 'face_val', 0).flip.any()


def test_random_sized_crop_fallback_on_a_1x300_image():
    p = D.plan_epoch([1] * 20, [300] * 20, 'fine_grained_train', 0)
    assert (p.crop == np.array([0, 149, 1, 1])).all()           # the centred min(W, H) square


def test_center_crop_rounds_half_to_even():
    assert D.center_offset(256, 224) == 16
    assert D.center_offset(225, 224) == 0       # round(0.5) = 0
    assert D.center_offset(227, 224) == 2       # round(1.5) = 2
    assert D.center_offset(229, 224) == 2       # round(2.5) = 2
    assert D.center_offset(231, 224) == 4       # round(3.5) = 4
    p = D.plan_epoch([256, 227, 341], [229, 300, 256], 'fine_grained_val', 0)
    assert p.window.tolist() == [[16, 2], [2, 38], [58, 16]]


def test_short_side_resize_sizes():
    assert D.resize_size(500, 375, 256) == (341, 256)           # int(256 * 500 / 375)
    assert D.resize_size(375, 500, 256) == (256, 341)
    assert D.resize_size(256, 400, 256) == (256, 400)           # short side already 256: untouched
    assert D.resize_size(400, 256, 256) == (400, 256)
    assert D.resize_size(100, 100, 112) == (112, 112)
    assert D.resize_size(250, 250, 112) == (112, 112)
    assert D.resize_size(10, 300, (224, 224)) == (224, 224)
    assert D.resize_size(120, 90, (100, 50)) == (50, 100)       # Scale((w, h))
    assert D.resize_size(7, 9, None) == (7, 9)


def test_len_with_and_without_drop_last():
    assert D.num_batches(10, 4) == 3 and D.num_batches(10, 4, drop_last=True) == 2
    assert D.num_batches(8, 4) == 2 == D.num_batches(8, 4, True)
    assert D.num_batches(3, 4) == 1 and D.num_batches(3, 4, True) == 0


def test_shard_rows_and_uneven_refusal():
    assert [D.shard_rows(8, r, 4) for r in range(4)] == [(0, 2), (2, 4), (4, 6), (6, 8)]
    assert D.shard_rows(6, 1, 2) == (3, 6)
    with pytest.raises(ValueError, match='not divisible'):
        D.shard_rows(6, 0, 4)


# ------------------------------------------------------------------------------------------------ image folders, LFW pairs
def test_image_folder_scan_rules(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(0)
    for cls_name in ('zebra', 'Apple', 'mango'):
        os.makedirs(tmp_path / cls_name / 'sub')
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / 'zebra' / 'b.png')
    Image.fromarray(gray).save(tmp_path / 'zebra' / 'a.PNG')
    Image.fromarray(rgb).save(tmp_path / 'Apple' / 'sub' / 'c.png')
    Image.fromarray(rgb).save(tmp_path / 'mango' / 'd.png')
    (tmp_path / 'mango' / 'notes.txt').write_text('not an image')
    (tmp_path / 'stray.png').write_bytes(b'')                     # files at the root are not a class
    images, labels, paths, classes = D.load_image_folder(str(tmp_path))
    assert classes == ['Apple', 'mango', 'zebra']
    assert [os.path.relpath(p, str(tmp_path)) for p in paths] == [os.path.join('Apple', 'sub', 'c.png'), os.path.join('mango', 'd.png'),
                                                                  os.path.join('zebra', 'a.PNG'), os.path.join('zebra', 'b.png')]
    assert labels == [0, 1, 2, 2]
    assert images[2].shape == (4, 6, 3) and (images[2] == gray[..., None]).all()
    assert np.array_equal(images[3], rgb)


def test_lfw_pairs_parser(tmp_path):
    for name, nums in (('Ann', (1, 2)), ('Bob', (1,)), ('Cy', (3,))):
        os.makedirs(tmp_path / 'lfw' / name)
        for k in nums:
            (tmp_path / 'lfw' / name / ('%s_%04d.jpg' % (name, k))).write_bytes(b'x')
    pairs = tmp_path / 'pairs.txt'
    pairs.write_text('10\t300\nAnn\t1\t2\nAnn\t1\t5\nBob\t1\tCy\t3\nBob\t2\tCy\t3\n')
    rows = D.read_lfw_pairs(str(pairs))
    assert rows == [['Ann', '1', '2'], ['Ann', '1', '5'], ['Bob', '1', 'Cy', '3'], ['Bob', '2', 'Cy', '3']]
    out, skipped = D.lfw_pair_paths(str(tmp_path / 'lfw'), rows)
    root = str(tmp_path / 'lfw')
    assert skipped == 2
    assert out == [(os.path.join(root, 'Ann', 'Ann_0001.jpg'), os.path.join(root, 'Ann', 'Ann_0002.jpg'), True),
                   (os.path.join(root, 'Bob', 'Bob_0001.jpg'), os.path.join(root, 'Cy', 'Cy_0003.jpg'), False)]


# ------------------------------------------------------------------------------------------------ C ABI validation (no device)
def _rs(**kw):
    f = dict(src_off=0, src_h=10, src_w=12, crop_y=0, crop_x=0, crop_h=10, crop_w=12, dst_off=0, out_h=5, out_w=6)
    f.update(kw)
    return L.ResampleItem(**f)


def _ti(**kw):
    f = dict(src_off=0, src_h=10, src_w=12, y0=0, x0=0, flip=0, cut_y0=0, cut_y1=0, cut_x0=0, cut_x1=0, reserved=0)
    f.update(kw)
    return L.TensorItem(**f)


FAKE = ctypes.c_void_p(1 << 40)           # never dereferenced: validation fails before any HIP call


def _resample(items, src_bytes=360, dst_bytes=90, ws_bytes=1 << 20):
    arr = (L.ResampleItem * len(items))(*items)
    return L.lib().cpg_image_resample(FAKE, src_bytes, arr, len(items), FAKE, dst_bytes, FAKE, ws_bytes, None)


def _to_tensor(items, out_h=4, out_w=4, dst_bytes=1 << 20, std=1.0):
    arr = (L.TensorItem * len(items))(*items)
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    s = (ctypes.c_float * 3)(std, std, std)
    return L.lib().cpg_image_to_tensor(FAKE, 360, arr, len(items), out_h, out_w, m, s, FAKE, dst_bytes, None)


@pytest.mark.parametrize('bad, words', [
    (dict(crop_y=1), 'crop'),                       # crop past the bottom of the image
    (dict(crop_x=-1, crop_w=5), 'crop'),
    (dict(crop_w=13), 'crop'),
    (dict(crop_h=0), 'crop'),                       # zero size
    (dict(out_w=0), 'output size'),
    (dict(src_h=0), 'image size'),
    (dict(src_off=1), 'store'),                     # image extends past src_bytes
    (dict(dst_off=1), 'destination'),               # destination past dst_bytes
    (dict(out_h=6), 'destination'),
])
def test_resample_refuses_bad_items_before_launching(bad, words):
    rc = _resample([_rs(), _rs(**bad)])
    assert rc == -1                                                   # CPG_E_INVALID
    err = L.lib().cpg_last_error().decode()
    assert 'item 1' in err and words in err, err


def test_resample_workspace_query_and_refusal():
    lib = L.lib()
    items = [_rs(), _rs(out_h=10), _rs(out_w=12), _rs(crop_h=7, crop_w=5, out_h=3, out_w=9)]
    arr = (L.ResampleItem * 4)(*items)
    # only items that change both sizes stage their horizontal pass: crop_h x out_w x 3 bytes, each rounded up to 16
    assert lib.cpg_image_resample_workspace_bytes(arr, 4) == 192 + 192
    assert lib.cpg_image_resample_workspace_bytes(arr, 0) == 0
    assert _resample(items, dst_bytes=1 << 20, ws_bytes=383) == -3      # CPG_E_WORKSPACE
    assert 'workspace' in lib.cpg_last_error().decode()
    assert _resample([], ws_bytes=0) == 0


@pytest.mark.parametrize('bad, words', [
    (dict(src_off=200), 'store'),
    (dict(src_w=0), 'image size'),
    (dict(flip=2), 'flip'),
    (dict(cut_y1=5), 'cutout'),
    (dict(cut_x0=-1), 'cutout'),
    (dict(y0=1 << 21), 'window'),
])
def test_to_tensor_refuses_bad_items_before_launching(bad, words):
    assert _to_tensor([_ti(), _ti(**bad)]) == -1
    err = L.lib().cpg_last_error().decode()
    assert 'item 1' in err and words in err, err


def test_to_tensor_refuses_short_destination_and_bad_sizes():
    assert _to_tensor([_ti()] * 3, dst_bytes=3 * 3 * 16 * 4 - 1) == -1
    assert 'destination' in L.lib().cpg_last_error().decode()
    assert _to_tensor([_ti()], out_h=0) == -1
    assert _to_tensor([_ti()], std=0.0) == -1


def test_cpu_store_has_no_fallback():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        D.ImageStore.from_arrays([np.zeros((4, 4, 3), np.uint8)], [0], device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        D.ImageStore(torch.zeros(48, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), [0], [4], [4])
