"""Case tables and bodies of the fp64 / oracle parity tests that run twice: plainly (tests/test_hip_parity.py, the ids they always
had) and with every buffer between guard bands (tests/test_guard_bands_gpu.py).  A body takes a buffer factory: PLAIN is what the
tests always did (`.to(DEV)`, torch.full, torch.empty); tests/_guarded.py has the guarded one.  Every assertion and tolerance lives
here, once; a body returns the tensors the kernels produced, so a guarded run can ask whose memory they are in."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from cpg_amd.models import layers as nl
from cpg_amd.utils.prune import SparsePruner
from oracle import ops                           # (checker only)

DEV = 'cuda:0'


class PlainBuffers(object):
    """Buffers as the tests always made them."""
    guarded = False

    def put(self, t, offset=0):
        """A const input on the device; offset: so many elements into a larger buffer (the off-by-4-bytes cases)."""
        if t is None:
            return None
        if not offset:
            return t.to(DEV).contiguous()
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
        v = buf[offset:].view(t.shape)
        v.copy_(t)
        return v

    def copy(self, t):
        """A tensor the kernels write in place, holding t's values."""
        return t.to(DEV)

    def full(self, shape, value, dtype=torch.float32):
        return torch.full(tuple(shape), value, dtype=dtype, device=DEV)

    def empty(self, shape, dtype=torch.float32):
        return torch.empty(tuple(shape), dtype=dtype, device=DEV)

    def zeros(self, shape, dtype=torch.float32):
        return torch.zeros(tuple(shape), dtype=dtype, device=DEV)

    def rehome(self, module, const_buffers=False):
        """Called once a module's parameters and buffers hold their values, before its first use."""
        return module


PLAIN = PlainBuffers()


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def close(got, want, rtol=1e-4, atol=1e-5, msg=''):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


def running_stats_close(got, want, msg=''):
    """The bar for BatchNorm running statistics that come out of a conv epilogue's partial sums (test_conv_epilogue_bn_statistics
    and the descriptor-space body of tests/_conv_space_cases.py): one definition."""
    close(got, want, rtol=1e-5, atol=1e-6, msg=msg)


def skip_gradient_fused_equals_plain(conv, x0, gy, gs):
    """A conv whose input also feeds an identity branch: through forward_with_skip the two gradients of the input meet inside the
    input-gradient kernel (cpg_conv2d_dgrad_add).  The fused entry point is really the one that runs, and y, gx and the parameter
    gradients equal the plain composition's to 1e-6 of their scale.  conv, x0, gy, gs (the skip branch's gradient) on the device;
    returns the fused run's (y, gx, gw[, gpm])."""
    from cpg_amd import _lib
    calls = []
    L = _lib.lib()
    raw = L.cpg_conv2d_dgrad_add

    class Spy(object):
        def __getattr__(self, name):
            if name == 'cpg_conv2d_dgrad_add':
                def f(*a):
                    calls.append(1)
                    return raw(*a)
                return f
            return getattr(L, name)
    res = {}
    for fused in (True, False):
        conv.zero_grad()
        x = x0.clone().requires_grad_(True)
        if fused:
            old, _lib._lib = _lib._lib, Spy()
            try:
                y, stats, skip = conv.forward_with_skip(x)
                (y * gy).sum().backward(retain_graph=True, inputs=[conv.weight])       # conv branch alone first: no addend yet
                conv.zero_grad()
                ((y * gy).sum() + (skip * gs).sum()).backward()
            finally:
                _lib._lib = old
        else:
            y = conv(x)
            ((y * gy).sum() + (x * gs).sum()).backward()
        res[fused] = (y.detach().clone(), x.grad.clone(), conv.weight.grad.clone()) + (
            () if conv.piggymask is None else (conv.piggymask.grad.clone(),))
    assert calls, 'the fused input-gradient entry point did not run'
    for a, b in zip(res[True], res[False]):
        sc = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-6 * sc
    return res[True]


# --------------------------------------------------------------------------- conv / linear vs oracle
CONV_ORACLE_CASES = [
    (4, 64, 56, 56, 128, 3, 1, 1, False, False),     # VGG mid layer (3x3 s1 p1), several tiles
    (3, 3, 224, 224, 64, 3, 1, 1, False, False),     # VGG first layer, Cin = 3
    (2, 128, 28, 28, 256, 3, 1, 1, False, True),     # with piggymask
    (5, 512, 14, 14, 512, 3, 1, 1, False, False),    # deep K (4608), small spatial
    (2, 64, 33, 47, 70, 3, 1, 1, True, True),        # ragged everything
    (2, 20, 15, 14, 130, 3, 1, 1, False, True),      # small-map config (<=16 wide), ragged rows, 2 channel tiles
    (1, 70, 30, 56, 64, 3, 1, 1, True, False),       # <=64-channel config, partial 32-wide tiles
    (3, 32, 14, 14, 96, 3, 1, 1, False, False),      # whole-image tiles; wgrad 7x14 units
    (2, 17, 10, 40, 33, 3, 1, 1, False, True),       # channel counts not multiples of the chunk / fragment
    (2, 24, 11, 56, 130, 3, 1, 1, True, False),      # 56-wide tiles (7 fragments), ragged rows, 2 channel tiles
    (1, 40, 9, 112, 48, 3, 1, 1, False, True),       # 56-wide tiles, <= 64 output channels; wgrad 2x28 units
    (3, 2, 13, 37, 70, 3, 1, 1, False, True),        # stem weight-gradient kernel (C <= 3), ragged tiles, 2 co blocks
    (5, 160, 28, 28, 136, 3, 1, 1, False, False),    # two-image 4x28 tiles with an odd image count
    (2, 32, 12, 28, 128, 3, 1, 1, True, True),       # two-image tiles, bias + piggymask
    (4, 16, 14, 14, 72, 3, 1, 1, True, True),        # 14x14 maps: channel-split virtual-row tiles (atomic accumulation), bias on one half
    (6, 32, 7, 7, 160, 3, 1, 1, False, True),        # 7x7 maps: virtual-row tiles over 6 images (fwd + dgrad), 7x8 wgrad units
    (37, 16, 7, 7, 24, 3, 1, 1, True, False),        # 7x7 maps, image count not a multiple of the tile, bias, <= 64 channels
    (5, 12, 6, 8, 20, 3, 1, 1, False, False),        # 6x8 maps: 7x8 wgrad units with a missing row
    (2, 4, 1, 1, 8, 3, 1, 1, True, True),            # 1x1 map: every tap but the centre is padding
    (1, 16, 2, 3, 16, 3, 1, 1, False, False),        # 2x3 map, single image
    (3, 16, 1, 1, 32, 1, 1, 0, False, True),         # pointwise on 1x1 maps (a linear layer in disguise)
    (2, 3, 64, 64, 16, 7, 2, 3, False, False),       # ResNet stem
    (3, 64, 28, 28, 256, 1, 1, 0, False, True),      # ResNet 1x1
    (3, 256, 28, 28, 512, 1, 2, 0, False, False),    # ResNet downsample
    (5, 32, 7, 7, 48, 1, 1, 0, False, True),         # pointwise kernel, 7x7 maps: scalar staging, tiles span 5 images
    (9, 48, 14, 14, 80, 1, 1, 0, True, False),       # pointwise kernel, float4 staging, tiles straddle images, bias
    (2, 16, 15, 15, 32, 1, 2, 0, False, True),       # pointwise stride 2 on an odd map (scatter + zero fill in dgrad)
    (2, 24, 8, 8, 16, 1, 1, 0, False, False),        # 1x1 with C % 16 != 0 -> generic kernel
    (2, 20, 15, 17, 24, 3, 2, 1, False, True),       # strided dgrad by residue classes, odd map
    (1, 8, 20, 20, 8, 5, 3, 2, True, False),         # stride 3, 5x5: nine residue classes with 1..4 taps
    (2, 8, 9, 9, 8, 1, 2, 0, False, False),          # 1x1 s2 on the generic kernel: three classes have no taps (zero fill)
    (2, 130, 12, 12, 70, 3, 2, 1, False, False),     # strided dgrad, > 64 input channels (128-wide tile), ragged channels
    (2, 64, 56, 56, 64, 3, 2, 1, True, False),       # SphereNet stride-2 with bias: <= 64-channel strided tiles, 28-wide class grid
    (3, 128, 56, 56, 128, 3, 2, 1, False, True),     # ResNet layer2 stride-2: two-image 4x28 output strips (odd image count), piggymask
    (5, 96, 28, 28, 136, 3, 2, 1, True, False),      # 14x14 outputs: whole-image strided tile, two-image class-grid tiles, bias
    (9, 64, 14, 14, 160, 3, 2, 1, False, True),      # 7x7 outputs: two-image 8x8 tiles; class grid: one row of eight images (9 images)
    (3, 160, 14, 14, 72, 3, 2, 1, False, False),     # the same with > 64 input channels in the input gradient
    (2, 32, 33, 70, 200, 3, 2, 1, True, True),       # odd map, 35-wide outputs: the general strided tiles
    (1, 16, 2, 2, 16, 3, 2, 1, False, False),        # 2x2 -> 1x1
    (3, 3, 64, 70, 64, 7, 2, 3, False, True),        # ResNet stem on the strided stem kernels: ragged tiles, piggymask
    (2, 3, 37, 45, 64, 7, 2, 3, True, False),        # ... odd map, bias
    (5, 3, 30, 64, 64, 3, 2, 1, True, False),        # SphereNet stem (3x3 s2 from 3 channels, bias)
    (2, 2, 16, 18, 64, 3, 2, 1, False, True),        # ... two input channels
    (1, 3, 224, 224, 64, 7, 2, 3, False, False),     # the ResNet stem's own map: 4 x 32 tiles, several tiles per wave
    # the GROWN VGG16 of configs[1] (raw multiplier 1.5 -> sqrt -> int(v * 1.2247): 78 / 156 / 313 / 627 channels,
    # CPG_cifar100_main_normal.py:115-116 + models/vgg.py:124-154): channel counts that are no multiple of the Winograd kernels' chunk (4) /
    # block (32): the last chunk / block overlaps its neighbour (wg_chunk_base, k0 / c0 in k_wgw)
    (1, 3, 224, 224, 78, 3, 1, 1, False, False),     # features.0 of the grown net (the 64-output stem kernel does not apply)
    (1, 78, 224, 224, 78, 3, 1, 1, False, True),     # features.3
    (2, 78, 112, 112, 156, 3, 1, 1, False, False),   # features.7
    (2, 156, 56, 56, 313, 3, 1, 1, False, True),     # features.14
    (3, 313, 28, 28, 627, 3, 1, 1, False, False),    # features.24
    (5, 627, 14, 14, 627, 3, 1, 1, False, True),     # features.34 (the narrow weight-gradient stages: image pairs, odd image count)
    (2, 33, 28, 28, 35, 3, 1, 1, True, True),        # one channel past the block on both sides, bias
    (2, 67, 14, 14, 61, 3, 1, 1, False, False),      # C % 4 = 3, K < 64 (k_wg1), narrow weight-gradient stages
    (3, 18, 12, 20, 19, 3, 1, 1, True, False),       # C % 4 = 2 just above the Winograd minimum (16)
]


def _once(refs, key, make):
    """make() -- the oracle's answer for `key` -- computed once per `refs` dict (None: every time) and never modified."""
    if refs is None:
        return make()
    if key not in refs:
        refs[key] = make()
    return refs[key]


def conv_oracle(N, C, H, W, K, k, s, p, bias, pm, buf=PLAIN, refs=None):
    """refs: a dict that keeps the oracle's results of this row for the next run of it (under other library options)."""
    row = (N, C, H, W, K, k, s, p, bias, pm)
    g = torch.Generator().manual_seed(N * 1000 + C + K)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, k, k, generator=g) * (2.0 / (C * k * k)) ** 0.5
    b = torch.randn(K, generator=g) * 0.1 if bias else None
    pmv = torch.rand(K, C, k, k, generator=g) * 0.012 if pm else None
    layer = nl.SharableConv2d(C, K, k, stride=s, padding=p, bias=bias).to(DEV)
    layer.weight.data.copy_(w)
    if bias:
        layer.bias.data.copy_(b)
    if pm:
        layer.piggymask = nn.Parameter(pmv.to(DEV))
    buf.rehome(layer)
    xd = buf.put(x).requires_grad_(True)
    y = layer(xd)
    want = _once(refs, ('y',) + row, lambda: ops.conv2d_forward(x.numpy(), w.numpy(), None if pmv is None else pmv.numpy(),
                                                                None if b is None else b.numpy(), s, p))
    close(y, want, rtol=1e-4, atol=2e-5, msg='y')
    gy = torch.randn(y.shape, generator=g)
    y.backward(buf.put(gy))
    r = _once(refs, ('grads',) + row, lambda: ops.conv2d_backward(x.numpy(), w.numpy(), gy.numpy(), None if pmv is None else pmv.numpy(),
                                                                  bias, s, p))
    scale = float(np.abs(r['gw']).max())
    close(xd.grad, r['gx'], rtol=1e-4, atol=2e-5, msg='gx')
    close(layer.weight.grad, r['gw'], rtol=1e-4, atol=1e-5 * max(scale, 1.0), msg='gw')
    outs = [y, xd.grad, layer.weight.grad]
    if pm:
        close(layer.piggymask.grad, r['gpm'], rtol=1e-4, atol=1e-5 * max(scale, 1.0), msg='gpm')
        outs.append(layer.piggymask.grad)
    if bias:
        close(layer.bias.grad, r['gb'], rtol=1e-4, atol=1e-3, msg='gb')
        outs.append(layer.bias.grad)
    return outs


GROUPED_CONV_CASES = [
    (3, 32, 64, 14, 14, 3, 1, 1, 4, False, True),      # ResNeXt-style 3x3: 4 groups of 8 -> 16 channels (generic kernels: < 16 channels a group)
    (2, 64, 64, 12, 12, 3, 1, 1, 2, True, False),      # two groups of 32 -> 32 (Winograd kernels per group), bias
    (2, 32, 32, 9, 9, 1, 1, 0, 4, True, True),         # grouped pointwise
    (2, 48, 96, 10, 10, 3, 2, 1, 3, False, False),     # strided, 3 groups
]


def grouped_conv_vs_oracle(N, C, K, H, W, k, s, p, G, bias, pm, buf=PLAIN):
    g = torch.Generator().manual_seed(N + C + K + G)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C // G, k, k, generator=g) * 0.2
    b = torch.randn(K, generator=g) * 0.1 if bias else None
    pmv = torch.rand(K, C // G, k, k, generator=g) * 0.012 if pm else None
    layer = nl.SharableConv2d(C, K, k, stride=s, padding=p, groups=G, bias=bias).to(DEV)
    layer.weight.data.copy_(w)
    if bias:
        layer.bias.data.copy_(b)
    if pm:
        layer.piggymask = nn.Parameter(pmv.to(DEV))
    buf.rehome(layer)
    xd = buf.put(x).requires_grad_(True)
    y = layer(xd)
    want = ops.conv2d_forward(x.numpy(), w.numpy(), None if pmv is None else pmv.numpy(), None if b is None else b.numpy(), s, p, 1, G)
    close(y, want, rtol=1e-4, atol=2e-5, msg='y')
    gy = torch.randn(y.shape, generator=g)
    y.backward(buf.put(gy))
    r = ops.conv2d_backward(x.numpy(), w.numpy(), gy.numpy(), None if pmv is None else pmv.numpy(), bias, s, p, 1, G)
    scale = float(np.abs(r['gw']).max())
    close(xd.grad, r['gx'], rtol=1e-4, atol=2e-5, msg='gx')
    close(layer.weight.grad, r['gw'], rtol=1e-4, atol=1e-5 * max(scale, 1.0), msg='gw')
    outs = [y, xd.grad, layer.weight.grad]
    if pm:
        close(layer.piggymask.grad, r['gpm'], rtol=1e-4, atol=1e-5 * max(scale, 1.0), msg='gpm')
        outs.append(layer.piggymask.grad)
    if bias:
        close(layer.bias.grad, r['gb'], rtol=1e-4, atol=1e-3, msg='gb')
        outs.append(layer.bias.grad)
    with torch.no_grad():
        y2, st = layer.forward_with_bn_stats(buf.put(x))
    assert st is None and torch.equal(y2, y.detach())
    return outs + [y2]


LINEAR_ORACLE_CASES = [(32, 25088, 512, False), (256, 4096, 4096, True), (7, 513, 129, True), (1, 64, 5, False),
                       (256, 4096, 4096, False), (100, 1024, 256, False), (48, 260, 384, False),
                       # features.45 of config 2 at its own shape (89 % of all masked weights), both mask modes,
                       # and at the per-GPU batch of the 8-GPU reference configuration / the validate batch
                       (256, 25088, 4096, False), (256, 25088, 4096, True), (32, 25088, 4096, True), (100, 25088, 4096, False),
                       # the grown network's FC layers (raw multiplier 1.5: 627 * 49 -> int(4096 * sqrt(1.5)) = 5016; odd row length)
                       (32, 30723, 5016, True), (16, 5016, 5016, False),
                       # <= 64 rows (the reference's own 256 / 8 split): the weight-streaming input gradient and the 32- / 64-row forward
                       # tiles -- ragged column tiles, row counts that leave waves without work, one and two row fragments
                       (32, 25088, 4096, False), (64, 4096, 4096, True), (33, 4100, 1000, False), (8, 132, 18, True), (64, 1028, 50, False)]


def linear_oracle(B, I, O, pm, buf=PLAIN):
    g = torch.Generator().manual_seed(B + I + O)
    x = torch.randn(B, I, generator=g)
    w = torch.randn(O, I, generator=g) * I ** -0.5
    b = torch.randn(O, generator=g) * 0.1
    pmv = torch.rand(O, I, generator=g) * 0.012 if pm else None
    layer = nl.SharableLinear(I, O).to(DEV)
    layer.weight.data.copy_(w)
    layer.bias.data.copy_(b)
    if pm:
        layer.piggymask = nn.Parameter(pmv.to(DEV))
    buf.rehome(layer)
    xd = buf.put(x).requires_grad_(True)
    y = layer(xd)
    close(y, ops.linear_forward(x.numpy(), w.numpy(), None if pmv is None else pmv.numpy(), b.numpy()), rtol=1e-4, atol=2e-5)
    gy = torch.randn(B, O, generator=g)
    y.backward(buf.put(gy))
    r = ops.linear_backward(x.numpy(), w.numpy(), gy.numpy(), None if pmv is None else pmv.numpy())
    # absolute floor = 1e-5 of the tensor's scale: an element that is a near-cancelling sum of B (or I) terms carries the
    # round-off of its addends, not of its own magnitude
    def floor(a):
        return max(2e-5, 1e-5 * float(np.abs(a).max()))
    close(xd.grad, r['gx'], rtol=1e-4, atol=floor(r['gx']), msg='gx')
    close(layer.weight.grad, r['gw'], rtol=1e-4, atol=floor(r['gw']), msg='gw')
    close(layer.bias.grad, r['gb'], rtol=1e-4, atol=1e-4, msg='gb')
    outs = [y, xd.grad, layer.weight.grad, layer.bias.grad]
    if pm:
        close(layer.piggymask.grad, r['gpm'], rtol=1e-4, atol=floor(r['gpm']), msg='gpm')
        outs.append(layer.piggymask.grad)
    return outs


LINEAR_SMALL_BATCH_SEEDS = range(12)


def linear_small_batch_random_shapes(seed, buf=PLAIN):
    rs = np.random.RandomState(1000 + seed)
    B, I, O, pm_on = int(rs.randint(1, 65)), 4 * int(rs.randint(1, 700)), int(rs.randint(1, 900)), bool(seed % 2)
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = buf.put(torch.randn(B, I, generator=g, device=DEV)).requires_grad_(True)
    w = torch.randn(O, I, generator=g, device=DEV) * I ** -0.5
    gy = buf.put(torch.randn(B, O, generator=g, device=DEV))
    layer = nl.SharableLinear(I, O).to(DEV)
    layer.weight.data.copy_(w)
    layer.bias.data.zero_()
    keep = 1.0
    if pm_on:
        pm = torch.rand(O, I, generator=g, device=DEV) * 0.012
        layer.piggymask = nn.Parameter(pm.clone())
        keep = (pm > 5e-3).double()
    buf.rehome(layer)
    y = layer(x)
    y.backward(gy)
    weff = w.double() * keep
    gweff = gy.double().t() @ x.detach().double()
    checks = [(y.detach(), x.detach().double() @ weff.t(), 'y'), (x.grad, gy.double() @ weff, 'gx'), (layer.weight.grad, gweff * keep, 'gw')]
    if pm_on:
        checks.append((layer.piggymask.grad, gweff * w.double(), 'gpm'))
    for got, want, name in checks:
        sc = max(float(want.abs().max()), 1e-30)
        assert float((got.double() - want).abs().max()) <= 1e-5 * sc, (name, B, I, O, pm_on)
    return [c[0] for c in checks]


# --------------------------------------------------------------------------- fused stem conv -> BatchNorm -> ReLU
FUSED_STEM_K = [64, 78, 65, 96]       # 64 = the width-1.0 stem; 78 = the grown VGG16's (int(64 sqrt(1.5)): three blocks, the last partial), 65 / 96 its extremes
FUSED_STEM_SHAPES = [(3, 3, 40, 70, False), (2, 3, 224, 224, True), (5, 1, 17, 33, False), (4, 2, 64, 64, True)]


def fused_stem_conv_bn_relu_matches_unfused(N, C, H, W, pm, wgrad_in_pass, K, monkeypatch, buf=PLAIN):
    from cpg_amd.models import fused_bn as fb
    monkeypatch.setattr(fb, 'FUSE_STEM_WGRAD', wgrad_in_pass)      # the weight gradient inside the apply pass, or gy written + cpg_conv2d_wgrad
    g = torch.Generator().manual_seed(7 * N + H)
    x = torch.randn(N, C, H, W, generator=g)
    w0 = torch.randn(K, C, 3, 3, generator=g) * 0.3
    pm0 = torch.rand(K, C, 3, 3, generator=g) * 0.012 if pm else None
    gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.2
    gz = torch.randn(N, K, H, W, generator=g)
    res = {}
    for fused in (True, False):
        seq = fb.FusedSequential(nl.SharableConv2d(C, K, 3, padding=1, bias=False), nn.BatchNorm2d(K), nn.ReLU(inplace=True)).to(DEV)
        seq[0].weight.data.copy_(w0)
        if pm:
            seq[0].piggymask = nn.Parameter(pm0.clone().to(DEV))
        seq[1].weight.data.copy_(gam)
        seq[1].bias.data.copy_(bet)
        seq.train()
        buf.rehome(seq)
        old = fb.FUSE_STEM
        fb.FUSE_STEM = fused
        try:
            z = seq(buf.put(x))
            z.backward(buf.put(gz))
        finally:
            fb.FUSE_STEM = old
        res[fused] = [z.detach().clone(), seq[0].weight.grad.clone(), seq[1].weight.grad.clone(), seq[1].bias.grad.clone(),
                      seq[1].running_mean.clone(), seq[1].running_var.clone(), seq[1].num_batches_tracked.clone()]
        if pm:
            res[fused].append(seq[0].piggymask.grad.clone())
        if fused:
            assert type(z.grad_fn).__name__ == '_StemConvBnReluFnBackward', type(z.grad_fn).__name__     # the fused path really ran
            outs = [z.detach(), seq[0].weight.grad, seq[1].weight.grad, seq[1].bias.grad] + ([seq[0].piggymask.grad] if pm else [])
    for a, b in zip(res[True], res[False]):
        sc = float(b.double().abs().max()) + 1e-12
        assert float((a.double() - b.double()).abs().max()) <= 2e-5 * sc, (float((a.double() - b.double()).abs().max()), sc)
    assert torch.equal(res[True][0], res[False][0])                # same statistics tiles, same arithmetic: the output is bit-identical
    # fp64 torch reference of the whole triple
    xd = x.double().to(DEV)
    weff = (w0 * ((pm0 > 5e-3).float() if pm else 1.0)).double().to(DEV).requires_grad_(True)
    gd, bd = gam.double().to(DEV).requires_grad_(True), bet.double().to(DEV).requires_grad_(True)
    zr = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.conv2d(xd, weff, padding=1), None, None, gd, bd, True, 0.1, 1e-5))
    zr.backward(gz.double().to(DEV))
    assert float((res[True][0].double() - zr.detach()).abs().max()) <= 2e-5 * float(zr.detach().abs().max())
    gw_ref = weff.grad * ((pm0 > 5e-3).double().to(DEV) if pm else 1.0)
    for got, want in ((res[True][1], gw_ref), (res[True][2], gd.grad), (res[True][3], bd.grad)):
        assert float((got.double() - want).abs().max()) <= 1e-4 * (float(want.abs().max()) + 1e-9)
    return outs


# --------------------------------------------------------------------------- Winograd tail pieces
WINOGRAD_TAIL_CASES = [(256, 256, 256, 14, True),      # SphereNet-20 conv3_x: 784 four-wave blocks = 3.06 rounds (16 left: 16 pieces each)
                       (256, 512, 512, 14, False),     # VGG16 features.34: 6.125 rounds (32 blocks left: 8 pieces)
                       (200, 192, 192, 14, True),      # two-wave blocks (three 64-channel blocks): 921 blocks = 1.8 rounds -> no tail
                       (29, 250, 192, 28, True),       # two-wave blocks, 534 = 1.04 rounds; ragged channels (250 read: the last chunk overlaps)
                       (11, 96, 128, 56, False)]       # 270 four-wave blocks; the tail starts in the middle of image 10


def winograd_tail_pieces_equal_the_single_launch(N, C, K, H, bias, libopt, buf=PLAIN):
    g = torch.Generator(device=DEV).manual_seed(N + C + K + H)
    x = torch.randn(N, C, H, H, generator=g, device=DEV)
    w = torch.randn(K, C, 3, 3, generator=g, device=DEV) * (2.0 / (C * 9)) ** 0.5
    b = torch.randn(K, generator=g, device=DEV) * 0.1 if bias else None
    gy = torch.randn(N, K, H, H, generator=g, device=DEV)
    layer = nl.SharableConv2d(C, K, 3, padding=1, bias=bias).to(DEV)
    layer.weight.data.copy_(w)
    if bias:
        layer.bias.data.copy_(b)
    buf.rehome(layer)
    gyd = buf.put(gy)
    outs = []

    def run():
        xd = buf.put(x.clone()).requires_grad_(True)
        y = layer(xd)
        y.backward(gyd)
        outs[:] = [y, xd.grad]
        return y.detach().clone(), xd.grad.clone()
    y1, gx1 = run()
    y1b, gx1b = run()
    kept = list(outs)                                                      # of a run with the tail pieces
    assert torch.equal(y1, y1b) and torch.equal(gx1, gx1b)                 # fixed-order sum of the pieces
    libopt.set('CPG_WINO_TAIL', 0)
    y0, gx0 = run()
    libopt.set('CPG_WINO_TAIL', None)
    has_tail = (N, C, K, H) != (200, 192, 192, 14)                         # (1.8 rounds: the leftover is more than half a round -- one launch)
    for a, ref in ((y1, y0), (gx1, gx0)):
        sc = float(ref.abs().max())
        assert float((a - ref).abs().max()) <= 2e-6 * sc
    if not has_tail:
        assert torch.equal(y1, y0) and torch.equal(gx1, gx0)
    else:
        # another association of the channel sum: the tail really ran (in the forward, the input gradient or both: they are planned apart)
        assert not (torch.equal(y1, y0) and torch.equal(gx1, gx0))
        head = max(1, N // 2)
        assert torch.equal(y1[:head], y0[:head]) and torch.equal(gx1[:head], gx0[:head])       # the full rounds are untouched
    if not bias:
        # ... and the forward WITH the BatchNorm statistics epilogue: the tail's statistics come from k_wg_tail_reduce<true>
        xs = buf.put(x)
        with torch.no_grad():
            ys1, st1 = layer.forward_with_bn_stats(xs)
            ys1b, st1b = layer.forward_with_bn_stats(xs)
            libopt.set('CPG_WINO_TAIL', 0)
            ys0, st0 = layer.forward_with_bn_stats(xs)
            libopt.set('CPG_WINO_TAIL', None)
        assert torch.equal(ys1, ys1b) and torch.equal(st1, st1b) and st1.shape == st0.shape
        assert float((ys1 - ys0).abs().max()) <= 2e-6 * float(ys0.abs().max())
        # per channel: sum and sum of squares over all statistics tiles (the tiles' own sums differ in association only)
        t1, t0 = st1.double().sum(1), st0.double().sum(1)
        assert float((t1 - t0).abs().max()) <= 1e-5 * float(t0.abs().max())
        want = torch.stack([ys0.double().sum((0, 2, 3)), (ys0.double() ** 2).sum((0, 2, 3))], 1)
        assert float((t1 - want).abs().max()) <= 1e-5 * float(want.abs().max())
        assert float((st1 - st0).abs().max()) <= 1e-4 * float(st0.abs().max())
        kept += [ys1, st1]
    rs = np.random.RandomState(N + H)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1)).double()
    gyp = torch.nn.functional.pad(gy, (1, 1, 1, 1)).double()
    wd = w.double()
    for _ in range(24):
        n, k, c = N - 1 - rs.randint(min(N, 3)), rs.randint(K), rs.randint(C)
        h, ww = rs.randint(H), rs.randint(H)
        want = float((xp[n, :, h:h + 3, ww:ww + 3] * wd[k]).sum()) + (float(b[k]) if bias else 0.0)
        assert abs(float(y1[n, k, h, ww]) - want) <= 1e-4 * abs(want) + 2e-5
        want = float((gyp[n, :, h:h + 3, ww:ww + 3].flip(-1, -2) * wd[:, c]).sum())
        assert abs(float(gx1[n, c, h, ww]) - want) <= 1e-4 * abs(want) + 2e-5
    return kept


def winograd_tail_degrades_to_the_single_launch(libopt, buf=PLAIN):
    """cpg_conv2d_fwd of (11, 96, 128, 56 x 56) through the raw C ABI: 270 four-wave blocks against 256 slots -- 14 blocks left, 12 pieces each,
    a 19.3 MB tail.  (a) the workspace cpg_conv2d_workspace_bytes asks for, (b) the same under CPG_WINO_TAIL=0, (c) a workspace of exactly
    cpg_conv2d_pack_bytes(d, 0) bytes under the default options: room for the packed filter, none for the tail pieces."""
    from cpg_amd import _lib as L
    lib = L.lib()
    N, C, K, H = 11, 96, 128, 56
    assert (N, C, K, H, False) in WINOGRAD_TAIL_CASES
    g = torch.Generator(device=DEV).manual_seed(N + C + K + H)
    x = buf.put(torch.randn(N, C, H, H, generator=g, device=DEV))
    w = buf.put(torch.randn(K, C, 3, 3, generator=g, device=DEV) * (2.0 / (C * 9)) ** 0.5)
    d = L.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, H, K, 3, 3
    d.stride_h = d.stride_w = d.pad_h = d.pad_w = d.dil_h = d.dil_w = d.groups = 1
    full, packed = int(lib.cpg_conv2d_workspace_bytes(ctypes.byref(d))), int(lib.cpg_conv2d_pack_bytes(ctypes.byref(d), 0))
    assert lib.cpg_conv2d_winograd(ctypes.byref(d), 0) == 1 and 0 < packed < full

    def fwd(nbytes):
        ws, nb = L.workspace(nbytes, x.device)
        assert nbytes <= nb < nbytes + 4
        y = buf.empty((N, K, H, H))
        rc = lib.cpg_conv2d_fwd(ctypes.byref(d), L.dptr(x), L.dptr(w), None, 0.0, None, L.dptr(y), L.dptr(ws), nbytes, L.stream_ptr())
        return rc, y
    rc_a, a = fwd(full)
    libopt.set('CPG_WINO_TAIL', 0)
    rc_b, b = fwd(full)
    libopt.set('CPG_WINO_TAIL', None)
    rc_c, c = fwd(packed)
    assert (rc_a, rc_b, rc_c) == (L.CPG_OK, L.CPG_OK, L.CPG_OK), lib.cpg_last_error()
    assert torch.equal(c, b)                       # no room for the pieces: the single launch, bit for bit
    assert not torch.equal(a, b)                   # another association of the channel sum: the tail really ran in (a)
    assert torch.equal(a[:5], b[:5])               # the full rounds are untouched
    return [a, b, c]


# --------------------------------------------------------------------------- fused BatchNorm -> ReLU
BN_RELU_SHAPES = [(8, 64, 56, 56), (4, 16, 224, 224), (16, 512, 14, 14), (3, 5, 7, 9), (2, 3, 1, 1),
                  # planes of >= 16 * 256 items that are no multiple of 4: the scalar large-plane walk, and with 129 x 129 its 16-trip flush
                  (2, 3, 65, 65), (1, 2, 129, 129)]


def bn_relu_cases():
    """(training, N, C, H, W, misaligned), with the ids of the two stacked parametrize decorators these cases grew out of."""
    cases = [(t,) + s + (False,) for s in BN_RELU_SHAPES for t in (True, False)]
    # one slice of >= 64 * 256 items of planes under 4096 items: the 64-visit flush of the flattened small-plane walk (134 MB a tensor)
    cases.append((True, 34, 2048, 21, 23, False))
    # input and incoming gradient 4 bytes off a 16-byte boundary: the scalar paths of apply, reduce and backward-apply at 4 | HW
    cases += [(t, 2, 3, 8, 8, True) for t in (True, False)]
    return [pytest.param(*c, id='%s-%d-%d-%d-%d' % c[:5] + ('-misaligned' if c[5] else '')) for c in cases]


def _bn_pair(C, training):
    ref_bn, bn = nn.BatchNorm2d(C).to(DEV), nn.BatchNorm2d(C).to(DEV)
    for m in (ref_bn, bn):
        m.weight.data.copy_(torch.linspace(0.5, 1.5, C))
        m.bias.data.copy_(torch.linspace(-0.3, 0.3, C))
        m.running_mean.copy_(torch.linspace(-0.1, 0.1, C))
        m.running_var.copy_(torch.linspace(0.8, 1.2, C))
        m.train(training)
    return ref_bn, bn


def fused_bn_relu_matches_torch(N, C, H, W, training, misaligned, buf=PLAIN):
    from cpg_amd.models.fused_bn import bn_relu
    g = torch.Generator().manual_seed(N * C + H)
    x = (torch.randn(N, C, H, W, generator=g) * 2.0 + 0.5)
    gy = torch.randn(N, C, H, W, generator=g)
    place = (lambda t: buf.put(t, 1)) if misaligned else buf.put
    ref_bn, bn = _bn_pair(C, training)
    if N * H * W == 1 and training:
        pytest.skip('torch rejects a single value per channel in training mode')
    buf.rehome(bn, const_buffers=not training)
    xr = x.to(DEV).requires_grad_(True)
    xf = place(x).requires_grad_(True)
    with torch.backends.cudnn.flags(enabled=False):
        yr = torch.relu(ref_bn(xr))
    yf = bn_relu(xf, bn, relu=True)
    close(yf, yr.detach().cpu().numpy(), rtol=1e-4, atol=1e-5, msg='y')
    yr.backward(gy.to(DEV))
    yf.backward(place(gy))
    gscale = float(xr.grad.abs().max()) + 1e-12
    close(xf.grad, xr.grad.cpu().numpy(), rtol=1e-3, atol=2e-5 * max(1.0, gscale), msg='gx')
    close(bn.weight.grad, ref_bn.weight.grad.cpu().numpy(), rtol=1e-3, atol=1e-3, msg='dgamma')
    close(bn.bias.grad, ref_bn.bias.grad.cpu().numpy(), rtol=1e-3, atol=1e-3, msg='dbeta')
    close(bn.running_mean, ref_bn.running_mean.cpu().numpy(), rtol=1e-5, atol=1e-6, msg='running_mean')
    close(bn.running_var, ref_bn.running_var.cpu().numpy(), rtol=1e-5, atol=1e-6, msg='running_var')
    assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked)
    return [yf, xf.grad, bn.weight.grad, bn.bias.grad]


# (block-per-plane, wave-per-plane and the flattened small-plane walk of the backward passes)
BN_RELU_POOL_SHAPES = [(4, 64, 56, 56), (2, 16, 224, 224), (8, 512, 14, 14), (3, 5, 6, 10), (2, 3, 2, 2), (2, 8, 112, 112),
                       (3, 7, 28, 28), (2, 5, 4, 8), (1, 2, 2, 4),
                       # 16 384 windows a plane: the 16-trip flush inside the large-plane walk of the reduction
                       (1, 2, 256, 256)]


def fused_bn_relu_pool_matches_torch(N, C, H, W, training, buf=PLAIN):
    from cpg_amd.models.fused_bn import bn_relu_pool
    g = torch.Generator().manual_seed(N * C + H + 1)
    x = (torch.randn(N, C, H, W, generator=g) * 2.0 + 0.3)
    gy = torch.randn(N, C, H // 2, W // 2, generator=g)
    ref_bn, bn = _bn_pair(C, training)
    buf.rehome(bn, const_buffers=not training)
    xr = x.to(DEV).requires_grad_(True)
    xf = buf.put(x).requires_grad_(True)
    yr = nn.functional.max_pool2d(torch.relu(ref_bn(xr)), 2, 2)
    yf = bn_relu_pool(xf, bn)
    close(yf, yr.detach().cpu().numpy(), rtol=1e-4, atol=1e-5, msg='y')
    yr.backward(gy.to(DEV))
    yf.backward(buf.put(gy))
    gscale = float(xr.grad.abs().max()) + 1e-12
    close(xf.grad, xr.grad.cpu().numpy(), rtol=1e-3, atol=2e-5 * max(1.0, gscale), msg='gx')
    close(bn.weight.grad, ref_bn.weight.grad.cpu().numpy(), rtol=1e-3, atol=1e-3, msg='dgamma')
    close(bn.bias.grad, ref_bn.bias.grad.cpu().numpy(), rtol=1e-3, atol=1e-3, msg='dbeta')
    close(bn.running_mean, ref_bn.running_mean.cpu().numpy(), rtol=1e-5, atol=1e-6, msg='running_mean')
    close(bn.running_var, ref_bn.running_var.cpu().numpy(), rtol=1e-5, atol=1e-6, msg='running_var')
    return [yf, xf.grad, bn.weight.grad, bn.bias.grad]


BN_RELU_POOL3_SHAPES = [(4, 16, 56, 56), (2, 64, 112, 112), (3, 5, 7, 9), (2, 3, 1, 1), (2, 8, 16, 15)]


def fused_bn_relu_pool3_matches_torch(N, C, H, W, training, buf=PLAIN):
    from cpg_amd.models import fused_bn
    torch.manual_seed(N + C + H)
    bn_a, bn_b = nn.BatchNorm2d(C).to(DEV), nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn_a.weight.uniform_(0.5, 1.5)
        bn_a.bias.uniform_(-0.5, 0.5)
        bn_a.running_mean.normal_(0, 0.3)
        bn_a.running_var.uniform_(0.5, 2.0)
    bn_b.load_state_dict(bn_a.state_dict())
    bn_a.train(training)
    bn_b.train(training)
    buf.rehome(bn_a, const_buffers=not training)
    pool, relu = nn.MaxPool2d(3, 2, 1), nn.ReLU(inplace=True)
    x0 = torch.randn(N, C, H, W, device=DEV) * 1.5 + 0.2
    xa, xb = buf.put(x0.clone()).requires_grad_(True), x0.clone().requires_grad_(True)
    assert fused_bn._is_pool3(pool)
    ya = fused_bn.conv_bn_act_pool(lambda t: t, bn_a, relu, pool, xa)
    assert ya.grad_fn is not None and 'Pool3' in type(ya.grad_fn).__name__
    yb = pool(relu(bn_b(xb)))
    np.testing.assert_allclose(ya.detach().cpu().numpy(), yb.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    gy = torch.randn_like(yb)
    ya.backward(buf.put(gy))
    yb.backward(gy)
    sc = float(xb.grad.abs().max()) + 1e-12
    np.testing.assert_allclose(xa.grad.cpu().numpy(), xb.grad.cpu().numpy(), rtol=1e-4, atol=2e-5 * sc + 2e-6)
    for pa, pb in ((bn_a.weight, bn_b.weight), (bn_a.bias, bn_b.bias)):
        sc = float(pb.grad.abs().max()) + 1e-12
        np.testing.assert_allclose(pa.grad.cpu().numpy(), pb.grad.cpu().numpy(), rtol=1e-4, atol=1e-5 * sc)
    np.testing.assert_allclose(bn_a.running_mean.cpu().numpy(), bn_b.running_mean.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bn_a.running_var.cpu().numpy(), bn_b.running_var.cpu().numpy(), rtol=1e-5, atol=1e-6)
    return [ya, xa.grad, bn_a.weight.grad, bn_a.bias.grad]


BN_SMALL_PLANES_CASES = [(4, 128, 4, 4, 1, 0), (4, 64, 4, 4, 1, 0), (4, 128, 2, 2, 1, 0), (4, 16, 16, 16, 1, 0),
                         (4, 32, 8, 8, 1, 0), (4, 256, 4, 4, 0, 0), (4, 256, 4, 4, 0, 1), (4, 512, 2, 2, 0, 1),
                         (8, 64, 56, 56, 1, 0)]


def fused_bn_small_planes_fp64(N, C, H, W, relu, add, buf=PLAIN):
    from cpg_amd.models import fused_bn
    g = torch.Generator().manual_seed(N * C + H + relu + 2 * add)
    x = torch.randn(N, C, H, W, generator=g) * 2 + torch.randn(1, C, 1, 1, generator=g)
    gy = torch.randn(N, C, H, W, generator=g)
    res = torch.randn(N, C, H, W, generator=g) if add else None
    bn = nn.BatchNorm2d(C)
    bn.weight.data = torch.rand(C, generator=g) + 0.5
    bn.bias.data = torch.randn(C, generator=g) * 0.3
    bn64 = nn.BatchNorm2d(C).double()
    bn64.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in bn.state_dict().items()})
    x64 = x.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True) if add else None
    y64 = bn64(x64)
    if add:
        y64 = y64 + r64
    if relu or add:
        y64 = torch.relu(y64)
    y64.backward(gy.double())
    bnd = buf.rehome(bn.to(DEV).train())
    xd = buf.put(x).requires_grad_(True)
    rd = buf.put(res).requires_grad_(True) if add else None
    act = nn.ReLU(inplace=True)
    yd = fused_bn.bn_add_act(bnd, act, xd, rd) if add else fused_bn.bn_act(bnd, act if relu else None, xd)
    yd.backward(buf.put(gy))

    def rel(a, b):
        return float((a.double().cpu() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))
    assert rel(yd.detach(), y64.detach()) < 1e-6
    assert rel(xd.grad, x64.grad) < 1e-6
    assert rel(bnd.weight.grad, bn64.weight.grad) < 1e-6 and rel(bnd.bias.grad, bn64.bias.grad) < 1e-6
    if add:
        assert rel(rd.grad, r64.grad) < 1e-6
    np.testing.assert_allclose(bnd.running_var.cpu().numpy(), bn64.running_var.float().numpy(), rtol=1e-5)
    return [yd, xd.grad, bnd.weight.grad, bnd.bias.grad] + ([rd.grad] if add else [])


BN_ADD_RELU_MASK_SHAPES = [(6, 24, 28, 28), (3, 16, 56, 56), (5, 8, 14, 14), (2, 8, 7, 7), (130, 4, 12, 20)]


def bn_add_relu_byte_mask_equals_reading_the_output(N, C, H, W, monkeypatch, buf=PLAIN):
    from cpg_amd.models import fused_bn
    g = torch.Generator().manual_seed(N * C + H)
    x = torch.randn(N, C, H, W, generator=g).to(DEV)
    res = torch.randn(N, C, H, W, generator=g).to(DEV)
    gy = buf.put(torch.randn(N, C, H, W, generator=g))
    outs = {}
    made = []
    for use_mask in (True, False):
        monkeypatch.setattr(fused_bn, 'RELU_BYTE_MASK', use_mask)
        bn = nn.BatchNorm2d(C).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C))
            bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
        buf.rehome(bn)
        xd, rd = buf.put(x.clone()).requires_grad_(True), buf.put(res.clone()).requires_grad_(True)
        y = fused_bn.bn_add_act(bn, nn.ReLU(), xd, rd)
        y.backward(gy)
        outs[use_mask] = (y.detach().clone(), xd.grad.clone(), rd.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone())
        made += [y, xd.grad, rd.grad, bn.weight.grad, bn.bias.grad]
    # output and masked gradient: exactly equal; the BatchNorm sums run through differently compiled copies of the same expression
    # (a select feeding a fused multiply-add): equal to the last bits
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][2], outs[False][2])
    for a, b in zip(outs[True], outs[False]):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    bn = nn.BatchNorm2d(C).to(DEV).train().double()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, C))
        bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
    yr = torch.relu(bn(x.double()) + res.double())
    assert float((outs[True][0].double() - yr).abs().max()) <= 2e-5 * float(yr.abs().max())
    # the residual's gradient is the masked gradient itself: exactly gy where the output is positive, exactly 0 elsewhere
    assert torch.equal(outs[True][2], torch.where(outs[True][0] > 0, gy, torch.zeros_like(gy)))
    return made


PRELU_BACKWARD_CASES = [(8, 64, 56, 56, False), (5, 12, 7, 9, False), (3, 16, 28, 28, True), (2, 3, 1, 1, False),
                        # a plane of >= 4096 items that is no multiple of 4: block-per-plane forward, scalar large-plane walk
                        (2, 3, 65, 65, False)]


def prelu_backward_matches_torch(N, C, H, W, shared, buf=PLAIN):
    from cpg_amd.models import fused_bn
    g = torch.Generator().manual_seed(N * 100 + C)
    x = torch.randn(N, C, H, W, generator=g).to(DEV)
    gy = buf.put(torch.randn(N, C, H, W, generator=g))
    mod = nn.PReLU(1 if shared else C).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) - 0.3)
    buf.rehome(mod)
    res0 = torch.randn(N, C, H, W, generator=g).to(DEV)
    made = []
    for with_res in (False, True):          # with_res: SphereNet's `x + relu(conv(y))` -- the residual add folded into the forward pass
        out = {}
        for enabled in (True, False):
            fused_bn.ENABLED = enabled
            try:
                xi = buf.put(x.clone()).requires_grad_(True)
                ri = buf.put(res0.clone()).requires_grad_(True)
                mod.zero_grad()
                y = fused_bn.prelu(mod, xi, res=ri if with_res else None)
                y.backward(gy)
            finally:
                fused_bn.ENABLED = True
            out[enabled] = (y.detach().cpu().numpy(), xi.grad.cpu().numpy(), mod.weight.grad.cpu().numpy(),
                            ri.grad.cpu().numpy() if with_res else None)
            if enabled:
                made += [y, xi.grad, mod.weight.grad]
        np.testing.assert_allclose(out[True][0], out[False][0], rtol=0, atol=0 if not with_res else 1e-6)
        np.testing.assert_array_equal(out[True][1], out[False][1])
        sc = float(np.abs(out[False][2]).max()) + 1e-12
        np.testing.assert_allclose(out[True][2], out[False][2], rtol=1e-4, atol=1e-5 * sc)
        if with_res:
            np.testing.assert_array_equal(out[True][3], out[False][3])
    return made


# --------------------------------------------------------------------------- pruner pieces
class TinyNet(nn.Module):
    def __init__(self, datasets):
        super().__init__()
        self.datasets = datasets
        self.conv = nl.SharableConv2d(3, 4, 3, padding=1, bias=False)
        self.fc = nl.SharableLinear(6, 5)


class Wrap(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.module = m

    def forward(self, x):
        return self.module(x)


def make_pruner(mode, datasets, dataset, owners, weights, begin=0, end=100, freq=10, initial=0.0, target=0.1, wd=4e-5,
                width=1.0, finetune_again=False, piggymasks=None):
    net = TinyNet(list(datasets)).to(DEV)
    net.conv.weight.data.copy_(T(weights['conv']))
    net.fc.weight.data.copy_(T(weights['fc']))
    net.fc.bias.data.zero_()
    if piggymasks is not None:
        net.conv.piggymask = nn.Parameter(T(piggymasks['conv']))
        net.fc.piggymask = nn.Parameter(T(piggymasks['fc']))
    model = Wrap(net)
    masks = {'module.conv': T(owners['conv'], torch.uint8), 'module.fc': T(owners['fc'], torch.uint8)}
    args = types.SimpleNamespace(mode=mode, dataset=dataset, finetune_again=finetune_again, target_sparsity=target,
                                 initial_sparsity=initial, pruning_frequency=freq, weight_decay=wd, network_width_multiplier=width)
    return SparsePruner(model, masks, args, begin, end, list(datasets).index(dataset) + 1), model, masks


MASK_KERNEL_SIZES = (1, 3, 5, 17, 255, 1025, 4099, 70001)


def mask_kernels_ragged_size_vs_oracle(n, buf=PLAIN):
    """One length through every elementwise kernel of the pruner (written in place: buf.copy, not buf.put)."""
    live = buf.copy
    g = torch.Generator().manual_seed(n)
    w = torch.randn(n, generator=g)
    gw = torch.randn(n, generator=g)
    gpm = torch.randn(n, generator=g)
    owner = torch.randint(0, 5, (n,), generator=g, dtype=torch.uint8)
    pm = torch.rand(n, generator=g) * 0.012
    conv = {'conv': w.numpy().reshape(1, 1, 1, n) * 0 if False else np.zeros((4, 3, 3, 3), np.float32), 'fc': np.zeros((5, 6), np.float32)}
    zo = {'conv': np.zeros((4, 3, 3, 3), np.uint8), 'fc': np.zeros((5, 6), np.uint8)}
    pruner, model, masks = make_pruner('finetune', ['a', 'b', 'c'], 'c', zo, conv)
    # swap the conv layer's tensors for 1-D ones of length n
    mod = model.module.conv
    mod.weight = nn.Parameter(live(w))
    mod.piggymask = nn.Parameter(live(pm))
    mod.weight.grad = live(gw)
    mod.piggymask.grad = live(gpm)
    model.module.fc.piggymask = nn.Parameter(torch.zeros(5, 6, device=DEV))
    masks['module.conv'] = live(owner)
    pruner.current_dataset_idx = 3
    pruner.do_weight_decay_and_make_grads_zero()
    wg, wp = ops.route_grads(gw.numpy(), w.numpy(), owner.numpy(), 3, 4e-5, gpm.numpy(), 'finetune')
    np.testing.assert_allclose(mod.weight.grad.cpu().numpy(), wg, rtol=3e-7, atol=0)
    np.testing.assert_array_equal(mod.piggymask.grad.cpu().numpy(), wp)
    owners = [owner.numpy(), zo['fc']]
    assert pruner.calculate_sparsity() == ops.sparsity(owners, 3)
    assert pruner.calculate_shared_part_ratio() == ops.shared_part_ratio(owners, [pm.numpy(), np.zeros((5, 6), np.float32)], 3)
    pruner.inference_dataset_idx = 2
    pruner.apply_mask()
    np.testing.assert_array_equal(mod.weight.data.cpu().numpy(), ops.apply_mask(w.numpy(), owner.numpy(), 2))
    pruner.current_dataset_idx = 3
    pruner.make_finetuning_mask()
    np.testing.assert_array_equal(masks['module.conv'].cpu().numpy(), ops.claim_free(owner.numpy(), 4))
    return [mod.weight.data, mod.piggymask.data, mod.weight.grad, mod.piggymask.grad, masks['module.conv']]


PACK_UNPACK_SIZES = [1, 3, 1023, 1024, 1025, 70_001, 3_000_001]


def gradient_pack_unpack_equals_boolean_indexing(n, select, buf=PLAIN):
    from cpg_amd import _lib as L
    lib = L.lib()
    g = torch.Generator().manual_seed(n + select)
    owner = buf.put(torch.randint(0, 4, (n,), generator=g, dtype=torch.uint8))
    grad = buf.put(torch.randn(n, generator=g))
    cur = 2
    sel = (owner == cur) if select == 0 else ((owner > 0) & (owner < cur))
    nblk = int(lib.cpg_owned_num_blocks(n))
    assert nblk == (n + 1023) // 1024
    counts = buf.empty((nblk,), torch.int32)
    s = L.stream_ptr()
    L.check('counts', lib.cpg_owned_block_counts(L.dptr(owner, torch.uint8), cur, select, n, ctypes.c_void_p(counts.data_ptr()), s))
    want_counts = torch.nn.functional.pad(sel.int(), (0, nblk * 1024 - n)).view(nblk, 1024).sum(1).int()
    assert torch.equal(counts, want_counts)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    offs = buf.put((ends - counts).contiguous())
    total = int(ends[-1])
    assert total == int(sel.sum())
    packed = buf.full((max(total, 1),), float('nan'))
    L.check('pack', lib.cpg_pack_owned(L.dptr(grad), L.dptr(owner, torch.uint8), cur, select, n, ctypes.c_void_p(offs.data_ptr()), L.dptr(packed), s))
    assert torch.equal(packed[:total], grad[sel])
    out = buf.full((n,), -7.0)
    L.check('unpack', lib.cpg_unpack_owned(L.dptr(buf.put(packed * 2)), L.dptr(owner, torch.uint8), cur, select, n, ctypes.c_void_p(offs.data_ptr()),
                                           L.dptr(out), s))
    assert torch.equal(out[sel], grad[sel] * 2) and bool((out[~sel] == -7.0).all())
    return [counts, packed, out]


def rank_prune_vs_oracle(w, owner, cur, ratio, buf=PLAIN, zero=False):
    """cpg_rank_prune (zero: cpg_rank_prune_zero, which also clears the released weights) through the raw C ABI against the oracle:
    owner bytes exact, k and the cutoff in the 32-byte result record.  w, owner: CPU tensors."""
    from cpg_amd import _lib as L
    lib, s = L.lib(), L.stream_ptr()
    n = w.numel()
    do = buf.copy(owner)
    dw = buf.copy(w) if zero else buf.put(w)
    res = buf.zeros((4,), torch.int64)
    ws, nb = L.workspace(lib.cpg_rank_prune_workspace_bytes(), DEV)
    fn = lib.cpg_rank_prune_zero if zero else lib.cpg_rank_prune
    assert fn(L.dptr(dw), L.dptr(do, torch.uint8), cur, ratio, n, ctypes.c_void_p(res.data_ptr()), L.dptr(ws), nb, s) == 0
    want, k, cutoff = ops.rank_prune(w.numpy(), owner.numpy(), cur, ratio)
    np.testing.assert_array_equal(do.cpu().numpy(), want)
    rec = L.PruneResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert rec.k == k and rec.cutoff == np.float32(cutoff) and rec.status == 0
    if zero:
        np.testing.assert_array_equal(dw.cpu().numpy(), ops.zero_pruned(w.numpy(), want))
    return [do, res, ws] + ([dw] if zero else [])
