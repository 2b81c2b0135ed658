"""The 2x2 window maxima of a conv output from the Winograd forward's epilogue (cpg_conv2d_fwd_attach_pool_max) and the pooled BatchNorm
passes that read them (cpg_bn_relu_pool_fwd_from_max / cpg_bn_relu_pool_bwd_from_max).

What must hold:
  conv        y and the statistics tiles are bit-equal with and without the attach; E is exactly amax over the windows of that y; a shape the
              query refuses (or a bias) makes an armed call fail with CPG_E_INVALID before anything is launched, and the arm does not
              survive that call.
  forward     the pooled output equals cpg_bn_relu_pool_fwd's elementwise as numbers (bn_affine is monotone in x, so for gamma > 0 the
              maximum commutes with it; gamma <= 0 planes read y as before), the running statistics and the counter are equal.
  backward    dbeta is bit-equal (the same terms in the same order); gx and dgamma are bit-equal unless two DIFFERENT values of a window
              round to the same BatchNorm output -- probability ~1e-7 per window for N(0,1) inputs, none for the seeds used here.  One
              constructed case forces such collisions and holds both paths to an fp64 reference.
  module      FusedSequential computes the same loss with the switch on and off, gradients within the parity bar."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from cpg_amd import _lib
from cpg_amd.models import fused_bn
from cpg_amd.models import layers as nl

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
THR = 0.005
EPS, MOM = 1e-5, 0.1
P = _lib.dptr

# (N, H, W) at C = 64: 45 tiles = one full run of 32 and a ragged one, both straddling images; runs that span several images
MAPS = [(5, 6, 6), (3, 8, 12), (2, 4, 4)]
# ... and one launch with more units than the chip holds at once, so that its last round runs as channel-split tail pieces whose window
# maxima come from the tail's reduction kernel (what the 28x28 and 14x14 layers of VGG16 do at batch 256): 18 000 tiles = 563 runs
TAIL_MAP = (5, 120, 120)


def _desc(N, C, H, W, K):
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, 3, 3
    d.stride_h = d.stride_w = d.pad_h = d.pad_w = d.dil_h = d.dil_w = d.groups = 1
    return d


def _conv_inputs(N, C, H, W, K, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * 0.05
    pm = torch.randn(K, C, 3, 3, generator=g) * 0.01 + THR
    return x.to(DEV), w.to(DEV), pm.to(DEV)


def _conv(d, x, w, pm, E=None, bias=None, expect=_lib.CPG_OK):
    """(y, stats) of cpg_conv2d_fwd_bnstats, with E attached when given; y and the statistics start out as NaN."""
    lib = _lib.lib()
    tiles = lib.cpg_conv2d_bnstats_tiles(ctypes.byref(d))
    assert tiles > 0
    y = torch.full((d.N, d.K, d.H, d.W), float('nan'), device=DEV)
    stats = torch.full((d.K, tiles, 2), float('nan'), device=DEV)
    ws, nb = _lib.workspace(lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    if E is not None:
        assert lib.cpg_conv2d_fwd_attach_pool_max(P(E), E.numel() * 4) == _lib.CPG_OK
    rc = lib.cpg_conv2d_fwd_bnstats(ctypes.byref(d), P(x), P(w), P(pm), THR, P(bias), P(y), P(stats), stats.numel() * 4, P(ws), nb,
                                    _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.cpg_last_error())
    return y, stats


@pytest.mark.parametrize('K', [64, 128])          # 64: blocks of one unit; 128: two units per block sharing the input transform
@pytest.mark.parametrize('N,H,W', MAPS + [TAIL_MAP])
def test_conv_writes_window_maxima(N, H, W, K):
    lib = _lib.lib()
    d = _desc(N, 64, H, W, K)
    assert lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(d)) == 1
    x, w, pm = _conv_inputs(N, 64, H, W, K, seed=11 + K + H)
    y0, s0 = _conv(d, x, w, pm)
    E = torch.full((N, K, H // 2, W // 2), float('nan'), device=DEV)
    y1, s1 = _conv(d, x, w, pm, E=E)
    assert not torch.isnan(y0).any() and not torch.isnan(s0).any()
    assert torch.equal(y1, y0) and torch.equal(s1, s0)
    assert torch.equal(E, F.max_pool2d(y0, 2, 2))
    assert torch.equal(E, y0.view(N, K, H // 2, 2, W // 2, 2).amax(dim=(3, 5)))


def test_refused_shapes_and_the_one_shot_arm():
    lib = _lib.lib()
    ok = _desc(2, 64, 4, 4, 64)
    refused = [_desc(2, 128, 7, 7, 64),          # odd map
               _desc(2, 64, 4, 4, 96),           # not whole 64-channel blocks
               _desc(2, 32, 4, 4, 64)]           # the one-wave kernel
    for d in refused:
        assert lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(d)) == 0
    with _lib.option('CPG_NO_POOL_MAX', 1):
        assert lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(ok)) == 0
    with _lib.option('CPG_WINO_KERNEL', 'wave'):
        assert lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(ok)) == 0
    with _lib.option('CPG_NO_WINO', 1):
        assert lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(ok)) == 0
    assert lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(ok)) == 1
    assert lib.cpg_conv2d_fwd_attach_pool_max(ctypes.c_void_p(1 << 20), 0) == _lib.CPG_E_INVALID
    assert lib.cpg_conv2d_fwd_attach_pool_max(None, 0) == _lib.CPG_OK                  # disarms

    sentinel = 7.0
    E = torch.full((2, 128, 4, 4), sentinel, device=DEV)          # (large enough for every shape below)
    x_ok, w_ok, pm_ok = _conv_inputs(2, 64, 4, 4, 64, seed=3)
    for d in refused:
        x, w, pm = _conv_inputs(d.N, d.C, d.H, d.W, d.K, seed=5)
        y, _ = _conv(d, x, w, pm, E=E, expect=_lib.CPG_E_INVALID)
        assert torch.isnan(y).all()                                # refused before anything was launched
        # the arm did not survive the failed call: the next, supported, call writes no maxima
        _conv(ok, x_ok, w_ok, pm_ok)
        assert (E == sentinel).all()
    # a bias
    bias = torch.zeros(64, device=DEV)
    y, _ = _conv(ok, x_ok, w_ok, pm_ok, E=E, bias=bias, expect=_lib.CPG_E_INVALID)
    assert torch.isnan(y).all()
    _conv(ok, x_ok, w_ok, pm_ok)
    assert (E == sentinel).all()
    # a buffer that is too small
    small = torch.full((2 * 64 * 2 * 2 - 1,), sentinel, device=DEV)
    _conv(ok, x_ok, w_ok, pm_ok, E=small, expect=_lib.CPG_E_INVALID)
    assert (small == sentinel).all()
    # ... and the arm is consumed by a successful call too
    Eok = torch.full((2, 64, 2, 2), sentinel, device=DEV)
    y, _ = _conv(ok, x_ok, w_ok, pm_ok, E=Eok)
    assert torch.equal(Eok, F.max_pool2d(y, 2, 2))
    Eok.fill_(sentinel)
    _conv(ok, x_ok, w_ok, pm_ok)
    assert (Eok == sentinel).all()


# ---------------------------------------------------------------------------------------------------------------- BatchNorm side
# (N, C, H, W): the three maps above; 49 windows per plane (no 16-byte rows of E); 1024 windows (a block per plane, planes walked
# flattened by the reduction); 4096 windows (planes walked image by image)
BN_SHAPES = [(5, 64, 6, 6), (3, 64, 8, 12), (2, 64, 4, 4), (2, 3, 14, 14), (2, 8, 64, 64), (2, 4, 128, 128)]


def _mixed_gamma(C, g):
    """positive, negative and exactly 0 in one launch"""
    gamma = torch.randn(C, generator=g).abs() + 0.25
    gamma[1::3] *= -1.0
    gamma[2::5] = 0.0
    return gamma


def _bn_case(N, C, H, W, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    y = torch.randn(N, C, H, W, generator=g)
    gamma, beta = _mixed_gamma(C, g), torch.randn(C, generator=g) * 0.3
    gp = torch.randn(N, C, H // 2, W // 2, generator=g)
    # statistics tiles as a conv would leave them: two tiles per channel, {sum, sum of squares} in fp32
    half = (N + 1) // 2
    parts = [y[:half], y[half:]]
    stats = torch.stack([torch.stack([p.sum(dim=(0, 2, 3)), (p * p).sum(dim=(0, 2, 3))], dim=1) for p in parts], dim=1).contiguous()
    y, gamma, beta, gp, stats = [t.to(DEV) for t in (y, gamma, beta, gp, stats)]
    E = F.max_pool2d(y, 2, 2).contiguous()
    return y, E, gamma, beta, gp, stats


def _pool_fwd(y, E, gamma, beta, stats, from_max):
    """(pooled, mean, invstd, running_mean, running_var, counter): finalize + apply, the old pair of calls or the one new call"""
    lib = _lib.lib()
    N, C, H, W = y.shape
    s = _lib.stream_ptr()
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rm, rv = torch.full((C,), 0.5, device=DEV), torch.full((C,), 2.0, device=DEV)
    nbt = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    out = torch.full((N, C, H // 2, W // 2), float('nan'), device=DEV)
    if from_max:
        _lib.call('cpg_bn_relu_pool_fwd_from_max', P(y), P(E), P(stats), stats.shape[1], P(gamma), P(beta), EPS, MOM, P(rm), P(rv),
                  P(nbt, torch.int64), P(mean), P(invstd), P(out), N, C, H, W, s)
    else:
        _lib.call('cpg_bn_stats_finalize_count', P(stats), stats.shape[1], N, C, H * W, EPS, MOM, P(rm), P(rv), P(mean), P(invstd),
                  P(nbt, torch.int64), s)
        _lib.call('cpg_bn_relu_pool_fwd', P(y), P(gamma), P(beta), EPS, MOM, None, None, P(mean), P(invstd), P(out), N, C, H, W, 0, None, 0, s)
    torch.cuda.synchronize()
    return out, mean, invstd, rm, rv, nbt


def _pool_bwd(y, E, gp, gamma, beta, mean, invstd, from_max):
    lib = _lib.lib()
    N, C, H, W = y.shape
    gx = torch.full_like(y, float('nan'))
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
    ws, nb = _lib.workspace(lib.cpg_bn_workspace_bytes(N, C, H * W), DEV)
    tail = (P(gp), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dgamma), P(dbeta), N, C, H, W, 1, P(ws), nb, _lib.stream_ptr())
    if from_max:
        _lib.call('cpg_bn_relu_pool_bwd_from_max', P(y), P(E), *tail)
    else:
        _lib.call('cpg_bn_relu_pool_bwd', P(y), *tail)
    torch.cuda.synchronize()
    return gx, dgamma, dbeta


@pytest.mark.parametrize('shape', BN_SHAPES)
def test_pooled_forward_from_max(shape):
    y, E, gamma, beta, gp, stats = _bn_case(*shape, seed=101 + shape[2])
    assert (gamma > 0).any() and (gamma < 0).any() and (gamma == 0).any()
    old = _pool_fwd(y, E, gamma, beta, stats, False)
    new = _pool_fwd(y, E, gamma, beta, stats, True)
    assert not torch.isnan(old[0]).any()
    assert bool((new[0] == old[0]).all())                         # as numbers: the sign of a zero is not told apart
    for a, b in zip(new[1:], old[1:]):
        assert torch.equal(a, b)
    assert int(new[5]) == 42


@pytest.mark.parametrize('shape', BN_SHAPES)
def test_pooled_backward_from_max(shape):
    y, E, gamma, beta, gp, stats = _bn_case(*shape, seed=211 + shape[2])
    _, mean, invstd, _, _, _ = _pool_fwd(y, E, gamma, beta, stats, False)
    gx0, dg0, db0 = _pool_bwd(y, E, gp, gamma, beta, mean, invstd, False)
    gx1, dg1, db1 = _pool_bwd(y, E, gp, gamma, beta, mean, invstd, True)
    assert not torch.isnan(gx0).any()
    assert torch.equal(db1, db0)
    assert torch.equal(dg1, dg0)
    assert torch.equal(gx1, gx0)


def test_attach_form_of_the_pooled_pair():
    """cpg_bn_relu_pool_attach_max + cpg_bn_relu_pool_fwd / _bwd is the _from_max pair (what the Python layer calls, so that the entry
    points of the pooled group keep their names); one-shot, and a buffer that is too small is refused."""
    lib = _lib.lib()
    N, C, H, W = shape = (3, 64, 8, 12)
    y, E, gamma, beta, gp, stats = _bn_case(*shape, seed=77)
    ref = _pool_fwd(y, E, gamma, beta, stats, True)
    mean, invstd = ref[1], ref[2]
    bwd_ref = _pool_bwd(y, E, gp, gamma, beta, mean, invstd, True)
    # a wrong E shows whether a call read it: all-zero maxima give relu(bn(0)) in every gamma > 0 plane
    zeros = torch.zeros_like(E)
    s = _lib.stream_ptr()

    def fwd(att):
        out = torch.full((N, C, H // 2, W // 2), float('nan'), device=DEV)
        if att is not None:
            assert lib.cpg_bn_relu_pool_attach_max(P(att), att.numel() * 4) == _lib.CPG_OK
        rc = lib.cpg_bn_relu_pool_fwd(P(y), P(gamma), P(beta), EPS, MOM, None, None, P(mean), P(invstd), P(out), N, C, H, W, 0, None, 0, s)
        torch.cuda.synchronize()
        return rc, out
    rc, out = fwd(E)
    assert rc == _lib.CPG_OK and torch.equal(out, ref[0])
    rc, out_z = fwd(zeros)
    assert rc == _lib.CPG_OK and not torch.equal(out_z, ref[0])            # the attached buffer is what the call read ...
    rc, out = fwd(None)
    assert rc == _lib.CPG_OK and bool((out == ref[0]).all())               # ... and the arm was used up by it
    assert lib.cpg_bn_relu_pool_attach_max(P(E), E.numel() * 4 - 4) == _lib.CPG_OK
    rc, out = fwd(None)
    assert rc == _lib.CPG_E_INVALID and torch.isnan(out).all()
    rc, out = fwd(None)
    assert rc == _lib.CPG_OK                                               # (disarmed by the refused call)
    assert lib.cpg_bn_relu_pool_attach_max(P(E), E.numel() * 4) == _lib.CPG_OK
    assert lib.cpg_bn_relu_pool_attach_max(None, 0) == _lib.CPG_OK         # disarms
    # backward
    gx = torch.full_like(y, float('nan'))
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
    ws, nb = _lib.workspace(lib.cpg_bn_workspace_bytes(N, C, H * W), DEV)
    assert lib.cpg_bn_relu_pool_attach_max(P(E), E.numel() * 4) == _lib.CPG_OK
    _lib.call('cpg_bn_relu_pool_bwd', P(y), P(gp), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dgamma), P(dbeta), N, C, H, W, 1, P(ws), nb, s)
    torch.cuda.synchronize()
    for a, b in zip((gx, dgamma, dbeta), bwd_ref):
        assert torch.equal(a, b)


def test_pooled_backward_value_ties_against_fp64():
    """Two different y of one window that round to the same BatchNorm output: the old reduction takes xhat of the first, the new one xhat
    of the larger.  Forced here by |gamma invstd| = 2^-6 against beta = 1: the outputs lie next to 1 with a spacing of 2^-23, i.e. 7.6e-6 in
    xhat, so neighbouring y collapse.  In every eighth window the maximum sits in the first element and its successor (one ulp up) in
    the last, the other two well below; a few windows of the random rest collapse on their own.  (gamma is a power of two so that xhat * gamma
    is exact and xhat * gamma + beta rounds once whether or not it is compiled to a fused multiply-add: the fp32 values below are the
    kernels'.)
    The reference is the backward formula in fp64 torch with the window's winner taken from those fp32 forward values, first maximum in
    row-major order, as torch's own fp32 max_pool2d routes -- in fp64 nothing would tie and the gradient would go to a different ELEMENT
    of such a window, which is not what either path (or torch in fp32) computes.
    Bar: test_hip_parity.close's, rtol 1e-4 and atol 1e-5 of the reference's scale, for both paths; an affected term of sum(g xhat) moves
    by at most the xhat distance of two collapsing values, 7.6e-6."""
    N, C, H, W = 4, 8, 32, 32
    g = torch.Generator(device='cpu').manual_seed(5)
    y = torch.randn(N, C, H, W, generator=g)
    yw = y.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4).clone()
    top = yw.max(dim=1).values[::8]
    yw[::8] = torch.stack([top, top - 1.0, top - 1.0, torch.nextafter(top, torch.full_like(top, float('inf')))], dim=1)
    y = yw.view(N, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H, W).contiguous()
    gamma = torch.full((C,), 2.0 ** -6)
    beta = torch.ones(C)
    gp = torch.randn(N, C, H // 2, W // 2, generator=g)
    var, mu = torch.var_mean(y.double(), dim=(0, 2, 3), unbiased=False)
    mean, invstd = mu.float(), torch.rsqrt(var + EPS).float()
    # the fp32 forward values and their routing
    a32 = (y - mean.view(1, C, 1, 1)) * invstd.view(1, C, 1, 1) * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)
    z32 = torch.relu(a32)
    _, idx = F.max_pool2d(z32, 2, 2, return_indices=True)
    win = a32.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    yw = y.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    top = win.max(dim=-1, keepdim=True).values
    tied = ((win == top) & (top > 0)).sum(dim=-1) > 1
    distinct = tied & (yw.masked_fill(win != top, float('-inf')).max(dim=-1).values != yw.masked_fill(win != top, float('inf')).min(dim=-1).values)
    print('windows whose maximum is shared by different y: %d of %d' % (int(distinct.sum()), distinct.numel()))
    assert int(distinct.sum()) >= distinct.numel() // 16
    # fp64 backward with that routing
    yd, gd, md, isd = y.double(), gamma.double().view(1, C, 1, 1), mean.double().view(1, C, 1, 1), invstd.double().view(1, C, 1, 1)
    pooled = torch.gather(z32.view(N, C, -1), 2, idx.view(N, C, -1)).view_as(gp)
    gz = torch.zeros(N, C, H * W, dtype=torch.float64).scatter_(2, idx.view(N, C, -1), (gp.double() * (pooled > 0)).view(N, C, -1)).view(N, C, H, W)
    xhat = (yd - md) * isd
    n = N * H * W
    dbeta_ref = gz.sum(dim=(0, 2, 3))
    dgamma_ref = (gz * xhat).sum(dim=(0, 2, 3))
    gx_ref = (gz - dbeta_ref.view(1, C, 1, 1) / n - xhat * dgamma_ref.view(1, C, 1, 1) / n) * isd * gd

    yg, gpg, gammag, betag, meang, invstdg = [t.to(DEV) for t in (y, gp, gamma, beta, mean, invstd)]
    E = F.max_pool2d(yg, 2, 2).contiguous()
    res = {name: _pool_bwd(yg, E, gpg, gammag, betag, meang, invstdg, fm) for name, fm in (('reads y', False), ('reads E', True))}

    def err(got, want):
        want = want.numpy()
        scale = float(np.abs(want).max())
        return float(np.abs(got.cpu().double().numpy() - want).max()) / scale, scale

    for name, (gx, dg, db) in res.items():
        print('%s: max error / scale: gx %.3g, dgamma %.3g, dbeta %.3g' % (name, err(gx, gx_ref)[0], err(dg, dgamma_ref)[0], err(db, dbeta_ref)[0]))
    for name, (gx, dg, db) in res.items():
        for what, got, want in (('gx', gx, gx_ref), ('dgamma', dg, dgamma_ref), ('dbeta', db, dbeta_ref)):
            scale = err(got, want)[1]
            np.testing.assert_allclose(got.cpu().double().numpy(), want.numpy(), rtol=1e-4, atol=1e-5 * scale, err_msg='%s: %s' % (name, what))
    assert torch.equal(res['reads E'][2], res['reads y'][2])


# ---------------------------------------------------------------------------------------------------------------- module level
def _stack(seed):
    torch.manual_seed(seed)
    net = fused_bn.FusedSequential(
        nl.SharableConv2d(64, 64, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
        nl.SharableConv2d(64, 64, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
        nn.MaxPool2d(2, 2)).to(DEV)
    with torch.no_grad():
        for m in (net[0], net[3]):
            m.weight.normal_(0.0, 0.05)
        net[4].weight.copy_(_mixed_gamma(64, torch.Generator(device='cpu').manual_seed(seed)).to(DEV))
        net[4].bias.normal_(0.0, 0.3)
    return net.train()


class _Calls(object):
    """counts the calls of the entry points that matter here"""
    names = ('cpg_conv2d_fwd_attach_pool_max', 'cpg_bn_relu_pool_attach_max', 'cpg_bn_relu_pool_fwd', 'cpg_bn_relu_pool_bwd')

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.names, 0)
        real = _lib.call

        def call(name, *args):
            if name in self.n:
                self.n[name] += 1
            return real(name, *args)
        monkeypatch.setattr(_lib, 'call', call)


def _step(net, x, target):
    for p in net.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    out = net(xin)
    loss = ((out - target) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    return [loss.detach(), out.detach(), xin.grad] + [p.grad for p in net.parameters()], [b.clone() for b in net.buffers()]


def test_fused_sequential_with_the_switch_on_and_off(monkeypatch):
    g = torch.Generator(device='cpu').manual_seed(9)
    x = torch.randn(5, 64, 6, 6, generator=g).to(DEV)
    target = torch.randn(5, 64, 3, 3, generator=g).to(DEV)
    calls = _Calls(monkeypatch)
    net = _stack(3)
    twin = copy.deepcopy(net)
    on, buf_on = _step(net, x, target)
    # (the module hands E to the pooled pair through the attach form: once for the forward, once for the backward)
    assert calls.n == {'cpg_conv2d_fwd_attach_pool_max': 1, 'cpg_bn_relu_pool_attach_max': 2, 'cpg_bn_relu_pool_fwd': 1, 'cpg_bn_relu_pool_bwd': 1}
    with _lib.option('CPG_NO_POOL_MAX', 1):
        off, buf_off = _step(twin, x, target)
    assert calls.n == {'cpg_conv2d_fwd_attach_pool_max': 1, 'cpg_bn_relu_pool_attach_max': 2, 'cpg_bn_relu_pool_fwd': 2, 'cpg_bn_relu_pool_bwd': 2}
    assert bool((on[0] == off[0]).all()) and bool((on[1] == off[1]).all())          # the loss and the output, as numbers
    for a, b in zip(buf_on, buf_off):
        assert torch.equal(a, b)
    for a, b in zip(on[2:], off[2:]):
        want = b.cpu().double().numpy()
        np.testing.assert_allclose(a.cpu().double().numpy(), want, rtol=1e-4, atol=1e-5 * max(float(np.abs(want).max()), 1.0))
