"""The BatchNorm -> ReLU backward apply pass riding in the Winograd weight-gradient kernel (cpg_conv2d_wgrad_attach_bn_bwd): the rider's
gy must be the standalone pass's bit for bit (one shared device function), the hosting weight gradient must not change, a whole training
step must come out the same with the rider on and off, and a descriptor the query refuses must take the standalone path.

Comparisons are on the BIT patterns (int32 views) of everything that is not a NaN -- stricter than torch.equal: -0.0 is not 0.0 --
and NaNs must sit at the same places (torch.equal itself is False for any tensor that holds one, even against itself; a NaN's sign and
payload depend on which instruction of the same expression met it first, e.g. a packed fma with a negated operand against a subtract,
and carry no information)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

from conftest import ROOT

from cpg_amd import _lib
from cpg_amd.models import fused_bn
from cpg_amd.models import layers as nl

DEV = 'cuda:0'
THR = 0.005


def _desc(N, C, H, W, K):
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, 3, 3
    d.stride_h = d.stride_w = d.pad_h = d.pad_w = d.dil_h = d.dil_w = d.groups = 1
    return d


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    keep = ~torch.isnan(a)
    return torch.equal(_bits(a)[keep], _bits(b)[keep])


def test_rider_query_and_switch_on_the_host():
    """The query needs no GPU: the GS = 4 shapes say yes, shapes whose blocks are not four whole waves of one input-channel block and the
    direct kernels say no, CPG_NO_WW_RIDER turns every answer to no; attach checks its arguments and disarms on NULL."""
    lib = _lib.lib()
    yes = [(2, 128, 112, 112, 128), (2, 256, 56, 56, 256), (2, 512, 28, 28, 512), (2, 512, 14, 14, 512), (3, 64, 14, 14, 128)]
    no = [(2, 64, 28, 28, 96),          # three output-channel blocks: the last block of the launch would have idle waves
          (2, 64, 28, 28, 64),          # two output-channel blocks: pairs share (GS = 2)
          (2, 64, 30, 30, 128),         # not a Winograd weight-gradient shape
          (2, 3, 28, 28, 128)]
    for s in yes:
        assert lib.cpg_conv2d_wgrad_rider_supported(ctypes.byref(_desc(*s))) == 1, s
    for s in no:
        assert lib.cpg_conv2d_wgrad_rider_supported(ctypes.byref(_desc(*s))) == 0, s
    with _lib.option('CPG_NO_WW_RIDER', 1):
        for s in yes:
            assert lib.cpg_conv2d_wgrad_rider_supported(ctypes.byref(_desc(*s))) == 0, s
    with _lib.option('CPG_NO_WINO_WGRAD', 1):
        assert lib.cpg_conv2d_wgrad_rider_supported(ctypes.byref(_desc(*yes[0]))) == 0
    p = ctypes.c_void_p(1 << 20)
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(p, p, p, p, 2, 32, 198) == _lib.CPG_E_INVALID          # 4 does not divide HW
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(p, ctypes.c_void_p((1 << 20) + 4), p, p, 2, 32, 196) == _lib.CPG_E_INVALID
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(p, p, p, p, 256, 64, 224 * 224) == _lib.CPG_E_INVALID  # >= 2 GiB
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(p, p, p, p, 2, 32, 196) == _lib.CPG_OK
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(None, None, None, None, 0, 0, 0) == _lib.CPG_OK        # disarms


def test_rider_instances_compiled_code():
    """The rider instances of k_wgw: nothing spills, every accumulator write is a zero-fill, arch VGPRs <= 256 -- and the instances
    without a rider keep the register and LDS counts they had (133 / 124 / 155 arch VGPRs, 75 264 and 102 400 bytes)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'k.s')
        subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fno-gpu-rdc', '-x', 'hip', '-S', '--cuda-device-only',
                        os.path.join(ROOT, 'cpg_amd', 'csrc', 'conv3x3_wino_wgrad.hip'), '-o', out], check=True, capture_output=True,
                       timeout=600)
        txt = open(out).read()
    seen = {}
    for m in re.finditer(r'^(_Z\w*k_wgwI(\w+?)EEv\w+):[^\n]*\n(.*?)^\.Lfunc_end', txt, re.S | re.M):
        name, inst, body = m.group(1), m.group(2), m.group(3)
        vg = int(re.search(r'\.set %s\.num_vgpr, (\d+)' % re.escape(name), txt).group(1))
        lds = int(re.search(r'\.amdhsa_kernel %s\n.*?group_segment_fixed_size (\d+)' % re.escape(name), txt, re.S).group(1))
        seen[inst] = (vg, lds)
        if not inst.endswith('Li0E'):
            zero = len(re.findall(r'v_accvgpr_write_b32 a\d+, 0\b', body))
            assert zero == 256 and len(re.findall(r'v_accvgpr_write', body)) == zero, (inst, zero)
            assert 'scratch_' not in body, inst
            assert vg <= 256, (inst, vg)
            assert 's_barrier' in body
    print('k_wgw instances (arch VGPRs, LDS bytes):', seen)
    assert {'Lb0ELi4ELi1E', 'Lb0ELi4ELi2E', 'Lb1ELi4ELi1E', 'Lb1ELi4ELi2E'} <= set(seen)
    assert seen['Lb0ELi4ELi0E'] == (133, 75264) and seen['Lb1ELi4ELi0E'] == (124, 75264) and seen['Lb0ELi2ELi0E'] == (155, 102400)


# ---------------------------------------------------------------------------------------------------------------- on the card
# (N, C, H, W, K): the rider's tensor is the host conv's input [N][C][H][W], the host conv is C -> K
VGG_PAIRS = [('features.7-10', (2, 128, 112, 112, 128)), ('features.14-17', (2, 256, 56, 56, 256)), ('features.17-20', (2, 256, 56, 56, 256)),
             ('features.24-27', (2, 512, 28, 28, 512)), ('features.27-30', (2, 512, 28, 28, 512)), ('features.34-37', (2, 512, 14, 14, 512)),
             ('features.37-40', (4, 512, 14, 14, 512))]
OTHER = [('narrow-14x14-odd-batch', (3, 64, 14, 14, 128)),
         ('uneven', (3, 96, 28, 28, 128)),                 # 1152 wave-items over the waves of 12 unit pairs: no even share
         ('leftover-loop', (1, 32, 28, 28, 128)),          # one stage per wave: more items per wave than its stages carry
         ('more-waves-than-items', (1, 32, 14, 14, 256)),  # 32 planes = 32 items, waves beyond them get nothing
         ('wide-56-grown', (2, 78, 56, 56, 128))]          # a channel count that is no multiple of 32 on the host's input side


def _run_pair(shape, seed, special=False, pm=True, rider=True):
    """(gy, dgamma, dbeta, gW, gPM) of BatchNorm -> ReLU backward + the host weight gradient; rider: through the attach call."""
    N, C, H, W, K = shape
    lib = _lib.lib()
    g = torch.Generator(device='cpu').manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    y = rnd(N, C, H, W)                                     # the BatchNorm's input
    gz = rnd(N, C, H, W)                                    # gradient reaching relu(bn(y)) = the host conv's input gradient
    if special:
        # NaN / +-inf in the first four channels only (one of them turns its channel's two means, hence the whole channel, into NaN);
        # -0.0 everywhere
        vals = [float('nan'), float('inf'), float('-inf')]
        for i in range(12):
            (y if i % 2 else gz)[i % N, i % 4].view(-1)[(i * 7919 + 13) % (H * W)] = vals[i % 3]
        for i in range(64):
            y.view(-1)[(i * 7919 + 13) % y.numel()] = -0.0
            gz.view(-1)[(i * 104729 + 5) % gz.numel()] = -0.0
    gamma, beta = rnd(C).abs() + 0.5, rnd(C) * 0.3
    mean, invstd = rnd(C) * 0.2, 1.0 / (rnd(C).abs() + 0.5)
    x = torch.relu(rnd(N, C, H, W))                          # the host conv's input and output gradient
    go = rnd(N, K, H, W)
    w = rnd(K, C, 3, 3) * 0.05
    pmask = (rnd(K, C, 3, 3) * 0.01 + THR) if pm else None
    y, gz, gamma, beta, mean, invstd, x, go, w = [t.to(DEV) for t in (y, gz, gamma, beta, mean, invstd, x, go, w)]
    pmask = None if pmask is None else pmask.to(DEV)
    d = _desc(N, C, H, W, K)
    s = _lib.stream_ptr()
    gyb = torch.full_like(y, 7.0)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
    gw = torch.empty_like(w)
    gpm = None if pmask is None else torch.empty_like(w)
    wsb, nbb = _lib.workspace(lib.cpg_bn_workspace_bytes(N, C, H * W), DEV)
    ws, nb = _lib.workspace(lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    P = _lib.dptr
    if rider:
        assert lib.cpg_conv2d_wgrad_rider_supported(ctypes.byref(d)) == 1
        table = torch.empty(C, 8, device=DEV)
        _lib.check('reduce', lib.cpg_bn_relu_bwd_reduce(P(y), P(gz), P(gamma), P(beta), P(mean), P(invstd), P(dgamma), P(dbeta), P(table),
                                                        N, C, H * W, P(wsb), nbb, s))
        _lib.check('attach', lib.cpg_conv2d_wgrad_attach_bn_bwd(P(y), P(gz), P(gyb), P(table), N, C, H * W))
    else:
        _lib.check('bn', lib.cpg_bn_relu_bwd(P(y), P(gz), P(gamma), P(beta), P(mean), P(invstd), P(gyb), P(dgamma), P(dbeta), N, C, H * W, 1, 1,
                                             P(wsb), nbb, s))
    _lib.check('wgrad', lib.cpg_conv2d_wgrad(ctypes.byref(d), P(x), P(go), P(w), P(pmask), THR, P(gw), P(gpm), None, P(ws), nb, s))
    torch.cuda.synchronize()
    return gyb, dgamma, dbeta, gw, gpm


def _check_pair(shape, seed, **kw):
    a = _run_pair(shape, seed, rider=True, **kw)
    b = _run_pair(shape, seed, rider=False, **kw)
    names = ('gy', 'dgamma', 'dbeta', 'gW', 'gPM')
    for n, ta, tb in zip(names, a, b):
        if ta is None:
            assert tb is None
            continue
        diff = ((_bits(ta) != _bits(tb)) & ~(torch.isnan(ta) & torch.isnan(tb))).sum().item()
        print('%s %s: %d of %d words differ (%d NaN)' % (shape, n, diff, ta.numel(), int(torch.isnan(ta).sum())))
        assert _same(ta, tb), (shape, n, diff)


@pytest.mark.gpu
@pytest.mark.parametrize('name,shape', VGG_PAIRS, ids=[n for n, _ in VGG_PAIRS])
def test_rider_matches_standalone_pass_on_vgg_pairs(name, shape):
    _check_pair(shape, 11)


@pytest.mark.gpu
@pytest.mark.parametrize('name,shape', OTHER, ids=[n for n, _ in OTHER])
def test_rider_covers_every_item_once(name, shape):
    """Narrow maps, item counts that do not divide over waves or k-steps, ranges longer than the stages that carry them (the loop before
    the epilogue), waves without any item.  A launch whose last block has idle waves cannot take a rider at all: the GS = 4 instances
    only run grids of whole blocks, such shapes are refused by the query (test_rider_query_and_switch_on_the_host) and fall back
    (test_refused_descriptor_takes_the_standalone_path)."""
    _check_pair(shape, 23)
    _check_pair(shape, 24, pm=False)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 128, 28, 28, 128), (2, 64, 14, 14, 128)], ids=['wide', 'narrow'])
def test_rider_passes_nan_inf_and_negative_zero_through_unchanged(shape):
    _check_pair(shape, 31, special=True)


@pytest.mark.gpu
def test_rider_is_one_shot_and_refused_launches_fail_before_launching():
    lib = _lib.lib()
    N, C, H, W, K = 2, 64, 28, 28, 96                    # three output-channel blocks: no rider
    d = _desc(N, C, H, W, K)
    t = lambda *s: torch.randn(*s, device=DEV)
    y, gz, x, go, w = t(N, C, H, W), t(N, C, H, W), t(N, C, H, W), t(N, K, H, W), t(K, C, 3, 3)
    gyb, table = torch.full_like(y, 7.0), torch.zeros(C, 8, device=DEV)
    gw = torch.full_like(w, 5.0)
    ws, nb = _lib.workspace(lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    P = _lib.dptr
    s = _lib.stream_ptr()
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(P(y), P(gz), P(gyb), P(table), N, C, H * W) == _lib.CPG_OK
    rc = lib.cpg_conv2d_wgrad(ctypes.byref(d), P(x), P(go), P(w), None, THR, P(gw), None, None, P(ws), nb, s)
    assert rc == -2
    torch.cuda.synchronize()
    assert bool((gw == 5.0).all()) and bool((gyb == 7.0).all())
    # the failed call disarmed the thread: the next one is a plain weight gradient
    rc = lib.cpg_conv2d_wgrad(ctypes.byref(d), P(x), P(go), P(w), None, THR, P(gw), None, None, P(ws), nb, s)
    assert rc == _lib.CPG_OK
    torch.cuda.synchronize()
    assert bool((gyb == 7.0).all()) and not bool((gw == 5.0).any())


def _stack(widths=(32, 128, 128, 128), widths14=(128, 128)):
    """conv-BN-ReLU x 3 at 28 x 28, pool, conv-BN-ReLU x 2 at 14 x 14: two wide rider pairs, one narrow, one pooled BatchNorm"""
    mods, cin = [], 32
    for i, c in enumerate(widths[1:]):
        mods += [nl.SharableConv2d(cin, c, 3, padding=1, bias=False), nn.BatchNorm2d(c), nn.ReLU(inplace=True)]
        cin = c
    mods.append(nn.MaxPool2d(2, 2))
    for c in widths14:
        mods += [nl.SharableConv2d(cin, c, 3, padding=1, bias=False), nn.BatchNorm2d(c), nn.ReLU(inplace=True)]
        cin = c
    return fused_bn.FusedSequential(*mods)


def _train(widths, widths14, with_pm, count=None):
    torch.manual_seed(5)
    net = _stack(widths, widths14)
    for m in net:
        if isinstance(m, nl.SharableConv2d):
            nn.init.kaiming_normal_(m.weight)
            if with_pm:
                m.piggymask = nn.Parameter(torch.randn_like(m.weight) * 0.01 + THR)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.5, 1.5)
            nn.init.normal_(m.bias, 0.0, 0.2)
    net = net.to(DEV).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9)
    g = torch.Generator(device='cpu').manual_seed(9)
    for step in range(3):
        x = torch.randn(4, 32, 28, 28, generator=g).to(DEV).requires_grad_(True)     # (the first conv needs its input gradient too)
        t = torch.randn(4, widths14[-1], 14, 14, generator=g).to(DEV)
        opt.zero_grad(set_to_none=True)
        loss = ((net(x) - t) ** 2).mean()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    state['x.grad'] = x.grad.detach().clone()
    return state


@pytest.mark.gpu
@pytest.mark.parametrize('with_pm', [False, True], ids=['task1', 'piggymask'])
def test_three_sgd_steps_agree_with_and_without_the_rider(with_pm, monkeypatch):
    calls = []
    real = nl._bn_bwd_rider

    def counted(*a, **k):
        r = real(*a, **k)
        calls.append(r is not None)
        return r
    monkeypatch.setattr(nl, '_bn_bwd_rider', counted)
    monkeypatch.setattr(fused_bn, 'ENABLE_WGRAD_RIDER', True)
    on = _train((32, 128, 128, 128), (128, 128), with_pm)
    assert len(calls) == 3 * 3 and all(calls), calls          # two wide pairs and the narrow one, three steps
    del calls[:]
    with _lib.option('CPG_NO_WW_RIDER', 1):
        off = _train((32, 128, 128, 128), (128, 128), with_pm)
    assert not calls
    assert set(on) == set(off)
    for k in on:
        if on[k].dtype == torch.float32:
            assert _same(on[k], off[k]), k
        else:
            assert torch.equal(on[k], off[k]), k


@pytest.mark.gpu
def test_refused_descriptor_takes_the_standalone_path(monkeypatch):
    """96-channel layers (three output-channel blocks: a last block with idle waves) are refused by the query: no reduce-only launch, no
    attach, and the step is the one the library computes with the rider switched off, bit for bit."""
    calls = []
    real = nl._bn_bwd_rider
    monkeypatch.setattr(nl, '_bn_bwd_rider', lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(fused_bn, 'ENABLE_WGRAD_RIDER', True)
    on = _train((32, 96, 96, 96), (96, 96), False)
    assert not calls
    with _lib.option('CPG_NO_WW_RIDER', 1):
        off = _train((32, 96, 96, 96), (96, 96), False)
    for k in on:
        assert torch.equal(on[k], off[k]) if on[k].dtype != torch.float32 else _same(on[k], off[k]), k
    monkeypatch.setattr(fused_bn, 'ENABLE_WGRAD_RIDER', False)       # ... and with no hint at all (the code path before the rider existed)
    none = _train((32, 96, 96, 96), (96, 96), False)
    for k in on:
        assert torch.equal(on[k], none[k]) if on[k].dtype != torch.float32 else _same(on[k], none[k]), k
