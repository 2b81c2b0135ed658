"""The residual topologies' inference kernels against the fp64 reference of tests/_evalres.py: cpg_conv2d_fwd_bn_eval on the pointwise
shapes (k_pw's BNE instances, all five forward tiles) and on the 3x3 stride-2 shapes (k_c3_fwd's S2* tiles with a C3BnEval), and
cpg_conv2d_fwd_bn_eval_add, the block tail with the residual in the pointwise epilogue.

Every shape is the smallest that reaches its tile's edges (partial pixel tiles, tiles that straddle images, a partial channel tile);
every case runs six weight patterns and checks
  * identity BatchNorm (gamma 1, beta 0, mean 0, var 1, eps 0), relu off: bit-equal to cpg_conv2d_fwd on the same inputs -- the same
    tile and accumulation order, so this pins every address the epilogue computes; `_add` bit-equal to that output + residual in
    fp32; relu on: to its clamp_min(0);
  * general BatchNorm (gamma of both signs, var in [0.5, 2]), relu on / off, with / without residual: every element inside the
    a-priori bound L * U32 * |s| * (|x| (*) |w_eff|) + U32 * (shift_mag + 2 |residual|); dead output channels inside its second term;
  * skip_stats == {0, 0}: these shapes skip nothing.
The largest observed error / bound ratios are printed per tile (profiles/resnet_eval_fuse.md records them).
Network level: a width-0.25 ResNet-50 and the PackNet ResNet-50 in eval mode under no_grad, fused_bn.FUSE_EVAL_BLOCKS on against off:
launch counts by entry point, logits within the project's 1e-4 bar."""
import collections
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import _evalres as R
from oracle import ops

pytestmark = pytest.mark.gpu

from cpg_amd import _lib                         # noqa: E402
from cpg_amd.models import fused_bn              # noqa: E402
from cpg_amd.models import layers as nl          # noqa: E402

DEV = 'cuda:0'
THR = ops.DEFAULT_THRESHOLD
EPS = 1e-5

# id -> (tile, kernel size, (N, C, H, W, K, stride), library options, unaligned input)
CASES = collections.OrderedDict([
    # 720 grid positions: 3 full + 1 partial 224-pixel tile, every tile straddles images; channel tiles 128 + 16
    ('PwV-720', ('PwV', 1, (5, 32, 12, 12, 144, 1), {}, False)),
    ('PwV-partial', ('PwV', 1, (3, 16, 8, 8, 80, 1), {}, False)),                 # one partial tile
    ('PwS-odd', ('PwS', 1, (6, 48, 7, 7, 80, 1), {}, False)),                     # 49-pixel planes: per-pixel staging
    ('PwS-s2', ('PwS', 1, (3, 32, 14, 14, 144, 2), {}, False)),
    ('PwS-s2-nonsquare', ('PwS', 1, (2, 32, 10, 6, 80, 2), {}, False)),
    ('PwV64', ('PwV64', 1, (3, 32, 8, 8, 48, 1), {}, False)),
    ('PwS64-odd', ('PwS64', 1, (3, 32, 7, 7, 64, 1), {}, False)),
    ('PwS64-s2', ('PwS64', 1, (3, 32, 14, 14, 48, 2), {}, False)),
    ('PwV2-720', ('PwV2', 1, (5, 32, 12, 12, 144, 1), {'CPG_PW_TILE': 1}, False)),
    ('PwS-unaligned', ('PwS', 1, (5, 32, 12, 12, 144, 1), {}, True)),             # x one float into a larger buffer: the per-pixel tile
    ('S2P28', ('S2P28', 3, (2, 16, 56, 56, 80, 2), {}, False)),
    ('S2S16', ('S2S16', 3, (2, 16, 28, 28, 80, 2), {}, False)),
    ('S2M8', ('S2M8', 3, (3, 16, 14, 14, 80, 2), {}, False)),
    ('S2G64', ('S2G64', 3, (2, 16, 18, 22, 48, 2), {}, False)),
    ('S2G128', ('S2G128', 3, (2, 16, 36, 40, 80, 2), {}, False)),
])
PATTERNS = ('dense', 'task-mask', 'bias', 'alt-dead', 'all-dead', 'neg-zero')

RATIOS = {}             # tile -> largest (|y - ref| - shift term) / (L U32 |s| (|x| * |w_eff|)) seen: < 1 is inside the a-priori bound


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    if RATIOS:
        print('\neval-block error ratios, (|y - ref| - shift term) / (L U32 |s| (|x| * |w_eff|)), largest per tile:')
        print('  ' + '  '.join('%s=%.4f' % kv for kv in sorted(RATIOS.items())))


def make_pattern(name, K, C, k, g):
    """(w, pm, bias) of one weight pattern, fp32 CPU tensors (pm / bias may be None): test_eval_conv_gpu.make_pattern's idea for any
    kernel size."""
    w = torch.randn(K, C, k, k, generator=g) * float(np.sqrt(2.0 / (k * k * C)))
    pm = None
    if name == 'task-mask':
        pm = torch.where(torch.rand(K, C, k, k, generator=g) < 0.9, 0.01, 0.001)     # a tenth of the slots under the threshold
    elif name == 'alt-dead':
        w[1::2] = 0.0                                                               # every second output channel dead
    elif name == 'all-dead':
        w.zero_()
    elif name == 'neg-zero':
        live = torch.zeros(K, C, 1, 1, dtype=torch.bool)
        live[:(K * 5) // 9, :(C * 5) // 9] = True
        w = torch.where(live, w, torch.tensor(-0.0))
        assert bool(torch.signbit(w[K - 1, C - 1]).all())
    b = torch.randn(K, generator=g) * 0.3 if name in ('bias', 'alt-dead', 'all-dead') else None
    return w.contiguous(), (None if pm is None else pm.float().contiguous()), b


def make_bn(K, g):
    sign = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
    gamma = (torch.rand(K, generator=g) + 0.5) * sign
    beta = torch.rand(K, generator=g) - 0.5
    mean = torch.randn(K, generator=g) * 0.3
    var = torch.rand(K, generator=g) * 1.5 + 0.5
    return gamma, beta, mean, var


def _desc(N, C, H, W, K, k, s):
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K = N, C, H, W, K
    d.R = d.S = k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = k // 2
    d.dil_h = d.dil_w = d.groups = 1
    return d


def _dev(t, unaligned=False):
    if t is None:
        return None
    if not unaligned:
        return t.to(DEV).contiguous()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _out(d):
    oh = (d.H + 2 * d.pad_h - d.R) // d.stride_h + 1
    ow = (d.W + 2 * d.pad_w - d.S) // d.stride_w + 1
    return torch.full((d.N, d.K, oh, ow), float('nan'), device=DEV)


def run_fwd(d, x, w, pm, bias):
    L = _lib.lib()
    y = _out(d)
    ws, nbytes = _lib.workspace(L.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    rc = L.cpg_conv2d_fwd(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(pm), THR, _ptr(bias), _ptr(y), _ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.cpg_last_error()
    return y


def run_eval(d, x, w, pm, bias, bn, eps, relu, residual=None, add=False):
    """cpg_conv2d_fwd_bn_eval (add False) or cpg_conv2d_fwd_bn_eval_add on device tensors -> (status, y on the device, skip_stats).
    y starts as NaN and skip_stats as -7: a value the kernel never wrote cannot pass."""
    L = _lib.lib()
    y = _out(d)
    st = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    ws, nbytes = _lib.workspace(L.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    gamma, beta, mean, var = bn
    head = (ctypes.byref(d), _ptr(x), _ptr(w), _ptr(pm), THR, _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), eps)
    if add:
        rc = L.cpg_conv2d_fwd_bn_eval_add(*head, _ptr(residual), int(relu), _ptr(y), _ptr(ws), nbytes, _lib.stream_ptr())
    else:
        rc = L.cpg_conv2d_fwd_bn_eval(*head, int(relu), _ptr(y), _ptr(st), _ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, y, st.cpu().tolist()


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('cid', list(CASES))
def test_eval_block_kernels(cid, libopt):
    tile, k, (N, C, H, W, K, s), opts, unaligned = CASES[cid]
    for name, v in opts.items():
        libopt.set(name, v)
    d = _desc(N, C, H, W, K, k, s)
    L = _lib.lib()
    pointwise = k == 1
    assert L.cpg_conv2d_fwd_bn_eval_supported(ctypes.byref(d)) == 1
    assert L.cpg_conv2d_fwd_bn_eval_add_supported(ctypes.byref(d)) == (1 if pointwise else 0)
    assert L.cpg_conv2d_winograd(ctypes.byref(d), 3) == 0
    ident = tuple(t.to(DEV) for t in (torch.ones(K), torch.zeros(K), torch.zeros(K), torch.ones(K)))
    for pi, pattern in enumerate(PATTERNS):
        g = torch.Generator().manual_seed(N * 1000003 + C * 1009 + H * 31 + W * 7 + K + s * 131 + pi * 7919)
        x = torch.randn(N, C, H, W, generator=g)
        w, pm, b = make_pattern(pattern, K, C, k, g)
        bn = make_bn(K, g)
        xd, wd, pd, bd = _dev(x, unaligned), _dev(w), _dev(pm), _dev(b)
        bnd = tuple(_dev(t) for t in bn)
        y0 = run_fwd(d, xd, wd, pd, bd)
        assert bool(torch.isfinite(y0).all())
        res = torch.randn(y0.shape, generator=g)
        resd = _dev(res)
        tag = (cid, pattern)
        # 1. identity BatchNorm: the plain forward, bit for bit
        for relu in (0, 1):
            rc, y, st = run_eval(d, xd, wd, pd, bd, ident, 0.0, relu)
            assert rc == 0, (tag, L.cpg_last_error())
            assert st == [0, 0], (tag, st)                                           # 3. no skipping
            want = y0.clamp_min(0.0) if relu else y0
            assert _bits_equal(y, want), (tag, relu, float((y - want).abs().max()))
            if pointwise:
                rc, y, _ = run_eval(d, xd, wd, pd, bd, ident, 0.0, relu, resd, add=True)
                assert rc == 0, (tag, L.cpg_last_error())
                want = (y0 + resd).clamp_min(0.0) if relu else y0 + resd
                assert _bits_equal(y, want), (tag, relu, 'add', float((y - want).abs().max()))
        # 2. general BatchNorm against fp64
        parts = R.conv_parts(x, w, pm, s, k // 2, THR)
        dead = R.dead_output_channels(w, pm, THR)
        assert bool(dead.any()) == (pattern in ('alt-dead', 'all-dead', 'neg-zero')), tag
        for residual in ((None, res) if pointwise else (None,)):
            ref0, conv_term, shift_term = R.eval_res_terms(parts, b, *bn, EPS, residual)
            for relu in (0, 1):
                rc, y, st = run_eval(d, xd, wd, pd, bd, bnd, EPS, relu, resd if residual is not None else None, add=residual is not None)
                assert rc == 0, (tag, L.cpg_last_error())
                y = y.cpu()
                ref = ref0.clamp_min(0.0) if relu else ref0
                err = (y.double() - ref).abs()
                ratio = R.error_ratio(y, ref, conv_term, shift_term)
                print('%s %s relu=%d residual=%d: ratio %.4f' % (cid, pattern, relu, residual is not None, ratio))
                RATIOS[tile] = max(RATIOS.get(tile, 0.0), ratio)
                bad = ~(err <= conv_term + shift_term)
                assert not bool(bad.any()), ('%s relu=%d residual=%d: %d elements out of bound, worst ratio %.3g' % (
                    tag, relu, residual is not None, int(bad.sum()), ratio))
                if bool(dead.any()):             # no live weight: relu?(BN(bias or 0) [+ residual]) within the epilogue's own rounding
                    assert bool((err[:, dead] <= shift_term[:, dead]).all()), (tag, relu)


def test_refusals():
    """`_add` on a 3x3 descriptor: CPG_E_UNSUPPORTED and y untouched; a NULL residual: CPG_E_INVALID, y untouched."""
    g = torch.Generator().manual_seed(5)
    for k, s in ((3, 1), (3, 2)):
        N, C, H, W, K = 2, 16, 14, 14, 80
        d = _desc(N, C, H, W, K, k, s)
        xd, wd = _dev(torch.randn(N, C, H, W, generator=g)), _dev(torch.randn(K, C, k, k, generator=g))
        bnd = tuple(_dev(t) for t in make_bn(K, g))
        rc, y, _ = run_eval(d, xd, wd, None, None, bnd, EPS, 1, torch.zeros_like(_out(d)), add=True)
        assert rc == -2 and bool(torch.isnan(y).all()), (k, s, rc)                    # CPG_E_UNSUPPORTED
    N, C, H, W, K = 3, 16, 8, 8, 80
    d = _desc(N, C, H, W, K, 1, 1)
    xd, wd = _dev(torch.randn(N, C, H, W, generator=g)), _dev(torch.randn(K, C, 1, 1, generator=g))
    rc, y, _ = run_eval(d, xd, wd, None, None, tuple(_dev(t) for t in make_bn(K, g)), EPS, 1, None, add=True)
    assert rc == _lib.CPG_E_INVALID and bool(torch.isnan(y).all()), rc


# ---------------------------------------------------------------------------------------------------------------- network level
BN_LAUNCHES = ('cpg_bn_relu_fwd_eval', 'cpg_bn_add_relu_fwd', 'cpg_bn_relu_pool3_fwd', 'cpg_bn_relu_fwd_train')
FUSED = ('cpg_conv2d_fwd_bn_eval', 'cpg_conv2d_fwd_bn_eval_add')


def _randomise(net, g):
    for m in net.modules():
        if isinstance(m, (nl.SharableConv2d, nl.SharableLinear)):
            m.piggymask = nn.Parameter(torch.where(torch.rand(m.weight.shape, generator=g) < 0.9, 0.01, 0.001))
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5, generator=g)
                m.bias.uniform_(-0.2, 0.3, generator=g)
                m.running_mean.normal_(0, 0.2, generator=g)
                m.running_var.uniform_(0.5, 2.0, generator=g)
    return net.to(DEV).eval()


def _forward_counted(net, x, switch, monkeypatch):
    """(logits, Counter of C entry points launched through _lib.call) of one eval forward under no_grad with FUSE_EVAL_BLOCKS = switch."""
    counts = collections.Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    monkeypatch.setattr(fused_bn, 'FUSE_EVAL_BLOCKS', switch)
    monkeypatch.setattr(_lib, 'call', counting)
    try:
        with torch.no_grad():
            y = net(x)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_lib, 'call', real)
    return y, counts


def _check_on_off(net, x, monkeypatch):
    on, c_on = _forward_counted(net, x, True, monkeypatch)
    off, c_off = _forward_counted(net, x, False, monkeypatch)
    # off: launch for launch what it was -- 53 convs, a BatchNorm pass behind each (36 + 16 + the stem's pooled one), nothing fused
    assert c_off['cpg_conv2d_fwd'] == 53 and [c_off[n] for n in FUSED] == [0, 0], c_off
    assert [c_off[n] for n in BN_LAUNCHES] == [36, 16, 1, 0], c_off
    # on: the stem's pooled BatchNorm is the only BatchNorm launch left, 52 fused convs
    assert [c_on[n] for n in BN_LAUNCHES] == [0, 0, 1, 0], c_on
    assert [c_on[n] for n in FUSED] == [36, 16] and c_on['cpg_conv2d_fwd'] == 1, c_on
    assert set(c_on) - set(FUSED) <= set(c_off), (c_on, c_off)
    assert bool(torch.isfinite(on).all()) and on.shape == off.shape
    assert float((on - off).abs().max()) <= 1e-4 * float(off.abs().max()), (float((on - off).abs().max()), float(off.abs().max()))


def test_resnet50_quarter_width_on_vs_off(monkeypatch):
    """resnet50(network_width_multiplier=0.25): channels 16 ... 512, every conv behind the stem eligible."""
    from cpg_amd import models as M
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(3)
    net = M.resnet50(dataset_history=[], dataset2num_classes={}, network_width_multiplier=0.25, shared_layer_info={})
    net.add_dataset('t1', 7)
    net.set_dataset('t1')
    net = _randomise(net, g)
    _check_on_off(net, torch.randn(2, 3, 64, 64, generator=g).to(DEV), monkeypatch)


def test_packnet_resnet50_on_vs_off(monkeypatch):
    import cpg_amd.packnet_models as pm
    torch.manual_seed(4)
    g = torch.Generator().manual_seed(4)
    net = pm.factory('resnet50')(dataset_history=[], dataset2num_classes={})
    net.add_dataset('t1', 7)
    net.set_dataset('t1')
    net = _randomise(net, g)
    _check_on_off(net, torch.randn(2, 3, 64, 64, generator=g).to(DEV), monkeypatch)
