"""Tables, runners and the main case body of tests/test_eval_blocks_gpu.py (cpg_conv2d_fwd_bn_eval / _add on the pointwise and 3x3
stride-2 tiles against the fp64 reference of tests/_evalres.py), shared with tests/test_guard_bands_gpu.py.  The runners take a buffer
factory (tests/_parity_cases.py: PLAIN is today's torch.full / .to(DEV)); every assertion lives here."""
import collections
import ctypes

import numpy as np
import torch

import _evalres as R
from _parity_cases import PLAIN
from cpg_amd import _lib
from oracle import ops

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


def _out(d, buf=PLAIN):
    oh = (d.H + 2 * d.pad_h - d.R) // d.stride_h + 1
    ow = (d.W + 2 * d.pad_w - d.S) // d.stride_w + 1
    return buf.full((d.N, d.K, oh, ow), float('nan'))


def run_fwd(d, x, w, pm, bias, buf=PLAIN):
    L = _lib.lib()
    y = _out(d, buf)
    ws, nbytes = _lib.workspace(L.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    rc = L.cpg_conv2d_fwd(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(pm), THR, _ptr(bias), _ptr(y), _ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.cpg_last_error()
    return y


def run_eval(d, x, w, pm, bias, bn, eps, relu, residual=None, add=False, buf=PLAIN):
    """cpg_conv2d_fwd_bn_eval (add False) or cpg_conv2d_fwd_bn_eval_add on device tensors -> (status, y on the device, skip_stats).
    y starts as NaN and skip_stats as -7: a value the kernel never wrote cannot pass."""
    L = _lib.lib()
    y = _out(d, buf)
    st = buf.full((2,), -7, torch.int32)
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


def eval_block_case(cid, libopt, buf=PLAIN):
    tile, k, (N, C, H, W, K, s), opts, unaligned = CASES[cid]
    for name, v in opts.items():
        libopt.set(name, v)
    d = _desc(N, C, H, W, K, k, s)
    L = _lib.lib()
    pointwise = k == 1
    assert L.cpg_conv2d_fwd_bn_eval_supported(ctypes.byref(d)) == 1
    assert L.cpg_conv2d_fwd_bn_eval_add_supported(ctypes.byref(d)) == (1 if pointwise else 0)
    assert L.cpg_conv2d_winograd(ctypes.byref(d), 3) == 0
    ident = tuple(buf.put(t) for t in (torch.ones(K), torch.zeros(K), torch.zeros(K), torch.ones(K)))
    for pi, pattern in enumerate(PATTERNS):
        g = torch.Generator().manual_seed(N * 1000003 + C * 1009 + H * 31 + W * 7 + K + s * 131 + pi * 7919)
        x = torch.randn(N, C, H, W, generator=g)
        w, pm, b = make_pattern(pattern, K, C, k, g)
        bn = make_bn(K, g)
        xd, wd, pd, bd = buf.put(x, 1 if unaligned else 0), buf.put(w), buf.put(pm), buf.put(b)
        assert not unaligned or xd.data_ptr() % 16 == 4
        bnd = tuple(buf.put(t) for t in bn)
        y0 = run_fwd(d, xd, wd, pd, bd, buf=buf)
        assert bool(torch.isfinite(y0).all())
        res = torch.randn(y0.shape, generator=g)
        resd = buf.put(res)
        tag = (cid, pattern)
        # 1. identity BatchNorm: the plain forward, bit for bit
        for relu in (0, 1):
            rc, y, st = run_eval(d, xd, wd, pd, bd, ident, 0.0, relu, buf=buf)
            assert rc == 0, (tag, L.cpg_last_error())
            assert st == [0, 0], (tag, st)                                           # 3. no skipping
            want = y0.clamp_min(0.0) if relu else y0
            assert _bits_equal(y, want), (tag, relu, float((y - want).abs().max()))
            if pointwise:
                rc, y, _ = run_eval(d, xd, wd, pd, bd, ident, 0.0, relu, resd, add=True, buf=buf)
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
                rc, y, st = run_eval(d, xd, wd, pd, bd, bnd, EPS, relu, resd if residual is not None else None, add=residual is not None,
                                        buf=buf)
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
