"""Tables, runners and the main case body of tests/test_prelu_eval_gpu.py (cpg_conv2d_fwd_prelu_eval, bit-equal to the identity-BatchNorm
call followed by the torch expression), shared with tests/test_guard_bands_gpu.py.  The runners take a buffer factory
(tests/_parity_cases.py: PLAIN is today's torch.full / .to(DEV)); every assertion lives here."""
import collections
import ctypes

import numpy as np
import torch

from _parity_cases import PLAIN
from cpg_amd import _lib
from oracle import ops

DEV = 'cuda:0'
THR = ops.DEFAULT_THRESHOLD
NO_WINO = {'CPG_NO_WINO': 1}

# id -> ((N, C, H, W, K), stride, library options)
CASES = collections.OrderedDict([
    # Winograd inference kernels
    ('wg1', ((4, 32, 28, 28, 48), 1, {})),
    ('wg1-grown78', ((2, 78, 56, 56, 78), 1, {})),
    ('wg3', ((2, 128, 14, 14, 256), 1, {})),
    ('wg3-grown313', ((2, 156, 28, 28, 313), 1, {})),
    ('wg3odd-7x7', ((3, 128, 7, 7, 128), 1, {})),
    ('wg3odd-9x7', ((2, 256, 9, 7, 128), 1, {})),
    ('wg2', ((2, 64, 16, 16, 96), 1, {'CPG_WINO_KERNEL': 'pair'})),
    # direct 3x3 s1 tiles
    ('V7', ((5, 64, 7, 7, 64), 1, {})),
    ('S16', ((3, 64, 9, 11, 130), 1, {})),
    ('S16-c18', ((2, 18, 13, 13, 70), 1, {})),
    ('P28', ((2, 12, 28, 28, 128), 1, {})),
    ('D64', ((2, 8, 8, 56, 40), 1, {})),
    ('M64', ((2, 3, 32, 32, 64), 1, {})),
    ('M128', ((2, 20, 15, 33, 130), 1, {})),
    ('nowino-P28', ((2, 156, 28, 28, 313), 1, NO_WINO)),
    # 3x3 s2 tiles
    ('S2P28', ((2, 16, 56, 56, 80), 2, {})),
    ('S2S16', ((2, 16, 28, 28, 80), 2, {})),
    ('S2M8', ((3, 16, 14, 14, 80), 2, {})),
    ('S2G64', ((2, 16, 18, 22, 48), 2, {})),
    ('S2G128', ((2, 16, 36, 40, 80), 2, {})),
    # SphereNet's own first layer in small: 3 input channels are the strided stem's class, which has no such epilogue
    ('first-layer', ((2, 3, 16, 16, 64), 2, {})),
])
WINO = ('wg1', 'wg1-grown78', 'wg3', 'wg3-grown313', 'wg3odd-7x7', 'wg3odd-9x7', 'wg2')
# what cpg_conv2d_fwd_prelu_eval_supported answers: (without, with a residual)
SUPPORT = {cid: ((1, 1) if s == 1 else (1, 0)) for cid, (_, s, _) in CASES.items()}
SUPPORT['first-layer'] = (0, 0)
PATTERNS = ('dense', 'task-mask', 'bias', 'alt-dead', 'all-dead', 'neg-zero')


def make_pattern(name, K, C, g):
    """(w, pm, bias) of one weight pattern, fp32 CPU tensors (pm / bias may be None): the six of tests/test_eval_blocks_gpu.py."""
    w = torch.randn(K, C, 3, 3, generator=g) * float(np.sqrt(2.0 / (9 * C)))
    pm = None
    if name == 'task-mask':
        pm = torch.where(torch.rand(K, C, 3, 3, generator=g) < 0.9, 0.01, 0.001)     # a tenth of the slots under the threshold
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


def make_slopes(K, g):
    """K per-channel slopes of both signs that include exactly 0, 1 and a value > 1."""
    a = torch.randn(K, generator=g) * 0.5
    a[0], a[1 % K], a[2 % K], a[K - 1] = 0.0, 1.0, 1.75, -0.5
    assert bool((a == 0).any()) and bool((a == 1).any()) and bool((a > 1).any()) and bool((a < 0).any())
    return a


def _desc(shape, s, k=3, groups=1):
    N, C, H, W, K = shape
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K = N, C, H, W, K
    d.R = d.S = k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = k // 2
    d.dil_h = d.dil_w = 1
    d.groups = groups
    return d


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


SENTINEL = -12345.5


def _out(d, buf=PLAIN):
    oh = (d.H + 2 * d.pad_h - d.R) // d.stride_h + 1
    ow = (d.W + 2 * d.pad_w - d.S) // d.stride_w + 1
    return buf.full((d.N, d.K, oh, ow), SENTINEL)


def _ws(d, ws):
    if ws is None:
        return _lib.workspace(_lib.lib().cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    return ws, ws.numel() * 4


def run_ident(d, x, w, pm, bias, ws=None, buf=PLAIN):
    """conv + bias from the inference plan: cpg_conv2d_fwd_bn_eval with the identity BatchNorm -> (y on the device, skip_stats)."""
    L = _lib.lib()
    K = d.K
    one, zero = buf.put(torch.ones(K)), buf.put(torch.zeros(K))
    y = _out(d, buf)
    st = buf.full((2,), -7, torch.int32)
    ws, nbytes = _ws(d, ws)
    rc = L.cpg_conv2d_fwd_bn_eval(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(pm), THR, _ptr(bias), _ptr(one), _ptr(zero), _ptr(zero), _ptr(one),
                                  0.0, 0, _ptr(y), _ptr(st), _ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.cpg_last_error()
    return y, st.cpu().tolist()


def run_prelu(d, x, w, pm, bias, slope, res=None, ws=None, n_slopes=None, buf=PLAIN):
    """cpg_conv2d_fwd_prelu_eval on device tensors -> (status, y on the device, skip_stats).  y starts as a sentinel and skip_stats as -7:
    a value the kernel never wrote cannot pass."""
    L = _lib.lib()
    y = _out(d, buf)
    st = buf.full((2,), -7, torch.int32)
    ws, nbytes = _ws(d, ws)
    rc = L.cpg_conv2d_fwd_prelu_eval(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(pm), THR, _ptr(bias), _ptr(slope),
                                     slope.numel() if n_slopes is None else n_slopes, _ptr(res), _ptr(y), _ptr(st), _ptr(ws), nbytes,
                                     _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, y, st.cpu().tolist()


def expect(v, slope, res=None):
    """The fp32 torch expression: one rounded product, the select, one rounded sum (separate elementwise kernels: nothing fuses)."""
    a = slope.view(1, -1, 1, 1)
    z = torch.where(v > 0, v, a * v)
    return z if res is None else z + res


def _inputs(cid, pattern, buf=PLAIN):
    shape, s, _ = CASES[cid]
    N, C, H, W, K = shape
    g = torch.Generator().manual_seed(N * 1000003 + C * 1009 + H * 31 + W * 7 + K + s * 131 + PATTERNS.index(pattern) * 7919)
    x = torch.randn(N, C, H, W, generator=g)
    w, pm, b = make_pattern(pattern, K, C, g)
    slopes = make_slopes(K, g)
    shared = torch.tensor([-0.3 if pattern == 'dense' else 0.25])
    d = _desc(shape, s)
    oh, ow = (d.H + 2 * d.pad_h - d.R) // d.stride_h + 1, (d.W + 2 * d.pad_w - d.S) // d.stride_w + 1
    res = torch.randn((d.N, d.K, oh, ow), generator=g)
    return d, tuple(buf.put(t) for t in (x, w, pm, b)), buf.put(slopes), buf.put(shared), buf.put(res)


def _set(libopt, opts):
    for k, v in opts.items():
        libopt.set(k, v)


def prelu_eval_case(cid, libopt, buf=PLAIN):
    shape, s, opts = CASES[cid]
    _set(libopt, opts)
    L = _lib.lib()
    d = _desc(shape, s)
    sup = (L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 0), L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 1))
    assert sup == SUPPORT[cid], (cid, sup)
    if s == 1:      # the plan is cpg_conv2d_fwd_bn_eval's: Winograd exactly where that entry point runs Winograd
        assert L.cpg_conv2d_winograd(ctypes.byref(d), 3) == (1 if cid in WINO else 0), cid
    for pattern in PATTERNS:
        d, (x, w, pm, b), slopes, shared, res = _inputs(cid, pattern, buf)
        tag = (cid, pattern)
        if not sup[0]:
            rc, y, st = run_prelu(d, x, w, pm, b, slopes, buf=buf)
            assert rc == -2 and bool((y == SENTINEL).all()) and st == [-7, -7], (tag, rc)
            continue
        v, st0 = run_ident(d, x, w, pm, b, buf=buf)
        assert bool(torch.isfinite(v).all()), tag
        if s == 2:
            assert st0 == [0, 0], (tag, st0)
        for slope in (slopes, shared):
            for r in ((None, res) if sup[1] else (None,)):
                rc, y, st = run_prelu(d, x, w, pm, b, slope, r, buf=buf)
                assert rc == 0, (tag, L.cpg_last_error())
                want = expect(v, slope, r)
                assert torch.equal(y, want), (tag, slope.numel(), r is not None, int((y != want).sum()), float((y - want).abs().max()))
                assert st == st0, (tag, st, st0)                   # the skip of the identity-BatchNorm call, word for word
        if not sup[1]:                                             # a residual on a class that takes none: refused, nothing written
            rc, y, st = run_prelu(d, x, w, pm, b, slopes, res, buf=buf)
            assert rc == -2 and bool((y == SENTINEL).all()) and st == [-7, -7], (tag, rc)
        # the skip only ever drops exact zeros: bit-identical to the full contraction
        r = res if sup[1] else None
        rc, y_skip, _ = run_prelu(d, x, w, pm, b, slopes, r, buf=buf)
        libopt.set('CPG_NO_DEAD_SKIP', 1)
        rc2, y_full, st_full = run_prelu(d, x, w, pm, b, slopes, r, buf=buf)
        libopt.set('CPG_NO_DEAD_SKIP', None)
        assert rc == 0 and rc2 == 0 and st_full == [0, 0], (tag, st_full)
        assert torch.equal(y_full.view(torch.int32), y_skip.view(torch.int32)), tag
        if pattern == 'all-dead' and s == 1:
            assert st0[0] == 0 and st0[1] > 0, (tag, st0)          # every block skipped: it wrote prelu(bias) + residual
            want = expect(b.view(1, -1, 1, 1).expand_as(y_skip).contiguous(), slopes, r)
            assert torch.equal(y_skip, want), tag
