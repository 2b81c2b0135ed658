"""Tables, runners and the main case body of tests/test_eval_conv_gpu.py (cpg_conv2d_fwd_bn_eval against the fp64 reference of
tests/_evalconv.py), shared with tests/test_guard_bands_gpu.py.  The runners take a buffer factory (tests/_parity_cases.py: PLAIN is
today's torch.full / .to(DEV)); every assertion lives here."""
import ctypes

import numpy as np
import torch

import _evalconv as E
from _parity_cases import PLAIN
from cpg_amd import _lib
from oracle import ops

DEV = 'cuda:0'
THR = ops.DEFAULT_THRESHOLD
EPS = 1e-5
NO_WINO = {'CPG_NO_WINO': 1}

# id, kernel, output channels per block (the unit skip_stats[1] counts), (N, C, H, W, K), library options
CASES = [
    ('wg1', 'wg1', 32, (4, 32, 28, 28, 48), {}),
    ('wg1-grown78', 'wg1', 32, (2, 78, 56, 56, 78), {}),                 # C % 4 = 2: the last chunk overlaps its neighbour
    ('wg3', 'wg3', 64, (2, 128, 14, 14, 256), {}),
    ('wg3-grown313', 'wg3', 64, (2, 156, 28, 28, 313), {}),
    ('wg3odd-7x7', 'wg3', 64, (3, 128, 7, 7, 128), {}),
    ('wg3odd-9x7', 'wg3', 64, (2, 256, 9, 7, 128), {}),
    ('wg3odd-grown627', 'wg3', 64, (2, 313, 7, 7, 627), {}),            # C % 4 = 1
    ('wg2', 'wg2', 32, (2, 64, 16, 16, 96), {'CPG_WINO_KERNEL': 'pair'}),
    ('V7', 'direct', 128, (5, 64, 7, 7, 64), {}),
    ('S16', 'direct', 128, (3, 64, 9, 11, 130), {}),
    ('S16-c18', 'direct', 128, (2, 18, 13, 13, 70), {}),                 # C % 4 = 2: a ragged last chunk
    ('P28', 'direct', 128, (2, 12, 28, 28, 128), {}),
    ('D64', 'direct', 64, (2, 8, 8, 56, 40), {}),
    ('M64', 'direct', 64, (2, 3, 32, 32, 64), {}),
    ('M128', 'direct', 128, (2, 20, 15, 33, 130), {}),
    # even maps the Winograd kernels take by default, sent to the direct kernels
    ('nowino-M64', 'direct', 64, (4, 32, 28, 28, 48), NO_WINO),
    ('nowino-D64', 'direct', 64, (2, 78, 56, 56, 78), NO_WINO),
    ('nowino-S16', 'direct', 128, (2, 128, 14, 14, 256), NO_WINO),
    ('nowino-P28', 'direct', 128, (2, 156, 28, 28, 313), NO_WINO),
    # forced tile configs (CPG_C3_FORCE, an A/B knob), each only on the maps it was built for
    ('force-V14', 'direct', 128, (2, 128, 14, 14, 256), dict(NO_WINO, CPG_C3_FORCE=7)),
    ('force-S16', 'direct', 128, (2, 64, 16, 16, 96), dict(NO_WINO, CPG_C3_FORCE=2)),
    ('force-D128', 'direct', 128, (2, 78, 56, 56, 78), dict(NO_WINO, CPG_C3_FORCE=3)),
    ('force-D64', 'direct', 64, (2, 32, 8, 112, 130), dict(NO_WINO, CPG_C3_FORCE=4)),
]
CASE_BY_ID = {c[0]: c for c in CASES}
PATTERNS = ('dense', 'task-mask', 'grown-split', 'alt32-dead', 'pm-dead', 'one-weight', 'all-dead', 'neg-zero')

RATIOS = {}             # kernel family -> {case id: largest error ratio}


def _family(kernel):
    return 'direct' if kernel == 'direct' else 'winograd'


def _record(kernel, cid, r):
    d = RATIOS.setdefault(kernel, {})
    d[cid] = max(d.get(cid, 0.0), r)


def _split(n):
    """A split point in (0, n) that is no multiple of 4 (hence of 32 or 64 either)."""
    s = max(1, (n * 5) // 9)
    if s % 4 == 0:
        s -= 1
    return s


def make_pattern(name, K, C, g):
    """(w, pm, bias?) of one weight pattern, fp32 CPU tensors (pm / bias may be None)."""
    w = torch.randn(K, C, 3, 3, generator=g) * float(np.sqrt(2.0 / (9 * C)))
    pm = None
    m0, c0 = _split(K), _split(C)
    bias = name in ('grown-split', 'alt32-dead', 'one-weight', 'all-dead')
    if name == 'task-mask':
        owner = torch.randint(0, 4, (K, C, 3, 3), generator=g).numpy().astype(np.uint8)
        w = torch.from_numpy(ops.apply_mask(w.numpy(), owner, 2))
        pm = torch.where(torch.rand(K, C, 3, 3, generator=g) < 0.9, 0.01, 0.001)        # a tenth of the shared slots masked off
    elif name in ('grown-split', 'neg-zero'):
        live = torch.zeros(K, C, 1, 1, dtype=torch.bool)
        live[:m0, :c0] = True
        w = torch.where(live, w, torch.tensor(-0.0 if name == 'neg-zero' else 0.0))
    elif name == 'alt32-dead':
        w[(torch.arange(K) // 32) % 2 == 1] = 0.0
    elif name == 'pm-dead':
        pm = torch.full((K, C, 3, 3), 0.01)
        pm[:, c0:] = THR                                  # bin(pm) = 0 at the threshold itself (x <= thr -> 0)
        pm[:, c0:, 0, 0] = THR * 0.5
    elif name == 'one-weight':
        w.zero_()
        w[K - 1, C - 1, 2, 2] = 0.75
    elif name == 'all-dead':
        w.zero_()
    if name == 'neg-zero':
        assert bool(torch.signbit(w[K - 1, C - 1]).all())
    b = torch.randn(K, generator=g) * 0.3 if bias else None
    return w.contiguous(), (None if pm is None else pm.float().contiguous()), b


def make_bn(K, g):
    gamma = torch.rand(K, generator=g) + 0.5
    beta = torch.rand(K, generator=g) - 0.5
    mean = torch.randn(K, generator=g) * 0.3
    var = torch.rand(K, generator=g) * 1.5 + 0.5
    var[0] = 0.0                                          # eps alone under the square root
    return gamma, beta, mean, var


def _desc(N, C, H, W, K):
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K = N, C, H, W, K
    d.R = d.S = 3
    d.stride_h = d.stride_w = d.pad_h = d.pad_w = d.dil_h = d.dil_w = d.groups = 1
    return d


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_eval(x, w, pm, bias, bn, relu, ws=None, buf=PLAIN):
    """cpg_conv2d_fwd_bn_eval on device tensors -> (status, y, skip_stats) on the host.  y starts as NaN and skip_stats as -7, so
    a value the kernel never wrote cannot pass."""
    L = _lib.lib()
    N, C, H, W = x.shape
    K = w.shape[0]
    d = _desc(N, C, H, W, K)
    y = buf.full((N, K, H, W), float('nan'))
    st = buf.full((2,), -7, torch.int32)
    if ws is None:
        ws, nbytes = _lib.workspace(L.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    else:
        nbytes = ws.numel() * 4
    gamma, beta, mean, var = bn
    rc = L.cpg_conv2d_fwd_bn_eval(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(pm), THR, _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(mean),
                                  _ptr(var), EPS, int(relu), _ptr(y), _ptr(st), _ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, y.cpu(), st.cpu().tolist()


def _ws_bytes(shape):
    return int(_lib.lib().cpg_conv2d_workspace_bytes(ctypes.byref(_desc(*shape))))


_REF = {}


def reference(shape, pattern, x, w, pm, b, bn, family):
    """(pre-ReLU ref, conv_term, shift_term), cached: the direct and Winograd cases of one shape share inputs."""
    key = (shape, pattern, family)
    if key not in _REF:
        _REF[key] = E.eval_conv_terms(x, w, pm, b, *bn, eps=EPS, relu=False, threshold=THR, family=family)
    return _REF[key]


def _inputs(shape, pattern):
    N, C, H, W, K = shape
    g = torch.Generator().manual_seed(N * 1000003 + C * 1009 + H * 31 + W * 7 + K + PATTERNS.index(pattern) * 7919)
    x = torch.randn(N, C, H, W, generator=g)
    w, pm, b = make_pattern(pattern, K, C, g)
    bn = make_bn(K, g)
    return x, w, pm, b, bn


def _dead_blocks(dead, B):
    K = dead.numel()
    return sum(bool(dead[i:min(K, i + B)].all()) for i in range(0, K, B))


def _set(libopt, opts):
    for k, v in opts.items():
        libopt.set(k, v)


def eval_conv_case(cid, libopt, buf=PLAIN):
    _, kernel, B, shape, opts = CASE_BY_ID[cid]
    N, C, H, W, K = shape
    _set(libopt, opts)
    fam = _family(kernel)
    assert _lib.lib().cpg_conv2d_winograd(ctypes.byref(_desc(*shape)), 3) == (1 if fam == 'winograd' else 0), cid
    gamma = E.GAMMA[fam]
    skipped = {}
    for pattern in PATTERNS:
        x, w, pm, b, bn = _inputs(shape, pattern)
        xd, wd, pd, bd, bnd = buf.put(x), buf.put(w), buf.put(pm), buf.put(b), tuple(buf.put(t) for t in bn)
        ref0, conv_term, shift_term = reference(shape, pattern, x, w, pm, b, bn, fam)
        dead = E.dead_output_channels(w, pm, THR)
        outs = {}
        for relu in (0, 1):
            rc, y, st = run_eval(xd, wd, pd, bd, bnd, relu, buf=buf)
            assert rc == 0, (cid, pattern, _lib.lib().cpg_last_error())
            ref = ref0.clamp_min(0.0) if relu else ref0
            err = (y.double() - ref).abs()
            bound = gamma * conv_term + shift_term
            bad = ~(err <= bound)
            assert not bool(bad.any()), ('%s %s relu=%d: %d elements out of bound, worst err %.3g at bound %.3g' % (
                cid, pattern, relu, int(bad.sum()), float(err[bad].max()) if bool(torch.isfinite(err[bad]).any()) else float('nan'),
                float(bound[bad][0])))
            if bool(dead.any()):             # no live weight: relu?(BN(bias or 0)) within the epilogue's own rounding
                assert bool((err[:, dead] <= shift_term[:, dead]).all()), (cid, pattern, relu)
            _record(kernel, cid, E.error_ratio(y, ref, conv_term, shift_term))
            outs[relu] = y
            # skip_stats
            assert st[0] == E.live_input_extent(w, pm, THR), (cid, pattern, st)
            nb = _dead_blocks(dead, B)
            assert (st[1] > 0) == (nb > 0), (cid, pattern, st, nb)
            skipped[pattern] = st[1]
        # the skip only ever drops exact zeros: bit-identical to the full contraction
        libopt.set('CPG_NO_DEAD_SKIP', 1)
        rc, y_full, st_full = run_eval(xd, wd, pd, bd, bnd, 0, buf=buf)
        libopt.set('CPG_NO_DEAD_SKIP', None)
        assert rc == 0 and st_full == [0, 0], (cid, pattern, st_full)
        assert torch.equal(y_full, outs[0]), (cid, pattern, float((y_full - outs[0]).abs().max()))
    for p in ('dense', 'task-mask', 'pm-dead'):
        assert skipped[p] == 0, (cid, p, skipped)
    assert skipped['all-dead'] > 0, (cid, skipped)
    assert (skipped['alt32-dead'] > 0) == (B == 32), (cid, skipped)
    assert skipped['grown-split'] < skipped['all-dead'], (cid, skipped)
    assert (skipped['grown-split'] > 0) == (-(-_split(K) // B) * B < K), (cid, skipped)
