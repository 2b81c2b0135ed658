"""SphereNet's inference epilogue (cpg_conv2d_fwd_prelu_eval: conv -> + bias -> PReLU [-> + residual] in one kernel, the PRE instances of
k_wg1 / k_wg2 / k_wg3 and k_c3_fwd) against code that exists without it.

Reference: cpg_conv2d_fwd_bn_eval with the identity BatchNorm (gamma 1, beta 0, mean 0, var 1, eps 0, relu off) on the same inputs and
option table -- conv + bias from the SAME inference plan --, then torch.where(v > 0, v, a * v) (+ res) in fp32 torch.  The fused result
must be bit-equal as numbers (torch.equal: -0 equals +0): the product is rounded, then selected, then the sum is rounded.  No tolerance
is involved.

Every shape is the smallest that reaches its kernel's edges (the tables of tests/test_eval_conv_gpu.py and tests/test_eval_blocks_gpu.py);
every case runs six weight patterns x {K slopes, one shared slope} x {no residual, residual where the query takes one}, and checks
skip on == CPG_NO_DEAD_SKIP=1 bit for bit and skip_stats == those of the identity-BatchNorm call.
Network level: a width-0.25 spherenet20 and the PackNet spherenet20 in eval mode under no_grad, fused_bn.FUSE_EVAL_PRELU on against off:
launch counts by entry point, logits and embeddings within the project's 1e-4 bar; under grad mode nothing changes."""
import collections
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import _evalconv as E                          # noqa: F401  (the helper modules of the tests these shapes come from)
import _evalres as R                           # noqa: F401
from oracle import ops

pytestmark = pytest.mark.gpu

from cpg_amd import _lib                         # noqa: E402
from cpg_amd.models import fused_bn              # noqa: E402
from cpg_amd.models import layers as nl          # noqa: E402

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


def _out(d):
    oh = (d.H + 2 * d.pad_h - d.R) // d.stride_h + 1
    ow = (d.W + 2 * d.pad_w - d.S) // d.stride_w + 1
    return torch.full((d.N, d.K, oh, ow), SENTINEL, device=DEV)


def _ws(d, ws):
    if ws is None:
        return _lib.workspace(_lib.lib().cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    return ws, ws.numel() * 4


def run_ident(d, x, w, pm, bias, ws=None):
    """conv + bias from the inference plan: cpg_conv2d_fwd_bn_eval with the identity BatchNorm -> (y on the device, skip_stats)."""
    L = _lib.lib()
    K = d.K
    one, zero = torch.ones(K, device=DEV), torch.zeros(K, device=DEV)
    y = _out(d)
    st = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    ws, nbytes = _ws(d, ws)
    rc = L.cpg_conv2d_fwd_bn_eval(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(pm), THR, _ptr(bias), _ptr(one), _ptr(zero), _ptr(zero), _ptr(one),
                                  0.0, 0, _ptr(y), _ptr(st), _ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.cpg_last_error()
    return y, st.cpu().tolist()


def run_prelu(d, x, w, pm, bias, slope, res=None, ws=None, n_slopes=None):
    """cpg_conv2d_fwd_prelu_eval on device tensors -> (status, y on the device, skip_stats).  y starts as a sentinel and skip_stats as -7:
    a value the kernel never wrote cannot pass."""
    L = _lib.lib()
    y = _out(d)
    st = torch.full((2,), -7, dtype=torch.int32, device=DEV)
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


def _inputs(cid, pattern):
    shape, s, _ = CASES[cid]
    N, C, H, W, K = shape
    g = torch.Generator().manual_seed(N * 1000003 + C * 1009 + H * 31 + W * 7 + K + s * 131 + PATTERNS.index(pattern) * 7919)
    x = torch.randn(N, C, H, W, generator=g)
    w, pm, b = make_pattern(pattern, K, C, g)
    slopes = make_slopes(K, g)
    shared = torch.tensor([-0.3 if pattern == 'dense' else 0.25])
    d = _desc(shape, s)
    res = torch.randn(tuple(_out(d).shape), generator=g)
    return d, tuple(_dev(t) for t in (x, w, pm, b)), _dev(slopes), _dev(shared), _dev(res)


def _set(libopt, opts):
    for k, v in opts.items():
        libopt.set(k, v)


@pytest.mark.parametrize('cid', list(CASES))
def test_prelu_eval_is_bit_equal(cid, libopt):
    shape, s, opts = CASES[cid]
    _set(libopt, opts)
    L = _lib.lib()
    d = _desc(shape, s)
    sup = (L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 0), L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 1))
    assert sup == SUPPORT[cid], (cid, sup)
    if s == 1:      # the plan is cpg_conv2d_fwd_bn_eval's: Winograd exactly where that entry point runs Winograd
        assert L.cpg_conv2d_winograd(ctypes.byref(d), 3) == (1 if cid in WINO else 0), cid
    for pattern in PATTERNS:
        d, (x, w, pm, b), slopes, shared, res = _inputs(cid, pattern)
        tag = (cid, pattern)
        if not sup[0]:
            rc, y, st = run_prelu(d, x, w, pm, b, slopes)
            assert rc == -2 and bool((y == SENTINEL).all()) and st == [-7, -7], (tag, rc)
            continue
        v, st0 = run_ident(d, x, w, pm, b)
        assert bool(torch.isfinite(v).all()), tag
        if s == 2:
            assert st0 == [0, 0], (tag, st0)
        for slope in (slopes, shared):
            for r in ((None, res) if sup[1] else (None,)):
                rc, y, st = run_prelu(d, x, w, pm, b, slope, r)
                assert rc == 0, (tag, L.cpg_last_error())
                want = expect(v, slope, r)
                assert torch.equal(y, want), (tag, slope.numel(), r is not None, int((y != want).sum()), float((y - want).abs().max()))
                assert st == st0, (tag, st, st0)                   # the skip of the identity-BatchNorm call, word for word
        if not sup[1]:                                             # a residual on a class that takes none: refused, nothing written
            rc, y, st = run_prelu(d, x, w, pm, b, slopes, res)
            assert rc == -2 and bool((y == SENTINEL).all()) and st == [-7, -7], (tag, rc)
        # the skip only ever drops exact zeros: bit-identical to the full contraction
        r = res if sup[1] else None
        rc, y_skip, _ = run_prelu(d, x, w, pm, b, slopes, r)
        libopt.set('CPG_NO_DEAD_SKIP', 1)
        rc2, y_full, st_full = run_prelu(d, x, w, pm, b, slopes, r)
        libopt.set('CPG_NO_DEAD_SKIP', None)
        assert rc == 0 and rc2 == 0 and st_full == [0, 0], (tag, st_full)
        assert torch.equal(y_full.view(torch.int32), y_skip.view(torch.int32)), tag
        if pattern == 'all-dead' and s == 1:
            assert st0[0] == 0 and st0[1] > 0, (tag, st0)          # every block skipped: it wrote prelu(bias) + residual
            want = expect(b.view(1, -1, 1, 1).expand_as(y_skip).contiguous(), slopes, r)
            assert torch.equal(y_skip, want), tag


@pytest.mark.parametrize('cid,other', [('wg1', 'wg1'), ('wg1', 'wg1-grown78'), ('M128', 'M128'), ('M128', 'S16'), ('wg3odd-7x7', 'wg3')])
def test_workspace_reuse_rezeroes_liveness(cid, other, libopt):
    """A sparse layer, then a dense one, then the sparse one again, all in one workspace: the liveness words are re-zeroed by every call,
    so skip_stats and the outputs equal those of fresh calls."""
    L = _lib.lib()
    ds, sparse, sl_s, _, res_s = _inputs(cid, 'neg-zero')
    dd, dense, sl_d, _, res_d = _inputs(other, 'dense')
    nb = max(int(L.cpg_conv2d_workspace_bytes(ctypes.byref(ds))), int(L.cpg_conv2d_workspace_bytes(ctypes.byref(dd))))
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=DEV)

    def call(d, a, slope, res, shared):
        rc, y, st = run_prelu(d, *a, slope, res, ws if shared else None)
        assert rc == 0, L.cpg_last_error()
        return y, st
    fresh_s, fresh_d = call(ds, sparse, sl_s, res_s, False), call(dd, dense, sl_d, res_d, False)
    seq = [call(ds, sparse, sl_s, res_s, True), call(dd, dense, sl_d, res_d, True), call(ds, sparse, sl_s, res_s, True)]
    for (y, st), (fy, fst) in zip(seq, [fresh_s, fresh_d, fresh_s]):
        assert st == fst, (cid, other, st, fst)
        assert torch.equal(y, fy), (cid, other)
    if cid == other:                            # (stale flags of the dense layer would show in the sparse one's statistics)
        assert fresh_s[1][0] < fresh_d[1][0], (fresh_s[1], fresh_d[1])


def test_refusals(libopt):
    """Pointwise and grouped descriptors: 0 / CPG_E_UNSUPPORTED; n_slopes = 2 and a NULL slope: CPG_E_INVALID; the channel-split 14 x 14
    tile: refused by the query and the call.  y keeps its sentinel every time."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(11)
    N, C, H, W, K = 2, 32, 14, 14, 64
    x = _dev(torch.randn(N, C, H, W, generator=g))
    slope = _dev(make_slopes(K, g))
    for k, groups in ((1, 1), (3, 2)):
        d = _desc((N, C, H, W, K), 1, k, groups)
        w = _dev(torch.randn(K, C // groups, k, k, generator=g))
        for with_res in (0, 1):
            assert L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), with_res) == 0, (k, groups)
        rc, y, st = run_prelu(d, x, w, None, None, slope, None, ws=torch.empty(1 << 18, device=DEV))
        assert rc == -2 and bool((y == SENTINEL).all()) and st == [-7, -7], (k, groups, rc)
    d = _desc((N, C, H, W, K), 1)
    w = _dev(torch.randn(K, C, 3, 3, generator=g))
    assert L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 1) == 1
    rc, y, st = run_prelu(d, x, w, None, None, slope, None, n_slopes=2)
    assert rc == _lib.CPG_E_INVALID and bool((y == SENTINEL).all()) and st == [-7, -7], rc
    y = _out(d)
    ws, nbytes = _ws(d, None)
    rc = L.cpg_conv2d_fwd_prelu_eval(ctypes.byref(d), _ptr(x), _ptr(w), None, THR, None, None, K, None, _ptr(y), None, _ptr(ws), nbytes,
                                     _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.CPG_E_INVALID and bool((y == SENTINEL).all()), rc
    # CPG_C3_FORCE=8 with CPG_NO_WINO picks the 14 x 14 channel-split tile, which has no fused epilogue
    libopt.set('CPG_NO_WINO', 1)
    libopt.set('CPG_C3_FORCE', 8)
    shape = (2, 128, 14, 14, 256)
    d = _desc(shape, 1)
    assert L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 0) == 0 and L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 1) == 0
    x = _dev(torch.randn(2, 128, 14, 14, generator=g))
    w = _dev(torch.randn(256, 128, 3, 3, generator=g))
    rc, y, st = run_prelu(d, x, w, None, None, _dev(make_slopes(256, g)))
    assert rc == -2 and bool((y == SENTINEL).all()) and st == [-7, -7], rc


@pytest.mark.parametrize('cid', ['wg1', 'wg3odd-7x7', 'S16', 'S2G64'])
def test_unfused_prelu_pass_is_the_same_expression(cid, libopt):
    """cpg_prelu_fwd on the reference conv output is bit-equal to the torch expression: sharing the formula with the conv epilogues did
    not change k_prelu_fwd (7 x 7 and 9 x 11 planes take its scalar path, the others its float4 path)."""
    _set(libopt, CASES[cid][2])
    d, (x, w, pm, b), slopes, shared, res = _inputs(cid, 'bias')
    v, _ = run_ident(d, x, w, pm, b)
    N, K, OH, OW = v.shape
    for slope in (slopes, shared):
        for r in (None, res):
            y = torch.full_like(v, SENTINEL)
            _lib.call('cpg_prelu_fwd', _ptr(v), _ptr(r), _ptr(slope), _ptr(y), N, K, OH * OW, slope.numel(), _lib.stream_ptr())
            torch.cuda.synchronize()
            assert torch.equal(y, expect(v, slope, r)), (cid, slope.numel(), r is not None)


# ---------------------------------------------------------------------------------------------------------------- network level
N_CONVS = 20        # conv -> PReLU pairs of SphereNet-20
N_FUSED = 19        # descriptors the query supports: all but conv1_1 (3 input channels: the strided stem's class has no such epilogue)
N_RESIDUAL = 8      # residual units (1 + 2 + 4 + 1): their second pair carries the residual
# (so with the switch on a forward launches N_FUSED fused convs and, for the N_CONVS - N_FUSED = 1 pair the query refuses, cpg_conv2d_fwd
#  AND the cpg_prelu_fwd behind it: the PReLU launches drop from 20 to 20 - n, to 0 only where n = 20)
NAMES = ('cpg_conv2d_fwd_prelu_eval', 'cpg_conv2d_fwd', 'cpg_prelu_fwd')


def _mask_and_randomise(net, g, masked):
    """apply_mask at task 2 of a random 4-owner assignment on every trunk conv, random PReLU slopes of both signs, non-zero conv biases."""
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d) or isinstance(m, nl.SharableConv2d)]
    assert len(convs) == N_CONVS
    with torch.no_grad():
        for m in convs:
            owner = torch.randint(0, 4, m.weight.shape, generator=g).numpy().astype(np.uint8)
            m.weight.copy_(torch.from_numpy(ops.apply_mask(m.weight.detach().numpy(), owner, 2)))
            m.bias.normal_(0, 0.1, generator=g)
            if masked:
                m.piggymask = nn.Parameter(torch.where(torch.rand(m.weight.shape, generator=g) < 0.9, 0.01, 0.001))
        for m in net.modules():
            if isinstance(m, nn.PReLU):
                m.weight.normal_(0.1, 0.3, generator=g)
    return net.to(DEV).eval()


def _counted(fn, switch, monkeypatch):
    """(result, Counter of the C entry points launched through _lib.call, residual-carrying fused calls) of fn() with FUSE_EVAL_PRELU = switch."""
    counts = collections.Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        if name == 'cpg_conv2d_fwd_prelu_eval' and args[8] is not None:
            counts['with_residual'] += 1
        return real(name, *args)
    monkeypatch.setattr(fused_bn, 'FUSE_EVAL_PRELU', switch)
    monkeypatch.setattr(_lib, 'call', counting)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_lib, 'call', real)
    return out, counts


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())


def _logits(net, x):
    """|x| cos(theta) of the angular head (its second output, |x| phi(theta), steps where floor(m theta / pi) does)."""
    out = net(x)
    return out[0] if isinstance(out, tuple) else out


def _check_on_off(net, x, monkeypatch):
    def infer():
        with torch.no_grad():
            return _logits(net, x), net.forward_to_embeddings(x)
    (lon, eon), c_on = _counted(infer, True, monkeypatch)
    (loff, eoff), c_off = _counted(infer, False, monkeypatch)
    # off: launch for launch what it was -- per forward 20 convs and a PReLU pass behind each (two forwards here), nothing fused
    assert [c_off[n] for n in NAMES] == [0, 2 * N_CONVS, 2 * N_CONVS], c_off
    # on: 19 fused convs, 8 of them with the unit's residual; conv1_1 and its PReLU pass as before
    assert [c_on[n] for n in NAMES] == [2 * N_FUSED, 2 * (N_CONVS - N_FUSED), 2 * (N_CONVS - N_FUSED)], c_on
    assert c_on['with_residual'] == 2 * N_RESIDUAL, c_on
    assert set(c_on) - {'cpg_conv2d_fwd_prelu_eval', 'with_residual'} <= set(c_off), (c_on, c_off)
    for on, off in ((lon, loff), (eon, eoff)):
        assert bool(torch.isfinite(on).all()) and on.shape == off.shape
        assert _close(on, off), (float((on - off).abs().max()), float(off.abs().max()))

    # grad mode: nothing changes -- the parent's launches, and a train step that is bit-identical with the switch on and off
    def step():
        net.train()
        net.zero_grad(set_to_none=True)
        out = _logits(net, x)
        out.square().mean().backward()
        grads = [p.grad.detach().clone() for p in net.parameters() if p.grad is not None]
        net.eval()
        return out.detach(), grads
    (o1, g1), t_on = _counted(step, True, monkeypatch)
    (o0, g0), t_off = _counted(step, False, monkeypatch)
    assert t_on == t_off and t_on['cpg_conv2d_fwd_prelu_eval'] == 0 and t_on['cpg_prelu_fwd'] == N_CONVS, (t_on, t_off)
    assert torch.equal(o1, o0) and len(g1) == len(g0) and len(g1) >= 2 * N_CONVS
    for a, b in zip(g1, g0):
        assert torch.equal(a, b)


def test_spherenet20_quarter_width_on_vs_off(monkeypatch):
    from cpg_amd import models as M
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(5)
    net = M.spherenet20(dataset_history=[], dataset2num_classes={}, network_width_multiplier=0.25, shared_layer_info={})
    net.add_dataset('face_verification', 9)
    net.set_dataset('face_verification')
    net = _mask_and_randomise(net, g, True)
    _check_on_off(net, torch.randn(2, 3, 112, 112, generator=g).to(DEV), monkeypatch)


def test_packnet_spherenet20_on_vs_off(monkeypatch):
    import cpg_amd.packnet_models as pm
    torch.manual_seed(6)
    g = torch.Generator().manual_seed(6)
    net = pm.factory('spherenet20')(dataset_history=[], dataset2num_classes={})
    net.add_dataset('face_verification', 9)
    net.set_dataset('face_verification')
    net = _mask_and_randomise(net, g, False)
    _check_on_off(net, torch.randn(2, 3, 112, 112, generator=g).to(DEV), monkeypatch)
