"""cpg_conv2d_fwd_bn_eval_pool: conv3x3 s1 p1 -> BatchNorm2d(eval) [-> ReLU] -> MaxPool2d(2, 2) as one kernel that writes the pooled tensor
alone (the POOL instances of k_wg1 / k_wg2 / k_wg3), with the dead-channel skip of cpg_conv2d_fwd_bn_eval.

Held to three things: the fp64 reference of tests/_evalconv.py pooled (max pooling is 1-Lipschitz in the max norm, so the elementwise bound
is pooled with the values: the committed GAMMA_WINO, no new constant); max_pool2d of what cpg_conv2d_fwd_bn_eval writes for the same inputs,
bit for bit; and, on special values, the stock modules in fp64.  y_pooled starts as NaN and skip_stats as -7 in every call, so a value the
kernel never wrote cannot pass.  The shapes are the smallest that reach each instance and each ragged edge."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _evalconv as E
from oracle import ops

pytestmark = pytest.mark.gpu

from cpg_amd import _lib                                   # noqa: E402
from cpg_amd.models import layers as nl                    # noqa: E402
from cpg_amd.models.fused_bn import FusedSequential        # noqa: E402
from cpg_amd.packnet_models.layers import PlainConv2d      # noqa: E402
import _special as S                                       # noqa: E402
from _eval_conv_cases import DEV, EPS, PATTERNS, THR, _desc, _dev, _inputs, _ptr, _set, _split, _ws_bytes, reference, run_eval   # noqa: E402
from _guarded import GuardedBuffers, guarding              # noqa: E402
from _parity_cases import PLAIN                            # noqa: E402

UNSUPPORTED = -2
# id -> (the kernel the planner picks: 32 or 64 output channels per block, (N, C, H, W, K), library options)
CASES = {
    'wg1': ('k_wg1', (4, 32, 28, 28, 48), {}),
    'wg1-grown78': ('k_wg1', (2, 78, 56, 56, 78), {}),               # C % 4 = 2: the last chunk overlaps its neighbour; K = 78: ragged block
    'wg3': ('k_wg3', (2, 128, 14, 14, 256), {}),                     # whole units; tile runs span images (49 tiles per image)
    'wg3-grown313': ('k_wg3', (2, 156, 28, 28, 313), {}),            # ragged last block (313 = 4 * 64 + 57), ragged last run
    'wg2': ('k_wg2', (2, 64, 16, 16, 96), {'CPG_WINO_KERNEL': 'pair'}),
    'one-tile': ('k_wg3', (3, 64, 2, 2, 64), {}),                    # one tile per image: 3 of a run's 32 tiles exist
    'odd-tiles-per-row': ('k_wg3', (2, 64, 6, 10, 64), {}),          # 3 x 5 tiles per image, a short last run, H != W
}


def _supported(d):
    return _lib.lib().cpg_conv2d_fwd_bn_eval_pool_supported(ctypes.byref(d))


def _pool(t):
    return F.max_pool2d(t, 2, 2)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_pool(x, w, pm, bias, bn, relu, ws=None, buf=PLAIN, desc=None, eps=EPS):
    """cpg_conv2d_fwd_bn_eval_pool on device tensors -> (status, y_pooled, skip_stats) on the host."""
    L = _lib.lib()
    N, C, H, W = x.shape
    K = w.shape[0]
    d = _desc(N, C, H, W, K) if desc is None else desc
    y = buf.full((N, K, H // 2, W // 2), float('nan'))
    st = buf.full((2,), -7, torch.int32)
    if ws is None:
        ws, nbytes = _lib.workspace(L.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    else:
        nbytes = ws.numel() * 4
    gamma, beta, mean, var = bn
    rc = L.cpg_conv2d_fwd_bn_eval_pool(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(pm), THR, _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(mean),
                                       _ptr(var), eps, int(relu), _ptr(y), _ptr(st), _ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, y.cpu(), st.cpu().tolist()


def pool_case(cid, libopt, buf=PLAIN):
    _, shape, opts = CASES[cid]
    _set(libopt, opts)
    d = _desc(*shape)
    assert _lib.lib().cpg_conv2d_winograd(ctypes.byref(d), 3) == 1, cid
    assert _supported(d) == 1, cid
    for pattern in PATTERNS:
        x, w, pm, b, bn = _inputs(shape, pattern)
        xd, wd, pd, bd, bnd = buf.put(x), buf.put(w), buf.put(pm), buf.put(b), tuple(buf.put(t) for t in bn)
        ref0, conv_term, shift_term = reference(shape, pattern, x, w, pm, b, bn, 'winograd')
        bound = _pool(E.GAMMA_WINO * conv_term + shift_term)
        shift_p = _pool(shift_term)
        dead = E.dead_output_channels(w, pm, THR)
        outs = {}
        for relu in (0, 1):
            rc, yp, st = run_pool(xd, wd, pd, bd, bnd, relu, buf=buf)
            assert rc == 0, (cid, pattern, _lib.lib().cpg_last_error())
            ref = _pool(ref0.clamp_min(0.0) if relu else ref0)
            err = (yp.double() - ref).abs()
            worst = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max())
            print('%s %s relu=%d: largest |y - ref| / bound %.4f' % (cid, pattern, relu, worst))
            bad = ~(err <= bound)
            assert not bool(bad.any()), '%s %s relu=%d: %d pooled elements out of bound' % (cid, pattern, relu, int(bad.sum()))
            if bool(dead.any()):             # no live weight: the pooled relu?(BN(bias or 0)) within the epilogue's own rounding
                assert bool((err[:, dead] <= shift_p[:, dead]).all()), (cid, pattern, relu)
            # bit for bit the pooled output of the existing entry point, and its skip statistics
            rc, y, st_full = run_eval(xd, wd, pd, bd, bnd, relu, buf=buf)
            assert rc == 0
            assert _bits_equal(yp, _pool(y)), (cid, pattern, relu, float((yp - _pool(y)).abs().max()))
            assert st == st_full and st[0] == E.live_input_extent(w, pm, THR), (cid, pattern, st, st_full)
            outs[relu] = yp
        libopt.set('CPG_NO_DEAD_SKIP', 1)
        rc, y_noskip, st_noskip = run_pool(xd, wd, pd, bd, bnd, 0, buf=buf)
        libopt.set('CPG_NO_DEAD_SKIP', None)
        assert rc == 0 and st_noskip == [0, 0], (cid, pattern, st_noskip)
        assert _bits_equal(y_noskip, outs[0]), (cid, pattern)
        if pattern == 'all-dead':
            assert st[1] > 0, (cid, st)


@pytest.mark.parametrize('cid', list(CASES))
def test_pooled_matches_fp64_and_the_unpooled_entry(cid, libopt):
    pool_case(cid, libopt)


@pytest.mark.parametrize('cid', ['wg3-grown313', 'one-tile'])
def test_guard_bands(cid, libopt):
    """An epilogue that still addressed the full-resolution plane would overrun the quarter-size output: no guard word and no byte of
    the inputs may change."""
    with guarding() as led:
        pool_case(cid, libopt, buf=GuardedBuffers(DEV))
        led.verify()
        assert led.workspace_requests >= 1 and led.arenas
        assert any(a.label.startswith('full(') for a in led.arenas) and any(a.label.startswith('input') for a in led.arenas)


# ---------------------------------------------------------------------------------------------------------------- special values
SPECIAL_EPS = 0.25


def _special_case(C, K, seed):
    """Inputs on which every fp32 operation of the kernel is exact (small integers, filters of {-4, 0, 4}: G g G^T holds integers;
    BatchNorm parameters that are powers of two or halves, eps = 1/4 and var in {3/4, 15/4, 0}: var + eps in {1, 4, 1/4}), so the fp64 arbiter cast to fp32 is the answer bit
    for bit.  Output channel 0 is the identity on input channel 0 times 4, with gamma = 2^114: an input of +-4096 overflows to +-Inf in
    the epilogue's multiply (2^128) and to the same Inf when the arbiter's 2^128 is cast.  Image 0, channel 0 carries the windows:
        (0, 0) one +Inf            (0, 2) one -Inf beside numbers        (2, 0) four times -Inf        (2, 2) a four-way tie        (3, 3) two +Inf
    and image 1 a NaN in another channel (it reaches every output channel of the windows round it)."""
    g = torch.Generator().manual_seed(seed)
    N, H, W = 2, 8, 8
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).float()
    w = 4.0 * torch.randint(-1, 2, (K, C, 3, 3), generator=g).float()
    w[0] = 0.0
    w[0, 0, 1, 1] = 4.0
    x[0, 0, 0:2, 0:2] = torch.tensor([[4096.0, 1.0], [0.0, -1.0]])
    x[0, 0, 0:2, 4:6] = torch.tensor([[1.0, -4096.0], [2.0, -1.0]])
    x[0, 0, 4:6, 0:2] = -4096.0
    x[0, 0, 4:6, 4:6] = 2.0
    x[0, 0, 6:8, 6:8] = torch.tensor([[4096.0, -2.0], [1.0, 4096.0]])
    x[1, 3, 5, 2] = float('nan')
    pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (K,), generator=g)]      # noqa: E731
    gamma, beta, mean, var = pick([0.5, 1.0, 2.0, -1.0]), pick([-1.0, -0.5, 0.0, 0.5, 1.5]), pick([-2.0, -1.0, 0.0, 1.0]), pick([0.75, 3.75, 0.0])
    gamma[0], beta[0], mean[0], var[0] = 2.0 ** 114, 0.0, 0.0, 0.75
    return x, w, (gamma, beta, mean, var)


@pytest.mark.parametrize('cid,C,K,opts', [('k_wg1', 16, 32, {}), ('k_wg3', 64, 64, {}), ('k_wg2', 64, 64, {'CPG_WINO_KERNEL': 'pair'})])
def test_special_values_match_stock_torch_in_fp64(cid, C, K, opts, libopt):
    _set(libopt, opts)
    x, w, bn = _special_case(C, K, 5)
    assert _supported(_desc(2, C, 8, 8, K)) == 1
    conv = F.conv2d(x.double(), w.double(), None, 1, 1)
    z = F.batch_norm(conv, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, SPECIAL_EPS)
    assert bool(torch.isposinf(z[0, 0]).sum() == 0) and float(z[0, 0, 0, 0]) == 2.0 ** 128          # finite in fp64, Inf once cast
    for relu in (0, 1):
        want = _pool(torch.relu(z) if relu else z).float()
        rc, yp, _ = run_pool(_dev(x), _dev(w), None, None, tuple(_dev(t) for t in bn), relu, eps=SPECIAL_EPS)
        assert rc == 0
        assert S.same_nonfinite(yp, want), (cid, relu)
        ok = ~torch.isnan(want)
        assert torch.equal(yp[ok], want[ok]), (cid, relu, float((yp[ok] - want[ok]).abs().nan_to_num().max()))
        # the windows this case is about
        inf = float('inf')
        assert yp[0, 0, 0, 0] == inf and yp[0, 0, 3, 3] == inf
        assert yp[0, 0, 0, 2] == 8.0 * 2.0 ** 114 and yp[0, 0, 2, 2] == 8.0 * 2.0 ** 114
        assert yp[0, 0, 2, 0] == (0.0 if relu else -inf)
        assert bool(torch.isnan(yp[1, :, 2, 1]).all()) and bool(torch.isfinite(yp[1, :, 0, 3]).all())
        # ... and it is what the unpooled entry point gives
        L = _lib.lib()
        y = torch.full((2, K, 8, 8), float('nan'), device=DEV)
        ws, nbytes = _lib.workspace(L.cpg_conv2d_workspace_bytes(ctypes.byref(_desc(2, C, 8, 8, K))), DEV)
        dv = [_dev(t) for t in (x, w) + bn]
        rc = L.cpg_conv2d_fwd_bn_eval(ctypes.byref(_desc(2, C, 8, 8, K)), _ptr(dv[0]), _ptr(dv[1]), None, THR, None, _ptr(dv[2]), _ptr(dv[3]),
                                      _ptr(dv[4]), _ptr(dv[5]), SPECIAL_EPS, relu, _ptr(y), None, _ptr(ws), nbytes, _lib.stream_ptr())
        assert rc == 0
        py = _pool(y.cpu())
        assert S.same_nonfinite(yp, py) and torch.equal(yp[ok], py[ok]), (cid, relu)


@pytest.mark.parametrize('cid', ['wg1', 'wg2', 'wg3-grown313'])
def test_nan_in_skipped_work(cid, libopt):
    """A NaN or Inf in an input channel past the last live chunk, or feeding an output block with no live weight, does not reach the pooled
    output while the skip is on; with CPG_NO_DEAD_SKIP=1 it does -- the contract of cpg_conv2d_fwd_bn_eval."""
    kernel, shape, opts = CASES[cid]
    N, C, H, W, K = shape
    B = 64 if kernel == 'k_wg3' else 32
    _set(libopt, opts)
    x, w, pm, b, bn = _inputs(shape, 'grown-split')
    m0, c0 = _split(K), _split(C)
    skipped_from, dead_from = 4 * (-(-c0 // 4)), -(-m0 // B) * B
    assert skipped_from < C and dead_from < K, cid
    xn = x.clone()
    xn[0, skipped_from, H // 2, W // 2] = float('inf')
    xn[N - 1, C - 1, 0, W - 1] = float('nan')
    bnd = tuple(_dev(t) for t in bn)
    ref0, conv_term, shift_term = reference(shape, 'grown-split', x, w, pm, b, bn, 'winograd')
    for relu in (0, 1):
        rc, yp, _ = run_pool(_dev(xn), _dev(w), _dev(pm), _dev(b), bnd, relu)
        assert rc == 0 and bool(torch.isfinite(yp).all()), (cid, relu)
        ref = _pool(ref0.clamp_min(0.0) if relu else ref0)
        assert bool(((yp.double() - ref).abs() <= _pool(E.GAMMA_WINO * conv_term + shift_term)).all()), (cid, relu)
    libopt.set('CPG_NO_DEAD_SKIP', 1)
    for relu in (0, 1):
        rc, y_full, _ = run_pool(_dev(xn), _dev(w), _dev(pm), _dev(b), bnd, relu)
        assert rc == 0 and bool(torch.isnan(y_full).any()), (cid, relu)
    libopt.set('CPG_NO_DEAD_SKIP', None)
    xl = x.clone()
    xl[0, 0, H // 2, W // 2] = float('nan')         # a live chunk: reaches the live channels, never the dead blocks
    rc, y_l, _ = run_pool(_dev(xl), _dev(w), _dev(pm), _dev(b), bnd, 0)
    assert rc == 0 and bool(torch.isnan(y_l[:, :m0]).any()), cid
    assert bool(((y_l[:, dead_from:].double() - _pool(ref0)[:, dead_from:]).abs() <= _pool(shift_term)[:, dead_from:]).all()), cid


# ---------------------------------------------------------------------------------------------------------------- refusals
def _general_desc(N, C, H, W, K, k=3, s=1, G=1):
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, k, k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = k // 2
    d.dil_h = d.dil_w = 1
    d.groups = G
    return d


REFUSED = {
    'odd-map': (_general_desc(3, 128, 7, 7, 128), {}),
    'no-wino': (_general_desc(2, 128, 14, 14, 256), {'CPG_NO_WINO': 1}),
    'block-kernel': (_general_desc(2, 128, 14, 14, 256), {'CPG_WINO_KERNEL': 'block'}),
    '3x3-s2': (_general_desc(2, 64, 16, 16, 64, s=2), {}),
    '1x1': (_general_desc(2, 64, 16, 16, 64, k=1), {}),
    'groups-2': (_general_desc(2, 64, 16, 16, 64, G=2), {}),
}


@pytest.mark.parametrize('rid', list(REFUSED))
def test_refusals_touch_nothing(rid, libopt):
    d, opts = REFUSED[rid]
    _set(libopt, opts)
    assert _supported(d) == 0, rid
    g = torch.Generator().manual_seed(3)
    x = torch.randn(d.N, d.C, d.H, d.W, generator=g)
    w = torch.randn(d.K, d.C // d.groups, d.R, d.S, generator=g) * 0.05
    bn = (torch.ones(d.K), torch.zeros(d.K), torch.zeros(d.K), torch.ones(d.K))
    rc, yp, st = run_pool(_dev(x), _dev(w), None, None, tuple(_dev(t) for t in bn), 1, desc=d)
    assert rc == UNSUPPORTED, (rid, rc, _lib.lib().cpg_last_error())
    assert b'cpg_conv2d_fwd_bn_eval_pool' in _lib.lib().cpg_last_error()
    assert yp.numel() > 0 and bool(torch.isnan(yp).all()) and st == [-7, -7], rid


# ---------------------------------------------------------------------------------------------------------------- workspace, streams
@pytest.mark.parametrize('cid,other', [('wg1', 'wg1'), ('wg1', 'wg1-grown78'), ('wg3', 'wg3')])
def test_workspace_reuse_rezeroes_liveness(cid, other, libopt):
    """sparse -> dense -> sparse in one workspace: every call re-zeroes the liveness words."""
    shape, oshape = CASES[cid][1], CASES[other][1]
    ws = torch.empty((max(_ws_bytes(shape), _ws_bytes(oshape)) + 3) // 4, dtype=torch.float32, device=DEV)
    on_dev = lambda a: [_dev(t) if not isinstance(t, tuple) else tuple(_dev(u) for u in t) for t in a]      # noqa: E731
    sparse, dense = on_dev(_inputs(shape, 'grown-split')), on_dev(_inputs(oshape, 'dense'))

    def call(a, shared):
        x, w, pm, b, bn = a
        rc, y, st = run_pool(x, w, pm, b, bn, 1, ws if shared else None)
        assert rc == 0
        return y, st
    fresh_s, fresh_d = call(sparse, False), call(dense, False)
    for (y, st), (fy, fst) in zip([call(sparse, True), call(dense, True), call(sparse, True)], [fresh_s, fresh_d, fresh_s]):
        assert st == fst and _bits_equal(y, fy), (cid, other, st, fst)
    if shape == oshape:
        assert fresh_s[1][0] < fresh_d[1][0], (fresh_s[1], fresh_d[1])


def test_side_stream_equals_stream_zero():
    shape = CASES['wg3-grown313'][1]
    a = [_dev(t) if not isinstance(t, tuple) else tuple(_dev(u) for u in t) for t in _inputs(shape, 'task-mask')]
    x, w, pm, b, bn = a
    rc0, y0, st0 = run_pool(x, w, pm, b, bn, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rc1, y1, st1 = run_pool(x, w, pm, b, bn, 1)
    torch.cuda.current_stream().wait_stream(side)
    assert rc0 == 0 and rc1 == 0 and st0 == st1 and _bits_equal(y0, y1)


# ---------------------------------------------------------------------------------------------------------------- the network
VGG_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']


def _vgg_feature_stack():
    """The width-0.25 VGG feature stack of tests/test_eval_conv_gpu.py: a two-task owner pattern inside a grown split, apply_mask at task 1."""
    from cpg_amd.models.vgg import _conv_stack
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(11)
    mods = _conv_stack(VGG_CFG, 0.25, True, 1)
    for m in mods:
        if isinstance(m, nl.SharableConv2d):
            K, C = m.weight.shape[:2]
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            owner = torch.randint(1, 3, (K, C, 3, 3), generator=g)
            owner[torch.rand(K, C, 3, 3, generator=g) < 0.1] = 0
            owner[_split(K // 2):] = 2
            if C > 3:
                owner[:, _split(C // 2):] = 2
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(ops.apply_mask(m.weight.detach().numpy(), owner.numpy().astype(np.uint8), 1)))
                m.piggymask = nn.Parameter(torch.where(torch.rand(K, C, 3, 3, generator=g) < 0.95, 0.01, 0.001))
        elif isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5, generator=g)
                m.bias.uniform_(-0.2, 0.3, generator=g)
                m.running_mean.normal_(0, 0.2, generator=g)
                m.running_var.uniform_(0.5, 2.0, generator=g)
    return mods, g


def _plain_twin(mods):
    """The same stack from PlainConv2d (no piggymask): each weight is the masked layer's effective weight."""
    out = []
    for m in mods:
        if isinstance(m, nl.SharableConv2d):
            p = PlainConv2d(m.in_channels, m.out_channels, 3, padding=1, bias=False)
            weff = ops.effective_weight(m.weight.detach().numpy(), m.piggymask.detach().numpy(), m.info['threshold'])
            with torch.no_grad():
                p.weight.copy_(torch.from_numpy(weff))
            out.append(p)
        else:
            out.append(copy.deepcopy(m))
    return out


def test_vgg_features_with_the_pooled_groups_fused():
    mods, g = _vgg_feature_stack()
    twin = FusedSequential(*_plain_twin(mods)).to(DEV).eval()
    seq = FusedSequential(*mods).to(DEV).eval()
    x = torch.randn(6, 3, 32, 32, generator=g).to(DEV)
    groups, i = [], 0
    while i < len(mods):
        j = i + 3 + (1 if i + 3 < len(mods) and isinstance(mods[i + 3], nn.MaxPool2d) else 0)
        groups.append(list(range(i, j)))
        i = j
    assert len(groups) == 13 and sum(len(grp) == 4 for grp in groups) == 5
    was = FusedSequential.fuse_eval_pool
    try:
        with torch.no_grad():
            FusedSequential.fuse_eval_pool = True
            FusedSequential.skip_log = []
            whole = seq(x)
            log = [t.cpu().tolist() for t in FusedSequential.skip_log]
            FusedSequential.skip_log = []
            h, pooled_skips = x, []
            for grp in groups:
                sub = FusedSequential(*[mods[k] for k in grp]).eval()
                before = len(FusedSequential.skip_log)
                out = sub(h)
                if len(grp) == 4:
                    conv, bn = mods[grp[0]], mods[grp[1]]
                    assert _supported(_desc(*h.shape, conv.out_channels)) == 1, grp
                    assert len(FusedSequential.skip_log) == before + 1, grp           # the pooled step took the group
                    pooled_skips.append(FusedSequential.skip_log[-1].cpu().tolist()[1])
                    ref, ct, sh = E.eval_conv_terms(h, conv.weight, conv.piggymask, None, bn.weight, bn.bias, bn.running_mean,
                                                    bn.running_var, eps=bn.eps, relu=True, threshold=conv.info['threshold'], family='winograd')
                    err = (out.cpu().double() - _pool(ref)).abs()
                    assert out.shape == (h.shape[0], conv.out_channels, h.shape[2] // 2, h.shape[3] // 2)
                    assert bool((err <= _pool(E.GAMMA_WINO * ct + sh)).all()), (grp, float(err.max()))
                h = out
            FusedSequential.skip_log = None
            plain = twin(x)
            FusedSequential.fuse_eval_pool = False
            FusedSequential.skip_log = []
            unfused = seq(x)
            log_off = len(FusedSequential.skip_log)
    finally:
        FusedSequential.fuse_eval_pool = was
        FusedSequential.skip_log = None
    assert torch.equal(whole, h)
    assert len(log) == 13 and log_off == 8, (len(log), log_off)       # one entry per conv; without the step the five pooled groups log nothing
    assert any(s > 0 for s in pooled_skips), pooled_skips
    assert _bits_equal(whole, plain)
    a, b = whole.flatten(1), unfused.flatten(1)
    assert torch.equal(a.argmax(1), b.argmax(1))
    assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
