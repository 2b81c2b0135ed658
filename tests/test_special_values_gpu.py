"""The fused activation kernels on NaN, Inf, exact zeros and ties (tests/_special.py builds the inputs and holds the arbiter: the
stock modules in fp64 on the CPU), and the convolutions on a NaN that must stay inside its image.

Per case (include/cpg_hip.h, "Non-finite values, zeros and ties"):
  (a) forward    NaN at exactly the arbiter's positions, +Inf and -Inf at exactly the arbiter's positions, in outputs, pooled outputs,
                 window maxima and updated running statistics;
  (b) finite     the bar the entry point's fp64 test already uses: 1e-6 of scale for bn_relu / bn_add_act
                 (test_fused_bn_small_planes_fp64), hold() of tests/test_loss_heads_gpu.py -- max(4 x the stock fp32 result's own distance
                 to fp64, 4 * 2^-23) -- elsewhere.  The inference conv epilogues are held to (d) instead: every finite output is
                 BIT-equal to the unpoisoned call, which tests/test_eval_conv_gpu.py, test_eval_blocks_gpu.py and test_prelu_eval_gpu.py
                 hold to fp64;
  (c) gradients  the set of non-zero positions of gx (and of the residual's gradient) is the arbiter's -- the first-maximum routing,
                 overlapping windows included, from the byte mask and from the recomputed mask alike; dgamma / dbeta to bar (b); an
                 exact 0 of the arbiter is an exact 0 here;
  (d) contained  every channel the pattern did not touch is bit-equal to the same call without the poison.
Not compared (tests/_special.py: exclusions): backward values where the arbiter's forward activation is non-finite (eval mode: that
element; training mode: its channel) -- torch lets gy through a NaN activation, the kernels zero it -- and the signs of zeros.

On the parent of the commit that added this file, (a) fails wherever a ReLU or a pooling maximum meets a NaN (fmaxf(NaN, 0) = 0):
bn-nan_x-*, add-nan_x-*, add-nan_res-*, pool2-nan_x-*, pool3-nan_x-*, the attached-maxima cases, the stem, the inference epilogues
and the conv's window maxima; profiles/special_values.md lists the ids.
"""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _special as S
from cpg_amd import _lib
from cpg_amd.models import fused_bn
from cpg_amd.models import layers as nl

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FLOOR = 4 * 2.0 ** -23
FP64_BAR = 1e-6                      # test_fused_bn_small_planes_fp64's


def hold(what, got, stock32, ref64, skip=None, flat=False):
    """Bar (b) on the positions where the arbiter is finite and `skip` is False; prints its figures before it asserts."""
    e, own = S.finite_err(got, ref64, skip), S.finite_err(stock32, ref64, skip)
    bar = FP64_BAR if flat else max(4 * own, FLOOR)
    print('%-28s err %.3e  bar %.3e (stock fp32 %.3e)' % (what, e, bar, own))
    assert e <= bar, (what, e, bar)


def same_nonfinite(what, got, ref, keep=None):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if keep is not None:
        got, ref = got[keep], ref[keep]
    assert S.same_nonfinite(got, ref), '%s: NaN %d / arbiter %d, Inf %d / arbiter %d' % (
        what, int(torch.isnan(got).sum()), int(torch.isnan(ref).sum()), int(torch.isinf(got).sum()), int(torch.isinf(ref).sum()))


def same_support(what, got, ref, keep=None):
    """Non-zero where the arbiter is non-zero, exactly zero where it is exactly zero (on its finite positions inside `keep`)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    m = torch.isfinite(ref) if keep is None else torch.isfinite(ref) & keep
    wrong = ((got != 0) != (ref != 0)) & m
    assert not bool(wrong.any()), '%s: %d positions differ in support, first %s' % (what, int(wrong.sum()), wrong.nonzero()[0].tolist())


def bit_equal(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- BatchNorm family
def _pool_stats(x):
    """[C][N][2] partial sums of x, one tile per image, as a conv epilogue would hand them over (fp32 values of fp64 sums)."""
    xd = x.double()
    return torch.stack([xd.sum(dim=(2, 3)).t(), (xd * xd).sum(dim=(2, 3)).t()], dim=2).float().contiguous()


def run_fused(op, t, train, variant=None):
    """The fused entry point of cpg_amd.models.fused_bn for `op` on the case's tensors -> results on the host."""
    bn = S._module(t, torch.float32, train).to(DEV)
    assert not t['x'].requires_grad
    x = t['x'].to(DEV).requires_grad_(True)
    res = t['res'].to(DEV).requires_grad_(True) if op == 'add' else None
    relu = nn.ReLU(inplace=True)
    extra = {}
    if op in ('bn', 'bn_norelu'):
        y = fused_bn.bn_relu(x, bn, relu=op == 'bn')
    elif op == 'add':
        old = fused_bn.RELU_BYTE_MASK
        fused_bn.RELU_BYTE_MASK = variant != 'recomputed'
        try:
            y = fused_bn.bn_add_act(bn, relu, x, res)
            assert y.grad_fn.has_mask == (variant != 'recomputed' and x.shape[2] * x.shape[3] % 4 == 0)
        finally:
            fused_bn.RELU_BYTE_MASK = old
    elif op == 'pool2' and variant == 'from_max':
        # the window maxima of x as the conv in front would have written them (NaN kept, as max_pool2d does), attached through
        # cpg_bn_relu_pool_attach_max by the Function; training mode takes the statistics from that conv's partial sums
        E = F.max_pool2d(t['x'], 2, 2).to(DEV)
        args, training, nbt = fused_bn._bn_args(bn)
        y = fused_bn._BnReluPoolFn.apply(x, *args, _pool_stats(t['x']).to(DEV) if train else None, nbt, E)
        extra['E'] = E
    elif op == 'pool2':
        y = fused_bn.bn_relu_pool(x, bn)
    else:
        y = fused_bn.conv_bn_act_pool(lambda v: v, bn, relu, nn.MaxPool2d(3, 2, 1), x)
        assert 'Pool3' in type(y.grad_fn).__name__
    assert type(y.grad_fn).__name__.startswith('_Bn'), type(y.grad_fn).__name__           # a fused Function really ran
    y.backward(t['gy'].to(DEV))
    torch.cuda.synchronize()
    out = dict(y=y.detach(), gx=x.grad, gres=None if res is None else res.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
               running_mean=bn.running_mean, running_var=bn.running_var, **extra)
    return {k: (None if v is None else v.detach().cpu()) for k, v in out.items()}


_REFS = {}


def arbiter(op, pattern, train, shape):
    """(case tensors, fp64 arbiter, stock fp32) -- computed once per case and shared by the variants that run it."""
    key = (op, pattern, train, shape)
    if key not in _REFS:
        t = S.build(op, pattern, shape)
        _REFS[key] = (t, S.stock(op, t, train), S.stock(op, t, train, torch.float32))
    return _REFS[key]


def check_case(case, variant=None):
    op, pattern, train, shape = case
    t, ref, s32 = arbiter(op, pattern, train, shape)
    got = run_fused(op, t, train, variant)
    flat = op in ('bn', 'bn_norelu', 'add')
    bad, chan = S.exclusions(ref, train)
    assert S.cap_holds(t, ref, train)
    # (a) forward
    same_nonfinite('y', got['y'], ref['y'])
    if train:
        same_nonfinite('running_mean', got['running_mean'], ref['running_mean'])
        same_nonfinite('running_var', got['running_var'], ref['running_var'])
    # (b) finite positions
    hold('y', got['y'], s32['y'], ref['y'], flat=flat)
    if train:
        hold('running_mean', got['running_mean'], s32['running_mean'], ref['running_mean'], flat=flat)
        hold('running_var', got['running_var'], s32['running_var'], ref['running_var'], flat=flat)
    # (c) gradients, outside the exclusions
    assert got['gx'] is not None and (got['gres'] is None) == (op != 'add')
    for name in ('gx', 'gres'):
        if got[name] is None:
            continue
        same_nonfinite(name, got[name], ref[name], keep=~bad)
        same_support(name, got[name], ref[name], keep=~bad)
        hold(name, got[name], s32[name], ref[name], skip=bad, flat=flat)
    for name in ('dgamma', 'dbeta'):
        same_nonfinite(name, got[name], ref[name], keep=~chan)
        same_support(name, got[name], ref[name], keep=~chan)
        hold(name, got[name], s32[name], ref[name], skip=chan, flat=flat)
    # (d) containment: the channels the pattern did not touch, against the same call without it
    if t['poisoned']:
        clean = run_fused(op, S.build(op, 'plain', shape), train, variant)
        others = [c for c in range(shape[1]) if c not in t['poisoned']]
        for name in ('y', 'gx', 'gres'):
            if got[name] is not None:
                assert bit_equal(got[name][:, others], clean[name][:, others]), name
        for name in ('dgamma', 'dbeta') + (('running_mean', 'running_var') if train else ()):
            assert bit_equal(got[name][others], clean[name][others]), name


CASES = S.cases()


@pytest.mark.parametrize('case', [c for c in CASES if c[0] in ('bn', 'bn_norelu', 'pool2', 'pool3')], ids=S.case_id)
def test_fused_bn_special_values(case):
    check_case(case)


@pytest.mark.parametrize('mask', ['byte', 'recomputed'])
@pytest.mark.parametrize('case', [c for c in CASES if c[0] == 'add'], ids=S.case_id)
def test_fused_bn_add_relu_special_values(case, mask):
    """relu(bn(x) + res) with the forward's byte mask and with the mask recomputed from the saved output: both are the arbiter's."""
    check_case(case, mask)


@pytest.mark.parametrize('case', [c for c in CASES if c[0] == 'pool2'], ids=S.case_id)
def test_fused_bn_relu_pool_from_attached_maxima(case):
    """The pooled passes reading window maxima (gamma > 0 planes: relu(affine(max)) in place of max(relu(affine))): a NaN window gives
    E = NaN and relu(affine(NaN)) = NaN; tied windows route as from x."""
    check_case(case, 'from_max')


# ---------------------------------------------------------------------------------------------------------------- PReLU
def _prelu_cases():
    out = []
    for pattern in S.PRELU_PATTERNS[1:]:
        for slopes in S.PRELU_SLOPES:
            for with_res in (False, True):
                if pattern == 'nan_res' and not with_res:
                    continue
                # 8x8: vector path; 7x9: scalar path; 64x64: a block per plane; 128x128: planes walked image by image in the backward
                shapes = [(2, 4, 8, 8), (2, 4, 7, 9)] + ([(2, 4, 64, 64), (1, 4, 128, 128)] if slopes == 'per_channel' else [])
                out += [(pattern, slopes, with_res, s) for s in shapes]
    return out


def _run_prelu(t):
    mod = nn.PReLU(t['alpha'].numel()).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(t['alpha'])
    x = t['x'].to(DEV).requires_grad_(True)
    res = None if t['res'] is None else t['res'].to(DEV).requires_grad_(True)
    y = fused_bn.prelu(mod, x, res)
    assert type(y.grad_fn).__name__.startswith('_PReluFn'), type(y.grad_fn).__name__
    y.backward(t['gy'].to(DEV))
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu(), gx=x.grad.cpu(), galpha=mod.weight.grad.cpu(), gres=None if res is None else res.grad.cpu())


@pytest.mark.parametrize('pattern,slopes,with_res,shape', _prelu_cases(),
                         ids=lambda v: 'x'.join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_prelu_special_values(pattern, slopes, with_res, shape):
    """PReLU [+ residual]: torch and the kernels agree element for element here (a NaN input gives a NaN output, a * gy as its
    gradient and a NaN slope gradient in both), so nothing is excluded."""
    t = S.build_prelu(pattern, slopes, shape, with_res)
    ref, s32 = S.stock_prelu(t), S.stock_prelu(t, torch.float32)
    got = _run_prelu(t)
    for name in ('y', 'gx', 'galpha', 'gres'):
        if got[name] is None:
            continue
        same_nonfinite(name, got[name], ref[name])
        if name != 'y':
            same_support(name, got[name], ref[name])
        hold(name, got[name], s32[name], ref[name])
    if t['poisoned']:
        clean = _run_prelu(S.build_prelu('plain', slopes, shape, with_res))
        others = [c for c in range(shape[1]) if c not in t['poisoned']]
        for name in ('y', 'gx', 'gres'):
            if got[name] is not None:
                assert bit_equal(got[name][:, others], clean[name][:, others]), name
        if slopes != 'shared':
            assert bit_equal(got['galpha'][others], clean['galpha'][others])


# ---------------------------------------------------------------------------------------------------------------- conv-fused entry points
def _conv(C, K, k, stride, padding, w, bias=None):
    layer = nl.SharableConv2d(C, K, k, stride=stride, padding=padding, bias=bias is not None).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(w)
        if bias is not None:
            layer.bias.copy_(bias)
    return layer


def _wide_bn(K, train, dtype=torch.float32):
    return S._module(dict(gamma=S._per_channel(S.KIND_GAMMA, K), beta=S._per_channel(S.KIND_BETA, K),
                          running_mean=S._per_channel(S.KIND_RMEAN, K), running_var=S._per_channel(S.KIND_RVAR, K)), dtype, train)


@pytest.mark.parametrize('pattern', ['nan_w', 'nan_gy'])
def test_stem_conv_bn_relu_special_values(pattern):
    """The fused stem (conv output never written): a NaN weight in output channel 1 makes that channel -- statistics, running statistics,
    output -- NaN and no other; a NaN in the incoming gradient stays in its channel; the gamma = 0 channels ride along (their weight
    gradient is exactly 0)."""
    N, C, H, W, K, k0 = 2, 3, 12, 20, 64, 1
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * 0.3
    gz = torch.randn(N, K, H, W, generator=g)

    def fused(w, gz):
        seq = fused_bn.FusedSequential(_conv(C, K, 3, 1, 1, w), _wide_bn(K, True), nn.ReLU(inplace=True)).to(DEV)
        z = seq(x.to(DEV))
        assert type(z.grad_fn).__name__ == '_StemConvBnReluFnBackward', type(z.grad_fn).__name__
        z.backward(gz.to(DEV))
        torch.cuda.synchronize()
        return dict(y=z.detach().cpu(), gw=seq[0].weight.grad.cpu(), dgamma=seq[1].weight.grad.cpu(), dbeta=seq[1].bias.grad.cpu(),
                    running_mean=seq[1].running_mean.cpu(), running_var=seq[1].running_var.cpu())

    def stock(w, gz, dtype):
        wd = w.to(dtype).requires_grad_(True)
        bn = _wide_bn(K, True, dtype)
        z = torch.relu(bn(F.conv2d(x.to(dtype), wd, padding=1)))
        z.backward(gz.to(dtype))
        return dict(y=z.detach(), gw=wd.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean, running_var=bn.running_var)

    wp, gzp = w.clone(), gz.clone()
    if pattern == 'nan_w':
        wp[k0, 1, 1, 1] = S.NAN
    else:
        gzp[0, k0, H // 2, W // 2] = S.NAN
    got, clean = fused(wp, gzp), fused(w, gz)
    ref, s32 = stock(wp, gzp, torch.float64), stock(wp, gzp, torch.float32)
    chan = torch.isnan(ref['y']).any(dim=3).any(dim=2).any(dim=0)
    assert chan.tolist() == [c == k0 and pattern == 'nan_w' for c in range(K)]
    others = [c for c in range(K) if c != k0]
    for name in ('y', 'running_mean', 'running_var'):
        same_nonfinite(name, got[name], ref[name])
        hold(name, got[name], s32[name], ref[name])
    for name in ('gw', 'dgamma', 'dbeta'):
        keep = ~chan.view(-1, *([1] * (got[name].dim() - 1))).expand_as(got[name])
        same_nonfinite(name, got[name], ref[name], keep=keep)
        same_support(name, got[name], ref[name], keep=keep)
        hold(name, got[name], s32[name], ref[name], skip=~keep)
    for name in got:
        a, b = (got[name][:, others], clean[name][:, others]) if name == 'y' else (got[name][others], clean[name][others])
        assert bit_equal(a, b), name


# (id, shape N C H W K, kernel, stride, padding, options): one shape per inference epilogue with a ReLU or PReLU in it
EVAL_CONVS = [
    ('wg1', (4, 32, 28, 28, 48), 3, 1, 1, {}),
    ('wg3', (2, 128, 14, 14, 256), 3, 1, 1, {}),
    ('wg3odd', (3, 128, 7, 7, 128), 3, 1, 1, {}),
    ('wg2', (2, 64, 16, 16, 96), 3, 1, 1, {'CPG_WINO_KERNEL': 'pair'}),
    ('direct', (4, 32, 28, 28, 48), 3, 1, 1, {'CPG_NO_WINO': 1}),
    ('pointwise', (2, 64, 14, 14, 64), 1, 1, 0, {}),
    ('s2', (2, 64, 14, 14, 64), 3, 2, 1, {}),
]


def _eval_inputs(shape, k, seed=3):
    N, C, H, W, K = shape
    g = torch.Generator().manual_seed(seed + C + K)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, k, k, generator=g) * (2.0 / (C * k * k)) ** 0.5
    return x, w


@pytest.mark.parametrize('cid,shape,k,stride,padding,opts', EVAL_CONVS, ids=[c[0] for c in EVAL_CONVS])
def test_eval_conv_bn_relu_keeps_nan(cid, shape, k, stride, padding, opts, libopt):
    """Under torch.no_grad(), conv_bn_act / conv_bn_add_act as one kernel: a NaN weight in output channel 1 makes exactly that channel
    NaN (as F.conv2d -> BatchNorm2d -> relu in fp64), a NaN in the residual exactly that element; everything else is bit-equal to the
    unpoisoned call."""
    for name, v in opts.items():
        libopt.set(name, v)
    N, C, H, W, K = shape
    x, w = _eval_inputs(shape, k)
    wp = w.clone()
    wp[1, 0, k // 2, k // 2] = S.NAN
    bn = _wide_bn(K, False).to(DEV)
    relu = nn.ReLU()
    calls = []
    orig = _lib.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)

    def run(w, res=None):
        conv = _conv(C, K, k, stride, padding, w)
        _lib.call = spy
        try:
            with torch.no_grad():
                if res is None:
                    return fused_bn.conv_bn_act(conv, bn, relu, x.to(DEV)).cpu()
                return fused_bn.conv_bn_add_act(conv, bn, relu, x.to(DEV), res.to(DEV)).cpu()
        finally:
            _lib.call = orig

    got, clean = run(wp), run(w)
    assert calls.count('cpg_conv2d_fwd_bn_eval') == 2, calls             # the one-kernel path really ran
    ref = torch.relu(_wide_bn(K, False, torch.float64)(F.conv2d(x.double(), wp.double(), stride=stride, padding=padding)))
    assert bool(torch.isnan(ref[:, 1]).all()) and int(torch.isnan(ref).sum()) == ref[:, 1].numel()
    same_nonfinite('y', got, ref)
    others = [c for c in range(K) if c != 1]
    assert bit_equal(got[:, others], clean[:, others])
    if cid == 'pointwise':
        res = torch.randn(clean.shape, generator=torch.Generator().manual_seed(9))
        resp = res.clone()
        resp[1, 2, 3, 4] = S.NAN
        del calls[:]
        got, clean = run(w, resp), run(w, res)
        assert calls.count('cpg_conv2d_fwd_bn_eval_add') == 2, calls
        assert int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[1, 2, 3, 4]))
        got[1, 2, 3, 4] = clean[1, 2, 3, 4]
        assert bit_equal(got, clean)


@pytest.mark.parametrize('cid,shape,k,stride,padding,opts', [c for c in EVAL_CONVS if c[2] == 3], ids=[c[0] for c in EVAL_CONVS if c[2] == 3])
def test_eval_conv_prelu_keeps_nan(cid, shape, k, stride, padding, opts, libopt, monkeypatch):
    """With FUSE_EVAL_PRELU, conv_prelu as one kernel: the same two poisons through the PReLU (+ residual) epilogue."""
    for name, v in opts.items():
        libopt.set(name, v)
    monkeypatch.setattr(fused_bn, 'FUSE_EVAL_PRELU', True)
    N, C, H, W, K = shape
    x, w = _eval_inputs(shape, k)
    bias = torch.linspace(-0.2, 0.2, K)
    wp = w.clone()
    wp[1, 0, 1, 1] = S.NAN
    mod = nn.PReLU(K).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(torch.linspace(-0.5, 0.75, K))
    calls = []
    orig = _lib.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)

    def run(w, res=None):
        conv = _conv(C, K, 3, stride, padding, w, bias)
        _lib.call = spy
        try:
            with torch.no_grad():
                return fused_bn.conv_prelu(conv, mod, x.to(DEV), None if res is None else res.to(DEV)).cpu()
        finally:
            _lib.call = orig

    got, clean = run(wp), run(w)
    assert calls.count('cpg_conv2d_fwd_prelu_eval') == 2, calls
    ref = F.prelu(F.conv2d(x.double(), wp.double(), bias.double(), stride=stride, padding=padding), mod.weight.detach().cpu().double())
    same_nonfinite('y', got, ref)
    others = [c for c in range(K) if c != 1]
    assert bit_equal(got[:, others], clean[:, others])
    if stride == 1:
        res = torch.randn(clean.shape, generator=torch.Generator().manual_seed(9))
        resp = res.clone()
        resp[1, 2, 3, 4] = S.NAN
        del calls[:]
        got, clean = run(w, resp), run(w, res)
        assert calls.count('cpg_conv2d_fwd_prelu_eval') == 2, calls
        assert int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[1, 2, 3, 4]))
        got[1, 2, 3, 4] = clean[1, 2, 3, 4]
        assert bit_equal(got, clean)


# (N, H, W, K) at C = 64: runs of tiles that straddle images; more units than the chip holds at once, whose last round's maxima come from
# the tail's reduction kernel (tests/test_pool_max_gpu.py: MAPS, TAIL_MAP)
@pytest.mark.parametrize('N,H,W,K', [(3, 8, 12, 64), (3, 8, 12, 128), (5, 120, 120, 64)])
def test_conv_window_maxima_keep_nan(N, H, W, K):
    """The 2 x 2 window maxima the Winograd forward's epilogue writes for the pooled BatchNorm: a NaN in the conv output is a NaN in its
    window's maximum, as in max_pool2d of that output -- in the kernel's own epilogue and in the tail's reduction."""
    lib = _lib.lib()
    d = nl._conv_desc((N, 64, H, W), (K, 64, 3, 3), (1, 1), (1, 1), (1, 1), 1)
    assert lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(d)) == 1
    g = torch.Generator().manual_seed(K + H)
    x = torch.randn(N, 64, H, W, generator=g)
    w = (torch.randn(K, 64, 3, 3, generator=g) * 0.05).to(DEV)
    x[0, 3, H // 2, W // 2] = S.NAN                                  # an interior pixel of the first image ...
    x[N - 1, 5, H - 1, W - 1] = S.NAN                                # ... and the last pixel of the last one (the tail's share)
    x = x.to(DEV)
    tiles = lib.cpg_conv2d_bnstats_tiles(ctypes.byref(d))
    y = torch.zeros((N, K, H, W), device=DEV)
    stats = torch.zeros((K, tiles, 2), device=DEV)
    E = torch.zeros((N, K, H // 2, W // 2), device=DEV)
    ws, nb = _lib.workspace(lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    assert lib.cpg_conv2d_fwd_attach_pool_max(_lib.dptr(E), E.numel() * 4) == _lib.CPG_OK
    rc = lib.cpg_conv2d_fwd_bnstats(ctypes.byref(d), _lib.dptr(x), _lib.dptr(w), None, 0.005, None, _lib.dptr(y), _lib.dptr(stats),
                                    stats.numel() * 4, _lib.dptr(ws), nb, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.CPG_OK, lib.cpg_last_error()
    want = F.max_pool2d(y, 2, 2)
    assert bool(torch.isnan(y).any()) and bool(torch.isnan(y[0]).any()) and bool(torch.isnan(y[N - 1]).any())
    assert not bool(torch.isnan(y[1:N - 1]).any())
    assert bool((torch.isnan(E) == torch.isnan(want)).all()), (int(torch.isnan(E).sum()), int(torch.isnan(want).sum()))
    assert torch.equal(torch.nan_to_num(E, nan=0.0), torch.nan_to_num(want, nan=0.0))


# ---------------------------------------------------------------------------------------------------------------- convolutions
# The smallest member of each multi-image tile class of test_conv_oracle's table (tests/test_hip_parity.py): N, C, H, W, K, k, s, p
CONV_TILE_CLASSES = [
    (6, 32, 7, 7, 160, 3, 1, 1),         # 7x7 maps: virtual-row tiles over 6 images
    (3, 32, 14, 14, 96, 3, 1, 1),        # 14x14 maps: tiles that hold two images
    (4, 16, 14, 14, 72, 3, 1, 1),        # 14x14 maps: channel-split virtual-row tiles
    (2, 32, 12, 28, 128, 3, 1, 1),       # two-image 4x28 strips
    (9, 48, 14, 14, 80, 1, 1, 0),        # pointwise tiles that straddle images
    (5, 32, 7, 7, 48, 1, 1, 0),          # pointwise on 7x7 maps: tiles span 5 images
    (9, 64, 14, 14, 160, 3, 2, 1),       # 3x3 s2, 7x7 outputs: two-image 8x8 tiles
]


def _near(shape4, n0, ph, pw, reach=3):
    """bool[N, 1, H, W]: image n0, within `reach` pixels of (ph, pw)."""
    N, _, H, W = shape4
    m = torch.zeros(N, 1, H, W, dtype=torch.bool)
    m[n0, 0, max(0, ph - reach):ph + reach + 1, max(0, pw - reach):pw + reach + 1] = True
    return m


def _contained(what, got, clean, footprint, near, n0):
    """Other images bit-equal; in image n0 the footprint is NaN and everything else is bit-equal, or NaN within the tile of the poison."""
    got, clean = got.cpu(), clean.cpu()
    rest = [n for n in range(got.shape[0]) if n != n0]
    assert bit_equal(got[rest], clean[rest]), '%s: another image changed' % what
    assert not bool(torch.isnan(clean).any())
    assert bool(torch.isnan(got)[footprint].all()), '%s: a finite value inside the footprint' % what
    same = got.view(torch.int32) == clean.view(torch.int32)
    ok = footprint | same | (torch.isnan(got) & near)
    assert bool(ok[n0].all()), '%s: %d elements of the poisoned image differ outside the tile' % (what, int((~ok[n0]).sum()))


@pytest.mark.parametrize('wino', [True, False], ids=['wino', 'direct'])
@pytest.mark.parametrize('N,C,H,W,K,k,s,p', CONV_TILE_CLASSES)
def test_conv_keeps_nan_inside_its_image(N, C, H, W, K, k, s, p, wino, libopt):
    """A NaN in the last row and column of an image that is not the batch's last -- where a tile that holds two images, or a run of tiles
    that straddles them, would carry it over: forward and weight gradient (NaN in x), input gradient (NaN in gy)."""
    if not wino:
        libopt.set('CPG_NO_WINO', 1)
    g = torch.Generator().manual_seed(N * 1000 + C + K)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, k, k, generator=g) * (2.0 / (C * k * k)) ** 0.5
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    gy = torch.randn(N, K, OH, OW, generator=g)
    n0, c0, k0 = N - 2, 1, 2
    xp, gyp = x.clone(), gy.clone()
    xp[n0, c0, H - 1, W - 1] = S.NAN
    gyp[n0, k0, OH - 1, OW - 1] = S.NAN
    layer = _conv(C, K, k, s, p, w)

    def run(x, gy):
        layer.zero_grad()
        xd = x.to(DEV).requires_grad_(True)
        y = layer(xd)
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
        return y.detach().cpu(), xd.grad.cpu(), layer.weight.grad.cpu()

    y0, gx0, gw0 = run(x, gy)
    y1, gx1, gw1 = run(xp, gy)
    _, gx2, _ = run(x, gyp)
    # the arbiter's footprints: F.conv2d in fp64 and its input gradient
    xd = x.double().requires_grad_(True)
    fy = torch.isnan(F.conv2d(xp.double(), w.double(), stride=s, padding=p))
    F.conv2d(xd, w.double(), stride=s, padding=p).backward(gyp.double())
    fx = torch.isnan(xd.grad)
    assert bool(fy[n0].any()) and not bool(fy[[n for n in range(N) if n != n0]].any()) and bool(fx[n0].any())
    _contained('y', y1, y0, fy, _near(y0.shape, n0, (H - 1) // s, (W - 1) // s), n0)
    _contained('gx', gx2, gx0, fx, _near(gx0.shape, n0, min(H - 1, s * (OH - 1)), min(W - 1, s * (OW - 1))), n0)
    assert bit_equal(gx1, gx0)                                        # (the input gradient does not read x)
    # weight gradient: NaN in gW[:, c0] at every tap that reads the pixel (from the last row and column the first taps of a 3x3 p1 never
    # do; the arbiter says which) -- the Winograd kernels make all of gW[:, c0] NaN -- and no other input channel changes
    wd = w.double().requires_grad_(True)
    F.conv2d(xp.double(), wd, stride=s, padding=p).backward(gy.double())
    fw = torch.isnan(wd.grad)
    assert bool(fw[:, c0].any()) and not bool(fw[:, [c for c in range(C) if c != c0]].any())
    assert bool(torch.isnan(gw1)[fw].all()), 'weight gradient: a finite value at a tap that reads the NaN'
    slice_ok = torch.isnan(gw1[:, c0]) | (gw1[:, c0].contiguous().view(torch.int32) == gw0[:, c0].contiguous().view(torch.int32))
    assert bool(slice_ok.all()), 'weight gradient: a tap of the poisoned channel that does not read the NaN changed'
    rest = [c for c in range(C) if c != c0]
    assert bit_equal(gw1[:, rest], gw0[:, rest]), 'weight gradient: another input channel changed'
