"""Special-value inputs for the fused activation kernels (BatchNorm2d -> ReLU [-> MaxPool2d], relu(bn(x) + res), PReLU) and the
arbiter they are held to -- no GPU here; tests/test_special_values_host.py checks this file on the arbiter alone and
tests/test_special_values_gpu.py runs the kernels on what it builds.

Every BatchNorm input is an (N, 4k, H, W) fp32 tensor whose channels cycle through four kinds (KIND):
    0  gamma > 0            1  gamma < 0            2  gamma = 0, beta > 0  (z == beta)            3  gamma = 0, beta = 0  (z == 0)
so the gamma = 0 kinds ride along in every case.  The patterns:
    plain     nothing special: the call the others are compared with for containment
    nan_x     one NaN in x at an interior element of (n = 0, c = 0)
    inf_x     +Inf in x in channel 0 and -Inf in channel 1 of image 0 (eval mode only: Inf - Inf in the batch statistics is nan_x again)
    nan_gy    one NaN in the incoming gradient, channel 0
    nan_res   one NaN in the residual of relu(bn(x) + res), channel 0
    ties      x constant on every pooling window: a coarse randn repeated 2 x 2 (MaxPool2d(2, 2)), a constant per (n, c) plane with
              both signs of bn(x) (MaxPool2d(3, 2, 1), whose windows overlap).  Identical x give identical bn(x) in any precision, so the
              ties are exact in the fp32 kernels and in the fp64 arbiter alike
    zeros     eval mode, x == running_mean (a power of two) in every channel and beta = 0: z is exactly 0 everywhere

The arbiter is the stock modules in fp64 on the CPU on the same fp32 values (nn.BatchNorm2d, torch.relu, F.max_pool2d, F.prelu,
F.conv2d); `stock32` is the same chain in fp32, whose distance to the arbiter is the bar of tests/test_loss_heads_gpu.py's hold().

What is NOT compared (exclusions()): backward values at elements whose forward activation is non-finite in the arbiter (eval mode) or
in that element's whole channel (training mode: one NaN makes the batch statistics, hence the channel, NaN), and the parameter gradients
of such a channel: torch's threshold_backward lets gy through a NaN activation, the kernels zero it (include/cpg_hip.h).  The cap on
that: every builder poisons ONE channel (inf_x: two elements in two channels, as the pattern is defined), so no case may exclude more
than the poisoned channels -- cap_holds() is a condition on the arbiter's own output, not a measurement of a kernel.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1
KIND_GAMMA = (1.3, -0.9, 0.0, 0.0)
KIND_BETA = (0.2, -0.1, 0.4, 0.0)
KIND_RMEAN = (0.1, -0.2, 0.05, 0.3)
KIND_RVAR = (0.9, 1.2, 1.0, 0.8)
PATTERNS = ('plain', 'nan_x', 'inf_x', 'nan_gy', 'nan_res', 'ties', 'zeros')
OPS = ('bn', 'bn_norelu', 'add', 'pool2', 'pool3')
NAN, INF = float('nan'), float('inf')


# The smallest shape on each side of every path switch of csrc/bn_kernels.hip:
#   2x4x8x8      16-byte vector path, one wave per plane (HW < 4096; < 1024 windows), planes walked flattened by the reductions
#   2x4x7x9      HW % 4 != 0: the scalar paths of the plain passes; MaxPool2d(3, 2, 1): odd rows and columns, no 8-byte pairs
#   2x4x6x10     15 windows per plane: no 16-byte rows of window maxima
#   2x4x64x64    HW = 4096: a block per plane; 1024 windows per plane: a block per plane in the pooled passes (wave_windows)
#   1x4x128x128  HW / 4 = 16 * 256 and 4096 windows: the reductions walk the plane image by image, four visits per trip
#   2x4x40x24    MaxPool2d(3, 2, 1): 20 window rows = three strips of eight, the last one ragged
_PLAIN_SHAPES = [(2, 4, 8, 8), (2, 4, 7, 9), (2, 4, 64, 64), (1, 4, 128, 128)]
SHAPES = {'bn': _PLAIN_SHAPES, 'bn_norelu': _PLAIN_SHAPES, 'add': _PLAIN_SHAPES,
          'pool2': [(2, 4, 8, 8), (2, 4, 6, 10), (2, 4, 64, 64), (1, 4, 128, 128)],
          'pool3': [(2, 4, 8, 8), (2, 4, 7, 9), (2, 4, 40, 24)]}


def cases():
    """Every (op, pattern, train, shape) the two test files run; 'plain' is not a case of its own (it is each case's clean twin)."""
    return [(op, pattern, train, shape) for op in OPS for pattern in PATTERNS[1:] for train in (True, False)
            if applies(op, pattern, train) for shape in SHAPES[op]]


def case_id(c):
    op, pattern, train, shape = c
    return '%s-%s-%s-%s' % (op, pattern, 'train' if train else 'eval', 'x'.join(str(v) for v in shape))


def applies(op, pattern, train):
    """Whether `pattern` is defined for `op` in that mode."""
    if pattern in ('inf_x', 'zeros') and train:
        return False
    if pattern == 'nan_res':
        return op == 'add'
    if pattern == 'ties':
        return op in ('pool2', 'pool3')
    return True


def out_shape(op, shape):
    N, C, H, W = shape
    if op == 'pool2':
        return (N, C, H // 2, W // 2)
    if op == 'pool3':
        return (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    return shape


def _per_channel(kinds, C):
    return torch.tensor([kinds[c % 4] for c in range(C)], dtype=torch.float32)


def build(op, pattern, shape, seed=0):
    """The fp32 CPU inputs of one case: x, gy, res (op 'add'), gamma, beta, running_mean, running_var, and `poisoned`: the channels the
    pattern touches.  The same (op, shape, seed) gives the same tensors under every pattern but for the pattern's own elements."""
    N, C, H, W = shape
    assert C >= 4 and C % 4 == 0 and (pattern == 'plain' or applies(op, pattern, False))
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + N)
    x = torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3
    gy = torch.randn(out_shape(op, shape), generator=g)
    res = torch.randn(N, C, H, W, generator=g) if op == 'add' else None
    coarse = torch.randn(N, C, (H + 1) // 2, (W + 1) // 2, generator=g) * 1.5 + 0.3
    t = dict(gamma=_per_channel(KIND_GAMMA, C), beta=_per_channel(KIND_BETA, C), running_mean=_per_channel(KIND_RMEAN, C),
             running_var=_per_channel(KIND_RVAR, C), poisoned=[])
    h, w = H // 2, W // 2
    if pattern == 'nan_x':
        x[0, 0, h, w] = NAN
        t['poisoned'] = [0]
    elif pattern == 'inf_x':
        x[0, 0, h, w] = INF
        x[0, 1, h - 1, w - 1] = -INF
        t['poisoned'] = [0, 1]
    elif pattern == 'nan_gy':
        gy[0, 0, gy.shape[2] // 2, gy.shape[3] // 2] = NAN
        t['poisoned'] = [0]
    elif pattern == 'nan_res':
        res[0, 0, h, w] = NAN
        t['poisoned'] = [0]
    elif pattern == 'ties':
        if op == 'pool2':
            x = coarse.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)[:, :, :H, :W].contiguous()
        else:
            # a constant per plane, alternating around the channel's running mean from image to image: with N >= 2 the batch mean lies
            # between them, so xhat -- and with it z = bn(x) wherever gamma != 0 -- takes both signs, in eval mode as in training mode
            sign = torch.tensor([1.0 if n % 2 == 0 else -1.0 for n in range(N)]).view(N, 1, 1, 1)
            level = (0.75 + 0.5 * torch.rand(N, C, 1, 1, generator=g)) * sign + t['running_mean'].view(1, C, 1, 1)
            x = level.expand(N, C, H, W).contiguous()
    elif pattern == 'zeros':
        # powers of two: the stock eval-mode BatchNorm computes x * a + (beta - mean * a) with a fused multiply-add, which is exactly 0 at
        # x == mean only when mean * a is exact
        t['running_mean'] = _per_channel((0.5, -0.25, 2.0, 0.125), C)
        x = t['running_mean'].view(1, C, 1, 1).expand(N, C, H, W).contiguous()
        t['beta'] = torch.zeros(C)
        res = None if res is None else torch.zeros_like(res)
    t.update(x=x, gy=gy, res=res)
    return t


def _module(t, dtype, train):
    C = t['gamma'].numel()
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).to(dtype)
    with torch.no_grad():
        bn.weight.copy_(t['gamma'])
        bn.bias.copy_(t['beta'])
        bn.running_mean.copy_(t['running_mean'])
        bn.running_var.copy_(t['running_var'])
    return bn.train(train)


def stock(op, t, train, dtype=torch.float64):
    """The stock modules on the CPU in `dtype` (fp64: the arbiter): y, z (in front of the ReLU), act (the activation in front of the
    pool -- y itself without one), gx, gres, dgamma, dbeta, running_mean, running_var."""
    bn = _module(t, dtype, train)
    x = t['x'].detach().clone().to(dtype).requires_grad_(True)              # (leaves of their own: the case's tensors stay plain)
    res = t['res'].detach().clone().to(dtype).requires_grad_(True) if op == 'add' else None
    z = bn(x)
    if op == 'add':
        z = z + res
    act = z if op == 'bn_norelu' else torch.relu(z)
    y = F.max_pool2d(act, 2, 2) if op == 'pool2' else F.max_pool2d(act, 3, 2, 1) if op == 'pool3' else act
    y.backward(t['gy'].to(dtype))
    return dict(y=y.detach(), z=z.detach(), act=act.detach(), gx=x.grad, gres=None if res is None else res.grad, dgamma=bn.weight.grad,
                dbeta=bn.bias.grad, running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone())


def exclusions(ref, train):
    """(bool mask over x's elements, bool mask over channels) of what the backward comparison leaves out -- see the module docstring."""
    bad = ~torch.isfinite(ref['act'])
    chan = bad.any(dim=3).any(dim=2).any(dim=0)
    if train:
        bad = chan.view(1, -1, 1, 1).expand_as(bad).clone()
    return bad, chan


def cap_holds(t, ref, train):
    """The exclusion cap: nothing outside the poisoned channels is excluded, and without a poison in the forward nothing at all."""
    bad, chan = exclusions(ref, train)
    allowed = torch.zeros_like(chan)
    for c in t['poisoned']:
        allowed[c] = True
    if bool((chan & ~allowed).any()):
        return False
    # eval mode: one element per poisoned channel; training mode: those channels whole
    per = bad[0, 0].numel() * bad.shape[0] if train else 1
    return int(bad.sum()) <= per * len(t['poisoned'])


def windows(op, a):
    """The pooling windows of `a` unfolded: [N, C, k * k, windows]; MaxPool2d(3, 2, 1)'s padding reads -inf, as in torch."""
    N, C, H, W = a.shape
    k, s, p = (2, 2, 0) if op == 'pool2' else (3, 2, 1)
    if p:
        a = F.pad(a, (p, p, p, p), value=-INF)
    u = F.unfold(a.reshape(N * C, 1, *a.shape[2:]), k, stride=s)
    return u.view(N, C, k * k, -1)


# ---------------------------------------------------------------------------------------------------------------- PReLU
PRELU_PATTERNS = ('plain', 'nan_x', 'inf_x', 'nan_gy', 'nan_res', 'zeros')
PRELU_SLOPES = ('per_channel', 'shared', 'zero', 'negative')


def build_prelu(pattern, slopes, shape, with_res, seed=0):
    """x, gy, res (or None), alpha for F.prelu(x, alpha) [+ res].  zeros: x is +0 and -0 in a checkerboard."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(77 + 1000 * seed + H + W)
    x = torch.randn(N, C, H, W, generator=g)
    gy = torch.randn(N, C, H, W, generator=g)
    res = torch.randn(N, C, H, W, generator=g) if with_res else None
    alpha = {'per_channel': torch.linspace(-0.5, 0.75, C), 'shared': torch.tensor([0.25]), 'zero': torch.zeros(C),
             'negative': -torch.linspace(0.25, 1.0, C)}[slopes]
    h, w = H // 2, W // 2
    poisoned = [0]
    if pattern == 'nan_x':
        x[0, 0, h, w] = NAN
    elif pattern == 'inf_x':
        x[0, 0, h, w] = INF
        x[0, 1, h - 1, w - 1] = -INF
        poisoned = [0, 1]
    elif pattern == 'nan_gy':
        gy[0, 0, h, w] = NAN
    elif pattern == 'nan_res':
        assert with_res
        res[0, 0, h, w] = NAN
    elif pattern == 'zeros':
        board = (torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % 2
        x = torch.where(board.bool(), torch.tensor(-0.0), torch.tensor(0.0)).expand(N, C, H, W).contiguous()
        poisoned = []
    else:
        poisoned = []
    return dict(x=x, gy=gy, res=res, alpha=alpha, poisoned=poisoned)


def stock_prelu(t, dtype=torch.float64):
    x = t['x'].detach().clone().to(dtype).requires_grad_(True)
    a = t['alpha'].detach().clone().to(dtype).requires_grad_(True)
    res = None if t['res'] is None else t['res'].detach().clone().to(dtype).requires_grad_(True)
    y = F.prelu(x, a)
    if res is not None:
        y = res + y
    y.backward(t['gy'].to(dtype))
    return dict(y=y.detach(), gx=x.grad, galpha=a.grad, gres=None if res is None else res.grad)


# ---------------------------------------------------------------------------------------------------------------- comparisons
def same_nonfinite(got, ref):
    """NaN at the same positions, +Inf at the same positions, -Inf at the same positions."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    return (bool((torch.isnan(got) == torch.isnan(ref)).all()) and bool((torch.isposinf(got) == torch.isposinf(ref)).all())
            and bool((torch.isneginf(got) == torch.isneginf(ref)).all()))


def finite_err(got, ref, skip=None):
    """max |got - ref| / max |ref| over the positions where ref is finite and `skip` is False (0.0 over no positions; inf when the
    scale is 0 and anything differs) -- err() of tests/test_loss_heads_gpu.py on those positions."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    m = torch.isfinite(ref)
    if skip is not None:
        m = m & ~skip
    if not bool(m.any()):
        return 0.0
    diff, scale = float((got[m] - ref[m]).abs().max()), float(ref[m].abs().max())
    if diff != diff:
        return INF
    if scale == 0.0:
        return 0.0 if diff == 0.0 else INF
    return diff / scale
