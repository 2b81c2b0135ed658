"""Reference networks and the situation driver of tests/test_autograd_contract_{host,gpu}.py.

Three small topologies exist twice, built from one seed with identical parameters and identical parameter names:

    the library net     SharableConv2d / SharableLinear / HeadLinear, FusedSequential, the blocks of models/resnet.py and the free functions
                        of models/fused_bn.py (needs the HIP device to run, not to be built);
    the reference net   stock torch.nn modules on the CPU, evaluated in float64 (the reference) and in float32 (the yardstick of
                        the bound: what stock torch loses to fp32 round-off on the same tensor).

A piggymask is restated in plain autograd: the effective weight is w * (pm > thr), gW = g_eff * bin(pm), gPM = g_eff * w.

run() puts either kind of net into one of the situations S0 .. S10 (frozen parameters, partial backward passes, a retained graph, gradient
accumulation, two live graphs, eval mode under autograd, a no_grad forward, non-dense tensors) and returns every tensor the situation
defines, by name.  reference() runs the float64 and the float32 reference, and reports the float64 run's conditioning margin: the
smallest |pre-activation| over every ReLU / PReLU input and the smallest gap between the two largest values of every max-pool window.
The comparisons only mean something at smooth points (one flipped ReLU mask moves a gradient by per cent), so the seeds below were
searched on the CPU for a margin of at least MARGIN = 2e-5, about twenty times the fp32 round-off of a pre-activation of order one;
tests/test_autograd_contract_host.py asserts that margin for every entry.  No element is ever masked out of a comparison.
"""
import copy
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

THR = 5e-3                  # the library's DEFAULT_THRESHOLD
MARGIN = 2e-5
B_FLOOR = 1e-5              # the bar test_bn_backward_hint_is_used_and_matches_fp64 holds for conv -> BN -> ReLU -> conv against fp64
B_FACTOR = 8.0              # ... or eight times stock fp32 torch's own error on the tensor (other summation order, Winograd transforms)
STAT_RTOL, STAT_ATOL = 1e-5, 1e-6

TOPOLOGIES = ('A', 'B_identity', 'B_down', 'B_basic', 'C')
SITUATIONS = ('S0a', 'S0b', 'S1', 'S2', 'S3', 'S4', 'S5', 'S6', 'S7', 'S8', 'S9', 'S10')

# (topology, situation) -> seed with a conditioning margin >= MARGIN, found by search_seeds() on the CPU.  S0a, S0b, S1, S2, S3, S4, S5 and
# S9 see the same activations (first micro-batch, train mode) and share the topology's 'train' seed; S6 and S7 also run the second
# micro-batch, S8 normalises with the running statistics, S10 feeds the strided view.
_SAME_AS_TRAIN = ('S0a', 'S0b', 'S1', 'S2', 'S3', 'S4', 'S5', 'S9')
_SEED_TABLE = {
    'A': {'train': 11, 'two': 686, 'eval': 6, 'view': 13},
    'B_identity': {'train': 3, 'two': 3, 'eval': 4, 'view': 3},
    'B_down': {'train': 0, 'two': 0, 'eval': 0, 'view': 0},
    'B_basic': {'train': 1, 'two': 1, 'eval': 1, 'view': 1},
    'C': {'train': 8, 'two': 8, 'eval': 8, 'view': 4},
}


def seed_class(sit):
    return 'train' if sit in _SAME_AS_TRAIN else {'S6': 'two', 'S7': 'two', 'S8': 'eval', 'S10': 'view'}[sit]


def seed_of(topo, sit):
    return _SEED_TABLE[topo][seed_class(sit)]


# ------------------------------------------------------------------------------------------------- reference layers (stock torch.nn)
def _masked(weight, pm):
    """w * bin(pm) with the straight-through gradient written out: the value of `b + (pm - pm.detach())` is b exactly, its derivative
    with respect to pm is one, so autograd returns gW = g_eff * b and gPM = g_eff * w."""
    if pm is None:
        return weight
    b = (pm.detach() > THR).to(weight.dtype)
    return weight * (b + (pm - pm.detach()))


class RefConv2d(nn.Conv2d):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.piggymask = None

    def forward(self, x):
        return self._conv_forward(x, _masked(self.weight, self.piggymask), self.bias)


class RefLinear(nn.Linear):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.piggymask = None

    def forward(self, x):
        return F.linear(x, _masked(self.weight, self.piggymask), self.bias)


class RefBottleneck(nn.Module):
    """torchvision's Bottleneck, which models/resnet.py restates (names as there)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = RefConv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = RefConv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = RefConv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU()
        self.downsample = downsample

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class RefBasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = RefConv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU()
        self.conv2 = RefConv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


# ------------------------------------------------------------------------------------------------- the topologies
def _planes(feat, plane_w):
    """S10 on B and C: the block output is consumed through a transpose (times a fixed, non-symmetric plane of weights, so that the
    gradient that comes back is a dense tensor seen through the transpose: non-contiguous)."""
    return feat if plane_w is None else feat.transpose(2, 3) * plane_w


class NetA(nn.Module):
    """VGG-like: conv(3->64) BN ReLU, conv(64->128) BN ReLU, conv(128->128) BN ReLU MaxPool(2, 2), View, linear(128*7*7 -> 10) in ONE
    (Fused)Sequential.  On 3 x 3 x 14 x 14: the fused stem (input without a gradient), the weight-gradient rider pairs (3, 64, 14, 14, 128)
    -- BatchNorm seq.1 in conv seq.3, only when the stem does not fuse: the fused stem runs its own BatchNorm backward -- and
    (3, 128, 14, 14, 128) -- BatchNorm seq.4 in conv seq.6 --, fused statistics, the pooled BatchNorm.  The first conv and the linear
    layer carry a piggymask, the convs in the middle do not."""
    x_shape = (3, 3, 14, 14)
    x_grad = False              # the default of the situations that do not say (the stem only fuses without an input gradient)
    classes = 10

    def __init__(self, lib):
        super().__init__()
        if lib:
            from cpg_amd.models import fused_bn, layers as nl
            from cpg_amd.models.vgg import View
            conv, lin, seq, flat = nl.SharableConv2d, nl.SharableLinear, fused_bn.FusedSequential, View(-1, 128 * 7 * 7)
        else:
            conv, lin, seq, flat = RefConv2d, RefLinear, nn.Sequential, nn.Flatten()
        mods, cin = [], 3
        for c in (64, 128, 128):
            mods += [conv(cin, c, 3, padding=1, bias=False), nn.BatchNorm2d(c), nn.ReLU(inplace=bool(lib))]
            cin = c
        mods += [nn.MaxPool2d(2, 2), flat, lin(128 * 7 * 7, self.classes)]
        self.seq = seq(*mods)
        self.masked = ['seq.0', 'seq.11']

    def forward(self, x, plane_w=None):
        return self.seq(x)

    def subsets(self):
        """S4: one middle conv's weight alone (the host of a rider with and without the fused stem); that weight and the weight of the
        BatchNorm below it; the head alone."""
        return [['seq.6.weight'], ['seq.6.weight', 'seq.4.weight'], ['seq.11.weight', 'seq.11.bias']]


class NetB(nn.Module):
    """One residual block of models/resnet.py, the mean over the plane, a HeadLinear."""
    x_grad = True               # a block's input is an activation: it needs its gradient (the skip epilogue only fuses then)
    classes = 10
    KINDS = {'B_identity': ('Bottleneck', 64, 16, 1, (4, 64, 8, 8)),        # 16-divisible: conv_bn_act_skip's skip-add epilogue
             'B_down': ('Bottleneck', 32, 16, 2, (4, 32, 8, 8)),            # stride 2, conv1x1 -> BN downsample (the lone BatchNorm)
             'B_basic': ('BasicBlock', 16, 16, 1, (4, 16, 8, 8))}

    def __init__(self, lib, kind):
        super().__init__()
        block, inplanes, planes, stride, self.x_shape = self.KINDS[kind]
        if lib:
            from cpg_amd.models import fused_bn, layers as nl, resnet
            cls, seq, head, c1 = getattr(resnet, block), fused_bn.FusedSequential, nl.HeadLinear, resnet.conv1x1
        else:
            cls, seq, head = {'Bottleneck': RefBottleneck, 'BasicBlock': RefBasicBlock}[block], nn.Sequential, nn.Linear
            c1 = lambda i, o, s: RefConv2d(i, o, 1, s, bias=False)
        out_planes = planes * cls.expansion
        down = None
        if stride != 1 or inplanes != out_planes:
            down = seq(c1(inplanes, out_planes, stride), nn.BatchNorm2d(out_planes))
        self.block = cls(inplanes, planes, stride, down)
        self.head = head(out_planes, self.classes)
        self.masked = ['block.conv1', 'block.conv2']
        self.kind = kind

    def forward(self, x, plane_w=None):
        return self.head(_planes(self.block(x), plane_w).mean((2, 3)))

    def subsets(self):
        return [['block.conv2.weight'], ['block.conv2.weight', 'block.bn1.weight'], ['head.weight', 'head.bias']]


class NetC(nn.Module):
    """What models/spherenet.py:105-110 does for one stage: conv_prelu (3x3 s2, bias), then one residual unit -- conv_prelu_skip and
    conv_prelu(..., res=skip) (3x3 s1, bias, per-channel PReLU) --, the flattened map, a HeadLinear.  64 channels on 14 x 14 maps."""
    x_shape = (3, 3, 28, 28)
    x_grad = True
    classes = 10

    def __init__(self, lib):
        super().__init__()
        self.lib = lib
        if lib:
            from cpg_amd.models import layers as nl
            conv, head = nl.SharableConv2d, nl.HeadLinear
        else:
            conv, head = RefConv2d, nn.Linear
        self.conv1, self.relu1 = conv(3, 64, 3, 2, 1), nn.PReLU(64)
        self.conv2, self.relu2 = conv(64, 64, 3, 1, 1), nn.PReLU(64)
        self.conv3, self.relu3 = conv(64, 64, 3, 1, 1), nn.PReLU(64)
        self.head = head(64 * 14 * 14, self.classes)
        self.masked = ['conv3']

    def forward(self, x, plane_w=None):
        if self.lib:
            from cpg_amd.models.fused_bn import conv_prelu, conv_prelu_skip
            x = conv_prelu(self.conv1, self.relu1, x)
            y, skip = conv_prelu_skip(self.conv2, self.relu2, x)
            x = conv_prelu(self.conv3, self.relu3, y, res=skip)
        else:
            x = self.relu1(self.conv1(x))
            x = x + self.relu3(self.conv3(self.relu2(self.conv2(x))))
        return self.head(_planes(x, plane_w).reshape(x.shape[0], -1))

    def subsets(self):
        # (no BatchNorm here: the activation below the middle conv is a PReLU)
        return [['conv2.weight'], ['conv2.weight', 'relu1.weight'], ['head.weight', 'head.bias']]


EXTRA_TOPOLOGIES = {}       # name -> class(lib): topologies that other modules add (tests/_train_loop.py: the mini ResNet 'R')


def _new(topo, lib):
    if topo in EXTRA_TOPOLOGIES:
        return EXTRA_TOPOLOGIES[topo](lib)
    if topo == 'A':
        return NetA(lib)
    if topo == 'C':
        return NetC(lib)
    return NetB(lib, topo)


def _is_matrix_weight(name, p):
    return name.endswith('weight') and p.dim() >= 2


def build_reference(topo, seed):
    """The float32 reference net of `topo`, initialised from `seed` at a well-conditioned point (He-normal convs, BatchNorm weights in
    [0.5, 1.5], non-trivial running statistics, PReLU slopes in [0.1, 0.4], piggymasks rand * 0.012 around the 5e-3 threshold)."""
    g = torch.Generator().manual_seed(seed)
    net = _new(topo, False)
    mods = dict(net.named_modules())
    for name in net.masked:
        mods[name].piggymask = nn.Parameter(torch.rand(mods[name].weight.shape, generator=g) * 0.012)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]       # (pre-activations of order one in eval mode too)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.0 / m.weight.shape[1]) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            elif isinstance(m, nn.PReLU):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.3 + 0.1)
    return net


def build_library(topo, ref32, device):
    """The library net of `topo` with the parameters and buffers of `ref32` (strict: the names must agree)."""
    net = _new(topo, True)
    mods = dict(net.named_modules())
    for name, m in ref32.named_modules():        # a piggymask wherever the reference has one (build_reference: the layers of net.masked)
        if getattr(m, 'piggymask', None) is not None:
            mods[name].piggymask = nn.Parameter(torch.zeros(mods[name].weight.shape))
    net.load_state_dict(ref32.state_dict(), strict=True)
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in ref32.named_parameters()]
    return net.to(device)


def make_data(topo, seed):
    """Two micro-batches, the big tensor whose every second pixel is S10's input, and S10's plane of weights (CPU, float32)."""
    net = _new(topo, False)
    N, C, H, W = net.x_shape
    g = torch.Generator().manual_seed(seed + 7919)
    oh = {'A': 14, 'C': 14, 'B_down': 4}.get(topo, 8)          # the map the block hands on
    return {'x1': torch.randn(N, C, H, W, generator=g), 't1': torch.randint(0, net.classes, (N,), generator=g),
            'x2': torch.randn(N, C, H, W, generator=g), 't2': torch.randint(0, net.classes, (N,), generator=g),
            'xbig': torch.randn(N, C, 2 * H, 2 * W, generator=g),
            'plane_w': None if topo == 'A' else torch.rand(oh, oh, generator=g) + 0.5,
            'x_grad': net.x_grad}


# ------------------------------------------------------------------------------------------------- the situations
def _freeze(net, what):
    for name, p in net.named_parameters():
        if what == 'all' or (what == 'weights' and _is_matrix_weight(name, p)):
            p.requires_grad_(False)
    if what == 'norm':
        for m in net.modules():
            if isinstance(m, (nn.BatchNorm2d, nn.PReLU)):
                for p in m.parameters():
                    p.requires_grad_(False)


def run(net, sit, data, device='cpu', dtype=torch.float32, mark=None):
    """Put `net` (library or reference: the same code drives both) into situation `sit` and return {name: tensor or None}:
    'out...' outputs, 'grad:<parameter>' / 'grad:x' gradients (None where none may exist), 'buf:<buffer>' running statistics and
    counters afterwards.  mark(label), when given, is called between the phases ('forward', 'backward', 'backward2', ...) so that a
    test can tell which kernels ran in which."""
    mark = mark or (lambda label: None)
    res = {}
    params = dict(net.named_parameters())
    cv = lambda t: None if t is None else t.to(device=device, dtype=dtype if t.is_floating_point() else t.dtype)
    x1, x2, t1, t2 = cv(data['x1']), cv(data['x2']), cv(data['t1']), cv(data['t2'])
    want_x = data['x_grad']

    def keep(t):
        return None if t is None else t.detach().clone()

    def grads(tag=''):
        for n, p in params.items():
            res[tag + 'grad:' + n] = keep(p.grad)

    def buffers(tag=''):
        for n, b in net.named_buffers():
            res[tag + 'buf:' + n] = keep(b)

    def loss_of(x, t):
        out = net(x)
        return out, F.cross_entropy(out, t)

    net.train()
    if sit in ('S0a', 'S0b', 'S1', 'S2', 'S9'):
        _freeze(net, {'S1': 'weights', 'S2': 'norm'}.get(sit, 'none'))
        if sit == 'S9':
            mark('nograd')
            with torch.no_grad():
                res['dry:out'] = keep(net(x1))
            buffers('dry:')
        x = x1.clone().requires_grad_({'S0a': False, 'S0b': True}.get(sit, want_x))
        mark('forward')
        out, loss = loss_of(x, t1)
        mark('backward')
        loss.backward()
        res['out'], res['grad:x'] = keep(out), keep(x.grad)
    elif sit == 'S3':
        _freeze(net, 'all')
        x = x1.clone().requires_grad_(True)
        mark('forward')
        out, loss = loss_of(x, t1)
        mark('backward')
        gx, = torch.autograd.grad(loss, x)
        res['out'], res['grad:x'] = keep(out), keep(gx)
    elif sit == 'S4':
        for k, names in enumerate(net.subsets()):
            net.zero_grad(set_to_none=True)
            x = x1.clone().requires_grad_(want_x)
            mark('forward%d' % k)
            out, loss = loss_of(x, t1)
            mark('backward%d' % k)
            loss.backward(inputs=[params[n] for n in names], retain_graph=True)
            grads('%d:' % k)
            res['%d:grad:x' % k] = keep(x.grad)
            mark('grad%d' % k)
            got = torch.autograd.grad(loss, [params[n] for n in names])
            for n, gv in zip(names, got):
                res['%d:ag:grad:%s' % (k, n)] = keep(gv)
            res['%d:out' % k] = keep(out)
        net.zero_grad(set_to_none=True)
    elif sit == 'S5':
        x = x1.clone().requires_grad_(want_x)
        mark('forward')
        out, loss = loss_of(x, t1)
        mark('backward')
        loss.backward(retain_graph=True)
        mark('backward2')
        loss.backward()
        res['out'], res['grad:x'] = keep(out), keep(x.grad)
    elif sit == 'S6':
        xa, xb = x1.clone().requires_grad_(want_x), x2.clone().requires_grad_(want_x)
        for tag, x, t in (('', xa, t1), ('second:', xb, t2)):
            mark('forward')
            out, loss = loss_of(x, t)
            mark('backward')
            loss.backward()
            res[tag + 'out'], res[tag + 'grad:x'] = keep(out), keep(x.grad)
    elif sit == 'S7':
        xa, xb = x1.clone().requires_grad_(want_x), x2.clone().requires_grad_(want_x)
        mark('forward')
        oa, la = loss_of(xa, t1)
        ob, lb = loss_of(xb, t2)
        mark('backward')
        (la + lb).backward()
        res['out'], res['second:out'], res['grad:x'], res['second:grad:x'] = keep(oa), keep(ob), keep(xa.grad), keep(xb.grad)
    elif sit == 'S8':
        net.eval()
        buffers('before:')
        x = x1.clone().requires_grad_(want_x)
        mark('forward')
        out, loss = loss_of(x, t1)
        mark('backward')
        loss.backward()
        res['out'], res['grad:x'] = keep(out), keep(x.grad)
    elif sit == 'S10':
        xbig = cv(data['xbig']).requires_grad_(want_x)
        mark('forward')
        out = net(xbig[:, :, ::2, ::2], cv(data['plane_w']))
        mark('backward')
        out.sum().backward()                        # an expanded, stride-0 upstream gradient
        res['out'], res['grad:x'] = keep(out), keep(xbig.grad)
    else:
        raise ValueError(sit)
    mark('done')
    if sit != 'S4':
        grads()
    buffers()
    return res


# ------------------------------------------------------------------------------------------------- margin, reference, bound
class Margin(object):
    """Forward pre-hooks on every ReLU / PReLU / MaxPool2d of a reference net: the smallest |pre-activation| and the smallest gap between
    the two largest values of a pooling window (taken on the ReLU's INPUT: ReLU and max commute, and two clipped zeros tie without
    carrying any gradient).  MaxPool2d(2, 2) and the overlapping MaxPool2d(3, 2, 1) (padded with -inf, as the pool pads; there a window
    whose maximum the ReLU clips carries no gradient and does not count).  trace=True also keeps every tensor the margin was taken over,
    in call order: ('act', module name, pre-activation) and ('pool', module name, window gaps, +inf where a window does not count)."""

    def __init__(self, net, trace=False):
        self.value, self.count, self._pre = float('inf'), 0, None
        self.trace = [] if trace else None
        self._names = {m: n for n, m in net.named_modules()}
        for m in net.modules():
            if isinstance(m, (nn.ReLU, nn.PReLU)):
                m.register_forward_pre_hook(self._act)
            elif isinstance(m, nn.MaxPool2d):
                m.register_forward_pre_hook(self._pool)

    def _act(self, mod, args):
        x = args[0].detach()
        self._pre = x
        self.count += x.numel()
        self.value = min(self.value, float(x.abs().min()))
        if self.trace is not None:
            self.trace.append(('act', self._names[mod], x))

    def _pool(self, mod, args):
        pre = self._pre
        k, s, p = mod.kernel_size, mod.stride, mod.padding
        assert pre is not None and pre.shape == args[0].shape and (k, s, p) in ((2, 2, 0), (3, 2, 1))
        win = F.pad(pre, (p, p, p, p), value=float('-inf')).unfold(2, k, s).unfold(3, k, s).reshape(*pre.shape[:2], -1, k * k)
        top = win.topk(2, dim=-1).values
        gap = top[..., 0] - top[..., 1]
        if k == 3:
            gap = torch.where(top[..., 0] > 0, gap, torch.full_like(gap, float('inf')))
        self.count += int(torch.isfinite(gap).sum())
        self.value = min(self.value, float(gap.min()))
        if self.trace is not None:
            self.trace.append(('pool', self._names[mod], gap))


@functools.lru_cache(maxsize=None)
def reference(topo, sit, seed):
    """(float64 results, float32 results, margin of the float64 run, number of activations / windows the margin is over) of the
    reference net in one situation.  Cached: the tensors are shared between tests and must not be written to."""
    ref32 = build_reference(topo, seed)
    data = make_data(topo, seed)
    ref64 = copy.deepcopy(ref32).double()
    margin = Margin(ref64)
    r64 = run(ref64, sit, data, 'cpu', torch.float64)
    r32 = run(copy.deepcopy(ref32), sit, data, 'cpu', torch.float32)
    return r64, r32, margin.value, margin.count


def base_name(name):
    """'1:ag:grad:seq.3.weight' -> 'grad:seq.3.weight': the tensor of S0 a situation's tensor corresponds to."""
    for key in ('grad:', 'buf:', 'out'):
        at = name.find(key)
        if at >= 0:
            return name[at:]
    return name


def _is_stat(name):
    return 'buf:' in name


def _rel32(name, r64, r32):
    a, b = r64.get(name), r32.get(name)
    if a is None or b is None or not a.is_floating_point():
        return None
    sc = float(a.abs().max())
    return float((b.double() - a).abs().max()) / sc if sc > 0 else 0.0


def bounds(topo, sit, seed):
    """{name: b} for every floating-point output and gradient of the situation: b = max(1e-5, 8 x stock fp32's relative error on that
    tensor), and never looser than the bound of the corresponding tensor in S0 of the topology (S0a / S0b, whichever has it)."""
    r64, r32, _, _ = reference(topo, sit, seed)
    s0 = {}
    for s in ('S0a', 'S0b'):
        a64, a32, _, _ = reference(topo, s, seed_of(topo, s))
        for n in a64:
            e = _rel32(n, a64, a32)
            if e is not None and not _is_stat(n):
                s0[n] = min(s0.get(n, float('inf')), max(B_FLOOR, B_FACTOR * e))
    out = {}
    for n in r64:
        e = _rel32(n, r64, r32)
        if e is None or _is_stat(n):
            continue
        out[n] = min(max(B_FLOOR, B_FACTOR * e), s0.get(base_name(n), float('inf')))
    return out


def compare(got, topo, sit, seed, log=print):
    """Every tensor of the situation against the float64 reference; returns the list of misses (empty: all within bounds).  Each figure
    is logged before anything is judged."""
    r64, _, _, _ = reference(topo, sit, seed)
    bnd = bounds(topo, sit, seed)
    bad = []
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    for n in sorted(r64):
        want, have = r64[n], got[n]
        if want is None or have is None:
            log('%s %s %s: reference %s, got %s' % (topo, sit, n, 'None' if want is None else 'tensor', 'None' if have is None else 'tensor'))
            if (want is None) != (have is None):
                bad.append((n, 'None mismatch'))
            continue
        have = have.detach().cpu()
        if tuple(have.shape) != tuple(want.shape):
            bad.append((n, 'shape %s vs %s' % (tuple(have.shape), tuple(want.shape))))
            continue
        if not want.is_floating_point():
            log('%s %s %s: %s (reference %s)' % (topo, sit, n, have.tolist(), want.tolist()))
            if not torch.equal(have, want):
                bad.append((n, 'counter %s vs %s' % (have.tolist(), want.tolist())))
            continue
        err = (have.double() - want).abs()
        if _is_stat(n):
            over = float((err - (STAT_ATOL + STAT_RTOL * want.abs())).max())
            log('%s %s %s: max err %.3g, worst excess over atol + rtol |ref| %.3g' % (topo, sit, n, float(err.max()), over))
            if not over <= 0:
                bad.append((n, 'running statistic off by %.3g' % float(err.max())))
            continue
        sc = float(want.abs().max())
        e = float(err.max())
        log('%s %s %s: max err %.3g = %.3g of max|ref| %.3g (bound %.3g)' % (topo, sit, n, e, e / sc if sc else float('nan'), sc, bnd[n]))
        if not e <= bnd[n] * sc:
            bad.append((n, 'err %.3g of scale, bound %.3g' % (e / sc if sc else float('inf'), bnd[n])))
    return bad


def search_seeds(topo, cls, first=0, count=64):
    """Development aid (python -c 'import _autograd_ref as r; print(r.search_seeds("A", "train"))'): the seeds in [first, first + count)
    whose margin reaches MARGIN in every situation of the class."""
    sits = {'train': ('S0b',), 'two': ('S7',), 'eval': ('S8',), 'view': ('S10',)}[cls]
    ok = []
    for seed in range(first, first + count):
        if all(reference(topo, s, seed)[2] >= MARGIN for s in sits):
            ok.append(seed)
        reference.cache_clear()
    return ok


# ------------------------------------------------------------------------------------------------- off-centre channels
# Train-mode conv -> BatchNorm -> ReLU whose statistics come from the conv epilogue's fp32 {sum y, sum y^2} partial sums over at most 448
# outputs, merged as E[y^2] - mean^2 (k_bn_finalize_tiles): that formula loses |mean|^2 / var of its precision.  The cases have few tiles
# per channel (little averages out) and channels whose |mean| / std runs from about 0 to RATIO_MAX.
RATIO_MAX = 8.0
STAT_BOUND = 1e-4           # batch mean within 1e-4 std, invstd within 1e-4 relative (the project's target up to ratio 10, see the host test)
OFFCENTRE = {               # kind: (N, C, H, W, K, kernel, seed)
    'pointwise': (5, 32, 7, 7, 48, 1, 6),
    '3x3': (2, 8, 10, 12, 24, 3, 4),
    'stem': (3, 3, 14, 14, 64, 3, 9),
}


def _channel_stats(y):
    var, mean = torch.var_mean(y, dim=(0, 2, 3), unbiased=False)
    return mean, var


@functools.lru_cache(maxsize=None)
def offcentre(kind):
    """Inputs (float32, CPU) and the float64 / stock float32 results of one off-centre case.  The input carries a per-channel offset;
    the random weights are projected so that an un-padded output is centred, then output channel k gets a positive offset on its centre
    tap, solved (in float64) for |mean| / std = RATIO_MAX * k / (K - 1)."""
    N, C, H, W, K, R, seed = OFFCENTRE[kind]
    g = torch.Generator().manual_seed(seed)
    off = torch.linspace(0.5, 1.5, C, dtype=torch.float64)
    sigma = C ** 0.5 / 16.0                                       # (a channel of centre-tap offset alone sits at |mean| / std = 16)
    x = (off.view(1, C, 1, 1) + sigma * torch.randn(N, C, H, W, generator=g, dtype=torch.float64)).float()
    w0 = torch.randn(K, C, R, R, generator=g, dtype=torch.float64) * (1.0 / (C * R * R)) ** 0.5
    offw = off.view(1, C, 1, 1).expand(K, C, R, R)
    w0 = w0 - offw * ((w0 * offw).sum((1, 2, 3), keepdim=True) / (offw * offw).sum((1, 2, 3), keepdim=True))
    unit = torch.zeros(1, C, R, R, dtype=torch.float64)
    unit[:, :, R // 2, R // 2] = 1.0
    x64 = x.double()
    y0, y1 = F.conv2d(x64, w0, padding=R // 2), F.conv2d(x64, unit, padding=R // 2)
    m1, v1 = float(y1.mean()), float(y1.var(unbiased=False))
    delta = torch.zeros(K, dtype=torch.float64)
    for k in range(K):
        yk = y0[:, k:k + 1]
        m0, v0 = float(yk.mean()), float(yk.var(unbiased=False))
        c01 = float(((yk - m0) * (y1 - m1)).mean())
        ratio = lambda d: abs(m0 + d * m1) / (v0 + 2 * d * c01 + d * d * v1) ** 0.5
        target, lo, hi = RATIO_MAX * k / (K - 1), 0.0, 64.0
        if ratio(0.0) < target:
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if ratio(mid) < target else (lo, mid)
            delta[k] = hi
    w = (w0 + delta.view(K, 1, 1, 1) * unit).float()
    gamma = (torch.rand(K, generator=g) + 0.5)
    beta = (torch.rand(K, generator=g) - 0.5)
    gz = torch.randn(N, K, H, W, generator=g)
    case = {'x': x, 'w': w, 'gamma': gamma, 'beta': beta, 'gz': gz, 'kernel': R, 'x_grad': kind != 'stem', 'delta': delta}
    for dtype, tag in ((torch.float64, 'r64'), (torch.float32, 'r32')):
        xr = x.clone().to(dtype).requires_grad_(case['x_grad'])          # (clone: .to() of a float32 tensor is the tensor itself)
        wr = w.clone().to(dtype).requires_grad_(True)
        bn = nn.BatchNorm2d(K).to(dtype).train()
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
        y = F.conv2d(xr, wr, padding=R // 2)
        pre = bn(y)
        z = torch.relu(pre)
        (z * gz.to(dtype)).sum().backward()
        mean, var = _channel_stats(y.detach())
        case[tag] = {'out': z.detach(), 'grad:x': None if xr.grad is None else xr.grad.detach(), 'grad:w': wr.grad.detach(),
                     'grad:gamma': bn.weight.grad.detach(), 'grad:beta': bn.bias.grad.detach(),
                     'buf:running_mean': bn.running_mean.detach().clone(), 'buf:running_var': bn.running_var.detach().clone(),
                     'mean': mean, 'std': var.sqrt(), 'invstd': torch.rsqrt(var + bn.eps), 'ratio': mean.abs() / var.sqrt(),
                     'margin': float(pre.detach().abs().min())}
    return case


def two_sums_invstd_error(ratio, n=448, seed=0):
    """The relative invstd error of the epilogue's formula in its least favourable order: ONE tile of n outputs, sum y and sum y^2
    accumulated strictly sequentially in float32, merged in float64 as E[y^2] - mean^2."""
    import numpy as np
    rng = np.random.RandomState(seed)
    y = (rng.standard_normal(n) + ratio).astype(np.float32)
    s = np.cumsum(y, dtype=np.float32)[-1]
    q = np.cumsum(y * y, dtype=np.float32)[-1]
    mean = float(s) / n
    var = max(float(q) / n - mean * mean, 0.0)
    y64 = y.astype(np.float64)
    true = 1.0 / np.sqrt(y64.var() + 1e-5)
    return abs(1.0 / np.sqrt(var + 1e-5) - true) / true
