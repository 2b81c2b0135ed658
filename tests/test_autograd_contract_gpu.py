"""The fused layers under real autograd use, against float64 (tests/_autograd_ref.py: the reference, its conditioning margin, the bound).

Every other training-path test runs the autograd glue of models/layers.py and models/fused_bn.py in one situation: all parameters
trainable, one forward, one backward(), a contiguous upstream gradient, a fresh leaf as input.  The glue chooses its kernels by exactly
what that leaves out (ctx.needs_input_grad, one-shot hand-offs between Functions -- BnBwdHint, BiasGradSink, the packed operand --,
x.requires_grad, None gradients).  Here three small topologies run in situations S0 .. S10 on the library and on stock torch.nn in
float64, and outputs, every gradient that should exist (and the absence of every one that should not), running statistics and counters
are compared.  Per tensor: max|got - ref| <= b max|ref| with b = max(1e-5, 8 x stock fp32 torch's error on that tensor), never looser
than S0's; running statistics rtol 1e-5 / atol 1e-6; counters exactly.

A situation test is worth nothing if the fast path silently declined, so each case also says which entry points ran in which phase
(a recorder over _lib.call and a counting wrapper over layers._bn_bwd_rider).

One statement about PyTorch the assertions rest on: ctx.needs_input_grad of a custom Function is fixed when the forward runs; neither
backward(inputs=...) nor torch.autograd.grad changes it per call (torch 2.10).  Frozen parameters (S1 - S3) therefore switch the
weight-gradient calls, the rider and the stem's weight gradient off; a partial backward (S4) does not: the conv that hosts a rider still
computes both of its gradients, the rider's result is simply not taken when the BatchNorm's node is not part of that pass.  What S4
asserts instead is that a SECOND pass over the same graph finds the hand-offs consumed and takes the stand-alone kernels.

The off-centre tests pin the range in which the fused BatchNorm statistics (fp32 {sum, sum of squares} partials merged as
E[y^2] - mean^2) hold 1e-4: channels with |mean| / std from 0 to 8 (measured: batch mean within 7e-7 std, invstd within 4e-6).  The
stand-alone pass is held to 1e-6 at ratio 1000 on invstd; its batch mean is a float32 OUTPUT, so that one is held to 1e-6 std plus half
a float32 ulp of the mean itself (3e-5 std at ratio 1000: the format's, not the kernel's).  That test found k_bn_stats squaring and
summing in fp32 between its fp64 folds: invstd off by 1.4e-3 at ratio 800, the output by 1.1e-3 of its scale; with both sums in fp64
from the first term: 5e-8 and 6e-6.  No bound differs from the ones above.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _autograd_ref as R

from cpg_amd import _lib
from cpg_amd.models import fused_bn
from cpg_amd.models import layers as nl

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [(t, s) for t in R.TOPOLOGIES for s in R.SITUATIONS]


class Probe(object):
    """Which entry points of the library ran, and whether the rider did, per phase of the situation driver."""

    def __init__(self, monkeypatch):
        self.phase, self.calls, self.riders = 'setup', [], []
        real_call, real_rider = _lib.call, nl._bn_bwd_rider

        def call(name, *args):
            self.calls.append((self.phase, name))
            return real_call(name, *args)

        def rider(*args, **kw):
            r = real_rider(*args, **kw)
            self.riders.append((self.phase, r is not None))
            return r
        monkeypatch.setattr(_lib, 'call', call)
        monkeypatch.setattr(nl, '_bn_bwd_rider', rider)

    def mark(self, label):
        self.phase = label

    def n(self, name, phase=None):
        return sum(1 for p, c in self.calls if c == name and (phase is None or p == phase))

    def rode(self, phase=None):
        return [ok for p, ok in self.riders if phase is None or p == phase]

    def summary(self):
        out = {}
        for p, c in self.calls:
            out.setdefault(p, {}).setdefault(c, 0)
            out[p][c] += 1
        return out


@pytest.fixture
def probe(monkeypatch):
    return Probe(monkeypatch)


def _paths_a(sit, p):
    stem = p.n('cpg_stem_bn_stats', 'forward')
    if sit in ('S0a', 'S1', 'S2', 'S5', 'S9', 'S10'):
        # the input needs no gradient: fused stem (its own BatchNorm backward and, unless everything it owns is frozen, weight gradient)
        assert stem == 1 and p.n('cpg_stem_bn_relu_bwd_reduce', 'backward') == 1 and p.n('cpg_stem_bn_relu_bwd_wgrad', 'backward') == 1
        assert p.n('cpg_conv2d_fwd_bnstats', 'forward') == 2 and p.n('cpg_bn_relu_pool_fwd', 'forward') == 1
    if sit in ('S0a', 'S2', 'S9', 'S10'):
        assert p.rode('backward') == [True] and p.n('cpg_conv2d_wgrad_attach_bn_bwd', 'backward') == 1       # BatchNorm seq.4 in conv seq.6
        assert p.n('cpg_bn_relu_bwd', 'backward') == 0 and p.n('cpg_bn_relu_pool_bwd', 'backward') == 1
    if sit == 'S0b':
        # the input needs its gradient: no fused stem, and BatchNorm seq.1 rides in conv seq.3 as well
        assert stem == 0 and p.n('cpg_conv2d_fwd_bnstats', 'forward') == 3
        assert p.rode('backward') == [True, True] and p.n('cpg_bn_relu_bwd', 'backward') == 0
    if sit == 'S1':
        # frozen conv weights without a piggymask: no weight-gradient call, hence no rider; the stand-alone BatchNorm backward instead
        assert p.rode() == [] and p.n('cpg_conv2d_wgrad', 'backward') == 0 and p.n('cpg_bn_relu_bwd', 'backward') == 1
    if sit == 'S3':
        assert stem == 0 and p.rode() == [] and p.n('cpg_bn_relu_bwd', 'backward') == 2 and p.n('cpg_bn_relu_pool_bwd', 'backward') == 1
    if sit == 'S4':
        for k in (0, 1):
            # first pass: neither BatchNorm's node (k = 0) / the rider's result taken by BatchNorm seq.4 (k = 1); the second pass over
            # the retained graph finds the hint consumed
            assert p.n('cpg_bn_relu_bwd', 'backward%d' % k) == 0 and p.rode('grad%d' % k) == []
            assert p.n('cpg_conv2d_wgrad_attach_bn_bwd', 'grad%d' % k) == 0 and p.n('cpg_conv2d_wgrad', 'grad%d' % k) == 1
        assert p.rode('backward1') == [True]
        assert p.n('cpg_bn_relu_bwd', 'grad0') == 0 and p.n('cpg_bn_relu_bwd', 'grad1') == 1
        assert p.n('cpg_conv2d_wgrad', 'backward2') == p.n('cpg_conv2d_wgrad', 'grad2') == 0 and p.n('cpg_linear_wgrad', 'grad2') == 1
    if sit == 'S5':
        # second pass over the retained graph: hint and packed operands are used up, the stand-alone BatchNorm backward runs
        assert p.rode('backward') == [True] and p.rode('backward2') == [] and p.n('cpg_bn_relu_bwd', 'backward') == 0
        assert p.n('cpg_bn_relu_bwd', 'backward2') == 1 and p.n('cpg_conv2d_use_packed', 'backward2') == 0
        assert p.n('cpg_stem_bn_relu_bwd_reduce', 'backward2') == 1 and p.n('cpg_stem_bn_relu_bwd_wgrad', 'backward2') == 1
    if sit in ('S6', 'S7'):
        assert stem == 2 and p.rode('backward') == [True, True] and p.n('cpg_bn_relu_bwd') == 0
    if sit == 'S8':
        assert stem == 0 and p.rode() == [] and p.n('cpg_conv2d_fwd_bnstats') == 0 and p.n('cpg_bn_stats_finalize_count') == 0
        assert p.n('cpg_bn_relu_fwd_eval', 'forward') == 2 and p.n('cpg_bn_relu_bwd', 'backward') == 2
    if sit == 'S9':
        assert p.n('cpg_stem_bn_stats', 'nograd') == 0 and p.n('cpg_conv2d_fwd_bnstats', 'nograd') == 3


def _paths_b(topo, sit, p):
    adds = p.n('cpg_conv2d_dgrad_add')
    if topo == 'B_identity':
        # the skip-add epilogue runs exactly when the block's input needs its gradient
        # (S4: no subset reaches conv1; S5: the epilogue needs no hand-off, the second pass takes it again)
        want = {'S0a': 0, 'S5': 2, 'S6': 2, 'S7': 2, 'S4': 0}.get(sit, 1)
        assert adds == want, (adds, want)
    if topo == 'B_basic':
        assert adds == 0
    if sit in ('S0a', 'S0b'):
        assert p.n('cpg_bn_add_relu_fwd', 'forward') == 1 and p.n('cpg_bn_add_relu_bwd', 'backward') == 1
        assert p.n('cpg_conv2d_fwd_bnstats', 'forward') == {'B_identity': 3, 'B_down': 4, 'B_basic': 2}[topo]
    if sit == 'S3':
        assert p.n('cpg_conv2d_wgrad') == 0 and p.n('cpg_linear_wgrad') == 0
    if sit == 'S8':
        assert p.n('cpg_conv2d_fwd_bnstats') == 0 and p.n('cpg_bn_stats_finalize_count') == 0 and p.n('cpg_bn_stats_finalize') == 0


def _paths_c(sit, p):
    if sit in ('S0a', 'S0b', 'S1', 'S2', 'S9', 'S10'):
        # every PReLU delivers the bias gradient of the conv in front of it; the unit's first conv adds the skip gradient in its epilogue
        assert p.n('cpg_prelu_bwd_bias', 'backward') == 3 and p.n('cpg_prelu_bwd', 'backward') == 0
        assert p.n('cpg_conv2d_dgrad_add', 'backward') == 1
    if sit == 'S3':
        assert p.n('cpg_conv2d_wgrad') == 0 and p.n('cpg_linear_wgrad') == 0 and p.n('cpg_conv2d_dgrad_add', 'backward') == 1
    if sit == 'S5':
        # second pass: every sink is used up, the PReLUs run their plain backward and the convs reduce their own bias gradient
        assert p.n('cpg_prelu_bwd_bias', 'backward2') == 0 and p.n('cpg_prelu_bwd', 'backward2') == 3
        assert p.n('cpg_prelu_bwd_bias', 'backward') == 3 and p.n('cpg_conv2d_use_packed', 'backward2') == 0
    if sit == 'S9':
        assert p.n('cpg_prelu_fwd', 'nograd') == 3


@pytest.mark.parametrize('topo,sit', CASES)
def test_situation_matches_fp64(topo, sit, probe):
    seed = R.seed_of(topo, sit)
    net = R.build_library(topo, R.build_reference(topo, seed), DEV)
    got = R.run(net, sit, R.make_data(topo, seed), DEV, torch.float32, mark=probe.mark)
    torch.cuda.synchronize()
    print('%s %s entry points per phase: %s; rider: %s' % (topo, sit, probe.summary(), probe.riders))
    bad = R.compare(got, topo, sit, seed)
    if sit == 'S8':
        for n in got:
            if n.startswith('before:'):
                assert torch.equal(got[n], got[n[7:]]), n          # eval mode: statistics and counters bit-identical to before
    if topo == 'A':
        _paths_a(sit, probe)
    elif topo == 'C':
        _paths_c(sit, probe)
    else:
        _paths_b(topo, sit, probe)
    assert not bad, bad


def _rel(a, b):
    return float((a.detach().double().cpu() - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize('kind', ['pointwise', 'wino'])
def test_skip_function_with_one_gradient_missing(kind, probe):
    """_MaskedConv2dSkipFn gets None for either incoming gradient (set_materialize_grads(False)): only the skip branch used -- the
    conv's output is dead, the input gradient is the skip gradient itself and the parameters get none --, only the conv branch used,
    and both; against float64, at the shapes of B's conv1 (1x1, 64 -> 16) and C's conv2 (3x3, 64 -> 64, bias, through conv_prelu_skip)."""
    g = torch.Generator().manual_seed(5)
    if kind == 'pointwise':
        N, C, K, H, ks = 4, 64, 16, 8, 1
    else:
        N, C, K, H, ks = 3, 64, 64, 14, 3
    x0 = torch.randn(N, C, H, H, generator=g)
    w = torch.randn(K, C, ks, ks, generator=g) * (2.0 / (C * ks * ks)) ** 0.5
    b = torch.randn(K, generator=g) * 0.1 if ks == 3 else None
    gy, gs = torch.randn(N, K, H, H, generator=g), torch.randn(N, C, H, H, generator=g)
    conv = nl.SharableConv2d(C, K, ks, padding=ks // 2, bias=b is not None).to(DEV)
    act = nn.PReLU(K).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        if b is not None:
            conv.bias.copy_(b)

    def lib(use_y, use_skip):
        conv.zero_grad(set_to_none=True)
        act.zero_grad(set_to_none=True)
        x = x0.to(DEV).requires_grad_(True)
        if ks == 1:
            y, _, skip = conv.forward_with_skip(x)
        else:
            y, skip = fused_bn.conv_prelu_skip(conv, act, x)
        assert 'SkipFn' in type(skip.grad_fn).__name__
        loss = (y * gy.to(DEV)).sum() * float(use_y) if use_y else 0.0
        if use_skip:
            loss = loss + (skip * gs.to(DEV)).sum()
        loss.backward()
        return x.grad, conv.weight.grad, conv.bias.grad if b is not None else None

    def ref(use_y, use_skip, dtype):
        x = x0.clone().to(dtype).requires_grad_(True)
        wr = w.clone().to(dtype).requires_grad_(True)
        br = None if b is None else b.clone().to(dtype).requires_grad_(True)
        y = F.conv2d(x, wr, br, padding=ks // 2)
        if ks == 3:
            y = F.prelu(y, act.weight.detach().cpu().to(dtype))
        loss = (y * gy.to(dtype)).sum() * float(use_y) + (x * gs.to(dtype)).sum() * float(use_skip)
        loss.backward()
        return x.grad, wr.grad, None if br is None else br.grad

    gx, gw, gb = lib(False, True)
    assert torch.equal(gx.cpu(), gs) and gw is None and gb is None
    for use_y, use_skip in ((True, False), (True, True)):
        got, r64, r32 = lib(use_y, use_skip), ref(use_y, use_skip, torch.float64), ref(use_y, use_skip, torch.float32)
        for name, a, want, w32 in zip(('gx', 'gw', 'gb'), got, r64, r32):
            if want is None:
                assert a is None
                continue
            bound = max(R.B_FLOOR, R.B_FACTOR * _rel(w32, want))
            print('%s y=%s skip=%s %s: %.3g of scale (bound %.3g)' % (kind, use_y, use_skip, name, _rel(a, want), bound))
            assert _rel(a, want) <= bound, name
    assert probe.n('cpg_conv2d_dgrad_add') == 1 and probe.n('cpg_conv2d_dgrad') == 1


# ------------------------------------------------------------------------------------------------- off-centre channels
@pytest.mark.parametrize('kind', sorted(R.OFFCENTRE))
def test_offcentre_fused_statistics(kind, probe):
    """Train-mode conv -> BatchNorm -> ReLU with the statistics from the conv epilogue (fuse_stats), channels at |mean| / std from 0 to 8,
    few tiles per channel: batch mean within 1e-4 std, invstd within 1e-4 relative, output / gradients / running statistics within the
    module's bounds, all against float64."""
    c = R.offcentre(kind)
    N, C, H, W, K, ks, _ = R.OFFCENTRE[kind]
    conv = nl.SharableConv2d(C, K, ks, padding=ks // 2, bias=False)
    bn = nn.BatchNorm2d(K)
    with torch.no_grad():
        conv.weight.copy_(c['w'])
        bn.weight.copy_(c['gamma'])
        bn.bias.copy_(c['beta'])
    seq = fused_bn.FusedSequential(conv, bn, nn.ReLU(inplace=True)).to(DEV).train()
    x = c['x'].to(DEV).requires_grad_(c['x_grad'])
    z = seq(x)
    fn = z.grad_fn
    assert type(fn).__name__ == ('_StemConvBnReluFnBackward' if kind == 'stem' else '_BnReluFnBackward')
    assert probe.n('cpg_stem_bn_stats' if kind == 'stem' else 'cpg_conv2d_fwd_bnstats') == 1 and probe.n('cpg_bn_relu_fwd_train') == 0
    assert probe.n('cpg_bn_stats_finalize_count') + probe.n('cpg_bn_stats_finalize') == 1
    mean, invstd = (t.detach().double().cpu() for t in fn.saved_tensors[-2:])
    (z * c['gz'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    r64, r32 = c['r64'], c['r32']
    emean = (mean - r64['mean']).abs() / r64['std']
    einv = (invstd / r64['invstd'] - 1).abs()
    worst = int(einv.argmax())
    print('%s: batch mean off by at most %.3g std, invstd by %.3g relative (channel %d, |mean| / std %.3g)'
          % (kind, float(emean.max()), float(einv.max()), worst, float(r64['ratio'][worst])))
    got = {'out': z, 'grad:x': x.grad, 'grad:w': conv.weight.grad, 'grad:gamma': bn.weight.grad, 'grad:beta': bn.bias.grad}
    bad = []
    for n, a in got.items():
        if r64[n] is None:
            assert a is None
            continue
        bound = max(R.B_FLOOR, R.B_FACTOR * _rel(r32[n], r64[n]))
        e = _rel(a, r64[n])
        print('%s %s: %.3g of scale (bound %.3g)' % (kind, n, e, bound))
        if not e <= bound:
            bad.append((n, e, bound))
    for n, a in (('buf:running_mean', bn.running_mean), ('buf:running_var', bn.running_var)):
        err = (a.detach().double().cpu() - r64[n].double()).abs()
        over = float((err - (R.STAT_ATOL + R.STAT_RTOL * r64[n].double().abs())).max())
        print('%s %s: max err %.3g, worst excess over atol + rtol |ref| %.3g' % (kind, n, float(err.max()), over))
        if not over <= 0:
            bad.append((n, float(err.max())))
    assert int(bn.num_batches_tracked) == 1
    assert float(emean.max()) <= R.STAT_BOUND and float(einv.max()) <= R.STAT_BOUND
    assert not bad, bad


def test_offcentre_standalone_statistics_at_ratio_1000(probe):
    """The stand-alone statistics pass (cpg_bn_relu_fwd_train: fp64 partial sums) with channels at |mean| / std from 0 to 1000:
    invstd within 1e-6 relative; the batch mean, a float32 output, within 1e-6 std plus half a float32 ulp of itself."""
    N, C, H, W = 4, 16, 14, 14
    g = torch.Generator().manual_seed(3)
    ratio = torch.linspace(0, 1000, C)
    x = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) + ratio.view(1, C, 1, 1).double()).float()
    bn = nn.BatchNorm2d(C).to(DEV).train()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    z = fused_bn.bn_relu(x.to(DEV).requires_grad_(True), bn)
    assert probe.n('cpg_bn_relu_fwd_train') == 1 and type(z.grad_fn).__name__ == '_BnReluFnBackward'
    mean, invstd = (t.detach().double().cpu() for t in z.grad_fn.saved_tensors[-2:])
    var64, mean64 = torch.var_mean(x.double(), dim=(0, 2, 3), unbiased=False)
    inv64 = torch.rsqrt(var64 + bn.eps)
    z64 = torch.relu((x.double() - mean64.view(1, C, 1, 1)) * (inv64 * gamma.double()).view(1, C, 1, 1) + beta.double().view(1, C, 1, 1))
    z32 = torch.relu(F.batch_norm(x, None, None, gamma, beta, True, 0.1, bn.eps))
    half_ulp = (torch.nextafter(mean64.float().abs(), torch.tensor(float('inf'))) - mean64.float().abs()).double() / 2
    emean = ((mean - mean64).abs() - half_ulp).clamp(min=0) / var64.sqrt()
    einv = (invstd / inv64 - 1).abs()
    bound = max(R.B_FLOOR, R.B_FACTOR * _rel(z32, z64))
    print('ratio 1000: mean off by %.3g std beyond half an ulp (raw %.3g std), invstd by %.3g relative, output %.3g of scale (bound %.3g)'
          % (float(emean.max()), float(((mean - mean64).abs() / var64.sqrt()).max()), float(einv.max()), _rel(z, z64), bound))
    assert float(einv.max()) <= 1e-6 and float(emean.max()) <= 1e-6
    assert _rel(z, z64) <= bound
