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

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from cpg_amd import _lib                         # noqa: E402
from cpg_amd.models import fused_bn              # noqa: E402
from cpg_amd.models import layers as nl          # noqa: E402

# tables, runners and the body of test_eval_block_kernels: shared with tests/test_guard_bands_gpu.py
import _eval_block_cases as EB                   # noqa: E402
from _eval_block_cases import CASES, DEV, EPS, RATIOS, _desc, _dev, _out, make_bn, run_eval    # noqa: E402


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    if RATIOS:
        print('\neval-block error ratios, (|y - ref| - shift term) / (L U32 |s| (|x| * |w_eff|)), largest per tile:')
        print('  ' + '  '.join('%s=%.4f' % kv for kv in sorted(RATIOS.items())))


@pytest.mark.parametrize('cid', list(CASES))
def test_eval_block_kernels(cid, libopt):
    EB.eval_block_case(cid, libopt)


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
