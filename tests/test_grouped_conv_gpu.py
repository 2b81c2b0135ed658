"""groups > 1 on the grouped kernels (csrc/conv_grouped.hip): all groups of a pass in one launch, against the oracle's
F.conv2d(groups=G) restatement -- through the layer, through the raw C ABI, and against the per-group path (CPG_NO_GROUPED=1).

Tolerances are those of test_hip_parity.test_grouped_conv_vs_oracle: y / gx rtol 1e-4, atol 2e-5; gw / gpm rtol 1e-4,
atol 1e-5 * max(|gw|max, 1); gb atol 1e-3."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import cpg_amd._lib as L                        # noqa: E402
from cpg_amd.models import layers as nl          # noqa: E402
from oracle import ops                           # noqa: E402  (checker only)

DEV = 'cuda:0'
CPG_E_UNSUPPORTED = -2

# (N, C, K, H, W, k, stride, pad, dil, G)
CASES = {
    'depthwise_odd': (3, 40, 40, 13, 9, 3, 1, 1, 1, 40),
    'depthwise_s2_odd_map': (2, 24, 24, 15, 15, 3, 2, 1, 1, 24),
    'depthwise_multiplier2': (2, 16, 32, 10, 12, 3, 1, 1, 1, 16),
    'depthwise_5x5': (1, 8, 8, 11, 11, 5, 1, 2, 1, 8),
    'depthwise_dilated': (2, 12, 12, 14, 14, 3, 1, 2, 2, 12),
    'narrow_32x4d': (3, 32, 32, 14, 14, 3, 1, 1, 1, 8),
    'narrow_4to8_rect': (2, 16, 32, 9, 17, 3, 1, 1, 1, 4),
    'grouped_pointwise_s2': (2, 32, 32, 9, 9, 1, 2, 0, 1, 4),
    'wide_48to80': (2, 96, 160, 12, 20, 3, 1, 1, 1, 2),
    'wide_s2_16to32': (3, 48, 96, 10, 10, 3, 2, 1, 1, 3),
    'wide_7x7_map': (1, 128, 128, 7, 7, 3, 1, 1, 1, 4),
}
DETERMINISM = {'depthwise_split': (6, 32, 32, 28, 28, 3, 1, 1, 1, 32), 'wide_48to80': CASES['wide_48to80']}


def close(got, want, rtol, atol, msg):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


def make_inputs(case, bias, pm):
    """The seeded-generator recipe of test_grouped_conv_vs_oracle."""
    N, C, K, H, W, k, s, p, dil, G = case
    g = torch.Generator().manual_seed(N + C + K + G)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C // G, k, k, generator=g) * 0.2
    b = torch.randn(K, generator=g) * 0.1 if bias else None
    pmv = torch.rand(K, C // G, k, k, generator=g) * 0.012 if pm else None
    oh = (H + 2 * p - dil * (k - 1) - 1) // s + 1
    ow = (W + 2 * p - dil * (k - 1) - 1) // s + 1
    gy = torch.randn(N, K, oh, ow, generator=g)
    return x, w, b, pmv, gy


def make_layer(case, w, b, pmv):
    N, C, K, H, W, k, s, p, dil, G = case
    layer = nl.SharableConv2d(C, K, k, stride=s, padding=p, dilation=dil, groups=G, bias=b is not None).to(DEV)
    layer.weight.data.copy_(w)
    if b is not None:
        layer.bias.data.copy_(b)
    if pmv is not None:
        layer.piggymask = nn.Parameter(pmv.to(DEV))
    return layer


def run_layer(case, x, w, b, pmv, gy):
    """(y, gx, gw, gpm or None, gb or None) of one forward + backward through the public layer."""
    layer = make_layer(case, w, b, pmv)
    xd = x.to(DEV).requires_grad_(True)
    y = layer(xd)
    y.backward(gy.to(DEV))
    return (y.detach(), xd.grad, layer.weight.grad, None if pmv is None else layer.piggymask.grad,
            None if b is None else layer.bias.grad), layer


def oracle(case, x, w, b, pmv, gy):
    N, C, K, H, W, k, s, p, dil, G = case
    pn = None if pmv is None else pmv.numpy()
    want = ops.conv2d_forward(x.numpy(), w.numpy(), pn, None if b is None else b.numpy(), s, p, dil, G)
    r = ops.conv2d_backward(x.numpy(), w.numpy(), gy.numpy(), pn, b is not None, s, p, dil, G)
    return want, r


def check_five(got, want, r, pm, bias, tag=''):
    y, gx, gw, gpm, gb = got
    scale = float(np.abs(r['gw']).max())
    close(y, want, 1e-4, 2e-5, tag + 'y')
    close(gx, r['gx'], 1e-4, 2e-5, tag + 'gx')
    close(gw, r['gw'], 1e-4, 1e-5 * max(scale, 1.0), tag + 'gw')
    if pm:
        close(gpm, r['gpm'], 1e-4, 1e-5 * max(scale, 1.0), tag + 'gpm')
    if bias:
        close(gb, r['gb'], 1e-4, 1e-3, tag + 'gb')


@pytest.mark.parametrize('idx,name', list(enumerate(CASES)))
def test_grouped_layer_vs_oracle(idx, name, monkeypatch):
    """Output and every gradient of the layer against the oracle; bias and piggymask alternate over the cases; and
    forward_with_bn_stats gives the same bits and no statistics.  Always on the grouped kernels (the layer's own dispatch sends
    3x3 s1 p1 layers and strided layers with >= 16 channels per group to the per-group path: test_grouped_conv_vs_oracle covers that)."""
    monkeypatch.setattr(nl, 'GROUPED_PER_GROUP_MIN', None)
    case = CASES[name]
    bias, pm = idx % 2 == 0, idx % 2 == 1 or idx % 3 == 0
    x, w, b, pmv, gy = make_inputs(case, bias, pm)
    got, layer = run_layer(case, x, w, b, pmv, gy)
    want, r = oracle(case, x, w, b, pmv, gy)
    check_five(got, want, r, pm, bias)
    with torch.no_grad():
        y2, st = layer.forward_with_bn_stats(x.to(DEV))
    assert st is None and torch.equal(y2, got[0])
    assert not layer._per_group()


def test_wide_winograd_groups_stay_per_group(monkeypatch):
    """The measured dispatch rule: from 16 channels per group a 3x3 s1 p1 layer and a strided layer run one groups == 1 launch per
    group (4 / 4 / 4 calls for G = 4, 3 / 3 / 3 for G = 3), anything else the grouped kernels."""
    case = CASES['wide_s2_16to32']
    inputs = make_inputs(case, False, True)
    assert _count_calls(monkeypatch, lambda: run_layer(case, *inputs)) == (3, 3, 3)
    case = CASES['wide_7x7_map']
    inputs = make_inputs(case, False, True)
    assert _count_calls(monkeypatch, lambda: run_layer(case, *inputs)) == (4, 4, 4)
    monkeypatch.setattr(nl, 'GROUPED_PER_GROUP_MIN', None)
    assert _count_calls(monkeypatch, lambda: run_layer(case, *inputs)) == (1, 1, 1)


def _desc(case):
    N, C, K, H, W, k, s, p, dil, G = case
    d = L.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, k, k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = p
    d.dil_h = d.dil_w = dil
    d.groups = G
    return d


@pytest.mark.parametrize('name', ['narrow_32x4d', 'wide_48to80'])
def test_grouped_c_abi_through_ctypes(name):
    """cpg_conv2d_workspace_bytes / _fwd / _dgrad / _wgrad (with gb) on a groups > 1 descriptor: CPG_OK and the oracle's numbers; gw, gpm
    and gb pre-filled with NaN come back finite everywhere (they are overwritten, and no element is outside every group)."""
    case = CASES[name]
    x, w, b, pmv, gy = make_inputs(case, True, True)
    want, r = oracle(case, x, w, b, pmv, gy)
    lib = L.lib()
    d = _desc(case)
    nbytes = lib.cpg_conv2d_workspace_bytes(ctypes.byref(d))
    assert nbytes >= case[2] * 4
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=DEV)
    xd, wd, bd, pd, gyd = (t.to(DEV).contiguous() for t in (x, w, b, pmv, gy))
    y = torch.full(want.shape, float('nan'), device=DEV)
    gx = torch.full(x.shape, float('nan'), device=DEV)
    gw, gpm = torch.full(w.shape, float('nan'), device=DEV), torch.full(w.shape, float('nan'), device=DEV)
    gb = torch.full((case[2],), float('nan'), device=DEV)
    P, s = L.dptr, L.stream_ptr()
    thr = nl.DEFAULT_THRESHOLD
    assert lib.cpg_conv2d_fwd(ctypes.byref(d), P(xd), P(wd), P(pd), thr, P(bd), P(y), P(ws), ws.numel() * 4, s) == L.CPG_OK, lib.cpg_last_error()
    assert lib.cpg_conv2d_dgrad(ctypes.byref(d), P(gyd), P(wd), P(pd), thr, P(gx), P(ws), ws.numel() * 4, s) == L.CPG_OK, lib.cpg_last_error()
    assert lib.cpg_conv2d_wgrad(ctypes.byref(d), P(xd), P(gyd), P(wd), P(pd), thr, P(gw), P(gpm), P(gb), P(ws), ws.numel() * 4,
                                s) == L.CPG_OK, lib.cpg_last_error()
    torch.cuda.synchronize()
    for t in (y, gx, gw, gpm, gb):
        assert bool(torch.isfinite(t).all())
    check_five((y, gx, gw, gpm, gb), want, r, True, True)


def test_grouped_c_abi_rejects_indivisible_channels():
    """C % groups != 0: CPG_E_INVALID, and the output buffer keeps its sentinel."""
    lib = L.lib()
    d = _desc((2, 30, 32, 8, 8, 3, 1, 1, 1, 4))
    y = torch.full((2, 32, 8, 8), -7.0, device=DEV)
    x = torch.zeros(2, 30, 8, 8, device=DEV)
    w = torch.zeros(32, 8, 3, 3, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.float32, device=DEV)
    rc = lib.cpg_conv2d_fwd(ctypes.byref(d), L.dptr(x), L.dptr(w), None, 0.0, None, L.dptr(y), L.dptr(ws), ws.numel() * 4, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.CPG_E_INVALID
    assert bool((y == -7.0).all())
    assert lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)) == 0


def _count_calls(monkeypatch, fn):
    counts = {'cpg_conv2d_fwd': 0, 'cpg_conv2d_dgrad': 0, 'cpg_conv2d_wgrad': 0}
    real = L.call

    def counting(name, *args):
        if name in counts:
            counts[name] += 1
        return real(name, *args)

    monkeypatch.setattr(L, 'call', counting)
    fn()
    monkeypatch.setattr(L, 'call', real)
    return counts['cpg_conv2d_fwd'], counts['cpg_conv2d_dgrad'], counts['cpg_conv2d_wgrad']


def test_one_application_per_pass(monkeypatch):
    """A G = 8 layer's forward + backward: one cpg_conv2d_fwd / _dgrad / _wgrad each; eight each with CPG_NO_GROUPED=1."""
    case = CASES['narrow_32x4d']
    inputs = make_inputs(case, True, True)
    assert _count_calls(monkeypatch, lambda: run_layer(case, *inputs)) == (1, 1, 1)
    with L.option('CPG_NO_GROUPED', 1):
        assert _count_calls(monkeypatch, lambda: run_layer(case, *inputs)) == (8, 8, 8)


@pytest.mark.parametrize('name', ['narrow_4to8_rect', 'wide_s2_16to32'])
def test_switch_equivalence(name, monkeypatch):
    """The grouped kernels against the per-group path (CPG_NO_GROUPED=1) on the same layer: another summation order, the same tolerances."""
    monkeypatch.setattr(nl, 'GROUPED_PER_GROUP_MIN', None)     # (the grouped kernels for the wide strided shape too)
    case = CASES[name]
    x, w, b, pmv, gy = make_inputs(case, True, True)
    got, _ = run_layer(case, x, w, b, pmv, gy)
    with L.option('CPG_NO_GROUPED', 1):
        assert L.lib().cpg_conv2d_workspace_bytes(ctypes.byref(_desc(case))) == 0      # reported as unsupported, as before
        ref, _ = run_layer(case, x, w, b, pmv, gy)
    ref = [t.cpu().numpy() for t in ref]
    check_five(got, ref[0], {'gx': ref[1], 'gw': ref[2], 'gpm': ref[3], 'gb': ref[4]}, True, True, tag=name + ' ')


@pytest.mark.parametrize('name', list(DETERMINISM))
def test_grouped_bit_reproducible(name, monkeypatch):
    """Two runs on identical inputs: y, gx, gw, gpm and gb bit-equal (no floating-point atomics; the depthwise shape is sized so that
    the weight gradient is split over image slices)."""
    monkeypatch.setattr(nl, 'GROUPED_PER_GROUP_MIN', None)          # (the grouped kernels, whatever the layer's dispatch would pick)
    case = DETERMINISM[name]
    if name == 'depthwise_split':
        nbytes = L.lib().cpg_conv2d_workspace_bytes(ctypes.byref(_desc(case)))
        assert nbytes >= 2 * case[2] * (case[1] // case[9]) * 9 * 4            # at least two partial copies of the weight gradient
    inputs = make_inputs(case, True, True)
    a, _ = run_layer(case, *inputs)
    b, _ = run_layer(case, *inputs)
    for u, v, what in zip(a, b, ('y', 'gx', 'gw', 'gpm', 'gb')):
        assert torch.equal(u, v), what
