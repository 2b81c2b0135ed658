"""The armed side arguments of the C ABI on the device (tests/test_side_args_host.py has what is decided before a launch): two channels
armed for one call, threads, the inference entry points' corner, and the Python layer's arm-then-call helper.

Shapes are the smallest whose forward streams a packed operand: 2x64x4x4 -> 64 (3x3 s1 p1, the two-wave Winograd kernel) and
2x16x4x4 -> 16 (1x1); the tests assert that instead of assuming it.  Inputs are seeded, outputs start as NaN, comparisons are bit-equal.
No call here faults: what is refused is refused before a launch.

Everything but the last group pins what the library did before the armed values became arguments below the ABI boundary and passes on
that library unchanged."""
import ctypes
import threading

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from cpg_amd import _lib
from cpg_amd.models import fused_bn
from cpg_amd.models import layers as nl

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
THR = 0.005
P = _lib.dptr
WORKSPACE = -3
C3 = (2, 64, 4, 4, 64, 3)
C1 = (2, 16, 4, 4, 16, 1)


def _desc(N, C, H, W, K, k):
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, k, k
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.groups = 1
    d.pad_h = d.pad_w = k // 2
    return d


class _Case(object):
    """one shape with seeded inputs, its workspace, and the plain forward's output as the reference (computed once, never written again)"""

    def __init__(self, shape, seed):
        N, C, H, W, K, k = shape
        self.d = _desc(*shape)
        g = torch.Generator(device='cpu').manual_seed(seed)
        self.x = torch.randn(N, C, H, W, generator=g).to(DEV)
        self.w = (torch.randn(K, C, k, k, generator=g) * 0.05).to(DEV)
        self.pm = (torch.randn(K, C, k, k, generator=g) * 0.01 + THR).to(DEV)
        lib = _lib.lib()
        self.nb = [int(lib.cpg_conv2d_pack_bytes(ctypes.byref(self.d), p)) for p in (0, 1, 2)]
        assert self.nb[0] > 0 and self.nb[0] != 256, self.nb          # the forward streams a packed operand, and the junk below is not it
        self.ws, self.wsb = _lib.workspace(lib.cpg_conv2d_workspace_bytes(ctypes.byref(self.d)), DEV)
        self.junk = torch.zeros(64, device=DEV)
        rc, self.ref = self.fwd()
        assert rc == _lib.CPG_OK and not torch.isnan(self.ref).any()

    def out(self):
        d = self.d
        return torch.full((d.N, d.K, d.H, d.W), float('nan'), device=DEV)

    def fwd(self):
        y = self.out()
        rc = _lib.lib().cpg_conv2d_fwd(ctypes.byref(self.d), P(self.x), P(self.w), P(self.pm), THR, None, P(y), P(self.ws), self.wsb, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, y

    def fwd_bnstats(self):
        lib, d = _lib.lib(), self.d
        tiles = lib.cpg_conv2d_bnstats_tiles(ctypes.byref(d))
        assert tiles > 0
        y, stats = self.out(), torch.full((d.K, tiles, 2), float('nan'), device=DEV)
        rc = lib.cpg_conv2d_fwd_bnstats(ctypes.byref(d), P(self.x), P(self.w), P(self.pm), THR, None, P(y), P(stats), stats.numel() * 4, P(self.ws),
                                        self.wsb, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.CPG_OK, lib.cpg_last_error()
        return y, stats

    def fwd_bn_eval(self):
        K = self.d.K
        gamma, beta, mean, var = torch.ones(K, device=DEV), torch.zeros(K, device=DEV), torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
        y = self.out()
        rc = _lib.lib().cpg_conv2d_fwd_bn_eval(ctypes.byref(self.d), P(self.x), P(self.w), P(self.pm), THR, None, P(gamma), P(beta), P(mean), P(var),
                                               1e-5, 1, P(y), None, P(self.ws), self.wsb, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, y

    def arm_junk(self):
        assert _lib.lib().cpg_conv2d_use_packed(P(self.junk), 256) == _lib.CPG_OK


@pytest.fixture(scope='module')
def c3():
    return _Case(C3, seed=21)


@pytest.fixture(scope='module')
def c1():
    return _Case(C1, seed=22)


def test_packed_operand_and_window_maxima_armed_for_one_call(c3):
    lib, d = _lib.lib(), c3.d
    assert c3.nb[2] > 0 and lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(d)) == 1
    y0, s0 = c3.fwd_bnstats()
    assert not torch.isnan(y0).any() and not torch.isnan(s0).any()
    pk = torch.full((c3.nb[2] // 4,), float('nan'), device=DEV)
    _lib.check('pack', lib.cpg_conv2d_pack(ctypes.byref(d), P(c3.w), P(c3.pm), THR, 2, P(pk), c3.nb[2], 0, None, 0, _lib.stream_ptr()))
    E = torch.full((d.N, d.K, d.H // 2, d.W // 2), float('nan'), device=DEV)
    assert lib.cpg_conv2d_use_packed(P(pk), c3.nb[2]) == _lib.CPG_OK
    assert lib.cpg_conv2d_fwd_attach_pool_max(P(E), E.numel() * 4) == _lib.CPG_OK
    y1, s1 = c3.fwd_bnstats()
    assert torch.equal(y1, y0) and torch.equal(s1, s0)
    assert torch.equal(E, F.max_pool2d(y0, 2, 2))
    # both were used up by that one call: a poisoned operand and a sentinel in E show whether the next call touches either
    pk.fill_(float('nan'))
    E.fill_(7.0)
    y2, s2 = c3.fwd_bnstats()
    assert torch.equal(y2, y0) and torch.equal(s2, s0)
    assert bool((E == 7.0).all())


def test_an_armed_operand_is_invisible_to_other_threads(c3):
    c3.arm_junk()
    got = {}

    def other():
        torch.cuda.set_device(0)
        got['fwd'] = c3.fwd()
    t = threading.Thread(target=other)
    t.start()
    t.join()
    rc, y = got['fwd']
    assert rc == _lib.CPG_OK and torch.equal(y, c3.ref)
    rc, y = c3.fwd()                                  # this thread's junk is still armed, and refused before anything is launched
    assert rc < 0 and torch.isnan(y).all()
    rc, y = c3.fwd()
    assert rc == _lib.CPG_OK and torch.equal(y, c3.ref)


def test_eval_entry_point_on_the_3x3_route_leaves_the_operand_armed(c3):
    """include/cpg_hip.h: the inference entry points take a packed operand on the pointwise and the 3x3 stride-2 routes only."""
    c3.arm_junk()
    rc, y = c3.fwd_bn_eval()
    assert rc == _lib.CPG_OK and not torch.isnan(y).any()
    rc, y = c3.fwd()
    assert rc < 0 and torch.isnan(y).all()           # the junk was still armed
    rc, y = c3.fwd()
    assert rc == _lib.CPG_OK and torch.equal(y, c3.ref)


def test_eval_entry_point_on_the_pointwise_route_takes_the_operand(c1):
    rc, want = c1.fwd_bn_eval()
    assert rc == _lib.CPG_OK and not torch.isnan(want).any()
    c1.arm_junk()
    rc, y = c1.fwd_bn_eval()
    assert rc < 0 and torch.isnan(y).all()           # refused, nothing written
    rc, y = c1.fwd_bn_eval()
    assert rc == _lib.CPG_OK and torch.equal(y, want)
    rc, y = c1.fwd()
    assert rc == _lib.CPG_OK and torch.equal(y, c1.ref)


# ------------------------------------------------------------------------------------------------ the Python layer's arm-then-call helper
class _Boom(Exception):
    pass


def _raise_in(monkeypatch, target, after):
    """_lib.call raises _Boom in place of the first `target` call that follows an `after` call: the arms went through, the armed call
    is never made.  Returns a dict with the thread the exception was raised on."""
    real, state = _lib.call, {'armed': False, 'thread': None}

    def call(name, *args):
        if name == after:
            state['armed'] = True
        if name == target and state['armed']:
            state['thread'] = threading.get_ident()
            raise _Boom(target)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', call)
    return state


class _InBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def _on_backward_thread(fn):
    """fn() on autograd's worker thread of the device -- where a backward's arms are made -- with its result and that thread's id"""
    out = {}
    x = torch.zeros(1, device=DEV, requires_grad=True)
    _InBackward.apply(x, lambda: out.update(v=fn(), thread=threading.get_ident())).sum().backward()
    return out['v'], out['thread']


def _stack(seed=3):
    """test_pool_max_gpu._stack: conv-BN-ReLU, conv-BN-ReLU-pool at 64 channels (run at 5 x 64 x 6 x 6)"""
    torch.manual_seed(seed)
    net = fused_bn.FusedSequential(
        nl.SharableConv2d(64, 64, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
        nl.SharableConv2d(64, 64, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
        nn.MaxPool2d(2, 2)).to(DEV)
    with torch.no_grad():
        for m in (net[0], net[3]):
            m.weight.normal_(0.0, 0.05)
    return net.train()


def _stack_input(requires_grad=True):
    g = torch.Generator(device='cpu').manual_seed(9)
    return torch.randn(5, 64, 6, 6, generator=g).to(DEV).requires_grad_(requires_grad)


BIG = (64, 64, 8, 8)        # maxima armed for 5 x 64 x 6 x 6 are too short for this tensor: an armed call says so, an unarmed one goes on


def _null_fwd_bnstats():
    d = _desc(*BIG, 64, 3)
    rc = _lib.lib().cpg_conv2d_fwd_bnstats(ctypes.byref(d), None, None, None, 0.0, None, None, None, 0, ctypes.c_void_p(16), 1 << 20, None)
    return rc, _lib.lib().cpg_last_error().decode()


def _null_pool_fwd():
    rc = _lib.lib().cpg_bn_relu_pool_fwd(None, None, None, 1e-5, 0.1, None, None, None, None, None, *BIG, 0, None, 0, None)
    return rc, _lib.lib().cpg_last_error().decode()


def _null_pool_bwd():
    rc = _lib.lib().cpg_bn_relu_pool_bwd(None, None, None, None, None, None, None, None, None, *BIG, 1, None, 0, None)
    return rc, _lib.lib().cpg_last_error().decode()


def _null_wgrad():
    d = _desc(2, 16, 8, 8, 32, 3)            # no Winograd weight gradient: an armed rider is CPG_E_UNSUPPORTED, before the null pointers
    assert _lib.lib().cpg_conv2d_wgrad_rider_supported(ctypes.byref(d)) == 0
    rc = _lib.lib().cpg_conv2d_wgrad(ctypes.byref(d), None, None, None, None, 0.0, None, None, None, ctypes.c_void_p(16), 1 << 20, None)
    return rc, _lib.lib().cpg_last_error().decode()


def test_helper_disarms_the_packed_operand(monkeypatch):
    """Site 1 of 5 (models/layers.py, the conv calls that stream a packed operand).  The follow-up runs on doubled weights: a call that
    still found the operand of the old weights armed would compute from those."""
    conv = nl.SharableConv2d(64, 64, kernel_size=3, padding=1, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.normal_(0.0, 0.05)
    x = _stack_input()
    _raise_in(monkeypatch, 'cpg_conv2d_fwd', after='cpg_conv2d_use_packed')
    with pytest.raises(_Boom):
        conv(x)
    monkeypatch.undo()
    with torch.no_grad():
        conv.weight.mul_(2.0)
    lib, d = _lib.lib(), _desc(5, 64, 6, 6, 64, 3)
    ws, wsb = _lib.workspace(lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)), DEV)
    ys = []
    for _ in range(2):                      # (the second call is unarmed whatever the first one found)
        y = torch.full((5, 64, 6, 6), float('nan'), device=DEV)
        _lib.check('fwd', lib.cpg_conv2d_fwd(ctypes.byref(d), P(x.detach()), P(conv.weight.detach()), None, THR, None, P(y), P(ws), wsb, _lib.stream_ptr()))
        torch.cuda.synchronize()
        ys.append(y)
    assert not torch.isnan(ys[0]).any() and torch.equal(ys[0], ys[1])


def test_helper_disarms_the_conv_window_maxima(monkeypatch):
    """Site 2 of 5 (models/layers.py, the conv in front of a pooled BatchNorm: window maxima and packed operand armed together).
    NEW behaviour, with the three cases below: before the helper, only the packed-operand site disarmed when something raised between
    the arm and the call, so these four do not pass on the library's earlier Python layer."""
    net, x = _stack(), _stack_input()
    _raise_in(monkeypatch, 'cpg_conv2d_fwd_bnstats', after='cpg_conv2d_fwd_attach_pool_max')
    with pytest.raises(_Boom):
        net(x)
    monkeypatch.undo()
    rc, text = _null_fwd_bnstats()
    assert rc == WORKSPACE and 'statistics buffer' in text, (rc, text)


def test_helper_disarms_the_pooled_forward_maxima(monkeypatch):
    """Site 4 of 5 (models/fused_bn.py, _BnReluPoolFn.forward)."""
    net, x = _stack(), _stack_input()
    _raise_in(monkeypatch, 'cpg_bn_relu_pool_fwd', after='cpg_bn_relu_pool_attach_max')
    with pytest.raises(_Boom):
        net(x)
    monkeypatch.undo()
    rc, text = _null_pool_fwd()
    assert rc == _lib.CPG_E_INVALID and 'null pointer' in text, (rc, text)


def test_helper_disarms_the_pooled_backward_maxima(monkeypatch):
    """Site 5 of 5 (models/fused_bn.py, _pool_backward).  A backward arms autograd's worker thread, so the follow-up runs there too."""
    net, x = _stack(), _stack_input()
    loss = net(x).square().mean()
    state = _raise_in(monkeypatch, 'cpg_bn_relu_pool_bwd', after='cpg_bn_relu_pool_attach_max')
    with pytest.raises(Exception, match='cpg_bn_relu_pool_bwd'):
        loss.backward()
    monkeypatch.undo()
    (rc, text), thread = _on_backward_thread(_null_pool_bwd)
    assert thread == state['thread'] and thread is not None
    assert rc == _lib.CPG_E_INVALID and 'null pointer' in text, (rc, text)


def test_helper_disarms_the_rider(monkeypatch):
    """Site 3 of 5 (models/layers.py, the BatchNorm backward riding in the weight gradient).  6 x 6 maps have no Winograd weight gradient,
    so this case runs at the smallest shape whose weight gradient takes a rider, 3 x 64 x 14 x 14 -> 128."""
    monkeypatch.setattr(fused_bn, 'ENABLE_WGRAD_RIDER', True)
    torch.manual_seed(4)
    net = fused_bn.FusedSequential(
        nl.SharableConv2d(64, 64, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
        nl.SharableConv2d(64, 128, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(128), nn.ReLU(inplace=True)).to(DEV).train()
    assert _lib.lib().cpg_conv2d_wgrad_rider_supported(ctypes.byref(_desc(3, 64, 14, 14, 128, 3))) == 1
    g = torch.Generator(device='cpu').manual_seed(9)
    x = torch.randn(3, 64, 14, 14, generator=g).to(DEV).requires_grad_(True)
    loss = net(x).square().mean()
    state = _raise_in(monkeypatch, 'cpg_conv2d_wgrad', after='cpg_conv2d_wgrad_attach_bn_bwd')
    with pytest.raises(Exception, match='cpg_conv2d_wgrad'):
        loss.backward()
    assert state['thread'] is not None
    # (monkeypatch.undo() would also put ENABLE_WGRAD_RIDER back: harmless, nothing of the library's Python layer runs below)
    monkeypatch.undo()
    (rc, text), thread = _on_backward_thread(_null_wgrad)
    assert thread == state['thread']
    assert rc == _lib.CPG_E_INVALID and 'null pointer' in text, (rc, text)
