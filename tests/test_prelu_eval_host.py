"""Host-side contract of SphereNet's inference epilogue (cpg_conv2d_fwd_prelu_eval): what SharableConv2d.forward_prelu_eval refuses
before it touches the library, the method PlainConv2d borrows, the header / ctypes table / version script agreement on the two new
symbols, the planner's answers and the argument errors.  No GPU: every library call here returns before anything is launched."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT

import cpg_amd._lib as L
from cpg_amd.models import fused_bn
from cpg_amd.models.layers import SharableConv2d
from cpg_amd.packnet_models.layers import PlainConv2d

NEW = ('cpg_conv2d_fwd_prelu_eval_supported', 'cpg_conv2d_fwd_prelu_eval')


def _desc(N=4, C=32, H=14, W=14, K=64, k=3, s=1, G=1):
    d = L.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, k, k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = k // 2
    d.dil_h = d.dil_w = 1
    d.groups = G
    return d


class _NoLibrary(object):
    """Stands in for cpg_amd._lib: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError('forward_prelu_eval reached the library (%s)' % name)


@pytest.mark.parametrize('conv', [SharableConv2d(8, 16, 3, 1, 1), PlainConv2d(8, 16, 3, 1, 1)], ids=['sharable', 'plain'])
def test_refused_before_any_library_call(conv, monkeypatch):
    """Grad mode, a module that is not a plain nn.PReLU, a wrong slope count: None, and nothing of the library is touched."""
    from cpg_amd.models import layers as nl
    monkeypatch.setattr(nl, '_lib', _NoLibrary())
    x = torch.zeros(2, 8, 6, 6)

    class MyPReLU(nn.PReLU):
        pass
    with torch.enable_grad():
        assert conv.forward_prelu_eval(x, nn.PReLU(16)) is None
    with torch.no_grad():
        assert conv.forward_prelu_eval(x, nn.ReLU()) is None
        assert conv.forward_prelu_eval(x, MyPReLU(16)) is None
        assert conv.forward_prelu_eval(x, nn.PReLU(8)) is None
        assert conv.forward_prelu_eval(x, nn.PReLU(2)) is None
        assert conv.forward_prelu_eval(torch.zeros(2, 4, 6, 6), nn.PReLU(16)) is None      # channels do not match the weight


def test_plain_conv_borrows_the_method():
    """PlainConv2d.forward_prelu_eval IS SharableConv2d's, and it reads only what a PlainConv2d has (the rule of tests/test_packnet_host.py)."""
    assert PlainConv2d.forward_prelu_eval is SharableConv2d.forward_prelu_eval
    assert PlainConv2d._forward_eval is SharableConv2d._forward_eval          # the frame the method runs in: the same function on both
    conv = PlainConv2d(16, 32, 3, padding=1)
    names = set(re.findall(r'self\.(\w+)', inspect.getsource(SharableConv2d.forward_prelu_eval)))
    assert '_forward_eval' in names
    names |= set(re.findall(r'self\.(\w+)', inspect.getsource(SharableConv2d._forward_eval)))
    assert {'weight', 'piggymask', 'info', 'stride', 'groups', 'bias'} <= names
    allowed = {'piggymask', 'info', '_math', 'groups', 'stride', 'padding', 'dilation', 'weight', 'bias', 'forward', '_forward_eval'}
    assert names <= allowed, names - allowed
    for name in names:
        assert hasattr(conv, name), name


_CTYPES = {'int32_t': ctypes.c_int32, 'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _header_prototype(name):
    text = open(os.path.join(ROOT, 'include', 'cpg_hip.h')).read()
    m = re.search(r'^(\w+)\s+%s\(([^;]*)\);' % name, text, re.M)
    assert m, name
    args = []
    for a in m.group(2).split(','):
        a = ' '.join(a.split())
        if '*' in a:
            args.append(ctypes.POINTER(L.ConvDesc) if 'cpg_conv_desc' in a else ctypes.c_void_p)
        else:
            args.append(_CTYPES[a.replace('const ', '').split()[0]])
    return _CTYPES[m.group(1)], args


@pytest.mark.parametrize('name', NEW)
def test_header_table_and_version_script_agree(name):
    from cpg_amd import build
    assert L.ABI_VERSION == 3 and L.lib().cpg_version() == 3
    assert name in L.EXPORTS
    res, args = L._SIGNATURES[name]
    assert (res, args) == _header_prototype(name)
    fn = getattr(L.lib(), name)                       # exported by the built library
    assert fn.restype is res and list(fn.argtypes) == args
    assert re.search(r'^\s+%s;$' % name, open(build.export_map()).read(), re.M)
    assert len(_header_prototype('cpg_conv2d_fwd_prelu_eval')[1]) == 14


# id -> (descriptor, answer without a residual, answer with one)
QUERIES = {
    '3x3-s1': (_desc(), 1, 1),
    '3x3-s1-odd': (_desc(C=128, K=128, H=7, W=7), 1, 1),
    '3x3-s2': (_desc(s=2), 1, 0),
    '3x3-s2-stem': (_desc(C=3, H=112, W=112, s=2), 0, 0),
    '1x1': (_desc(k=1), 0, 0),
    '1x1-s2': (_desc(k=1, s=2), 0, 0),
    '5x5': (_desc(k=5), 0, 0),
    'groups-2': (_desc(G=2), 0, 0),
}


def _answers(d):
    lib = L.lib()
    return lib.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 0), lib.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 1)


@pytest.mark.parametrize('qid', sorted(QUERIES))
def test_planner_answers_and_refusals(qid):
    d, plain, add = QUERIES[qid]
    assert _answers(d) == (plain, add), qid
    assert L.lib().cpg_conv2d_fwd_bn_eval_supported(ctypes.byref(d)) >= plain       # nothing the BatchNorm entry point refuses
    one = ctypes.c_void_p(16)          # (never dereferenced: each call below returns before anything is launched)
    for with_res, ok in ((0, plain), (1, add)):
        if not ok:
            rc = L.lib().cpg_conv2d_fwd_prelu_eval(ctypes.byref(d), one, one, None, 0.0, None, one, d.K, one if with_res else None, one, None,
                                                   one, 1 << 20, None)
            assert rc == -2, (qid, with_res, rc)                    # CPG_E_UNSUPPORTED


def test_argument_errors():
    d = QUERIES['3x3-s1'][0]
    one = ctypes.c_void_p(16)
    call = L.lib().cpg_conv2d_fwd_prelu_eval
    assert call(ctypes.byref(d), one, one, None, 0.0, None, None, d.K, None, one, None, one, 1 << 20, None) == L.CPG_E_INVALID    # NULL slope
    for n in (0, 2, d.K - 1, d.K + 1):
        assert call(ctypes.byref(d), one, one, None, 0.0, None, one, n, None, one, None, one, 1 << 20, None) == L.CPG_E_INVALID, n
        assert b'n_slopes' in L.lib().cpg_last_error()
    assert call(None, one, one, None, 0.0, None, one, 1, None, one, None, one, 1 << 20, None) == L.CPG_E_INVALID


def test_options_move_the_answer_with_the_plan():
    """The query is the planner's: the switches that take the class away from cpg_conv2d_fwd_bn_eval take it away here, and the
    channel-split 14 x 14 tile (no fused epilogue) answers 0."""
    d = _desc(N=2, C=128, K=256)
    assert _answers(d) == (1, 1)
    with L.option('CPG_DISABLE_CONV3X3', 1):
        assert _answers(d) == (0, 0) and _answers(QUERIES['3x3-s2'][0]) == (0, 0)
    with L.option('CPG_NO_S2', 1):
        assert _answers(d) == (1, 1) and _answers(QUERIES['3x3-s2'][0]) == (0, 0)
    with L.option('CPG_NO_WINO', 1):
        assert _answers(d) == (1, 1)
        for force in (7, 8):
            with L.option('CPG_C3_FORCE', force):
                assert _answers(d) == ((1, 1) if force == 7 else (0, 0)), force
    assert _answers(d) == (1, 1)


def test_switch_and_docs():
    assert isinstance(fused_bn.FUSE_EVAL_PRELU, bool)
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'cpg_conv2d_fwd_prelu_eval' in text and 'FUSE_EVAL_PRELU' in text
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'spherenet_eval_fuse.md'))


def test_helpers_try_the_fused_call_first_under_no_grad(monkeypatch):
    """conv_prelu / conv_prelu_skip hand the pair to forward_prelu_eval under no_grad with the switch on, and to nothing new otherwise."""
    calls = []

    class Conv(nn.Module):
        bias = None

        def forward_prelu_eval(self, x, mod, res=None, skip_stats=None):
            calls.append(res is not None)
            return x + 1

        def forward(self, x, **kw):
            return x
    conv, mod, x = Conv(), nn.PReLU(3), torch.zeros(1, 3, 2, 2)
    monkeypatch.setattr(fused_bn, 'FUSE_EVAL_PRELU', True)
    with torch.no_grad():
        assert torch.equal(fused_bn.conv_prelu(conv, mod, x, res=x), x + 1)
        y, skip = fused_bn.conv_prelu_skip(conv, mod, x)
        assert torch.equal(y, x + 1) and skip is x
        assert calls == [True, False]
        monkeypatch.setattr(fused_bn, 'FUSE_EVAL_PRELU', False)
        assert torch.equal(fused_bn.conv_prelu(conv, mod, x), mod(x)) and calls == [True, False]
    monkeypatch.setattr(fused_bn, 'FUSE_EVAL_PRELU', True)
    assert torch.equal(fused_bn.conv_prelu(conv, mod, x), mod(x)) and calls == [True, False]       # grad mode: as before
