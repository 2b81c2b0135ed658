"""Host-side contract of the pooled inference epilogue (cpg_conv2d_fwd_bn_eval_pool): the header / ctypes table / version script agreement
on the two symbols, the planner's answers and the refusals, the argument errors (the rules tests/test_eval_epilogue_host.py holds the
siblings to), what SharableConv2d.forward_bn_eval_pool refuses, the method PlainConv2d borrows and the steps FusedSequential takes with
the switch off and on.  No GPU: every library call here returns before anything is launched."""
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
from cpg_amd.models.fused_bn import FusedSequential
from cpg_amd.models.layers import SharableConv2d
from cpg_amd.packnet_models.layers import PlainConv2d

NEW = ('cpg_conv2d_fwd_bn_eval_pool_supported', 'cpg_conv2d_fwd_bn_eval_pool')
UNSUPPORTED = -2
ONE = ctypes.c_void_p(16)           # a non-null pointer nothing reads: every call here returns before anything is launched
FAR = ctypes.c_void_p(1 << 40)      # ... and one far from it (y_pooled must not overlap x)
BYTES = 1 << 20


def _desc(N=2, C=32, H=14, W=14, K=64, k=3, s=1, G=1):
    d = L.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, k, k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = k // 2
    d.dil_h = d.dil_w = 1
    d.groups = G
    return d


def _query(d):
    return L.lib().cpg_conv2d_fwd_bn_eval_pool_supported(None if d is None else ctypes.byref(d))


def _call(d, x=ONE, w=ONE, y=FAR, gamma=ONE, beta=ONE, mean=ONE, var=ONE):
    return L.lib().cpg_conv2d_fwd_bn_eval_pool(None if d is None else ctypes.byref(d), x, w, None, 0.0, None, gamma, beta, mean, var, 1e-5, 1,
                                               y, None, ONE, BYTES, None)


def _refused(rc, status):
    text = L.lib().cpg_last_error().decode()
    assert rc == status, (rc, text)
    assert 'cpg_conv2d_fwd_bn_eval_pool:' in text or 'cpg_conv2d_fwd_bn_eval_pool(' in text, text


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
    assert L.ABI_VERSION == 3 and L.lib().cpg_version() == 3          # unchanged: callers probe for the symbol
    assert name in L.EXPORTS
    res, args = L._SIGNATURES[name]
    assert (res, args) == _header_prototype(name)
    fn = getattr(L.lib(), name)
    assert fn.restype is res and list(fn.argtypes) == args
    assert re.search(r'^\s+%s;$' % name, open(build.export_map()).read(), re.M)
    # the call takes exactly the arguments of cpg_conv2d_fwd_bn_eval
    assert _header_prototype('cpg_conv2d_fwd_bn_eval_pool') == _header_prototype('cpg_conv2d_fwd_bn_eval')


# id -> (descriptor, options, answer)
QUERIES = {
    'wg1': (_desc(4, 32, 28, 28, 48), {}, 1),
    'wg1-grown78': (_desc(2, 78, 56, 56, 78), {}, 1),
    'wg3': (_desc(2, 128, 14, 14, 256), {}, 1),
    'wg3-grown313': (_desc(2, 156, 28, 28, 313), {}, 1),
    'wg3-grown627': (_desc(2, 313, 14, 14, 627), {}, 1),
    'wg2': (_desc(2, 64, 16, 16, 96), {'CPG_WINO_KERNEL': 2}, 1),
    'one-tile': (_desc(3, 64, 2, 2, 64), {}, 1),
    'odd-tiles-per-row': (_desc(2, 64, 6, 10, 64), {}, 1),
    'vgg16-64@224': (_desc(256, 64, 224, 224, 64), {}, 1),
    'odd-map': (_desc(3, 128, 7, 7, 128), {}, 0),
    'odd-width': (_desc(2, 128, 8, 7, 128), {}, 0),
    'no-wino': (_desc(2, 128, 14, 14, 256), {'CPG_NO_WINO': 1}, 0),
    'block-kernel': (_desc(2, 128, 14, 14, 256), {'CPG_WINO_KERNEL': 0}, 0),
    'stem': (_desc(2, 3, 32, 32, 64), {}, 0),                       # 3 input channels: a direct tile
    'conv3x3-off': (_desc(2, 128, 14, 14, 256), {'CPG_DISABLE_CONV3X3': 1}, 0),
    '3x3-s2': (_desc(s=2), {}, 0),
    '1x1': (_desc(k=1), {}, 0),
    '5x5': (_desc(k=5), {}, 0),
    'groups-2': (_desc(G=2), {}, 0),
}


@pytest.mark.parametrize('qid', sorted(QUERIES))
def test_planner_answers_and_the_call_agrees(qid, libopt):
    """The query is the planner's answer under the current option table, and the call refuses exactly what it answers 0 for -- before
    anything is launched (these pointers are never read)."""
    d, opts, answer = QUERIES[qid]
    for k, v in opts.items():
        libopt.set(k, v)
    assert _query(d) == answer, qid
    if answer:
        assert L.lib().cpg_conv2d_winograd(ctypes.byref(d), 3) == 1 and L.lib().cpg_conv2d_fwd_bn_eval_supported(ctypes.byref(d)) == 1
        _refused(_call(d, x=None), L.CPG_E_INVALID)        # (admitted: the next check is the pointers')
    else:
        _refused(_call(d), UNSUPPORTED)
        _refused(_call(d, x=None), UNSUPPORTED)            # the shape is judged before the pointers, as in cpg_conv2d_fwd_bn_eval


def test_options_move_the_answer_with_the_plan():
    d = QUERIES['wg3'][0]
    assert _query(d) == 1
    with L.option('CPG_NO_WINO', 1):
        assert _query(d) == 0
    for kernel, answer in ((0, 0), (1, 1), (2, 1), (3, 1)):          # block | wave | pair | 64
        with L.option('CPG_WINO_KERNEL', kernel):
            assert _query(d) == answer, kernel
    with L.option('CPG_NO_DEAD_SKIP', 1):
        assert _query(d) == 1
    assert _query(d) == 1


@pytest.mark.parametrize('arg', ['x', 'w', 'y', 'gamma', 'beta', 'mean', 'var'])
def test_null_tensor(arg):
    _refused(_call(QUERIES['wg1'][0], **{arg: None}), L.CPG_E_INVALID)


def test_null_and_malformed_descriptor():
    assert _query(None) == 0
    assert _call(None) == L.CPG_E_INVALID
    bad = _desc()
    bad.groups = 3                   # divides neither C nor K
    assert _query(bad) == 0
    for rc in (_call(bad), _call(bad, x=None)):
        assert rc == L.CPG_E_INVALID and b'groups' in L.lib().cpg_last_error()
    neg = _desc()
    neg.H = 0
    assert _query(neg) == 0 and _call(neg) == L.CPG_E_INVALID


def test_output_may_not_overlap_the_input():
    d = QUERIES['wg1'][0]
    _refused(_call(d, x=ONE, y=ONE), L.CPG_E_INVALID)
    assert b'overlaps' in L.lib().cpg_last_error()
    inside = ctypes.c_void_p(16 + 4 * (d.N * d.C * d.H * d.W - 1))      # the last element of x
    _refused(_call(d, x=ONE, y=inside), L.CPG_E_INVALID)


# ---------------------------------------------------------------------------------------------------------------- the Python layers
class _DeviceLike(torch.Tensor):
    """A CPU tensor that says it is on the device: what the steps and methods look at before they touch the library."""
    is_cuda = True


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError('forward_bn_eval_pool reached the library (%s)' % name)


@pytest.mark.parametrize('conv', [SharableConv2d(16, 16, 3, 1, 1), PlainConv2d(16, 16, 3, 1, 1)], ids=['sharable', 'plain'])
def test_refused_before_any_library_call(conv, monkeypatch):
    from cpg_amd.models import layers as nl
    monkeypatch.setattr(nl, '_lib', _NoLibrary())
    bn = nn.BatchNorm2d(16).eval()
    x = torch.zeros(2, 16, 8, 8)
    with torch.enable_grad():
        assert conv.forward_bn_eval_pool(x, bn) is None
        assert conv.forward_bn_eval_pool(x.as_subclass(_DeviceLike), bn) is None       # grad mode alone refuses
    with torch.no_grad():
        assert conv.forward_bn_eval_pool(x, bn) is None            # a CPU tensor


def test_plain_conv_borrows_the_method():
    assert PlainConv2d.forward_bn_eval_pool is SharableConv2d.forward_bn_eval_pool
    assert PlainConv2d._forward_eval is SharableConv2d._forward_eval
    conv = PlainConv2d(16, 32, 3, padding=1)
    names = set(re.findall(r'self\.(\w+)', inspect.getsource(SharableConv2d.forward_bn_eval_pool)))
    assert '_forward_eval' in names
    names |= set(re.findall(r'self\.(\w+)', inspect.getsource(SharableConv2d._forward_eval)))
    allowed = {'piggymask', 'info', '_math', 'groups', 'stride', 'padding', 'dilation', 'weight', 'bias', 'forward', '_forward_eval'}
    assert names <= allowed, names - allowed
    for name in names:
        assert hasattr(conv, name), name


class _Conv(nn.Module):
    """A conv that records which of its entry points FusedSequential called (no library, CPU tensors made to look like device ones)."""

    def __init__(self, calls, pool_answer):
        super().__init__()
        self.calls, self.pool_answer = calls, pool_answer

    def forward_bn_eval_pool(self, x, bn, relu=True, skip_stats=None):
        self.calls.append('pool')
        return None if self.pool_answer is None else x[:, :, ::2, ::2] + self.pool_answer

    def forward_bn_eval(self, x, bn, relu=True, skip_stats=None):
        self.calls.append('bn_eval')
        return x + 1

    def forward(self, x, **kw):
        self.calls.append('forward')
        return x


def _steps(monkeypatch, switch, pool_answer, grad=False, with_pool=True):
    """The calls a conv -> BatchNorm2d(eval) -> ReLU [-> MaxPool2d(2, 2)] group makes, and which step answered."""
    calls, taken = [], []
    mods = [_Conv(calls, pool_answer), nn.BatchNorm2d(4).eval(), nn.ReLU()] + ([nn.MaxPool2d(2, 2)] if with_pool else [])
    seq = FusedSequential(*mods).eval()
    monkeypatch.setattr(FusedSequential, 'fuse_eval_pool', switch)
    for name in ('_bn_relu', '_lone_bn', '_conv_bn_relu_pool_eval', '_conv_bn_relu_eval', '_conv_bn_eval', '_stem', '_conv_bn_relu_pool', '_conv'):
        def spy(window, input, stats, hint, _f=getattr(seq, name), _n=name):
            done = _f(window, input, stats, hint)
            if done is not None:
                taken.append(_n)
            return done
        monkeypatch.setattr(seq, name, spy)
    monkeypatch.setattr(fused_bn, 'fusable', lambda m, x: False)       # (the BatchNorm passes are not this test's: stock modules run them)
    x = torch.zeros(1, 4, 4, 4).as_subclass(_DeviceLike)
    with (torch.enable_grad() if grad else torch.no_grad()):
        y = seq(x)
    return calls, taken, y


def test_switch_off_takes_exactly_todays_steps(monkeypatch):
    assert isinstance(FusedSequential.fuse_eval_pool, bool)
    calls, taken, y = _steps(monkeypatch, False, 5.0)
    assert 'pool' not in calls and '_conv_bn_relu_pool_eval' not in taken
    assert calls == ['forward'] and taken[0] == '_conv', (calls, taken)              # the plain conv, then the BatchNorm -> ReLU -> pool modules
    assert tuple(y.shape) == (1, 4, 2, 2)
    calls, taken, _ = _steps(monkeypatch, False, 5.0, with_pool=False)
    assert calls == ['bn_eval'] and taken == ['_conv_bn_relu_eval']


def test_switch_on_tries_the_pooled_call_first_and_falls_back(monkeypatch):
    calls, taken, y = _steps(monkeypatch, True, 5.0)
    assert calls == ['pool'] and taken == ['_conv_bn_relu_pool_eval'], (calls, taken)        # 4 modules consumed by one step
    assert tuple(y.shape) == (1, 4, 2, 2) and float(y.min()) == 5.0
    # the method refuses: the steps of the switch-off run, exactly
    off_calls, off_taken, off_y = _steps(monkeypatch, False, None)
    calls, taken, y = _steps(monkeypatch, True, None)
    assert calls == ['pool'] + off_calls and taken == off_taken and torch.equal(y.as_subclass(torch.Tensor), off_y.as_subclass(torch.Tensor))
    # grad mode, and a group without a pool: the step declines without calling the conv
    calls, taken, _ = _steps(monkeypatch, True, 5.0, grad=True)
    assert 'pool' not in calls and '_conv_bn_relu_pool_eval' not in taken
    calls, taken, _ = _steps(monkeypatch, True, 5.0, with_pool=False)
    assert calls == ['bn_eval'] and taken == ['_conv_bn_relu_eval']


def test_skip_log_gets_one_entry_per_pooled_call(monkeypatch):
    seen = []

    class Conv(_Conv):
        def forward_bn_eval_pool(self, x, bn, relu=True, skip_stats=None):
            seen.append(skip_stats)
            return x[:, :, ::2, ::2]
    seq = FusedSequential(Conv([], 0.0), nn.BatchNorm2d(4).eval(), nn.ReLU(), nn.MaxPool2d(2, 2)).eval()
    monkeypatch.setattr(FusedSequential, 'fuse_eval_pool', True)
    monkeypatch.setattr(FusedSequential, 'skip_log', [])
    with torch.no_grad():
        seq(torch.zeros(1, 4, 4, 4).as_subclass(_DeviceLike))
    assert len(FusedSequential.skip_log) == 1 and seen[0] is FusedSequential.skip_log[0] and seen[0].dtype == torch.int32


def test_docs_and_tool():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'cpg_conv2d_fwd_bn_eval_pool' in text and 'fuse_eval_pool' in text
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'vgg_eval_pool_fuse.md'))
    assert 'vgg16' in open(os.path.join(ROOT, 'tools', 'eval_bench.py')).read()
