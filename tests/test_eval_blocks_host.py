"""Host-side contract of the residual topologies' inference entry points (cpg_conv2d_fwd_bn_eval on the pointwise and 3x3 s2 shapes,
cpg_conv2d_fwd_bn_eval_add): support queries, the library switches, the ctypes table against the header, the fp64 reference the GPU
tests use, and the method PlainConv2d borrows.  No GPU: every library call here returns before anything is launched."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import _evalres as R
import cpg_amd._lib as L


def _desc(N=4, C=32, H=14, W=14, K=64, k=1, s=1, p=0, G=1):
    d = L.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, k, k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = p
    d.dil_h = d.dil_w = 1
    d.groups = G
    return d


# id -> (descriptor, cpg_conv2d_fwd_bn_eval_supported, cpg_conv2d_fwd_bn_eval_add_supported)
QUERIES = {
    '1x1-s1': (_desc(), 1, 1),
    '1x1-s2': (_desc(s=2), 1, 1),
    '1x1-c24': (_desc(C=24), 0, 0),
    '3x3-s2': (_desc(k=3, s=2, p=1), 1, 0),
    '3x3-s1-p1': (_desc(k=3, s=1, p=1), 1, 0),
    '7x7-s2': (_desc(C=3, H=64, W=64, k=7, s=2, p=3), 0, 0),
    'groups-2': (_desc(G=2), 0, 0),
}


def _answers(d):
    lib = L.lib()
    return lib.cpg_conv2d_fwd_bn_eval_supported(ctypes.byref(d)), lib.cpg_conv2d_fwd_bn_eval_add_supported(ctypes.byref(d))


@pytest.mark.parametrize('qid', sorted(QUERIES))
def test_support_queries(qid):
    d, plain, add = QUERIES[qid]
    assert _answers(d) == (plain, add), qid
    assert L.lib().cpg_conv2d_winograd(ctypes.byref(d), 3) == 0 or qid == '3x3-s1-p1'
    if not add:       # refused from the descriptor alone, before any pointer is looked at
        rc = L.lib().cpg_conv2d_fwd_bn_eval_add(ctypes.byref(d), *([None] * 3), 0.0, *([None] * 5), 1e-5, None, 1, None, None, 0, None)
        assert rc == -2, (qid, rc)                          # CPG_E_UNSUPPORTED


@pytest.mark.parametrize('option,qid', [('CPG_DISABLE_CONV1X1', '1x1-s1'), ('CPG_DISABLE_CONV1X1', '1x1-s2'),
                                        ('CPG_DISABLE_CONV3X3', '3x3-s1-p1'), ('CPG_DISABLE_CONV3X3', '3x3-s2'), ('CPG_NO_S2', '3x3-s2')])
def test_library_options_take_their_class_away(option, qid):
    d, plain, add = QUERIES[qid]
    assert _answers(d) == (plain, add)
    with L.option(option, 1):
        assert _answers(d) == (0, 0), (option, qid)
    assert _answers(d) == (plain, add)


def test_options_leave_the_other_classes_alone():
    with L.option('CPG_NO_S2', 1):
        assert _answers(QUERIES['3x3-s1-p1'][0]) == (1, 0) and _answers(QUERIES['1x1-s2'][0]) == (1, 1)
    with L.option('CPG_DISABLE_CONV1X1', 1):
        assert _answers(QUERIES['3x3-s2'][0]) == (1, 0)


_CTYPES = {'int32_t': ctypes.c_int32, 'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _header_prototype(name):
    """(restype, argtypes) of `name` as include/cpg_hip.h declares it: pointers to cpg_conv_desc / anything else -> the binding's
    descriptor pointer / c_void_p."""
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


@pytest.mark.parametrize('name', ['cpg_conv2d_fwd_bn_eval_add_supported', 'cpg_conv2d_fwd_bn_eval_add'])
def test_abi_table_has_the_new_slots(name):
    assert L.ABI_VERSION == 3 and L.lib().cpg_version() == 3
    assert name in L.EXPORTS
    res, args = L._SIGNATURES[name]
    assert (res, args) == _header_prototype(name)
    fn = getattr(L.lib(), name)
    assert fn.restype is res and list(fn.argtypes) == args
    assert len(_header_prototype('cpg_conv2d_fwd_bn_eval_add')[1]) == 17


def test_null_residual_is_invalid():
    d = QUERIES['1x1-s1'][0]
    one = ctypes.c_void_p(16)          # (never dereferenced: the call returns on the NULL residual)
    rc = L.lib().cpg_conv2d_fwd_bn_eval_add(ctypes.byref(d), one, one, None, 0.0, None, one, one, one, one, 1e-5, None, 1, one, one, 1 << 20, None)
    assert rc == L.CPG_E_INVALID and b'residual' in L.lib().cpg_last_error()


@pytest.mark.parametrize('k,s,p', [(1, 1, 0), (1, 2, 0), (3, 2, 1), (3, 1, 1)])
def test_reference_agrees_with_torch(k, s, p):
    """_evalres against fp64 F.conv2d + F.batch_norm(training=False) + add + relu on the CPU, with a piggymask and a conv bias; and
    the bound's parts are what the docstring says."""
    g = torch.Generator().manual_seed(7 + k + s)
    N, C, H, W, K = 2, 16, 9, 7, 24
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, k, k, generator=g) * 0.2
    pm = torch.where(torch.rand(K, C, k, k, generator=g) < 0.8, 0.01, 0.001)
    bias, beta, mean = (torch.randn(K, generator=g) for _ in range(3))
    gamma = torch.randn(K, generator=g)
    var = torch.rand(K, generator=g) * 1.5 + 0.5
    weff = (w * (pm > 5e-3).float()).double()
    conv = F.conv2d(x.double(), weff, bias.double(), stride=s, padding=p)
    bn = F.batch_norm(conv, mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    res = torch.randn(bn.shape, generator=g)
    for residual in (None, res):
        for relu in (False, True):
            want = bn if residual is None else bn + residual.double()
            want = F.relu(want) if relu else want
            ref, bound = R.eval_res_ref(x, w, pm, bias, gamma, beta, mean, var, 1e-5, s, p, residual, relu, threshold=5e-3)
            assert ref.dtype == torch.float64 and ref.shape == want.shape
            assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
            assert bool((bound > 0).all())
    parts = R.conv_parts(x, w, pm, s, p, 5e-3)
    assert parts[2] == C * k * k
    _, ct, st = R.eval_res_terms(parts, bias, gamma, beta, mean, var, 1e-5)
    _, ct_r, st_r = R.eval_res_terms(parts, bias, gamma, beta, mean, var, 1e-5, res)
    sabs = (gamma.double() / torch.sqrt(var.double() + 1e-5)).abs()
    assert torch.equal(ct, ct_r) and torch.allclose(st_r - st, 2 * R.U32 * res.double().abs(), rtol=1e-12, atol=0)
    assert torch.allclose(ct, C * k * k * R.U32 * sabs[:, None, None] * F.conv2d(x.double().abs(), weff.abs(), None, stride=s, padding=p), rtol=1e-12)
    assert torch.allclose(st[0, :, 0, 0], R.U32 * 8 * (sabs * (bias.double().abs() + mean.double().abs()) + beta.double().abs()), rtol=1e-12)


def test_plain_conv_borrows_the_tail_method():
    """PlainConv2d.forward_bn_eval_add IS SharableConv2d's, and every attribute that method reads exists on a PlainConv2d (the rule
    tests/test_packnet_host.py holds the other borrowed methods to)."""
    from cpg_amd.models.layers import SharableConv2d
    from cpg_amd.packnet_models.layers import PlainConv2d
    assert PlainConv2d.forward_bn_eval_add is SharableConv2d.forward_bn_eval_add
    assert PlainConv2d._forward_eval is SharableConv2d._forward_eval          # the frame the method runs in: the same function on both
    conv = PlainConv2d(16, 32, 1, bias=False)
    names = set(re.findall(r'self\.(\w+)', inspect.getsource(SharableConv2d.forward_bn_eval_add)))
    assert '_forward_eval' in names
    names |= set(re.findall(r'self\.(\w+)', inspect.getsource(SharableConv2d._forward_eval)))
    assert {'weight', 'piggymask', 'info', 'stride', 'groups'} <= names
    for name in names:
        assert hasattr(conv, name), name


def test_switch_defaults_and_docs():
    from cpg_amd.models import fused_bn
    assert isinstance(fused_bn.FUSE_EVAL_BLOCKS, bool)
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'cpg_conv2d_fwd_bn_eval_add' in text and 'FUSE_EVAL_BLOCKS' in text
    digest = open(os.path.join(ROOT, 'tools', 'build_digest.py')).read()
    assert "'cpg_conv2d_fwd_bn_eval_add_supported'" in digest
