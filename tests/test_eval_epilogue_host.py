"""What the three inference entry points of the C ABI (cpg_conv2d_fwd_bn_eval, _bn_eval_add, _prelu_eval) refuse before any launch:
the status code, and the public entry point's name in cpg_last_error().  Called through ctypes with pointers that are never
dereferenced; needs the built library and no GPU.  Where two things are wrong at once, the status is that of the check that comes first."""
import ctypes

import pytest

import cpg_amd._lib as L

UNSUPPORTED = -2
ONE = ctypes.c_void_p(16)           # a non-null pointer nothing reads: every call here returns before anything is launched
BYTES = 1 << 20


def _desc(C=16, K=32, k=3, s=1):
    d = L.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = 2, C, 8, 8, K, k, k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = k // 2
    d.dil_h = d.dil_w = 1
    d.groups = 1
    return d


DESCS = {'3x3': _desc(), '3x3s2': _desc(s=2), '1x1': _desc(k=1), '5x5': _desc(k=5)}


def _bn_eval(d, x=ONE, w=ONE, y=ONE, gamma=ONE, beta=ONE, mean=ONE, var=ONE):
    return L.lib().cpg_conv2d_fwd_bn_eval(ctypes.byref(d), x, w, None, 0.0, None, gamma, beta, mean, var, 1e-5, 1, y, None, ONE, BYTES, None)


def _bn_eval_add(d, x=ONE, w=ONE, y=ONE, gamma=ONE, beta=ONE, mean=ONE, var=ONE, residual=ONE):
    return L.lib().cpg_conv2d_fwd_bn_eval_add(ctypes.byref(d), x, w, None, 0.0, None, gamma, beta, mean, var, 1e-5, residual, 1, y, ONE, BYTES,
                                              None)


def _prelu_eval(d, x=ONE, w=ONE, y=ONE, slope=ONE, n_slopes=None, residual=None):
    return L.lib().cpg_conv2d_fwd_prelu_eval(ctypes.byref(d), x, w, None, 0.0, None, slope, d.K if n_slopes is None else n_slopes, residual, y,
                                             None, ONE, BYTES, None)


def _refused(rc, status, name):
    text = L.lib().cpg_last_error().decode()
    assert rc == status, (rc, text)
    # the public entry point itself, not one whose name merely begins with it
    assert (name + ':') in text or (name + '(') in text, text


@pytest.mark.parametrize('arg', ['x', 'w', 'y'])
def test_null_tensor(arg):
    for did in ('3x3', '3x3s2', '1x1'):
        _refused(_bn_eval(DESCS[did], **{arg: None}), L.CPG_E_INVALID, 'cpg_conv2d_fwd_bn_eval')
    _refused(_bn_eval_add(DESCS['1x1'], **{arg: None}), L.CPG_E_INVALID, 'cpg_conv2d_fwd_bn_eval_add')
    for did in ('3x3', '3x3s2'):
        _refused(_prelu_eval(DESCS[did], **{arg: None}), L.CPG_E_INVALID, 'cpg_conv2d_fwd_prelu_eval')


@pytest.mark.parametrize('arg', ['gamma', 'beta', 'mean', 'var'])
def test_null_batchnorm_parameter(arg):
    for did in ('3x3', '3x3s2', '1x1'):
        _refused(_bn_eval(DESCS[did], **{arg: None}), L.CPG_E_INVALID, 'cpg_conv2d_fwd_bn_eval')
    _refused(_bn_eval_add(DESCS['1x1'], **{arg: None}), L.CPG_E_INVALID, 'cpg_conv2d_fwd_bn_eval_add')


def test_null_slope():
    for did in ('3x3', '3x3s2'):
        _refused(_prelu_eval(DESCS[did], slope=None), L.CPG_E_INVALID, 'cpg_conv2d_fwd_prelu_eval')


@pytest.mark.parametrize('did', ['3x3', '3x3s2'])
def test_slope_count(did):
    d = DESCS[did]
    for n in (0, 2, d.K - 1, d.K + 1, -1):
        _refused(_prelu_eval(d, n_slopes=n), L.CPG_E_INVALID, 'cpg_conv2d_fwd_prelu_eval')
        assert b'n_slopes' in L.lib().cpg_last_error()


def test_residual_on_the_strided_3x3():
    _refused(_prelu_eval(DESCS['3x3s2'], residual=ONE), UNSUPPORTED, 'cpg_conv2d_fwd_prelu_eval')
    _refused(_bn_eval_add(DESCS['3x3s2']), UNSUPPORTED, 'cpg_conv2d_fwd_bn_eval_add')


def test_bn_eval_add_takes_the_pointwise_shapes_only():
    _refused(_bn_eval_add(DESCS['3x3']), UNSUPPORTED, 'cpg_conv2d_fwd_bn_eval_add')
    _refused(_bn_eval_add(DESCS['1x1'], residual=None), L.CPG_E_INVALID, 'cpg_conv2d_fwd_bn_eval_add')
    assert b'residual' in L.lib().cpg_last_error()
    _refused(_bn_eval_add(DESCS['3x3'], residual=None), UNSUPPORTED, 'cpg_conv2d_fwd_bn_eval_add')      # the shape is judged first


def test_prelu_eval_has_no_pointwise_kernel():
    for residual in (None, ONE):
        _refused(_prelu_eval(DESCS['1x1'], residual=residual), UNSUPPORTED, 'cpg_conv2d_fwd_prelu_eval')


def test_5x5():
    d = DESCS['5x5']
    _refused(_bn_eval(d), UNSUPPORTED, 'cpg_conv2d_fwd_bn_eval')
    _refused(_bn_eval_add(d), UNSUPPORTED, 'cpg_conv2d_fwd_bn_eval_add')
    _refused(_prelu_eval(d), UNSUPPORTED, 'cpg_conv2d_fwd_prelu_eval')
    _refused(_prelu_eval(d, residual=ONE), UNSUPPORTED, 'cpg_conv2d_fwd_prelu_eval')
    # the BatchNorm entry points judge the shape before the pointers, the PReLU one the pointers and the slope count first
    _refused(_bn_eval(d, x=None), UNSUPPORTED, 'cpg_conv2d_fwd_bn_eval')
    _refused(_bn_eval_add(d, residual=None), UNSUPPORTED, 'cpg_conv2d_fwd_bn_eval_add')
    _refused(_prelu_eval(d, x=None), L.CPG_E_INVALID, 'cpg_conv2d_fwd_prelu_eval')
    _refused(_prelu_eval(d, n_slopes=3), L.CPG_E_INVALID, 'cpg_conv2d_fwd_prelu_eval')


def test_null_and_malformed_descriptor():
    """make_geom's verdict comes before everything else, in all three."""
    lib = L.lib()
    assert lib.cpg_conv2d_fwd_bn_eval(None, ONE, ONE, None, 0.0, None, ONE, ONE, ONE, ONE, 1e-5, 1, ONE, None, ONE, BYTES, None) == L.CPG_E_INVALID
    assert lib.cpg_conv2d_fwd_bn_eval_add(None, ONE, ONE, None, 0.0, None, ONE, ONE, ONE, ONE, 1e-5, ONE, 1, ONE, ONE, BYTES, None) == L.CPG_E_INVALID
    assert lib.cpg_conv2d_fwd_prelu_eval(None, ONE, ONE, None, 0.0, None, ONE, 1, None, ONE, None, ONE, BYTES, None) == L.CPG_E_INVALID
    bad = _desc()
    bad.groups = 3                   # divides neither C nor K
    for rc in (_bn_eval(bad), _bn_eval_add(bad), _prelu_eval(bad), _prelu_eval(bad, x=None)):
        assert rc == L.CPG_E_INVALID and b'groups' in lib.cpg_last_error()
