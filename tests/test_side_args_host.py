"""The four "arm the calling thread, then make the call" channels of the C ABI (cpg_conv2d_use_packed, cpg_conv2d_fwd_attach_pool_max,
cpg_conv2d_wgrad_attach_bn_bwd, cpg_bn_relu_pool_attach_max): WHICH entry point takes an armed value, that it is gone afterwards whatever
the status, and that no other entry point touches it.  Every call here is one the code refuses before it launches anything: non-null
pointers that nothing reads, NULL tensors in each follow-up call so that it stops at a pointer or buffer check.  Needs the built
library and no GPU.

These tests pin the behaviour the library had while the values lived in four thread-local contexts read deep in the launch code; they
pass on that library unchanged.  The one exception is test_thread_state_has_one_home, which describes the source after the values
became arguments below the ABI boundary."""
import ctypes
import os
import re

import pytest

import cpg_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, WORKSPACE = -2, -3
ONE = ctypes.c_void_p(16)           # a non-null, 16-byte aligned pointer nothing reads
BYTES = 1 << 20


def _desc(N, C, H, W, K, k=3):
    d = L.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, k, k
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.groups = 1
    d.pad_h = d.pad_w = k // 2
    return d


def _text():
    return L.lib().cpg_last_error().decode()


@pytest.fixture(autouse=True)
def _disarmed():
    """every test starts and ends with nothing armed on this thread"""
    def disarm():
        lib = L.lib()
        assert lib.cpg_conv2d_use_packed(None, 0) == L.CPG_OK
        assert lib.cpg_conv2d_fwd_attach_pool_max(None, 0) == L.CPG_OK
        assert lib.cpg_conv2d_wgrad_attach_bn_bwd(None, None, None, None, 0, 0, 0) == L.CPG_OK
        assert lib.cpg_bn_relu_pool_attach_max(None, 0) == L.CPG_OK
    disarm()
    yield
    disarm()


def _wgrad(d):
    return L.lib().cpg_conv2d_wgrad(ctypes.byref(d), None, None, None, None, 0.0, None, None, None, ONE, BYTES, None)


def _fwd_bnstats(d):
    return L.lib().cpg_conv2d_fwd_bnstats(ctypes.byref(d), None, None, None, 0.0, None, None, None, 0, ONE, BYTES, None)


def _fwd(d):
    return L.lib().cpg_conv2d_fwd(ctypes.byref(d), None, None, None, 0.0, None, None, ONE, BYTES, None)


def test_rider_is_taken_by_the_weight_gradient_that_refuses_it():
    lib = L.lib()
    d = _desc(2, 16, 8, 8, 32)                  # a valid descriptor, no Winograd weight gradient: no rider
    assert lib.cpg_conv2d_wgrad_rider_supported(ctypes.byref(d)) == 0
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(ONE, ONE, ONE, ONE, 2, 32, 196) == L.CPG_OK
    assert _wgrad(d) == UNSUPPORTED and 'BatchNorm backward is attached' in _text()      # (judged before the null pointers)
    assert _wgrad(d) == L.CPG_E_INVALID and 'cpg_conv2d_wgrad: null pointer' in _text()   # the first call disarmed


def test_conv_maxima_are_taken_by_fwd_bnstats_whatever_its_status():
    lib = L.lib()
    d = _desc(2, 64, 4, 4, 64)
    assert lib.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(d)) == 1
    assert lib.cpg_conv2d_fwd_attach_pool_max(ONE, 4) == L.CPG_OK
    assert _fwd_bnstats(d) == L.CPG_E_INVALID and 'window-maxima buffer 4 <' in _text()
    assert _fwd_bnstats(d) == WORKSPACE and 'statistics buffer' in _text()


def test_conv_maxima_survive_another_entry_point():
    lib = L.lib()
    d = _desc(2, 64, 4, 4, 64)
    assert lib.cpg_conv2d_fwd_attach_pool_max(ONE, 4) == L.CPG_OK
    assert _fwd(d) == L.CPG_E_INVALID and 'cpg_conv2d_fwd: null pointer' in _text()
    assert _wgrad(d) == L.CPG_E_INVALID and 'cpg_conv2d_wgrad: null pointer' in _text()
    assert _fwd_bnstats(d) == L.CPG_E_INVALID and 'window-maxima buffer 4 <' in _text()  # still armed: only this entry point takes them
    assert _fwd_bnstats(d) == WORKSPACE


def test_a_refused_attach_leaves_the_channel_disarmed():
    lib = L.lib()
    d = _desc(2, 64, 4, 4, 64)
    assert lib.cpg_conv2d_fwd_attach_pool_max(ONE, 4) == L.CPG_OK
    assert lib.cpg_conv2d_fwd_attach_pool_max(ONE, 0) == L.CPG_E_INVALID       # an empty buffer: refused, and the earlier arm is gone
    assert _fwd_bnstats(d) == WORKSPACE
    assert lib.cpg_bn_relu_pool_attach_max(ONE, 4) == L.CPG_OK
    assert lib.cpg_bn_relu_pool_attach_max(ctypes.c_void_p(18), 4) == L.CPG_E_INVALID    # misaligned
    assert _pool_fwd(1, 1, 2, 2) == L.CPG_E_INVALID and 'cpg_bn_relu_pool_fwd: null pointer' in _text()
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(ONE, ONE, ONE, ONE, 2, 32, 196) == L.CPG_OK
    assert lib.cpg_conv2d_wgrad_attach_bn_bwd(ONE, ONE, ONE, ONE, 2, 32, 198) == L.CPG_E_INVALID
    assert _wgrad(_desc(2, 16, 8, 8, 32)) == L.CPG_E_INVALID and 'null pointer' in _text()


def _pool_fwd(N, C, H, W):
    return L.lib().cpg_bn_relu_pool_fwd(None, None, None, 1e-5, 0.1, None, None, None, None, None, N, C, H, W, 0, None, 0, None)


def _pool_bwd(N, C, H, W):
    return L.lib().cpg_bn_relu_pool_bwd(None, None, None, None, None, None, None, None, None, N, C, H, W, 1, None, 0, None)


def _pool_fwd_from_max(N, C, H, W):
    return L.lib().cpg_bn_relu_pool_fwd_from_max(None, ONE, None, 0, None, None, 1e-5, 0.1, None, None, None, None, None, None, N, C, H, W, None)


def _pool_bwd_from_max(N, C, H, W):
    return L.lib().cpg_bn_relu_pool_bwd_from_max(None, ONE, None, None, None, None, None, None, None, None, N, C, H, W, 1, None, 0, None)


# (N, C, H, W), bytes armed.  1 x 1 x 2 x 2 has ONE window, so "one float short" of it would be an empty buffer, which the attach itself
# refuses (test_a_refused_attach_leaves_the_channel_disarmed): there the armed buffer is the largest short one, 3 bytes; the two-window
# plane is armed exactly one float short.
SHORT = [((1, 1, 2, 2), 3), ((1, 1, 2, 4), 4)]


@pytest.mark.parametrize('entry,name', [(_pool_fwd, 'cpg_bn_relu_pool_fwd'), (_pool_bwd, 'cpg_bn_relu_pool_bwd')])
@pytest.mark.parametrize('shape,armed', SHORT)
def test_pooled_pair_maxima_are_taken_first_and_by_that_pair_only(entry, name, shape, armed):
    lib = L.lib()
    assert armed < shape[0] * shape[1] * (shape[2] // 2) * (shape[3] // 2) * 4
    assert lib.cpg_bn_relu_pool_attach_max(ONE, armed) == L.CPG_OK
    # the _from_max pair takes its maxima as an argument and never looks at the armed ones
    assert _pool_fwd_from_max(*shape) == L.CPG_E_INVALID and 'cpg_bn_relu_pool_fwd_from_max: null pointer' in _text()
    assert _pool_bwd_from_max(*shape) == L.CPG_E_INVALID and 'cpg_bn_relu_pool_bwd_from_max: null pointer' in _text()
    assert entry(*shape) == L.CPG_E_INVALID and (name + ': the window maxima attached') in _text() and "not this tensor's" in _text()
    assert entry(*shape) == L.CPG_E_INVALID and (name + ': null pointer') in _text()          # disarmed by the refused call


@pytest.mark.parametrize('entry', [_pool_fwd, _pool_bwd])
def test_pooled_pair_maxima_are_taken_before_the_dimensions_are_judged(entry):
    lib = L.lib()
    assert lib.cpg_bn_relu_pool_attach_max(ONE, 4) == L.CPG_OK
    assert entry(0, 1, 2, 2) == L.CPG_E_INVALID and "not this tensor's" in _text()      # not "non-positive dimension": the take came first
    assert entry(0, 1, 2, 2) == L.CPG_E_INVALID and 'non-positive dimension' in _text()
    assert lib.cpg_bn_relu_pool_attach_max(ONE, 4) == L.CPG_OK
    assert entry(1, 1, 3, 2) == L.CPG_E_INVALID and 'must be even' in _text()      # one window: the buffer is long enough; H is odd
    assert entry(1, 1, 2, 2) == L.CPG_E_INVALID and 'null pointer' in _text()      # ... and that call had disarmed


def test_thread_state_has_one_home():
    """NEW with the refactor (the one test of this file that cannot pass on the library it was written against): the armed values live
    in cpg_common.cpp, nowhere else is there thread-local state, and the accessors, take-in-place helpers and scope guards that read it
    deep in the launch code are gone."""
    csrc = os.path.join(ROOT, 'cpg_amd', 'csrc')
    files = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc))] + [os.path.join(ROOT, 'tools', 'csrc', 'wino_wgrad_template.hip')]
    gone = re.compile(r'\b(pack_ctx|pool_max_ctx|bn_pool_max_ctx|take_packed|PackScope|PoolMaxScope|RiderScope)\b')
    for path in files:
        text = open(path).read()
        if os.path.basename(path) != 'cpg_common.cpp':
            assert 'thread_local' not in text, path
        assert gone.search(text) is None, (path, gone.search(text).group(0))
    assert 'thread_local' in open(os.path.join(csrc, 'cpg_common.cpp')).read()
