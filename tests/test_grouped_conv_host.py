"""Host-side contract of groups > 1 in the C ABI (no GPU needed: every call here returns before anything is launched)."""
import ctypes
import os
import re

from conftest import ROOT

import cpg_amd._lib as L


def _desc(N=4, C=32, H=14, W=14, K=64, k=3, s=1, p=1, G=4):
    d = L.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, k, k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = p
    d.dil_h = d.dil_w = 1
    d.groups = G
    return d


def test_grouped_null_pointers_are_invalid_not_unsupported():
    """Descriptor first, then null pointers: a valid groups = 4 descriptor with null tensors is CPG_E_INVALID."""
    lib = L.lib()
    d = _desc()
    assert lib.cpg_conv2d_fwd(ctypes.byref(d), None, None, None, 0.0, None, None, None, 0, None) == L.CPG_E_INVALID
    assert b'null pointer' in lib.cpg_last_error()
    assert lib.cpg_conv2d_dgrad(ctypes.byref(d), None, None, None, 0.0, None, None, 0, None) == L.CPG_E_INVALID
    assert lib.cpg_conv2d_wgrad(ctypes.byref(d), None, None, None, None, 0.0, None, None, None, None, 0, None) == L.CPG_E_INVALID
    # ... and a descriptor whose groups do not divide the channels is invalid whatever the pointers are
    for bad in (_desc(C=30), _desc(K=62), _desc(G=0), _desc(G=-2)):
        assert lib.cpg_conv2d_fwd(ctypes.byref(bad), None, None, None, 0.0, None, None, None, 0, None) == L.CPG_E_INVALID
        assert lib.cpg_conv2d_workspace_bytes(ctypes.byref(bad)) == 0


def test_grouped_workspace_and_queries():
    """The workspace holds at least the bias gradient's partial sums (>= one float per output channel) and the split weight-gradient
    partials (>= one copy of the [K][C/G][R][S] gradient); no packed operand, no fused statistics, no fused epilogues."""
    lib = L.lib()
    for d in (_desc(), _desc(C=32, K=32, G=32), _desc(N=6, C=96, K=160, G=2, H=12, W=20)):
        nbytes = lib.cpg_conv2d_workspace_bytes(ctypes.byref(d))
        assert nbytes >= d.K * 4
        assert nbytes >= d.K * (d.C // d.groups) * d.R * d.S * 4
        for which in (0, 1, 2):
            assert lib.cpg_conv2d_pack_bytes(ctypes.byref(d), which) == 0
        assert lib.cpg_conv2d_bnstats_tiles(ctypes.byref(d)) == 0
        assert lib.cpg_conv2d_dgrad_add_supported(ctypes.byref(d)) == 0
        assert lib.cpg_conv2d_fwd_bn_eval_supported(ctypes.byref(d)) == 0
        assert lib.cpg_conv2d_wgrad_rider_supported(ctypes.byref(d)) == 0
        assert lib.cpg_conv2d_dgrad_bnbwd_tiles(ctypes.byref(d)) == 0
        for which in (0, 1, 2, 3):
            assert lib.cpg_conv2d_winograd(ctypes.byref(d), which) == 0
        # the fused-statistics forward stays unsupported for groups > 1 (CPG_E_UNSUPPORTED), before any pointer is looked at
        assert lib.cpg_conv2d_fwd_bnstats(ctypes.byref(d), None, None, None, 0.0, None, None, None, 0, None, 0, None) == -2


def test_cpg_no_grouped_switch():
    """CPG_NO_GROUPED round-trips through cpg_set_option / cpg_get_option, turns grouped descriptors back into 'unsupported', and has
    its row in INTEGRATION.md's switch table."""
    lib = L.lib()
    d = _desc()
    assert L.get_option('CPG_NO_GROUPED') in (None, 0)
    with L.option('CPG_NO_GROUPED', 1):
        assert L.get_option('CPG_NO_GROUPED') == 1
        assert lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)) == 0
        assert lib.cpg_conv2d_fwd(ctypes.byref(d), None, None, None, 0.0, None, None, None, 0, None) == -2        # CPG_E_UNSUPPORTED
        one = _desc(G=1)
        assert lib.cpg_conv2d_workspace_bytes(ctypes.byref(one)) > 0           # groups == 1 is not the switch's business
        with L.option('CPG_NO_GROUPED', 0):
            assert L.get_option('CPG_NO_GROUPED') == 0 and lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)) > 0
    assert L.get_option('CPG_NO_GROUPED') in (None, 0)
    assert lib.cpg_conv2d_workspace_bytes(ctypes.byref(d)) > 0
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert re.search(r'^\| `CPG_NO_GROUPED=1` \|', text, re.M)
