"""SphereNet's inference epilogue (cpg_conv2d_fwd_prelu_eval: conv -> + bias -> PReLU [-> + residual] in one kernel, the PRE instances of
k_wg1 / k_wg2 / k_wg3 and k_c3_fwd) against code that exists without it.

Reference: cpg_conv2d_fwd_bn_eval with the identity BatchNorm (gamma 1, beta 0, mean 0, var 1, eps 0, relu off) on the same inputs and
option table -- conv + bias from the SAME inference plan --, then torch.where(v > 0, v, a * v) (+ res) in fp32 torch.  The fused result
must be bit-equal as numbers (torch.equal: -0 equals +0): the product is rounded, then selected, then the sum is rounded.  No tolerance
is involved.

Every shape is the smallest that reaches its kernel's edges (the tables of tests/test_eval_conv_gpu.py and tests/test_eval_blocks_gpu.py);
every case runs six weight patterns x {K slopes, one shared slope} x {no residual, residual where the query takes one}, and checks
skip on == CPG_NO_DEAD_SKIP=1 bit for bit and skip_stats == those of the identity-BatchNorm call.
Network level: a width-0.25 spherenet20 and the PackNet spherenet20 in eval mode under no_grad, fused_bn.FUSE_EVAL_PRELU on against off:
launch counts by entry point, logits and embeddings within the project's 1e-4 bar; under grad mode nothing changes."""
import collections
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import _evalconv as E                          # noqa: F401  (the helper modules of the tests these shapes come from)
import _evalres as R                           # noqa: F401
from oracle import ops

pytestmark = pytest.mark.gpu

from cpg_amd import _lib                         # noqa: E402
from cpg_amd.models import fused_bn              # noqa: E402
from cpg_amd.models import layers as nl          # noqa: E402

# tables, runners and the body of test_prelu_eval_is_bit_equal: shared with tests/test_guard_bands_gpu.py
import _prelu_eval_cases as PE                   # noqa: E402
from _prelu_eval_cases import (CASES, DEV, SENTINEL, THR, _desc, _dev, _inputs, _out, _ptr, _set, _ws, expect, make_slopes,    # noqa: E402
                               run_ident, run_prelu)


@pytest.mark.parametrize('cid', list(CASES))
def test_prelu_eval_is_bit_equal(cid, libopt):
    PE.prelu_eval_case(cid, libopt)


@pytest.mark.parametrize('cid,other', [('wg1', 'wg1'), ('wg1', 'wg1-grown78'), ('M128', 'M128'), ('M128', 'S16'), ('wg3odd-7x7', 'wg3')])
def test_workspace_reuse_rezeroes_liveness(cid, other, libopt):
    """A sparse layer, then a dense one, then the sparse one again, all in one workspace: the liveness words are re-zeroed by every call,
    so skip_stats and the outputs equal those of fresh calls."""
    L = _lib.lib()
    ds, sparse, sl_s, _, res_s = _inputs(cid, 'neg-zero')
    dd, dense, sl_d, _, res_d = _inputs(other, 'dense')
    nb = max(int(L.cpg_conv2d_workspace_bytes(ctypes.byref(ds))), int(L.cpg_conv2d_workspace_bytes(ctypes.byref(dd))))
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=DEV)

    def call(d, a, slope, res, shared):
        rc, y, st = run_prelu(d, *a, slope, res, ws if shared else None)
        assert rc == 0, L.cpg_last_error()
        return y, st
    fresh_s, fresh_d = call(ds, sparse, sl_s, res_s, False), call(dd, dense, sl_d, res_d, False)
    seq = [call(ds, sparse, sl_s, res_s, True), call(dd, dense, sl_d, res_d, True), call(ds, sparse, sl_s, res_s, True)]
    for (y, st), (fy, fst) in zip(seq, [fresh_s, fresh_d, fresh_s]):
        assert st == fst, (cid, other, st, fst)
        assert torch.equal(y, fy), (cid, other)
    if cid == other:                            # (stale flags of the dense layer would show in the sparse one's statistics)
        assert fresh_s[1][0] < fresh_d[1][0], (fresh_s[1], fresh_d[1])


def test_refusals(libopt):
    """Pointwise and grouped descriptors: 0 / CPG_E_UNSUPPORTED; n_slopes = 2 and a NULL slope: CPG_E_INVALID; the channel-split 14 x 14
    tile: refused by the query and the call.  y keeps its sentinel every time."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(11)
    N, C, H, W, K = 2, 32, 14, 14, 64
    x = _dev(torch.randn(N, C, H, W, generator=g))
    slope = _dev(make_slopes(K, g))
    for k, groups in ((1, 1), (3, 2)):
        d = _desc((N, C, H, W, K), 1, k, groups)
        w = _dev(torch.randn(K, C // groups, k, k, generator=g))
        for with_res in (0, 1):
            assert L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), with_res) == 0, (k, groups)
        rc, y, st = run_prelu(d, x, w, None, None, slope, None, ws=torch.empty(1 << 18, device=DEV))
        assert rc == -2 and bool((y == SENTINEL).all()) and st == [-7, -7], (k, groups, rc)
    d = _desc((N, C, H, W, K), 1)
    w = _dev(torch.randn(K, C, 3, 3, generator=g))
    assert L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 1) == 1
    rc, y, st = run_prelu(d, x, w, None, None, slope, None, n_slopes=2)
    assert rc == _lib.CPG_E_INVALID and bool((y == SENTINEL).all()) and st == [-7, -7], rc
    y = _out(d)
    ws, nbytes = _ws(d, None)
    rc = L.cpg_conv2d_fwd_prelu_eval(ctypes.byref(d), _ptr(x), _ptr(w), None, THR, None, None, K, None, _ptr(y), None, _ptr(ws), nbytes,
                                     _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.CPG_E_INVALID and bool((y == SENTINEL).all()), rc
    # CPG_C3_FORCE=8 with CPG_NO_WINO picks the 14 x 14 channel-split tile, which has no fused epilogue
    libopt.set('CPG_NO_WINO', 1)
    libopt.set('CPG_C3_FORCE', 8)
    shape = (2, 128, 14, 14, 256)
    d = _desc(shape, 1)
    assert L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 0) == 0 and L.cpg_conv2d_fwd_prelu_eval_supported(ctypes.byref(d), 1) == 0
    x = _dev(torch.randn(2, 128, 14, 14, generator=g))
    w = _dev(torch.randn(256, 128, 3, 3, generator=g))
    rc, y, st = run_prelu(d, x, w, None, None, _dev(make_slopes(256, g)))
    assert rc == -2 and bool((y == SENTINEL).all()) and st == [-7, -7], rc


@pytest.mark.parametrize('cid', ['wg1', 'wg3odd-7x7', 'S16', 'S2G64'])
def test_unfused_prelu_pass_is_the_same_expression(cid, libopt):
    """cpg_prelu_fwd on the reference conv output is bit-equal to the torch expression: sharing the formula with the conv epilogues did
    not change k_prelu_fwd (7 x 7 and 9 x 11 planes take its scalar path, the others its float4 path)."""
    _set(libopt, CASES[cid][2])
    d, (x, w, pm, b), slopes, shared, res = _inputs(cid, 'bias')
    v, _ = run_ident(d, x, w, pm, b)
    N, K, OH, OW = v.shape
    for slope in (slopes, shared):
        for r in (None, res):
            y = torch.full_like(v, SENTINEL)
            _lib.call('cpg_prelu_fwd', _ptr(v), _ptr(r), _ptr(slope), _ptr(y), N, K, OH * OW, slope.numel(), _lib.stream_ptr())
            torch.cuda.synchronize()
            assert torch.equal(y, expect(v, slope, r)), (cid, slope.numel(), r is not None)


# ---------------------------------------------------------------------------------------------------------------- network level
N_CONVS = 20        # conv -> PReLU pairs of SphereNet-20
N_FUSED = 19        # descriptors the query supports: all but conv1_1 (3 input channels: the strided stem's class has no such epilogue)
N_RESIDUAL = 8      # residual units (1 + 2 + 4 + 1): their second pair carries the residual
# (so with the switch on a forward launches N_FUSED fused convs and, for the N_CONVS - N_FUSED = 1 pair the query refuses, cpg_conv2d_fwd
#  AND the cpg_prelu_fwd behind it: the PReLU launches drop from 20 to 20 - n, to 0 only where n = 20)
NAMES = ('cpg_conv2d_fwd_prelu_eval', 'cpg_conv2d_fwd', 'cpg_prelu_fwd')


def _mask_and_randomise(net, g, masked):
    """apply_mask at task 2 of a random 4-owner assignment on every trunk conv, random PReLU slopes of both signs, non-zero conv biases."""
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d) or isinstance(m, nl.SharableConv2d)]
    assert len(convs) == N_CONVS
    with torch.no_grad():
        for m in convs:
            owner = torch.randint(0, 4, m.weight.shape, generator=g).numpy().astype(np.uint8)
            m.weight.copy_(torch.from_numpy(ops.apply_mask(m.weight.detach().numpy(), owner, 2)))
            m.bias.normal_(0, 0.1, generator=g)
            if masked:
                m.piggymask = nn.Parameter(torch.where(torch.rand(m.weight.shape, generator=g) < 0.9, 0.01, 0.001))
        for m in net.modules():
            if isinstance(m, nn.PReLU):
                m.weight.normal_(0.1, 0.3, generator=g)
    return net.to(DEV).eval()


def _counted(fn, switch, monkeypatch):
    """(result, Counter of the C entry points launched through _lib.call, residual-carrying fused calls) of fn() with FUSE_EVAL_PRELU = switch."""
    counts = collections.Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        if name == 'cpg_conv2d_fwd_prelu_eval' and args[8] is not None:
            counts['with_residual'] += 1
        return real(name, *args)
    monkeypatch.setattr(fused_bn, 'FUSE_EVAL_PRELU', switch)
    monkeypatch.setattr(_lib, 'call', counting)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_lib, 'call', real)
    return out, counts


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())


def _logits(net, x):
    """|x| cos(theta) of the angular head (its second output, |x| phi(theta), steps where floor(m theta / pi) does)."""
    out = net(x)
    return out[0] if isinstance(out, tuple) else out


def _check_on_off(net, x, monkeypatch):
    def infer():
        with torch.no_grad():
            return _logits(net, x), net.forward_to_embeddings(x)
    (lon, eon), c_on = _counted(infer, True, monkeypatch)
    (loff, eoff), c_off = _counted(infer, False, monkeypatch)
    # off: launch for launch what it was -- per forward 20 convs and a PReLU pass behind each (two forwards here), nothing fused
    assert [c_off[n] for n in NAMES] == [0, 2 * N_CONVS, 2 * N_CONVS], c_off
    # on: 19 fused convs, 8 of them with the unit's residual; conv1_1 and its PReLU pass as before
    assert [c_on[n] for n in NAMES] == [2 * N_FUSED, 2 * (N_CONVS - N_FUSED), 2 * (N_CONVS - N_FUSED)], c_on
    assert c_on['with_residual'] == 2 * N_RESIDUAL, c_on
    assert set(c_on) - {'cpg_conv2d_fwd_prelu_eval', 'with_residual'} <= set(c_off), (c_on, c_off)
    for on, off in ((lon, loff), (eon, eoff)):
        assert bool(torch.isfinite(on).all()) and on.shape == off.shape
        assert _close(on, off), (float((on - off).abs().max()), float(off.abs().max()))

    # grad mode: nothing changes -- the parent's launches, and a train step that is bit-identical with the switch on and off
    def step():
        net.train()
        net.zero_grad(set_to_none=True)
        out = _logits(net, x)
        out.square().mean().backward()
        grads = [p.grad.detach().clone() for p in net.parameters() if p.grad is not None]
        net.eval()
        return out.detach(), grads
    (o1, g1), t_on = _counted(step, True, monkeypatch)
    (o0, g0), t_off = _counted(step, False, monkeypatch)
    assert t_on == t_off and t_on['cpg_conv2d_fwd_prelu_eval'] == 0 and t_on['cpg_prelu_fwd'] == N_CONVS, (t_on, t_off)
    assert torch.equal(o1, o0) and len(g1) == len(g0) and len(g1) >= 2 * N_CONVS
    for a, b in zip(g1, g0):
        assert torch.equal(a, b)


def test_spherenet20_quarter_width_on_vs_off(monkeypatch):
    from cpg_amd import models as M
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(5)
    net = M.spherenet20(dataset_history=[], dataset2num_classes={}, network_width_multiplier=0.25, shared_layer_info={})
    net.add_dataset('face_verification', 9)
    net.set_dataset('face_verification')
    net = _mask_and_randomise(net, g, True)
    _check_on_off(net, torch.randn(2, 3, 112, 112, generator=g).to(DEV), monkeypatch)


def test_packnet_spherenet20_on_vs_off(monkeypatch):
    import cpg_amd.packnet_models as pm
    torch.manual_seed(6)
    g = torch.Generator().manual_seed(6)
    net = pm.factory('spherenet20')(dataset_history=[], dataset2num_classes={})
    net.add_dataset('face_verification', 9)
    net.set_dataset('face_verification')
    net = _mask_and_randomise(net, g, False)
    _check_on_off(net, torch.randn(2, 3, 112, 112, generator=g).to(DEV), monkeypatch)
