"""The inference conv kernels (cpg_conv2d_fwd_bn_eval: conv3x3 s1 p1 -> BatchNorm2d(eval) [-> ReLU] in one kernel, with the
dead-channel skip) against the fp64 reference of tests/_evalconv.py.

Manager.validate runs every eval-mode conv -> BatchNorm2d -> ReLU group through these kernels: the Winograd BNE instances of
k_wg1 / k_wg2 / k_wg3 (and k_wg3's ODD instance) and k_c3_fwd with the C3BnEval epilogue in every tile config.  Every family
runs eight weight patterns, from dense to entirely dead, and each case checks
  * every element against the reference's elementwise bound, dead output channels against relu?(BN(bias)) within the
    epilogue's own rounding;
  * skip on == skip off (CPG_NO_DEAD_SKIP=1) bit for bit: a skipped chunk or block only ever drops exact zeros;
  * skip_stats: {4 * (chunks up to the last live input chunk), number of skipped blocks > 0 exactly when a whole block of output
    channels is dead}; {0, 0} with the skip off.
The ratios of the measured errors to the contraction term of the bound are collected per kernel family; CPG_EVALCONV_RATIOS=<path>
writes them as JSON (tests/_evalconv.py's GAMMA constants are set from them)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _evalconv as E
from oracle import ops

pytestmark = pytest.mark.gpu

from cpg_amd import _lib                        # noqa: E402
from cpg_amd.models import layers as nl          # noqa: E402
from cpg_amd.models.fused_bn import FusedSequential   # noqa: E402

# tables, runners and the body of test_eval_conv_matches_fp64: shared with tests/test_guard_bands_gpu.py
import _eval_conv_cases as EC                    # noqa: E402
from _eval_conv_cases import (CASES, CASE_BY_ID, DEV, RATIOS, _desc, _dev, _family, _inputs, _set, _split, _ws_bytes,    # noqa: E402
                               reference, run_eval)


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    if not RATIOS:
        return
    summary = {k: {'max': max(v.values()), 'cases': v} for k, v in sorted(RATIOS.items())}
    print('\neval-conv error ratios (|y - ref| - shift term) / (U32 |s| (|x| * |w_eff|)):')
    for k, v in summary.items():
        print('  %-6s max %.3f  %s' % (k, v['max'], ' '.join('%s=%.2f' % kv for kv in sorted(v['cases'].items()))))
    path = os.environ.get('CPG_EVALCONV_RATIOS')
    if path:
        with open(path, 'w') as f:
            json.dump(summary, f, indent=1, sort_keys=True)


@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_eval_conv_matches_fp64(cid, libopt):
    EC.eval_conv_case(cid, libopt)


@pytest.mark.parametrize('cid,other', [('wg1', 'wg1'), ('wg1', 'wg1-grown78'), ('M128', 'M128'), ('M128', 'S16'),
                                       ('wg3odd-7x7', 'wg3')])
def test_workspace_reuse_rezeroes_liveness(cid, other, libopt):
    """A sparse layer, then a dense one, then the sparse one again, all in one workspace: the liveness words are re-zeroed by
    every call, so skip_stats and the outputs equal those of fresh calls."""
    shape, oshape = CASE_BY_ID[cid][3], CASE_BY_ID[other][3]
    ws = torch.empty((max(_ws_bytes(shape), _ws_bytes(oshape)) + 3) // 4, dtype=torch.float32, device=DEV)
    sparse = [_dev(t) if not isinstance(t, tuple) else tuple(_dev(u) for u in t) for t in _inputs(shape, 'grown-split')]
    dense = [_dev(t) if not isinstance(t, tuple) else tuple(_dev(u) for u in t) for t in _inputs(oshape, 'dense')]

    def call(a, shared):
        x, w, pm, b, bn = a
        rc, y, st = run_eval(x, w, pm, b, bn, 1, ws if shared else None)
        assert rc == 0
        return y, st
    fresh_s, fresh_d = call(sparse, False), call(dense, False)
    seq = [call(sparse, True), call(dense, True), call(sparse, True)]
    for (y, st), (fy, fst) in zip(seq, [fresh_s, fresh_d, fresh_s]):
        assert st == fst, (cid, other, st, fst)
        assert torch.equal(y, fy), (cid, other)
    if shape == oshape:                         # (stale flags of the dense layer would show in the sparse one's statistics)
        assert fresh_s[1][0] < fresh_d[1][0], (fresh_s, fresh_d)


@pytest.mark.parametrize('cid', ['wg1', 'wg2', 'wg3-grown313', 'wg3odd-grown627', 'M128', 'S16', 'nowino-D64'])
def test_nonfinite_inputs_in_skipped_work_do_not_propagate(cid, libopt):
    """The one deliberate difference from the reference (include/cpg_hip.h): a NaN or Inf in an input channel past the last live
    chunk, or feeding an output block with no live weight, does not reach the output -- that work is skipped.  With
    CPG_NO_DEAD_SKIP=1 it does (0 * Inf = NaN), as in the reference."""
    _, kernel, B, shape, opts = CASE_BY_ID[cid]
    N, C, H, W, K = shape
    _set(libopt, opts)
    x, w, pm, b, bn = _inputs(shape, 'grown-split')
    m0, c0 = _split(K), _split(C)
    skipped_from = 4 * (-(-c0 // 4))            # first channel of the first skipped chunk
    dead_from = -(-m0 // B) * B                 # first output channel of the first dead block
    assert skipped_from < C and dead_from < K, cid
    xn = x.clone()
    xn[0, skipped_from, H // 2, W // 2] = float('inf')
    xn[N - 1, C - 1, 0, W - 1] = float('nan')
    bnd = tuple(_dev(t) for t in bn)
    fam = _family(kernel)
    ref0, conv_term, shift_term = reference(shape, 'grown-split', x, w, pm, b, bn, fam)   # (those channels' weights are all zero)
    for relu in (0, 1):
        rc, y, st = run_eval(_dev(xn), _dev(w), _dev(pm), _dev(b), bnd, relu)
        assert rc == 0
        ref = ref0.clamp_min(0.0) if relu else ref0
        assert bool(torch.isfinite(y).all()), (cid, relu)
        assert bool(((y.double() - ref).abs() <= E.GAMMA[fam] * conv_term + shift_term).all()), (cid, relu)
    libopt.set('CPG_NO_DEAD_SKIP', 1)
    for relu in (0, 1):                         # (the epilogue's ReLU keeps a NaN, as torch.relu does)
        rc, y_full, _ = run_eval(_dev(xn), _dev(w), _dev(pm), _dev(b), bnd, relu)
        assert rc == 0 and bool(torch.isnan(y_full).any()), (cid, relu)
    libopt.set('CPG_NO_DEAD_SKIP', None)
    # a NaN in a LIVE chunk reaches the live channels either way, but never the dead blocks while the skip is on
    xl = x.clone()
    xl[0, 0, H // 2, W // 2] = float('nan')
    rc, y_l, _ = run_eval(_dev(xl), _dev(w), _dev(pm), _dev(b), bnd, 0)
    assert rc == 0
    assert bool(torch.isnan(y_l[:, :m0]).any()), cid
    assert bool(((y_l[:, dead_from:].double() - ref0[:, dead_from:]).abs() <= shift_term[:, dead_from:]).all()), cid


def test_channel_split_tile_is_refused(libopt):
    """CPG_C3_FORCE=8 picks the 14 x 14 channel-split tile, which has no BatchNorm epilogue: refused, nothing written."""
    libopt.set('CPG_NO_WINO', 1)
    libopt.set('CPG_C3_FORCE', 8)
    shape = (2, 128, 14, 14, 256)
    x, w, pm, b, bn = _inputs(shape, 'dense')
    rc, y, st = run_eval(_dev(x), _dev(w), _dev(pm), _dev(b), tuple(_dev(t) for t in bn), 1)
    assert rc == -2, rc                        # CPG_E_UNSUPPORTED
    assert st == [-7, -7] and bool(torch.isnan(y).all())


VGG_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']


def test_vgg_features_match_fp64_layer_by_layer():
    """A width-0.25 VGG feature stack in eval mode with a two-task owner pattern inside a grown split (task 1 owns a corner of every
    layer, apply_mask at task 1): fuse_eval=True against the fp64 reference applied to each conv group's own input, and the
    winning feature against fuse_eval=False."""
    from cpg_amd.models.vgg import _conv_stack
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(11)
    mods = _conv_stack(VGG_CFG, 0.25, True, 1)
    for m in mods:
        if isinstance(m, nl.SharableConv2d):
            K, C = m.weight.shape[:2]
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            owner = torch.randint(1, 3, (K, C, 3, 3), generator=g)                       # tasks 1 and 2 inside the corner
            owner[torch.rand(K, C, 3, 3, generator=g) < 0.1] = 0                         # ... and some free slots
            owner[_split(K // 2):] = 2                                                    # the grown part: task 2's
            if C > 3:
                owner[:, _split(C // 2):] = 2
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(ops.apply_mask(m.weight.detach().numpy(), owner.numpy().astype(np.uint8), 1)))
                m.piggymask = nn.Parameter(torch.where(torch.rand(K, C, 3, 3, generator=g) < 0.95, 0.01, 0.001))
        elif isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5, generator=g)
                m.bias.uniform_(-0.2, 0.3, generator=g)
                m.running_mean.normal_(0, 0.2, generator=g)
                m.running_var.uniform_(0.5, 2.0, generator=g)
    seq = FusedSequential(*mods).to(DEV).eval()
    x = torch.randn(6, 3, 32, 32, generator=g).to(DEV)
    # groups: conv, BN, ReLU (+ MaxPool2d) -- the same fusion decisions as in the whole stack
    groups, i = [], 0
    while i < len(mods):
        j = i + 3 + (1 if i + 3 < len(mods) and isinstance(mods[i + 3], nn.MaxPool2d) else 0)
        groups.append(list(range(i, j)))
        i = j
    FusedSequential.skip_log = []
    try:
        with torch.no_grad():
            seq.fuse_eval = True
            whole = seq(x)
            h = x
            for grp in groups:
                sub = FusedSequential(*[mods[k] for k in grp]).eval()
                out = sub(h)
                conv, bn = mods[grp[0]], mods[grp[1]]
                # (a group with a pool runs the plain forward and the fused BatchNorm -> ReLU -> pool kernel)
                d = _desc(*h.shape, conv.out_channels)
                fam = 'winograd' if _lib.lib().cpg_conv2d_winograd(ctypes.byref(d), 0 if len(grp) == 4 else 3) else 'direct'
                ref, ct, sh = E.eval_conv_terms(h, conv.weight, conv.piggymask, None, bn.weight, bn.bias, bn.running_mean,
                                                bn.running_var, eps=bn.eps, relu=True, threshold=conv.info['threshold'], family=fam)
                bound = E.GAMMA[fam] * ct + sh
                if len(grp) == 4:                # max pooling is 1-Lipschitz in the max norm: pool the bound with the values
                    ref = torch.nn.functional.max_pool2d(ref, 2, 2)
                    bound = torch.nn.functional.max_pool2d(bound, 2, 2)
                err = (out.cpu().double() - ref).abs()
                assert bool((err <= bound).all()), (grp, float(err.max()))
                h = out
            seq.fuse_eval = False
            unfused = seq(x)
            seq.fuse_eval = True
        log = [t.cpu().tolist() for t in FusedSequential.skip_log]
    finally:
        FusedSequential.skip_log = None
    assert torch.equal(whole, h)
    assert log and any(s > 0 for _, s in log), log          # the fused inference convs ran and skipped dead blocks
    a, b = whole.flatten(1), unfused.flatten(1)
    assert torch.equal(a.argmax(1), b.argmax(1))
    assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
