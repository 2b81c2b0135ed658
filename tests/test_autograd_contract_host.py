"""The reference of tests/test_autograd_contract_gpu.py, checked on the CPU: every hard-coded seed gives the float64 reference a
conditioning margin of at least 2e-5 (no ReLU / PReLU input and no max-pool runner-up within fp32 round-off of a kink), the situation
driver obeys plain autograd identities on the reference (so a mismatch on the GPU is the library's), the bound never falls below the
1e-5 floor nor rises above the topology's S0, and the envelope of the fused BatchNorm statistics' two-sums formula is on record."""
import numpy as np
import pytest
import torch

import _autograd_ref as R

CASES = [(t, s) for t in R.TOPOLOGIES for s in R.SITUATIONS]


def _ref(topo, sit, seed=None):
    return R.reference(topo, sit, R.seed_of(topo, sit) if seed is None else seed)


def _close(a, b, tol=1e-11):
    if a is None or b is None:
        return a is None and b is None
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('topo,sit', CASES)
def test_every_hard_coded_seed_has_the_margin(topo, sit):
    r64, r32, margin, count = _ref(topo, sit)
    print('%s %s seed %d: margin %.3g over %d activations / windows' % (topo, sit, R.seed_of(topo, sit), margin, count))
    assert count > 1000 and margin >= R.MARGIN
    # ... and stock fp32 stayed on the same side of every kink: its error is round-off, not a flipped mask
    for n, b in R.bounds(topo, sit, R.seed_of(topo, sit)).items():
        assert R.B_FLOOR <= b <= 1e-4, (n, b)


@pytest.mark.parametrize('topo', R.TOPOLOGIES)
def test_reference_situations_obey_autograd_identities(topo):
    """All situations from ONE seed (float64: the identities hold to round-off wherever the margin is, and they are exact statements
    about autograd, not about conditioning)."""
    seed = R.seed_of(topo, 'S0a')
    r = {s: R.reference(topo, s, seed)[0] for s in R.SITUATIONS}
    s0a, s0b = r['S0a'], r['S0b']
    pnames = [n[5:] for n in s0a if n.startswith('grad:') and n != 'grad:x']
    probe = R.build_reference(topo, seed)
    norm = {'%s.%s' % (mn, pn) for mn, m in probe.named_modules() if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.PReLU))
            for pn, _ in m.named_parameters()}
    matrices = {n for n, p in probe.named_parameters() if n.endswith('weight') and p.dim() >= 2}
    assert norm and matrices and not norm & matrices
    frozen = lambda n, what: what == 'all' or (what == 'weights' and n in matrices) or (what == 'norm' and n in norm)
    # S0: an input gradient exists exactly when it was asked for, and asking changes nothing else
    assert s0a['grad:x'] is None and s0b['grad:x'] is not None
    for n in s0a:
        if n != 'grad:x':
            assert _close(s0a[n], s0b[n]), n
    # a piggymask's gradients: gW = g_eff * bin, gPM = g_eff * w  =>  gW * w == gPM * bin, gW == 0 where the mask is off
    net = R.build_reference(topo, seed).double()
    mods = dict(net.named_modules())
    for name in net.masked:
        m = mods[name]
        b = (m.piggymask > R.THR).double()
        assert 0.2 < float(b.mean()) < 0.8
        gw, gpm = s0a['grad:%s.weight' % name], s0a['grad:%s.piggymask' % name]
        assert _close(gw * m.weight.detach(), gpm * b) and float((gw * (1 - b)).abs().max()) == 0.0 and float((gpm * (1 - b)).abs().max()) > 0
    # S1 / S2 / S3: frozen parameters end without a gradient, every other gradient is S0's
    for sit, what in (('S1', 'weights'), ('S2', 'norm'), ('S3', 'all')):
        nfrozen = 0
        for n in pnames:
            if frozen(n, what):
                assert r[sit]['grad:' + n] is None, (sit, n)
                nfrozen += 1
            else:
                assert _close(r[sit]['grad:' + n], s0b['grad:' + n]), (sit, n)
        assert nfrozen > 0 and (what == 'all' or nfrozen < len(pnames))
        assert _close(r[sit]['out'], s0a['out'])
    assert _close(r['S3']['grad:x'], s0b['grad:x'])
    # S4: each subset by backward(inputs=...) and by autograd.grad; nothing outside the subset
    for k, names in enumerate(R._new(topo, False).subsets()):
        for n in pnames:
            got = r['S4']['%d:grad:%s' % (k, n)]
            if n in names:
                assert _close(got, s0a['grad:' + n]) and _close(r['S4']['%d:ag:grad:%s' % (k, n)], s0a['grad:' + n]), (k, n)
            else:
                assert got is None, (k, n)
        assert r['S4']['%d:grad:x' % k] is None
    # S5: twice the gradient; S6 = S7: the sum of the two micro-batches' gradients, statistics updated twice
    for n in pnames + ['x']:
        if s0a['grad:' + n] is not None or n != 'x':
            want = s0b['grad:' + n] if n == 'x' and r['S5']['grad:x'] is not None else s0a['grad:' + n]
            assert _close(r['S5']['grad:' + n], None if want is None else 2 * want), n
    for n in r['S6']:
        assert _close(r['S6'][n].double() if r['S6'][n] is not None else None, r['S7'][n].double() if r['S7'][n] is not None else None), n
    data = R.make_data(topo, seed)
    swapped = dict(data, x1=data['x2'], t1=data['t2'])
    other = R.run(R.build_reference(topo, seed).double(), 'S0a', swapped, 'cpu', torch.float64)
    for n in pnames:
        assert _close(r['S6']['grad:' + n], s0a['grad:' + n] + other['grad:' + n]), n
    for n in s0a:
        if n.endswith('num_batches_tracked'):
            assert int(s0a[n]) == 1 and int(r['S6'][n]) == int(r['S7'][n]) == int(r['S9'][n]) == 2 and int(r['S8'][n]) == 0 and int(r['S4'][n]) == 3
    # S8: eval mode leaves the buffers alone, and its gradients are another function's (running statistics, not the batch's)
    for n in r['S8']:
        if n.startswith('before:'):
            assert torch.equal(r['S8'][n], r['S8'][n[7:]]), n
    assert _close(r['S8']['out'], s0a['out'], 1e-3) == (topo == 'C')        # (C has no BatchNorm: eval mode changes nothing there)
    # S9: the no_grad forward is S0's forward; the step after it has S0's gradients and twice-updated statistics
    assert _close(r['S9']['dry:out'], s0a['out'])
    for n in s0a:
        if n.startswith('buf:'):
            assert _close(r['S9']['dry:' + n].double(), s0a[n].double()), n
        elif n != 'grad:x' or not R.make_data(topo, seed)['x_grad']:
            assert _close(r['S9'][n], s0a[n]), n
    # S10: only every second pixel of the big tensor is read
    gx = r['S10']['grad:x']
    if gx is not None:
        assert float(gx[:, :, 1::2].abs().max()) == 0.0 and float(gx[:, :, :, 1::2].abs().max()) == 0.0 and float(gx[:, :, ::2, ::2].abs().min()) > 0
    else:
        assert topo == 'A'


def test_compare_reports_misses_and_passes_the_fp32_reference():
    """compare() itself: stock fp32 is within its own bound; a gradient off by 1e-4 of its scale, a missing gradient, a gradient
    that should not exist and a counter that is off by one are all reported."""
    topo, sit = 'B_basic', 'S1'
    seed = R.seed_of(topo, sit)
    r64, r32, _, _ = R.reference(topo, sit, seed)
    quiet = lambda *a: None
    assert R.compare(dict(r32), topo, sit, seed, log=quiet) == []
    frozen = [n for n in r64 if r64[n] is None and n != 'grad:x'][0]
    live = [n for n in r64 if n.startswith('grad:') and r64[n] is not None][0]
    for name, value in ((live, r32[live] * (1 + 1e-4)), (live, None), (frozen, torch.zeros(1)),
                        ('buf:block.bn1.num_batches_tracked', r32['buf:block.bn1.num_batches_tracked'] + 1),
                        ('buf:block.bn1.running_var', r32['buf:block.bn1.running_var'] * (1 + 1e-4))):
        bad = R.compare(dict(r32, **{name: value}), topo, sit, seed, log=quiet)
        assert [n for n, _ in bad] == [name], (name, bad)


@pytest.mark.parametrize('kind', sorted(R.OFFCENTRE))
def test_offcentre_reference_spans_the_ratios(kind):
    c = R.offcentre(kind)
    ratio = c['r64']['ratio']
    print('%s: |mean| / std from %.3g to %.3g, margin %.3g, centre-tap offsets %.3g .. %.3g'
          % (kind, float(ratio.min()), float(ratio.max()), c['r64']['margin'], float(c['delta'].min()), float(c['delta'].max())))
    assert float(ratio.min()) <= 0.1 and 6.0 <= float(ratio.max()) <= 10.0
    assert float(c['delta'].min()) >= 0.0 and int((c['delta'] > 0).sum()) >= c['delta'].numel() // 2
    assert c['r64']['margin'] >= R.MARGIN
    # stock fp32 (a two-pass variance) holds the statistics bound with room to spare: the bound is about the formula, not about fp32
    assert float(((c['r32']['mean'].double() - c['r64']['mean']).abs() / c['r64']['std']).max()) <= 1e-5
    assert float((c['r32']['invstd'].double() / c['r64']['invstd'] - 1).abs().max()) <= 1e-5


def test_two_sums_formula_envelope():
    """E[y^2] - mean^2 from float32 sums of one 448-element tile, strictly sequential accumulation, float64 merge -- the fused
    statistics' formula in its least favourable order: the relative invstd error stays inside the project's 1e-4 up to |mean| / std = 10
    (the worst of 32 draws) and is outside it at 30 (the typical draw)."""
    err = {ratio: [R.two_sums_invstd_error(ratio, seed=s) for s in range(32)] for ratio in (0, 1, 3, 8, 10, 30)}
    for ratio in sorted(err):
        print('ratio %d: invstd error median %.3g, max %.3g' % (ratio, float(np.median(err[ratio])), max(err[ratio])))
    for ratio in (0, 1, 3, 8, 10):
        assert max(err[ratio]) <= R.STAT_BOUND, ratio
    assert max(err[3]) <= 1e-5
    assert float(np.median(err[30])) > R.STAT_BOUND
