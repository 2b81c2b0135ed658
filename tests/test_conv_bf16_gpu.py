"""The bf16 and bf16x3 convolution kernels (csrc/conv3x3_bf16.hip) held to what the fp32 kernels are held to: a per-element a-priori
bound against a float64 model of their own arithmetic and the sharper r_gpu <= M r_emulation (tests/_bf16_cases.py has the table, the
oracle and the body), repeatability, misplaced pointers, guard bands round every output and both workspaces, NaN containment, the
non-finite behaviour include/cpg_hip.h states, and the autograd situations S0 .. S10 of tests/_autograd_ref.py under bf16x3."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _autograd_ref as R
import _bf16_cases as B
import _conv_space_cases as CS
import _guarded
import _parity_cases as PC

from cpg_amd import _lib
from cpg_amd.models import layers as nl

pytestmark = pytest.mark.gpu
DEV = PC.DEV
ROW_IDS = list(B.ROWS)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# --------------------------------------------------------------------------- the body
@pytest.mark.parametrize('variant', B.VARIANTS)
@pytest.mark.parametrize('math', B.MATHS)
@pytest.mark.parametrize('row', ROW_IDS)
def test_bf16_rows_against_the_model(row, math, variant):
    B.body(row, variant, math)


def test_worst_a_priori_ratio_per_configuration():
    """Every row once more (plain variant, the C entry points), then the worst ratio each of the 10 + 6 configurations reached and
    the largest r_gpu / r_emulation, of everything this process ran so far."""
    for row in B.ROWS:
        for math in B.MATHS:
            B.check(row, 'plain', math, B.run_abi(row, 'plain', math), 'abi', log=lambda s: None)
    assert set(B.WORST) == set(B.FWD_CFG) | set(B.WG_CFG)
    for cfg in list(B.FWD_CFG) + list(B.WG_CFG):
        print('configuration %-8s worst a-priori ratio %.3e (%s)' % ((cfg,) + B.WORST[cfg]))
    key = max(B.QS, key=B.QS.get)
    print('largest r_gpu / r_emulation: Q = %.3f at %s; M = %d' % (B.QS[key], key, B.M))
    assert 4 * B.QS[key] <= B.M <= B.M_CAP


# --------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize('math', B.MATHS)
@pytest.mark.parametrize('row', ROW_IDS)
def test_a_second_run_is_bit_equal(row, math):
    """Split-K is reduced in a fixed order and these kernels use no atomics."""
    layer = B.make_layer(row, 'plain', math)
    for first, second in ((B.run_layer(row, 'plain', math, layer=layer), B.run_layer(row, 'plain', math, layer=layer)),
                          (B.run_abi(row, 'bias+pm', math), B.run_abi(row, 'bias+pm', math))):
        assert set(first) == set(second)
        for name in first:
            assert _bits(first[name], second[name]), (row, math, name)


# --------------------------------------------------------------------------- misplaced pointers
@pytest.mark.parametrize('math', B.MATHS)
@pytest.mark.parametrize('row', ROW_IDS)
def test_misplaced_pointers_give_the_same_bits(row, math):
    """This family has no alignment predicate: inputs and parameters 1 and 3 floats off 16-byte alignment (through the layer with a bias
    and a piggymask, through the layer without -- there the weight gradient is the bf16 kernel's --, and the entry points directly,
    x, gy, w, pm and bias all moved), every output 1 and 3 floats off (the entry points directly) -- the float64 checks of the body,
    and the bits of the aligned run."""
    variant = 'bias+pm'
    layer = B.make_layer(row, variant, math)
    aligned = B.run_layer(row, variant, math, layer=layer)
    aligned_abi = B.run_abi(row, variant, math)
    aligned_plain = B.run_layer(row, 'plain', math)
    for place in CS.PLACEMENTS:
        got = B.run_layer(row, variant, math, buf=CS.placed(place))
        B.check(row, variant, math, got, 'layer')
        for name in ('y', 'gx'):                                # (gw, gpm, gb: the fp32 kernel, with a bias; its float64 check ran)
            assert _bits(got[name], aligned[name]), (row, math, place, name)
        got = B.run_layer(row, 'plain', math, buf=CS.placed(place))             # the weight gradient on k_c3b_wgrad, x / gy / w moved
        B.check(row, 'plain', math, got, 'layer')
        assert set(got) == {'y', 'gx', 'gw'}
        for name in got:
            assert _bits(got[name], aligned_plain[name]), (row, math, place, 'plain', name)
        got = B.run_abi(row, variant, math, buf=CS.placed(place))               # ... and with a piggymask: gw and gpm of the direct call
        B.check(row, variant, math, got, 'abi')
        assert set(got) == {'y', 'gx', 'gw', 'gpm'}
        for name in got:
            assert _bits(got[name], aligned_abi[name]), (row, math, place, 'abi', name)
    for off in (1, 3):
        got = B.run_abi(row, variant, math, off=off)
        B.check(row, variant, math, got, 'abi')
        for name in got:
            assert got[name].data_ptr() % 16 == 4 * off and _bits(got[name], aligned_abi[name]), (row, math, off, name)
    again = B.run_layer(row, variant, math, layer=layer)
    for name in aligned:
        assert _bits(again[name], aligned[name]), (row, math, name)


# --------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize('variant', B.VARIANTS)
@pytest.mark.parametrize('math', B.MATHS)
@pytest.mark.parametrize('row', ROW_IDS)
def test_bf16_rows_between_guard_bands(row, math, variant):
    """The body with every input frozen and every output and workspace between guards; the interposed workspace allocator hands out
    exactly the queried bytes, which holds k_c3b_pack and the split-K partials to the published sizes."""
    d = B.desc_of(row)
    nb = int(_lib.lib().cpg_conv2d_bf16_workspace_bytes(ctypes.byref(d)))
    nbw = int(_lib.lib().cpg_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d)))
    with _guarded.guarding() as led:
        outs = B.body(row, variant, math, _guarded.GuardedBuffers(DEV))
        led.verify()
        for i, t in enumerate(outs):
            assert led.holds(t), 'output %d of the body is not in guarded memory' % i
        labels = [a.label for a in led.arenas]
        asked = lambda n: sum(1 for s in labels if s.startswith('workspace(%d)' % n))          # noqa: E731
        # forward and input gradient ask for the pack workspace, the weight gradient (without a bias) for the split-K partials; the
        # backward's own request for the fp32 kernels' workspace is told apart by its size or, where that is the partials', counted
        fp = int(_lib.lib().cpg_conv2d_workspace_bytes(ctypes.byref(d)))
        assert nb not in (nbw, fp), (nb, nbw, fp)
        assert asked(nb) == 2 and asked(nbw) == (variant == 'plain') + (fp == nbw), (nb, nbw, fp, labels)
        assert led.workspaces >= (2 if variant == 'bias+pm' else 3)
        assert led.original_workspace_calls == 0 and led.passed_through == [], led.passed_through


# --------------------------------------------------------------------------- NaN containment
def _poisoned(row, math, what, value=float('nan')):
    """The layer's plain results and those with `value` in the last row and column of image N - 2 (the only image, when N = 1) of
    x or gy: (clean, got, the image, the channel)."""
    N, C, H, W, K = B.ROWS[row]
    x, w, b, pm, gy = B.inputs(row, 'plain')
    n0, c0 = max(N - 2, 0), 1
    xp, gyp = x.clone(), gy.clone()
    (xp if what == 'x' else gyp)[n0, c0, H - 1, W - 1] = value
    layer = B.make_layer(row, 'plain', math)
    clean = {k: v.cpu() for k, v in B.run_layer(row, 'plain', math, layer=layer).items()}
    got = {k: v.cpu() for k, v in B.run_layer(row, 'plain', math, layer=layer, x=xp, gy=gyp).items()}
    return clean, got, n0, c0


def _contained(name, got, clean, footprint, n0, bad=torch.isnan):
    rest = [n for n in range(got.shape[0]) if n != n0]
    assert _bits(got[rest], clean[rest]), '%s: another image changed' % name
    assert bool(torch.isfinite(clean).all()) and bool(footprint[n0].any()) and not bool(footprint[rest].any())
    assert bool(bad(got)[footprint].all()), '%s: a finite value inside the footprint' % name
    same = got.view(torch.int32) == clean.view(torch.int32)
    assert bool((footprint | same).all()), '%s: %d elements outside float64\'s footprint changed' % (name, int((~(footprint | same)).sum()))


@pytest.mark.parametrize('math', B.MATHS)
@pytest.mark.parametrize('row', ['a', 'c', 'h', 'j'])
def test_bf16_keeps_nan_inside_its_image(row, math):
    N, C, H, W, K = B.ROWS[row]
    x, w, b, pm, gy = B.inputs(row, 'plain')
    # NaN in x: forward and weight gradient
    clean, got, n0, c0 = _poisoned(row, math, 'x')
    xp = x.clone()
    xp[n0, c0, H - 1, W - 1] = float('nan')
    _contained('y', got['y'], clean['y'], torch.isnan(F.conv2d(xp.double(), w.double(), padding=1)), n0)
    assert _bits(got['gx'], clean['gx'])                                   # (the input gradient does not read x)
    fw = torch.isnan(B.wgrad_op(xp, gy, torch.float64))
    rest = [c for c in range(C) if c != c0]
    assert bool(fw[:, c0].any()) and not bool(fw[:, rest].any())
    assert bool(torch.isnan(got['gw'])[fw].all()), 'weight gradient: a finite value at a tap that reads the NaN'
    assert _bits(got['gw'][:, rest], clean['gw'][:, rest]), 'weight gradient: another input channel changed'
    sl = torch.isnan(got['gw'][:, c0]) | (got['gw'][:, c0].contiguous().view(torch.int32) == clean['gw'][:, c0].contiguous().view(torch.int32))
    assert bool(sl.all())
    # NaN in gy: input gradient and weight gradient
    clean, got, n0, k0 = _poisoned(row, math, 'gy')
    gyp = gy.clone()
    gyp[n0, k0, H - 1, W - 1] = float('nan')
    _contained('gx', got['gx'], clean['gx'], torch.isnan(F.conv_transpose2d(gyp.double(), w.double(), padding=1)), n0)
    assert _bits(got['y'], clean['y'])
    fw = torch.isnan(B.wgrad_op(x, gyp, torch.float64))
    rest = [k for k in range(K) if k != k0]
    assert bool(fw[k0].any()) and not bool(fw[rest].any())
    assert bool(torch.isnan(got['gw'])[fw].all())
    assert _bits(got['gw'][rest], clean['gw'][rest]), 'weight gradient: another output channel changed'


@pytest.mark.parametrize('math', B.MATHS)
def test_an_inf_operand_is_nan_under_bf16x3_and_inf_under_bf16(math):
    """include/cpg_hip.h: lo = Inf - Inf, so bf16x3 turns an Inf operand into NaN; plain bf16 keeps it an Inf."""
    x, w = B.inputs('c', 'plain')[:2]
    clean, got, n0, c0 = _poisoned('c', math, 'x', float('inf'))
    xp = x.clone()
    xp[n0, c0, -1, -1] = float('inf')
    foot = ~torch.isfinite(F.conv2d(xp.double(), w.double(), padding=1))
    _contained('y', got['y'], clean['y'], foot, n0, bad=torch.isnan if math == 'bf16x3' else torch.isinf)


@pytest.mark.parametrize('math', B.MATHS)
def test_a_finite_value_above_the_bf16_range_is_not_finite(math):
    """include/cpg_hip.h: both arithmetics round |v| above bf16's largest finite value (3.3895e38) to Inf."""
    x, w = B.inputs('c', 'plain')[:2]
    clean, got, n0, c0 = _poisoned('c', math, 'x', 3.4e38)
    xp = x.clone()
    xp[n0, c0, -1, -1] = float('inf')
    foot = ~torch.isfinite(F.conv2d(xp.double(), w.double(), padding=1))
    _contained('y', got['y'], clean['y'], foot, n0, bad=lambda t: ~torch.isfinite(t))


# --------------------------------------------------------------------------- the autograd situations under bf16x3
class Probe(object):
    """Which entry points ran in which phase of the situation driver, with the descriptor of those that take one first, and the
    weight-gradient rider's calls."""

    def __init__(self):
        self.phase, self.calls, self.riders = 'setup', [], []

    def __enter__(self):
        self.real_call, self.real_rider = _lib.call, nl._bn_bwd_rider

        def call(name, *args):
            d = getattr(args[0], '_obj', None) if args else None
            self.calls.append((self.phase, name, isinstance(d, _lib.ConvDesc) and B.eligible_desc(d)))
            return self.real_call(name, *args)

        def rider(*args, **kw):
            self.riders.append(self.phase)
            return self.real_rider(*args, **kw)
        _lib.call, nl._bn_bwd_rider = call, rider
        return self

    def __exit__(self, *exc):
        _lib.call, nl._bn_bwd_rider = self.real_call, self.real_rider
        return False

    def mark(self, label):
        self.phase = label

    def per_phase(self, pred):
        out = {}
        for phase, name, elig in self.calls:
            if pred(name, elig):
                out[phase] = out.get(phase, 0) + 1
        return out


X3_CASES = [(t, s) for t in B.x3_topologies() for s in R.SITUATIONS]


def test_the_topologies_with_an_eligible_convolution():
    assert B.x3_topologies() == ('A', 'B_identity', 'B_basic', 'C')         # (B_down's only 3x3 convolution has stride 2)


@pytest.mark.parametrize('topo,sit', X3_CASES)
def test_situation_under_bf16x3(topo, sit):
    seed = R.seed_of(topo, sit)
    data = R.make_data(topo, seed)

    def once(math):
        nl.set_conv_math(math)
        net = R.build_library(topo, R.build_reference(topo, seed), DEV)
        with Probe() as probe:
            got = R.run(net, sit, data, DEV, torch.float32, mark=probe.mark)
            torch.cuda.synchronize()
        return got, probe
    try:
        before, p32 = once('fp32')
        got, p3 = once('bf16x3')
        after, _ = once('fp32')
    finally:
        nl.set_conv_math('fp32')
    bad = B.x3_compare(got, topo, sit, seed)
    # the *_bf16x3 entry points in the phases where fp32 shows cpg_conv2d_fwd*, cpg_conv2d_dgrad* and cpg_conv2d_wgrad on the same layers
    biased = topo == 'C'                   # (its eligible convolutions carry a bias: their weight gradient stays on the fp32 kernel)
    for kind in ('fwd', 'dgrad', 'wgrad'):
        fp32 = p32.per_phase(lambda n, e: e and '_bf16' not in n and (n.startswith('cpg_conv2d_' + kind) if kind != 'wgrad' else n == 'cpg_conv2d_wgrad'))
        x3 = p3.per_phase(lambda n, e: n == 'cpg_conv2d_%s_bf16x3' % kind or (kind == 'wgrad' and biased and e and n == 'cpg_conv2d_wgrad'))
        print('%s %s %s per phase: fp32 %s, bf16x3 %s' % (topo, sit, kind, fp32, x3))
        assert fp32 == x3 and (fp32 or kind == 'wgrad'), (kind, fp32, x3)
        if kind == 'wgrad' and biased:
            assert not p3.per_phase(lambda n, e: n == 'cpg_conv2d_wgrad_bf16x3')
    stray = p3.per_phase(lambda n, e: (e and '_bf16x3' not in n and not (biased and n == 'cpg_conv2d_wgrad')) or n.endswith('_bf16')
                         or n in ('cpg_conv2d_dgrad_bnbwd', 'cpg_conv2d_wgrad_attach_bn_bwd'))
    assert not stray and p3.riders == [], (stray, p3.riders)
    # no hand-off, packed operand or hint survived the bf16x3 pass: fp32 afterwards is fp32 before, bit for bit
    assert set(after) == set(before)
    for n in before:
        assert (before[n] is None and after[n] is None) or torch.equal(before[n], after[n]), n
    assert not bad, bad
