"""The opt-in bf16 / bf16x3 arithmetics of the 3x3 s1 p1 convolution (csrc/conv3x3_bf16.hip): a table of the smallest shapes that put every
tile configuration on its ragged edges, a float64 oracle of the kernels' own stated arithmetic, an a-priori per-element bound, and ONE
body that tests/test_conv_bf16_gpu.py runs plainly, on misplaced pointers and between guard bands.  tests/test_conv_bf16_host.py checks
the table against the selection predicates of run() and wpick() (restated below) and the oracle against itself, without a GPU.

The model.  hi = bf16(v) (round to nearest even), lo = bf16(v - hi) (the subtraction is exact in fp32).
    bf16     conv(a_hi, b_hi)
    bf16x3   conv(a_hi, b_hi) + conv(a_hi, b_lo) + conv(a_lo, b_hi)
in float64, for the forward (a = x, b = W * bin(pm)), the input gradient (a = gy) and the weight gradient (a = x, b = gy; then the
autograd epilogue gW = g * bin(pm), gPM = g * W).  Products of two bf16 are exact in fp32, so all that separates a kernel from the
model is the fp32 accumulation of T products (T = L for bf16, 3 L for bf16x3; L = 9 C forward, 9 K input gradient, N H W weight
gradient) and one more fp32 operation on the result (the bias add, the g * W product):

    |got - model| <= T * U * mag + U * |result|        mag: the same contraction over absolute values; U = 2^-23

U is a whole ulp, not the half ulp of round-to-nearest: the matrix unit's adder is not documented to round to nearest.  That bound is a
hard condition, and far too loose to be the only one: a kernel that drops a_lo * b_hi on one column stays inside it.  So, per tensor,

    r = max |got - model| / (T * U * mag)   over the elements with mag > 0

is taken for the GPU result and for a CPU emulation (F.conv2d in fp32 on the split operands, summed in fp32), and r_gpu <= M * r_emulation
is asserted.  M is set as GAMMA_DIRECT of tests/_evalconv.py is: the smallest power of two that is at least four times the largest
r_gpu / r_emulation measured on the MI355X over every row, variant, math, tensor and way in (the layer, the C entry points); it may not exceed 64
(the host test shows three mutants -- a dropped a_lo * b_hi on the last column, truncation instead of rounding, a channel tail that is
not zero-filled -- at more than 64 times the emulation's r on every row).

    Measured on the MI355X: Q = 6.03, set by row f (2, 136, 7, 20, 20), plain, bf16x3, y (configuration X3N; the same figure through the layer
    and through cpg_conv2d_fwd_bf16x3), so M = 32.  The next figures: 4.95 (row c, bias + pm, bf16x3, gx), 4.86 (row d, bias + pm, bf16x3,
    y), 4.41 (row g, bias + pm, bf16x3, gx); plain bf16 stays below 3.4.  bf16x3 sits above 1 as a family: the emulation rounds each of the
    three convolutions at its own magnitude, the kernels add all 3 L products into one accumulator at the magnitude of the largest.
"""
import collections
import contextlib
import copy
import ctypes
import functools
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import _parity_cases as PC

THR = 5e-3
U = 2.0 ** -23
M_CAP = 64
Q_MEASURED, Q_ROW = 6.03, 'f'           # the largest r_gpu / r_emulation on the MI355X and the row that set it (docstring)
M = 32                                  # the smallest power of two >= 4 Q
BAR = {'bf16': 2e-2, 'bf16x3': 1e-4}    # the documented bars against float64 on the unrounded operands, of the tensor's scale
BF16_AT_LEAST = 1e-5                    # ... and plain bf16 is further than this from it: it really rounded its operands

MATHS = ('bf16', 'bf16x3')
VARIANTS = ('plain', 'bias+pm')
# row -> (N, C, H, W, K)
ROWS = collections.OrderedDict([
    ('a', (2, 24, 9, 56, 72)),       # W128 / X3W, W64 / X3W, G64: H tail; C tail in the last chunk; 2 tiles_m at BM = 64; 8 dead columns of a 64-wide unit
    ('b', (1, 72, 3, 112, 24)),      # W64 / X3W, W128 / X3W, G64: H below TH; two units per row, the second with 48 valid columns
    ('c', (2, 40, 13, 14, 80)),      # S16 / X3S, N64 / X3S, G16: H and W tails of the 14 x 16 tile
    ('d', (2, 80, 15, 16, 40)),      # N64 / X3S, N128 / X3S, G16: H = 15 just misses S16 and P28
    ('e', (1, 20, 14, 28, 136)),     # P28 / X3N1, N64 / X3N, G32: two tiles_m with a tail of 8; masked group at the right border
    ('f', (2, 136, 7, 20, 20)),      # N64 / X3N, P28 / X3N1, G32: three tiles_ci, tail of 8
    ('g', (1, 16, 10, 37, 65)),      # N128 / X3N1, N64 / X3N, G32: one chunk only (no prefetch); forward tile tail of 5 columns; straddling masked group
    ('h', (3, 65, 5, 60, 16)),       # N64 / X3N, N128 / X3N1, G32: W > 56 and W % 8 != 0; channel tail of 1
    ('i', (1, 32, 2, 72, 32)),       # N64 / X3N, N64 / X3N, G64: W % 8 == 0 and W % 56 != 0; unit height exactly TH
    ('j', (9, 16, 8, 8, 16)),        # N64 / X3S, N64 / X3S, G16: more splits than units, so empty splits write zero partials
])
# the claims of the table, as the host test holds them: row -> ((forward bf16, x3), (input gradient bf16, x3), weight gradient)
CLAIMS = {
    'a': (('B16W128', 'X3W'), ('B16W64', 'X3W'), 'G64'), 'b': (('B16W64', 'X3W'), ('B16W128', 'X3W'), 'G64'),
    'c': (('B16S16', 'X3S'), ('B16N64', 'X3S'), 'G16'), 'd': (('B16N64', 'X3S'), ('B16N128', 'X3S'), 'G16'),
    'e': (('B16P28', 'X3N1'), ('B16N64', 'X3N'), 'G32'), 'f': (('B16N64', 'X3N'), ('B16P28', 'X3N1'), 'G32'),
    'g': (('B16N128', 'X3N1'), ('B16N64', 'X3N'), 'G32'), 'h': (('B16N64', 'X3N'), ('B16N128', 'X3N1'), 'G32'),
    'i': (('B16N64', 'X3N'), ('B16N64', 'X3N'), 'G64'), 'j': (('B16N64', 'X3S'), ('B16N64', 'X3S'), 'G16'),
}

# --------------------------------------------------------------------------- run(), wpick() and the plans of conv3x3_bf16.hip, restated
Fwd = collections.namedtuple('Fwd', 'BM TH TW NP NSTAGE')
FWD_CFG = collections.OrderedDict([
    ('B16W128', Fwd(128, 8, 56, 1, 2)), ('B16W64', Fwd(64, 8, 56, 1, 2)), ('B16S16', Fwd(128, 14, 16, 1, 2)),
    ('B16P28', Fwd(128, 7, 32, 1, 2)), ('B16N128', Fwd(128, 8, 32, 1, 2)), ('B16N64', Fwd(64, 8, 32, 1, 2)),
    ('X3N1', Fwd(128, 8, 32, 2, 1)), ('X3W', Fwd(64, 8, 56, 2, 2)), ('X3S', Fwd(64, 8, 16, 2, 2)), ('X3N', Fwd(64, 8, 32, 2, 2))])
Wg = collections.namedtuple('Wg', 'TH TW MASKW NP')
WG_CFG = collections.OrderedDict([
    ('B16G64', Wg(2, 64, False, 1)), ('B16G32', Wg(4, 32, True, 1)), ('B16G16', Wg(8, 16, True, 1)),
    ('X3G64', Wg(1, 64, False, 2)), ('X3G32', Wg(2, 32, True, 2)), ('X3G16', Wg(4, 16, True, 2))])
K_CUS, K_XCDS = 256, 8                  # csrc/cpg_common.h


def fwd_config(math, m, H, W):
    """run(): m = channels produced (K forward, C for the input gradient)."""
    if math == 'bf16x3':
        if m > 64 and W % 56 != 0 and W > 16:
            return 'X3N1'
        if W % 56 == 0:
            return 'X3W'
        return 'X3S' if W <= 16 else 'X3N'
    if W % 56 == 0:
        return 'B16W128' if m > 64 else 'B16W64'
    if m > 64 and W <= 16 and H <= 14:
        return 'B16S16'
    if m > 64 and W <= 32 and H % 7 == 0:
        return 'B16P28'
    return 'B16N128' if m > 64 else 'B16N64'


def wgrad_config(math, W):
    """wpick()."""
    g = 'G64' if (W % 8 == 0 and W >= 56) else 'G32' if W > 16 else 'G16'
    return ('X3' if math == 'bf16x3' else 'B16') + g


def configs(row, math):
    """tensor -> the tile configuration that computes it."""
    N, C, H, W, K = ROWS[row]
    wg = wgrad_config(math, W)
    return {'y': fwd_config(math, K, H, W), 'gx': fwd_config(math, C, H, W), 'gw': wg, 'gpm': wg}


def _ceil(a, b):
    return -(-a // b)


def pack_bytes(c_read, m, planes=2):
    """packb_bytes(): the packed weights of one forward / input-gradient call."""
    return _ceil(c_read, 16) * planes * 18 * (_ceil(m, 128) * 128) * 16


def wplan(cfg, N, C, H, W, K):
    """wplan<Cfg>(): units, splits and the bytes of the split-K partials."""
    c = WG_CFG[cfg]
    tiles_x, tiles_y = _ceil(W, c.TW), _ceil(H, c.TH)
    units = N * tiles_x * tiles_y
    tiles = _ceil(K, 64) * _ceil(C, 64)
    want = min(max(min(_ceil(3 * K_CUS, tiles), units), 1), 4096)
    want = _ceil(want, K_XCDS) * K_XCDS
    return {'tiles_x': tiles_x, 'tiles_y': tiles_y, 'units': units, 'nsplit': want, 'units_per_split': _ceil(units, want),
            'ws_bytes': want * K * C * 9 * 4}


def desc_of(row, **over):
    from cpg_amd import _lib
    N, C, H, W, K = ROWS[row]
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = N, C, H, W, K, 3, 3
    d.stride_h = d.stride_w = d.pad_h = d.pad_w = d.dil_h = d.dil_w = d.groups = 1
    for k, v in over.items():
        setattr(d, k, v)
    return d


# --------------------------------------------------------------------------- operands, the model, the bound, the emulation
def split(v):
    """(hi, lo) of a float32 CPU tensor, as pack2() / lo_part() make them."""
    assert v.dtype == torch.float32
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def truncated(v):
    """bf16 by chopping the low 16 bits (what a kernel without v_cvt_pk_bf16_f32's rounding would stage)."""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


def fwd_op(a, b, dt):
    return F.conv2d(a.to(dt), b.to(dt), padding=1)


def dgrad_op(a, b, dt):
    return F.conv_transpose2d(a.to(dt), b.to(dt), padding=1)


def wgrad_op(x, gy, dt):
    """g[k][c][r][s] = sum over n, h, w of gy[n][k][h][w] * x[n][c][h + r - 1][w + s - 1]."""
    return F.conv2d(x.to(dt).transpose(0, 1), gy.to(dt).transpose(0, 1), padding=1).transpose(0, 1).contiguous()


def terms(math, a, b):
    """The operand pairs the kernels multiply: a, b are (hi, lo)."""
    return [(a[0], b[0])] if math == 'bf16' else [(a[0], b[0]), (a[0], b[1]), (a[1], b[0])]


def contract(op, pairs, dt, drop_last_column_of=None):
    """Sum of op over the pairs, small terms first as the kernels do, in dt; drop_last_column_of: index of a pair that is left out on
    the last output column (a mutant)."""
    out = None
    for i in reversed(range(len(pairs))):
        t = op(pairs[i][0], pairs[i][1], dt)
        if i == drop_last_column_of:
            t = t.clone()
            t[..., -1] = 0
        out = t if out is None else out + t
    return out


def inputs(row, variant):
    """x, w, b, pm, gy as fp32 CPU tensors, drawn as tests/_parity_cases.py conv_oracle draws them."""
    N, C, H, W, K = ROWS[row]
    g = torch.Generator().manual_seed(zlib.crc32(('bf16 ' + row + variant).encode()) & 0x7FFFFFFF)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
    both = variant == 'bias+pm'
    b = torch.randn(K, generator=g) * 0.1 if both else None
    pm = torch.rand(K, C, 3, 3, generator=g) * 0.012 if both else None
    gy = torch.randn(N, K, H, W, generator=g)
    return x, w, b, pm, gy


Ref = collections.namedtuple('Ref', 'model mag T extra emu')      # each but T: tensor name -> float64 CPU tensor (emu: float32)


def arithmetic(math, x, w, b, pm, gy, dt=torch.float64, mutant=None):
    """{y, gx, gw[, gpm]} of the stated arithmetic, accumulated in dt.  mutant: None | 'drop' (a_lo * b_hi left out on the last column
    of every tensor; bf16x3) | 'trunc' (the activation operand -- x, gy for the input gradient -- chopped, not rounded; bf16)."""
    keep = None if pm is None else (pm > THR).float()
    weff = w if keep is None else w * keep
    sx, sg, sw = split(x), split(gy), split(weff)
    if mutant == 'trunc':
        sx, sg = (truncated(x), sx[1]), (truncated(gy), sg[1])
    drop = 2 if mutant == 'drop' else None
    out = {'y': contract(fwd_op, terms(math, sx, sw), dt, drop), 'gx': contract(dgrad_op, terms(math, sg, sw), dt, drop)}
    if b is not None:
        out['y'] = out['y'] + b.to(dt).view(1, -1, 1, 1)
    g = contract(wgrad_op, terms(math, sx, sg), dt, drop)
    out['gw'] = g if keep is None else g * keep.to(dt)
    if pm is not None:
        out['gpm'] = g * w.to(dt)
    return out


def magnitudes(math, x, w, b, pm, gy):
    keep = None if pm is None else (pm > THR).float()
    weff = w if keep is None else w * keep
    ab = lambda s: tuple(t.abs() for t in s)            # noqa: E731
    sx, sg, sw = ab(split(x)), ab(split(gy)), ab(split(weff))
    dt = torch.float64
    g = contract(wgrad_op, terms(math, sx, sg), dt)
    out = {'y': contract(fwd_op, terms(math, sx, sw), dt), 'gx': contract(dgrad_op, terms(math, sg, sw), dt),
           'gw': g if keep is None else g * keep.double()}
    if pm is not None:
        out['gpm'] = g * w.double().abs()
    return out


def tail_mutant(math, x, w, b, pm, gy):
    """{y, gx} of a kernel whose last 16-channel chunk is not zero-filled past the channel count, in fp32: chunk position C + j holds
    channel j of the NEXT image (the patch loader without its range check) and channel j of the same filter (the pack kernel without
    its own).  Only the tensors whose contraction has a tail (C % 16 for y, K % 16 for gx).  This is the DOUBLE failure: with finite
    data a kernel that misses only one of the two zero fills multiplies the stray values by zeros and is bit-correct, so no bound on
    finite data can see it.  The single failure on the activation side shows with a NaN in the next image's first channels, which
    tests/test_conv_bf16_gpu.py test_bf16_keeps_nan_inside_its_image has on row h (image 0's tail position 65 + 1 is image 1's channel
    1, the poisoned one: 'another image changed')."""
    N, C, H, W = x.shape
    K = w.shape[0]
    keep = None if pm is None else (pm > THR).float()
    weff = w if keep is None else w * keep
    out = {}
    tc, tk = -C % 16, -K % 16
    if tc:
        x2 = torch.cat([x, x.roll(-1, 0)[:, :tc]], 1)
        w2 = torch.cat([weff, weff[:, :tc]], 1)
        out['y'] = contract(fwd_op, terms(math, split(x2), split(w2)), torch.float32)
        if b is not None:
            out['y'] = out['y'] + b.view(1, -1, 1, 1)
    if tk:
        g2 = torch.cat([gy, gy.roll(-1, 0)[:, :tk]], 1)
        w2 = torch.cat([weff, weff[:tk]], 0)
        out['gx'] = contract(dgrad_op, terms(math, split(g2), split(w2)), torch.float32)
    return out


_REFS = {}


def reference(row, variant):
    """{'in': inputs, 'true': float64 results on the unrounded operands, math: Ref}, computed once and never modified."""
    key = (row, variant)
    if key in _REFS:
        return _REFS[key]
    N, C, H, W, K = ROWS[row]
    x, w, b, pm, gy = ins = inputs(row, variant)
    keep = None if pm is None else (pm > THR).double()
    weff = w.double() if keep is None else w.double() * keep
    g = wgrad_op(x, gy, torch.float64)
    true = {'y': F.conv2d(x.double(), weff, None if b is None else b.double(), padding=1),
            'gx': F.conv_transpose2d(gy.double(), weff, padding=1), 'gw': g if keep is None else g * keep}
    if pm is not None:
        true['gpm'] = g * w.double()
    if b is not None:
        true['gb'] = gy.double().sum((0, 2, 3))
    ref = {'in': ins, 'true': true}
    for math in MATHS:
        n = len(terms(math, (0, 0), (0, 0)))
        model = arithmetic(math, *ins)
        T = {'y': n * 9 * C, 'gx': n * 9 * K, 'gw': n * N * H * W, 'gpm': n * N * H * W}
        zero = lambda name: torch.zeros_like(model[name])            # noqa: E731
        extra = {'y': U * model['y'].abs() if b is not None else zero('y'), 'gx': zero('gx'), 'gw': zero('gw')}
        if pm is not None:
            extra['gpm'] = U * model['gpm'].abs()
        ref[math] = Ref(model, magnitudes(math, *ins), T, extra, arithmetic(math, *ins, dt=torch.float32))
    _REFS[key] = ref
    return ref


def ratios(got, ref, name):
    """(r, worst |got - model| / bound) of one tensor; r over the elements with mag > 0 (0.0 when there is none)."""
    err = (got.detach().cpu().double() - ref.model[name]).abs()
    tum = ref.T[name] * U * ref.mag[name]
    bound = tum + ref.extra[name]
    live = tum > 0
    r = float((err[live] / tum[live]).max()) if bool(live.any()) else 0.0
    over = err > bound
    hard = float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
    return r, (float('inf') if bool(over.any()) else hard)


# --------------------------------------------------------------------------- the body
ENTRY = {'bf16': ('cpg_conv2d_fwd_bf16', 'cpg_conv2d_dgrad_bf16', 'cpg_conv2d_wgrad_bf16'),
         'bf16x3': ('cpg_conv2d_fwd_bf16x3', 'cpg_conv2d_dgrad_bf16x3', 'cpg_conv2d_wgrad_bf16x3')}
CONV_ENTRIES = ('cpg_conv2d_fwd', 'cpg_conv2d_dgrad', 'cpg_conv2d_wgrad')
WORST = {}          # configuration -> (worst a-priori ratio seen, where)
QS = {}             # (row, variant, math, tensor, way in) -> r_gpu / r_emulation


@contextlib.contextmanager
def recording():
    """The entry points _lib.call makes, in order."""
    from cpg_amd import _lib
    names, real = [], _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = real


def make_layer(row, variant, math, buf=PC.PLAIN):
    from cpg_amd.models import layers as nl
    N, C, H, W, K = ROWS[row]
    x, w, b, pm, gy = inputs(row, variant)
    layer = nl.SharableConv2d(C, K, 3, padding=1, bias=b is not None).to(PC.DEV)
    layer.math = math
    layer.weight.data.copy_(w)
    if b is not None:
        layer.bias.data.copy_(b)
    if pm is not None:
        layer.piggymask = nn.Parameter(pm.to(PC.DEV))
    return buf.rehome(layer)


def run_layer(row, variant, math, buf=PC.PLAIN, layer=None, x=None, gy=None):
    """Forward and backward through SharableConv2d(math): {y, gx, gw[, gpm, gb]} on the device; the recorder's statement of which
    entry points ran (with a bias the weight gradient is cpg_conv2d_wgrad, the fp32 kernel)."""
    ins = inputs(row, variant)
    layer = layer or make_layer(row, variant, math, buf)
    layer.zero_grad(set_to_none=True)
    xd = buf.put(ins[0] if x is None else x).requires_grad_(True)
    with recording() as names:
        y = layer(xd)
        y.backward(buf.put(ins[4] if gy is None else gy))
    fwd, dgrad, wgrad = ENTRY[math]
    want = [fwd, dgrad, 'cpg_conv2d_wgrad' if ins[2] is not None else wgrad]
    assert [n for n in names if n.startswith(CONV_ENTRIES)] == want, (row, variant, math, names)
    got = {'y': y.detach(), 'gx': xd.grad, 'gw': layer.weight.grad}
    if layer.piggymask is not None:
        got['gpm'] = layer.piggymask.grad
    if layer.bias is not None:
        got['gb'] = layer.bias.grad
    return got


def misplaced(shape, off):
    """(whole, view): a NaN-filled buffer and a view of `shape` that starts `off` floats in, with four floats of NaN behind it."""
    n = int(np.prod(shape))
    whole = torch.full((n + off + 4,), float('nan'), device=PC.DEV)
    view = whole[off:off + n].view(shape)
    assert view.data_ptr() % 16 == (4 * off) % 16 and view.is_contiguous()
    return whole, view


def run_abi(row, variant, math, buf=PC.PLAIN, off=0):
    """The three entry points of `math` called directly, with workspaces of exactly the queried bytes and every output NaN on entry
    (off: so many floats into a buffer of its own).  The direct weight-gradient call takes no bias: it runs the bf16 kernel in both
    variants.  {y, gx, gw[, gpm]}; no element unwritten, nothing written round a misplaced output."""
    from cpg_amd import _lib
    x, w, b, pm, gy = inputs(row, variant)
    L, d, s, P = _lib.lib(), desc_of(row), _lib.stream_ptr(), _lib.dptr
    import _conv_space_cases as CS
    # (a placement moves activations and parameters by amounts of their own, as its rehome() does for a layer)
    par = (lambda t: PC.PlainBuffers.put(buf, t, buf.par)) if isinstance(buf, CS.PlacedBuffers) else buf.put
    xd, gyd, wd, bd, pd = buf.put(x), buf.put(gy), par(w), par(b), par(pm)
    if isinstance(buf, CS.PlacedBuffers):
        assert xd.data_ptr() % 16 == gyd.data_ptr() % 16 == 4 * buf.act and wd.data_ptr() % 16 == 4 * buf.par
    nb, nbw = int(L.cpg_conv2d_bf16_workspace_bytes(ctypes.byref(d))), int(L.cpg_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d)))
    assert nb > 0 and nbw > 0 and nb % 4 == 0 and nbw % 4 == 0
    ws, wsw = buf.empty((nb // 4,)), buf.empty((nbw // 4,))
    assert ws.data_ptr() % 16 == 0 and wsw.data_ptr() % 16 == 0
    made = {}

    def out(name, shape):
        made[name] = misplaced(shape, off) if off else (None, buf.full(shape, float('nan')))
        return made[name][1]
    fwd, dgrad, wgrad = ENTRY[math]
    _lib.call(fwd, ctypes.byref(d), P(xd), P(wd), P(pd), THR, P(bd), P(out('y', gy.shape)), P(ws), nb, s)
    _lib.call(dgrad, ctypes.byref(d), P(gyd), P(wd), P(pd), THR, P(out('gx', x.shape)), P(ws), nb, s)
    _lib.call(wgrad, ctypes.byref(d), P(xd), P(gyd), P(wd), P(pd), THR, P(out('gw', w.shape)),
              P(out('gpm', w.shape)) if pm is not None else None, P(wsw), nbw, s)
    torch.cuda.synchronize()
    got = {}
    for name, (whole, view) in made.items():
        if whole is not None:
            n = view.numel()
            assert bool(torch.isnan(whole[:off]).all()) and bool(torch.isnan(whole[off + n:]).all()), (row, math, off, name, 'written outside')
        assert not bool(torch.isnan(view).any()), (row, variant, math, off, name, 'an element was not written')
        got[name] = view
    return got


def rel(got, want):
    sc = float(want.abs().max())
    return float((got.detach().cpu().double() - want).abs().max()) / sc if sc else 0.0


def check(row, variant, math, got, via, log=print):
    """Every tensor of one run against the model (the hard bound, then r_gpu <= M r_emulation), against float64 on the unrounded
    operands (the documented bars) and, where the fp32 kernel ran (the layer's weight gradient with a bias), at its tolerances.
    Every figure is logged before anything is judged."""
    ref = reference(row, variant)
    m, true = ref[math], ref['true']
    fp32 = ('gw', 'gpm', 'gb') if via == 'layer' and 'gb' in true else ()
    assert set(got) == set(true) - ({'gb'} if via == 'abi' else set()), (sorted(got), sorted(true))
    cfgs = configs(row, math)
    figures = []
    for name in ('y', 'gx', 'gw', 'gpm'):
        if name not in got or name in fp32:
            continue
        assert got[name].shape == m.model[name].shape
        r_gpu, hard = ratios(got[name], m, name)
        r_emu, _ = ratios(m.emu[name], m, name)
        q = r_gpu / r_emu if r_emu else float('inf')
        e_true = rel(got[name], true[name])
        log('bf16 row %s %-7s %-6s %-5s %-3s [%s]: a-priori ratio %.3e (hard bound: %.3e of it), emulation %.3e, r_gpu / r_emulation %.3f; '
            '%.3e of scale from float64' % (row, variant, math, via, name, cfgs[name], r_gpu, hard, r_emu, q, e_true))
        if r_gpu > WORST.get(cfgs[name], (-1.0, None))[0]:
            WORST[cfgs[name]] = (r_gpu, '%s %s %s %s' % (row, variant, via, name))
        QS[(row, variant, math, name, via)] = q
        figures.append((name, r_gpu, hard, r_emu, q, e_true))
    for name, r_gpu, hard, r_emu, q, e_true in figures:
        where = (row, variant, math, via, name, cfgs[name])
        assert hard <= 1.0, where + ('outside the a-priori bound', hard)
        assert r_gpu <= M * r_emu, where + ('r_gpu %.3e > %d x emulation %.3e' % (r_gpu, M, r_emu),)
        assert e_true < BAR[math], where + (e_true,)
        if math == 'bf16':
            assert e_true > BF16_AT_LEAST, where + (e_true, 'not the bf16 arithmetic')
    if fp32:
        scale = max(float(true['gw'].abs().max()), 1.0)
        PC.close(got['gw'], true['gw'].numpy(), rtol=1e-4, atol=1e-5 * scale, msg='%s gw (fp32 kernel)' % row)
        PC.close(got['gpm'], true['gpm'].numpy(), rtol=1e-4, atol=1e-5 * scale, msg='%s gpm (fp32 kernel)' % row)
        PC.close(got['gb'], true['gb'].numpy(), rtol=1e-4, atol=1e-3, msg='%s gb' % row)


def body(row, variant, math, buf=PC.PLAIN):
    """One row in one variant and arithmetic, through the layer and through the C entry points; returns the tensors the kernels wrote."""
    a = run_layer(row, variant, math, buf)
    b = run_abi(row, variant, math, buf)
    check(row, variant, math, a, 'layer')
    check(row, variant, math, b, 'abi')
    for name in ('y', 'gx') + (() if 'gb' in a else ('gw',)):
        assert torch.equal(a[name], b[name]), (row, variant, math, name, 'the layer and the entry point disagree')
    return list(a.values()) + list(b.values())


# --------------------------------------------------------------------------- the autograd situations under bf16x3
def eligible(conv):
    """A conv module (library or reference) the bf16 entry points take: 3x3 / stride 1 / pad 1, >= 16 channels on both sides."""
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)            # noqa: E731
    return (pair(conv.kernel_size) == (3, 3) and pair(conv.stride) == (1, 1) and pair(conv.padding) == (1, 1) and pair(conv.dilation) == (1, 1)
            and conv.groups == 1 and conv.in_channels >= 16 and conv.out_channels >= 16)


def eligible_desc(d):
    return ((d.R, d.S, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w, d.groups) == (3, 3, 1, 1, 1, 1, 1, 1, 1)
            and d.C >= 16 and d.K >= 16)


def _split64(t):
    hi, lo = split(t.detach().float().contiguous())
    return hi.double(), lo.double()


class SplitConv3x3(torch.autograd.Function):
    """The three-term split model of a 3x3 s1 p1 convolution and of both its gradients, in float64 (operands first rounded to the
    fp32 the library holds them in)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        y = contract(fwd_op, terms('bf16x3', _split64(x), _split64(w)), torch.float64)
        return y if bias is None else y + bias.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        sx, sw, sg = _split64(x), _split64(w), _split64(gy)
        gx = contract(dgrad_op, terms('bf16x3', sg, sw), torch.float64) if ctx.needs_input_grad[0] else None
        gw = contract(wgrad_op, terms('bf16x3', sx, sg), torch.float64) if ctx.needs_input_grad[1] else None
        gb = gy.sum((0, 2, 3)) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return gx, gw, gb


@contextlib.contextmanager
def split_model_convs():
    """The reference nets of tests/_autograd_ref.py with every eligible convolution replaced by SplitConv3x3."""
    import _autograd_ref as R

    def conv_forward(self, x, w, b):
        if eligible(self) and x.dtype == torch.float64:
            return SplitConv3x3.apply(x, w, b)
        return nn.Conv2d._conv_forward(self, x, w, b)
    R.RefConv2d._conv_forward = conv_forward
    try:
        yield
    finally:
        del R.RefConv2d._conv_forward


def x3_topologies():
    import _autograd_ref as R
    return tuple(t for t in R.TOPOLOGIES if any(isinstance(m, R.RefConv2d) and eligible(m) for m in R._new(t, False).modules()))


@functools.lru_cache(maxsize=None)
def x3_bounds(topo, sit, seed):
    """{name: max(1e-4, 8 x E)}: E the relative error, on that tensor, of the float64 topology whose eligible convolutions compute the
    split model.  1e-4 is the project's bar for bf16x3, 8 x tests/_autograd_ref.py's margin over its stock reference."""
    import _autograd_ref as R
    r64 = R.reference(topo, sit, seed)[0]
    with split_model_convs():
        rs = R.run(copy.deepcopy(R.build_reference(topo, seed)).double(), sit, R.make_data(topo, seed), 'cpu', torch.float64)
    out = {}
    for n, want in r64.items():
        if want is None or not want.is_floating_point() or 'buf:' in n:
            continue
        sc = float(want.abs().max())
        e = float((rs[n] - want).abs().max()) / sc if sc else 0.0
        out[n] = max(BAR['bf16x3'], R.B_FACTOR * e)
    return out


def x3_compare(got, topo, sit, seed, log=print):
    """tests/_autograd_ref.py compare() with x3_bounds: which gradients exist, running statistics and counters held as there."""
    import _autograd_ref as R
    r64 = R.reference(topo, sit, seed)[0]
    bnd = x3_bounds(topo, sit, seed)
    bad = []
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    for n in sorted(r64):
        want, have = r64[n], got[n]
        if want is None or have is None:
            if (want is None) != (have is None):
                bad.append((n, 'None mismatch'))
            continue
        have = have.detach().cpu()
        if tuple(have.shape) != tuple(want.shape):
            bad.append((n, 'shape %s vs %s' % (tuple(have.shape), tuple(want.shape))))
        elif not want.is_floating_point():
            if not torch.equal(have, want):
                bad.append((n, 'counter %s vs %s' % (have.tolist(), want.tolist())))
        elif 'buf:' in n:
            err = (have.double() - want).abs()
            over = float((err - (R.STAT_ATOL + R.STAT_RTOL * want.abs())).max())
            log('%s %s bf16x3 %s: max err %.3g, worst excess over atol + rtol |ref| %.3g' % (topo, sit, n, float(err.max()), over))
            if not over <= 0:
                bad.append((n, 'running statistic off by %.3g' % float(err.max())))
        else:
            sc = float(want.abs().max())
            e = float((have.double() - want).abs().max())
            log('%s %s bf16x3 %s: max err %.3g = %.3g of max|ref| %.3g (bound %.3g)' % (topo, sit, n, e, e / sc if sc else float('nan'), sc, bnd[n]))
            if not e <= bnd[n] * sc:
                bad.append((n, 'err %.3g of scale, bound %.3g' % (e / sc if sc else float('inf'), bnd[n])))
    return bad

