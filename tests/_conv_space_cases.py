"""The descriptor space of the conv entry points: a hand table of near misses of every fast class and of the generic family's own
branches (SPACE_CASES), a seeded stratified sampler (sweep_cases) and ONE body (conv_space) that holds whatever SharableConv2d
runs for a descriptor to torch's float64 conv2d and its autograd.  tests/test_conv_descriptor_space_host.py checks the table,
the sampler and the planner answers without a GPU; tests/test_conv_descriptor_space_gpu.py runs the body plainly and with
misplaced pointers; tests/test_guard_bands_gpu.py runs the table between guard bands.

What is pinned here is DISPATCH: every descriptor make_geom accepts runs a kernel that computes that descriptor.  Maps and
channel counts are tiny on purpose (routes decide on classes, not sizes) but chosen so that a misroute WOULD land on the fast
kernel: >= 16 channels on both sides and a multiple of 4 for the Winograd kernels, even maps, C <= 3 and K = 64 for the stems.

Tolerances are tests/_parity_cases.py conv_oracle's, nothing new: rtol 1e-4 throughout, atol 2e-5 for y and gx,
1e-5 * max(max|gw|, 1) for gw and gpm, 1e-3 for gb."""
import collections
import ctypes
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import _parity_cases as PC

THR = 5e-3
RTOL = 1e-4
ATOL_Y = 2e-5
ATOL_GW = 1e-5          # times max(max|gw|, 1)
ATOL_GB = 1e-3
LIMIT_N, LIMIT_CH, LIMIT_MAP = 3, 64, 24          # the hand table's rows stay at or below these

Case = collections.namedtuple('Case', 'id cls N C H W K R S sh sw ph pw dh dw G bias pm plan bitexact mis')

# The planner queries of tests/test_conv_descriptor_space_host.py, by the key the table uses for them.  A `plan` entry of a row
# is the expected NON-ZERO answer; every query a row does not name must answer 0.  For the two *_tiles queries the entry True
# stands for "some positive count" (the count itself is the tile plan's business, the launch sizes its buffer from the same call).
PLAN_KEYS = ('wino0', 'wino1', 'wino2', 'wino3', 'bn_eval', 'bn_eval_add', 'prelu_eval0', 'prelu_eval1', 'dgrad_add', 'rider', 'pool_max',
             'stem_bn', 'bf16', 'wgrad_bf16', 'bnstats_tiles', 'bnbwd_tiles')

# include/cpg_hip.h, "Inference ...": the pointwise class is `1x1, any stride, pad 0, C and K multiples of 16` -- stride and
# dilation (which a 1x1 kernel cannot see) do not leave it: the inference epilogues and the fused statistics apply ...
PW = {'bn_eval': 1, 'bn_eval_add': 1, 'bnstats_tiles': True}
# ... and `Dense 1x1 layers` (cpg_conv2d_dgrad_add) are the stride-1 ones among them
PW_DENSE = dict(PW, dgrad_add=1)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _row(cid, cls, nchw, K, k, s=1, p=0, d=1, G=1, bias=False, pm=False, plan=None, bitexact=False, mis=False):
    N, C, H, W = nchw
    (R, S), (sh, sw), (ph, pw), (dh, dw) = _pair(k), _pair(s), _pair(p), _pair(d)
    return Case(cid, cls, N, C, H, W, K, R, S, sh, sw, ph, pw, dh, dw, G, bias, pm, dict(plan or {}), bitexact, mis)


def _near(prefix, cls, nchw, K, rows):
    return [_row(prefix + '-' + tag, cls, nchw, K, **kw) for tag, kw in rows]


# bitexact: the route has no alignment predicate, so a run on misplaced pointers takes the same kernels and must give the same BITS
# (the generic implicit GEMM, Winograd / direct 3x3, 3x3 s2, both stem families; their one exception is the bias gradient, whose
# float4 flavour asks for a 16-byte aligned gy: gb is compared bit for bit only where gy keeps its alignment).  The pointwise
# kernels and the linear layers switch on the alignment of their INPUTS, the grouped kernels on that of the OUTPUT they store (and
# only on maps >= 16 wide): float64 checks only.
# mis: the row runs in test_space_table_misaligned (inputs and parameters moved) and test_space_outputs_misplaced (outputs moved).
C3 = (2, 16, 8, 8)
VS = (2, 3, 12, 12)
_NEAR_C3 = [
    ('p10', dict(k=3, p=(1, 0))), ('p01', dict(k=3, p=(0, 1), bias=True)), ('p00', dict(k=3, p=0, pm=True)), ('p22', dict(k=3, p=2)),
    ('s12', dict(k=3, s=(1, 2), p=1, pm=True)), ('s21', dict(k=3, s=(2, 1), p=1, bias=True)),
    ('d12', dict(k=3, d=(1, 2), p=(1, 2))), ('d22', dict(k=3, d=2, p=2, bias=True, pm=True)),
    ('k31', dict(k=(3, 1), p=(1, 0))), ('k13', dict(k=(1, 3), p=(0, 1), pm=True)), ('k35', dict(k=(3, 5), p=(1, 2), bias=True)),
]
SPACE_CASES = (
    # ---- near 3x3 s1 p1: one field off the class of cpg_conv3x3_supported (Winograd forward / input gradient, direct 3x3) ...
    _near('n3', 'near-3x3', C3, 16, _NEAR_C3)
    # ... and off the fused VGG stem (cpg_stem_bn_supported: 3x3 s1 p1 from <= 3 channels to 64) and the stem weight gradient
    + _near('nv', 'near-3x3', VS, 64, _NEAR_C3)
    # ---- near 3x3 s2 p1 (cpg_conv3x3s2_supported: >= 16 channels on both sides)
    + _near('ns2', 'near-3x3s2', (2, 16, 12, 12), 16, [
        ('p10', dict(k=3, s=2, p=(1, 0), bias=True)), ('p01', dict(k=3, s=2, p=(0, 1))), ('p00', dict(k=3, s=2, p=0, pm=True)),
        ('s21', dict(k=3, s=(2, 1), p=1)), ('s12', dict(k=3, s=(1, 2), p=1, bias=True, pm=True)), ('d2', dict(k=3, s=2, d=2, p=2))])
    + [_row('ns2-c8', 'near-3x3s2', (2, 8, 12, 12), 16, 3, s=2, p=1, pm=True)]            # < 16 input channels: the generic family
    # ---- near the strided image stems (cpg_conv_stem2_ok: 7x7 s2 p3 and 3x3 s2 p1 from <= 3 channels)
    + _near('nst', 'near-stem2', (2, 3, 20, 22), 64, [
        ('7p32', dict(k=7, s=2, p=(3, 2))), ('7s21', dict(k=7, s=(2, 1), p=3, bias=True)), ('5', dict(k=5, s=2, p=2, pm=True)),
        ('3p10', dict(k=3, s=2, p=(1, 0), bias=True, pm=True)), ('7d2', dict(k=7, s=2, p=3, d=2))])
    + [_row('nst-7c4', 'near-stem2', (2, 4, 20, 22), 64, 7, s=2, p=3, pm=True)]           # one input channel too many
    # ---- pointwise: unequal strides (forward staging, scatter + memset input gradient, per-pixel weight gradient), dilation (cannot
    # matter: still the pointwise class), padding (border outputs are the bias alone; the generic family)
    + [_row('pw-s21', 'pointwise', (2, 32, 12, 12), 64, 1, s=(2, 1), pm=True, plan=PW, mis=True),
       _row('pw-s12-k80', 'pointwise', (2, 16, 15, 14), 80, 1, s=(1, 2), bias=True, plan=PW, mis=True),
       _row('pw-s32', 'pointwise', (3, 48, 15, 14), 32, 1, s=(3, 2), plan=PW, mis=True),
       _row('pw-s21-k80', 'pointwise', (2, 32, 12, 12), 80, 1, s=(2, 1), bias=True, pm=True, plan=PW, mis=True),
       _row('pw-p11', 'pointwise', (2, 32, 12, 12), 64, 1, p=1, bias=True, bitexact=True, mis=True),
       _row('pw-p01-k80', 'pointwise', (2, 16, 15, 14), 80, 1, p=(0, 1), pm=True, bitexact=True),
       _row('pw-d23-k80', 'pointwise', (2, 32, 12, 12), 80, 1, d=(2, 3), bias=True, plan=PW_DENSE, mis=True),
       _row('pw-d23', 'pointwise', (2, 16, 15, 14), 64, 1, d=(2, 3), pm=True, plan=PW_DENSE, mis=True),
       # K <= 64, dense, a 144-pixel plane: the forward's float4 <-> per-pixel flip of the narrow tile (PW_V64 <-> PW_S64)
       _row('pw-d21-k48', 'pointwise', (2, 32, 12, 12), 48, 1, d=(2, 1), plan=PW_DENSE, mis=True)]
    # ---- the generic input gradient's residue classes (cpg_conv2d_dgrad_generic)
    + [_row('dg-s23', 'generic-dgrad', (2, 12, 13, 14), 20, 3, s=(2, 3), p=1, pm=True, bitexact=True),      # sh != sw
       _row('dg-k23-s31', 'generic-dgrad', (2, 20, 11, 9), 12, (2, 3), s=(3, 1), bias=True, bitexact=True, mis=True),   # rho = 2 >= R: a whole class without taps
       _row('dg-k4s2', 'generic-dgrad', (2, 8, 10, 12), 24, 4, s=2, p=1, bitexact=True),                     # two taps per class and axis
       _row('dg-s4-5x6', 'generic-dgrad', (3, 6, 5, 6), 10, 3, s=4, bias=True, pm=True, bitexact=True),      # one output; class 3 has no taps
       _row('dg-s4-2x3', 'generic-dgrad', (2, 6, 2, 3), 10, 3, s=4, p=1, bitexact=True),                     # h_start >= H for rho = 0
       _row('dg-s2d2', 'generic-dgrad', (2, 12, 12, 10), 16, 3, s=2, d=2, p=2, pm=True, bitexact=True),      # strided + dilated: one launch
       _row('dg-s21-d12', 'generic-dgrad', (2, 16, 9, 12), 12, 3, s=(2, 1), d=(1, 2), p=(1, 2), bias=True, bitexact=True, mis=True),
       _row('dg-k2s3', 'generic-dgrad', (2, 10, 11, 11), 14, 2, s=3, p=1, bitexact=True)]                    # class 2 has no taps on either axis
    # ---- degenerate geometry the ABI accepts
    + [_row('dz-p3', 'degenerate', (2, 8, 6, 6), 8, 3, p=3, bias=True, bitexact=True),                       # the outer ring of outputs sees padding only
       _row('dz-k5-3x3', 'degenerate', (2, 8, 3, 3), 12, 5, p=2, pm=True, bitexact=True),                    # kernel larger than the map
       _row('dz-k7d2-9x9', 'degenerate', (1, 4, 9, 9), 6, 7, d=2, p=6, bias=True, bitexact=True),            # extent 13 on a 9 x 9 map
       _row('dz-k13-h1', 'degenerate', (3, 16, 1, 9), 16, (1, 3), p=(0, 1), bitexact=True),                  # H = 1
       _row('dz-k31-w1', 'degenerate', (3, 16, 10, 1), 16, (3, 1), p=(1, 0), bias=True, pm=True, bitexact=True),      # W = 1
       _row('dz-keqmap', 'degenerate', (2, 6, 5, 7), 9, (5, 7), pm=True, bitexact=True)]                     # kernel == map: OH = OW = 1
    # ---- grouped, off the 3x3 / 5x5 templates of conv_grouped.hip (launch_gd_ks) and round the 16-channels-per-group MFMA boundary
    + [_row('g-dw3', 'grouped', (2, 24, 10, 10), 24, 3, p=1, G=24, bias=True, mis=True),                     # depthwise
       _row('g-mult2', 'grouped', (2, 12, 9, 11), 24, 3, p=1, G=12, pm=True),                                # channel multiplier 2
       _row('g-dw5s2', 'grouped', (2, 24, 11, 10), 24, 5, s=2, p=2, G=24),
       _row('g-dw35', 'grouped', (2, 16, 8, 12), 16, (3, 5), p=(1, 2), G=16, bias=True, pm=True, mis=True),  # rectangular: the run-time KS = 0 path
       _row('g-dw3d2', 'grouped', (2, 24, 10, 10), 24, 3, d=2, p=2, G=24, pm=True),
       _row('g16-s21', 'grouped', (2, 32, 12, 12), 32, 3, s=(2, 1), p=1, G=2, bias=True),                    # 16 per group: the MFMA boundary
       _row('g16-k13', 'grouped', (2, 32, 12, 12), 32, (1, 3), p=(0, 1), G=2, pm=True, mis=True),
       _row('g16-p10', 'grouped', (2, 32, 12, 12), 32, 3, p=(1, 0), G=2),
       _row('g15', 'grouped', (2, 30, 12, 12), 30, 3, p=1, G=2, bias=True, mis=True),                        # 15 per group: direct
       _row('g-k7', 'grouped', (2, 16, 12, 12), 16, 7, p=3, G=4, pm=True),
       _row('g-pw-s12', 'grouped', (2, 32, 9, 10), 32, 1, s=(1, 2), G=4, bias=True, mis=True),
       # maps >= 16 wide with 4 | width: four outputs per lane, stored as one float4 where `out` (y / gx) is 16-byte aligned
       # (conv_grouped.hip's vec_ok).  SharableConv2d allocates y and gx itself: only test_space_outputs_misplaced moves them.
       _row('g-dw3-w16', 'grouped', (2, 8, 6, 16), 8, 3, p=1, G=8, bias=True, mis=True),                     # the 3x3 unit-stride template
       _row('g4-k13-w20', 'grouped', (2, 8, 5, 20), 8, (1, 3), p=(0, 1), G=2, pm=True, mis=True)]            # the run-time path
    # ---- the fast families themselves, one row each: they check no alignment and read x with 8-byte loads (the misaligned test's
    # rows; `plan` holds what makes each the family it is said to be)
    + [_row('f-wino', 'fast', (2, 32, 8, 8), 32, 3, p=1, pm=True, bitexact=True, mis=True,                   # Winograd forward and input gradient
            plan={'wino0': 1, 'wino1': 1, 'wino3': 1, 'bn_eval': 1, 'prelu_eval0': 1, 'prelu_eval1': 1, 'bf16': 1, 'wgrad_bf16': 1,
                  'bnstats_tiles': True, 'bnbwd_tiles': True}),
       _row('f-direct', 'fast', (2, 16, 7, 9), 16, 3, p=1, bias=True, bitexact=True, mis=True,               # odd map: the direct 3x3 kernels
            plan={'bn_eval': 1, 'prelu_eval0': 1, 'prelu_eval1': 1, 'bf16': 1, 'wgrad_bf16': 1, 'bnstats_tiles': True, 'bnbwd_tiles': True}),
       _row('f-wino-wgrad', 'fast', (2, 32, 14, 14), 32, 3, p=1, bitexact=True, mis=True,                    # 14 wide, 32 | channels: the adjoint transform
            plan={'wino0': 1, 'wino1': 1, 'wino2': 1, 'wino3': 1, 'bn_eval': 1, 'prelu_eval0': 1, 'prelu_eval1': 1, 'bf16': 1,
                  'wgrad_bf16': 1, 'bnstats_tiles': True, 'bnbwd_tiles': True}),
       _row('f-s2', 'fast', (2, 16, 12, 12), 16, 3, s=2, p=1, pm=True, bitexact=True, mis=True,
            plan={'bn_eval': 1, 'prelu_eval0': 1, 'bnstats_tiles': True}),
       _row('f-vgg-stem', 'fast', VS, 64, 3, p=1, bitexact=True, mis=True,
            plan={'stem_bn': 1, 'bn_eval': 1, 'prelu_eval0': 1, 'prelu_eval1': 1, 'bnstats_tiles': True, 'bnbwd_tiles': True}),
       _row('f-stem7', 'fast', (2, 3, 20, 22), 64, 7, s=2, p=3, pm=True, bitexact=True, mis=True, plan={'bnstats_tiles': True}),
       _row('f-stem3', 'fast', (2, 3, 20, 22), 64, 3, s=2, p=1, bias=True, bitexact=True, mis=True, plan={'bnstats_tiles': True})]
)
CASE_BY_ID = collections.OrderedDict((c.id, c) for c in SPACE_CASES)
NEAR_MISS_CLASSES = ('near-3x3', 'near-3x3s2', 'near-stem2', 'pointwise')

# linear shapes on alignment predicates: cpg_pw_gemm_nt_ok (x, w; and pm at igemm_conv.hip cpg_linear_fwd) and cpg_fc_small_dgrad_ok
# (w, pm through the layer; gx only in test_linear_dgrad_output_misplaced).  None of the four has the 192 tiles cpg_pw_gemm_nn_ok
# asks for, so the `& 15` terms of the nn GEMM routes (cpg_linear_dgrad's transpose route, cpg_linear_wgrad) do NOT flip on them.
LINEAR_MISALIGNED = [(8, 132, 18), (40, 256, 128), (130, 64, 128), (33, 4100, 1000)]
# name -> (floats the activations x / gy are moved into their buffer, floats the parameters w / pm / bias are)
PLACEMENTS = collections.OrderedDict([('act+1', (1, 0)), ('par+1', (0, 1)), ('all+3', (3, 3))])


# --------------------------------------------------------------------------- geometry
def out_hw(c):
    return ((c.H + 2 * c.ph - c.dh * (c.R - 1) - 1) // c.sh + 1, (c.W + 2 * c.pw - c.dw * (c.S - 1) - 1) // c.sw + 1)


def desc_of(c):
    from cpg_amd import _lib
    d = _lib.ConvDesc()
    d.N, d.C, d.H, d.W, d.K, d.R, d.S = c.N, c.C, c.H, c.W, c.K, c.R, c.S
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w, d.groups = c.sh, c.sw, c.ph, c.pw, c.dh, c.dw, c.G
    return d


def padding_only_mask(c):
    """bool[OH][OW]: output positions whose receptive field lies wholly in the padding.  A tap (r, s) reads the map iff its row AND
    its column are inside, so a position sees nothing iff every tap row is outside or every tap column is."""
    OH, OW = out_hw(c)

    def dead(n_out, stride, pad, dil, k, size):
        return torch.tensor([all(not 0 <= o * stride - pad + t * dil < size for t in range(k)) for o in range(n_out)])
    return dead(OH, c.sh, c.ph, c.dh, c.R, c.H)[:, None] | dead(OW, c.sw, c.pw, c.dw, c.S, c.W)[None, :]


# --------------------------------------------------------------------------- the seeded sweep
STRATA = ('3x3-like', '1x1', 'rect', 'strided', 'dilated', 'grouped')


def strata_counts(n):
    """Equal shares, the remainder to the first strata."""
    return [n // len(STRATA) + (1 if i < n % len(STRATA) else 0) for i in range(len(STRATA))]


def _draw(rs, stratum, cid):
    r = lambda lo, hi: int(rs.randint(lo, hi + 1))            # noqa: E731  (inclusive)
    R, S, sh, sw, dh, dw, G = r(1, 7), r(1, 7), r(1, 3), r(1, 3), r(1, 3), r(1, 3), 1
    C, K = r(1, 40), r(1, 40)
    if stratum == '3x3-like':         # a 3x3 one or two fields off the fast classes; channel counts the Winograd kernels would take, half the time
        R = S = 3
        sh, sw, dh, dw = r(1, 2), r(1, 2), 1, 1
        if r(0, 1):
            C, K = 4 * r(4, 10), 4 * r(4, 10)
    elif stratum == '1x1':            # channel counts of the pointwise class half the time
        R = S = 1
        if r(0, 1):
            C, K = 16 * r(1, 2), 16 * r(1, 2)
    elif stratum == 'rect':
        sh = sw = dh = dw = 1
        if R == S:
            S = S % 7 + 1
    elif stratum == 'strided':
        dh = dw = 1
        if sh == 1 and sw == 1:
            sh, sw = [(2, 1), (1, 2), (3, 3)][r(0, 2)]
    elif stratum == 'dilated':
        R, S = max(R, 2), max(S, 2)
        if dh == 1 and dw == 1:
            dh, dw = [(2, 1), (1, 3), (2, 2)][r(0, 2)]
    elif stratum == 'grouped':
        G = [2, 3, 4][r(0, 2)]
        if r(0, 3) == 0:              # depthwise with a channel multiplier of 1 or 2
            G = r(2, 24)
            C, K = 1, r(1, 2)
        C, K = C * G, K * G
    ph, pw = r(0, dh * (R - 1) + 1), r(0, dw * (S - 1) + 1)
    N, H, W = r(1, 3), r(1, 20), r(1, 20)
    H = max(H, dh * (R - 1) + 1 - 2 * ph)                     # raised until OH, OW >= 1: no draw is rejected
    W = max(W, dw * (S - 1) + 1 - 2 * pw)
    return Case(cid, stratum, N, C, H, W, K, R, S, sh, sw, ph, pw, dh, dw, G, bool(r(0, 1)), bool(r(0, 1)), {}, False, False)


def sweep_cases(n=160, seed=20261):
    rs = np.random.RandomState(seed)
    out = []
    for stratum, count in zip(STRATA, strata_counts(n)):
        for _ in range(count):
            out.append(_draw(rs, stratum, '%d-%d' % (seed, len(out))))
    return out


# --------------------------------------------------------------------------- inputs and the float64 reference, once per case
_REFS = {}


def inputs(c):
    """x, w, b, pm, gy as fp32 CPU tensors, drawn as conv_oracle draws them."""
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()) & 0x7FFFFFFF)
    cg = c.C // c.G
    x = torch.randn(c.N, c.C, c.H, c.W, generator=g)
    w = torch.randn(c.K, cg, c.R, c.S, generator=g) * (2.0 / (cg * c.R * c.S)) ** 0.5
    b = torch.randn(c.K, generator=g) * 0.1 if c.bias else None
    pm = torch.rand(c.K, cg, c.R, c.S, generator=g) * 0.012 if c.pm else None
    gy = torch.randn((c.N, c.K) + out_hw(c), generator=g)
    return x, w, b, pm, gy


def conv_and_grads(c, x, w, b, pm, gy, dtype):
    """torch's conv2d and its autograd in `dtype` on the CPU: {y, gx, gw, gpm, gb}, with gw = gW_eff * bin(pm) and gpm = gW_eff * W
    (oracle/ops.py conv2d_backward)."""
    keep = None if pm is None else (pm > THR).to(dtype)
    xd = x.to(dtype).requires_grad_(True)
    weff = (w.to(dtype) if keep is None else w.to(dtype) * keep).requires_grad_(True)
    bd = None if b is None else b.to(dtype).requires_grad_(True)
    y = F.conv2d(xd, weff, bd, (c.sh, c.sw), (c.ph, c.pw), (c.dh, c.dw), c.G)
    y.backward(gy.to(dtype))
    out = {'y': y.detach(), 'gx': xd.grad, 'gw': weff.grad if keep is None else weff.grad * keep}
    if pm is not None:
        out['gpm'] = weff.grad * w.to(dtype)
    if b is not None:
        out['gb'] = bd.grad
    return out


def reference(c):
    if c.id not in _REFS:
        ins = inputs(c)
        _REFS[c.id] = (ins, conv_and_grads(c, *ins, dtype=torch.float64))
    return _REFS[c.id]


def tolerances(ref):
    """name -> (rtol, atol) of conv_oracle."""
    scale = max(float(ref['gw'].abs().max()), 1.0)
    return {'y': (RTOL, ATOL_Y), 'gx': (RTOL, ATOL_Y), 'gw': (RTOL, ATOL_GW * scale), 'gpm': (RTOL, ATOL_GW * scale), 'gb': (RTOL, ATOL_GB)}


def worst(got, want, rtol, atol):
    """(largest |got - want|, largest |got - want| / (atol + rtol |want|)): <= 1 is numpy's assert_allclose passing."""
    err = (got.detach().cpu().double() - want).abs()
    if not err.numel():
        return 0.0, 0.0
    return float(err.max()), float((err / (atol + rtol * want.abs())).max())


# --------------------------------------------------------------------------- placement
class PlacedBuffers(PC.PlainBuffers):
    """PLAIN with every activation `act` floats and every parameter `par` floats into a larger buffer."""

    def __init__(self, act, par):
        self.act, self.par = act, par

    def put(self, t, offset=0):
        v = PC.PlainBuffers.put(self, t, offset or self.act)
        assert v is None or v.data_ptr() % 16 == (4 * (offset or self.act)) % 16
        return v

    def rehome(self, module, const_buffers=False):
        for p in module.parameters():
            p.data = PC.PlainBuffers.put(self, p.data, self.par)
            assert p.data_ptr() % 16 == (4 * self.par) % 16
        return module


def placed(place):
    return PC.PLAIN if place is None else PlacedBuffers(*PLACEMENTS[place])


# --------------------------------------------------------------------------- the body
def make_layer(c, w, b, pm, buf, dil=None):
    from cpg_amd.models import layers as nl
    layer = nl.SharableConv2d(c.C, c.K, (c.R, c.S), stride=(c.sh, c.sw), padding=(c.ph, c.pw), dilation=dil or (c.dh, c.dw), groups=c.G,
                              bias=c.bias).to(PC.DEV)
    layer.weight.data.copy_(w)
    if c.bias:
        layer.bias.data.copy_(b)
    if c.pm:
        layer.piggymask = nn.Parameter(pm.to(PC.DEV))
    return buf.rehome(layer)


def run_layer(layer, x, gy, buf):
    """Forward and backward through SharableConv2d: {y, gx, gw, gpm, gb} on the device."""
    xd = buf.put(x).requires_grad_(True)
    y = layer(xd)
    y.backward(buf.put(gy))
    out = {'y': y.detach(), 'gx': xd.grad, 'gw': layer.weight.grad}
    if layer.piggymask is not None:
        out['gpm'] = layer.piggymask.grad
    if layer.bias is not None:
        out['gb'] = layer.bias.grad
    return out


def check_stats(c, st, tiles, ref, buf=PC.PLAIN):
    """The partial sums stats[K][tiles][2] of a fused-statistics forward, finalized by the library, against the float64 running
    statistics at test_conv_epilogue_bn_statistics' bar.  Returns (running_mean, running_var)."""
    from cpg_amd import _lib
    assert st is not None and tuple(st.shape) == (c.K, tiles, 2), c.id
    OH, OW = out_hw(c)
    rm, rv = buf.zeros((c.K,)), buf.full((c.K,), 1.0)
    mean, invstd = buf.empty((c.K,)), buf.empty((c.K,))
    _lib.call('cpg_bn_stats_finalize', _lib.dptr(st.clone()), tiles, c.N, c.K, OH * OW, 1e-5, 0.1, _lib.dptr(rm), _lib.dptr(rv), _lib.dptr(mean),
              _lib.dptr(invstd), _lib.stream_ptr())
    y64, m = ref['y'], c.N * OH * OW
    mean64 = y64.mean(dim=(0, 2, 3))
    var64 = y64.var(dim=(0, 2, 3), unbiased=False)
    PC.running_stats_close(rm, (0.1 * mean64).numpy(), '%s running_mean' % c.id)
    PC.running_stats_close(rv, (0.9 + 0.1 * var64 * (m / max(m - 1, 1))).numpy(), '%s running_var' % c.id)
    return rm, rv


def conv_space(case, buf=PC.PLAIN, place=None, named=None):
    """One descriptor through SharableConv2d, forward and backward, against float64; then the statements that need no tolerance.
    place: a key of PLACEMENTS (buf is then ignored).  named: a dict that receives name -> the layer's output.  Every figure is
    printed before it is asserted (profiles/conv_descriptor_space.md is made from that output).  Returns the tensors the kernels produced."""
    from cpg_amd import _lib
    c = case
    if place is not None:
        buf = placed(place)
    (x, w, b, pm, gy), ref = reference(c)
    layer = make_layer(c, w, b, pm, buf)
    got = run_layer(layer, x, gy, buf)
    assert set(got) == set(ref)
    if named is not None:
        named.update(got)
    tol = tolerances(ref)
    for name in ('y', 'gx', 'gw', 'gpm', 'gb'):
        if name in ref:
            assert got[name].shape == ref[name].shape, (c.id, name)
            err, ratio = worst(got[name], ref[name], *tol[name])
            print('conv_space %s %s %s: worst error %.3e = %.4f of the tolerance' % (c.id, c.cls, name, err, ratio))
    for name in ('y', 'gx', 'gw', 'gpm', 'gb'):
        if name in ref:
            PC.close(got[name], ref[name].numpy(), rtol=tol[name][0], atol=tol[name][1], msg='%s %s' % (c.id, name))
    outs = [got[n] for n in ('y', 'gx', 'gw', 'gpm', 'gb') if n in got]

    # outputs that see only padding: the bias exactly, or +0.0
    mask = padding_only_mask(c)
    if bool(mask.any()):
        seen = got['y'].cpu()[:, :, mask]                     # [N][K][positions]
        if c.bias:
            assert torch.equal(seen, b[None, :, None].expand_as(seen)), c.id
        else:
            assert not bool(seen.view(torch.int32).any()), '%s: a padding-only output is not +0.0' % c.id

    # the fused BatchNorm statistics: the same y, bit for bit; statistics exactly where the planner says so, held to the float64 sums
    with torch.no_grad():
        y2, st = layer.forward_with_bn_stats(buf.put(x))
    assert torch.equal(y2, got['y']), c.id
    outs.append(y2)
    tiles = int(_lib.lib().cpg_conv2d_bnstats_tiles(ctypes.byref(desc_of(c))))
    if tiles == 0 or c.G > 1:
        assert st is None, c.id
    else:
        rm, rv = check_stats(c, st, tiles, ref, buf)
        outs += [st, rm, rv]

    # a 1x1 kernel cannot see its dilation: all five outputs bit-equal to the same layer built with dilation 1
    if c.R == 1 and c.S == 1 and (c.dh, c.dw) != (1, 1):
        plain = run_layer(make_layer(c, w, b, pm, buf, dil=(1, 1)), x, gy, buf)
        for name in got:
            assert torch.equal(got[name], plain[name]), (c.id, name, 'dilation changed a 1x1 layer')
    return outs


# --------------------------------------------------------------------------- the entry points themselves, outputs misplaced
def _misplaced(shape, off):
    """(whole, view): a NaN-filled buffer and a view of `shape` that starts `off` floats in, with four floats of NaN behind it."""
    n = int(np.prod(shape))
    whole = torch.full((n + off + 4,), float('nan'), device=PC.DEV)
    view = whole[off:off + n].view(shape)
    assert view.data_ptr() % 16 == (4 * off) % 16 and view.is_contiguous()
    return whole, view


def abi_outputs(case, off):
    """cpg_conv2d_fwd, _fwd_bnstats (where it has tiles), _dgrad and _wgrad called DIRECTLY, with every output -- y, the statistics,
    gx, gw, gpm, gb -- `off` floats into a buffer of its own and every input aligned: the output pointers are the ones SharableConv2d
    never misplaces (it allocates them).  Each output is held to float64 at conv_space's tolerances, has no element left unwritten,
    and nothing before or behind it was written.  Returns name -> tensor."""
    from cpg_amd import _lib
    c = case
    (x, w, b, pm, gy), ref = reference(c)
    L, d, s = _lib.lib(), desc_of(c), _lib.stream_ptr()
    P = _lib.dptr
    xd, wd, bd, pd, gyd = (None if t is None else t.to(PC.DEV).contiguous() for t in (x, w, b, pm, gy))
    ws, nb = _lib.workspace(L.cpg_conv2d_workspace_bytes(ctypes.byref(d)), PC.DEV)
    made = {}

    def out(name, shape):
        made[name] = _misplaced(shape, off)
        return made[name][1]
    head = (ctypes.byref(d), P(xd), P(wd), P(pd), THR, P(bd))
    _lib.call('cpg_conv2d_fwd', *head, P(out('y', ref['y'].shape)), P(ws), nb, s)
    tiles = int(L.cpg_conv2d_bnstats_tiles(ctypes.byref(d)))
    if tiles > 0:
        st = out('stats', (c.K, tiles, 2))
        _lib.call('cpg_conv2d_fwd_bnstats', *head, P(out('y2', ref['y'].shape)), P(st), st.numel() * 4, P(ws), nb, s)
    _lib.call('cpg_conv2d_dgrad', ctypes.byref(d), P(gyd), P(wd), P(pd), THR, P(out('gx', x.shape)), P(ws), nb, s)
    _lib.call('cpg_conv2d_wgrad', ctypes.byref(d), P(xd), P(gyd), P(wd), P(pd), THR, P(out('gw', w.shape)),
              P(out('gpm', w.shape)) if c.pm else None, P(out('gb', (c.K,))) if c.bias else None, P(ws), nb, s)
    torch.cuda.synchronize()
    got = {}
    for name, (whole, view) in made.items():
        n = view.numel()
        assert bool(torch.isnan(whole[:off]).all()) and bool(torch.isnan(whole[off + n:]).all()), (c.id, off, name, 'written outside the tensor')
        assert not bool(torch.isnan(view).any()), (c.id, off, name, 'an element was not written')
        got[name] = view
    tol = tolerances(ref)
    for name in ('y', 'gx', 'gw', 'gpm', 'gb'):
        if name in ref:
            err, ratio = worst(got[name], ref[name], *tol[name])
            print('abi_outputs %s %s +%d %s: worst error %.3e = %.4f of the tolerance' % (c.id, c.cls, off, name, err, ratio))
            PC.close(got[name], ref[name].numpy(), rtol=tol[name][0], atol=tol[name][1], msg='%s +%d %s' % (c.id, off, name))
    if tiles > 0:
        assert torch.equal(got['y2'], got['y']), (c.id, off)
        check_stats(c, got['stats'], tiles, ref)
    return got


def linear_dgrad_output(B, I, O, pm, off):
    """cpg_linear_dgrad called directly with gx `off` floats into its buffer (fc_small.hip's test of gx): held to float64 at
    linear_oracle's bar.  Returns gx."""
    from cpg_amd import _lib
    g = torch.Generator().manual_seed(B + I + O)
    w = torch.randn(O, I, generator=g) * I ** -0.5
    pmv = torch.rand(O, I, generator=g) * 0.012 if pm else None
    gy = torch.randn(B, O, generator=g)
    weff = w.double() * ((pmv > THR).double() if pm else 1.0)
    want = gy.double() @ weff
    whole, gx = _misplaced((B, I), off)
    ws, nb = _lib.workspace(_lib.lib().cpg_linear_workspace_bytes(B, I, O), PC.DEV)
    P = _lib.dptr
    gyd, wd, pd = gy.to(PC.DEV), w.to(PC.DEV), (None if pmv is None else pmv.to(PC.DEV))        # (named: alive until the call has run)
    _lib.call('cpg_linear_dgrad', P(gyd), P(wd), P(pd), THR, P(gx), B, I, O, P(ws), nb, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole[:off]).all()) and bool(torch.isnan(whole[off + B * I:]).all()) and not bool(torch.isnan(gx).any())
    PC.close(gx, want.numpy(), rtol=1e-4, atol=max(2e-5, 1e-5 * float(want.abs().max())), msg='gx')
    return gx
