"""An fp64 reference for the inference conv kernels (cpg_conv2d_fwd_bn_eval: conv3x3 s1 p1 -> BatchNorm2d(eval) [-> ReLU] as one
kernel), for the tests.

    y = relu?( BN_eval( conv3x3_s1_p1(x, w * bin(pm)) + bias ) )

The effective weight is oracle.ops.effective_weight (fp32, the reference's own expression); the convolution is a float64
F.conv2d on the CPU; the BatchNorm is F.batch_norm(training=False)'s formula, (v - mean) / sqrt(var + eps) * gamma + beta,
evaluated in float64 from the fp32 parameters.

Alongside it comes an elementwise error bound for an fp32 kernel:

    bound = gamma_k * U32 * |s| * (|x| (*) |w_eff|)  +  U32 * shift_mag,     s = gamma / sqrt(var + eps)

(|x| (*) |w_eff|: the fp64 convolution of the absolute values.)  The first term is the contraction's rounding, with one constant per
kernel family (GAMMA).  The Winograd kernels round intermediate values that mix a 4 x 4 input patch with every tap of the filter and
cancel only in exact arithmetic, so their magnitude is |x| summed over the 5 x 5 window around the output pixel (the union of the
patches of the tile positions it can take) times sum |w_eff[k][c]| over the taps, in place of |x| (*) |w_eff|: with one live tap
and an input near zero under it, the error is the neighbours' rounding, not that tap's.  The second is the epilogue's.  Its five fp32 operations -- bias add, mean subtract, 1 / sqrt(var + eps), the
two multiplies, the beta add -- each err by at most U32 of their result.  shift_mag = 8 * (|s| * (|bias| + |mean|) + |beta|) bounds
them by the magnitudes of the shift's parts, not by |beta - s * (mean - bias)|: those two may cancel.  For an output channel with no
live weight |x| (*) |w_eff| is 0, so the bound is the shift term alone: the kernel must write BN(bias) to within its own rounding.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ops

U32 = 2.0 ** -24                 # fp32 unit roundoff

# Smallest power of two that clears, by a factor of at least 4, the largest ratio
#     max over elements with |x| (*) |w_eff| > 0 of  (|y - ref| - U32 * shift_mag) / (U32 * |s| * (|x| (*) |w_eff|))
# measured on an MI355X over every case of tests/test_eval_conv_gpu.py (the test module records the ratios it sees).
# direct k_c3_fwd (C3BnEval), every tile config: 3.65-6.43 per case, largest 6.43 (D128 forced and D64, 78 -> 78 at 56 x 56) -> 32
GAMMA_DIRECT = 32.0
# Winograd BNE: k_wg1 0.12-0.16, k_wg2 0.15, k_wg3 (ODD included) 0.13-0.56, largest 0.56 (k_wg3, 156 -> 313 at 28 x 28) -> 4
# (against the 5 x 5 window magnitude of the module docstring, which is about 25x the direct kernels' |x| (*) |w_eff|)
GAMMA_WINO = 4.0
GAMMA = {'direct': GAMMA_DIRECT, 'winograd': GAMMA_WINO}


def _f64(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def eval_conv_terms(x, w, pm=None, bias=None, gamma=None, beta=None, mean=None, var=None, eps=1e-5, relu=True,
                    threshold=ops.DEFAULT_THRESHOLD, family='direct'):
    """(ref, conv_term, shift_term), all float64 CPU tensors of y's shape: the reference output, U32 * |s| * (the family's
    contraction magnitude) and U32 * shift_mag (see the module docstring).  Tensors may live anywhere; they are read as fp32
    values."""
    w = torch.as_tensor(w).detach().cpu().float()
    pmn = None if pm is None else torch.as_tensor(pm).detach().cpu().float().numpy()
    weff = torch.from_numpy(ops.effective_weight(w.numpy(), pmn, threshold)).double()
    xd = _f64(x)
    K = weff.shape[0]
    conv = F.conv2d(xd, weff, None, stride=1, padding=1)
    if family == 'winograd':
        l1 = weff.abs().sum((2, 3), keepdim=True).expand(-1, -1, 5, 5).contiguous()
        absconv = F.conv2d(xd.abs(), l1, None, stride=1, padding=2)
    else:
        absconv = F.conv2d(xd.abs(), weff.abs(), None, stride=1, padding=1)
    b = _f64(bias) if bias is not None else torch.zeros(K, dtype=torch.float64)
    g, be, mu, va = _f64(gamma), _f64(beta), _f64(mean), _f64(var)
    s = g / torch.sqrt(va + float(eps))
    ref = (conv + b[:, None, None] - mu[:, None, None]) * s[:, None, None] + be[:, None, None]
    if relu:
        ref = ref.clamp_min(0.0)
    conv_term = U32 * s.abs()[:, None, None] * absconv
    shift_mag = 8.0 * (s.abs() * (b.abs() + mu.abs()) + be.abs())
    shift_term = (U32 * shift_mag)[:, None, None].expand_as(ref)
    return ref, conv_term, shift_term


def eval_conv_ref(x, w, pm=None, bias=None, gamma=None, beta=None, mean=None, var=None, eps=1e-5, relu=True,
                  threshold=ops.DEFAULT_THRESHOLD, family='direct'):
    """(ref, bound): the fp64 reference output and the elementwise bound for a kernel of `family` ('direct' | 'winograd', or a
    number: the contraction constant itself)."""
    ref, conv_term, shift_term = eval_conv_terms(x, w, pm, bias, gamma, beta, mean, var, eps, relu, threshold,
                                                 family if isinstance(family, str) else 'direct')
    k = GAMMA[family] if isinstance(family, str) else float(family)
    return ref, k * conv_term + shift_term


def error_ratio(y, ref, conv_term, shift_term):
    """Largest (|y - ref| - shift_term) / conv_term over the elements with conv_term > 0: the smallest contraction constant
    under which y meets the bound (0.0 when no such element exceeds its shift term)."""
    err = (torch.as_tensor(y).detach().cpu().double() - ref).abs() - shift_term
    m = conv_term > 0
    if not bool(m.any()):
        return 0.0
    return max(0.0, float((err[m] / conv_term[m]).max()))


def live_input_extent(w, pm=None, threshold=ops.DEFAULT_THRESHOLD):
    """4 * (number of 4-channel input chunks up to the last one with a non-zero effective weight), 0 when every weight is
    dead: what the kernels report in skip_stats[0]."""
    w = torch.as_tensor(w).detach().cpu().float().numpy()
    pmn = None if pm is None else torch.as_tensor(pm).detach().cpu().float().numpy()
    weff = ops.effective_weight(w, pmn, threshold)
    live = np.nonzero((weff != 0).any(axis=(0, 2, 3)))[0]
    return 0 if live.size == 0 else 4 * (int(live[-1]) // 4 + 1)


def dead_output_channels(w, pm=None, threshold=ops.DEFAULT_THRESHOLD):
    """bool[K]: output channels whose effective weights are all zero (+0.0 or -0.0)."""
    w = torch.as_tensor(w).detach().cpu().float().numpy()
    pmn = None if pm is None else torch.as_tensor(pm).detach().cpu().float().numpy()
    weff = ops.effective_weight(w, pmn, threshold)
    return torch.from_numpy(~(weff != 0).any(axis=(1, 2, 3)))
