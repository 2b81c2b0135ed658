"""An fp64 reference for the residual topologies' inference kernels (cpg_conv2d_fwd_bn_eval on the pointwise and the 3x3 stride-2
shapes, cpg_conv2d_fwd_bn_eval_add), for the tests: tests/_evalconv.py for any conv geometry, with the block's residual.

    y = relu?( BN_eval( conv(x, w * bin(pm), stride, padding) + bias ) + residual? )

The effective weight is oracle.ops.effective_weight, the convolution a float64 F.conv2d on the CPU and the BatchNorm
F.batch_norm(training=False)'s formula in float64 from the fp32 parameters, as there.  The elementwise bound for an fp32 kernel is

    bound = L * U32 * |s| * (|x| (*) |w_eff|)  +  U32 * (shift_mag + 2 * |residual|),        s = gamma / sqrt(var + eps)

L = C * R * S, the contraction length: a sum of L fp32 products in ANY order errs by at most gamma_L = L u / (1 - L u) ~ L * U32 of
the sum of their magnitudes, so the constant is a-priori and nothing is measured to set it (the direct 3x3 kernels' GAMMA_DIRECT of
_evalconv.py is a measured one).  shift_mag is _evalconv.py's, 8 * (|s| * (|bias| + |mean|) + |beta|): the epilogue's handful of fp32
operations, each within U32 of its result, bounded by the magnitudes of the shift's parts.  The residual term is the one extra add:
U32 of its result, which is at most |residual| plus the BatchNorm output the other terms already bound -- 2 * |residual| covers it.
ReLU is 1-Lipschitz, so the bound of the value before it holds after it.  Where an output channel has no live weight the first term
is 0: the kernel must write BN(bias) [+ residual] to within the second term alone.
"""
import torch
import torch.nn.functional as F

from _evalconv import U32, error_ratio, dead_output_channels          # noqa: F401  (re-exported for the tests)
from oracle import ops


def _f64(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def conv_parts(x, w, pm=None, stride=1, padding=0, threshold=ops.DEFAULT_THRESHOLD):
    """(conv, |x| (*) |w_eff|, L): the fp64 convolution with the effective weight, that of the absolute values, and the contraction
    length.  The part of the reference that does not depend on the bias, the BatchNorm or the residual: compute it once per input."""
    w = torch.as_tensor(w).detach().cpu().float()
    pmn = None if pm is None else torch.as_tensor(pm).detach().cpu().float().numpy()
    weff = torch.from_numpy(ops.effective_weight(w.numpy(), pmn, threshold)).double()
    xd = _f64(x)
    conv = F.conv2d(xd, weff, None, stride=stride, padding=padding)
    absconv = F.conv2d(xd.abs(), weff.abs(), None, stride=stride, padding=padding)
    return conv, absconv, int(w.shape[1] * w.shape[2] * w.shape[3])


def eval_res_terms(parts, bias, gamma, beta, mean, var, eps, residual=None):
    """(ref, conv_term, shift_term), float64 CPU tensors of y's shape: the reference BEFORE the ReLU, L * U32 * |s| * (|x| (*) |w_eff|)
    and U32 * (shift_mag + 2 * |residual|) (module docstring).  parts: conv_parts(...)."""
    conv, absconv, L = parts
    K = conv.shape[1]
    b = _f64(bias) if bias is not None else torch.zeros(K, dtype=torch.float64)
    g, be, mu, va = _f64(gamma), _f64(beta), _f64(mean), _f64(var)
    s = g / torch.sqrt(va + float(eps))
    ref = (conv + b[:, None, None] - mu[:, None, None]) * s[:, None, None] + be[:, None, None]
    conv_term = L * U32 * s.abs()[:, None, None] * absconv
    shift_mag = 8.0 * (s.abs() * (b.abs() + mu.abs()) + be.abs())           # (_evalconv.eval_conv_terms' definition)
    shift_term = (U32 * shift_mag)[:, None, None].expand_as(ref)
    if residual is not None:
        r = _f64(residual)
        ref = ref + r
        shift_term = shift_term + 2.0 * U32 * r.abs()
    return ref, conv_term, shift_term


def eval_res_ref(x, w, pm=None, bias=None, gamma=None, beta=None, mean=None, var=None, eps=1e-5, stride=1, padding=0, residual=None,
                 relu=True, threshold=ops.DEFAULT_THRESHOLD):
    """(ref, bound): the fp64 reference output and the elementwise bound, in one call."""
    ref, conv_term, shift_term = eval_res_terms(conv_parts(x, w, pm, stride, padding, threshold), bias, gamma, beta, mean, var, eps, residual)
    return (ref.clamp_min(0.0) if relu else ref), conv_term + shift_term
