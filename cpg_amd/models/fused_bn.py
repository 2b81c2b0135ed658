"""Fused BatchNorm2d -> ReLU for the blocks that follow every masked conv of the VGG topologies
(reference: `layers += [conv2d, nn.BatchNorm2d(c), nn.ReLU(inplace=True)]`, models/vgg.py:137-141).

The modules stay what they are in the reference (an `nn.BatchNorm2d` with its parameters / buffers and an
`nn.ReLU`), so state_dict keys, optimizer parameter lists and `shared_layer_info` bookkeeping are
unchanged; only the arithmetic of the pair is replaced by libcpg_hip.so's three-pass forward / five-pass
backward (csrc/bn_kernels.hip).  Semantics are torch.nn.BatchNorm2d's: batch statistics in training mode
(biased variance for the normalisation, unbiased for running_var, momentum update, num_batches_tracked),
running statistics in eval mode.  SURVEY.md section 8(f) item 2.
"""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from .layers import BiasGradSink, BnBwdHint, PoolMaxSink, _conv_desc

# ---- module-level switches (the per-Sequential ones -- fuse, fuse_pool, fuse_stats, fuse_eval -- are FusedSequential's attributes) ----
ENABLED = True          # module-wide switch (tests compare the fused against the stock evaluation)
# The BatchNorm backward reduction riding in the next conv's input-gradient epilogue.  OFF by default: it removes the 2-read
# reduction kernels (-2.4 ms per VGG16 step) but the input-gradient kernels pay the HBM time of the extra reads in an epilogue
# that nothing hides (+0.28 ms per layer); interleaved in-process A/B (tools/step_ab.py): 184.6 ms with it, 183.8 ms without.
ENABLE_BWD_HINT = False
# The BatchNorm backward APPLY pass riding in the next conv's Winograd weight-gradient kernel (MFMA-bound, HBM mostly idle: the loads are
# requested four k-steps ahead and every element is done once).  The library switch CPG_NO_WW_RIDER turns it off per process.
ENABLE_WGRAD_RIDER = True
RELU_BYTE_MASK = True   # relu(bn(x) + res): the forward leaves the ReLU mask as one byte per four outputs for the backward
FUSE_STEM = True        # conv(<= 3 -> 64 channels, 3x3 s1 p1) -> BatchNorm2d -> ReLU: the conv output is never written (cpg_stem_bn_*)
FUSE_STEM_WGRAD = True  # ... and its weight gradient inside the BatchNorm backward's apply pass (cpg_stem_bn_relu_bwd_wgrad)
FUSE_SKIP_ADD = True    # residual blocks: the identity branch's gradient is added in conv1's input-gradient epilogue
# Inference on the residual topologies: conv -> BatchNorm2d(eval) [-> + residual] [-> ReLU] as ONE kernel wherever the conv has such an
# epilogue (cpg_conv2d_fwd_bn_eval / _add: pointwise, 3x3 s1, 3x3 s2).  Off: conv, then the BatchNorm pass, launch for launch as before.
FUSE_EVAL_BLOCKS = True
# Inference on SphereNet: conv -> (+ bias) -> PReLU [-> + the unit's residual] as ONE kernel wherever the conv has such an epilogue
# (cpg_conv2d_fwd_prelu_eval: 3x3 s1, 3x3 s2 without a residual).  Off: conv, then cpg_prelu_fwd, launch for launch as before.
# OFF by default (profiles/spherenet_eval_fuse.md): the full-width forward measured 2.96 ms on against 2.66 ms off at batch 100 and 6.07
# against 5.89 ms at batch 256.  The epilogue itself saves what was estimated on the 56 x 56 layers (-0.046 ms per pair), but the fused call
# runs the INFERENCE plan of the conv, and on the eight 256 -> 256 pairs at 14 x 14 that plan -- the two-wave Winograd kernel without the
# shared input transform and without the tail launch of the training forward -- is 0.043 ms per pair slower than cpg_conv2d_fwd + the pass.
FUSE_EVAL_PRELU = False


def _batch_stats(stats, nbt, N, C, HW, eps, momentum, running_mean, running_var, training, device):
    """(mean, invstd, counter still to bump) a fused BatchNorm forward normalises with:
      eval                        the running statistics;
      training, `stats` given     finalised from the producing conv's [C][tiles][2] partial sums, the running statistics updated
                                  (cpg_bn_stats_finalize) -- and `nbt`, the layer's num_batches_tracked, bumped in the same launch when
                                  it is a one-element int64 HIP tensor (cpg_bn_stats_finalize_count: stock torch spends one `add<long>`
                                  launch per layer on it, 53 per ResNet-50 step);
      training, no `stats`        two empty vectors for the layer's own kernel to fill.
    The Function bumps a counter that comes back (not None) with _count() after its kernels."""
    if not training:
        return running_mean, torch.rsqrt(running_var + eps), nbt
    mean = torch.empty(C, dtype=torch.float32, device=device)
    invstd = torch.empty(C, dtype=torch.float32, device=device)
    if stats is not None:
        args = (_lib.dptr(stats, name='bn partial sums'), stats.shape[1], N, C, HW, float(eps), float(momentum),
                _lib.dptr(running_mean, name='running_mean'), _lib.dptr(running_var, name='running_var'), _lib.dptr(mean), _lib.dptr(invstd))
        if nbt is not None and running_mean is not None and nbt.is_cuda and nbt.dtype == torch.int64 and nbt.numel() == 1:
            _lib.call('cpg_bn_stats_finalize_count', *args, _lib.dptr(nbt, torch.int64, 'num_batches_tracked'), _lib.stream_ptr())
            nbt = None
        else:
            _lib.call('cpg_bn_stats_finalize', *args, _lib.stream_ptr())
    return mean, invstd, nbt


def _count(nbt):
    """nn.BatchNorm2d's `num_batches_tracked += 1` of a training-mode forward, where no kernel of the layer took it along."""
    if nbt is not None:
        nbt.add_(1)


def _bn_args(bn):
    """(what every fused BatchNorm Function takes after its input: parameters, running statistics, eps, momentum, training;
    training; the counter a training-mode forward bumps, or None)."""
    training = bn.training or not bn.track_running_stats
    rm, rv = (bn.running_mean, bn.running_var) if bn.track_running_stats else (None, None)
    nbt = bn.num_batches_tracked if (training and bn.track_running_stats) else None
    return (bn.weight, bn.bias, rm, rv, bn.eps, bn.momentum, training), training, nbt


def _bn_forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, training, stats, nbt, launch):
    """The forward frame of the fused BatchNorm Functions: the dense input and its shape, the statistics (_batch_stats), the workspace
    when the layer's own kernel computes them (`own_stats`: training mode and no partial sums from the producing conv), the
    Function's kernels, the counter, the saved tensors.
    launch(x, N, C, HW, mean, invstd, own_stats, ws, nb) runs the kernels and returns (y, further tensors to save)."""
    x = x.contiguous()
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // (N * C)
    mean, invstd, nbt = _batch_stats(stats, nbt, N, C, HW, eps, momentum, running_mean, running_var, training, x.device)
    own_stats = bool(training and stats is None)
    ws, nb = _lib.workspace(_lib.lib().cpg_bn_workspace_bytes(N, C, HW), x.device) if own_stats else (None, 0)
    y, extra = launch(x, N, C, HW, mean, invstd, own_stats, ws, nb)
    _count(nbt)
    ctx.save_for_backward(x, gamma, beta, mean, invstd, *extra)
    ctx.training = bool(training)
    return y


def _bn_backward(ctx, gy):
    """The backward frame: (saved tensors, the dense incoming gradient, N, C, HW, gx, dgamma, dbeta, workspace, its size)."""
    x, gamma, beta = ctx.saved_tensors[:3]
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // (N * C)
    ws, nb = _lib.workspace(_lib.lib().cpg_bn_workspace_bytes(N, C, HW), x.device)
    return ctx.saved_tensors, gy.contiguous(), N, C, HW, torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta), ws, nb


class _BnReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, training, relu, stats=None, hint=None, nbt=None):
        def launch(x, N, C, HW, mean, invstd, own_stats, ws, nb):
            y = torch.empty_like(x)
            if own_stats:
                _lib.call('cpg_bn_relu_fwd_train', _lib.dptr(x, name='input'), _lib.dptr(gamma, name='bn.weight'),
                          _lib.dptr(beta, name='bn.bias'), float(eps), float(momentum), _lib.dptr(running_mean, name='running_mean'),
                          _lib.dptr(running_var, name='running_var'), _lib.dptr(mean), _lib.dptr(invstd), _lib.dptr(y), N, C, HW, int(relu),
                          _lib.dptr(ws), nb, _lib.stream_ptr())
            else:
                # eval, or the producing conv already accumulated the partial sums: the apply pass alone
                _lib.call('cpg_bn_relu_fwd_eval', _lib.dptr(x, name='input'), _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(mean),
                          _lib.dptr(invstd), _lib.dptr(y), N, C, HW, int(relu), _lib.stream_ptr())
            ctx.hint = hint if (hint is not None and relu and training) else None
            if ctx.hint is not None:
                hint.fill(x, gamma, beta, mean, invstd, y.shape)
            return y, ()
        ctx.relu = bool(relu)
        return _bn_forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, training, stats, nbt, launch)

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        hint, ctx.hint = ctx.hint, None
        partials = None
        if hint is not None:
            result = hint.take(gy)
            if result is not None:
                # the consumer conv's weight-gradient kernel already ran this whole backward on exactly this gradient tensor
                return tuple(result) + (None,) * 9
            partials, hint.partials = hint.partials, None
        (x, gamma, beta, mean, invstd), gy, N, C, HW, gx, dgamma, dbeta, ws, nb = _bn_backward(ctx, gy)
        if partials is not None:
            # the consumer conv's input-gradient kernel already masked gy by the ReLU and reduced it per (channel, tile)
            _lib.call('cpg_bn_bwd_from_partials', _lib.dptr(partials), hint.tiles, _lib.dptr(x), _lib.dptr(gy, name='grad_output'),
                      _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(mean), _lib.dptr(invstd), _lib.dptr(gx), _lib.dptr(dgamma),
                      _lib.dptr(dbeta), N, C, HW, _lib.dptr(ws), nb, _lib.stream_ptr())
        else:
            _lib.call('cpg_bn_relu_bwd', _lib.dptr(x), _lib.dptr(gy, name='grad_output'), _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(mean),
                      _lib.dptr(invstd), _lib.dptr(gx), _lib.dptr(dgamma), _lib.dptr(dbeta), N, C, HW, int(ctx.relu), int(ctx.training),
                      _lib.dptr(ws), nb, _lib.stream_ptr())
        return (gx, dgamma, dbeta) + (None,) * 9


class _BnAddReluFn(torch.autograd.Function):
    """relu(bn(x) + res) -- forward in the two passes of plain BN; backward = ReLU mask from the saved output, the plain
    BN backward kernels, and the masked gradient itself for the residual."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, running_mean, running_var, eps, momentum, training, stats=None, nbt=None):
        res = res.contiguous()

        def launch(x, N, C, HW, mean, invstd, own_stats, ws, nb):
            y = torch.empty_like(x)
            # the backward's ReLU mask as one byte per four outputs, written by the forward pass (the backward then does not re-read y)
            mask = None
            nmask = _lib.lib().cpg_bn_add_relu_mask_bytes(N, C, HW) if (RELU_BYTE_MASK and any(ctx.needs_input_grad)) else 0
            if nmask and x.data_ptr() % 16 == 0 and res.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0:
                mask = torch.empty(nmask, dtype=torch.uint8, device=x.device)
            # (not own_stats -- eval, or partial sums from the producing conv's epilogue, cpg_conv2d_fwd_bnstats: the apply pass alone)
            _lib.call('cpg_bn_add_relu_fwd', _lib.dptr(x, name='input'), _lib.dptr(res, name='residual'), _lib.dptr(gamma), _lib.dptr(beta),
                      float(eps), float(momentum), _lib.dptr(running_mean if own_stats else None),
                      _lib.dptr(running_var if own_stats else None), _lib.dptr(mean), _lib.dptr(invstd), _lib.dptr(y),
                      N, C, HW, int(own_stats), _lib.dptr(ws), nb, _lib.stream_ptr(), _lib.dptr(mask, torch.uint8))
            ctx.has_mask = mask is not None
            return y, (y if mask is None else mask,)
        return _bn_forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, training, stats, nbt, launch)

    @staticmethod
    def backward(ctx, gy):
        (x, gamma, beta, mean, invstd, y), gy, N, C, HW, gx, dgamma, dbeta, ws, nb = _bn_backward(ctx, gy)
        mask, y = (y, None) if ctx.has_mask else (None, y)
        if mask is not None and gy.data_ptr() % 16:
            gy = gy.clone()
        gz = torch.empty_like(x)                       # gy * [y > 0]: the residual branch's gradient, written by the reduction pass
        _lib.call('cpg_bn_add_relu_bwd', _lib.dptr(x), _lib.dptr(y), _lib.dptr(gy, name='grad_output'), _lib.dptr(gamma), _lib.dptr(beta),
                  _lib.dptr(mean), _lib.dptr(invstd), _lib.dptr(gx), _lib.dptr(gz), _lib.dptr(dgamma), _lib.dptr(dbeta),
                  N, C, HW, int(ctx.training), _lib.dptr(ws), nb, _lib.stream_ptr(), _lib.dptr(mask, torch.uint8))
        return (gx, gz, dgamma, dbeta) + (None,) * 7


def _pool_backward(name, ctx, gp):
    """The backward shared by both BatchNorm2d -> ReLU -> MaxPool2d Functions (cpg_bn_relu_pool_bwd / cpg_bn_relu_pool3_bwd; with the
    window maxima saved by the forward, attached to the same call: cpg_bn_relu_pool_attach_max)."""
    (x, gamma, beta, mean, invstd, *emax), gp, N, C, _, gx, dgamma, dbeta, ws, nb = _bn_backward(ctx, gp)
    arms = tuple(('cpg_bn_relu_pool_attach_max', (_lib.dptr(e), e.numel() * 4)) for e in emax)
    _lib.call_armed(arms, name, _lib.dptr(x), _lib.dptr(gp, name='grad_output'), _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(mean),
                    _lib.dptr(invstd), _lib.dptr(gx), _lib.dptr(dgamma), _lib.dptr(dbeta), N, C, x.shape[2], x.shape[3], int(ctx.training),
                    _lib.dptr(ws), nb, _lib.stream_ptr())
    return (gx, dgamma, dbeta) + (None,) * 8


class _BnReluPoolFn(torch.autograd.Function):
    """BatchNorm2d -> ReLU -> MaxPool2d(2, 2); only the pooled tensor is written.  pool_max: the window maxima of x from the conv that
    produced it (PoolMaxSink.E, with that conv's `stats`): the forward apply pass and the backward reduction read them instead of x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, training, stats=None, nbt=None, pool_max=None):
        def launch(x, N, C, HW, mean, invstd, own_stats, ws, nb):
            H, W = x.shape[2:]
            y = torch.empty((N, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
            use_max = pool_max is not None and not own_stats
            arms = (('cpg_bn_relu_pool_attach_max', (_lib.dptr(pool_max, name='window maxima'), pool_max.numel() * 4)),) if use_max else ()
            _lib.call_armed(arms, 'cpg_bn_relu_pool_fwd', _lib.dptr(x, name='input'), _lib.dptr(gamma, name='bn.weight'),
                            _lib.dptr(beta, name='bn.bias'), float(eps), float(momentum), _lib.dptr(running_mean if own_stats else None),
                            _lib.dptr(running_var if own_stats else None), _lib.dptr(mean), _lib.dptr(invstd),
                            _lib.dptr(y), N, C, H, W, int(own_stats), _lib.dptr(ws), nb, _lib.stream_ptr())
            return y, ((pool_max,) if use_max else ())
        return _bn_forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, training, stats, nbt, launch)

    @staticmethod
    def backward(ctx, gp):
        return _pool_backward('cpg_bn_relu_pool_bwd', ctx, gp)


class _BnReluPool3Fn(torch.autograd.Function):
    """BatchNorm2d -> ReLU -> MaxPool2d(3, 2, 1) (the ResNet stem's tail); only the pooled tensor is written."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, training, stats, nbt=None):
        def launch(x, N, C, HW, mean, invstd, own_stats, ws, nb):
            H, W = x.shape[2:]
            if own_stats:
                # (the producing conv has no fused-statistics kernel -- narrow test nets: torch's own reduction for the statistics)
                var, mu = torch.var_mean(x, dim=(0, 2, 3), unbiased=False)
                mean.copy_(mu)
                invstd.copy_(torch.rsqrt(var + eps))
                n = x.numel() // C
                with torch.no_grad():
                    running_mean.mul_(1 - momentum).add_(mu, alpha=momentum)
                    running_var.mul_(1 - momentum).add_(var * (n / max(n - 1, 1)), alpha=momentum)
            y = torch.empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
            _lib.call('cpg_bn_relu_pool3_fwd', _lib.dptr(x, name='input'), _lib.dptr(gamma, name='bn.weight'), _lib.dptr(beta, name='bn.bias'),
                      _lib.dptr(mean), _lib.dptr(invstd), _lib.dptr(y), N, C, H, W, _lib.stream_ptr())
            return y, ()
        return _bn_forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, training, stats, nbt, launch)

    @staticmethod
    def backward(ctx, gp):
        return _pool_backward('cpg_bn_relu_pool3_bwd', ctx, gp)


def _is_pool(m, kernel, stride, padding):
    """`m` is a plain nn.MaxPool2d(kernel, stride, padding)."""
    def pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return (isinstance(m, nn.MaxPool2d) and pair(m.kernel_size) == (kernel, kernel) and pair(m.stride) == (stride, stride)
            and pair(m.padding) == (padding, padding) and pair(m.dilation) == (1, 1) and not m.ceil_mode and not m.return_indices)


def _is_pool2(m):
    return _is_pool(m, 2, 2, 0)


def _is_pool3(m):
    return _is_pool(m, 3, 2, 1)


def _stats_from_conv(bn, fuse_stats, x=None, need_grad=False):
    """`bn` can take its batch statistics from the epilogue of the conv in front of it: a training-mode, stat-tracking, affine
    BatchNorm2d with an exponential-average momentum, under the caller's `fuse_stats` switch (FusedSequential's -- an instance's in
    its forward, the class's in the free functions).  x: the conv's input, where the site has not yet established that it is on the
    device; need_grad: the site only fuses under autograd."""
    return (fuse_stats and isinstance(bn, nn.BatchNorm2d) and bn.training and bn.track_running_stats and bn.affine
            and bn.momentum is not None and (x is None or x.is_cuda) and (not need_grad or torch.is_grad_enabled()))


def conv_bn_act_pool(conv, bn, act, pool, x):
    """pool(act(bn(conv(x)))): the ResNet stem (models/resnet.py:208-211).  conv -> BatchNorm statistics in the conv epilogue,
    BatchNorm -> ReLU -> MaxPool2d(3, 2, 1) as one forward kernel and two backward kernels when the plane fits LDS."""
    y, stats = _conv_with_stats(conv, bn, x)
    if (ENABLED and FusedSequential.fuse_pool and type(act) is nn.ReLU and _is_pool3(pool) and fusable(bn, y) and bn.track_running_stats
            and _lib.lib().cpg_bn_relu_pool3_supported(int(y.shape[2]), int(y.shape[3]))):
        args, training, nbt = _bn_args(bn)
        return _BnReluPool3Fn.apply(y, *args, stats if training else None, nbt)
    if stats is not None and type(act) is nn.ReLU and fusable(bn, y):
        return pool(bn_relu(y, bn, relu=True, stats=stats))
    return pool(bn_act(bn, act, y))


def bn_relu_pool(x, bn, stats=None, pool_max=None):
    """max_pool2d(relu(bn(x)), 2, 2) with `bn` an nn.BatchNorm2d module; H and W must be even.  `stats`: partial sums
    of x from the conv that produced it (SharableConv2d.forward_with_bn_stats); pool_max: that conv's window maxima (PoolMaxSink.E)."""
    args, training, nbt = _bn_args(bn)
    use = training and stats is not None
    return _BnReluPoolFn.apply(x, *args, stats if training else None, nbt, pool_max if use else None)


def fusable(bn, x):
    """An affine, stat-tracking (or eval-mode) BatchNorm2d on a 4-D fp32 HIP tensor with the default
    exponential-average momentum -- everything the CPG topologies construct."""
    return (isinstance(bn, nn.BatchNorm2d) and bn.affine and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and bn.momentum is not None and (bn.track_running_stats or bn.training))


def bn_relu(x, bn, relu=True, stats=None, hint=None):
    """y = relu(bn(x)) with `bn` an nn.BatchNorm2d module (its buffers are updated as torch would).  hint: a BnBwdHint when the
    caller hands y to exactly one masked 3x3 conv (FusedSequential does)."""
    args, training, nbt = _bn_args(bn)
    return _BnReluFn.apply(x, *args, relu, stats if (training and bn.track_running_stats) else None, hint if training else None, nbt)


class _PReluFn(torch.autograd.Function):
    """nn.PReLU (+ an optional residual added to its output: SphereNet's `x + relu(conv(y))`) as one forward pass (cpg_prelu_fwd)
    and a one-pass backward (cpg_prelu_bwd); the residual's gradient is the incoming gradient itself."""

    @staticmethod
    def forward(ctx, x, weight, res=None, bias_sink=None):
        ctx.bias_sink = bias_sink        # BiasGradSink of the biased conv that produced x (its only consumer is this PReLU)
        N, C = x.shape[0], x.shape[1]
        HW = x.numel() // max(N * C, 1)
        y = torch.empty_like(x)
        if x.numel():
            _lib.call('cpg_prelu_fwd', _lib.dptr(x, name='input'), _lib.dptr(res, name='residual'), _lib.dptr(weight, name='prelu.weight'),
                      _lib.dptr(y), N, C, HW, weight.numel(), _lib.stream_ptr())
        ctx.save_for_backward(x, weight)
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        sink, ctx.bias_sink = ctx.bias_sink, None
        if not x.numel():
            return torch.zeros_like(x), torch.zeros_like(weight), (gy if ctx.has_res else None), None
        N, C = x.shape[0], x.shape[1]
        HW = x.numel() // (N * C)
        ws, nb = _lib.workspace(_lib.lib().cpg_prelu_workspace_bytes(N, C, HW), x.device)
        gx = torch.empty_like(x)
        gw = torch.empty_like(weight)
        head = (_lib.dptr(x), _lib.dptr(gy), _lib.dptr(weight), _lib.dptr(gx), _lib.dptr(gw))
        tail = (N, C, HW, weight.numel(), _lib.dptr(ws), nb, _lib.stream_ptr())
        if sink is not None:
            gbias = torch.empty(C, dtype=torch.float32, device=x.device)
            _lib.call('cpg_prelu_bwd_bias', *head, _lib.dptr(gbias), *tail)
            sink.gb = gbias
        else:
            _lib.call('cpg_prelu_bwd', *head, *tail)
        return gx, gw, (gy if ctx.has_res else None), None


def _dense4d(t):
    return t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()


def _prelu_fits(mod, x, conv=None):
    """The eligibility that prelu, conv_prelu and conv_prelu_skip share: a plain nn.PReLU with one slope, or one per channel, on a HIP
    tensor; with `conv` (the masked conv in front of it) also that the pair runs under autograd, in fp32, as ONE conv call (a grouped
    conv runs one call per group: each computes its own bias gradient)."""
    return (ENABLED and type(mod) is nn.PReLU and x.is_cuda and mod.weight.numel() in (1, x.shape[1] if conv is None else conv.out_channels)
            and (conv is None or (torch.is_grad_enabled() and conv._math() == 'fp32' and getattr(conv, 'groups', 1) == 1)))


def _conv_prelu_eval(conv, mod, x, res=None):
    """Inference: mod(conv(x)) [+ res] as one kernel (FUSE_EVAL_PRELU, under torch.no_grad(), a conv that offers forward_prelu_eval), or
    None -- the method itself refuses what it has no kernel for."""
    if ENABLED and FUSE_EVAL_PRELU and not torch.is_grad_enabled() and hasattr(conv, 'forward_prelu_eval'):
        return conv.forward_prelu_eval(x, mod, res)
    return None


def conv_prelu(conv, mod, x, res=None):
    """mod(conv(x)) [+ res] for SphereNet's biased conv -> PReLU pairs (models/spherenet.py:203-247): the PReLU's backward pass also
    delivers the conv's bias gradient (the per-channel sum of the gradient it writes), so the conv's backward runs no bias reduction.
    Under torch.no_grad() the pair (and the residual) is one kernel where the conv has the epilogue (_conv_prelu_eval)."""
    y = _conv_prelu_eval(conv, mod, x, res)
    if y is not None:
        return y
    if getattr(conv, 'bias', None) is not None and _prelu_fits(mod, x, conv):
        sink = BiasGradSink()
        y = conv(x, bias_sink=sink)
        if _dense4d(y) and (res is None or (res.shape == y.shape and res.is_contiguous())):
            return _PReluFn.apply(y, mod.weight, res, sink)
        return prelu(mod, y, res)
    return prelu(mod, conv(x), res)


def conv_prelu_skip(conv, mod, x):
    """(mod(conv(x)), x) for the FIRST conv of a SphereNet residual unit (models/spherenet.py:121-131: `x = x + relu(conv(relu(conv(x))))`):
    x feeds this conv and the unit's sum.  The returned x is routed through the conv's autograd node, which then receives BOTH gradients
    of x and adds the sum's in its input-gradient epilogue (cpg_conv2d_dgrad_add: the two-wave Winograd kernel's ADD instances) instead of
    leaving a separate add kernel to autograd.  Falls back to (conv_prelu(conv, mod, x), x) when the pair does not qualify -- under
    torch.no_grad() that is the one-kernel inference pair."""
    y = _conv_prelu_eval(conv, mod, x)
    if y is not None:
        return y, x
    if x.requires_grad and _prelu_fits(mod, x, conv) and x.dim() == 4 and x.is_contiguous():
        sink = BiasGradSink() if getattr(conv, 'bias', None) is not None else None
        y, _, skip = conv.forward_with_skip(x, bias_sink=sink, want_stats=False)
        if _dense4d(y):                  # (a conv output: always 4-D)
            return _PReluFn.apply(y, mod.weight, None, sink), skip
        return prelu(mod, y), skip
    return conv_prelu(conv, mod, x), x


def prelu(mod, x, res=None):
    """mod(x) [+ res] for an nn.PReLU module (models/spherenet.py); HIP kernels when the tensor qualifies."""
    if (_dense4d(x) and _prelu_fits(mod, x)
            and (res is None or (res.shape == x.shape and res.is_contiguous() and res.dtype == torch.float32 and res.is_cuda))):
        return _PReluFn.apply(x, mod.weight, res)
    y = mod(x)
    return y if res is None else res + y


def bn_act(bn, act, x):
    """act(bn(x)) for the residual topologies (models/resnet.py: `self.relu(self.bn1(...))`, `self.bn3(...)`): one fused
    kernel pair when `act` is a plain nn.ReLU (or None) and `bn` qualifies, the stock modules otherwise."""
    if ENABLED and (act is None or type(act) is nn.ReLU) and fusable(bn, x):
        return bn_relu(x, bn, relu=act is not None)
    y = bn(x)
    return y if act is None else act(y)


def bn_add_act(bn, act, x, res, stats=None):
    """act(bn(x) + res), the tail of a residual block; fused when `act` is a plain nn.ReLU and `bn` qualifies.  stats: partial sums
    of x from the conv that produced it (conv_bn_add_act)."""
    if ENABLED and type(act) is nn.ReLU and fusable(bn, x) and bn.track_running_stats and res.shape == x.shape:
        args, training, nbt = _bn_args(bn)
        return _BnAddReluFn.apply(x, res, *args, stats if training else None, nbt)
    out = bn(x)
    out = out + res
    return act(out)


def _conv_with_stats(conv, bn, x):
    """(conv(x), partial sums for `bn` or None): the conv's epilogue accumulates the BatchNorm statistics when the pair qualifies
    (a masked conv with a fused-statistics kernel feeding a training-mode, stat-tracking BatchNorm2d)."""
    if ENABLED and hasattr(conv, 'forward_with_bn_stats') and _stats_from_conv(bn, FusedSequential.fuse_stats, x, need_grad=True):
        return conv.forward_with_bn_stats(x)
    return conv(x), None


def _eval_blocks(conv, bn, x, method='forward_bn_eval'):
    """Inference may run `conv` and `bn` as one kernel: FUSE_EVAL_BLOCKS, under torch.no_grad(), a conv that offers `method`, an
    eval-mode, affine, stat-tracking BatchNorm2d, fp32 on the device (the conv's own method still answers None for shapes without such
    a kernel and for another arithmetic)."""
    return (ENABLED and FUSE_EVAL_BLOCKS and not torch.is_grad_enabled() and hasattr(conv, method) and isinstance(bn, nn.BatchNorm2d)
            and not bn.training and bn.track_running_stats and bn.affine and x.is_cuda and x.dtype == torch.float32
            and bn.weight.dtype == torch.float32)


def conv_bn_act(conv, bn, act, x):
    """act(bn(conv(x))) for the residual topologies (models/resnet.py:86-93): bn_act with the statistics pass folded into the conv; at
    inference the whole triple is the conv's kernel (_eval_blocks)."""
    if (act is None or type(act) is nn.ReLU) and _eval_blocks(conv, bn, x):
        y = conv.forward_bn_eval(x, bn, relu=act is not None)
        if y is not None:
            return y
    y, stats = _conv_with_stats(conv, bn, x)
    if stats is not None and (act is None or type(act) is nn.ReLU) and fusable(bn, y):
        return bn_relu(y, bn, relu=act is not None, stats=stats)
    return bn_act(bn, act, y)


class _StemConvBnReluFn(torch.autograd.Function):
    """z = relu(bn(conv(x))) for the network stem (models/vgg.py:137-141) with the conv output recomputed in every pass that needs it
    instead of stored: forward = statistics pass + BatchNorm/ReLU pass over the image, backward = reduction pass + apply pass over gz
    (each recomputes conv(x)), then the stem's weight gradient from the resulting gy.  The image gets no gradient."""

    @staticmethod
    def forward(ctx, x, weight, pm, thr, gamma, beta, running_mean, running_var, eps, momentum, nbt=None):
        x = x.contiguous()
        w = weight.contiguous()
        p = None if pm is None else pm.contiguous()
        d = _conv_desc(x.shape, w.shape, (1, 1), (1, 1), (1, 1), 1)
        s = _lib.stream_ptr()
        thr = float(thr)
        N, K, H, W = x.shape[0], w.shape[0], x.shape[2], x.shape[3]
        tiles = _lib.lib().cpg_stem_bn_tiles(ctypes.byref(d))
        stats = torch.empty((K, tiles, 2), dtype=torch.float32, device=x.device)
        _lib.call('cpg_stem_bn_stats', ctypes.byref(d), _lib.dptr(x, name='input'), _lib.dptr(w, name='weight'), _lib.dptr(p, name='piggymask'),
                  thr, None, _lib.dptr(stats), stats.numel() * 4, s)
        mean, invstd, nbt = _batch_stats(stats, nbt, N, K, H * W, eps, momentum, running_mean, running_var, True, x.device)
        z = torch.empty((N, K, H, W), dtype=torch.float32, device=x.device)
        _lib.call('cpg_stem_bn_relu_fwd', ctypes.byref(d), _lib.dptr(x), _lib.dptr(w), _lib.dptr(p), thr, None, _lib.dptr(gamma, name='bn.weight'),
                  _lib.dptr(beta, name='bn.bias'), _lib.dptr(mean), _lib.dptr(invstd), _lib.dptr(z), s)
        _count(nbt)
        ctx.save_for_backward(x, w, p, gamma, beta, mean, invstd)
        ctx.desc, ctx.thr, ctx.tiles = d, thr, tiles
        return z

    @staticmethod
    def backward(ctx, gz):
        x, w, p, gamma, beta, mean, invstd = ctx.saved_tensors
        d, thr, tiles = ctx.desc, ctx.thr, ctx.tiles
        gz = gz.contiguous()
        L = _lib.lib()
        s = _lib.stream_ptr()
        N, K, H, W = x.shape[0], w.shape[0], x.shape[2], x.shape[3]
        partials = torch.empty((K, tiles, 2), dtype=torch.float32, device=x.device)
        args = (ctypes.byref(d), _lib.dptr(x), _lib.dptr(w), _lib.dptr(p), thr, None, _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(mean),
                _lib.dptr(invstd))
        _lib.call('cpg_stem_bn_relu_bwd_reduce', *args, _lib.dptr(gz, name='grad_output'), _lib.dptr(partials), partials.numel() * 4, s)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        coef = torch.empty(2 * K, dtype=torch.float32, device=x.device)
        _lib.call('cpg_bn_bwd_finalize_partials', _lib.dptr(partials), tiles, N, K, H * W, _lib.dptr(dgamma), _lib.dptr(dbeta), _lib.dptr(coef), s)
        gw = gpm = None
        if ctx.needs_input_grad[1] or (p is not None and ctx.needs_input_grad[2]):
            gw = torch.empty_like(w)
            gpm = None if p is None else torch.empty_like(p)
            if FUSE_STEM_WGRAD:
                # gy is contracted with the image patch in the pass that forms it (never written)
                ws, nbytes = _lib.workspace(L.cpg_stem_bn_wgrad_workspace(ctypes.byref(d)), x.device)
                _lib.call('cpg_stem_bn_relu_bwd_wgrad', *args, _lib.dptr(coef), _lib.dptr(gz), _lib.dptr(gw), _lib.dptr(gpm), _lib.dptr(ws),
                          nbytes, s)
            else:
                gy = torch.empty((N, K, H, W), dtype=torch.float32, device=x.device)
                _lib.call('cpg_stem_bn_relu_bwd_apply', *args, _lib.dptr(coef), _lib.dptr(gz), _lib.dptr(gy), s)
                ws, nbytes = _lib.workspace(L.cpg_conv2d_workspace_bytes(ctypes.byref(d)), x.device)
                _lib.call('cpg_conv2d_wgrad', ctypes.byref(d), _lib.dptr(x), _lib.dptr(gy), _lib.dptr(w), _lib.dptr(p), thr, _lib.dptr(gw),
                          _lib.dptr(gpm), None, _lib.dptr(ws), nbytes, s)
        return (None, gw, gpm, None, dgamma, dbeta) + (None,) * 5


def stem_conv_bn_relu(conv, bn, x):
    """relu(bn(conv(x))) through _StemConvBnReluFn when the triple qualifies (a bias-free masked 3x3 s1 p1 stem in fp32 feeding a
    training-mode, stat-tracking BatchNorm2d, an input that needs no gradient), else None."""
    if not (ENABLED and FUSE_STEM and FusedSequential.fuse and hasattr(conv, 'forward_with_bn_stats')
            and _stats_from_conv(bn, FusedSequential.fuse_stats, x, need_grad=True)
            and x.dim() == 4 and x.dtype == torch.float32 and not x.requires_grad
            and conv.bias is None and conv._math() == 'fp32' and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1)
            and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and x.shape[0] > 0
            and x.shape[1] == conv.weight.shape[1] and bn.weight.dtype == torch.float32):
        return None
    d = _conv_desc(x.shape, conv.weight.shape, (1, 1), (1, 1), (1, 1), 1)
    if not _lib.lib().cpg_stem_bn_supported(ctypes.byref(d)):
        return None
    return _StemConvBnReluFn.apply(x, conv.weight, conv.piggymask, conv.info['threshold'], bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                   bn.eps, bn.momentum, bn.num_batches_tracked)


def conv_bn_act_skip(conv, bn, act, x):
    """(act(bn(conv(x))), x for the block's second branch -- the identity or the downsample conv): conv_bn_act for the first conv of
    a residual block (models/resnet.py:84-104).  When the conv's input gradient can take an addend (dense 1x1 layers), x is routed
    through the conv's autograd node, which then receives both of x's gradients and sums them in its kernel's epilogue."""
    if (ENABLED and FUSE_SKIP_ADD and hasattr(conv, 'forward_with_skip') and x.is_cuda and torch.is_grad_enabled() and x.requires_grad
            and conv._math() == 'fp32' and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.in_channels % 16 == 0
            and conv.out_channels % 16 == 0):
        # (partial sums only for a BatchNorm that takes them: an eval-mode one normalises with its running statistics)
        y, stats, skip = conv.forward_with_skip(x, want_stats=bool(_stats_from_conv(bn, FusedSequential.fuse_stats)))
        if stats is not None and (act is None or type(act) is nn.ReLU) and fusable(bn, y):
            return bn_relu(y, bn, relu=act is not None, stats=stats), skip
        return bn_act(bn, act, y), skip
    return conv_bn_act(conv, bn, act, x), x


def conv_bn_add_act(conv, bn, act, x, res):
    """act(bn(conv(x)) + res): the block tail (models/resnet.py:94-104) with the statistics from the conv's epilogue; at inference
    the whole tail is the conv's kernel (_eval_blocks: the pointwise conv3 of a Bottleneck)."""
    if type(act) is nn.ReLU and _eval_blocks(conv, bn, x, 'forward_bn_eval_add'):
        y = conv.forward_bn_eval_add(x, bn, res, relu=True)
        if y is not None:
            return y
    y, stats = _conv_with_stats(conv, bn, x)
    return bn_add_act(bn, act, y, res, stats)


class FusedSequential(nn.Sequential):
    """nn.Sequential that runs BatchNorm2d -> ReLU (-> MaxPool2d(2, 2)) groups through the fused kernels.
    Module registration (names, parameters, buffers) is exactly nn.Sequential's."""

    fuse = True
    fuse_pool = True
    fuse_stats = True       # conv -> BatchNorm2d: the conv kernel's epilogue produces the batch-statistics partial sums
    fuse_eval = True        # inference: conv -> BatchNorm2d(eval) -> ReLU as one kernel (BatchNorm folded into the conv epilogue)
    # inference: conv -> BatchNorm2d(eval) -> ReLU -> MaxPool2d(2, 2) as one kernel (the pool window is the Winograd output tile; the
    # full-resolution activation is never written).  The measurement decides the default: profiles/vgg_eval_pool_fuse.md
    fuse_eval_pool = False
    skip_log = None         # diagnostics: set to a list to collect one int32[2] tensor per fused inference conv --
    #                         {4 * (4-channel input chunks up to the last live one), output blocks skipped by the dead-channel test}

    def forward(self, input):
        """Every step looks at the next four modules (None past the end) and at
            input   the activation so far,
            stats   its partial sums, when the module that produced it was asked for them,
            hint    the BnBwdHint for the conv that consumes it, when it came out of a fused BatchNorm -> ReLU,
        and either declines (None) or returns (modules consumed, input, stats, hint).  _conv takes whatever the others leave."""
        mods = list(self._modules.values())
        n = len(mods)
        mods += [None] * 3
        steps = (self._bn_relu, self._lone_bn, self._conv_bn_relu_pool_eval, self._conv_bn_relu_eval, self._conv_bn_eval, self._stem, self._conv_bn_relu_pool, self._conv)
        i, stats, hint = 0, None, None
        while i < n:
            window = mods[i:i + 4]
            for step in steps:
                done = step(window, input, stats, hint)
                if done is not None:
                    break
            k, input, stats, hint = done
            i += k
        return input

    def _bn_relu(self, mods, input, stats, hint):
        """BatchNorm2d -> ReLU, with the MaxPool2d(2, 2) behind them when the plane is even."""
        m, relu, nxt2, _ = mods
        if not (self.fuse and ENABLED and isinstance(m, nn.BatchNorm2d) and isinstance(relu, nn.ReLU) and fusable(m, input)):
            return None
        if self.fuse_pool and _is_pool2(nxt2) and input.shape[2] % 2 == 0 and input.shape[3] % 2 == 0 and m.track_running_stats:
            return 3, bn_relu_pool(input, m, stats), None, None
        # BatchNorm -> ReLU feeding a masked conv directly: let that conv's backward do part of this BatchNorm's backward
        # (only this Sequential knows that nothing else reads the activation)
        hint = BnBwdHint(ENABLE_BWD_HINT, ENABLE_WGRAD_RIDER) if (
            (ENABLE_BWD_HINT or ENABLE_WGRAD_RIDER) and m.training and torch.is_grad_enabled()
            and hasattr(nxt2, 'forward_with_bn_stats')) else None
        return 2, bn_relu(input, m, relu=True, stats=stats, hint=hint), None, hint

    def _lone_bn(self, mods, input, stats, hint):
        """A BatchNorm2d with no ReLU behind it (ResNet shortcut: conv1x1 -> BN)."""
        m = mods[0]
        if not (self.fuse and ENABLED and isinstance(m, nn.BatchNorm2d) and fusable(m, input)):
            return None
        return 1, bn_relu(input, m, relu=False, stats=stats), None, hint

    def _conv_bn_relu_pool_eval(self, mods, input, stats, hint):
        """Inference (fuse_eval_pool): conv -> BatchNorm2d(eval) -> ReLU -> MaxPool2d(2, 2) as one kernel that writes the pooled tensor
        alone.  Where the conv has no such kernel for this shape (forward_bn_eval_pool returns None) the steps below run exactly as
        without this one."""
        m, bn, relu, pool = mods
        if not (self.fuse_eval_pool and self.fuse and self.fuse_eval and self.fuse_pool and ENABLED and not torch.is_grad_enabled()
                and hasattr(m, 'forward_bn_eval_pool') and isinstance(bn, nn.BatchNorm2d) and not bn.training
                and bn.track_running_stats and bn.affine and isinstance(relu, nn.ReLU) and _is_pool2(pool) and input.is_cuda):
            return None
        st = None if self.skip_log is None else torch.zeros(2, dtype=torch.int32, device=input.device)
        y = m.forward_bn_eval_pool(input, bn, relu=True, skip_stats=st)
        if y is None:
            return None
        if st is not None:
            self.skip_log.append(st)
        return 4, y, None, None

    def _conv_bn_relu_eval(self, mods, input, stats, hint):
        """Inference: conv -> BatchNorm2d(eval) -> ReLU as one kernel.  (A following MaxPool2d(2, 2) is _conv_bn_relu_pool_eval's where that
        step takes it; otherwise it keeps the conv + fused BN/ReLU/pool pair.)"""
        m, bn, relu, nxt3 = mods
        if not (self.fuse and self.fuse_eval and ENABLED and not torch.is_grad_enabled() and hasattr(m, 'forward_bn_eval')
                and isinstance(bn, nn.BatchNorm2d) and not bn.training and bn.track_running_stats and bn.affine
                and isinstance(relu, nn.ReLU) and input.is_cuda and not (self.fuse_pool and _is_pool2(nxt3))):
            return None
        st = None if self.skip_log is None else torch.zeros(2, dtype=torch.int32, device=input.device)
        y = m.forward_bn_eval(input, bn, relu=True, skip_stats=st)
        if y is None:
            return None
        if st is not None:
            self.skip_log.append(st)
        return 3, y, None, hint

    def _conv_bn_eval(self, mods, input, stats, hint):
        """Inference: conv -> BatchNorm2d(eval) with NO ReLU behind it (the ResNet shortcut, conv1x1 -> BN) as one kernel.  A pair with
        a ReLU behind it is _conv_bn_relu_eval's, whether or not that step took it."""
        m, bn, nxt2, _ = mods
        if not (self.fuse and self.fuse_eval and not isinstance(nxt2, nn.ReLU) and _eval_blocks(m, bn, input)):
            return None
        y = m.forward_bn_eval(input, bn, relu=False)
        return None if y is None else (2, y, None, None)

    def _stem(self, mods, input, stats, hint):
        """The stem: conv -> BatchNorm2d -> ReLU without ever writing the conv output (a following MaxPool2d keeps the pair, as above)."""
        m, bn, relu, nxt3 = mods
        if not (self.fuse and FUSE_STEM and isinstance(bn, nn.BatchNorm2d) and type(relu) is nn.ReLU
                and hasattr(m, 'forward_with_bn_stats') and getattr(m, 'in_channels', 99) <= 3
                and not (self.fuse_pool and _is_pool2(nxt3))):
            return None
        z = stem_conv_bn_relu(m, bn, input)
        return None if z is None else (3, z, None, None)

    def _conv_bn_relu_pool(self, mods, input, stats, hint):
        """A masked conv in front of a training-mode BatchNorm2d -> ReLU -> MaxPool2d(2, 2): the conv is also asked for the maximum of
        every pool window of its output (PoolMaxSink), which the pooled BatchNorm passes then read instead of the output itself.  Where
        the conv cannot deliver them -- or the group behind it does not fuse -- this is _conv's step and the next one is _bn_relu's."""
        m, bn, relu, pool = mods
        if not (self.fuse and self.fuse_pool and ENABLED and hasattr(m, 'forward_with_bn_stats') and isinstance(relu, nn.ReLU)
                and _is_pool2(pool) and _stats_from_conv(bn, self.fuse_stats, input)):
            return None
        sink = PoolMaxSink()
        y, stats = m.forward_with_bn_stats(input, bn_hint=hint, pool_sink=sink)
        if sink.E is None or stats is None or not fusable(bn, y):
            return 1, y, stats, None
        return 4, bn_relu_pool(y, bn, stats, sink.E), None, None

    def _conv(self, mods, input, stats, hint):
        """Any other module; a masked conv in front of a training-mode BatchNorm2d also returns that BatchNorm's partial sums."""
        m, nxt = mods[0], mods[1]
        if self.fuse and ENABLED and hasattr(m, 'forward_with_bn_stats') and _stats_from_conv(nxt, self.fuse_stats, input):
            return (1,) + tuple(m.forward_with_bn_stats(input, bn_hint=hint)) + (None,)
        if hint is not None and hasattr(m, 'forward_with_bn_stats'):
            return 1, m(input, bn_hint=hint), None, None
        return 1, m(input), None, None
