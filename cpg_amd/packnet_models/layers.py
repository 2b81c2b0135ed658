"""Plain (unmasked) operators of the PackNet baseline stack on the C-ABI kernels.

The reference's packnet_models build their trunks from stock nn.Conv2d / nn.Linear and tell prunable layers apart with
`isinstance(module, nn.Conv2d) or isinstance(module, nn.Linear)` (utils/packnet_prune.py:72,90,...).  These classes ARE nn.Conv2d /
nn.Linear -- constructor, parameters, state_dict keys and seeded initialisation are torch's -- and only their forward / backward run the
library's convolution and GEMM kernels, with no piggymask (the kernels' `pm == NULL` form, as models.layers.HeadLinear for one layer).
They offer the hooks FusedSequential and the residual-block helpers look for (`forward_with_bn_stats`, `forward_with_skip`,
`forward_bn_eval`, `forward_bn_eval_pool`, `forward_bn_eval_add`, `forward_prelu_eval`, and `_forward_eval`, the frame those four share), so the baselines get the fused BatchNorm, stem, skip-add and inference paths of the CPG models.  fp32, HIP tensors only: no CPU fallback.
"""
import types

import torch.nn as nn

from ..models import layers as nl


class PlainConv2d(nn.Conv2d):
    # what SharableConv2d's methods below and fused_bn read besides nn.Conv2d's own attributes: no mask, threshold unused (read-only)
    piggymask = None
    info = types.MappingProxyType({'threshold': 0.0})

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if self.padding_mode != 'zeros' or isinstance(self.padding, str):
            raise NotImplementedError('PlainConv2d: only zero padding given as numbers')

    def _math(self):
        return 'fp32'

    def forward(self, input, bn_hint=None, bias_sink=None):
        if self.groups != 1:             # all groups in one launch per pass (no statistics epilogue, hint or sink on that route)
            bn_hint = bias_sink = None
        return nl._MaskedConv2dFn.apply(input, self.weight, None, self.bias, 0.0, self.stride, self.padding, self.dilation, self.groups,
                                        False, 'fp32', bn_hint, bias_sink)

    forward_with_bn_stats = nl.SharableConv2d.forward_with_bn_stats
    forward_with_skip = nl.SharableConv2d.forward_with_skip      # (residual blocks: fused_bn.conv_bn_act_skip / conv_prelu_skip)
    _forward_eval = nl.SharableConv2d._forward_eval                  # (the frame of the four inference methods below)
    forward_bn_eval = nl.SharableConv2d.forward_bn_eval
    forward_bn_eval_pool = nl.SharableConv2d.forward_bn_eval_pool    # (the conv in front of a MaxPool2d(2, 2) at inference: FusedSequential)
    forward_bn_eval_add = nl.SharableConv2d.forward_bn_eval_add      # (the Bottleneck tail at inference: fused_bn.conv_bn_add_act)
    forward_prelu_eval = nl.SharableConv2d.forward_prelu_eval        # (SphereNet's conv -> PReLU [-> + residual] at inference: fused_bn.conv_prelu)


class PlainLinear(nn.Linear):
    def forward(self, input):
        return nl._MaskedLinearFn.apply(input, self.weight, None, self.bias, 0.0)
