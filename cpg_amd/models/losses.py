"""Loss heads on the HIP library (include/cpg_hip.h: cpg_softmax_xent_*, cpg_angle_head_*): the step from the network's output to the
loss, the accuracy and the gradient that starts the backward pass.  OPT-IN (args.fused_loss of utils/manager.py); the stock modules
(nn.CrossEntropyLoss, models/spherenet.py AngleLinear + AngleLoss) stay the default.

FusedCrossEntropyLoss restates nn.CrossEntropyLoss(weight) with its mean reduction and keeps the batch's correct count (what
classification_accuracy would count) as a device tensor.  FusedAngleLoss is AngleLoss with a second entry, head_loss, that takes the
embeddings and the AngleLinear module and evaluates phi(theta) in the target column only.  As everywhere in the package there is no
CPU fallback: a CPU or non-fp32 tensor raises.
"""
import torch
import torch.nn as nn

from .. import _lib
from .spherenet import AngleLoss

__all__ = ['FusedCrossEntropyLoss', 'FusedAngleLoss']


def _target_ptr(target, rows):
    if target.dim() != 1 or target.shape[0] != rows:
        raise RuntimeError('fused loss: target must be one class index per row, got %s for %d rows' % (tuple(target.shape), rows))
    return _lib.dptr(target.contiguous(), torch.int64, name='target')


def _scalar(device):
    return torch.empty((), dtype=torch.float32, device=device)


def _grad_ptr(g):
    """The upstream gradient of the loss as a device scalar."""
    return _lib.dptr(g.reshape(1).contiguous(), name='grad_output')


class _SoftmaxXentFn(torch.autograd.Function):
    """(loss, correct) of logits [B][C]; backward is the row pass once more, gradient only (loss and count are not formed again)."""

    @staticmethod
    def forward(ctx, logits, target, weight):
        if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
            raise RuntimeError('FusedCrossEntropyLoss: logits must be [rows >= 1][classes >= 1], got %s' % (tuple(logits.shape),))
        z = logits.contiguous()
        t = target.contiguous()
        B, C = z.shape
        if weight is not None and weight.shape != (C,):
            raise RuntimeError('FusedCrossEntropyLoss: weight must hold one value per class (%d), got %s' % (C, tuple(weight.shape)))
        zp, tp, wp = _lib.dptr(z, name='logits'), _target_ptr(t, B), _lib.dptr(weight, name='class weight')
        loss, correct = _scalar(z.device), _scalar(z.device)
        ws, nbytes = _lib.workspace(_lib.lib().cpg_loss_heads_workspace_bytes(B, 0, C), z.device)
        _lib.call('cpg_softmax_xent_fwd', zp, tp, wp, B, C, _lib.dptr(loss), _lib.dptr(correct), _lib.dptr(ws), nbytes, _lib.stream_ptr())
        ctx.save_for_backward(z, t, weight)
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, gloss, _gcorrect):
        z, t, weight = ctx.saved_tensors
        B, C = z.shape
        dz = torch.empty_like(z)
        ws, nbytes = _lib.workspace(_lib.lib().cpg_loss_heads_workspace_bytes(B, 0, C), z.device)
        _lib.call('cpg_softmax_xent_fwd_bwd', _lib.dptr(z), _lib.dptr(t, torch.int64), _lib.dptr(weight), _grad_ptr(gloss), B, C,
                  None, None, _lib.dptr(dz), _lib.dptr(ws), nbytes, _lib.stream_ptr())
        return dz, None, None


class FusedCrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight=weight) (mean reduction; targets outside [0, C), ignore_index = -100 included, count with weight 0).
    After a call `correct` is the number of rows whose first maximum is the target and `accuracy` that count over the rows of the batch
    -- classification_accuracy's value -- both on the device."""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer('weight', None if weight is None else weight.detach().clone().contiguous())
        self.correct = None
        self.accuracy = None

    def forward(self, logits, target):
        loss, correct = _SoftmaxXentFn.apply(logits, target, self.weight)
        self.correct = correct
        self.accuracy = correct / logits.shape[0]
        return loss


class _AngleHeadFn(torch.autograd.Function):
    """(loss, correct) of embeddings x [B][D] against AngleLinear's weight [D][C], m = 4, gamma = 0, at the given lambda."""

    @staticmethod
    def forward(ctx, x, weight, target, lamb):
        if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[0] or x.shape[0] < 1:
            raise RuntimeError('FusedAngleLoss: embeddings %s do not match weight %s' % (tuple(x.shape), tuple(weight.shape)))
        x2, w, t = x.contiguous(), weight.contiguous(), target.contiguous()
        (B, D), C = x2.shape, w.shape[1]
        xp, wp, tp = _lib.dptr(x2, name='embeddings'), _lib.dptr(w, name='weight'), _target_ptr(t, B)
        dev = x2.device
        what = torch.empty_like(w)
        colnorm = torch.empty(C, dtype=torch.float32, device=dev)
        f = torch.empty((B, C), dtype=torch.float32, device=dev)
        saved = torch.empty((B, 4), dtype=torch.float32, device=dev)
        loss, correct = _scalar(dev), _scalar(dev)
        ws, nbytes = _lib.workspace(_lib.lib().cpg_loss_heads_workspace_bytes(B, D, C), dev)
        _lib.call('cpg_angle_head_fwd', xp, wp, tp, B, D, C, 4, 0.0, float(lamb), _lib.dptr(what), _lib.dptr(colnorm), _lib.dptr(f),
                  _lib.dptr(saved), _lib.dptr(loss), _lib.dptr(correct), _lib.dptr(ws), nbytes, _lib.stream_ptr())
        ctx.save_for_backward(x2, what, colnorm, f, saved, t)
        ctx.lamb = float(lamb)
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, gloss, _gcorrect):
        x2, what, colnorm, f, saved, t = ctx.saved_tensors
        (B, D), C = x2.shape, what.shape[1]
        gx, gw = torch.empty_like(x2), torch.empty_like(what)
        ws, nbytes = _lib.workspace(_lib.lib().cpg_loss_heads_workspace_bytes(B, D, C), x2.device)
        _lib.call('cpg_angle_head_bwd', _lib.dptr(x2), _lib.dptr(what), _lib.dptr(colnorm), _lib.dptr(f), _lib.dptr(saved),
                  _lib.dptr(t, torch.int64), _grad_ptr(gloss), B, D, C, 4, 0.0, ctx.lamb, _lib.dptr(gx), _lib.dptr(gw), _lib.dptr(ws), nbytes,
                  _lib.stream_ptr())
        return gx, gw, None, None


class FusedAngleLoss(AngleLoss):
    """AngleLoss (same `it`, `lamb`, `LambdaMin`, `LambdaMax` and advance rule; called with AngleLinear's (cos, phi) tuple it IS the
    parent) plus head_loss, which replaces `criterion(angle_linear(embeddings), target)` by the fused kernels.  The fused path is m = 4
    and gamma = 0; any other head or loss takes the stock modules."""

    def __init__(self, gamma=0):
        super().__init__(gamma)
        self.correct = None

    def head_loss(self, embeddings, angle_linear, target):
        if self.gamma != 0 or angle_linear.m != 4:
            return self(angle_linear(embeddings), target)
        it = self.it + 1
        lamb = max(self.LambdaMin, self.LambdaMax / (1 + 0.1 * it))
        loss, self.correct = _AngleHeadFn.apply(embeddings, angle_linear.weight, target, lamb)
        self.it, self.lamb = it, lamb
        return loss
