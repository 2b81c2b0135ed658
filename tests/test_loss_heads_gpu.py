"""Loss heads on the GPU (include/cpg_hip.h: cpg_softmax_xent_*, cpg_angle_head_*; cpg_amd/models/losses.py) against stock torch in fp64.

Accuracy measure: err(a, b) = max|a - b| / max|b|.  The arbiter is the fp64 CPU result of the stock code (F.cross_entropy; AngleLinear +
AngleLoss in double); the bar is max(4 * err(stock fp32 CPU result, fp64), 4 * 2^-23), both terms computed here on the same inputs: the
fp32 oracle's own distance is the bar, the factor 4 allows another summation order over 512- and 4 630-long sums
without admitting a wrong term, and the second term keeps the bar off zero on tiny shapes.  Where the fp64 result is identically zero
(one class: loss and gradient are 0) the fused result has to be exactly zero.  Every comparison prints its figures before it asserts.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu
# inputs, references, bars and the bodies of the shape tests: shared with tests/test_guard_bands_gpu.py
import _loss_cases as LC                        # noqa: E402
from _loss_cases import DEV, XENT_CASES, fused_angle, fused_xent, hold, stock_xent, sweep_inputs, xent_inputs    # noqa: E402


# ------------------------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize('B,C,weights', XENT_CASES)
def test_cross_entropy_shapes(B, C, weights):
    LC.cross_entropy_case(B, C, weights)


def test_cross_entropy_extreme_row_and_nan():
    z, t, w = xent_inputs(3, 65, 'none')
    z[1, :5] = torch.tensor([1e4, -1e4, 80.0, -80.0, 0.0])
    z[1, 5:] = 0.0
    t[1] = 2
    l64, g64 = stock_xent(z, t, w, torch.float64)
    l32, g32 = stock_xent(z, t, w, torch.float32)
    loss, grad, _, _ = fused_xent(z, t, w)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    hold('loss, extreme row', loss, l32, l64)
    hold('dlogits, extreme row', grad, g32, g64)
    z[0, 7] = float('nan')
    loss, _, _, _ = fused_xent(z, t, w)
    assert np.isnan(loss)


@pytest.mark.parametrize('weights', ['none', 'random'])
def test_cross_entropy_ignored_and_out_of_range_rows(weights):
    B, C = 6, 10
    z, t, w = xent_inputs(B, C, weights)
    t = torch.tensor([3, -100, 7, C, 0, 9])
    keep = torch.tensor([0, 2, 4, 5])
    l64, g64 = stock_xent(z[keep], t[keep], w, torch.float64)
    l32, g32 = stock_xent(z[keep], t[keep], w, torch.float32)
    loss, grad, correct, _ = fused_xent(z, t, w)
    hold('loss, ignored rows', loss, l32, l64)
    hold('dlogits, ignored rows', grad[keep.numpy()], g32, g64)
    assert not grad[[1, 3]].any()                                          # exactly zero rows
    assert correct == int((z[keep].argmax(1) == t[keep]).sum())


def test_non_fp32_tensors_raise_and_no_grad_runs_the_forward_only():
    from cpg_amd.models.losses import FusedAngleLoss, FusedCrossEntropyLoss
    from cpg_amd.models.spherenet import AngleLinear
    t = torch.tensor([1, 0, 2], device=DEV)
    with pytest.raises(TypeError, match='must be torch.float32'):
        FusedCrossEntropyLoss()(torch.zeros(3, 4, device=DEV, dtype=torch.float64), t)
    with pytest.raises(TypeError, match='must be torch.int64'):
        FusedCrossEntropyLoss()(torch.zeros(3, 4, device=DEV), t.int())
    with pytest.raises(TypeError, match='must be torch.float32'):
        FusedAngleLoss().head_loss(torch.ones(3, 16, device=DEV, dtype=torch.float16), AngleLinear(16, 10).to(DEV), t)
    z = torch.randn(3, 4, device=DEV, requires_grad=True)
    with torch.no_grad():
        loss = FusedCrossEntropyLoss()(z, t)
    assert not loss.requires_grad and loss.grad_fn is None
    torch.testing.assert_close(loss, F.cross_entropy(z.detach(), t), rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------ angular head
def test_angle_head_matches_reference_fixture():
    """tests/golden/angle_head.npz (6 x 16 -> 10), three consecutive calls, at the bars the host test holds the stock modules to.  The
    fixture's gx is the SUM of the three calls' input gradients (x.grad was not zeroed when it was made)."""
    from cpg_amd.models.losses import FusedAngleLoss
    from cpg_amd.models.spherenet import AngleLinear
    g = load_golden('angle_head')
    lin = AngleLinear(16, 10)
    lin.weight.data.copy_(torch.from_numpy(g['w']))
    lin = lin.to(DEV)
    x = torch.from_numpy(g['x']).to(DEV).requires_grad_(True)
    t = torch.from_numpy(g['t']).to(DEV)
    crit = FusedAngleLoss()
    for k in range(3):
        lin.zero_grad()
        loss = crit.head_loss(x, lin, t)
        loss.backward()
        print('call %d: loss %.8f fixture %.8f' % (k, float(loss.detach()), g['losses'][k]))
        assert abs(float(loss.detach()) - g['losses'][k]) < 1e-5
        np.testing.assert_allclose(lin.weight.grad.cpu().numpy(), g['gw'][k], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(x.grad.cpu().numpy(), g['gx'], rtol=1e-4, atol=1e-6)
    assert crit.it == 3


@pytest.mark.parametrize('it', [1, 3000])
@pytest.mark.parametrize('B,D,C', LC.ANGLE_SWEEP_SHAPES)
def test_angle_head_margin_sweep(B, D, C, it):
    LC.angle_head_margin_sweep(B, D, C, it)


# ------------------------------------------------------------------------------------------------------------ determinism, streams
def _bytes(*arrays):
    return [np.asarray(a).tobytes() for a in arrays]


def test_two_runs_and_a_side_stream_give_identical_bytes():
    z, t, w = xent_inputs(33, 257, 'random')
    x, wa, ta = sweep_inputs(64, 512, 200)
    first = _bytes(*fused_xent(z, t, w)) + _bytes(*fused_angle(x, wa, ta, 3000))
    again = _bytes(*fused_xent(z, t, w)) + _bytes(*fused_angle(x, wa, ta, 3000))
    assert first == again
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _bytes(*fused_xent(z, t, w)) + _bytes(*fused_angle(x, wa, ta, 3000))
    torch.cuda.current_stream().wait_stream(side)
    assert first == on_side


# ------------------------------------------------------------------------------------------------------------ through Manager
VGG_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']


class _Wrap(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.module = m

    def forward(self, x):
        return self.module(x)


def _one_step(monkeypatch, arch, dataset, ncls, batch, size, fused):
    """One Manager.train step of one batch (+ one validation batch where the task has a classifier output) from a fixed seed."""
    import cpg_amd.models as M
    import cpg_amd.utils.manager as mgr_mod
    from cpg_amd.driver import default_args
    from cpg_amd.models import layers as nl
    from cpg_amd.utils import Metric, Optimizers
    seen = {}

    class Recording(Metric):
        def update(self, val, num):
            seen.setdefault(self.name, []).append(float(val))
            super().update(val, num)
    monkeypatch.setattr(mgr_mod, 'Metric', Recording)

    torch.manual_seed(11)
    kw = dict(dataset_history=[], dataset2num_classes={}, network_width_multiplier=0.25, shared_layer_info={})
    net = M.spherenet20(**kw) if arch == 'spherenet20' else M.custom_vgg_cifar100(VGG_CFG, **kw)
    net.add_dataset(dataset, ncls)
    net.set_dataset(dataset)
    model = _Wrap(net.to(DEV))
    masks = {n: torch.ones(m.weight.shape, dtype=torch.uint8, device=DEV) for n, m in model.named_modules()
             if isinstance(m, (nl.SharableConv2d, nl.SharableLinear))}
    g = torch.Generator().manual_seed(5)
    data = torch.randn(batch, 3, size, size, generator=g).to(DEV)
    target = torch.randint(0, ncls, (batch,), generator=g).to(DEV)
    args = default_args(mode='finetune', dataset=dataset, network_width_multiplier=0.25, fused_loss=fused)
    mgr = mgr_mod.Manager(args, model, {}, masks, [(data, target)], [(data, target)], 0, 1)
    opts = Optimizers()
    opts.add(torch.optim.SGD(list(model.parameters()), lr=1e-3, momentum=0.9, nesterov=True), 1e-3)
    train_acc, _ = mgr.train(opts, 0, [1e-3], 0)
    out = types.SimpleNamespace(loss=seen['train_loss'][0], train_acc=train_acc, it=getattr(mgr.criterion, 'it', None),
                                grads={n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters() if p.grad is not None},
                                val_acc=None if dataset == 'face_verification' else mgr.validate(0))
    return out


@pytest.mark.parametrize('arch,dataset,ncls,batch,size', [('spherenet20', 'face_verification', 10, 4, 112),
                                                          ('custom_vgg_cifar100', 't1', 10, 8, 32),
                                                          ('custom_vgg_cifar100', 'emotion', 7, 8, 32)])
def test_manager_step_with_and_without_fused_loss(monkeypatch, arch, dataset, ncls, batch, size):
    """Loss, accuracy and every parameter gradient of one train step agree at 1e-4 of each tensor's maximum (the project's gradient bar);
    the criterion's iteration count advanced once in both; validate returns the same accuracy.  The face task has no classifier
    accuracy in train (the reference computes none) and its evaluation is evalLFW, not validate, so there the accuracies compared are
    train's (undefined, 0 / 0, in both).  Owner masks are not compared after a training step."""
    off = _one_step(monkeypatch, arch, dataset, ncls, batch, size, fused=False)
    on = _one_step(monkeypatch, arch, dataset, ncls, batch, size, fused=True)
    print('loss off %.8f on %.8f' % (off.loss, on.loss))
    assert abs(on.loss - off.loss) <= 1e-4 * abs(off.loss)
    assert on.train_acc == off.train_acc or (np.isnan(on.train_acc) and np.isnan(off.train_acc) and dataset == 'face_verification')
    assert on.val_acc == off.val_acc
    assert on.it == off.it == (1 if dataset == 'face_verification' else None)
    assert set(on.grads) == set(off.grads) and on.grads
    worst = 0.0
    for n, ref in off.grads.items():
        scale = np.abs(ref).max()
        worst = max(worst, np.abs(on.grads[n] - ref).max() / scale if scale > 0 else float(np.abs(on.grads[n]).max() > 0))
        np.testing.assert_allclose(on.grads[n], ref, rtol=0, atol=1e-4 * scale, err_msg=n)
    print('worst gradient distance / max', worst)
