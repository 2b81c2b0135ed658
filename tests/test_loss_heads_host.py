"""Host-side contract of the loss heads (no GPU needed: every call here returns or raises before anything is launched)."""
import os
import re

import pytest
import torch

from conftest import ROOT

import cpg_amd._lib as L

ENTRY_POINTS = ('cpg_loss_heads_workspace_bytes', 'cpg_softmax_xent_fwd', 'cpg_softmax_xent_fwd_bwd', 'cpg_angle_head_fwd',
                'cpg_angle_head_bwd')


def test_fused_loss_is_off_by_default():
    from cpg_amd.driver import CPGSession, default_args
    assert default_args().fused_loss is False
    assert default_args(fused_loss=True).fused_loss is True
    import inspect
    assert inspect.signature(CPGSession.__init__).parameters['fused_loss'].default is False


def test_manager_picks_the_criterion_by_the_flag():
    """Off (and absent): the stock modules, exactly as before.  On: the fused ones, which are the stock AngleLoss's subclass and carry the
    emotion task's weights."""
    import types
    import torch.nn as nn
    from cpg_amd.models.losses import FusedAngleLoss, FusedCrossEntropyLoss
    from cpg_amd.models.spherenet import AngleLoss
    from cpg_amd.utils.manager import make_criterion

    def criterion(dataset, **flag):
        return make_criterion(types.SimpleNamespace(dataset=dataset, cuda=False, **flag))
    for flag in ({}, {'fused_loss': False}):
        assert type(criterion('face_verification', **flag)) is AngleLoss
        assert type(criterion('t1', **flag)) is nn.CrossEntropyLoss
        assert type(criterion('emotion', **flag)) is nn.CrossEntropyLoss
    assert type(criterion('face_verification', fused_loss=True)) is FusedAngleLoss
    assert type(criterion('t1', fused_loss=True)) is FusedCrossEntropyLoss
    emo = criterion('emotion', fused_loss=True)
    assert type(emo) is FusedCrossEntropyLoss and emo.weight.shape == (7,)
    torch.testing.assert_close(emo.weight, criterion('emotion').weight)


def test_cpu_tensors_raise():
    from cpg_amd.models.losses import FusedAngleLoss, FusedCrossEntropyLoss
    from cpg_amd.models.spherenet import AngleLinear
    t = torch.tensor([1, 0, 2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FusedCrossEntropyLoss()(torch.zeros(3, 4), t)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FusedCrossEntropyLoss(weight=torch.ones(4))(torch.zeros(3, 4), t)
    crit = FusedAngleLoss()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        crit.head_loss(torch.ones(3, 16), AngleLinear(16, 10), t)
    assert crit.it == 0                                      # a refused call does not advance the schedule


def test_other_margins_fall_back_to_the_stock_modules_and_the_library_refuses_them():
    """gamma != 0 or m != 4: head_loss IS the stock pair of modules (which run on any device), and the C entry points answer
    CPG_E_INVALID before they look at a pointer."""
    from cpg_amd.models.losses import FusedAngleLoss
    from cpg_amd.models.spherenet import AngleLinear, AngleLoss
    torch.manual_seed(3)
    x, t = torch.randn(5, 16), torch.tensor([1, 0, 2, 9, 4])
    for gamma, m in ((2, 4), (0, 3), (1, 2)):
        lin = AngleLinear(16, 10, m=m)
        fused, stock = FusedAngleLoss(gamma), AngleLoss(gamma)
        for _ in range(2):
            assert torch.equal(fused.head_loss(x, lin, t), stock(lin(x), t))
        assert fused.it == stock.it == 2 and fused.lamb == stock.lamb
    # called with AngleLinear's tuple the fused module is its parent
    lin = AngleLinear(16, 10)
    assert torch.equal(FusedAngleLoss()(lin(x), t), AngleLoss()(lin(x), t))
    lib = L.lib()
    for m, gamma in ((3, 0.0), (4, 1.0), (2, 2.0)):
        assert lib.cpg_angle_head_fwd(None, None, None, 4, 16, 10, m, gamma, 1500.0, *([None] * 7), 0, None) == L.CPG_E_INVALID
        assert b'only m = 4 and gamma = 0' in lib.cpg_last_error()
        assert lib.cpg_angle_head_bwd(*([None] * 7), 4, 16, 10, m, gamma, 1500.0, None, None, None, 0, None) == L.CPG_E_INVALID
    # ... and the supported margin with null tensors or a missing workspace is refused too, before any launch
    assert lib.cpg_angle_head_fwd(None, None, None, 4, 16, 10, 4, 0.0, 1500.0, *([None] * 7), 0, None) == L.CPG_E_INVALID
    assert lib.cpg_softmax_xent_fwd(None, None, None, 4, 10, None, None, None, 0, None) == L.CPG_E_INVALID
    assert lib.cpg_softmax_xent_fwd_bwd(None, None, None, None, 4, 10, None, None, None, None, 0, None) == L.CPG_E_INVALID


def test_workspace_query():
    lib = L.lib()
    assert lib.cpg_loss_heads_workspace_bytes(0, 0, 10) == 0 and lib.cpg_loss_heads_workspace_bytes(4, 0, 0) == 0
    xent = lib.cpg_loss_heads_workspace_bytes(256, 0, 4630)
    head = lib.cpg_loss_heads_workspace_bytes(256, 512, 4630)
    assert xent >= 256 * 2 * 4                               # per-row partial results
    # the head also holds df [B][C], the column partial sums and the linear kernels' workspace
    assert head >= xent + 256 * 4630 * 4 + 4630 * 4 + lib.cpg_linear_workspace_bytes(256, 4630, 512)


def test_entry_points_are_bound_and_documented():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    header = open(os.path.join(ROOT, 'include', 'cpg_hip.h')).read()
    for name in ENTRY_POINTS:
        assert name in L.EXPORTS
        assert re.search(r'^\| `%s` ' % name, text, re.M), name
        assert re.search(r'\b%s\(' % name, header), name
    assert 'models/spherenet.py:24-61' in header and 'utils/manager.py:29-36' in header          # the reference lines they replace
