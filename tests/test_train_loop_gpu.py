"""Short training loops of the ResNet pieces on the device, against float64 (tests/_train_loop.py: the loop driver, the plans, the
reference, its conditioning and the bound; tests/test_train_loop_host.py checks the reference alone).

Every other fp64 parity statement of the suite is one forward and one backward.  Here the library nets of tests/_autograd_ref.py and a
mini ResNet run plans P1 .. P5 (prune-mode steps with two rank-prune events, through torch's SGD and through MaskedSGD; a task-2 finetune
with piggymasks under MaskedAdam; steps / apply_mask / evaluation / steps; gradient accumulation), and at EVERY step logits, loss, every
gradient as backward left it and as the step consumed it, every update w_after - w_before, every momentum and Adam buffer, every
BatchNorm buffer and counter, every owner mask, the pruner's statistics and the prune ratio are compared with the float64 reference
that ran the same plan.  Per tensor: max|got - ref| <= b max|ref|, b = max(floor, 8 x stock fp32 torch's error on that tensor at that
step) with floor 1e-5 (for an update: 2^-23 max|w| / max|dw| where larger), never above 1e-4; running statistics rtol 1e-5 / atol 1e-6;
masks, counters, statistics and ratios exactly.  No element is masked out of a comparison.

A loop test whose fast path silently declined is worth nothing: each case says which entry points ran in which phase (the recorder of
tests/test_autograd_contract_gpu.py over _lib.call and the rider).

Measured on an MI355X, worst over the five plans, as a fraction of the tensor's largest entry, stock fp32 on the CPU in brackets:

    net          logits / loss       gradient            update              running statistics   bound at most
    A            1.1e-6 (5.8e-6)     1.5e-6 (1.3e-6)     1.1e-5 (1.1e-5)     0.10 of tolerance    8.8e-5
    B_identity   3.2e-7 (1.7e-7)     2.0e-6 (8.7e-7)     9.7e-6 (9.7e-6)     0.02                 7.8e-5
    B_down       2.1e-7 (1.5e-7)     9.0e-7 (3.7e-7)     7.3e-6 (7.3e-6)     0.03                 5.9e-5
    B_basic      2.7e-7 (2.6e-7)     6.4e-7 (1.5e-6)     7.3e-6 (7.3e-6)     0.02                 5.8e-5
    C            6.6e-7 (1.3e-6)     1.0e-6 (9.2e-7)     1.2e-5 (1.2e-5)     (no BatchNorm)       9.4e-5
    R            1.0e-6 (1.4e-6)     8.5e-6 (4.1e-6)     1.2e-5 (1.0e-5)     0.15                 9.6e-5

Momentum at most 8.4e-6 (R P3), Adam's moments 5.3e-6, the weights apply_mask leaves 3.4e-7; owner masks, counters, statistics and prune
ratios identical in all 30 cases.  An update's error is the rounding of the fp32 weight it is the difference of: the same for the
library and for stock fp32.  The whole file runs in 9 s.
"""
import pytest
import torch

import _train_loop as T
from test_autograd_contract_gpu import Probe

from cpg_amd.models import fused_bn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture
def probe(monkeypatch):
    return Probe(monkeypatch)


def _paths(topo, plan, p, layers):
    cfg = T.PLANS[plan]
    steps, fwd = cfg['steps'], cfg['steps'] * cfg['micro']
    # (one multi-tensor launch per parameter group that holds a covered weight)
    groups = 1 + sum(1 for k in T.GROUP_LR.get(topo, {}) if any((n + '.weight').startswith(k) for n in layers))
    # ---- the optimizer, the routing, the pruner
    if cfg['fused']:
        assert p.n('cpg_sgd_route_step_multi', 'step') == steps * groups and p.n('cpg_sgd_route_step') == 0
        assert p.n('cpg_route_grads') == 0
    else:
        assert p.n('cpg_route_grads', 'route') == steps * len(layers) and p.n('cpg_sgd_route_step_multi') == 0
    if cfg['mode'] == 'finetune':
        assert p.n('cpg_adam_route_step_multi', 'step') == steps and p.n('cpg_adam_route_step') == 0
        assert p.n('cpg_claim_free', 'setup') == len(layers) and p.n('cpg_rank_prune') == 0
    else:
        assert p.n('cpg_adam_route_step_multi') == 0 and p.n('cpg_claim_free') == 0
    if plan in ('P1', 'P2', 'P4'):
        assert p.n('cpg_rank_prune', 'prune') == 2 * len(layers)
        # the statistics' histogram: once, and again after each of the two events (cached on the mutation counter in between)
        assert p.n('cpg_mask_hist', 'stats') == 3 * len(layers)
    if plan == 'P5':
        assert p.n('cpg_rank_prune') == 0 and p.n('cpg_mask_hist', 'stats') == len(layers)
    assert p.n('cpg_apply_mask') == (len(layers) if plan == 'P4' else 0)
    # ---- the layers, per forward / backward
    f, b = (lambda name: p.n(name, 'forward')), (lambda name: p.n(name, 'backward'))
    if topo == 'A':
        assert f('cpg_stem_bn_stats') == fwd and b('cpg_stem_bn_relu_bwd_reduce') == fwd and b('cpg_stem_bn_relu_bwd_wgrad') == fwd
        assert f('cpg_conv2d_fwd_bnstats') == 2 * fwd and f('cpg_bn_relu_pool_fwd') == fwd and b('cpg_bn_relu_pool_bwd') == fwd
        assert p.rode('backward') == [True] * fwd and b('cpg_conv2d_wgrad_attach_bn_bwd') == fwd and b('cpg_bn_relu_bwd') == 0
        assert f('cpg_linear_fwd') == fwd and b('cpg_linear_wgrad') == fwd
    elif topo == 'C':
        assert b('cpg_prelu_bwd_bias') == 3 * fwd and b('cpg_prelu_bwd') == 0 and b('cpg_conv2d_dgrad_add') == fwd
    elif topo == 'R':
        # the stem (7x7 s2, statistics from its epilogue) and its pooled BatchNorm -> ReLU -> MaxPool2d(3, 2, 1) pair
        assert f('cpg_bn_relu_pool3_fwd') == fwd and b('cpg_bn_relu_pool3_bwd') == fwd
        assert f('cpg_conv2d_fwd_bnstats') == 12 * fwd and f('cpg_bn_relu_fwd_train') == 0
        assert f('cpg_bn_add_relu_fwd') == 3 * fwd and b('cpg_bn_add_relu_bwd') == 3 * fwd
        assert b('cpg_conv2d_dgrad_add') == 3 * fwd
    else:
        assert f('cpg_bn_add_relu_fwd') == fwd and b('cpg_bn_add_relu_bwd') == fwd
        assert f('cpg_conv2d_fwd_bnstats') == {'B_identity': 3, 'B_down': 4, 'B_basic': 2}[topo] * fwd
        assert b('cpg_conv2d_dgrad_add') == (0 if topo == 'B_basic' else fwd)          # (the Bottleneck's 1x1 conv1 takes the second branch's gradient)
    # ---- P4's evaluation: the inference epilogues, no training kernel
    if plan == 'P4':
        e = lambda name: p.n(name, 'eval')
        assert e('cpg_conv2d_fwd_bnstats') == 0 and e('cpg_bn_stats_finalize_count') == 0 and e('cpg_bn_relu_fwd_train') == 0
        if topo == 'C':
            # (FUSE_EVAL_PRELU is opt-in: the test switches it on for this case; the 3 -> 64 stride-2 conv has no such kernel)
            assert e('cpg_conv2d_fwd_prelu_eval') == 2 and e('cpg_prelu_fwd') == 1
        elif topo == 'A':
            # (the third conv's 14 x 14 x 128 map has no pooled inference kernel: its BatchNorm -> ReLU -> MaxPool2d runs as the pooled pass)
            assert e('cpg_conv2d_fwd_bn_eval') == 2 and e('cpg_conv2d_fwd_bn_eval_pool') + e('cpg_bn_relu_pool_fwd') == 1
        else:
            assert e('cpg_conv2d_fwd_bn_eval') >= 1 and e('cpg_conv2d_fwd_bn_eval_add') == (3 if topo == 'R' else 1 if topo != 'B_basic' else 0)


@pytest.mark.parametrize('topo,plan', T.CASES)
def test_loop_matches_fp64(topo, plan, probe, monkeypatch):
    if (topo, plan) == ('C', 'P4'):
        monkeypatch.setattr(fused_bn, 'FUSE_EVAL_PRELU', True)         # conv -> PReLU (+ residual) as one inference kernel: off by default
    seed = T.seed_of(topo, plan)
    data = T.make_data(topo, plan, seed)
    net = T.build_library(topo, T.build_reference(topo, plan, seed), DEV)
    got = T.run_loop(net, plan, data, DEV, torch.float32, mark=probe.mark)
    torch.cuda.synchronize()
    print('%s %s entry points per phase: %s; rider: %s' % (topo, plan, probe.summary(), probe.riders))
    bad, worst = T.compare(got, topo, plan, seed)
    for group, (e, n, step, e32, b) in sorted(worst.items()):
        print('FIGURE %s %s %s: worst %.3g of scale (%s, step %d; stock fp32 there %.3g, bound %.3g)' % (topo, plan, group, e, n, step, e32, b))
    _paths(topo, plan, probe, sorted(data['owners']))
    assert not bad, bad
