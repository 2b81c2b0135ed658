"""The reference of tests/test_train_loop_gpu.py, checked on the CPU (tests/_train_loop.py: the loop driver, the plans, the bound).

For every (topology, plan) of the seed table:

  * the float64 trajectory is well conditioned.  Every ReLU / PReLU input, every pool window's gap between its two largest values, every
    |piggymask - threshold| and, at a prune event, every candidate |weight|'s distance from the cutoff weight is at least 16 times
    what the stock float32 run of the same net is off by ON THAT SAME ELEMENT, at every layer and step.  The statement is per element
    because the layer-wide form (a layer's smallest margin against the layer's largest error) cannot be met by seeds: with the settings
    below, 21 to 26 of the mini ResNet's 44 layer-steps (activations and pool gaps of plan P1; smallest margin 8e-8 .. 9e-6, largest
    error 2e-5 .. 6e-5) miss it at seeds 0, 1, 2 and at the table's 669, 11 to 14 of 16 on topology A, 2 or 3 of 12 on B_identity; only
    B_basic (8 layer-steps of 4096 activations) meets it.  The layer's smallest margin, its largest error and the per-element ratio are
    printed per layer and step;
  * the bound is not vacuous: b = max(floor, 8 x stock fp32's error) <= 1e-4 for every floating-point tensor of every step, and the stock
    float32 run itself is inside it, with masks, counters, statistics and prune ratios identical to the float64 run's.  The running
    statistics have a fixed tolerance (rtol 1e-5, atol 1e-6) instead: there the seed leaves room, stock fp32 within a quarter of it;
  * the harness sees what it is for: the float64 reference run with ONE deliberately wrong statement (a conv's forward on last step's
    weights, a BatchNorm that skips one running-statistics update, the momentum buffers dropped for one step, a prune event skipped,
    apply_mask left out before the evaluation, the second micro-batch's gradient overwriting the first) is reported as a miss of at
    least ten times the bound, at that step or a later one and never before.  CPU runs of reference code: nothing is injected into the
    library.

What had to be chosen for the reference to meet these conditions (SGD at 0.05 everywhere and Adam's default eps do not):

  * an update is the difference of two fp32 weights, so it cannot be known better than 2^-23 max|w| / max|dw|, and stock fp32's own
    update error is that rounding (a third of it or so); b <= 1e-4 then asks for max|dw| >= 3e-3 max|w| or so from EVERY tensor.  BatchNorm weights (up to 1.5)
    with gradients of 0.02 need a rate of 0.1 or more: 0.2 on the one-block nets B_* (upd:block.bn2.weight was at 2.6e-4 with 0.05);
    0.08 on R (upd:layer3.bn2.weight was at 1.6e-4 with 0.05; at 0.1 stock fp32's gradients are off by 2e-5 at the last step).
  * A (three samples, a 6272-wide linear layer) at 0.05 sends its loss to 200 in one step, and the running mean of its last BatchNorm
    then separates by a factor of four per step: stock fp32 at 0.8 to 1.05 of the statistics' tolerance by the fourth step.  Rate 0.025
    and the linear layer (seq.11) at half of it: stock fp32 at 0.1 to 0.2 of the tolerance, every bound still <= 1e-4.
  * C (no BatchNorm, three samples, a 12 544-wide head) fits its batch within two steps at any rate above 0.005, and the gradient of a
    loss of 1e-5 is all cancellation (stock fp32 off by 100 %).  Rate 0.004, the head's weight at 0.01 of it, the head's bias at 0.2 of
    it (upd:head.bias), conv1.weight (largest weight 1.24) at twice it (upd:conv1.weight was at 1.7e-4): parameter groups, which
    MaskedSGD then has to honour as well.
  * Adam with torch's eps = 1e-8 steps by lr m / sqrt(v) whatever the gradient's size, so an element whose gradient is 1e-4 of the
    tensor's largest carries 1e4 times its share of the round-off: stock fp32's own piggymask update was off by 9e-2 of its scale on A
    and 2.6e-2 on R.  eps = 1e-2, the size of the piggymask gradients (0.01 .. 0.18), makes the update a smooth function of the moments;
    sqrt(v) and eps then both count in the denominator.  (upd:*.piggymask, all topologies.)
  * every plan has four steps (P5: four micro-batches, two steps): each further step costs R 1.2e5 more activations that must all stay
    clear of their kinks.  The seeds: 0 or 1 on the one-block nets; up to 868 on A and 669 on R, whose prune plans need every activation,
    every pool window and every candidate weight of 4 to 12 layers clear at once (about one seed in 500).
"""
import copy

import pytest
import torch

import _train_loop as T

FAULTS = [('stale_conv', 'P2', 1), ('skip_bn_stats', 'P2', 1), ('drop_momentum', 'P1', 2), ('skip_prune', 'P1', 1),
          ('no_apply_mask', 'P4', 1), ('overwrite_accum', 'P5', 0)]
FAULT_CASES = [(t,) + f for t in T.TOPOLOGIES for f in FAULTS if not (t == 'C' and f[0] == 'skip_bn_stats')]      # (C has no BatchNorm)


@pytest.mark.parametrize('topo,plan', T.CASES)
def test_reference_is_conditioned_and_its_bound_tight(topo, plan):
    seed = T.seed_of(topo, plan)
    wrong = T.check_reference(topo, plan, seed, log=print)
    r64, r32, cond = T.reference(topo, plan, seed)
    tight = min(cond, key=lambda c: c[3])
    top = max((b, n, s) for s, bs in enumerate(T.bounds(topo, plan, seed)) for n, b in bs.items())
    print('%s %s seed %d: %d quantities; tightest %s: margin / own fp32 error %.3g (smallest margin %.3g, largest error %.3g); largest bound %.3g '
          '(%s, step %d)' % (topo, plan, seed, len(cond), tight[0], tight[3], tight[1], tight[2], top[0], top[1], top[2]))
    assert not wrong, wrong
    cfg = T.PLANS[plan]
    assert len(r64) == cfg['steps'] and len(cond) >= cfg['steps'] * cfg['micro'] * 2
    masks = [{n: v for n, v in r.items() if n.startswith('mask:')} for r in r64]
    changed = [s for s in range(1, len(masks)) if any(not torch.equal(masks[s][n], masks[s - 1][n]) for n in masks[s])]
    if plan in ('P1', 'P2', 'P4'):
        # two rank-prune events, after the second and the third step, and steps that train with what they left
        assert changed == [1, 2] and [r['ratio'] for r in r64] == [0.0, 0.2625, 0.3, 0.3]
        assert all(any('_prune:' in n for n in r64[s]) for s in (1, 2))
        assert 0.25 < r64[1]['stat:sparsity'] < 0.27 and 0.29 < r64[3]['stat:sparsity'] < 0.40 and r64[0]['stat:sparsity'] == 0.0
        # (the second event ranks the released weights too, which momentum has moved on: more than 30 % can end up released)
    else:
        assert changed == [] and all(r.get('ratio', 0.0) == 0.0 for r in r64) and ('ratio' in r64[0]) == (plan == 'P5')
    if plan == 'P3':
        # owners 1 and 2 (the claimed free slots), a piggymask on every covered layer, some of them crossing the threshold on the way
        assert all(set(v.unique().tolist()) == {1, 2} for v in masks[0].values())
        pms = [n for n in r64[0] if n.startswith('_pm:')]
        assert len(pms) == len(masks[0]) and all('adam_v:' + n[4:] in r64[0] for n in pms)
        flips = sum(int(((r64[0][n] > T.R.THR) != (r64[-1][n] > T.R.THR)).sum()) for n in pms)
        print('%s P3: %d piggymask entries change sides of the threshold between the first and the last forward' % (topo, flips))
        assert flips > 0 and 0.0 < r64[0]['stat:shared_part_ratio'] < 1.0
    if plan == 'P4':
        zeroed = sum(int((r64[1][n] == 0).sum()) for n in r64[1] if n.startswith('applied:'))
        assert zeroed > 0 and 'eval:out' in r64[1] and 'eval:out' not in r64[0]
        for n, b in r64[1].items():                         # the evaluation left the statistics alone
            if n.startswith('buf:') and n.endswith('num_batches_tracked'):
                assert int(b) == 2
    if plan == 'P5':
        assert 'micro1:out' in r64[0] and 'micro1:loss' in r64[1]
        assert all(int(b) == 4 for n, b in r64[1].items() if n.endswith('num_batches_tracked'))


@pytest.mark.parametrize('topo,kind,plan,step', FAULT_CASES)
def test_wrong_reference_is_reported(topo, kind, plan, step):
    seed = T.seed_of(topo, plan)
    net = copy.deepcopy(T.build_reference(topo, plan, seed)).double()
    got = T.run_loop(net, plan, T.make_data(topo, plan, seed), 'cpu', torch.float64, fault=(kind, step))
    bad, _ = T.compare(got, topo, plan, seed, log=lambda *a: None)
    finite = [(s, n, x) for s, n, x, _ in bad if x != float('inf')]
    worst = max(finite, key=lambda m: m[2]) if finite else None
    print('%s %s %s at step %d: %d misses, first at step %s, worst %s' % (topo, plan, kind, step, len(bad), min(s for s, _, _, _ in bad) if bad else None, worst))
    assert bad and min(s for s, _, _, _ in bad) >= step
    assert worst is not None and worst[2] >= 10.0


def test_compare_reports_exact_things_exactly():
    """compare() itself: the float64 run against itself is clean; one owner byte, one counter, a statistic, the prune ratio and a
    missing gradient are each reported, at their step."""
    topo, plan = 'B_basic', 'P2'
    seed = T.seed_of(topo, plan)
    r64, _, _ = T.reference(topo, plan, seed)
    quiet = lambda *a: None
    assert T.compare([dict(r) for r in r64], topo, plan, seed, log=quiet)[0] == []
    mask = r64[2]['mask:block.conv1'].clone()
    mask.view(-1)[0] ^= 1
    for step, name, value in ((2, 'mask:block.conv1', mask), (1, 'buf:block.bn1.num_batches_tracked', r64[1]['buf:block.bn1.num_batches_tracked'] + 1),
                              (3, 'stat:sparsity', r64[3]['stat:sparsity'] + 1e-9), (1, 'ratio', 0.26), (0, 'grad:block.conv2.weight', None),
                              (2, 'upd:block.bn1.weight', r64[2]['upd:block.bn1.weight'] * (1 + 2e-4))):
        got = [dict(r) for r in r64]
        got[step][name] = value
        bad, _ = T.compare(got, topo, plan, seed, log=quiet)
        assert [(s, n) for s, n, _, _ in bad] == [(step, name)], (name, bad)
