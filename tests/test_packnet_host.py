"""PackNet baseline stack, CPU side: the host restatement (tests/_packnet.py) against the reference's fixtures, the mirror models'
topology, the learning-rate steps and the goals hand-off."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import _packnet as pk

GOLDEN = pk.GOLDEN


@pytest.fixture(scope='module')
def ops():
    return pk.load('packnet_ops')


def test_restated_prunes_reproduce_the_reference(ops):
    tags = pk.prune_tags(ops)
    assert {'mixed', 'cur_owns_nothing', 'ties', 'round_half_even_down', 'round_half_even_up', 'signed_zeros', 'nan_above_cutoff', 'nan_at_cutoff', 'k_zero',
            'three_blocks', 'gradual'} <= set(tags)
    for tag in tags:
        g = lambda k: ops['prune_%s_%s' % (tag, k)]      # noqa: E731
        status, owner, w = pk.rank_prune_zero(g('w'), g('owner'), int(g('cur')), float(g('ratio')))
        assert status == int(g('status')), tag
        assert np.array_equal(owner, g('owner_out')), tag
        assert w.tobytes() == g('w_out').tobytes(), tag                   # bit for bit: +0.0 under owner 0, NaN kept elsewhere
    assert int(ops['prune_k_zero_status']) == 2 and np.array_equal(ops['prune_k_zero_owner'], ops['prune_k_zero_owner_out'])
    # k = round(0.25 * 64) = 16 lands among the 30 slots of magnitude 0.25: every one of them goes, more than k in all
    assert not ops['prune_ties_owner_out'][:30].any() and int((ops['prune_ties_owner_out'] == 0).sum()) > 16
    assert int((ops['prune_round_half_even_down_owner_out'] == 0).sum()) == 2 and int((ops['prune_round_half_even_up_owner_out'] == 0).sum()) == 4


def test_restated_routing_masking_and_claiming_reproduce_the_reference(ops):
    w, g, owner = ops['route_w'], ops['route_g'], ops['route_owner']
    got = pk.route(g, w, owner, int(ops['route_cur']), float(ops['route_wd']))
    assert np.array_equal(got == 0, ops['route_g_out'] == 0)
    assert pk.scale_err(got, ops['route_g_out']) <= 1e-5
    assert pk.zero_pruned(w, owner).tobytes() == ops['zero_w_out'].tobytes()
    for idx in (1, 2, 3):
        assert pk.apply_mask(w, owner, idx).tobytes() == ops['apply_idx%d_w_out' % idx].tobytes()
    claimed, cur = pk.claim_free(owner, 3)
    assert np.array_equal(claimed, ops['claim_owner_out']) and cur == int(ops['claim_cur_out'])
    assert int(ops['init_cur_from_first_mask']) == 3


def test_restated_statistics_reproduce_the_reference(ops):
    tags = sorted(k[len('stats_'):-len('_values')] for k in ops.files if k.startswith('stats_') and k.endswith('_values'))
    assert {'idx_below_max', 'no_slot_ge_idx', 'after_prune'} <= set(tags)
    for tag in tags:
        got = pk.statistics(ops['stats_%s_first' % tag], int(ops['stats_%s_idx' % tag]))
        assert list(got) == list(ops['stats_%s_values' % tag]), tag          # equal as floats
    assert ops['stats_no_slot_ge_idx_values'][0] == 0.0 and ops['stats_after_prune_values'][0] == 0.0


@pytest.mark.parametrize('name', pk.STEP_FILES)
def test_restated_step_reproduces_the_reference(name):
    fx = pk.load(name)
    worst = pk.check_step(pk.cpu_step(fx), fx, 1e-5)
    print(name, worst)


def test_step_index_lists_every_step_file():
    index = pk.load('packnet_steps')
    steps = [e.split(':')[0] for e in index['events'].tolist() if ':' in e]
    assert steps == pk.STEP_FILES


def _crc(t):
    return zlib.crc32(np.ascontiguousarray(t.detach().numpy()).tobytes())


@pytest.mark.parametrize('arch', ['vgg16_bn_cifar100', 'vgg16_bn'])
def test_mirror_models_match_the_reference_topology(arch):
    import torch.nn as nn
    import cpg_amd.packnet_models as pm
    with open(os.path.join(GOLDEN, 'packnet_topology.json')) as f:
        topo = json.load(f)
    torch.manual_seed(topo['seed'])
    net = getattr(pm, arch)(pretrained=False, dataset_history=[], dataset2num_classes={})
    net.add_dataset('t1', 5)
    net.set_dataset('t1')
    want = topo[arch]
    assert [n for n, _ in net.named_modules()] == [n for n, _ in want['modules']]
    base = {'Conv2d': nn.Conv2d, 'Linear': nn.Linear, 'BatchNorm2d': nn.BatchNorm2d, 'ReLU': nn.ReLU, 'MaxPool2d': nn.MaxPool2d,
            'Dropout': nn.Dropout, 'ModuleList': nn.ModuleList}
    for (n, m), (_, kind) in zip(net.named_modules(), want['modules']):
        if kind in base:
            assert isinstance(m, base[kind]), (n, kind)                    # the reference's isinstance tests hold
    state = net.state_dict()
    assert list(state) == [k for k, _, _ in want['state']]
    for k, shape, digest in want['state']:
        assert list(state[k].shape) == shape, k
        assert _crc(state[k]) == digest, 'seeded initial value of %s' % k


def test_nan_cutoff_case_releases_nothing_and_still_zeroes(ops):
    """k lands on a NaN: `abs(w) <= nan` is false everywhere, so no owner changes; the slots already free are still zeroed."""
    owner, out, w_out = ops['prune_nan_at_cutoff_owner'], ops['prune_nan_at_cutoff_owner_out'], ops['prune_nan_at_cutoff_w_out']
    assert int(ops['prune_nan_at_cutoff_status']) == 0 and np.array_equal(owner, out) and (owner == 0).sum() == 3
    assert not w_out.view(np.uint32)[owner == 0].any() and np.isnan(w_out[owner != 0]).sum() == 2


def test_plain_conv_offers_what_the_borrowed_methods_read():
    """PlainConv2d borrows forward_with_bn_stats / forward_bn_eval (and the frame the inference methods share, _forward_eval) from
    SharableConv2d: every attribute they read must exist on it, and its shared `info` cannot be written."""
    import inspect
    import re
    from cpg_amd.models.layers import SharableConv2d
    from cpg_amd.packnet_models.layers import PlainConv2d
    conv = PlainConv2d(3, 8, 3, padding=1)
    assert PlainConv2d.forward_with_bn_stats is SharableConv2d.forward_with_bn_stats and PlainConv2d.forward_bn_eval is SharableConv2d.forward_bn_eval
    assert PlainConv2d._forward_eval is SharableConv2d._forward_eval
    assert '_forward_eval' in set(re.findall(r'self\.(\w+)', inspect.getsource(SharableConv2d.forward_bn_eval)))
    for fn in (SharableConv2d.forward_with_bn_stats, SharableConv2d.forward_bn_eval, SharableConv2d._forward_eval):
        for name in set(re.findall(r'self\.(\w+)', inspect.getsource(fn))):
            assert hasattr(conv, name), name
    assert conv.piggymask is None and conv.info['threshold'] == 0.0 and conv._math() == 'fp32'
    with pytest.raises(TypeError):
        conv.info['threshold'] = 1.0


def test_out_of_scope_factories_say_so():
    import cpg_amd.packnet_models as pm
    from cpg_amd.models.spherenet import AngleLoss
    assert pm.AngleLoss is AngleLoss
    for name in ('resnet18', 'resnet50', 'spherenet20'):
        with pytest.raises(NotImplementedError, match='out of scope'):
            getattr(pm, name)(dataset_history=[], dataset2num_classes={})


def test_learning_rate_steps_land_on_the_reference_epochs():
    from cpg_amd.baselines import lr_schedule
    ft = lr_schedule(1e-2, 'finetune', 100)
    drops = [e + 1 for e in range(99) if ft[e + 1] != ft[e]]               # epochs (1-based) after which the rate changes
    assert drops == [50, 80]
    assert ft[0] == 1e-2 and ft[50] == 1e-2 * 0.1 and ft[80] == 1e-2 * 0.1 * 0.1
    pr = lr_schedule(1e-3, 'prune', 30)
    assert [e + 1 for e in range(29) if pr[e + 1] != pr[e]] == [25] and pr[25] == 1e-3 * 0.1


def test_goals_round_trip(tmp_path):
    from cpg_amd.baselines import BaselineSession, read_goals
    s = BaselineSession(arch=lambda **kw: None, device='cpu')
    s._goals = {'fish': '{:.4f}'.format(0.81234), 'trees': '{:.4f}'.format(0.5)}
    assert s.accuracy_goals() == {'fish': '0.8123', 'trees': '0.5000'}
    path = str(tmp_path / 'baseline_acc.txt')
    with open(path, 'w') as f:
        json.dump({'people': '0.4000', 'fish': '0.1000'}, f)               # an earlier run's file: merged, this run's values win
    s.write_logfile(path)
    goals = read_goals(path)
    assert goals == {'people': '0.4000', 'fish': '0.8123', 'trees': '0.5000'}
    assert float(goals['fish']) == 0.8123
