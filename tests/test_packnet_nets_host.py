"""The PackNet ResNet-50 and SphereNet-20 without a GPU: topology, seeded initialisation and covered layers against what the reference's
packnet_models produced (tests/golden/packnet_nets_topology.json; generator: tests/golden/make_packnet_nets_golden.py), the checkpoint
dictionary of the face flow, the factories that cannot exist, and the learning-rate rules of the two mains as pure functions.
"""
import types

import pytest
import torch
import torch.nn as nn

from _packnet_nets import build, covered, crc, topology


# ---------------------------------------------------------------- H1
@pytest.mark.parametrize('arch', ['resnet50', 'spherenet20'])
def test_topology_and_seeded_init_equal_the_reference(arch):
    """Names, types, state_dict shapes, covered layers and the crc32 of every tensor after torch.manual_seed(1) + add_dataset: the
    digests pin that construction and initialisation consume the RNG exactly as the reference's do."""
    topo = topology()
    net = build(arch, topo)
    want = topo[arch]
    mods = list(net.named_modules())
    assert [n for n, _ in mods] == [n for n, _ in want['modules']]
    for (name, m), (_, ref_type) in zip(mods, want['modules']):
        if name == '':
            continue                                     # (the root class: ResNet / SphereNet20 in both)
        # ours are subclasses of the reference's layer types (PlainConv2d is an nn.Conv2d, FusedSequential an nn.Sequential, ...)
        assert ref_type in [c.__name__ for c in type(m).__mro__], (name, type(m).__name__, ref_type)
    assert type(net).__name__ == want['modules'][0][1]
    state = net.state_dict()
    assert list(state) == [k for k, _, _ in want['state']]
    for k, shape, _ in want['state']:
        assert list(state[k].shape) == shape, k
    assert [[n, m.weight.numel()] for n, m in covered(net)] == want['covered']
    assert len(want['covered']) == {'resnet50': 53, 'spherenet20': 20}[arch]
    assert min(n for _, n in want['covered']) == {'resnet50': 4096, 'spherenet20': 1728}[arch]
    bad = [k for k, _, digest in want['state'] if crc(state[k]) != digest]
    assert not bad, 'seeded init differs from the reference in %d tensors, first %s' % (len(bad), bad[:3])


def test_further_bottleneck_depths_share_the_class():
    import cpg_amd.packnet_models as pm
    net = pm.factory('resnet101')(dataset_history=[], dataset2num_classes={})
    assert len(covered(net)) == 1 + 3 * (3 + 4 + 23 + 3) + 4 and len(net.classifiers) == 0


# ---------------------------------------------------------------- H2
def _manager(net, dataset):
    from cpg_amd.driver import _Plain
    from cpg_amd.utils.packnet_manager import Manager, make_masks
    model = _Plain(net)
    args = types.SimpleNamespace(dataset=dataset, cuda=False, weight_decay=4e-5, mode='finetune', progress=False, log_path=None,
                                 checkpoint_format='{save_folder}/checkpoint-{epoch}.pth.tar')
    return Manager(args, model, {}, make_masks(model), None, None)


def test_spherenet_checkpoint_dictionary_and_stash_round_trip():
    from cpg_amd.utils.packnet_manager import TASK_KEYS
    topo = topology()
    net = build('spherenet20', topo)
    mgr = _manager(net, 'age')
    ck = mgr.checkpoint_dict()
    assert set(ck) == {'model_state_dict', 'dataset_history', 'dataset2num_classes', 'masks', 'shared_layer_info'}
    assert list(ck['model_state_dict']) == [k for k, _, _ in topo['spherenet20']['state']]
    assert set(ck['masks']) == {n for n, _ in topo['spherenet20']['covered']}
    info = ck['shared_layer_info']['age']
    assert set(info) == set(TASK_KEYS) | {'prelu_layer_weight'}                 # packnet_face_main.py:175-184
    convs = [n for n, m in net.named_modules() if isinstance(m, nn.Conv2d)]
    prelus = [n for n, m in net.named_modules() if isinstance(m, nn.PReLU)]
    assert sorted(info['conv_bias']) == sorted(convs) and sorted(info['prelu_layer_weight']) == sorted(prelus) and len(prelus) == 20
    assert not info['fc_bias'] and not info['bn_layer_weight']
    # the task's biases and slopes as they are now; then scramble the live ones and attach
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.PReLU):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g))
    mgr.collect_task_layers()
    want = {n: m.bias.detach().clone() for n, m in net.named_modules() if isinstance(m, nn.Conv2d)}
    want.update({n: m.weight.detach().clone() for n, m in net.named_modules() if isinstance(m, nn.PReLU)})
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                m.bias.add_(1.0)
            elif isinstance(m, nn.PReLU):
                m.weight.mul_(-3.0)
    mgr.attach_task_layers()
    for n, m in net.named_modules():
        if isinstance(m, nn.Conv2d):
            assert torch.equal(m.bias, want[n]), n
        elif isinstance(m, nn.PReLU):
            assert torch.equal(m.weight, want[n]), n


def test_vgg_task_dictionary_is_unchanged():
    import cpg_amd.packnet_models as pm
    from cpg_amd.utils.packnet_manager import TASK_KEYS, new_task_info
    assert tuple(new_task_info()) == TASK_KEYS and 'prelu_layer_weight' not in TASK_KEYS
    net = pm.vgg16_bn_cifar100(dataset_history=[], dataset2num_classes={})
    net.add_dataset('t1', 5)
    net.set_dataset('t1')
    assert set(_manager(net, 't1').checkpoint_dict()['shared_layer_info']['t1']) == set(TASK_KEYS)


# ---------------------------------------------------------------- H3
@pytest.mark.parametrize('name', ['resnet18', 'resnet34'])
def test_basic_block_resnets_say_why_they_cannot_exist(name):
    import cpg_amd.packnet_models as pm
    with pytest.raises(NotImplementedError, match='2048'):
        pm.factory(name)(dataset_history=[], dataset2num_classes={})


def test_flat_names_keep_raising_and_factory_finds_the_nets():
    """The package's flat attributes are what they were (tests/test_packnet_host.py pins that three of them raise); factory() is the way
    to every net, under the reference's names."""
    import cpg_amd.packnet_models as pm
    from cpg_amd.packnet_models import resnet, spherenet
    assert pm.factory('resnet50') is resnet.resnet50 and pm.factory('spherenet20') is spherenet.spherenet20
    assert pm.factory('vgg16_bn_cifar100') is pm.vgg16_bn_cifar100 and pm.factory('vgg16_bn') is pm.vgg16_bn
    with pytest.raises(KeyError):
        pm.factory('resnext50_32x4d')
    with pytest.raises(NotImplementedError, match='factory'):
        pm.resnet50(dataset_history=[], dataset2num_classes={})


def test_session_accepts_the_two_nets():
    from cpg_amd.baselines import BaselineSession
    import cpg_amd.packnet_models as pm
    for arch, policy in (('resnet50', 'imagenet'), ('spherenet20', 'face')):
        s = BaselineSession(arch=arch, device='cpu')
        assert s.factory is pm.factory(arch) and s.policy_name == policy
    assert BaselineSession(arch='vgg16_bn_cifar100', device='cpu').policy_name == 'cifar'
    assert BaselineSession(arch='vgg16_bn', device='cpu').policy_name == 'cifar'           # (unchanged; policy='imagenet' selects the main's rules)


# ---------------------------------------------------------------- H4
def test_plateau_rule_on_a_crafted_sequence():
    """packnet_face_main.py:334-378 by hand.  Accuracies: a best in epoch 1, then nothing better.  The stale count reaches 10 at the end of
    epoch 11 -> first decay; again at the end of epochs 21 and 31 -> second and third; the `>= 3` test stands BEFORE the decay, so epoch 31
    still ends normally and epoch 32, trained at lr * 1e-3, is the last."""
    from cpg_amd.baselines import PlateauRule, plateau_schedule
    lrs = plateau_schedule(0.1, [0.5] + [0.4] * 60)
    assert len(lrs) == 32
    assert lrs[:11] == [0.1] * 11 and lrs[11:21] == [0.1 * 0.1] * 10 and lrs[21:31] == [0.1 * 0.1 * 0.1] * 10
    assert lrs[31] == 0.1 * 0.1 * 0.1 * 0.1
    # a new best resets the count (:335-337): 9 stale epochs, a best, 9 stale epochs -> no decay in 20 epochs
    assert plateau_schedule(1e-3, [0.5] + [0.4] * 9 + [0.6] + [0.4] * 9) == [1e-3] * 20
    # an equal accuracy is not better (`>`), and 0.0 never beats the initial best of 0.0: no epoch of such a run is ever kept
    rule = PlateauRule()
    assert [rule.update(0.0)[0] for _ in range(3)] == [False] * 3 and rule.stale == 3
    rule = PlateauRule()
    assert rule.update(0.3) == (True, False, 1.0) and rule.update(0.3) == (False, False, 1.0)


def test_prune_mode_drops():
    """The cifar main drops after epoch 25 (unchanged), the face and imagenet mains after epoch 40 (packnet_face_main.py:380-384)."""
    from cpg_amd.baselines import LR_DROPS, PLATEAU_LR_DROPS, POLICIES, lr_schedule
    assert POLICIES['cifar']['drops'] is LR_DROPS and POLICIES['face']['drops'] is POLICIES['imagenet']['drops'] is PLATEAU_LR_DROPS
    pr = lr_schedule(1e-3, 'prune', 60, PLATEAU_LR_DROPS)
    assert [e + 1 for e in range(59) if pr[e + 1] != pr[e]] == [40] and pr[39] == 1e-3 and pr[40] == 1e-3 * 0.1
    assert lr_schedule(1e-2, 'finetune', 100, PLATEAU_LR_DROPS) == [1e-2] * 100          # (finetune follows the accuracies instead)
    assert lr_schedule(1e-3, 'prune', 30)[25] == 1e-3 * 0.1


def test_keeping_a_pruned_stage():
    """packnet_face_main.py:386-389: train accuracy above 0.97 and at most 0.01 below the goal; the cifar main: train accuracy only."""
    from cpg_amd.baselines import keep_pruned_stage
    assert keep_pruned_stage(0.98, 0.10) and not keep_pruned_stage(0.97, 0.99)
    assert keep_pruned_stage(0.98, 0.80, goal=0.805, max_val_drop=0.01)
    assert not keep_pruned_stage(0.98, 0.79, goal=0.805, max_val_drop=0.01)
    assert not keep_pruned_stage(0.90, 0.90, goal=0.805, max_val_drop=0.01)
    assert keep_pruned_stage(None, 0.80, goal=0.805, max_val_drop=0.01) and not keep_pruned_stage(float('nan'), 0.70, goal=0.805, max_val_drop=0.01)


# ---------------------------------------------------------------- the session's pieces that need no GPU
def test_pretrained_names_map_as_in_the_two_mains():
    """packnet_face_main.py:196-203 (everything but `fc*`; fc5 / fc6 become the face head's embedding layer and AngleLinear) and
    packnet_imagenet_main.py:177-184 (everything but `fc`, which becomes the `imagenet` head) -- and only for those first datasets."""
    from cpg_amd.baselines import BaselineSession, map_pretrained
    t = {k: torch.full((1,), float(i)) for i, k in enumerate(('conv1_1.weight', 'relu1_1.weight', 'fc5.weight', 'fc5.bias', 'fc6.weight'))}
    got = map_pretrained('face', t, 'face_verification')
    assert set(got) == {'conv1_1.weight', 'relu1_1.weight', 'classifiers.0.0.weight', 'classifiers.0.0.bias', 'classifiers.0.1.weight'}
    assert got['classifiers.0.0.weight'] is t['fc5.weight'] and got['classifiers.0.0.bias'] is t['fc5.bias']
    assert got['classifiers.0.1.weight'] is t['fc6.weight'] and got['conv1_1.weight'] is t['conv1_1.weight']
    assert set(map_pretrained('face', t, 'gender')) == {'conv1_1.weight', 'relu1_1.weight'}
    r = {k: torch.zeros(1) for k in ('conv1.weight', 'layer1.0.bn1.running_mean', 'fc.weight', 'fc.bias')}
    got = map_pretrained('imagenet', r, 'imagenet')
    assert set(got) == {'conv1.weight', 'layer1.0.bn1.running_mean', 'classifiers.0.weight', 'classifiers.0.bias'}
    assert got['classifiers.0.weight'] is r['fc.weight'] and got['classifiers.0.bias'] is r['fc.bias']
    assert set(map_pretrained('imagenet', r, 'cubs_cropped')) == {'conv1.weight', 'layer1.0.bn1.running_mean'}
    # ... and into a model: a SphereNet-20 with the face head takes every tensor of a face state_dict, and nothing else moves
    s = BaselineSession('spherenet20', device='cpu', seed=1)
    holder = s._fresh()
    s._start(holder, 'face_verification', 10)
    before = {k: v.clone() for k, v in holder.net.state_dict().items()}
    face = {'conv3_4.bias': torch.full((256,), 0.5), 'relu4_3.weight': torch.full((512,), 0.125), 'fc5.weight': torch.full((512, 25088), 1.5),
            'fc5.bias': torch.full((512,), 2.0), 'fc6.weight': torch.full((512, 10), 3.0)}
    s._load_pretrained(holder, 'face_verification', face)
    after = holder.net.state_dict()
    moved = {'conv3_4.bias': 'conv3_4.bias', 'relu4_3.weight': 'relu4_3.weight', 'classifiers.0.0.weight': 'fc5.weight',
             'classifiers.0.0.bias': 'fc5.bias', 'classifiers.0.1.weight': 'fc6.weight'}
    for k, v in after.items():
        if k.startswith('classifier.'):
            continue                                     # (the alias of the active head)
        assert torch.equal(v, face[moved[k]] if k in moved else before[k]), k


class _FakeHolder(object):
    def __init__(self):
        self.state, self.restored = 0, None

    def snapshot(self):
        return self.state

    def restore(self, snap):
        self.state = self.restored = snap


class _FakeManager(object):
    """train() moves the holder's state on by one; validate() returns the next of the given accuracies."""

    def __init__(self, holder, val_accs, dataset='flowers'):
        self.holder, self.val_accs, self.lrs_seen = holder, list(val_accs), []
        self.args = types.SimpleNamespace(dataset=dataset)

    def train(self, opts, epoch, lrs):
        self.holder.state += 1
        self.lrs_seen.append(opts[0].param_groups[0]['lr'])
        return 0.5 + 0.01 * epoch

    def validate(self, epoch):
        return self.val_accs[epoch]


def _fake_opts(lr):
    from cpg_amd.utils import Optimizers
    opts = Optimizers()
    opts.add(types.SimpleNamespace(param_groups=[{'lr': lr}]), lr)
    return opts


def test_plateau_finetune_keeps_the_best_epoch():
    """Under the 'imagenet' / 'face' policy the finetune phase ends on the state of its best validation epoch (the only checkpoint the
    reference keeps, packnet_face_main.py:335-347) and reports that epoch's accuracies; the rate drops after 10 epochs without a best."""
    from cpg_amd.baselines import BaselineSession
    s = BaselineSession(arch=lambda **kw: None, device='cpu', policy='imagenet')
    accs = [0.30, 0.50, 0.45, 0.40] + [0.35] * 10
    holder = _FakeHolder()
    mgr = _FakeManager(holder, accs)
    tr, va = s._epochs(holder, mgr, _fake_opts(1e-3), 'finetune', len(accs))
    assert (tr, va) == (0.5 + 0.01 * 1, 0.50)
    assert holder.restored == 2 and holder.state == 2                   # the state after the second epoch, not after the 14th
    # epochs 3 .. 12 are ten without a best: epochs 13 and 14 train at a tenth
    assert mgr.lrs_seen[:12] == [1e-3] * 12 and mgr.lrs_seen[12:] == [1e-3 * 0.1] * 2
    # no epoch beats 0.0: nothing is put back, the last epoch's numbers are reported
    holder = _FakeHolder()
    tr, va = s._epochs(holder, _FakeManager(holder, [0.0, 0.0]), _fake_opts(1e-3), 'finetune', 2)
    assert holder.restored is None and holder.state == 2 and (tr, va) == (0.51, 0.0)
    # the prune phase of these mains, and everything of the cifar main: last epoch, fixed drops
    holder = _FakeHolder()
    mgr = _FakeManager(holder, [0.9] + [0.1] * 40)
    tr, va = s._epochs(holder, mgr, _fake_opts(1e-3), 'prune', 41)
    assert holder.restored is None and va == 0.1 and mgr.lrs_seen[39] == 1e-3 and mgr.lrs_seen[40] == 1e-3 * 0.1
    c = BaselineSession(arch=lambda **kw: None, device='cpu')
    holder = _FakeHolder()
    mgr = _FakeManager(holder, [0.9, 0.1, 0.1])
    assert c._epochs(holder, mgr, _fake_opts(1e-2), 'finetune', 3)[1] == 0.1 and holder.restored is None


def test_plain_conv_offers_what_forward_with_skip_reads():
    """PlainConv2d borrows forward_with_skip too (residual blocks): every attribute it reads exists on an instance."""
    import inspect
    import re
    from cpg_amd.models.layers import SharableConv2d
    from cpg_amd.packnet_models.layers import PlainConv2d
    conv = PlainConv2d(8, 8, 1, bias=False)
    assert PlainConv2d.forward_with_skip is SharableConv2d.forward_with_skip
    names = set(re.findall(r'self\.(\w+)', inspect.getsource(SharableConv2d.forward_with_skip)))
    assert {'piggymask', 'info', 'groups', 'weight', 'bias', 'forward'} <= names
    for name in names:
        assert hasattr(conv, name), name
