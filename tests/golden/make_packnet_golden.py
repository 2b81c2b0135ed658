#!/usr/bin/env python3
"""Generate the PackNet fixtures under tests/golden/ by RUNNING the reference's PackNet stack (packnet_models/, utils/packnet_prune.py,
utils/packnet_manager.py), beside make_golden.py and under the same rules: the reference is imported at run time from its checkout
(the CPG_REFERENCE environment variable names it), nothing of its source travels, the fixtures are tensors, scalars and name lists only.

    CPG_REFERENCE=<checkout of ivclab/CPG> python tests/golden/make_packnet_golden.py

    packnet_ops.npz             crafted cases for every method of the reference's SparsePruner
    packnet_steps.npz           index of a two-task run of its Manager on a small net; one packnet_steps_NN.npz per train step holds the
                                complete state before the step and everything the step produced (teacher-forced: no check inherits drift)
    packnet_checkpoint-1.pth.tar    the checkpoint its save_checkpoint wrote after the last phase
    packnet_topology.json/.npz  module names, shapes and seeded-init digests of vgg16_bn_cifar100 and vgg16_bn; eval logits of the former
"""
import json
import os
import shutil
import sys
import tempfile
import types
import warnings
import zlib

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get('CPG_REFERENCE')
if not REF or not os.path.isdir(REF):
    sys.exit('make_packnet_golden: set CPG_REFERENCE to a checkout of the reference (ivclab/CPG)')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
warnings.filterwarnings('ignore')

# the reference calls .cuda() unconditionally (utils/packnet_prune.py:30,180); without a GPU make it the identity
torch.Tensor.cuda = lambda self, *a, **k: self
nn.Module.cuda = lambda self, *a, **k: self

import packnet_models  # noqa: E402  (reference)
from utils.packnet_prune import SparsePruner  # noqa: E402
from utils.packnet_manager import Manager  # noqa: E402
from utils import Optimizers  # noqa: E402


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    out['_torch_version'] = np.asarray(torch.__version__)
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %d bytes' % (name, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20), name


class Wrap(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.module = m

    def forward(self, x):
        return self.module(x)


# --------------------------------------------------------------------------
# 1. pruner methods on crafted tensors
# --------------------------------------------------------------------------
class Flat(nn.Module):
    """One bias-free nn.Linear per given weight vector (named l0, l1, ...), plus a `classifiers` list the pruner must skip."""

    def __init__(self, weights):
        super().__init__()
        for i, w in enumerate(weights):
            lin = nn.Linear(w.numel(), 1, bias=False)
            lin.weight.data = w.clone().reshape(1, -1)
            setattr(self, 'l%d' % i, lin)
        self.classifiers = nn.ModuleList([nn.Linear(3, 2)])


def flat_pruner(weights, owners, cur, idx, **args):
    model = Flat(weights)
    masks = {'l%d' % i: o.clone().reshape(1, -1) for i, o in enumerate(owners)}
    a = types.SimpleNamespace(weight_decay=4e-5, target_sparsity=0.0, initial_sparsity=0.0, pruning_frequency=1)
    a.__dict__.update(args)
    p = SparsePruner(model, masks, a, 0, 10, idx)
    p.current_dataset_idx = cur
    return model, masks, p


def gen_ops():
    out = {}
    g = torch.Generator().manual_seed(7)

    def prune_case(tag, w, owner, cur, ratio, gradual_step=None):
        w = w.float()
        owner = owner.to(torch.uint8)
        kw = dict(target_sparsity=ratio, initial_sparsity=0.0) if gradual_step is not None else {}
        model, masks, p = flat_pruner([w], [owner], cur, cur, **kw)
        status = 0
        try:
            if gradual_step is None:
                p.one_shot_prune(ratio)
            else:
                got = p.gradually_prune(gradual_step)
                ratio = got                                    # the ratio the schedule asked for at this step
        except (RuntimeError, IndexError) as e:                 # kthvalue(0): the reference's way out when k rounds to 0
            status = 2
            print('  %s: reference raised %s' % (tag, type(e).__name__))
        out.update({'prune_%s_w' % tag: w, 'prune_%s_owner' % tag: owner, 'prune_%s_cur' % tag: cur, 'prune_%s_ratio' % tag: float(ratio),
                    'prune_%s_status' % tag: status, 'prune_%s_owner_out' % tag: masks['l0'].reshape(-1),
                    'prune_%s_w_out' % tag: model.l0.weight.data.reshape(-1)})

    n = 1003                                                     # not a multiple of 4
    w = torch.randn(n, generator=g)
    owner = torch.randint(0, 4, (n,), generator=g)
    prune_case('mixed', w, owner, 2, 0.6)                        # candidates include owner-0 slots (stale, non-zero weights under them)
    prune_case('cur_owns_nothing', w, owner.clamp(max=2), 3, 0.5)    # candidates are the owner-0 slots alone: nothing released, zeros written
    t = torch.randn(64, generator=g)
    t[:24] = 0.25
    t[24:30] = -0.25
    prune_case('ties', t, torch.ones(64), 1, 0.25)               # the cutoff value is shared by 30 slots: all of them go
    prune_case('round_half_even_down', torch.randn(5, generator=g), torch.ones(5), 1, 0.5)      # 2.5 -> 2
    prune_case('round_half_even_up', torch.randn(7, generator=g), torch.ones(7), 1, 0.5)        # 3.5 -> 4
    z = torch.randn(41, generator=g)
    z[::5] = 0.0
    z[1::5] = -0.0
    prune_case('signed_zeros', z, torch.ones(41), 1, 0.3)
    q = torch.randn(37, generator=g)
    q[5] = float('nan')
    prune_case('nan_above_cutoff', q, torch.ones(37), 1, 0.5)
    prune_case('k_zero', torch.randn(9, generator=g), torch.ones(9), 1, 0.01)       # round(0.09) = 0: the reference's exit path
    big = torch.randn(4096 * 3 + 5, generator=g)
    prune_case('three_blocks', big, torch.randint(0, 3, (big.numel(),), generator=g), 2, 0.6)
    prune_case('gradual', torch.randn(515, generator=g), torch.randint(1, 3, (515,), generator=g), 2, 0.4, gradual_step=5)
    q = torch.randn(16, generator=torch.Generator().manual_seed(8))      # (its own generator: the cases around it keep their values)
    q[[2, 7, 11]] = float('nan')
    # k = round(0.9 * 14) = 13 of 14 candidates, 3 of them NaN: the cutoff IS a NaN, nothing is released, free slots are still zeroed
    prune_case('nan_at_cutoff', q, torch.tensor([1, 1, 0, 1, 0, 1, 1, 1, 2, 1, 1, 1, 0, 1, 2, 1]), 1, 0.9)

    # routing, zeroing, claiming
    w = torch.randn(n, generator=g)
    gw = torch.randn(n, generator=g)
    owner = torch.randint(0, 4, (n,), generator=g).to(torch.uint8)
    model, masks, p = flat_pruner([w], [owner], 2, 2, weight_decay=4e-5)
    model.l0.weight.grad = gw.clone().reshape(1, -1)
    p.do_weight_decay_and_make_grads_zero()
    out.update(route_w=w, route_g=gw, route_owner=owner, route_cur=2, route_wd=4e-5, route_g_out=model.l0.weight.grad.reshape(-1))
    model, masks, p = flat_pruner([w], [owner], 2, 2)
    p.make_pruned_zero()
    out.update(zero_w_out=model.l0.weight.data.reshape(-1))
    for idx in (1, 2, 3):
        model, masks, p = flat_pruner([w], [owner], 3, idx)
        p.apply_mask()
        out['apply_idx%d_w_out' % idx] = model.l0.weight.data.reshape(-1)
    model, masks, p = flat_pruner([w], [owner], 3, 3)
    p.make_finetuning_mask()
    out.update(claim_owner_out=masks['l0'].reshape(-1), claim_cur_out=int(p.current_dataset_idx))

    # statistics: the first layer only; idx below the maximum owner id; a first layer with no slot >= idx
    first = torch.randint(0, 4, (203,), generator=g).to(torch.uint8)
    second = torch.randint(0, 4, (77,), generator=g).to(torch.uint8)
    low = torch.randint(0, 2, (50,), generator=g).to(torch.uint8)
    cases = [('all', first, second, 3), ('idx_below_max', first, second, 1), ('idx_two', first, second, 2), ('no_slot_ge_idx', low, second, 3),
             ('after_prune', torch.where(first == 3, torch.zeros_like(first), first), second, 3)]
    for tag, a, b, idx in cases:
        _, _, p = flat_pruner([torch.zeros(a.numel()), torch.zeros(b.numel())], [a, b], int(max(a.max(), b.max())), idx)
        out.update({'stats_%s_first' % tag: a, 'stats_%s_second' % tag: b, 'stats_%s_idx' % tag: idx,
                    'stats_%s_values' % tag: np.array([p.calculate_sparsity(), p.calculate_curr_task_ratio(), p.calculate_zero_ratio()],
                                                      dtype=np.float64)})
    _, masks, p = flat_pruner([torch.zeros(8)], [torch.tensor([0, 1, 2, 3, 3, 1, 0, 2])], 0, 1)
    out['init_cur_from_first_mask'] = int(SparsePruner(p.model, masks, p.args, None, None, 1).current_dataset_idx)
    save('packnet_ops', **out)


# --------------------------------------------------------------------------
# 2. two tasks of the reference's Manager on a small net, one process per phase emulated through its own checkpoint files
# --------------------------------------------------------------------------
HEAD_IN = 64


class View(nn.Module):
    def __init__(self, *shape):
        super().__init__()
        self.shape = shape

    def forward(self, x):
        return x.view(*self.shape)


class SmallNet(packnet_models.VGG):
    """The reference's VGG bookkeeping (datasets, classifiers, add_dataset, set_dataset, forward) over a trunk defined here:
    conv 3->16 (no bias) BN ReLU pool, conv 16->32 (bias, no BatchNorm: its bias has a gradient) ReLU pool pool, 512 -> 64 -> 64; heads read
    64 features."""

    def __init__(self, dataset_history, dataset2num_classes):
        trunk = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1, bias=False), nn.BatchNorm2d(16), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2),
                              nn.Conv2d(16, 32, 3, padding=1, bias=True), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2),
                              nn.MaxPool2d(2, 2), View(-1, 512), nn.Linear(512, HEAD_IN), nn.ReLU(True), nn.Linear(HEAD_IN, HEAD_IN),
                              nn.ReLU(True))
        nn.Module.__init__(self)
        self.features = trunk
        self.datasets, self.classifiers = dataset_history, nn.ModuleList()
        self.dataset2num_classes = dataset2num_classes
        for num_classes in dataset2num_classes.values():
            self.classifiers.append(nn.Linear(HEAD_IN, num_classes))
        self._initialize_weights()

    def add_dataset(self, dataset, num_classes):
        if dataset not in self.datasets:
            self.datasets.append(dataset)
            self.dataset2num_classes[dataset] = num_classes
            head = nn.Linear(HEAD_IN, num_classes)
            self.classifiers.append(head)
            nn.init.normal_(head.weight, 0, 0.01)
            nn.init.constant_(head.bias, 0)


STEP_FILES = []


def gen_steps():
    folder = tempfile.mkdtemp()
    fmt = '{save_folder}/checkpoint-{epoch}.pth.tar'
    g = torch.Generator().manual_seed(11)
    NCLS = 5

    def batch():
        return torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, NCLS, (8,), generator=g)

    index = {}
    events = []

    def phase(tag, dataset, mode, lr, load, save_to, nsteps):
        """What one run of packnet_cifar100_main_normal.py does (:111-300), with one-batch loaders."""
        torch.manual_seed(1)
        if load:
            ck = torch.load(fmt.format(save_folder=load, epoch=1), weights_only=False)
            history, d2n, masks, info = ck['dataset_history'], ck['dataset2num_classes'], ck['masks'], ck['shared_layer_info']
        else:
            history, d2n, masks, info = [], {}, {}, {}
        net = SmallNet(history, d2n)
        net.add_dataset(dataset, NCLS)
        net.set_dataset(dataset)
        if dataset not in info:
            info[dataset] = {k: {} for k in ('conv_bias', 'bn_layer_running_mean', 'bn_layer_running_var', 'bn_layer_weight', 'bn_layer_bias',
                                             'fc_bias')}
        model = Wrap(net)
        if not masks:
            for name, module in model.named_modules():
                if isinstance(module, (nn.Conv2d, nn.Linear)) and 'classifiers' not in name:
                    masks[name] = torch.ByteTensor(module.weight.data.size()).fill_(0)
        args = types.SimpleNamespace(dataset=dataset, cuda=False, weight_decay=4e-5, checkpoint_format=fmt, mode=mode)
        val = batch()
        mgr = Manager(args, model, info, masks, None, [val])
        logits = []
        model.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
        losses = []
        crit = mgr.criterion
        mgr.criterion = lambda o, t: (lambda l: (losses.append(float(l)), l)[1])(crit(o, t))
        if mode == 'inference':
            mgr.load_checkpoint_for_inference(1, load)
            acc = mgr.validate(0)
            index.update({'%s_x' % tag: val[0], '%s_t' % tag: val[1], '%s_logits' % tag: logits[-1], '%s_acc' % tag: acc,
                          '%s_stats' % tag: np.array([mgr.pruner.calculate_sparsity(), mgr.pruner.calculate_curr_task_ratio(),
                                                      mgr.pruner.calculate_zero_ratio()], dtype=np.float64)})
            events.append(tag)
            return
        active = '.{}.'.format(net.datasets.index(dataset))
        params = [p for n, p in model.named_parameters() if 'classifiers' not in n or active in n]
        sgd = torch.optim.SGD(params, lr=lr, weight_decay=0.0, momentum=0.9, nesterov=True)
        opts = Optimizers()
        opts.add(sgd, lr)
        mgr.load_checkpoint(opts, 1 if load else 0, load)
        if mode == 'prune':
            acc = mgr.validate(-1)
            index.update({'%s_val0_x' % tag: val[0], '%s_val0_t' % tag: val[1], '%s_val0_logits' % tag: logits[-1], '%s_val0_acc' % tag: acc})
            mgr.one_shot_prune(0.6)
            index.update({'%s_pruned_%s' % (tag, k): v.clone() for k, v in masks.items()})
            index['%s_sparsity_after_prune' % tag] = mgr.pruner.calculate_sparsity()
            index['%s_zero_ratio_after_prune' % tag] = mgr.pruner.calculate_zero_ratio()
        else:
            mgr.pruner.make_finetuning_mask()
        names = dict(model.named_parameters())
        for s in range(nsteps):
            x, t = batch()
            rec = {'x': x, 't': t, 'lr': lr, 'cur': int(mgr.pruner.current_dataset_idx), 'dataset_index': net.datasets.index(dataset)}
            rec.update({'before_state_' + k: v.clone() for k, v in net.state_dict().items() if not k.startswith('classifier.')})
            rec.update({'mask_' + k: v.clone() for k, v in masks.items()})
            mom = {n: sgd.state[p]['momentum_buffer'].clone() for n, p in names.items() if p in sgd.state and 'momentum_buffer' in sgd.state[p]}
            rec.update({'before_momentum_' + n: v for n, v in mom.items()})
            rec['has_momentum'] = int(bool(mom))
            mgr.train_loader = [(x, t)]
            acc = mgr.train(opts, s, [lr])
            rec.update(logits=logits[-1], loss=losses[-1], acc=acc)
            rec.update({'after_state_' + k: v.clone() for k, v in net.state_dict().items() if not k.startswith('classifier.')})
            rec.update({'after_grad_' + n: p.grad.clone() for n, p in names.items() if p.grad is not None})
            rec.update({'after_momentum_' + n: sgd.state[p]['momentum_buffer'].clone() for n, p in names.items() if p in sgd.state})
            name = 'packnet_steps_%02d' % len(STEP_FILES)
            STEP_FILES.append(name)
            events.append('%s:%s:%s:%d' % (name, dataset, mode, s))
            save(name, **rec)
        acc = mgr.validate(nsteps - 1)
        index.update({'%s_val_x' % tag: val[0], '%s_val_t' % tag: val[1], '%s_val_logits' % tag: logits[-1], '%s_val_acc' % tag: acc})
        os.makedirs(save_to, exist_ok=True)
        mgr.save_checkpoint(opts, 0, save_to)

    d = lambda n: os.path.join(folder, n)     # noqa: E731
    phase('t1_finetune', 't1', 'finetune', 1e-2, None, d('t1s'), 2)
    phase('t1_prune', 't1', 'prune', 1e-3, d('t1s'), d('t1p'), 1)
    phase('t2_finetune', 't2', 'finetune', 1e-2, d('t1p'), d('t2s'), 2)
    phase('t2_prune', 't2', 'prune', 1e-3, d('t2s'), d('t2p'), 1)
    phase('infer_t1', 't1', 'inference', 0.0, d('t2p'), None, 0)
    phase('infer_t2', 't2', 'inference', 0.0, d('t2p'), None, 0)
    index['events'] = np.array(events)
    save('packnet_steps', **index)
    dst = os.path.join(OUT, 'packnet_checkpoint-1.pth.tar')
    shutil.copyfile(fmt.format(save_folder=d('t2p'), epoch=1), dst)
    print('wrote packnet_checkpoint-1.pth.tar,', os.path.getsize(dst), 'bytes')
    shutil.rmtree(folder)


# --------------------------------------------------------------------------
# 3. topology of the two provided models
# --------------------------------------------------------------------------
def crc(t):
    return zlib.crc32(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())


def gen_topology():
    topo = {'torch': torch.__version__, 'seed': 1}
    for arch in ('vgg16_bn_cifar100', 'vgg16_bn'):
        torch.manual_seed(1)
        net = packnet_models.__dict__[arch](pretrained=False, dataset_history=[], dataset2num_classes={})
        net.add_dataset('t1', 5)
        net.set_dataset('t1')
        topo[arch] = {'modules': [[n, type(m).__name__] for n, m in net.named_modules()],
                      'state': [[k, list(v.shape), crc(v)] for k, v in net.state_dict().items()]}
        if arch == 'vgg16_bn_cifar100':
            net.eval()
            x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1))
            with torch.no_grad():
                save('packnet_topology', x=x, logits=net(x))
        del net
    with open(os.path.join(OUT, 'packnet_topology.json'), 'w') as f:
        json.dump(topo, f, indent=0)
    print('wrote packnet_topology.json')


if __name__ == '__main__':
    gen_ops()
    gen_steps()
    gen_topology()
