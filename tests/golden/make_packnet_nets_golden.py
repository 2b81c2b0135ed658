#!/usr/bin/env python3
"""Generate the fixtures of the PackNet ResNet-50 and SphereNet-20 under tests/golden/ by RUNNING the reference's PackNet stack
(packnet_models/{resnet,spherenet}.py, utils/packnet_prune.py, utils/packnet_manager.py), beside make_packnet_golden.py and under its
rules: the reference is imported at run time from its checkout (the CPG_REFERENCE environment variable names it), nothing of its
source travels, the fixtures are tensors, scalars and name lists only.

    CPG_REFERENCE=<checkout of ivclab/CPG> python tests/golden/make_packnet_nets_golden.py

The two nets have no width multiplier (11.65 M and 23.45 M trunk weights), so no fixture holds a weight tensor or an input image:
inputs are regenerated from the seeds stored here (a crc32 of each is stored with it), weights from torch.manual_seed(1), and the
fixtures carry digests, small outputs and a seeded sample of 4096 weights per covered layer.

    packnet_nets_topology.json/.npz   named_modules() names and types, state_dict names / shapes / crc32 after torch.manual_seed(1) +
                                      add_dataset, the pruner's covered layers; eval-mode outputs of seeded batches
    packnet_nets_prune.npz            make_finetuning_mask + one_shot_prune(0.6) on the seeded-init weights: per covered layer k, cutoff,
                                      released count, crc32 of the owner mask and of the zeroed weights
    packnet_nets_steps_<net>.npz      the reference Manager from the seed: claim, 3 train steps, validate, one_shot_prune(0.6), 2 retrain
                                      steps, validate -- per step loss, logits, the pruner's three statistics; `band/*`: the distance to
                                      the same run with every input multiplied by (1 + 1e-6 N(0,1)), as sequence_resnet50.npz carries it:
                                      one figure per step and tensor, and the number of sampled owner bytes that differ after the prune
                                      (the largest over TWINS such repetitions, see there; `single_band/*`: how many of the other
                                      repetitions fall outside the band the first one alone would give)
    packnet_nets_steps_<net>_wN.npz   the weight sample after step N (one file per step: the size limit)

Harness shims: `.cuda()` is the identity (as in make_packnet_golden.py), and the reference's packnet_models.spherenet gets
torch.nn.functional as `F`, which its AngleLoss uses without importing.
"""
import json
import os
import sys
import types
import warnings
import zlib

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get('CPG_REFERENCE')
if not REF or not os.path.isdir(REF):
    sys.exit('make_packnet_nets_golden: set CPG_REFERENCE to a checkout of the reference (ivclab/CPG)')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
warnings.filterwarnings('ignore')

torch.Tensor.cuda = lambda self, *a, **k: self
nn.Module.cuda = lambda self, *a, **k: self

import packnet_models  # noqa: E402  (reference)
import packnet_models.spherenet as _ref_sphere  # noqa: E402
from utils.packnet_manager import Manager  # noqa: E402
from utils import Optimizers  # noqa: E402

_ref_sphere.F = torch.nn.functional

SEED = 1
SAMPLE = 4096
# what the reference's baseline scripts pass to packnet_imagenet_main.py / packnet_face_main.py for these nets (experiment2/
# baseline_imagenet.sh:24-32, experiment3/baseline_face.sh:28-38).  The mains' argparse default, 0.1, is not usable from a seeded
# initialisation: the reference's own SphereNet-20 run reaches a loss of 1.8e13 in step 2 and NaN in step 3, its ResNet-50 a loss of 158.
LR = 1e-3
PRUNE = 0.6
NETS = {'resnet50': dict(heads=[('t1', 5)], train=(4, 3, 64, 64), evals=[(4, 3, 64, 64), (2, 3, 224, 224)]),
        'spherenet20': dict(heads=[('age', 5), ('face_verification', 10)], train=(4, 3, 112, 112), evals=[(4, 3, 112, 112)])}
STEP_DATASET = {'resnet50': 't1', 'spherenet20': 'age'}
X_SEED, T_SEED, NOISE_SEED, IDX_SEED = 100, 200, 97, 1000
# The band is the largest distance over TWINS perturbed repetitions, not one: whether an element of a PReLU / ReLU input that lies inside
# the forward round-off takes the other side of zero is a yes / no event per repetition, and one such element moves every gradient below
# it by ~1e-3 of its scale (the reference's own fp32 and fp64 SphereNet-20 gradients of step 0 differ by 1.1e-2 in conv4_1 and 1.1e-3 to
# 1.8e-3 in the 17 layers below it, 6e-7 above it).  A single repetition without such an event gives a band of one ulp of the weights.
TWINS = 8


def crc(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return zlib.crc32(np.ascontiguousarray(t).tobytes())


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


def batch_x(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def batch_t(n, classes, seed):
    return torch.randint(0, classes, (n,), generator=torch.Generator().manual_seed(seed))


def build(arch):
    torch.manual_seed(SEED)
    net = packnet_models.__dict__[arch](dataset_history=[], dataset2num_classes={})
    for dataset, n in NETS[arch]['heads']:
        net.add_dataset(dataset, n)
    return net


def covered(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear)) and 'classifiers' not in n]


def manager(arch, net, dataset, mode='finetune', val=None):
    net.set_dataset(dataset)
    model = Wrap(net)
    masks = {n: torch.ByteTensor(m.weight.data.size()).fill_(0) for n, m in covered(model)}
    info = {dataset: {k: {} for k in ('conv_bias', 'bn_layer_running_mean', 'bn_layer_running_var', 'bn_layer_weight', 'bn_layer_bias',
                                      'fc_bias', 'prelu_layer_weight')}}
    args = types.SimpleNamespace(dataset=dataset, cuda=False, weight_decay=4e-5, mode=mode,
                                 checkpoint_format='{save_folder}/checkpoint-{epoch}.pth.tar')
    return model, masks, Manager(args, model, info, masks, None, val)


# --------------------------------------------------------------------------
def gen_topology():
    topo = {'torch': torch.__version__, 'seed': SEED}
    arrs = {}
    for arch, cfg in NETS.items():
        net = build(arch)
        net.set_dataset(cfg['heads'][0][0])
        topo[arch] = {'heads': [list(h) for h in cfg['heads']],
                      'modules': [[n, type(m).__name__] for n, m in net.named_modules()],
                      'state': [[k, list(v.shape), crc(v)] for k, v in net.state_dict().items()],
                      'covered': [[n, m.weight.numel()] for n, m in covered(Wrap(net))]}
        net.eval()
        for i, shape in enumerate(cfg['evals']):
            x = batch_x(shape, X_SEED + i)
            arrs.update({'%s/eval%d/shape' % (arch, i): np.array(shape), '%s/eval%d/x_seed' % (arch, i): X_SEED + i,
                         '%s/eval%d/x_crc' % (arch, i): crc(x)})
            for dataset, _ in cfg['heads']:
                net.set_dataset(dataset)
                with torch.no_grad():
                    out = net(x)
                if isinstance(out, tuple):                       # the A-Softmax head: (|x| cos, |x| phi)
                    arrs['%s/eval%d/%s/cos' % (arch, i, dataset)], arrs['%s/eval%d/%s/phi' % (arch, i, dataset)] = out
                    arrs['%s/eval%d/%s/embeddings' % (arch, i, dataset)] = net.forward_to_embeddings(x).detach()
                else:
                    arrs['%s/eval%d/%s/logits' % (arch, i, dataset)] = out
        del net
    save('packnet_nets_topology', **arrs)
    with open(os.path.join(OUT, 'packnet_nets_topology.json'), 'w') as f:
        json.dump(topo, f, indent=0)
    print('wrote packnet_nets_topology.json')


# --------------------------------------------------------------------------
class KthRecorder(object):
    """Records (k, value) of every Tensor.kthvalue call: the reference's own cutoff rank and value (utils/packnet_prune.py:29-30)."""

    def __enter__(self):
        self.calls, self.orig = [], torch.Tensor.kthvalue
        rec = self

        def kthvalue(t, k, *a, **kw):
            r = rec.orig(t, k, *a, **kw)
            rec.calls.append((int(k), float(r[0])))
            return r
        torch.Tensor.kthvalue = kthvalue
        return self

    def __exit__(self, *a):
        torch.Tensor.kthvalue = self.orig


def gen_prune():
    arrs = {}
    for arch in NETS:
        net = build(arch)
        model, masks, mgr = manager(arch, net, STEP_DATASET[arch])
        mgr.pruner.make_finetuning_mask()
        with KthRecorder() as rec:
            mgr.one_shot_prune(PRUNE)
        layers = covered(model)
        assert len(rec.calls) == len(layers)
        arrs['%s/layers' % arch] = np.array([n for n, _ in layers])
        arrs['%s/k' % arch] = np.array([k for k, _ in rec.calls], dtype=np.int64)
        arrs['%s/cutoff' % arch] = np.array([v for _, v in rec.calls], dtype=np.float32)
        arrs['%s/released' % arch] = np.array([int((masks[n] == 0).sum()) for n, _ in layers], dtype=np.int64)
        arrs['%s/mask_crc' % arch] = np.array([crc(masks[n]) for n, _ in layers], dtype=np.int64)
        arrs['%s/weight_crc' % arch] = np.array([crc(m.weight.data) for _, m in layers], dtype=np.int64)
        arrs['%s/ratio' % arch] = PRUNE
        del net
    save('packnet_nets_prune', **arrs)


# --------------------------------------------------------------------------
def sample_indices(layers):
    return [torch.randperm(m.weight.numel(), generator=torch.Generator().manual_seed(IDX_SEED + i))[:SAMPLE] for i, (_, m) in enumerate(layers)]


def run_steps(arch, noisy):
    # noisy: 0 for the run the fixture records, else the number of the perturbed twin (its own noise stream)
    """The reference Manager from the seed: claim, 3 train steps, validate, prune, 2 retrain steps, validate."""
    cfg = NETS[arch]
    dataset = STEP_DATASET[arch]
    classes = dict(cfg['heads'])[dataset]
    shape = cfg['train']
    gn = torch.Generator().manual_seed(NOISE_SEED + noisy)

    def xin(seed):
        x = batch_x(shape, seed)
        return x * (1 + 1e-6 * torch.randn(x.shape, generator=gn)) if noisy else x
    net = build(arch)
    val = (xin(X_SEED + 50), batch_t(shape[0], classes, T_SEED + 50))
    model, masks, mgr = manager(arch, net, dataset, val=[val])
    layers = covered(model)
    idx = sample_indices(layers)
    logits, losses = [], []
    model.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
    crit = mgr.criterion
    mgr.criterion = lambda o, t: (lambda l: (losses.append(float(l)), l)[1])(crit(o, t))
    active = '.{}.'.format(net.datasets.index(dataset))
    params = [p for n, p in model.named_parameters() if 'classifiers' not in n or active in n]
    out = {'loss': [], 'logits': [], 'stats': [], 'w': [], 'val_logits': [], 'val_acc': [], 'val_stats': []}

    def stats():
        return [mgr.pruner.calculate_sparsity(), mgr.pruner.calculate_curr_task_ratio(), mgr.pruner.calculate_zero_ratio()]

    def phase(nsteps, first):
        sgd = torch.optim.SGD(params, lr=LR, weight_decay=0.0, momentum=0.9, nesterov=True)
        opts = Optimizers()
        opts.add(sgd, LR)
        for s in range(first, first + nsteps):
            mgr.train_loader = [(xin(X_SEED + 10 + s), batch_t(shape[0], classes, T_SEED + 10 + s))]
            mgr.train(opts, s, [LR])
            out['loss'].append(losses[-1])
            out['logits'].append(logits[-1])
            out['stats'].append(stats())
            out['w'].append(torch.cat([m.weight.data.reshape(-1)[i] for (_, m), i in zip(layers, idx)]))
        out['val_acc'].append(mgr.validate(first + nsteps - 1))
        out['val_logits'].append(logits[-1])
        out['val_stats'].append(stats())

    mgr.pruner.make_finetuning_mask()
    phase(3, 0)
    mgr.one_shot_prune(PRUNE)
    out['stats_after_prune'] = stats()
    out['owner'] = torch.cat([masks[n].reshape(-1)[i] for (n, _), i in zip(layers, idx)])
    phase(2, 3)
    out['layers'] = [n for n, _ in layers]
    out['idx'] = idx
    return out


def gen_steps():
    for arch, cfg in NETS.items():
        a = run_steps(arch, 0)
        print('  %s losses %s' % (arch, ['%.4f' % v for v in a['loss']]))
        sizes = [len(i) for i in a['idx']]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        band, per_twin = {}, []
        for twin in range(1, TWINS + 1):
            b = run_steps(arch, twin)
            agree = (a['owner'] == b['owner']).float()
            one = {'loss': np.abs(np.array(a['loss']) - np.array(b['loss'])),
                   'logits': np.array([float((x - y).abs().max()) for x, y in zip(a['logits'], b['logits'])]),
                   'val_logits': np.array([float((x - y).abs().max()) for x, y in zip(a['val_logits'], b['val_logits'])]),
                   # (after the prune over the slots whose owner is the same in both runs: a weight next to the cutoff is released in one
                   #  run and kept in the other, which is a difference of its whole value -- those slots are counted in owner_moved)
                   'w': np.array([[float(((x - y).abs() * (agree if s >= 3 else 1))[offs[j]:offs[j + 1]].max()) for j in range(len(sizes))]
                                  for s, (x, y) in enumerate(zip(a['w'], b['w']))]),
                   'owner_moved': np.array(int((a['owner'] != b['owner']).sum()))}
            print('  %s twin %d: loss %s  w (worst layer) %s  owner bytes moved %d'
                  % (arch, twin, ['%.2g' % v for v in one['loss']], ['%.2g' % v for v in one['w'].max(axis=1)], one['owner_moved']))
            band = {k: np.maximum(band[k], v) if k in band else v for k, v in one.items()}
            per_twin.append(one)
        index = {'layers': np.array(a['layers']), 'offsets': offs, 'idx_seed': IDX_SEED, 'sample': SAMPLE,
                 'idx_crc': np.array([crc(i) for i in a['idx']], dtype=np.int64),
                 'dataset': STEP_DATASET[arch], 'classes': dict(cfg['heads'])[STEP_DATASET[arch]], 'lr': LR, 'ratio': PRUNE,
                 'shape': np.array(cfg['train']), 'x_seed0': X_SEED + 10, 't_seed0': T_SEED + 10, 'val_x_seed': X_SEED + 50,
                 'val_t_seed': T_SEED + 50, 'x_crc': np.array([crc(batch_x(cfg['train'], X_SEED + 10 + s)) for s in range(5)], dtype=np.int64),
                 'loss': np.array(a['loss']), 'logits': torch.stack(a['logits']), 'stats': np.array(a['stats']),
                 'val_logits': torch.stack(a['val_logits']), 'val_acc': np.array(a['val_acc']), 'val_stats': np.array(a['val_stats']),
                 'stats_after_prune': np.array(a['stats_after_prune']), 'owner': a['owner'], 'twins': TWINS}
        index.update({'band/' + k: v for k, v in band.items()})
        # what "one repetition is not a band" means, in figures: how many of the OTHER repetitions lie outside the band that the first
        # repetition alone would have given (any step, any layer), and by what factor at most
        for k in ('loss', 'logits', 'val_logits', 'w'):
            first = np.maximum(per_twin[0][k], np.finfo(np.float32).tiny)
            worst = [float((t[k] / first).max()) for t in per_twin[1:]]
            index['single_band/%s/outside' % k] = int(sum(w > 1.0 for w in worst))
            index['single_band/%s/worst_ratio' % k] = max(worst)
            print('  %s: %d of the %d other repetitions lie outside the first repetition\'s %s band, by up to x%.3g'
                  % (arch, index['single_band/%s/outside' % k], TWINS - 1, k, max(worst)))
        save('packnet_nets_steps_%s' % arch, **index)
        for s, w in enumerate(a['w']):
            save('packnet_nets_steps_%s_w%d' % (arch, s), w=w)


if __name__ == '__main__':
    gen_topology()
    gen_prune()
    gen_steps()
