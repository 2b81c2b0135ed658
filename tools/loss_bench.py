#!/usr/bin/env python3
"""In-process A/B of args.fused_loss (cpg_amd/models/losses.py) on whole train steps: after warming both variants, alternates
Manager.train epochs of --steps steps with the option off and on, --reps times, and prints ms/step of each (median, min, max over the
epochs) plus one JSON line.  Workloads: SphereNet-20 at 112x112, batch 256, face_verification with 4 630 classes (AngleLinear +
AngleLoss), and VGG16 at 224x224, batch 256, 5 classes (cross-entropy).

    python tools/loss_bench.py                       # both workloads, A/B
    python tools/loss_bench.py --arch spherenet20 --only on --reps 1      # one variant alone (the command a kernel trace wraps)

One model, one optimizer and one Manager per workload: the variants differ in Manager.fused_loss and the criterion object only, so they
train the same weights in turn.  Times are device events around an epoch, which ends in a synchronise.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpg_amd.models as M  # noqa: E402
from cpg_amd.driver import default_args  # noqa: E402
from cpg_amd.models import layers as nl  # noqa: E402
from cpg_amd.utils import Optimizers  # noqa: E402
from cpg_amd.utils.fused_sgd import MaskedSGD  # noqa: E402
from cpg_amd.utils.manager import Manager, make_criterion  # noqa: E402

VGG_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']
WORKLOADS = {'spherenet20': dict(size=112, dataset='face_verification', classes=4630),
             'vgg16': dict(size=224, dataset='task1', classes=5)}


class _Wrap(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.module = m

    def forward(self, x):
        return self.module(x)


def build(arch, batch, steps):
    w = WORKLOADS[arch]
    torch.manual_seed(1)
    kw = dict(dataset_history=[], dataset2num_classes={}, network_width_multiplier=1.0, shared_layer_info={})
    net = M.spherenet20(**kw) if arch == 'spherenet20' else M.custom_vgg(VGG_CFG, **kw)
    net.add_dataset(w['dataset'], w['classes'])
    net.set_dataset(w['dataset'])
    model = _Wrap(net.cuda())
    masks = {n: torch.ones(m.weight.shape, dtype=torch.uint8, device='cuda') for n, m in model.named_modules()
             if isinstance(m, (nl.SharableConv2d, nl.SharableLinear))}
    x = torch.randn(batch, 3, w['size'], w['size'], device='cuda')
    t = torch.randint(0, w['classes'], (batch,), device='cuda')
    args = default_args(mode='finetune', dataset=w['dataset'])
    mgr = Manager(args, model, {}, masks, [(x, t)] * steps, None, 0, 0)
    opts = Optimizers()
    opts.add(MaskedSGD(list(model.parameters()), pruner=mgr.pruner, lr=1e-4, momentum=0.9, nesterov=True), 1e-4)
    criteria = {False: mgr.criterion, True: make_criterion(default_args(dataset=w['dataset'], fused_loss=True))}
    return mgr, opts, criteria


def epoch(mgr, opts, criteria, fused):
    mgr.fused_loss, mgr.criterion = fused, criteria[fused]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    mgr.train(opts, 0, [1e-4], 0)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / len(mgr.train_loader)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', choices=sorted(WORKLOADS), action='append')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20, help='steps per Manager.train epoch')
    ap.add_argument('--reps', type=int, default=7, help='epochs per variant')
    ap.add_argument('--only', choices=['off', 'on'], help='run one variant alone (for a kernel trace)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('loss_bench: needs the GPU (a timing anywhere else says nothing)')
    variants = [False, True] if a.only is None else [a.only == 'on']
    result = {}
    for arch in a.arch or sorted(WORKLOADS):
        mgr, opts, criteria = build(arch, a.batch, a.steps)
        for v in variants:                                     # warm-up: every shape, both variants
            epoch(mgr, opts, criteria, v)
        ms = {v: [] for v in variants}
        for _ in range(a.reps):
            for v in variants:
                ms[v].append(epoch(mgr, opts, criteria, v))
        result[arch] = {}
        for v in variants:
            r = sorted(ms[v])
            name = 'fused_loss on' if v else 'fused_loss off'
            result[arch][name] = dict(median=round(r[len(r) // 2], 4), min=round(r[0], 4), max=round(r[-1], 4), epochs=len(r))
            print('%-12s %-15s median %.3f ms/step  (min %.3f, max %.3f over %d epochs of %d steps)'
                  % (arch, name, r[len(r) // 2], r[0], r[-1], len(r), a.steps), flush=True)
        del mgr, opts, criteria
        torch.cuda.empty_cache()
    print(json.dumps({'loss_bench': result, 'batch': a.batch, 'steps': a.steps}))


if __name__ == '__main__':
    main()
