#!/usr/bin/env python3
"""Measurements behind profiles/packnet.md, all in one process on the GPU, arms alternating.

1. The optimizer part of a PackNet step over the covered layers of vgg16_bn_cifar100 (15 layers, 33.6 M weights) and vgg16_bn (134 M), three
   ways:  (a) cpg_sgd_route_zero_step_multi -- the fused pass;  (b) cpg_sgd_route_step_multi + one cpg_zero_pruned per layer -- the best
   composition of the entry points that existed before it;  (c) the reference's op sequence on existing kernels: cpg_route_grads per layer
   -> torch.optim.SGD(momentum, nesterov) -> cpg_zero_pruned per layer.
2. cpg_rank_prune_zero against cpg_rank_prune + cpg_zero_pruned over the same layers.
3. Images per second of a whole PackNet task (claim, finetune epochs, validate, one-shot prune, retrain epochs, a validate per epoch) of
   vgg16_bn_cifar100 on synthetic data at batch 32 (the reference's) and 256.
4. (--nets) The train step of the PackNet ResNet-50 (224x224, cross-entropy) and SphereNet-20 (112x112, AngleLoss on the face head) as
   utils.packnet_manager.Manager.train runs it -- forward, loss, backward, the fused PackNetSGD step --, alternating with the CPG task-1
   step of the same topology exactly as tools/net_bench.py runs it (masked layers without piggymask, cross-entropy, torch.optim.SGD).

Times are device events around `--inner` repetitions of an arm, ending in a synchronise; every arm is warmed first; `--reps` windows per
arm, alternating.  Bytes per element are computed from the shapes and the owner mask (what the passes must move), not measured.

    python tools/packnet_bench.py [--out packnet_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpg_amd.packnet_models as pm  # noqa: E402
from cpg_amd import _lib as L  # noqa: E402
from cpg_amd.baselines import BaselineSession  # noqa: E402

HYPER = (2, 4e-5, 1e-4, 0.9, 1)          # cur, weight decay, lr, momentum, nesterov
COPY_TBS = 6.3                            # the device's measured copy rate


def layer_sizes(arch):
    with torch.device('meta'):
        net = getattr(pm, arch)(pretrained=True, dataset_history=[], dataset2num_classes={})
    return [m.weight.numel() for n, m in net.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear)) and 'classifiers' not in n]


def window(fn, inner, before=None):
    if before is not None:
        before()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def alternate(arms, reps, inner, before=None):
    for fn in arms.values():
        window(fn, 2, before)
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms[k].append(window(fn, inner, before))
    return {k: dict(mean=statistics.mean(v), stdev=statistics.stdev(v), min=min(v), max=max(v), windows=len(v)) for k, v in ms.items()}


def optimizer_arms(sizes, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    ws = [nn.Parameter(torch.randn(n, generator=g, device=dev) * 0.05) for n in sizes]
    gs = [torch.randn(n, generator=g, device=dev) * 1e-3 for n in sizes]
    owners = [torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.uint8) for n in sizes]
    bufs = [torch.zeros(n, device=dev) for n in sizes]
    for w, gr in zip(ws, gs):
        w.grad = gr
    sgd = torch.optim.SGD(ws, lr=HYPER[2], momentum=HYPER[3], nesterov=True)
    sgd.step()                                                   # creates torch's momentum buffers
    s = L.stream_ptr()
    rows = [(w.data_ptr(), gr.data_ptr(), b.data_ptr(), o.data_ptr(), w.numel()) for w, gr, b, o in zip(ws, gs, bufs, owners)]
    items = (L.SgdItem * len(rows))(*rows)

    def fused():
        L.call('cpg_sgd_route_zero_step_multi', items, len(rows), *HYPER, 0, s)

    def step_zero():
        L.call('cpg_sgd_route_step_multi', items, len(rows), *HYPER, 0, s)
        for w_, _, _, o_, n_ in rows:
            L.call('cpg_zero_pruned', w_, o_, n_, s)

    def unfused():
        for w_, g_, _, o_, n_ in rows:
            L.call('cpg_route_grads', g_, w_, o_, HYPER[0], HYPER[1], None, L.MODE_FINETUNE, n_, s)
        sgd.step()
        for w_, _, _, o_, n_ in rows:
            L.call('cpg_zero_pruned', w_, o_, n_, s)

    pristine = [t.detach().clone() for t in ws + gs]

    def restore():      # torch's foreach Nesterov update reuses .grad in place: every window starts from the same weights and gradients
        with torch.no_grad():
            for a, b in zip(ws + gs, pristine):
                a.copy_(b)

    free = sum(int((o == 0).sum()) for o in owners) / float(sum(sizes))
    return {'fused': fused, 'step_multi+zero': step_zero, 'route+torch_sgd+zero': unfused}, free, restore


def prune_arms(sizes, dev):
    g = torch.Generator(device=dev).manual_seed(2)
    w0 = [torch.randn(n, generator=g, device=dev) for n in sizes]
    o0 = [torch.randint(1, 3, (n,), generator=g, device=dev, dtype=torch.uint8) for n in sizes]
    w, o = [t.clone() for t in w0], [t.clone() for t in o0]
    res = torch.zeros(len(sizes), L.PRUNE_RESULT_BYTES // 8, dtype=torch.int64, device=dev)
    ws, nbytes = L.workspace(L.lib().cpg_rank_prune_workspace_bytes(), dev)
    s = L.stream_ptr()

    def restore():
        for a, b in zip(w + o, w0 + o0):
            a.copy_(b)

    def run(entry, zero):
        for i, (a, b) in enumerate(zip(w, o)):
            L.call(entry, L.dptr(a), L.dptr(b, torch.uint8), 2, 0.6, a.numel(), ctypes.c_void_p(res[i].data_ptr()), L.dptr(ws), nbytes, s)
            if zero:
                L.call('cpg_zero_pruned', L.dptr(a), L.dptr(b, torch.uint8), a.numel(), s)
    return {'rank_prune_zero': lambda: run('cpg_rank_prune_zero', False), 'rank_prune+zero_pruned': lambda: run('cpg_rank_prune', True)}, restore


def task_rate(batch, dev, train_batches, val_batches, epochs, prune_epochs):
    g = torch.Generator(device=dev).manual_seed(3)
    train = [(torch.randn(batch, 3, 32, 32, generator=g, device=dev), torch.randint(0, 5, (batch,), generator=g, device=dev))
             for _ in range(train_batches)]
    val = train[:val_batches]
    out = {}
    for tag, tb, e, pe in (('warm-up', 2, 1, 1), ('timed', train_batches, epochs, prune_epochs)):
        sess = BaselineSession(arch='vgg16_bn_cifar100', device=dev, seed=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.packnet_task('synthetic', 5, train[:tb], val, epochs=e, one_shot_prune_perc=0.6, prune_epochs=pe, min_train_acc=-1.0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = tb * (e + pe)
        images = batch * (steps + len(val) * (e + pe + 1))
        out = dict(batch=batch, train_steps=steps, validates=e + pe + 1, val_batches=len(val), seconds=dt, images=images,
                   images_per_s=images / dt, train_images_per_s_incl_everything=batch * steps / dt)
        del sess
        torch.cuda.empty_cache()
    return out


def net_step_arms(arch, batch, dev):
    import types
    import torch.nn.functional as F
    import cpg_amd.models as M
    from cpg_amd.driver import _Plain
    from cpg_amd.utils import Optimizers
    from cpg_amd.utils.fused_sgd import PackNetSGD
    from cpg_amd.utils.packnet_manager import Manager, make_masks
    face = arch == 'spherenet20'
    shape = (batch, 3, 112, 112) if face else (batch, 3, 224, 224)
    x = torch.randn(*shape, device=dev)
    t = torch.randint(0, 10, (batch,), device=dev)

    def packnet_arm(dataset):
        # the body of Manager.train without its metrics
        torch.manual_seed(1)
        net = pm.factory(arch)(dataset_history=[], dataset2num_classes={})
        net.add_dataset(dataset, 10)
        net.set_dataset(dataset)
        model = _Plain(net.to(dev)).train()
        args = types.SimpleNamespace(dataset=dataset, mode='finetune', weight_decay=4e-5, cuda=True, progress=False, log_path=None)
        mgr = Manager(args, model, {}, make_masks(model), None, None)
        mgr.pruner.make_finetuning_mask()
        opts = Optimizers()
        opts.add(PackNetSGD(list(model.parameters()), pruner=mgr.pruner, lr=1e-3, momentum=0.9, nesterov=True, mode='fused'), 1e-3)

        def packnet():
            opts.zero_grad()
            loss = mgr.criterion(model(x), t)
            loss.backward()
            mgr.pruner.do_weight_decay_and_make_grads_zero()
            opts.step()
            mgr.pruner.make_pruned_zero()
        return packnet
    arms = {'packnet_step': packnet_arm('face_verification' if face else 't')}
    if face:        # the comparator's head and loss on the PackNet trunk: what of a difference is the A-Softmax head (stock torch ops)
        arms['packnet_step(plain head, CE)'] = packnet_arm('t')
    # the comparator: tools/net_bench.py's step
    torch.manual_seed(1)
    cpg = getattr(M, arch)(dataset_history=[], dataset2num_classes={}, network_width_multiplier=1.0, shared_layer_info={})
    cpg.add_dataset('t', 10)
    cpg.set_dataset('t')
    cpg = cpg.to(dev).train()
    sgd = torch.optim.SGD(cpg.parameters(), lr=1e-3, momentum=0.9)

    def cpg_task1():
        sgd.zero_grad(set_to_none=True)
        F.cross_entropy(cpg(x), t).backward()
        sgd.step()
    arms['cpg_task1_step(net_bench)'] = cpg_task1
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-task', action='store_true')
    ap.add_argument('--nets', action='store_true', help='only section 4: the ResNet-50 / SphereNet-20 steps')
    ap.add_argument('--batch', type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('packnet_bench: needs the GPU (a timing anywhere else says nothing)')
    dev = 'cuda:0'
    result = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'inner': a.inner, 'optimizer': {}, 'prune': {}, 'task': [], 'nets': {}}
    for arch in ('resnet50', 'spherenet20') if a.nets else ():
        ms = alternate(net_step_arms(arch, a.batch, dev), a.reps, a.inner)
        for k, v in ms.items():
            v['images_per_s'] = a.batch / (v['mean'] * 1e-3)
            print('%-12s batch %d %-28s %8.2f ms +- %.2f (min %.2f max %.2f, %d windows)  %.0f img/s'
                  % (arch, a.batch, k, v['mean'], v['stdev'], v['min'], v['max'], v['windows'], v['images_per_s']), flush=True)
        result['nets'][arch] = dict(batch=a.batch, arms=ms)
        torch.cuda.empty_cache()
    for arch in () if a.nets else ('vgg16_bn_cifar100', 'vgg16_bn'):
        sizes = layer_sizes(arch)
        n = sum(sizes)
        arms, free, restore = optimizer_arms(sizes, dev)
        ms = alternate(arms, a.reps, a.inner, before=restore)
        layers = len(sizes)
        # what each arm must move per element: fp32 w / g / momentum, one owner byte; the separate zeroing pass reads the owner byte again
        # and rewrites the 16-byte groups that hold a free slot; torch's foreach Nesterov step is four passes (mul_, add_, add, add_)
        quad_free = 1.0 - (1.0 - free) ** 4
        one_pass = 13.0 + 12.0            # read w, g, momentum and the owner byte; write w, g, momentum
        nbytes = {'fused': one_pass, 'step_multi+zero': one_pass + 1.0 + 4.0 * quad_free, 'route+torch_sgd+zero': 13.0 + 44.0 + 1.0 + 4.0 * quad_free}
        launches = {'fused': (layers + 47) // 48, 'step_multi+zero': (layers + 47) // 48 + layers, 'route+torch_sgd+zero': '%d + torch foreach' % (2 * layers)}
        for k, v in ms.items():
            v.update(bytes_per_element=nbytes[k], tb_per_s=nbytes[k] * n / (v['mean'] * 1e-3) / 1e12, launches=launches[k])
            v['share_of_copy_rate'] = v['tb_per_s'] / COPY_TBS
            print('%-18s %-22s %8.3f ms +- %.3f (min %.3f max %.3f, %d windows)  %.1f B/elem  %.2f TB/s  launches %s'
                  % (arch, k, v['mean'], v['stdev'], v['min'], v['max'], v['windows'], nbytes[k], v['tb_per_s'], launches[k]), flush=True)
        result['optimizer'][arch] = dict(layers=layers, weights=n, free_fraction=free, arms=ms)
        del arms, restore
        torch.cuda.empty_cache()
        arms, restore = prune_arms(sizes, dev)
        ms = alternate(arms, a.reps, 1, before=restore)
        for k, v in ms.items():
            print('%-18s %-22s %8.3f ms +- %.3f (min %.3f max %.3f, %d windows)' % (arch, k, v['mean'], v['stdev'], v['min'], v['max'], v['windows']),
                  flush=True)
        result['prune'][arch] = dict(layers=layers, weights=n, arms=ms)
        del arms, restore
        torch.cuda.empty_cache()
    if not a.skip_task and not a.nets:
        for batch, tb in ((32, 60), (256, 30)):
            r = task_rate(batch, dev, tb, 5, 2, 1)
            print('task batch %d: %.2f s, %d train steps, %.0f images/s over the whole task' % (batch, r['seconds'], r['train_steps'], r['images_per_s']),
                  flush=True)
            result['task'].append(r)
    line = json.dumps({'packnet_bench': result})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
