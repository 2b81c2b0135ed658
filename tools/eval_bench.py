#!/usr/bin/env python3
"""Inference forward of a residual topology with its fused_bn switch on against off: FUSE_EVAL_BLOCKS for the ResNets
(profiles/resnet_eval_fuse.md), FUSE_EVAL_PRELU for --arch spherenet20 (profiles/spherenet_eval_fuse.md; 112 x 112),
FusedSequential.fuse_eval_pool for --arch vgg16 (profiles/vgg_eval_pool_fuse.md; VGG16-BN, the headline topology).

Full-width ResNet-50 (or --arch), model.eval() under torch.no_grad() at 224 x 224 -- Manager.validate's forward.  Both arms run in ONE
process, alternating window by window after both are warmed, so clock and allocator state are shared; a window is --forwards forwards
between two device events.  Per batch size one line, mean +- sample sd (min - max) of the windows per arm, and at the end one JSON
line with everything, plus the activation bytes per image each arm moves, computed from the layer shapes alone:
  off  every conv reads its input and writes its raw output; the BatchNorm pass behind it reads that back (+ the residual, in a block
       tail) and writes the activation;
  on   every conv behind the stem reads its input (+ the residual) and writes the activation.
SphereNet-20: "the pass behind it" is the PReLU pass (+ the unit's residual in the second pair of a unit); conv1_1 (3 input channels) has
no fused epilogue and runs conv + PReLU pass in both arms.
VGG16: every conv -> BatchNorm -> ReLU group is one kernel in both arms (reads its input, writes the activation) except the five in front
of a MaxPool2d(2, 2): off, the conv writes its raw output and the BatchNorm -> ReLU -> pool pass reads it back and writes a quarter of it;
on, one kernel reads the input and writes that quarter."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpg_amd.models as M  # noqa: E402
from cpg_amd.models import fused_bn  # noqa: E402
from cpg_amd.models import layers as nl  # noqa: E402


def byte_account(net, size):
    """Activation bytes read + written per image by the convs and the BatchNorm passes behind them, {'off': .., 'on': ..}, from the
    conv modules' input / output shapes (one image through the net on the device; weights and parameters not counted)."""
    shapes = []
    hooks = [m.register_forward_hook(lambda mod, inp, out, name=name: shapes.append((name, inp[0].numel(), out.numel())))
             for name, m in net.named_modules() if isinstance(m, nl.SharableConv2d)]
    was = fused_bn.FUSE_EVAL_BLOCKS
    fused_bn.FUSE_EVAL_BLOCKS = False           # (the hooks see the conv modules' own forward)
    try:
        with torch.no_grad():
            net(torch.zeros(1, 3, size, size, device=next(net.parameters()).device))
    finally:
        fused_bn.FUSE_EVAL_BLOCKS = was
        for h in hooks:
            h.remove()
    off = on = 0
    for name, n_in, n_out in shapes:
        tail = name.endswith('conv3')
        if name == 'conv1':                     # the stem: conv, then BatchNorm -> ReLU -> MaxPool2d(3, 2, 1) as one pass, in both arms
            both = n_in + n_out + n_out + n_out // 4
            off, on = off + both, on + both
            continue
        off += (n_in + n_out) + (n_out + (n_out if tail else 0) + n_out)
        on += n_in + (n_out if tail else 0) + n_out
    return {'off': 4 * off, 'on': 4 * on}


def byte_account_sphere(net, size):
    """The same account for SphereNet-20: conv -> PReLU pairs, the second pair of a residual unit also reads the unit's input."""
    shapes = []
    hooks = [m.register_forward_hook(lambda mod, inp, out, name=name: shapes.append((name, inp[0].numel(), out.numel())))
             for name, m in net.named_modules() if isinstance(m, nl.SharableConv2d)]
    was = getattr(fused_bn, 'FUSE_EVAL_PRELU', False)
    fused_bn.FUSE_EVAL_PRELU = False            # (the hooks see the conv modules' own forward)
    try:
        with torch.no_grad():
            net(torch.zeros(1, 3, size, size, device=next(net.parameters()).device))
    finally:
        fused_bn.FUSE_EVAL_PRELU = was
        for h in hooks:
            h.remove()
    off = on = 0
    for name, n_in, n_out in shapes:
        i = int(name.rsplit('_', 1)[1])
        res = n_out if i >= 3 and i % 2 == 1 else 0          # conv{s}_3, _5, ...: the unit's second pair
        pair = (n_in + n_out) + (n_out + res + n_out)
        off += pair
        on += pair if name == 'conv1_1' else n_in + res + n_out
    return {'off': 4 * off, 'on': 4 * on}


VGG16_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']


def byte_account_vgg(net, size):
    """The same account for VGG16's feature stack (see the module docstring), from the module list and the conv shapes."""
    mods = list(net.features.children())
    pooled = {id(m): isinstance(mods[i + 3], torch.nn.MaxPool2d) for i, m in enumerate(mods[:-3]) if isinstance(m, nl.SharableConv2d)}
    shapes = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: shapes.append((id(mod), inp[0].numel(), out.numel())))
             for m in mods if isinstance(m, nl.SharableConv2d)]
    was = fused_bn.FusedSequential.fuse_eval
    fused_bn.FusedSequential.fuse_eval = False  # (the hooks see the conv modules' own forward)
    try:
        with torch.no_grad():
            net(torch.zeros(1, 3, size, size, device=next(net.parameters()).device))
    finally:
        fused_bn.FusedSequential.fuse_eval = was
        for h in hooks:
            h.remove()
    off = on = 0
    for key, n_in, n_out in shapes:
        if pooled[key]:
            off += (n_in + n_out) + (n_out + n_out // 4)
            on += n_in + n_out // 4
        else:
            off, on = off + n_in + n_out, on + n_in + n_out
    return {'off': 4 * off, 'on': 4 * on}


def per_group(net, batch, size, forwards, windows):
    """--per-group (vgg16): every conv -> BatchNorm -> ReLU -> MaxPool2d(2, 2) group on its own, on a random input of the shape it sees in
    the network, switch on against off in alternating windows.  One row per group: ms per call of each arm."""
    mods = list(net.features.children())
    rows, x = [], torch.zeros(1, 3, size, size, device=next(net.parameters()).device)
    with torch.no_grad():
        i = 0
        while i < len(mods) and isinstance(mods[i], (nl.SharableConv2d, torch.nn.MaxPool2d)):
            if isinstance(mods[i], torch.nn.MaxPool2d):
                x, i = mods[i](x), i + 1
                continue
            pooled = isinstance(mods[i + 3], torch.nn.MaxPool2d)
            grp = fused_bn.FusedSequential(*mods[i:i + (4 if pooled else 3)]).eval()
            if pooled:
                xin = torch.randn(batch, *x.shape[1:], device=x.device)
                ms = {True: [], False: []}
                for w in range(windows + 1):                         # (window 0 warms both arms)
                    for switch in (True, False):
                        fused_bn.FusedSequential.fuse_eval_pool = switch
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        for _ in range(forwards):
                            grp(xin)
                        t1.record()
                        t1.synchronize()
                        if w:
                            ms[switch].append(t0.elapsed_time(t1) / forwards)
                rows.append({'group': '%d -> %d @ %d' % (mods[i].in_channels, mods[i].out_channels, x.shape[2]),
                             'on_ms': round(statistics.mean(ms[True]), 4), 'off_ms': round(statistics.mean(ms[False]), 4)})
                print('vgg16 batch %d group %-18s on %.3f ms  off %.3f ms (conv + BatchNorm/ReLU/pool pass)' % (
                    batch, rows[-1]['group'], rows[-1]['on_ms'], rows[-1]['off_ms']))
            fused_bn.FusedSequential.fuse_eval_pool = False
            x = grp(x)
            i += 4 if pooled else 3
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('--batches', type=int, nargs='+', default=[100, 256])
    ap.add_argument('--size', type=int, default=None, help='default: 224, spherenet20: 112')
    ap.add_argument('--forwards', type=int, default=10, help='forwards per timed window')
    ap.add_argument('--windows', type=int, default=12, help='windows per arm')
    ap.add_argument('--warmup', type=int, default=5, help='forwards per arm before the first window')
    ap.add_argument('--per-group', action='store_true', help='vgg16: also time each pooled group on its own, on against off')
    a = ap.parse_args()
    sphere, vgg = a.arch.startswith('spherenet'), a.arch == 'vgg16'
    # the switch and the object that holds it: a module attribute of fused_bn, or FusedSequential's class attribute
    SWITCH = 'FUSE_EVAL_PRELU' if sphere else 'fuse_eval_pool' if vgg else 'FUSE_EVAL_BLOCKS'
    holder = fused_bn.FusedSequential if vgg else fused_bn
    if a.size is None:
        a.size = 112 if sphere else 224
    dev = 'cuda:0'
    torch.manual_seed(1)
    kw = dict(dataset_history=[], dataset2num_classes={}, network_width_multiplier=1.0, shared_layer_info={})
    net = M.custom_vgg(VGG16_CFG, **kw) if vgg else getattr(M, a.arch)(**kw)
    net.add_dataset('t', 10)
    net.set_dataset('t')
    net = net.to(dev).eval()
    out = {'arch': a.arch, 'size': a.size, 'switch': SWITCH, 'forwards_per_window': a.forwards, 'windows_per_arm': a.windows, 'batches': {},
           'activation_bytes_per_image': (byte_account_sphere if sphere else byte_account_vgg if vgg else byte_account)(net, a.size)}

    def forward(x, switch):
        setattr(holder, SWITCH, switch)
        with torch.no_grad():
            return net(x)
    default = getattr(holder, SWITCH, None)     # (None: a tree without the switch -- both arms then run the one path it has)
    try:
        for batch in a.batches:
            x = torch.randn(batch, 3, a.size, a.size, device=dev)
            for switch in (True, False):
                for _ in range(a.warmup):
                    forward(x, switch)
            torch.cuda.synchronize()
            ms = {True: [], False: []}
            for _ in range(a.windows):
                for switch in (True, False):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.forwards):
                        forward(x, switch)
                    t1.record()
                    t1.synchronize()
                    ms[switch].append(t0.elapsed_time(t1) / a.forwards)
            row = {}
            for switch, label in ((True, 'on'), (False, 'off')):
                v = ms[switch]
                row[label] = {'mean_ms': round(statistics.mean(v), 4), 'sd_ms': round(statistics.stdev(v), 4), 'min_ms': round(min(v), 4),
                              'max_ms': round(max(v), 4)}
                print('%s batch %d %s %-3s: %.3f +- %.3f ms per forward (%.3f - %.3f), %.0f img/s' % (
                    a.arch, batch, SWITCH, label, row[label]['mean_ms'], row[label]['sd_ms'], row[label]['min_ms'], row[label]['max_ms'],
                    batch / row[label]['mean_ms'] * 1e3))
            gain = row['off']['mean_ms'] - row['on']['mean_ms']
            row['gain_ms'] = round(gain, 4)
            row['gain_over_2sd'] = bool(gain > 2 * max(row['on']['sd_ms'], row['off']['sd_ms']))
            row['off_spread_ms'] = round(row['off']['max_ms'] - row['off']['min_ms'], 4)      # the off arm's own window-to-window spread
            row['gain_over_off_spread'] = bool(gain > row['off_spread_ms'])
            if vgg and a.per_group:
                row['groups'] = per_group(net, batch, a.size, a.forwards, a.windows)
            out['batches'][str(batch)] = row
    finally:
        if default is None:
            delattr(holder, SWITCH)
        else:
            setattr(holder, SWITCH, default)
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
