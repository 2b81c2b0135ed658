#!/usr/bin/env python3
"""Forward, input gradient and weight gradient of SharableConv2d(groups=G) on ResNeXt- and MobileNet-style shapes, timed through
the PUBLIC layer only (so the same file runs on any commit: the grouped kernels where the library has them, one groups == 1
launch per group -- with autograd's slices and concatenation -- where it does not, or under CPG_NO_GROUPED=1).

HIP events around `--iters` back-to-back calls, `--warmup` untimed calls first, the median of `--reps` such rounds.  One JSON line per
shape: ms per pass, algorithmic GFLOP (2 N K OH OW (C/G) R S) and bytes (x + y + w, fp32), and the TFLOP/s and GB/s they imply.

    python tools/grouped_bench.py [--batch 256] [--reps 5] [--iters 3] [--warmup 2] [--only SUBSTRING] [--tag NAME]
                                  [--sweep] [--wide-min N] [--all-grouped]

--sweep times 256 -> 256 channels @28 x 28 at 4 ... 64 channels per group (and a few shapes between and beside those) instead, and --wide-min sets the library's
CPG_GROUPED_WIDE_MIN (1: every shape on the MFMA kernels, a large number: every shape on the direct kernels) -- together they
measure where the boundary between the two kernel families belongs.  --all-grouped lifts the layer's rule that keeps 3x3 s1 p1 layers
with wide groups on the per-group path (layers.GROUPED_PER_GROUP_MIN), so that the grouped kernels are timed on those shapes too; a tree
without that rule ignores it.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpg_amd.models import layers as nl          # noqa: E402

# name, C, K, H, k, stride, pad, groups
SHAPES = [
    ('resnext g4 128 @56', 128, 128, 56, 3, 1, 1, 4),
    ('resnext g4 256 @28', 256, 256, 28, 3, 1, 1, 4),
    ('resnext g4 512 @14', 512, 512, 14, 3, 1, 1, 4),
    ('resnext g4 1024 @7', 1024, 1024, 7, 3, 1, 1, 4),
    ('32x4d 128 g32 @56', 128, 128, 56, 3, 1, 1, 32),
    ('dw3 32 @112 s1', 32, 32, 112, 3, 1, 1, 32),
    ('dw3 32 @112 s2', 32, 32, 112, 3, 2, 1, 32),
    ('dw3 128 @56 s1', 128, 128, 56, 3, 1, 1, 128),
    ('dw3 128 @56 s2', 128, 128, 56, 3, 2, 1, 128),
    ('dw3 512 @14 s1', 512, 512, 14, 3, 1, 1, 512),
    ('dw3 512 @14 s2', 512, 512, 14, 3, 2, 1, 512),
    ('dw5 240 @28 s1', 240, 240, 28, 5, 1, 2, 240),
]
# 256 -> 256 @28, 3x3: channels per group 4, 8, 16, 32, 64
SWEEP = [('sweep 256 @28 cg%d' % (256 // G), 256, 256, 28, 3, 1, 1, G) for G in (64, 32, 16, 8, 4)]
# between and beside the sweep's points: 192 -> 192 @28 at 12, 24 and 48 channels per group, and wide groups that are no 3x3 s1 p1 layer
# (stride 2, 1x1, 5x5), which the per-group path serves with the generic / pointwise kernels instead of the Winograd ones
SWEEP += [('extra 192 @28 cg%d' % (192 // G), 192, 192, 28, 3, 1, 1, G) for G in (16, 8, 4)]
SWEEP += [('extra 256 @28 s2 cg16', 256, 256, 28, 3, 2, 1, 16), ('extra 256 @28 s2 cg64', 256, 256, 28, 3, 2, 1, 4),
          ('extra 256 @28 1x1 cg64', 256, 256, 28, 1, 1, 0, 4), ('extra 128 @28 5x5 cg32', 128, 128, 28, 5, 1, 2, 4)]


def timed(fn, warmup, iters, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        rounds.append(s.elapsed_time(e) / iters)
    return statistics.median(rounds)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--only', default='', help='substring of the shape name')
    ap.add_argument('--sweep', action='store_true', help='the channels-per-group sweep instead of the shape list')
    ap.add_argument('--wide-min', type=int, default=None, help='set CPG_GROUPED_WIDE_MIN')
    ap.add_argument('--all-grouped', action='store_true', help='no per-group exception for wide 3x3 s1 p1 groups')
    ap.add_argument('--tag', default='', help='copied into every line (which build this is)')
    a = ap.parse_args()
    dev = 'cuda:0'
    if a.wide_min is not None:
        from cpg_amd import _lib
        _lib.set_option('CPG_GROUPED_WIDE_MIN', a.wide_min)
    if a.all_grouped and hasattr(nl, 'GROUPED_PER_GROUP_MIN'):
        nl.GROUPED_PER_GROUP_MIN = None
    for name, C, K, H, k, s, p, G in (SWEEP if a.sweep else SHAPES):
        if a.only and a.only not in name:
            continue
        torch.manual_seed(0)
        layer = nl.SharableConv2d(C, K, k, stride=s, padding=p, groups=G, bias=False).to(dev)
        layer.weight.data.normal_(0, 0.05)
        x = torch.randn(a.batch, C, H, H, device=dev)
        with torch.no_grad():
            y = layer(x)
        gy = torch.randn_like(y)
        OH = y.shape[2]

        def fwd():
            with torch.no_grad():
                layer(x)

        ms = {'fwd': timed(fwd, a.warmup, a.iters, a.reps)}
        # input gradient alone: the weight asks for no gradient; weight gradient alone: the input asks for none
        layer.weight.requires_grad_(False)
        xg = x.clone().requires_grad_(True)
        yg = layer(xg)
        ms['dgrad'] = timed(lambda: torch.autograd.grad(yg, xg, gy, retain_graph=True), a.warmup, a.iters, a.reps)
        del yg, xg
        layer.weight.requires_grad_(True)
        yw = layer(x)
        ms['wgrad'] = timed(lambda: torch.autograd.grad(yw, layer.weight, gy, retain_graph=True), a.warmup, a.iters, a.reps)
        del yw
        gflop = 2.0 * a.batch * K * OH * OH * (C // G) * k * k / 1e9
        nbytes = 4.0 * (x.numel() + y.numel() + layer.weight.numel())
        out = {'shape': name, 'tag': a.tag, 'batch': a.batch, 'C': C, 'K': K, 'H': H, 'k': k, 'stride': s, 'groups': G,
               'gflop': round(gflop, 3), 'mbytes': round(nbytes / 1e6, 2)}
        for pas, t in ms.items():
            out[pas + '_ms'] = round(t, 4)
            out[pas + '_tflops'] = round(gflop / t, 3)
            out[pas + '_gbs'] = round(nbytes / t / 1e6, 1)
        print(json.dumps(out), flush=True)
        del x, y, gy, layer
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
