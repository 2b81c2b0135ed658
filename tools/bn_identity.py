#!/usr/bin/env python3
"""Output fingerprint of every status-returning entry point of csrc/bn_kernels.hip, for refactors that must not move a bit: each
entry point is called through cpg_amd._lib on seeded inputs and one line `entry case sha256` is printed per (entry point, case), the
hash taken over all output buffers of the call.  CPG_HIP_LIB selects the library, so two builds are compared by running this once per
library in fresh processes and comparing the two lists line by line (profiles/bn_pass_refactor.md):

    for L in parent.so new.so; do CPG_HIP_LIB=$PWD/$L python tools/bn_identity.py > $L.txt; done; cmp parent.so.txt new.so.txt

The shapes are the smallest that reach each branch of each kernel; the branch is named beside the shape.  `--no-large` leaves out
the three cases of 134 - 540 MB a tensor (nothing smaller reaches the 64-visit flush of the flattened walk).
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cpg_amd import _lib as L

DEV = 'cuda:0'
EPS, MOM = 1e-5, 0.1
gen = torch.Generator(device=DEV)

# plain passes (k_bn_stats, k_bn_apply, k_bn_bwd_reduce, k_bn_bwd_apply, k_prelu_*): walk_planes of the reductions and the plane groups
PLAIN = {
    'vec-large': (2, 3, 128, 128),      # float4 large-plane walk (>= 16 * 256 float4s a plane); block-per-plane groups (HW >= 4096)
    'scalar-large': (2, 3, 65, 65),     # scalar large-plane walk (HW no multiple of 4); block-per-plane groups
    'vec-flush16': (1, 2, 256, 256),    # 16 trips of the float4 large-plane walk: the flush inside it
    'scalar-flush16': (1, 2, 129, 129),  # 16 trips of the scalar large-plane walk
    'vec-small': (2, 3, 6, 10),         # flattened small-plane walk, float4; wave-per-plane groups (HW < 4096)
    'scalar-small': (3, 5, 7, 9),       # flattened small-plane walk, scalar; wave-per-plane groups
    'three-slices': (10, 700, 4, 4),    # three image slices per channel (4, 4 and 2 images)
}
LARGE = {'flush64': (34, 2048, 21, 23)}  # one slice of >= 64 * 256 items of planes under 4096: the 64-visit flush of the flattened walk
POOL2 = {
    'wave': (2, 3, 8, 8),               # fewer than 1024 windows: wave-per-plane groups, flattened reduction walk
    'block': (2, 3, 64, 64),            # 1024 windows: block-per-plane groups
    'large': (1, 2, 192, 192),          # 9216 windows: the large-plane reduction walk with its remainder loop
    'flush16': (1, 2, 256, 256),        # 16 384 windows: 16 trips of the large-plane reduction walk
}
POOL2_LARGE = {'flush64': (34, 2048, 44, 44)}   # 34 * 484 windows in one slice: the 64-visit flush of the flattened reduction walk
POOL3 = {
    'pairs-1strip': (2, 8, 16, 16),     # even W: rows as 8-byte pairs; OH = 8: one strip
    'scalar-1strip': (2, 8, 16, 15),    # odd W: the scalar path, elements past the edge
    'pairs-strips': (2, 4, 40, 40),     # OH = 20: three strips, the last one short
    'scalar-strips': (2, 3, 33, 31),    # odd H and W over several strips; staging rows that are no multiple of four
}


def rnd(*shape, seed, scale=1.0, shift=0.0, off=0):
    """Seeded normal values on the device; off = 1 puts the first element 4 bytes past a 16-byte boundary."""
    gen.manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + off, dtype=torch.float32, device=DEV)
    v = buf[off:].view(shape)
    v.copy_(torch.randn(shape, generator=gen, device=DEV) * scale + shift)
    return v


def out(*shape, off=0, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= s
    return torch.zeros(n + off, dtype=dtype, device=DEV)[off:].view(shape)


def report(entry, case, *outputs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outputs:
        h.update(t.contiguous().cpu().numpy().tobytes())
    print('%-30s %-44s %s' % (entry, case, h.hexdigest()), flush=True)


P, S = L.dptr, L.stream_ptr


def channel_params(C, seed):
    gamma = rnd(C, seed=seed, scale=0.3, shift=1.0)
    beta = rnd(C, seed=seed + 1, scale=0.3)
    return gamma, beta


def batch_stats(x):
    var, mean = torch.var_mean(x, dim=(0, 2, 3), unbiased=False)
    return mean.contiguous(), torch.rsqrt(var + EPS).contiguous()


def ws_for(N, C, HW):
    return L.workspace(L.lib().cpg_bn_workspace_bytes(N, C, HW), DEV)


def plain(tag, shape, off=0, every=True):
    """All plain BatchNorm entry points on one shape.  every=False: the training forward and one backward of each family only."""
    N, C, H, W = shape
    HW = H * W
    case = '%s %dx%dx%dx%d%s' % (tag, N, C, H, W, ' +4B' if off else '')
    x = rnd(*shape, seed=1, scale=2.0, shift=0.5, off=off)
    gy = rnd(*shape, seed=2, off=off)
    res = rnd(*shape, seed=3, off=off)
    gamma, beta = channel_params(C, 4)
    ws, nb = ws_for(N, C, HW)
    for relu in ((1, 0) if every else (1,)):
        for running in ((True, False) if every else (True,)):
            rm, rv = (rnd(C, seed=6, scale=0.1), rnd(C, seed=7, scale=0.1, shift=1.0)) if running else (None, None)
            mean, invstd, y = out(C), out(C), out(*shape, off=off)
            L.call('cpg_bn_relu_fwd_train', P(x), P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(mean), P(invstd), P(y), N, C, HW, relu, P(ws), nb, S())
            report('cpg_bn_relu_fwd_train', '%s relu=%d running=%d' % (case, relu, running), mean, invstd, y, *([rm, rv] if running else []))
    mean, invstd = batch_stats(x)
    if every:
        for relu in (1, 0):
            y = out(*shape, off=off)
            L.call('cpg_bn_relu_fwd_eval', P(x), P(gamma), P(beta), P(mean), P(invstd), P(y), N, C, HW, relu, S())
            report('cpg_bn_relu_fwd_eval', '%s relu=%d' % (case, relu), y)
    for relu, train in (((1, 1), (1, 0), (0, 1), (0, 0)) if every else ((1, 1),)):       # relu x train: all four k_bn_bwd_apply forms
        gx, dgamma, dbeta = out(*shape, off=off), out(C), out(C)
        L.call('cpg_bn_relu_bwd', P(x), P(gy), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dgamma), P(dbeta), N, C, HW, relu, train,
               P(ws), nb, S())
        report('cpg_bn_relu_bwd', '%s relu=%d train=%d' % (case, relu, train), gx, dgamma, dbeta)
    if every:
        dgamma, dbeta, table = out(C), out(C), out(C, 8)                                # the finalize kernel with the rider's table
        L.call('cpg_bn_relu_bwd_reduce', P(x), P(gy), P(gamma), P(beta), P(mean), P(invstd), P(dgamma), P(dbeta), P(table), N, C, HW, P(ws), nb, S())
        report('cpg_bn_relu_bwd_reduce', case, dgamma, dbeta, table)
    # relu(bn(x) + res): MASKY reduce by the byte mask (aligned, 4 | HW), by reading `out` (aligned, no mask), scalar (4 bytes off or odd HW)
    can_mask = L.lib().cpg_bn_add_relu_mask_bytes(N, C, HW) > 0 and not off
    for with_mask in ((True, False) if (can_mask and every) else (can_mask,)):
        for train in ((1, 0) if every else (1,)):
            rm, rv = rnd(C, seed=6, scale=0.1), rnd(C, seed=7, scale=0.1, shift=1.0)
            m2, i2 = (out(C), out(C)) if train else (mean, invstd)
            y = out(*shape, off=off)
            mask = out(L.lib().cpg_bn_add_relu_mask_bytes(N, C, HW), dtype=torch.uint8) if with_mask else None
            L.call('cpg_bn_add_relu_fwd', P(x), P(res), P(gamma), P(beta), EPS, MOM, P(rm if train else None), P(rv if train else None), P(m2), P(i2),
                   P(y), N, C, HW, train, P(ws), nb, S(), P(mask, torch.uint8))
            label = '%s train=%d %s' % (case, train, 'byte-mask' if with_mask else ('read-out' if can_mask else 'scalar'))
            report('cpg_bn_add_relu_fwd', label, y, m2, i2, rm, rv, *([mask] if with_mask else []))
            gx, gz, dgamma, dbeta = out(*shape, off=off), out(*shape, off=off), out(C), out(C)
            L.call('cpg_bn_add_relu_bwd', P(x), P(None if with_mask else y), P(gy), P(gamma), P(beta), P(m2), P(i2), P(gx), P(gz), P(dgamma), P(dbeta),
                   N, C, HW, train, P(ws), nb, S(), P(mask, torch.uint8))
            report('cpg_bn_add_relu_bwd', label, gx, gz, dgamma, dbeta)


def tiles(tag, shape, ntiles):
    """The two *_finalize_tiles kernels: 3 tiles (the remainder loop alone), 5 000 tiles (the four-way loop, then the remainder)."""
    N, C, H, W = shape
    HW = H * W
    case = '%s tiles=%d' % (tag, ntiles)
    partials = rnd(C, ntiles, 2, seed=11).abs_()
    for running in (True, False):
        rm, rv = (rnd(C, seed=6, scale=0.1), rnd(C, seed=7, scale=0.1, shift=1.0)) if running else (None, None)
        mean, invstd = out(C), out(C)
        L.call('cpg_bn_stats_finalize', P(partials), ntiles, N, C, HW, EPS, MOM, P(rm), P(rv), P(mean), P(invstd), S())
        report('cpg_bn_stats_finalize', '%s running=%d' % (case, running), mean, invstd, *([rm, rv] if running else []))
    rm, rv, nbt = rnd(C, seed=6, scale=0.1), rnd(C, seed=7, scale=0.1, shift=1.0), torch.full((1,), 41, dtype=torch.int64, device=DEV)
    mean, invstd = out(C), out(C)
    L.call('cpg_bn_stats_finalize_count', P(partials), ntiles, N, C, HW, EPS, MOM, P(rm), P(rv), P(mean), P(invstd), P(nbt, torch.int64), S())
    report('cpg_bn_stats_finalize_count', case, mean, invstd, rm, rv, nbt)
    partials = rnd(C, ntiles, 2, seed=12)
    dgamma, dbeta, coef = out(C), out(C), out(C, 2)
    L.call('cpg_bn_bwd_finalize_partials', P(partials), ntiles, N, C, HW, P(dgamma), P(dbeta), P(coef), S())
    report('cpg_bn_bwd_finalize_partials', case, dgamma, dbeta, coef)
    x, gm = rnd(*shape, seed=1, scale=2.0, shift=0.5), rnd(*shape, seed=2)
    gamma, beta = channel_params(C, 4)
    mean, invstd = batch_stats(x)
    gx, dgamma, dbeta = out(*shape), out(C), out(C)
    ws, nb = ws_for(N, C, HW)
    L.call('cpg_bn_bwd_from_partials', P(partials), ntiles, P(x), P(gm), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dgamma), P(dbeta), N, C, HW,
           P(ws), nb, S())
    report('cpg_bn_bwd_from_partials', case, gx, dgamma, dbeta)


def pool2(tag, shape, every=True):
    N, C, H, W = shape
    case = 'pool2-%s %dx%dx%dx%d' % (tag, N, C, H, W)
    x, gp = rnd(*shape, seed=1, scale=2.0, shift=0.3), rnd(N, C, H // 2, W // 2, seed=2)
    gamma, beta = channel_params(C, 4)
    ws, nb = ws_for(N, C, H * W)
    for train in ((1, 0) if every else (1,)):
        rm, rv = rnd(C, seed=6, scale=0.1), rnd(C, seed=7, scale=0.1, shift=1.0)
        mean, invstd = (out(C), out(C)) if train else batch_stats(x)
        y = out(N, C, H // 2, W // 2)
        L.call('cpg_bn_relu_pool_fwd', P(x), P(gamma), P(beta), EPS, MOM, P(rm if train else None), P(rv if train else None), P(mean), P(invstd), P(y),
               N, C, H, W, train, P(ws), nb, S())
        report('cpg_bn_relu_pool_fwd', '%s train=%d' % (case, train), y, mean, invstd, rm, rv)
        gx, dgamma, dbeta = out(*shape), out(C), out(C)
        L.call('cpg_bn_relu_pool_bwd', P(x), P(gp), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dgamma), P(dbeta), N, C, H, W, train, P(ws), nb, S())
        report('cpg_bn_relu_pool_bwd', '%s train=%d' % (case, train), gx, dgamma, dbeta)


def pool3(tag, shape):
    N, C, H, W = shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    case = 'pool3-%s %dx%dx%dx%d' % (tag, N, C, H, W)
    x, gp = rnd(*shape, seed=1, scale=2.0, shift=0.3), rnd(N, C, OH, OW, seed=2)
    gamma, beta = channel_params(C, 4)
    mean, invstd = batch_stats(x)
    y = out(N, C, OH, OW)
    L.call('cpg_bn_relu_pool3_fwd', P(x), P(gamma), P(beta), P(mean), P(invstd), P(y), N, C, H, W, S())
    report('cpg_bn_relu_pool3_fwd', case, y)
    ws, nb = ws_for(N, C, H * W)
    for train in (1, 0):
        gx, dgamma, dbeta = out(*shape), out(C), out(C)
        L.call('cpg_bn_relu_pool3_bwd', P(x), P(gp), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dgamma), P(dbeta), N, C, H, W, train, P(ws), nb, S())
        report('cpg_bn_relu_pool3_bwd', '%s train=%d' % (case, train), gx, dgamma, dbeta)


def prelu(tag, shape, off=0, every=True):
    """PReLU: slope shared / per channel, with / without the bias sum (backward), with / without a residual (forward)."""
    N, C, H, W = shape
    HW = H * W
    case = '%s %dx%dx%dx%d%s' % (tag, N, C, H, W, ' +4B' if off else '')
    x, gy, res = rnd(*shape, seed=1, off=off), rnd(*shape, seed=2, off=off), rnd(*shape, seed=3, off=off)
    ws, nb = L.workspace(L.lib().cpg_prelu_workspace_bytes(N, C, HW), DEV)
    for n_slopes in ((C, 1) if every else (C,)):
        slope = rnd(n_slopes, seed=5, scale=0.3, shift=0.2)
        kind = 'per-channel' if n_slopes == C else 'shared'
        if every:
            for r in (res, None):
                y = out(*shape, off=off)
                L.call('cpg_prelu_fwd', P(x), P(r), P(slope), P(y), N, C, HW, n_slopes, S())
                report('cpg_prelu_fwd', '%s %s res=%d' % (case, kind, r is not None), y)
            gx, gs = out(*shape, off=off), out(n_slopes)
            L.call('cpg_prelu_bwd', P(x), P(gy), P(slope), P(gx), P(gs), N, C, HW, n_slopes, P(ws), nb, S())
            report('cpg_prelu_bwd', '%s %s' % (case, kind), gx, gs)
        gx, gs, gb = out(*shape, off=off), out(n_slopes), out(C)
        L.call('cpg_prelu_bwd_bias', P(x), P(gy), P(slope), P(gx), P(gs), P(gb), N, C, HW, n_slopes, P(ws), nb, S())
        report('cpg_prelu_bwd_bias', '%s %s' % (case, kind), gx, gs, gb)


def main():
    print('# lib %s' % L.LIB_PATH, file=sys.stderr)
    for tag, shape in PLAIN.items():
        plain(tag, shape)
        prelu(tag, shape)
    for tag in ('vec-large', 'vec-small'):          # 4 | HW, but every tensor 4 bytes off a 16-byte boundary: the scalar paths by alignment
        plain(tag, PLAIN[tag], off=1)
        prelu(tag, PLAIN[tag], off=1)
    for ntiles in (3, 5000):
        tiles('vec-small', PLAIN['vec-small'], ntiles)
    tiles('vec-large', PLAIN['vec-large'], 3)
    for tag, shape in POOL2.items():
        pool2(tag, shape)
    for tag, shape in POOL3.items():
        pool3(tag, shape)
    if '--no-large' not in sys.argv:
        for tag, shape in LARGE.items():
            plain(tag, shape, every=False)
            prelu(tag, shape, every=False)
        for tag, shape in POOL2_LARGE.items():
            pool2(tag, shape, every=False)


if __name__ == '__main__':
    main()
