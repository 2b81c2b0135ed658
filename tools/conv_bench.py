#!/usr/bin/env python3
"""Per-layer microbenchmark of the masked conv / linear kernels through the C ABI (HIP events on the
launch stream).  Prints TFLOP/s per (layer, pass).  Used for A/B work on kernel configurations and as
the command profiled with rocprofv3 --pmc.

    python tools/conv_bench.py [--batch 256] [--iters 5] [--only fwd,dgrad,wgrad] [--layers 3,7]

Passes beside fwd / dgrad / wgrad and the opt-in bf16 ones: `wgradr` = the weight gradient with a BatchNorm-backward rider attached
(cpg_conv2d_wgrad_attach_bn_bwd on a tensor shaped like the layer's input; skipped where the query says no), `bnbwd` / `bnred` = the
standalone cpg_bn_relu_bwd on that tensor and its reduce + finalize part alone (their difference is the apply pass the rider replaces).
The pooled chain of a layer whose output goes through BatchNorm2d -> ReLU -> MaxPool2d(2, 2) (f3, f10, f17, f27, f34): `fwdstats` / `fwdstatsm`
= the forward with the statistics epilogue without / with the window maxima attached (cpg_conv2d_fwd_attach_pool_max; skipped where the
query says no), `bnpfwd` / `bnpfwdm` = the pooled apply pass reading the conv output / the maxima, `bnpbwd` / `bnpbwdm` = the pooled backward
(reduce + finalize + apply) with the reduction reading the conv output / the maxima: the apply pass is the same kernel in both, so their
difference is the reduction's.
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpg_amd import _lib                      # noqa: E402
from cpg_amd.models.layers import _conv_desc  # noqa: E402

# (name, Cin, Cout, H, multiplicity) of VGG16 @224 -- SURVEY.md section 8 table (f17/f20, f27/f30, f34/f37/f40 share shapes)
VGG = [('f0', 3, 64, 224, 1), ('f3', 64, 64, 224, 1), ('f7', 64, 128, 112, 1), ('f10', 128, 128, 112, 1), ('f14', 128, 256, 56, 1),
       ('f17', 256, 256, 56, 2), ('f24', 256, 512, 28, 1), ('f27', 512, 512, 28, 2), ('f34', 512, 512, 14, 3)]


def timeit(fn, iters):
    rc = fn()
    if rc:      # (an --ab value that changes the launch plan may outgrow the workspace sized for the default plan: say so, do not time the refusal)
        from cpg_amd import _lib
        raise RuntimeError('launch refused (rc %d): %s' % (rc, _lib.lib().cpg_last_error().decode() if hasattr(_lib.lib(), 'cpg_last_error') else ''))
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--only', default='fwd,dgrad,wgrad')
    ap.add_argument('--layers', default='')
    ap.add_argument('--pm', action='store_true')
    ap.add_argument('--shape', default='', help='extra 3x3 layer "C,K,H" (name x0) instead of the VGG list')
    ap.add_argument('--ab', default='', help='A/B inside one process: NAME=v1,v2,... toggles that env var between timed runs (median of --reps rounds)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--width-multiplier', type=float, default=1.0,
                    help="RAW width multiplier of the reference's command line: the VGG list with int(v * sqrt(m)) channels (1.5: 78 / 156 / 313 / 627)")
    ap.add_argument('--pmc-pass', action='store_true', help='no timing: launch every conv of one VGG16 pass exactly once (for rocprofv3 --pmc)')
    a = ap.parse_args()
    L = _lib.lib()
    dev = 'cuda:0'
    st = _lib.stream_ptr()
    sel = set(a.layers.split(',')) if a.layers else None
    print('%-6s %-6s %9s %9s' % ('layer', 'pass', 'ms', 'TFLOP/s'))
    tot = {}
    layers = VGG
    if a.width_multiplier != 1.0:
        r = a.width_multiplier ** 0.5
        layers = [(n, c if c == 3 else int(c * r), int(k * r), h, m) for n, c, k, h, m in VGG]
    if a.shape:
        c, k, h = (int(v) for v in a.shape.split(','))
        layers = [('x0', c, k, h, 1)]
    for name, C, K, H, mult in layers:
        if sel and name not in sel:
            continue
        x = torch.randn(a.batch, C, H, H, device=dev)
        w = torch.randn(K, C, 3, 3, device=dev) * 0.05
        pm = torch.rand(K, C, 3, 3, device=dev) * 0.012 if a.pm else None
        y = torch.empty(a.batch, K, H, H, device=dev)
        gy = torch.randn(a.batch, K, H, H, device=dev)
        gx = torch.empty_like(x)
        gw = torch.empty_like(w)
        gpm = torch.empty_like(w) if a.pm else None
        d = _conv_desc(x.shape, w.shape, (1, 1), (1, 1), (1, 1), 1)
        nws = L.cpg_conv2d_workspace_bytes(ctypes.byref(d))
        ws, nb = _lib.workspace(nws, dev)
        ws16, nb16 = _lib.workspace(L.cpg_conv2d_bf16_workspace_bytes(ctypes.byref(d)), dev)       # opt-in bf16 path (fwd16 / dgrad16)
        wsw16, nbw16 = _lib.workspace(L.cpg_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d)), dev)
        flops = 2.0 * a.batch * K * H * H * C * 9
        P = _lib.dptr
        tiles = L.cpg_conv2d_bnstats_tiles(ctypes.byref(d))
        stats = torch.empty(max(1, K * tiles * 2) * 4, device=dev)       # (x 4: an --ab over kernel variants may change the tile count)
        # the rider's side: BatchNorm -> ReLU backward of the layer below on a tensor shaped like x
        want_rider = bool({'wgradr', 'bnbwd', 'bnred'} & set(a.only.split(',')))
        ry, rgy = (torch.randn_like(x), torch.empty_like(x)) if want_rider else (None, None)       # (two more activation tensors: only when asked for)
        table = torch.empty(C, 8, device=dev)
        bp = [torch.rand(C, device=dev) + 0.5 for _ in range(4)]          # gamma, beta, mean, invstd
        dgb = [torch.empty(C, device=dev) for _ in range(2)]
        wsb, nbb = _lib.workspace(L.cpg_bn_workspace_bytes(a.batch, C, H * H), dev)
        rider_ok = bool(L.cpg_conv2d_wgrad_rider_supported(ctypes.byref(d))) and x.numel() * 4 < (1 << 31)
        # the pooled chain behind this layer: BatchNorm -> ReLU -> MaxPool2d(2, 2) on y, with or without y's window maxima
        pool_passes = {'fwdstatsm', 'bnpfwd', 'bnpfwdm', 'bnpbwd', 'bnpbwdm'} & set(a.only.split(','))
        pmax_ok = bool(L.cpg_conv2d_fwd_pool_max_supported(ctypes.byref(d)))
        if pool_passes:
            emax = torch.empty(a.batch, K, H // 2, H // 2, device=dev)
            ypool, gpool = torch.empty_like(emax), torch.randn_like(emax)
            kp = [torch.rand(K, device=dev) + 0.5 for _ in range(2)] + [torch.zeros(K, device=dev), torch.ones(K, device=dev)]   # gamma, beta, mean, invstd
            kdgb = [torch.empty(K, device=dev) for _ in range(2)]
            wsk, nbk = _lib.workspace(L.cpg_bn_workspace_bytes(a.batch, K, H * H), dev)
            if pool_passes - {'fwdstatsm'}:
                y.normal_()
                emax.copy_(torch.nn.functional.max_pool2d(y, 2, 2))
        bwd_tail = lambda: (P(gpool), P(kp[0]), P(kp[1]), P(kp[2]), P(kp[3]), P(gy), P(kdgb[0]), P(kdgb[1]), a.batch, K, H, H, 1, P(wsk), nbk, st)

        def fwdstats_max():
            rc = L.cpg_conv2d_fwd_attach_pool_max(P(emax), emax.numel() * 4)
            return rc or runs['fwdstats']()

        def wgrad_rider():
            rc = L.cpg_conv2d_wgrad_attach_bn_bwd(P(ry), P(gx), P(rgy), P(table), a.batch, C, H * H)
            return rc or L.cpg_conv2d_wgrad(ctypes.byref(d), P(x), P(gy), P(w), P(pm), 5e-3, P(gw), P(gpm), None, P(ws), nb, st)
        runs = {'wgradr': wgrad_rider,
                'fwdstatsm': fwdstats_max,
                'bnpfwd': lambda: L.cpg_bn_relu_pool_fwd(P(y), P(kp[0]), P(kp[1]), 1e-5, 0.1, None, None, P(kp[2]), P(kp[3]), P(ypool), a.batch, K, H, H, 0,
                                                         None, 0, st),
                'bnpfwdm': lambda: L.cpg_bn_relu_pool_fwd_from_max(P(y), P(emax), None, 0, P(kp[0]), P(kp[1]), 1e-5, 0.1, None, None, None, P(kp[2]),
                                                                   P(kp[3]), P(ypool), a.batch, K, H, H, st),
                'bnpbwd': lambda: L.cpg_bn_relu_pool_bwd(P(y), *bwd_tail()),           # (gy serves as the gradient output: same shape as y)
                'bnpbwdm': lambda: L.cpg_bn_relu_pool_bwd_from_max(P(y), P(emax), *bwd_tail()),
                'bnbwd': lambda: L.cpg_bn_relu_bwd(P(ry), P(gx), P(bp[0]), P(bp[1]), P(bp[2]), P(bp[3]), P(rgy), P(dgb[0]), P(dgb[1]), a.batch, C, H * H,
                                                   1, 1, P(wsb), nbb, st),
                'bnred': lambda: L.cpg_bn_relu_bwd_reduce(P(ry), P(gx), P(bp[0]), P(bp[1]), P(bp[2]), P(bp[3]), P(dgb[0]), P(dgb[1]), P(table), a.batch,
                                                          C, H * H, P(wsb), nbb, st),
                'fwdstats': lambda: L.cpg_conv2d_fwd_bnstats(ctypes.byref(d), P(x), P(w), P(pm), 5e-3, None, P(y), P(stats), stats.numel() * 4, P(ws), nb, st),
                'fwd': lambda: L.cpg_conv2d_fwd(ctypes.byref(d), P(x), P(w), P(pm), 5e-3, None, P(y), P(ws), nb, st),
                'dgrad': lambda: L.cpg_conv2d_dgrad(ctypes.byref(d), P(gy), P(w), P(pm), 5e-3, P(gx), P(ws), nb, st),
                'fwd16': lambda: L.cpg_conv2d_fwd_bf16(ctypes.byref(d), P(x), P(w), P(pm), 5e-3, None, P(y), P(ws16), nb16, st),
                'dgrad16': lambda: L.cpg_conv2d_dgrad_bf16(ctypes.byref(d), P(gy), P(w), P(pm), 5e-3, P(gx), P(ws16), nb16, st),
                'fwdx3': lambda: L.cpg_conv2d_fwd_bf16x3(ctypes.byref(d), P(x), P(w), P(pm), 5e-3, None, P(y), P(ws16), nb16, st),
                'dgradx3': lambda: L.cpg_conv2d_dgrad_bf16x3(ctypes.byref(d), P(gy), P(w), P(pm), 5e-3, P(gx), P(ws16), nb16, st),
                'wgradx3': lambda: L.cpg_conv2d_wgrad_bf16x3(ctypes.byref(d), P(x), P(gy), P(w), P(pm), 5e-3, P(gw), P(gpm), P(wsw16), nbw16, st),
                'wgrad16': lambda: L.cpg_conv2d_wgrad_bf16(ctypes.byref(d), P(x), P(gy), P(w), P(pm), 5e-3, P(gw), P(gpm), P(wsw16), nbw16, st),
                'wgrad': lambda: L.cpg_conv2d_wgrad(ctypes.byref(d), P(x), P(gy), P(w), P(pm), 5e-3, P(gw), P(gpm), None, P(ws), nb, st)}
        for k in a.only.split(','):
            if k in ('dgrad', 'dgrad16', 'dgradx3') and name == 'f0':
                continue
            if k == 'wgradr' and not rider_ok:
                continue
            if k in ('fwdstatsm', 'bnpfwdm', 'bnpbwdm') and not pmax_ok:
                continue
            if k == 'wgradr':
                gx.normal_()
                runs['bnred']()                   # (fills the coefficient table)
            if k in ('wgrad16', 'wgradx3') and not L.cpg_conv2d_wgrad_bf16_supported(ctypes.byref(d)):
                continue
            if k in ('fwd16', 'dgrad16', 'fwdx3', 'dgradx3') and not L.cpg_conv2d_bf16_supported(ctypes.byref(d)):
                continue
            if a.pmc_pass:
                for _ in range(mult):
                    runs[k]()
                torch.cuda.synchronize()
                continue
            if a.ab:
                var, vals = a.ab.split('=')
                vals = vals.split(',')
                res = {v: [] for v in vals}
                for v in vals:          # a value may change the launch plan (units per wave slot, ...): size the workspace for the largest
                    _lib.set_option(var, None if v == '-' else v)
                    need = L.cpg_conv2d_workspace_bytes(ctypes.byref(d))
                    if need > nb:
                        ws, nb = _lib.workspace(need, dev)
                for _ in range(a.reps):
                    for v in vals:
                        _lib.set_option(var, None if v == '-' else v)      # (the library reads the environment only when it is loaded)
                        res[v].append(timeit(runs[k], a.iters))
                _lib.set_option(var, None)
                print('%-6s %-6s ' % (name, k) + '  '.join('%s=%s: %.3f ms %.1f TF' % (var, v, sorted(t)[len(t) // 2], flops / sorted(t)[len(t) // 2] / 1e9)
                                                          for v, t in res.items()), flush=True)
                continue
            ms = timeit(runs[k], a.iters)
            print('%-6s %-6s %9.3f %9.1f' % (name, k, ms, flops / ms / 1e9), flush=True)
            t = tot.setdefault(k, [0.0, 0.0])
            t[0] += ms * mult
            t[1] += flops * mult
    for k, (ms, fl) in tot.items():
        print('TOTAL  %-6s %9.3f %9.1f   (13 convs of one VGG16 pass)' % (k, ms, fl / ms / 1e9))


if __name__ == '__main__':
    main()
