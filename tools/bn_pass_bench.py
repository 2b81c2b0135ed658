#!/usr/bin/env python3
"""Device time of the BatchNorm / PReLU entry points of csrc/bn_kernels.hip at the workloads' own shapes (batch 256): HIP events around
each call, 10 warm-up calls, REPS timed ones, medians in one `RESULT {json}` line.  CPG_HIP_LIB selects the library, so two builds are
compared by alternating fresh processes, as tools/routed_step_bench.py does (profiles/bn_pass_refactor.md):

    for L in parent.so new.so parent.so; do CPG_HIP_LIB=$PWD/$L python tools/bn_pass_bench.py 60; done
"""
import json, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cpg_amd import _lib as L

REPS, WARM = int(sys.argv[1]) if len(sys.argv) > 1 else 60, 10
DEV = 'cuda:0'
EPS, MOM = 1e-5, 0.1
gen = torch.Generator(device=DEV).manual_seed(3)
T = lambda *shape: torch.randn(shape, generator=gen, device=DEV)
E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
P, s = L.dptr, L.stream_ptr()


def plain(N, C, H, W):
    """Training forward and backward of BatchNorm -> ReLU."""
    HW = H * W
    x, gy, y, gx = T(N, C, H, W), T(N, C, H, W), E(N, C, H, W), E(N, C, H, W)
    gamma, beta, rm, rv, mean, invstd, dg, db = T(C), T(C), T(C), T(C).abs(), E(C), E(C), E(C), E(C)
    ws, nb = L.workspace(L.lib().cpg_bn_workspace_bytes(N, C, HW), DEV)
    return {'cpg_bn_relu_fwd_train': lambda: L.call('cpg_bn_relu_fwd_train', P(x), P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(mean), P(invstd), P(y),
                                                    N, C, HW, 1, P(ws), nb, s),
            'cpg_bn_relu_bwd': lambda: L.call('cpg_bn_relu_bwd', P(x), P(gy), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dg), P(db), N, C, HW, 1, 1,
                                              P(ws), nb, s)}


def pool2(N, C, H, W):
    x, gp, y, gx = T(N, C, H, W), T(N, C, H // 2, W // 2), E(N, C, H // 2, W // 2), E(N, C, H, W)
    gamma, beta, rm, rv, mean, invstd, dg, db = T(C), T(C), T(C), T(C).abs(), E(C), E(C), E(C), E(C)
    ws, nb = L.workspace(L.lib().cpg_bn_workspace_bytes(N, C, H * W), DEV)
    return {'cpg_bn_relu_pool_fwd': lambda: L.call('cpg_bn_relu_pool_fwd', P(x), P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(mean), P(invstd), P(y),
                                                   N, C, H, W, 1, P(ws), nb, s),
            'cpg_bn_relu_pool_bwd': lambda: L.call('cpg_bn_relu_pool_bwd', P(x), P(gp), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dg), P(db),
                                                   N, C, H, W, 1, P(ws), nb, s)}


def pool3(N, C, H, W):
    """The ResNet stem's tail: statistics come from the conv's epilogue, so the forward is the apply pass alone."""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, gp, y, gx = T(N, C, H, W), T(N, C, OH, OW), E(N, C, OH, OW), E(N, C, H, W)
    gamma, beta, dg, db = T(C), T(C), E(C), E(C)
    var, mu = torch.var_mean(x, dim=(0, 2, 3), unbiased=False)
    mean, invstd = mu.contiguous(), torch.rsqrt(var + EPS).contiguous()
    ws, nb = L.workspace(L.lib().cpg_bn_workspace_bytes(N, C, H * W), DEV)
    return {'cpg_bn_relu_pool3_fwd': lambda: L.call('cpg_bn_relu_pool3_fwd', P(x), P(gamma), P(beta), P(mean), P(invstd), P(y), N, C, H, W, s),
            'cpg_bn_relu_pool3_bwd': lambda: L.call('cpg_bn_relu_pool3_bwd', P(x), P(gp), P(gamma), P(beta), P(mean), P(invstd), P(gx), P(dg), P(db),
                                                    N, C, H, W, 1, P(ws), nb, s)}


def add_relu(N, C, H, W):
    """relu(bn(x) + res), the tail of a residual block: with the byte mask where the shape has one (4 | HW), else reading the output."""
    HW = H * W
    x, res, gy, y, gx, gz = T(N, C, H, W), T(N, C, H, W), T(N, C, H, W), E(N, C, H, W), E(N, C, H, W), E(N, C, H, W)
    gamma, beta, rm, rv, mean, invstd, dg, db = T(C), T(C), T(C), T(C).abs(), E(C), E(C), E(C), E(C)
    nmask = L.lib().cpg_bn_add_relu_mask_bytes(N, C, HW)
    mask = torch.empty(nmask, dtype=torch.uint8, device=DEV) if nmask else None
    ws, nb = L.workspace(L.lib().cpg_bn_workspace_bytes(N, C, HW), DEV)
    return {'cpg_bn_add_relu_fwd': lambda: L.call('cpg_bn_add_relu_fwd', P(x), P(res), P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(mean), P(invstd), P(y),
                                                  N, C, HW, 1, P(ws), nb, s, P(mask, torch.uint8)),
            'cpg_bn_add_relu_bwd': lambda: L.call('cpg_bn_add_relu_bwd', P(x), P(None if nmask else y), P(gy), P(gamma), P(beta), P(mean), P(invstd),
                                                  P(gx), P(gz), P(dg), P(db), N, C, HW, 1, P(ws), nb, s, P(mask, torch.uint8))}


def prelu(N, C, H, W):
    HW = H * W
    x, gy, y, gx, slope, gs, gb = T(N, C, H, W), T(N, C, H, W), E(N, C, H, W), E(N, C, H, W), T(C), E(C), E(C)
    ws, nb = L.workspace(L.lib().cpg_prelu_workspace_bytes(N, C, HW), DEV)
    return {'cpg_prelu_fwd': lambda: L.call('cpg_prelu_fwd', P(x), None, P(slope), P(y), N, C, HW, C, s),
            'cpg_prelu_bwd_bias': lambda: L.call('cpg_prelu_bwd_bias', P(x), P(gy), P(slope), P(gx), P(gs), P(gb), N, C, HW, C, P(ws), nb, s)}


WORKLOADS = [  # (network, maker, shape)
    ('vgg16', plain, (256, 64, 224, 224)), ('vgg16', pool2, (256, 64, 224, 224)), ('vgg16', plain, (256, 128, 112, 112)),
    ('vgg16', pool2, (256, 128, 112, 112)), ('vgg16', plain, (256, 512, 14, 14)), ('vgg16', pool2, (256, 512, 14, 14)),
    ('resnet50', pool3, (256, 64, 112, 112)), ('resnet50', add_relu, (256, 256, 56, 56)), ('resnet50', plain, (256, 2048, 7, 7)),
    ('resnet50', add_relu, (256, 2048, 7, 7)), ('spherenet20', prelu, (256, 64, 56, 48)),
]
out = {'lib': L.LIB_PATH}
for net, make, shape in WORKLOADS:
    arms = make(*shape)
    for name, f in arms.items():
        for _ in range(WARM):
            f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        out['%s %s %s' % (net, name, 'x'.join(map(str, shape)))] = round(statistics.median(ts), 2)
    del arms
    torch.cuda.empty_cache()
print('RESULT ' + json.dumps(out))
