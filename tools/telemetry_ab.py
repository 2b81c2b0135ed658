#!/usr/bin/env python3
"""What step telemetry costs (profiles/step_telemetry.md), telemetry off and on interleaved in ONE process on one GPU:

  kernels   HIP events around the three multi-tensor passes over the masked layers of a network (sizes read from the model), plain
            entry point against its `_stats` twin (the pass, the finalize launch and the health launch), alternating every repetition;
  step      the whole train step (forward, backward, routing, MaskedSGD.step) at --batch, the optimizer's `telemetry` attribute set
            and cleared in alternating blocks of --iters steps, --reps times: median ms per step of each arm and of each block.

    python tools/telemetry_ab.py --arch custom_vgg --arch resnet50
One `RESULT {json}` line per measurement.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpg_amd import _lib as L  # noqa: E402
from cpg_amd.driver import CPGSession, default_args, masked_layers  # noqa: E402
from cpg_amd.utils.telemetry import StepTelemetry  # noqa: E402

DEV = 'cuda:0'


def kernels(arch, sizes, reps, warm=10):
    g = torch.Generator().manual_seed(3)
    T = lambda n: torch.randn(n, generator=g).to(DEV)      # noqa: E731
    w, gw, b1 = [T(n) for n in sizes], [T(n) for n in sizes], [T(n) for n in sizes]
    b2 = [T(n).abs() for n in sizes]
    ow = [torch.randint(0, 4, (n,), generator=g, dtype=torch.uint8).to(DEV) for n in sizes]
    n = len(sizes)
    sgd = (L.SgdItem * n)(*[(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), a.numel()) for a, b, c, d in zip(w, gw, b1, ow)])
    adam = (L.AdamItem * n)(*[(a.data_ptr(), b.data_ptr(), c.data_ptr(), e.data_ptr(), d.data_ptr(), a.numel())
                              for a, b, c, e, d in zip(w, gw, b1, b2, ow)])
    need = L.lib().cpg_step_stats_workspace_bytes((ctypes.c_int64 * n)(*sizes), n)
    st = torch.zeros(n, 8, dtype=torch.float64, device=DEV)
    pa = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    he = torch.zeros(4, dtype=torch.int64, device=DEV)
    s = L.stream_ptr()
    tail = (ctypes.c_void_p(st.data_ptr()), ctypes.c_void_p(pa.data_ptr()), need, ctypes.c_void_p(he.data_ptr()), s)
    SGD, ADAM = (2, 4e-5, 1e-4, 0.9, 1, 0), (3, L.MODE_FINETUNE, 5e-4, 0.9, 0.999, 1e-8, 3)
    arms = {
        'cpg_sgd_route_step_multi': (lambda: L.call('cpg_sgd_route_step_multi', sgd, n, *SGD, s),
                                     lambda: L.call('cpg_sgd_route_step_multi_stats', sgd, n, *SGD, 1, *tail)),
        'cpg_sgd_route_zero_step_multi': (lambda: L.call('cpg_sgd_route_zero_step_multi', sgd, n, *SGD, s),
                                          lambda: L.call('cpg_sgd_route_zero_step_multi_stats', sgd, n, *SGD, 1, *tail)),
        'cpg_adam_route_step_multi': (lambda: L.call('cpg_adam_route_step_multi', adam, n, *ADAM, s),
                                      lambda: L.call('cpg_adam_route_step_multi_stats', adam, n, *ADAM, 5e-3, 1, *tail)),
    }
    for name, pair in arms.items():
        for f in pair:
            for _ in range(warm):
                f()
        torch.cuda.synchronize()
        ts = ([], [])
        for _ in range(reps):
            for k, f in enumerate(pair):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
        med = [statistics.median(t) for t in ts]
        print('RESULT ' + json.dumps({'what': 'kernels', 'arch': arch, 'entry': name, 'layers': n, 'elements': sum(sizes), 'reps': reps,
                                      'plain_us': round(med[0], 1), 'stats_us': round(med[1], 1), 'plain_min_us': round(min(ts[0]), 1),
                                      'stats_min_us': round(min(ts[1]), 1), 'delta_pct': round(100 * (med[1] / med[0] - 1), 2)}), flush=True)


def step_ab(arch, batch, iters, reps):
    sess = CPGSession(arch, 1.0, device=DEV, seed=1, data_parallel=False)
    sess.start_task('t', 100)
    args = default_args(dataset='t', lr=1e-3)
    mgr = sess._manager(args, [], [], 0, 0)
    mgr.pruner.make_finetuning_mask()
    opts = sess.make_optimizers(args, mgr.pruner)
    sizes = [m.weight.numel() for _, m in masked_layers(sess.net)]
    model = sess.model.train()
    x = torch.randn(batch, 3, 224, 224, device=DEV)
    t = torch.randint(0, 100, (batch,), device=DEV)
    tel = StepTelemetry()

    def step():
        opts.zero_grad()
        F.cross_entropy(model(x), t).backward()
        mgr.pruner.do_weight_decay_and_make_grads_zero()
        opts.step()
    import time
    blocks = {False: [], True: []}
    for on in (False, True, False, True):               # warm-up of both arms (allocations, the tables' first use)
        opts[0].telemetry = tel if on else None
        step()
    for _ in range(reps):
        for on in (False, True):
            opts[0].telemetry = tel if on else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                step()
            torch.cuda.synchronize()
            blocks[on].append((time.perf_counter() - t0) / iters * 1e3)
    tel.check()
    off, on = statistics.median(blocks[False]), statistics.median(blocks[True])
    print('RESULT ' + json.dumps({'what': 'step', 'arch': arch, 'batch': batch, 'iters': iters, 'reps': reps, 'masked_layers': len(sizes),
                                  'off_ms': round(off, 3), 'on_ms': round(on, 3), 'delta_pct': round(100 * (on / off - 1), 2),
                                  'off_blocks_ms': [round(v, 3) for v in blocks[False]], 'on_blocks_ms': [round(v, 3) for v in blocks[True]],
                                  'off_spread_pct': round(100 * (max(blocks[False]) - min(blocks[False])) / off, 2)}), flush=True)
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', action='append', default=None, help='custom_vgg (the VGG16 headline) and / or resnet50')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--iters', type=int, default=6)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--kernel-reps', type=int, default=40)
    a = ap.parse_args()
    for arch in a.arch or ['custom_vgg', 'resnet50']:
        sizes = step_ab(arch, a.batch, a.iters, a.reps)
        torch.cuda.empty_cache()
        kernels(arch, sizes, a.kernel_reps)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
