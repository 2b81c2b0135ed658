#!/usr/bin/env python3
"""Device time of the six routed optimizer entry points (cpg_sgd_route_step, cpg_sgd_route_zero_step, cpg_adam_route_step and their
multi-tensor forms) over the 15 masked layers of the width-1.0 VGG16, sizes read from the model: HIP events around one pass over all
15 layers, 10 warm-up passes, REPS timed ones, medians in one `RESULT {json}` line.  CPG_HIP_LIB selects the library, so two builds are
compared by alternating processes, as tools/ab_lib.sh does (profiles/routed_step_refactor.md):

    for L in parent.so new.so parent.so; do CPG_HIP_LIB=$PWD/$L python tools/routed_step_bench.py 60; done
"""
import json, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cpg_amd.models as models
from cpg_amd.models import layers as nl
from cpg_amd import _lib as L

REPS, WARM = int(sys.argv[1]) if len(sys.argv) > 1 else 60, 10
cfg = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']
net = models.custom_vgg_cifar100(cfg, dataset_history=[], dataset2num_classes={}, network_width_multiplier=1.0, shared_layer_info={})
sizes = [m.weight.numel() for m in net.modules() if isinstance(m, (nl.SharableConv2d, nl.SharableLinear))]
assert len(sizes) == 15, sizes
dev = 'cuda:0'
g = torch.Generator().manual_seed(3)
T = lambda n: torch.randn(n, generator=g).to(dev)
w = [T(n) for n in sizes]; gw = [T(n) for n in sizes]; b1 = [T(n) for n in sizes]; b2 = [T(n).abs() for n in sizes]
ow = [torch.randint(0, 4, (n,), generator=g, dtype=torch.uint8).to(dev) for n in sizes]
s = L.stream_ptr()
sgd_rows = [(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), a.numel()) for a, b, c, d in zip(w, gw, b1, ow)]
adam_rows = [(a.data_ptr(), b.data_ptr(), c.data_ptr(), e.data_ptr(), d.data_ptr(), a.numel()) for a, b, c, e, d in zip(w, gw, b1, b2, ow)]
sgd_items = (L.SgdItem * 15)(*sgd_rows); adam_items = (L.AdamItem * 15)(*adam_rows)
SGD = (2, 4e-5, 1e-4, 0.9, 1, 0); ADAM = (3, L.MODE_FINETUNE, 5e-4, 0.9, 0.999, 1e-8, 3)

def per_layer(entry, rows, hyper):
    def f():
        for r in rows:
            L.call(entry, *r[:-1], *hyper, r[-1], s)
    return f

arms = {
    'cpg_sgd_route_step_multi': lambda: L.call('cpg_sgd_route_step_multi', sgd_items, 15, *SGD, s),
    'cpg_sgd_route_zero_step_multi': lambda: L.call('cpg_sgd_route_zero_step_multi', sgd_items, 15, *SGD, s),
    'cpg_adam_route_step_multi': lambda: L.call('cpg_adam_route_step_multi', adam_items, 15, *ADAM, s),
    'cpg_sgd_route_step': per_layer('cpg_sgd_route_step', sgd_rows, SGD),
    'cpg_sgd_route_zero_step': per_layer('cpg_sgd_route_zero_step', sgd_rows, SGD),
    'cpg_adam_route_step': per_layer('cpg_adam_route_step', adam_rows, ADAM),
}
out = {'lib': L.LIB_PATH, 'elements': sum(sizes)}
for name, f in arms.items():
    for _ in range(WARM):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    out[name] = {'median_us': statistics.median(ts), 'min_us': min(ts), 'p90_us': sorted(ts)[int(0.9 * len(ts))]}
print('RESULT ' + json.dumps(out))
