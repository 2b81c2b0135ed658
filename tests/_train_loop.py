"""Short training loops of the ResNet pieces, driver and reference of tests/test_train_loop_{host,gpu}.py.

tests/_autograd_ref.py holds one forward and one backward of each small topology to float64.  Here the same nets (and a mini ResNet,
'R') run a few optimizer steps, so that state carried from one step to the next is compared as well: weights the fused optimizers wrote
through data_ptr(), operands packed at forward time, owner masks a prune event rewrote, BatchNorm statistics blended from a non-initial
state, momentum and Adam moments beside routed gradients, weights apply_mask() zeroed for an evaluation and left so.

    run_loop(net, plan, data, device, dtype)    drives the library net (SparsePruner, MaskedSGD / MaskedAdam, the HIP device) and the
                                                reference net (RefPruner: routing, claiming, apply_mask and rank pruning restated on plain
                                                tensors after oracle/ops.py; stock torch optimizers; float64 and once more float32)
    reference(topo, plan, seed)                 the float64 and the stock float32 trajectory and the conditioning of the float64 one
    bounds / compare                            per tensor and step, b = max(floor, 8 x stock fp32's error); the floor is B_FLOOR, and
                                                2^-23 max|w| / max|dw| for an update (the rounding of the fp32 weight it is the difference of)

Compared per step, by name: 'out' / 'loss', 'grad:<p>' (as backward left it), 'routed:<p>' (as the step consumed it), 'upd:<p>' = w after
- w before (an update error of 1e-3 is 1e-5 of the weight's scale: a weight comparison would not see it), 'mom:<p>', 'adam_m:<p>',
'adam_v:<p>', 'buf:<b>', 'mask:<layer>', 'stat:<statistic>' and 'ratio' (the prune ratio gradually_prune returns).  Keys that begin with
'_' carry what the conditioning is computed from and are not compared.

Plans (SGD-Nesterov 0.9, weight decay 4e-5 with the routing, two micro-batches alternating, four steps):
    P1  task 1, prune mode, owners all 1; torch.optim.SGD + do_weight_decay_and_make_grads_zero; rank-prune events after the second and
        the third step (ratios 0.2625 and 0.3), so that two steps train with masks an event left
    P2  the same through MaskedSGD
    P3  task 2, finetune: a piggymask on every covered layer, owners 1 / free, make_finetuning_mask claims the free slots as 2;
        MaskedSGD on the weights, MaskedAdam on the piggymasks
    P4  two steps and the first prune event, apply_mask and an eval forward under no_grad as Manager.validate does (the weights stay
        masked), two more steps with the second event between them
    P5  gradient accumulation: two backwards, one step, twice

The reference runs are pinned to one CPU thread: stock fp32's round-off is the yardstick of every bound and of the conditioning, and
its summation order should not depend on the machine's core count.
"""
import copy
import functools
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

import _autograd_ref as R
from oracle import ops as oops

# Learning rates per topology, and per parameter group where one rate does not serve every tensor: each value is there for a condition
# of the reference alone, named with its reason in tests/test_train_loop_host.py's docstring.
LR = {'A': 0.025, 'B_identity': 0.2, 'B_down': 0.2, 'B_basic': 0.2, 'C': 0.004, 'R': 0.08}
GROUP_LR = {'A': {'seq.11.': 0.5},           # topology -> {parameter name prefix: factor on LR[topology]}, one parameter group each
            'C': {'head.weight': 1e-2, 'head.bias': 0.2, 'conv1.weight': 2.0}}
LR_MASK = 5e-4              # Adam on the piggymasks (the reference's lr_mask)
ADAM_EPS = 1e-2             # ... with eps at the size of the piggymask gradients (torch's 1e-8 makes the update scale-free: see the host test)
WEIGHT_DECAY = 4e-5
COND_FACTOR = 16.0          # every margin >= 16 x the stock fp32 run's own error on the same quantity
BOUND_MAX = 1e-4
UPD_EPS = 2.0 ** -23
STAT_SLACK = 4.0            # the stock fp32 run's own running statistics stay within a quarter of STAT_RTOL / STAT_ATOL (see check_reference)

TOPOLOGIES = R.TOPOLOGIES + ('R',)
PLANS = {
    'P1': dict(mode='prune', fused=False, steps=4, micro=1, freq=1, begin=1, end=3, eval_after=None),
    'P2': dict(mode='prune', fused=True, steps=4, micro=1, freq=1, begin=1, end=3, eval_after=None),
    'P3': dict(mode='finetune', fused=True, steps=4, micro=1, freq=100, begin=1, end=3, eval_after=None),
    'P4': dict(mode='prune', fused=True, steps=4, micro=1, freq=1, begin=1, end=3, eval_after=1),
    'P5': dict(mode='prune', fused=True, steps=2, micro=2, freq=100, begin=1, end=3, eval_after=None),
}
CASES = [(t, p) for t in TOPOLOGIES for p in sorted(PLANS)]

# (topology, plan) -> seed whose float64 trajectory meets the conditioning and whose bounds stay <= 1e-4, found by search_seeds()
_SEEDS = {
    ('A', 'P1'): 294, ('A', 'P2'): 294, ('A', 'P3'): 6, ('A', 'P4'): 868, ('A', 'P5'): 3,
    ('B_identity', 'P1'): 1, ('B_identity', 'P2'): 1, ('B_identity', 'P3'): 1, ('B_identity', 'P4'): 1, ('B_identity', 'P5'): 0,
    ('B_down', 'P1'): 0, ('B_down', 'P2'): 0, ('B_down', 'P3'): 0, ('B_down', 'P4'): 0, ('B_down', 'P5'): 0,
    ('B_basic', 'P1'): 0, ('B_basic', 'P2'): 0, ('B_basic', 'P3'): 0, ('B_basic', 'P4'): 0, ('B_basic', 'P5'): 0,
    ('C', 'P1'): 9, ('C', 'P2'): 9, ('C', 'P3'): 336, ('C', 'P4'): 15, ('C', 'P5'): 1,
    ('R', 'P1'): 669, ('R', 'P2'): 669, ('R', 'P3'): 98, ('R', 'P4'): 213, ('R', 'P5'): 6,
}


def seed_of(topo, plan):
    return _SEEDS[(topo, plan)]


# ------------------------------------------------------------------------------------------------- topology R
class NetR(nn.Module):
    """A mini ResNet: the 7x7 s2 p3 stem (3 -> 64) -> BatchNorm -> ReLU -> MaxPool2d(3, 2, 1), a Bottleneck with a stride-1 downsample
    (64 -> 16 -> 64), one with a stride-2 downsample (64 -> 32 -> 128: the 3x3 s2 and the 1x1 s2), an identity Bottleneck (128 -> 32 ->
    128), the mean over the plane and a head.  On 4 x 3 x 32 x 32: 16 x 16 after the stem, 8 x 8 after the pool, 4 x 4 from the second
    block on.  The library side is models/resnet.py's Bottleneck / conv1x1 and models/fused_bn.py's conv_bn_act_pool / FusedSequential,
    as models/resnet.py's ResNet composes them."""
    x_shape = (4, 3, 32, 32)
    x_grad = False
    classes = 10

    def __init__(self, lib):
        super().__init__()
        self.lib = lib
        if lib:
            from cpg_amd.models import fused_bn, layers as nl, resnet
            block, seq, head, c1 = resnet.Bottleneck, fused_bn.FusedSequential, nl.HeadLinear, resnet.conv1x1
            self.conv1 = nl.SharableConv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        else:
            block, seq, head = R.RefBottleneck, nn.Sequential, nn.Linear
            c1 = lambda i, o, s: R.RefConv2d(i, o, 1, s, bias=False)
            self.conv1 = R.RefConv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=bool(lib))
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = block(64, 16, 1, seq(c1(64, 64, 1), nn.BatchNorm2d(64)))
        self.layer2 = block(64, 32, 2, seq(c1(64, 128, 2), nn.BatchNorm2d(128)))
        self.layer3 = block(128, 32, 1, None)
        self.head = head(128, self.classes)
        self.masked = ['conv1', 'layer2.conv2', 'layer3.conv1']

    def forward(self, x, plane_w=None):
        if self.lib:
            from cpg_amd.models.fused_bn import conv_bn_act_pool
            x = conv_bn_act_pool(self.conv1, self.bn1, self.relu, self.maxpool, x)
        else:
            x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer3(self.layer2(self.layer1(x)))
        return self.head(x.mean((2, 3)))


R.EXTRA_TOPOLOGIES['R'] = NetR


# ------------------------------------------------------------------------------------------------- nets and data of one (topology, plan)
def _covered_ref(m):
    return isinstance(m, (R.RefConv2d, R.RefLinear))


def build_reference(topo, plan, seed):
    """R.build_reference's net for a plan: task 1 has no piggymasks at all (as the driver leaves task 1), task 2 one on every covered
    layer (the statistics and MaskedAdam read every layer's)."""
    net = R.build_reference(topo, seed)
    g = torch.Generator().manual_seed(seed + 104729)
    for m in net.modules():
        if _covered_ref(m):
            if PLANS[plan]['mode'] != 'finetune':
                m.piggymask = None
            elif m.piggymask is None:
                m.piggymask = nn.Parameter(torch.rand(m.weight.shape, generator=g) * 0.012)
    return net


def build_library(topo, ref32, device):
    return R.build_library(topo, ref32, device)


def make_data(topo, plan, seed):
    """R.make_data's two micro-batches and the owner masks the plan starts from (CPU, uint8): all 1, or for task 2 a mix of 1 and free."""
    data = R.make_data(topo, seed)
    g = torch.Generator().manual_seed(seed + 15485863)
    owners = {}
    for n, m in R._new(topo, False).named_modules():
        if _covered_ref(m):
            if PLANS[plan]['mode'] == 'finetune':
                owners[n] = (torch.rand(m.weight.shape, generator=g) < 0.6).to(torch.uint8)
            else:
                owners[n] = torch.ones(m.weight.shape, dtype=torch.uint8)
    data['owners'], data['topo'] = owners, topo
    return data


def _args(cfg):
    return types.SimpleNamespace(mode=cfg['mode'], dataset='t2' if cfg['mode'] == 'finetune' else 't1', finetune_again=False,
                                 target_sparsity=0.3, initial_sparsity=0.0, pruning_frequency=cfg['freq'], weight_decay=WEIGHT_DECAY,
                                 network_width_multiplier=1.0)


# ------------------------------------------------------------------------------------------------- the pruner on plain tensors
class RefPruner(object):
    """SparsePruner's observable effect (utils/prune.py of the reference, as oracle/ops.py restates it per layer) on the reference net,
    in the net's own dtype: the schedule and the cutoff rank are oracle.ops' python arithmetic; ranking, routing, claiming and
    apply_mask are the same statements on torch tensors (oracle.ops casts to float32, the float64 reference must not)."""

    def __init__(self, net, masks, args, begin, end, inference_idx):
        self.net, self.masks, self.args = net, masks, args
        self.begin, self.end, self.last_prune_step = begin, end, begin
        self.inference_dataset_idx = inference_idx
        self.current_dataset_idx = 1                          # (datasets ['t1', 't2']: index + 1 in prune mode, len - 1 in finetune mode)
        self.trace = {}

    def _layers(self):
        return [(n, m) for n, m in self.net.named_modules() if _covered_ref(m)]

    def gradually_prune(self, step):
        if oops.time_to_update(step, self.begin, self.end, self.last_prune_step, self.args.pruning_frequency):
            self.last_prune_step = step
            ratio = oops.adjust_sparsity(step, self.begin, self.end, self.args.initial_sparsity, self.args.target_sparsity)
            for n, m in self._layers():
                self.masks[n] = self._rank_prune(n, m.weight.detach(), self.masks[n], ratio)
            return ratio
        return oops.adjust_sparsity(self.last_prune_step, self.begin, self.end, self.args.initial_sparsity, self.args.target_sparsity)

    def _rank_prune(self, name, w, owner, ratio):
        """oracle.ops.rank_prune."""
        cur = self.current_dataset_idx
        cand = (owner == cur) | (owner == 0)
        a = w.abs()
        vals = a[cand]
        k = oops.cutoff_rank(ratio, vals.numel())
        if k < 1 or k > vals.numel():
            raise oops.NotEnoughWeights('k=%d of n=%d' % (k, vals.numel()))
        srt, order = vals.sort()
        cutoff = srt[k - 1]
        self.trace[name] = {'abs': a.clone(), 'cand': cand, 'at': int(order[k - 1]), 'gap': float(srt[k] - cutoff) if k < vals.numel() else float('inf')}
        out = owner.clone()
        out[(a <= cutoff) & (owner == cur)] = 0
        return out

    def do_weight_decay_and_make_grads_zero(self):
        """oracle.ops.route_grads."""
        cur = self.current_dataset_idx
        for n, m in self._layers():
            owner = self.masks[n]
            if m.weight.grad is not None:
                m.weight.grad.add_(m.weight.detach(), alpha=self.args.weight_decay)
                m.weight.grad[owner != cur] = 0
            if m.piggymask is not None and m.piggymask.grad is not None:
                if self.args.mode == 'finetune':
                    m.piggymask.grad[(owner == 0) | (owner >= cur)] = 0
                else:
                    m.piggymask.grad.zero_()

    def apply_mask(self):
        """oracle.ops.apply_mask."""
        for n, m in self._layers():
            owner = self.masks[n]
            m.weight.data[(owner == 0) | (owner > self.inference_dataset_idx)] = 0

    def make_finetuning_mask(self):
        """oracle.ops.claim_free."""
        self.current_dataset_idx += 1
        for n, _ in self._layers():
            self.masks[n] = self.masks[n].clone()
            self.masks[n][self.masks[n] == 0] = self.current_dataset_idx

    def _owners(self):
        return [self.masks[n].numpy() for n, _ in self._layers()]

    def calculate_sparsity(self):
        return oops.sparsity(self._owners(), self.inference_dataset_idx)

    def calculate_curr_task_ratio(self):
        return oops.curr_task_ratio(self._owners(), self.inference_dataset_idx, self.args.network_width_multiplier)

    def calculate_zero_ratio(self):
        return oops.zero_ratio(self._owners(), self.args.network_width_multiplier)

    def calculate_shared_part_ratio(self):
        return oops.shared_part_ratio(self._owners(), [m.piggymask.detach().numpy() for _, m in self._layers()], self.inference_dataset_idx)


# ------------------------------------------------------------------------------------------------- the loop
def _setup(net, cfg, data, device, lib, topo):
    """(pruner, optimizers, names of the parameters whose .grad is the routed gradient only AFTER the step)."""
    args = _args(cfg)
    inference_idx = 2 if cfg['mode'] == 'finetune' else 1
    masks = {n: o.clone().to(device) for n, o in data['owners'].items()}
    named = dict(net.named_parameters())
    pms = [p for n, p in named.items() if n.endswith('piggymask')]
    # (one parameter group per entry of GROUP_LR[topo], the remaining parameters in the first)
    scales = GROUP_LR.get(topo, {})
    own = lambda n: next((k for k in scales if n.startswith(k) and not n.endswith('piggymask')), None)
    rest = [{'params': [p for n, p in named.items() if not n.endswith('piggymask') and own(n) is None]}]
    rest += [{'params': [p for n, p in named.items() if own(n) == k], 'lr': LR[topo] * scales[k]} for k in scales]
    late = set()
    if lib:
        from cpg_amd.utils.fused_sgd import MaskedAdam, MaskedSGD
        from cpg_amd.utils.prune import SparsePruner
        net.datasets = ['t1', 't2']
        pruner = SparsePruner(net, masks, args, cfg['begin'], cfg['end'], inference_idx)
        if cfg['fused']:
            opts = [MaskedSGD(rest, pruner=pruner, lr=LR[topo], momentum=0.9, nesterov=True)]
            late |= {n + '.weight' for n in masks}
            if pms:
                opts.append(MaskedAdam(pms, pruner=pruner, lr=LR_MASK, eps=ADAM_EPS))
                late |= {n + '.piggymask' for n in masks}
        else:
            opts = [torch.optim.SGD(rest, lr=LR[topo], momentum=0.9, nesterov=True)]
            assert not pms
    else:
        pruner = RefPruner(net, masks, args, cfg['begin'], cfg['end'], inference_idx)
        opts = [torch.optim.SGD(rest, lr=LR[topo], momentum=0.9, nesterov=True)]
        if pms:
            opts.append(torch.optim.Adam(pms, lr=LR_MASK, eps=ADAM_EPS))
    assert pruner.current_dataset_idx == 1
    return pruner, opts, late


def run_loop(net, plan, data, device='cpu', dtype=torch.float32, mark=None, fault=None):
    """Run `plan` on `net` (library or reference: the same code drives both) and return the list of per-step records {name: tensor,
    float or None}.  mark(label) is called between the phases ('setup', 'forward', 'backward', 'route', 'step', 'prune', 'stats',
    'apply_mask', 'eval').  fault = (kind, step) runs ONE deliberately wrong statement, on the reference only: the host test's proof
    that a stale operand, a skipped update or a dropped buffer would be seen."""
    mark = mark or (lambda label: None)
    cfg = PLANS[plan]
    lib = not any(_covered_ref(m) for m in net.modules())
    assert fault is None or not lib
    fkind, fstep = fault or (None, None)
    cv = lambda t: t.to(device=device, dtype=dtype if t.is_floating_point() else t.dtype)
    batches = [(cv(data['x1']), cv(data['t1'])), (cv(data['x2']), cv(data['t2']))]
    keep = lambda t: None if t is None else t.detach().clone()
    mark('setup')
    pruner, opts, late = _setup(net, cfg, data, device, lib, data['topo'])
    if cfg['mode'] == 'finetune':
        pruner.make_finetuning_mask()
    params = dict(net.named_parameters())
    mods = dict(net.named_modules())
    convs = [n for n, m in mods.items() if isinstance(m, nn.Conv2d)]
    bns = [n for n, m in mods.items() if isinstance(m, nn.BatchNorm2d)]
    prev_w = None
    records = []
    nb = 0
    net.train()
    for step in range(cfg['steps']):
        rec = {}
        faulty = step == fstep
        for n, p in params.items():
            if n.endswith('piggymask'):
                rec['_pm:' + n] = keep(p)
        for o in opts:
            o.zero_grad(set_to_none=True)
        for k in range(cfg['micro']):
            x, t = batches[nb % 2]
            nb += 1
            tag = '' if k == 0 else 'micro%d:' % k
            x = x.clone().requires_grad_(data['x_grad'])
            if faulty and fkind == 'overwrite_accum' and k > 0:
                for o in opts:
                    o.zero_grad(set_to_none=True)
            if faulty and fkind == 'stale_conv':
                w = mods[convs[len(convs) // 2]].weight
                now = w.data.clone()
                w.data.copy_(prev_w[convs[len(convs) // 2] + '.weight'])
            if faulty and fkind == 'skip_bn_stats':
                bn = mods[bns[len(bns) // 2]]
                bn.momentum = 0.0                # (the batch statistics still normalise; the running ones stay as they are)
            mark('forward')
            out = net(x)
            loss = F.cross_entropy(out, t)
            if faulty and fkind == 'stale_conv':
                w.data.copy_(now)
            if faulty and fkind == 'skip_bn_stats':
                bn.momentum = 0.1
                bn.num_batches_tracked -= 1
            mark('backward')
            loss.backward()
            rec[tag + 'out'], rec[tag + 'loss'] = keep(out), keep(loss)
        for n, p in params.items():
            rec['grad:' + n] = keep(p.grad)
        before = {n: keep(p) for n, p in params.items()}
        prev_w = before
        mark('route')
        pruner.do_weight_decay_and_make_grads_zero()
        routed = {n: keep(p.grad) for n, p in params.items()}
        if faulty and fkind == 'drop_momentum':
            for p in params.values():
                opts[0].state[p].pop('momentum_buffer', None)
        mark('step')
        for o in opts:
            o.step()
        for n, p in params.items():
            rec['routed:' + n] = keep(p.grad) if n in late else routed[n]
            rec['upd:' + n] = p.detach() - before[n]
            rec['_wmax:' + n] = float(p.detach().abs().max())
            for o in opts:
                st = o.state.get(p, {})
                for key, name in (('momentum_buffer', 'mom:'), ('exp_avg', 'adam_m:'), ('exp_avg_sq', 'adam_v:')):
                    if st.get(key) is not None:
                        rec[name + n] = keep(st[key])
        mark('prune')
        if cfg['mode'] == 'prune':
            rec['ratio'] = None if faulty and fkind == 'skip_prune' else pruner.gradually_prune(step + 1)
            if not lib:
                for n, tr in pruner.trace.items():
                    rec['_prune:' + n] = tr
                pruner.trace = {}
        mark('stats')
        rec['stat:sparsity'] = pruner.calculate_sparsity()
        rec['stat:curr_task_ratio'] = pruner.calculate_curr_task_ratio()
        rec['stat:zero_ratio'] = pruner.calculate_zero_ratio()
        if cfg['mode'] == 'finetune':
            rec['stat:shared_part_ratio'] = pruner.calculate_shared_part_ratio()
        for n in data['owners']:
            rec['mask:' + n] = keep(pruner.masks[n])
        if cfg['eval_after'] == step:
            # Manager.validate: apply_mask() (in place, and left so), then an eval-mode forward under no_grad
            mark('apply_mask')
            if not (faulty and fkind == 'no_apply_mask'):
                pruner.apply_mask()
            for n in data['owners']:
                rec['applied:' + n + '.weight'] = keep(params[n + '.weight'])
            net.eval()
            mark('eval')
            with torch.no_grad():
                rec['eval:out'] = keep(net(batches[0][0]))
            net.train()
        for n, b in net.named_buffers():
            rec['buf:' + n] = keep(b)
        records.append(rec)
    mark('done')
    return records


# ------------------------------------------------------------------------------------------------- reference, conditioning, bound
def _ratio(margin, err):
    """The smallest margin / error over the elements (inf where nothing is off)."""
    margin, err = margin.reshape(-1).double(), err.reshape(-1).double()
    at = err > 0
    return float((margin[at] / err[at]).min()) if bool(at.any()) else float('inf')


def _conditioning(m64, m32, r64, r32):
    """[(quantity, smallest margin of the float64 run, largest |fp32 - fp64| on it, smallest margin / own error over its elements)] per
    layer and step: every ReLU / PReLU input, every pool's window gaps, every piggymask against the threshold, the cutoff gap of
    every prune event (there: the distance of every other candidate |weight| from the cutoff element, against the two's errors)."""
    out, seen = [], {}
    assert len(m64.trace) == len(m32.trace)
    for (kind, name, a), (kind32, name32, b) in zip(m64.trace, m32.trace):
        assert (kind, name, a.shape) == (kind32, name32, b.shape)
        seen[(kind, name)] = seen.get((kind, name), 0) + 1
        label = '%s %s call %d' % (kind, name, seen[(kind, name)])
        if kind == 'act':
            e = (b.double() - a).abs()
            out.append((label, float(a.abs().min()), float(e.max()), _ratio(a.abs(), e)))
        else:
            both = torch.isfinite(a) & torch.isfinite(b)
            e = (b.double()[both] - a[both]).abs()
            # (a window that counts in one run only: its maximum is within round-off of the ReLU's kink, which the 'act' entry reports)
            out.append((label, float(a.min()), float(e.max()), _ratio(a[both], e)))
    for step, (ra, rb) in enumerate(zip(r64, r32)):
        for n in ra:
            if n.startswith('_pm:'):
                m, e = (ra[n] - R.THR).abs(), (rb[n].double() - ra[n]).abs()
                out.append(('piggymask %s step %d' % (n[4:], step), float(m.min()), float(e.max()), _ratio(m, e)))
            elif n.startswith('_prune:'):
                # the released set is {|w| <= the k-th smallest}: it changes when a candidate changes sides of the cutoff element
                a, at = ra[n]['abs'][ra[n]['cand']], ra[n]['at']
                e = (rb[n]['abs'][ra[n]['cand']].double() - a).abs()
                others = torch.ones_like(a, dtype=torch.bool)
                others[at] = False
                out.append(('cutoff %s step %d' % (n[7:], step), ra[n]['gap'], float(e.max()), _ratio((a - a[at]).abs()[others], (e + e[at])[others])))
    return out


@functools.lru_cache(maxsize=None)
def reference(topo, plan, seed):
    """(float64 records, float32 records, conditioning) of the reference net.  Cached: shared between tests, not to be written to."""
    data = make_data(topo, plan, seed)
    ref32 = build_reference(topo, plan, seed)
    ref64 = copy.deepcopy(ref32).double()
    m64, m32 = R.Margin(ref64, trace=True), R.Margin(ref32, trace=True)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)             # (the stock fp32 run's round-off is the yardstick: one summation order, whatever the machine's core count)
    try:
        r64 = run_loop(ref64, plan, data, 'cpu', torch.float64)
        r32 = run_loop(ref32, plan, data, 'cpu', torch.float32)
    finally:
        torch.set_num_threads(threads)
    return r64, r32, _conditioning(m64, m32, r64, r32)


def _kind(name):
    if name.startswith('_'):
        return 'aux'
    if name.startswith(('mask:', 'stat:')) or name == 'ratio':
        return 'exact'
    if 'buf:' in name:
        return 'stat'
    return 'upd' if name.startswith('upd:') else 'float'


def _rel(a, b):
    sc = float(b.abs().max())
    e = float((a.detach().double().cpu() - b).abs().max())
    return (e / sc if sc > 0 else (0.0 if e == 0 else float('inf'))), sc


def bounds(topo, plan, seed):
    """[{name: b}] per step for every floating-point tensor but the running statistics: b = max(floor, B_FACTOR x stock fp32's error),
    floor = B_FLOOR; for an update, 2^-23 max|w| / max|dw| where that is larger (an update is the difference of two fp32 weights: it
    carries their rounding, half an ulp of the weight each, whatever the kernel does)."""
    r64, r32, _ = reference(topo, plan, seed)
    out = []
    for ra, rb in zip(r64, r32):
        bs = {}
        for n, want in ra.items():
            if _kind(n) not in ('float', 'upd') or want is None:
                continue
            e, sc = _rel(rb[n], want)
            floor = R.B_FLOOR
            if _kind(n) == 'upd' and sc > 0:
                floor = max(floor, UPD_EPS * ra['_wmax:' + n[4:]] / sc)
            bs[n] = max(floor, R.B_FACTOR * e)
        out.append(bs)
    return out


def compare(got, topo, plan, seed, log=print):
    """Every tensor of every step against the float64 reference.  Returns (misses, worst): misses = [(step, name, excess, text)] with
    excess = error / allowed (> 1, inf for a mismatch of something exact); worst = {kind: (largest error of scale, name, step)} over
    outputs, gradients and updates.  Each figure is logged before anything is judged."""
    r64, r32, _ = reference(topo, plan, seed)
    bnd = bounds(topo, plan, seed)
    bad, worst = [], {}
    assert len(got) == len(r64)
    for step, (have_rec, want_rec) in enumerate(zip(got, r64)):
        pub = lambda rec: {n for n in rec if _kind(n) != 'aux'}
        assert pub(have_rec) == pub(want_rec), sorted(pub(have_rec) ^ pub(want_rec))
        for n in sorted(pub(want_rec)):
            want, have = want_rec[n], have_rec[n]
            where = '%s %s step %d %s' % (topo, plan, step, n)
            if want is None or have is None:
                log('%s: reference %s, got %s' % (where, 'None' if want is None else 'tensor', 'None' if have is None else 'tensor'))
                if (want is None) != (have is None):
                    bad.append((step, n, float('inf'), 'None mismatch'))
                continue
            if not torch.is_tensor(want):
                log('%s: %r (reference %r)' % (where, have, want))
                if have != want:
                    bad.append((step, n, float('inf'), '%r vs %r' % (have, want)))
                continue
            have = have.detach().cpu()
            if tuple(have.shape) != tuple(want.shape):
                bad.append((step, n, float('inf'), 'shape %s vs %s' % (tuple(have.shape), tuple(want.shape))))
                continue
            if not want.is_floating_point():
                ndiff = int((have != want).sum())
                log('%s: %d of %d entries differ' % (where, ndiff, want.numel()))
                if ndiff:
                    bad.append((step, n, float('inf'), '%d of %d entries differ' % (ndiff, want.numel())))
                continue
            err = (have.double() - want).abs()
            if _kind(n) == 'stat':
                over = float((err / (R.STAT_ATOL + R.STAT_RTOL * want.abs())).max())
                log('%s: max err %.3g, %.3g of atol + rtol |ref|' % (where, float(err.max()), over))
                if not over <= 1:
                    bad.append((step, n, over, 'running statistic off by %.3g' % float(err.max())))
                continue
            e, sc = _rel(have, want)
            e32, _ = _rel(r32[step][n], want)
            log('%s: %.3g of max|ref| %.3g (stock fp32 %.3g, bound %.3g)' % (where, e, sc, e32, bnd[step][n]))
            group = 'out' if n.endswith(('out', 'loss')) else n.split(':')[0]
            if e > worst.get(group, (-1.0,))[0]:
                worst[group] = (e, n, step, e32, bnd[step][n])
            if not e <= bnd[step][n]:
                bad.append((step, n, e / bnd[step][n], 'err %.3g of scale, bound %.3g' % (e, bnd[step][n])))
    return bad, worst


def check_reference(topo, plan, seed, log=lambda *a: None):
    """What tests/test_train_loop_host.py asserts of one entry, as a list of complaints (empty: the seed serves)."""
    r64, r32, cond = reference(topo, plan, seed)
    wrong = []
    for label, margin, err32, ratio in cond:
        log('%s %s seed %d %s: smallest margin %.3g, stock fp32 off by at most %.3g, smallest margin / own error %.3g'
            % (topo, plan, seed, label, margin, err32, ratio))
        if not ratio >= COND_FACTOR:
            wrong.append('%s: margin / error %.3g < %g' % (label, ratio, COND_FACTOR))
    for step, bs in enumerate(bounds(topo, plan, seed)):
        for n, b in bs.items():
            if not b <= BOUND_MAX:
                wrong.append('step %d %s: bound %.3g' % (step, n, b))
    bad, _ = compare(r32, topo, plan, seed, log=lambda *a: None)
    wrong += ['fp32 reference: step %d %s %s' % (s, n, text) for s, n, _, text in bad]
    # Running statistics have a fixed tolerance, not a multiple of stock fp32's error: the seed has to leave room under it.  A statistic
    # averages the round-off of at least 64 conv outputs, so it depends less on an implementation's summation order than the single
    # elements B_FACTOR = 8 allows for: half of that, stock fp32 within a quarter of the tolerance at every step.
    for step, (ra, rb) in enumerate(zip(r64, r32)):
        for n, want in ra.items():
            if _kind(n) == 'stat' and want.is_floating_point():
                over = float(((rb[n].double() - want).abs() / (R.STAT_ATOL + R.STAT_RTOL * want.abs())).max())
                if not over * STAT_SLACK <= 1:
                    wrong.append('step %d %s: stock fp32 at %.3g of the tolerance' % (step, n, over))
    return wrong


def search_seeds(topo, plan, first=0, count=32):
    """Development aid (python -c 'import _train_loop as T; print(T.search_seeds("R", "P1"))'): the seeds in [first, first + count)
    that meet every condition of check_reference."""
    ok = []
    for seed in range(first, first + count):
        if not check_reference(topo, plan, seed):
            ok.append(seed)
        reference.cache_clear()
    return ok
