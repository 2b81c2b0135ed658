"""Fused masked SGD.

`MaskedSGD` is a torch.optim.SGD whose step() handles every masked weight (SharableConv2d / SharableLinear
`.weight`) with ONE libcpg_hip.so pass that also performs the reference's gradient routing
(`SparsePruner.do_weight_decay_and_make_grads_zero`, utils/prune.py:203-205); all other parameters (BN affine,
biases, the task head) take torch's own SGD path.  Results equal routing-then-torch-SGD to 1 ulp (the fused
multiply-adds differ in rounding), including the momentum that keeps moving released / frozen weights for a few
steps after their gradient is zeroed (SURVEY 8a note).

Usage (drop-in for CPG_cifar100_main_normal.py:339-341 + utils/manager.py:67-70):

    optimizer_network = MaskedSGD(params_to_optimize_via_SGD, pruner=manager.pruner, lr=lr, momentum=0.9, nesterov=True)
    ...
    loss.backward(); manager.pruner.do_weight_decay_and_make_grads_zero(); optimizers.step()

While a MaskedSGD is attached, `do_weight_decay_and_make_grads_zero()` skips the weight part (piggymask
gradients are still routed there) and step() does it fused; `.grad` ends up routed exactly as before.

OPT-IN step telemetry: `telemetry=StepTelemetry()` (utils/telemetry.py) makes step() call the entry points' `_stats` twins -- the same
update bit for bit, plus one record per layer and a sticky health record reduced in the same pass.  Each optimizer gets its own tables
inside the telemetry object.  Default None: the plain entry points, as ever.
"""
import functools
import os

import torch

from .. import _lib

# CPG_MULTI_TENSOR=0: one cpg_sgd_route_step / cpg_adam_route_step launch per layer (the behaviour up to round 5; A/B switch)
MULTI_TENSOR = os.environ.get('CPG_MULTI_TENSOR', '1') not in ('0', '')


class _RoutedSGD(torch.optim.SGD):
    """What MaskedSGD and PackNetSGD share: a torch.optim.SGD whose step() sends every weight its pruner covers (`pruner._layers()`)
    through `_launch` -- decay, routing and the momentum step in the library's one pass -- and leaves the rest to torch's own SGD."""

    def __init__(self, params, pruner, lr, momentum, nesterov, kw):
        self.telemetry = kw.pop('telemetry', None)
        if kw.get('weight_decay', 0.0) != 0.0 or kw.get('dampening', 0.0) != 0.0:
            raise ValueError('%s mirrors the reference optimizer: weight_decay = dampening = 0 '
                             '(the decay is applied with the gradient routing)' % type(self).__name__)
        super().__init__(params, lr=lr, momentum=momentum, nesterov=nesterov, weight_decay=0.0, dampening=0.0)
        self.pruner = pruner
        self._masked = {}                        # id(param) -> mask name

    def _launch(self, rows, hyper, s, stats=None):
        """Step the (w, grad, momentum, owner, n) rows of one launch; hyper = (cur, wd, lr, momentum, nesterov, first_step).  stats: None, or
        a telemetry step's `stats(entry, multi)` (_launch_stats with the rows bound), which makes the `_stats` twin of `entry` step them."""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        pr = self.pruner
        if not self._masked:
            self._masked = {id(module.weight): name for name, module in pr._layers()}
        s = _lib.stream_ptr()
        held = []
        tab = self.telemetry.tables(self, 'sgd') if self.telemetry is not None else None
        if tab is not None:
            tab.begin()
        for gi, group in enumerate(self.param_groups):
            # every covered weight of the group that shares `first` (no momentum buffer yet / has one) goes into ONE multi-tensor launch
            # (cpg_sgd_route_step_multi: 53 layers of ResNet-50 = 2 launches instead of 53)
            batches = {True: [], False: []}
            names = {True: [], False: []}
            for p in group['params']:
                name = self._masked.get(id(p))
                if name is None or p.grad is None:
                    continue
                state = self.state[p]
                first = state.get('momentum_buffer') is None
                if first:
                    state['momentum_buffer'] = torch.empty_like(p, memory_format=torch.contiguous_format)
                owner = pr._owner(name, p.data)
                batches[first].append((_lib.dptr(p.data, name='weight').value, _lib.dptr(p.grad, name='weight.grad').value,
                                       _lib.dptr(state['momentum_buffer'], name='momentum').value,
                                       _lib.dptr(owner, torch.uint8, 'mask').value, p.numel()))
                names[first].append(name)
                held.append((p, p.grad))
                p.grad = None                    # hide from torch's SGD for the rest of this step
            for first, rows in batches.items():
                if rows:
                    hyper = (int(pr.current_dataset_idx), float(pr.args.weight_decay), float(group['lr']), float(group['momentum']),
                             int(bool(group['nesterov'])), int(first))
                    stats = None if tab is None else functools.partial(_launch_stats, tab, _lib.SgdItem, rows, names[first], hyper, (s,),
                                                                       (gi, first), held[-1][0].device)
                    self._launch(rows, hyper, s, stats)
        loss = super().step(closure)
        for p, g in held:
            p.grad = g
        return loss


def _launch_multi(entry, rows, hyper, s):
    _lib.call(entry, (_lib.SgdItem * len(rows))(*rows), len(rows), *hyper, s)


def _launch_stats(tab, item_type, rows, names, before, after, slot, device, entry, multi):
    """The `_stats` twin of the multi-tensor `entry` on a telemetry step's tables (utils.telemetry._Tables): one call for the rows, or
    (multi False: CPG_MULTI_TENSOR=0 where the plain path honours it) one one-row call per layer, each with a health slot of its own."""
    if multi:
        return tab.call(entry + '_stats', (item_type * len(rows))(*rows), rows, names, before, after, slot, device)
    for row, name in zip(rows, names):
        tab.call(entry + '_stats', (item_type * 1)(row), [row], [name], before, after, (slot, name), device)


class MaskedSGD(_RoutedSGD):
    """The CPG step: every SharableConv2d / SharableLinear `.weight` through cpg_sgd_route_step_multi."""

    def __init__(self, params, pruner, lr, momentum=0.9, nesterov=True, **kw):
        super().__init__(params, pruner, lr, momentum, nesterov, kw)
        pruner.fused_weight_step = True          # tells the pruner to leave masked-weight grads to us

    def _launch(self, rows, hyper, s, stats=None):
        if stats is not None:
            return stats('cpg_sgd_route_step_multi', MULTI_TENSOR)
        if MULTI_TENSOR:
            return _launch_multi('cpg_sgd_route_step_multi', rows, hyper, s)
        for w_, g_, b_, o_, n_ in rows:
            _lib.call('cpg_sgd_route_step', w_, g_, b_, o_, *hyper, n_, s)


class MaskedAdam(torch.optim.Adam):
    """torch.optim.Adam for the piggymasks (CPG_cifar100_main_normal.py:342-346) whose step() handles every
    `module.piggymask` with ONE pass that also performs the piggymask part of the gradient routing
    (utils/prune.py:206-210) -- cpg_adam_route_step.  Other parameters in its groups take torch's own path.  While a
    MaskedAdam is attached, `do_weight_decay_and_make_grads_zero()` leaves piggymask gradients alone; `.grad` ends up
    routed exactly as before, and the optimizer state keeps torch's keys (step, exp_avg, exp_avg_sq)."""

    def __init__(self, params, pruner, lr, betas=(0.9, 0.999), eps=1e-8, telemetry=None, **kw):
        self.telemetry = telemetry
        if kw.get('weight_decay', 0.0) != 0.0 or kw.get('amsgrad', False) or kw.get('maximize', False):
            raise ValueError('MaskedAdam mirrors the reference optimizer: weight_decay = 0, amsgrad = maximize = False')
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=0.0)
        self.pruner = pruner
        pruner.fused_piggymask_step = True
        self._masked = {}

    def _refresh(self):
        self._masked = {id(module.piggymask): name for name, module in self.pruner._layers() if module.piggymask is not None}

    @torch.no_grad()
    def step(self, closure=None):
        self._refresh()                          # piggymasks are re-created between phases (driver._fresh_piggymasks)
        s = _lib.stream_ptr()
        pr = self.pruner
        mode = {'finetune': _lib.MODE_FINETUNE, 'prune': _lib.MODE_PRUNE}.get(pr.args.mode)
        held, idle = [], []
        tab = self.telemetry.tables(self, 'pm') if self.telemetry is not None else None
        if tab is not None:
            tab.begin()
        for gi, group in enumerate(self.param_groups):
            beta1, beta2 = group['betas']
            batches = {}                         # Adam step count -> rows of one multi-tensor launch
            names = {}
            for p in group['params']:
                name = self._masked.get(id(p))
                if name is None or p.grad is None or mode is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = torch.tensor(0.0, dtype=torch.float32)
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    # the moments are exactly zero until the kernel below has run once.  The flag lives IN the state (not in a set of
                    # id(p) beside it), so that load_state_dict() / any replacement of the state drops it with the state it described
                    state['_pristine'] = True
                state['step'] += 1
                held.append((p, p.grad))
                if mode == _lib.MODE_PRUNE and state.get('_pristine', False):
                    # Prune mode routes EVERY piggymask gradient to zero (utils/prune.py:209-210), and this parameter's moments are
                    # still exactly zero: Adam's update is then m = v = 0, pm -= step_size * 0 / eps -- nothing changes, bit for bit.
                    # The whole prune phase of the reference (lr_mask 0, a fresh optimizer per phase) is this case: only the routed
                    # gradient (all zeros) has to be left in .grad -- 4 B per element instead of the 37 B of the full pass.
                    # Telemetry: no kernel runs, so the record is made up on the host when it is read -- all zeros, which is what the
                    # STATS kernel reports for ANY prune-mode step (the kept set of cpg_pm_step_stats is empty outside finetune mode):
                    # zero flips, and `picked` 0 of 0 kept slots (picked_ratio None), the same before and after the moments wake up.
                    if tab is not None:
                        tab.idle.append(name)
                    idle.append(p.grad)
                    p.grad = None
                    continue
                state.pop('_pristine', None)
                owner = pr._owner(name, p.data)
                batches.setdefault(int(state['step']), []).append(
                    (_lib.dptr(p.data, name='piggymask').value, _lib.dptr(p.grad, name='piggymask.grad').value,
                     _lib.dptr(state['exp_avg']).value, _lib.dptr(state['exp_avg_sq']).value,
                     _lib.dptr(owner, torch.uint8, 'mask').value, p.numel()))
                names.setdefault(int(state['step']), []).append(name)
                p.grad = None
            for bi, (step, rows) in enumerate(batches.items()):   # (cpg_adam_route_step_multi: every piggymask of the group in one launch)
                if tab is not None:
                    _launch_stats(tab, _lib.AdamItem, rows, names[step],
                                  (int(pr.current_dataset_idx), mode, float(group['lr']), float(beta1), float(beta2), float(group['eps']), step,
                                   self.telemetry.thr), (s,), (gi, bi), held[-1][0].device, 'cpg_adam_route_step_multi', MULTI_TENSOR)
                    continue
                if not MULTI_TENSOR:
                    for p_, g_, a_, b_, o_, n_ in rows:
                        _lib.call('cpg_adam_route_step', p_, g_, a_, b_, o_, int(pr.current_dataset_idx), mode, float(group['lr']), float(beta1),
                                  float(beta2), float(group['eps']), step, n_, s)
                    continue
                items = (_lib.AdamItem * len(rows))(*rows)
                _lib.call('cpg_adam_route_step_multi', items, len(rows), int(pr.current_dataset_idx), mode, float(group['lr']), float(beta1),
                          float(beta2), float(group['eps']), step, s)
        if idle:
            torch._foreach_zero_(idle)           # (one multi-tensor kernel)
        if len(held) > len(idle):
            pr._pm_mutations += 1                # the kernel wrote through data_ptr(): tensor._version did not move
        loss = super().step(closure)
        for p, g in held:
            p.grad = g
        return loss


class PackNetSGD(_RoutedSGD):
    """MaskedSGD's counterpart for the PackNet baseline stack (packnet_cifar100_main_normal.py:229-230 + utils/packnet_manager.py:63-69):
    a torch.optim.SGD whose step() sends every weight the PackNet pruner covers (utils.packnet_prune.SparsePruner: each nn.Conv2d /
    nn.Linear outside `classifiers`) through ONE multi-tensor pass that adds the weight decay, routes the gradient, takes the
    momentum step and pins the weights nobody owns to zero -- cpg_sgd_route_zero_step_multi.  BatchNorm, biases and the active head take
    torch's own SGD path.  `.grad` is left routed as the reference leaves it.

    mode:
        'fused'      (default) the pass above; the pruner's do_weight_decay_and_make_grads_zero() and make_pruned_zero() skip the
                     covered weights while this optimizer is attached.  The default by measurement: profiles/packnet.md.
        'step+zero'  cpg_sgd_route_step_multi, then one cpg_zero_pruned per layer: the best composition of the entry points that
                     existed before the fused pass (bit-equal results, one more pass and one launch per layer).
        'unfused'    the reference's op sequence on the library's kernels: the pruner routes (cpg_route_grads), torch's SGD steps, the
                     pruner zeroes (cpg_zero_pruned); this class then is a plain torch.optim.SGD.  Equal to 'fused' to the rounding of
                     the fused multiply-adds (tests/test_packnet_gpu.py).
    """
    MODES = ('fused', 'step+zero', 'unfused')

    def __init__(self, params, pruner, lr, momentum=0.9, nesterov=True, mode='fused', **kw):
        if mode not in self.MODES:
            raise ValueError('PackNetSGD mode must be one of %s, got %r' % (', '.join(self.MODES), mode))
        if mode == 'unfused' and kw.get('telemetry') is not None:
            raise ValueError("PackNetSGD mode 'unfused' steps through torch's own SGD: there is no pass for the step telemetry to ride in")
        super().__init__(params, pruner, lr, momentum, nesterov, kw)
        self.mode = mode
        pruner.fused_weight_step = mode != 'unfused'

    def detach(self):
        """Hand decay, routing and zeroing back to the pruner's own methods (another optimizer takes over)."""
        self.pruner.fused_weight_step = False

    def _launch(self, rows, hyper, s, stats=None):
        if stats is not None:            # ('step+zero': the records describe the weights before the zero pin below)
            stats('cpg_sgd_route_zero_step_multi' if self.mode == 'fused' else 'cpg_sgd_route_step_multi', True)
            if self.mode == 'fused':
                return
        elif self.mode == 'fused':
            return _launch_multi('cpg_sgd_route_zero_step_multi', rows, hyper, s)
        else:
            _launch_multi('cpg_sgd_route_step_multi', rows, hyper, s)
        for w_, _, _, o_, n_ in rows:
            _lib.call('cpg_zero_pruned', w_, o_, n_, s)

    def step(self, closure=None):
        if self.mode == 'unfused':
            if self.telemetry is not None:
                raise RuntimeError("PackNetSGD mode 'unfused' cannot feed a StepTelemetry")
            return torch.optim.SGD.step(self, closure)
        return super().step(closure)
