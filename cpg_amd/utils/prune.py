"""SparsePruner on MI355X: the reference's utils/prune.py behind the same class API.

Every method keeps the reference's name, arguments and observable effect; the per-layer tensor
work is one libcpg_hip.so call each (include/cpg_hip.h):

    _pruning_mask / gradually_prune / one_shot_prune   -> cpg_rank_prune   (utils/prune.py:30-109)
    calculate_* (4 statistics)                         -> cpg_mask_hist    (utils/prune.py:111-193)
    do_weight_decay_and_make_grads_zero                -> cpg_route_grads  (utils/prune.py:195-211)
    make_pruned_zero / apply_mask                      -> cpg_zero_pruned / cpg_apply_mask (:213-231)
    make_finetuning_mask                               -> cpg_claim_free   (utils/prune.py:233-243)

Differences that are deliberate (values identical, stalls removed):
  * the k-th-value search runs on the device (the reference copies every layer to the host);
    the only host read-back is one 32-byte result record per layer after a prune event, needed to
    reproduce the reference's `sys.exit(2)` when a layer has too few candidates;
  * the four statistics share one histogram pass and are cached until a mask (or, for the shared
    ratio, a piggymask) is mutated -- detected through tensor._version plus an internal counter.
"""
import ctypes
import sys

import torch

from .. import _lib
from ..models import layers as nl
from .checkpoint import _root
from .pruner_base import PrunerBase


def _masked(module):
    return isinstance(module, (nl.SharableConv2d, nl.SharableLinear))


class SparsePruner(PrunerBase):
    """Performs pruning on the given model (utils/prune.py:6-28)."""
    RANK_PRUNE = 'cpg_rank_prune'
    _epochs = 0

    def __init__(self, model, masks, args, begin_prune_step, end_prune_step, inference_dataset_idx):
        super().__init__(model, masks, args, begin_prune_step, end_prune_step, inference_dataset_idx)
        datasets = _root(model).datasets
        again = bool(getattr(args, 'finetune_again', False))
        if args.mode in ('prune', 'inference') or (args.mode == 'finetune' and again):
            self.current_dataset_idx = datasets.index(args.dataset) + 1
        elif args.mode == 'finetune':
            self.current_dataset_idx = len(datasets) - 1
        else:
            print("We do not support '{}' mode".format(args.mode))
            sys.exit(-1)
        self.fused_piggymask_step = False   # set by utils.fused_sgd.MaskedAdam: it routes piggymask grads itself
        SparsePruner._epochs += 1
        self._epoch = SparsePruner._epochs      # distinguishes this pruner's mutation counter from an earlier pruner's (plan caches)
        self._pm_mutations = 0       # bumped when a kernel of ours rewrites a piggymask through its raw pointer (MaskedAdam)

    def _layers(self):
        for name, module in self.model.named_modules():
            if _masked(module):
                yield name, module

    def one_shot_prune(self, one_shot_prune_perc):
        """utils/prune.py:94-109: fixed-ratio prune, then zero the released weights."""
        print('Pruning for dataset idx: %d' % (self.current_dataset_idx))
        print('Pruning each layer by removing %.2f%% of values' % (100 * one_shot_prune_perc))
        self._rank_prune_layers(one_shot_prune_perc)
        self.make_pruned_zero()

    # ------------------------------------------------------------------ statistics
    def _histogram(self, with_piggymask=False):
        """257-entry count vector over all masked layers: [#owner==id for id in 0..255] + [#picked]."""
        layers = list(self._layers())
        key = (self._mutations, self._pm_mutations if with_piggymask else 0, with_piggymask, self.inference_dataset_idx,
               tuple((id(self.masks[n]), self.masks[n]._version) for n, _ in layers),
               tuple((id(m.piggymask), m.piggymask._version) for _, m in layers if m.piggymask is not None)
               if with_piggymask else ())
        if key == self._hist_key:
            return self._hist
        if not layers:
            return [0] * 257
        dev = layers[0][1].weight.device
        hist = torch.zeros(257, dtype=torch.int64, device=dev)
        s = _lib.stream_ptr()
        for name, module in layers:
            owner = self._owner(name, module.weight.data)
            pm = None
            if with_piggymask:
                pm = module.piggymask.data.contiguous()       # AttributeError on None, as in the reference
            _lib.call('cpg_mask_hist', _lib.dptr(owner, torch.uint8, 'mask'), _lib.dptr(pm, name='piggymask'), int(self.inference_dataset_idx),
                      owner.numel(), ctypes.c_void_p(hist.data_ptr()), s)
        self._hist = hist.cpu().tolist()
        self._hist_key = key
        return self._hist

    def _numel(self):
        return sum(self.masks[n].numel() for n, _ in self._layers())

    def calculate_sparsity(self):
        """#free / #(free or owned by the inference task) (utils/prune.py:111-136)."""
        h = self._histogram()
        idx = self.inference_dataset_idx
        total = h[0] + (h[idx] if 0 < idx < 256 else 0)
        return float(h[0]) / float(total) if total != 0 else 0.0

    def calculate_curr_task_ratio(self):
        """utils/prune.py:138-157."""
        h = self._histogram()
        return float(h[self.inference_dataset_idx]) / self._numel() * (self.args.network_width_multiplier ** 2)

    def calculate_zero_ratio(self):
        """utils/prune.py:159-178."""
        h = self._histogram()
        return float(h[0]) / self._numel() * (self.args.network_width_multiplier ** 2)

    def calculate_shared_part_ratio(self):
        """Share of older tasks' weights picked by the piggymask (utils/prune.py:180-193)."""
        h = self._histogram(with_piggymask=True)
        total = sum(h[1:self.inference_dataset_idx])
        return float(h[256]) / float(total) if total != 0 else 0.0

    # ------------------------------------------------------------------ gradient routing
    def do_weight_decay_and_make_grads_zero(self):
        """Sets grads of fixed weights to 0 (utils/prune.py:195-211), one fused pass per layer."""
        assert self.masks
        s = _lib.stream_ptr()
        mode = {'finetune': _lib.MODE_FINETUNE, 'prune': _lib.MODE_PRUNE}.get(self.args.mode)
        for name, module in self._layers():
            w = module.weight
            if self.fused_weight_step:
                # weight part deferred to MaskedSGD.step(); only the piggymask gradient is routed here
                pm = module.piggymask
                if pm is None or pm.grad is None or mode is None or self.fused_piggymask_step:
                    continue       # (piggymask gradients are routed inside MaskedAdam.step() when one is attached)
                owner = self._owner(name, w.data)
                scratch = torch.zeros_like(w.data)
                _lib.call('cpg_route_grads', _lib.dptr(scratch), _lib.dptr(w.data.contiguous(), name='weight'), _lib.dptr(owner, torch.uint8, 'mask'),
                          int(self.current_dataset_idx), 0.0, _lib.dptr(pm.grad.data, name='piggymask.grad'), mode, scratch.numel(), s)
                continue
            if w.grad is None:
                # the reference still routes a piggymask grad here; without a weight grad only that part applies
                gw = None
            else:
                gw = w.grad.data
            pm = module.piggymask
            gpm = pm.grad.data if (pm is not None and pm.grad is not None and mode is not None and not self.fused_piggymask_step) else None
            if gw is None and gpm is None:
                continue
            owner = self._owner(name, w.data)
            if gw is None:
                # rare: only the piggymask received a gradient; run the routing on a scratch weight grad
                gw = torch.zeros_like(w.data)
            if not gw.is_contiguous() or (gpm is not None and not gpm.is_contiguous()):
                raise RuntimeError('gradient of %s is not contiguous' % name)
            _lib.call('cpg_route_grads', _lib.dptr(gw, name='weight.grad'), _lib.dptr(w.data.contiguous(), name='weight'),
                      _lib.dptr(owner, torch.uint8, 'mask'), int(self.current_dataset_idx), float(self.args.weight_decay),
                      _lib.dptr(gpm, name='piggymask.grad'), mode if mode is not None else _lib.MODE_FINETUNE, gw.numel(), s)
