"""The PackNet SparsePruner on MI355X: the reference's utils/packnet_prune.py behind the same class API.

It is NOT utils.prune.SparsePruner with the piggymask left off; where the two differ the reference's PackNet lines decide:

    layers covered          every nn.Conv2d / nn.Linear whose name lacks 'classifiers'
    current_dataset_idx     masks[first key].max()                                                    (utils/packnet_prune.py:17-18)
    calculate_sparsity      #(owner > idx) / #(owner >= idx) over the FIRST layer only, 0.0 on an empty denominator -- it reads 0.0
                            right after a prune in the reference, and that is what comes out here      (:101-117)
    task / zero ratio       over the first layer only, both from one cpg_mask_hist of that layer     (:119-143)
    routing                 decay added, then only owner != cur zeroed -> cpg_route_grads             (:146-159)
    prunes                  zero the weights in place -> cpg_rank_prune_zero                          (:64-99)
    make_pruned_zero        after every step (utils/packnet_manager.py:69) -> cpg_zero_pruned, or nothing while a
                            utils.fused_sgd.PackNetSGD is attached: its step pins those weights itself
    apply_mask              -> cpg_apply_mask (:173-183);  make_finetuning_mask -> cpg_claim_free (:185-198)

The only host read-backs are one 32-byte record per layer after a prune (the reference's failing `kthvalue(0)` becomes the
`SystemExit(2)` of utils.prune.SparsePruner) and one histogram of the first layer, cached until a mask mutates.
"""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from .pruner_base import PrunerBase


class SparsePruner(PrunerBase):
    """Performs pruning on the given model (utils/packnet_prune.py:5-20)."""
    RANK_PRUNE = 'cpg_rank_prune_zero'       # owners released and the weights under owner 0 zeroed in its final pass

    def __init__(self, model, masks, args, begin_prune_step, end_prune_step, inference_dataset_idx):
        super().__init__(model, masks, args, begin_prune_step, end_prune_step, inference_dataset_idx)
        valid_key = list(masks.keys())[0]
        self.current_dataset_idx = int(masks[valid_key].max())

    def _layers(self, with_classifiers=False):
        for name, module in self.model.named_modules():
            if isinstance(module, nn.Conv2d) or isinstance(module, nn.Linear):
                if 'classifiers' in name and not with_classifiers:
                    continue
                yield name, module

    def one_shot_prune(self, one_shot_prune_perc):
        """utils/packnet_prune.py:82-99; the prune has zeroed the released weights."""
        print('Pruning for dataset idx: %d' % (self.current_dataset_idx))
        print('Pruning each layer by removing %.2f%% of values' % (100 * one_shot_prune_perc))
        self._rank_prune_layers(one_shot_prune_perc)

    # ------------------------------------------------------------------ statistics (FIRST Conv2d / Linear of the model only: the `break`s)
    def _first_hist(self):
        """(256 owner-id counts, numel) of the first layer's mask; the statistics loops do not skip 'classifiers' (:104-111)."""
        first = next(self._layers(with_classifiers=True), None)
        if first is None:
            return None, 0
        name, module = first
        m = self.masks[name]
        key = (self._mutations, id(m), m._version)
        if key != self._hist_key:
            owner = self._owner(name, module.weight.data)
            hist = torch.zeros(257, dtype=torch.int64, device=owner.device)
            _lib.call('cpg_mask_hist', _lib.dptr(owner, torch.uint8, 'mask'), None, 0, owner.numel(), ctypes.c_void_p(hist.data_ptr()),
                      _lib.stream_ptr())
            self._hist = hist.cpu().tolist()[:256]
            m = self.masks[name]
            self._hist_key = (self._mutations, id(m), m._version)
        return self._hist, self.masks[name].numel()

    def calculate_sparsity(self):
        """#(owner > idx) / #(owner >= idx) (utils/packnet_prune.py:101-117)."""
        h, _ = self._first_hist()
        if h is None:
            return 0.0
        idx = int(self.inference_dataset_idx)
        above = sum(h[idx + 1:])
        total = above + (h[idx] if 0 <= idx < 256 else 0)
        return float(above) / float(total) if total != 0 else 0.0

    def calculate_curr_task_ratio(self):
        """utils/packnet_prune.py:119-130."""
        h, numel = self._first_hist()
        return float(h[int(self.inference_dataset_idx)]) / numel

    def calculate_zero_ratio(self):
        """utils/packnet_prune.py:132-143."""
        h, numel = self._first_hist()
        return float(h[0]) / numel

    # ------------------------------------------------------------------ the step's passes
    def do_weight_decay_and_make_grads_zero(self):
        """grad += weight_decay * w, then grad[owner != cur] = 0 (utils/packnet_prune.py:146-159): one pass per layer.  With a
        PackNetSGD attached this is part of its step."""
        assert self.masks
        if self.fused_weight_step:
            return
        s = _lib.stream_ptr()
        for name, module in self._layers():
            if module.weight.grad is None:
                continue
            w, gw = module.weight.data, module.weight.grad.data
            if not gw.is_contiguous():
                raise RuntimeError('gradient of %s is not contiguous' % name)
            _lib.call('cpg_route_grads', _lib.dptr(gw, name='weight.grad'), _lib.dptr(w, name='weight'),
                      _lib.dptr(self._owner(name, w), torch.uint8, 'mask'), int(self.current_dataset_idx), float(self.args.weight_decay),
                      None, _lib.MODE_FINETUNE, gw.numel(), s)

    def make_pruned_zero(self, force=False):
        """w[owner == 0] = 0 (utils/packnet_prune.py:161-171).  With a PackNetSGD attached its step has done this already; `force`
        runs the pass regardless."""
        assert self.masks
        if self.fused_weight_step and not force:
            return
        super().make_pruned_zero()
