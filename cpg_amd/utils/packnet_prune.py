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
import sys

import torch
import torch.nn as nn

from .. import _lib


class SparsePruner(object):
    """Performs pruning on the given model (utils/packnet_prune.py:5-20)."""

    def __init__(self, model, masks, args, begin_prune_step, end_prune_step, inference_dataset_idx):
        self.model = model
        self.args = args
        self.sparsity_func_exponent = 3
        self.begin_prune_step = begin_prune_step
        self.end_prune_step = end_prune_step
        self.last_prune_step = begin_prune_step
        self.masks = masks
        valid_key = list(masks.keys())[0]
        self.current_dataset_idx = int(masks[valid_key].max())
        self.inference_dataset_idx = inference_dataset_idx
        self.fused_weight_step = False   # set by utils.fused_sgd.PackNetSGD: decay, routing and make_pruned_zero of the masked weights are its step
        self._mutations = 0              # bumped whenever a kernel of ours rewrites a mask in place
        self._hist_key = None
        self._hist = None
        self.last_prune_records = []
        self.prune_events = 0

    # ------------------------------------------------------------------ helpers
    def _layers(self, with_classifiers=False):
        for name, module in self.model.named_modules():
            if isinstance(module, nn.Conv2d) or isinstance(module, nn.Linear):
                if 'classifiers' in name and not with_classifiers:
                    continue
                yield name, module

    def _owner(self, name, like):
        m = self.masks[name]
        if m.dtype != torch.uint8:
            raise TypeError('mask %s must be uint8 (torch.ByteTensor), got %s' % (name, m.dtype))
        if m.device != like.device or not m.is_contiguous():
            m = m.to(like.device).contiguous()          # (the reference moves masks next to the weights lazily, :180)
            self.masks[name] = m
        if m.shape != like.shape:
            raise RuntimeError('mask %s has shape %s, weight has %s' % (name, tuple(m.shape), tuple(like.shape)))
        return m

    @staticmethod
    def _weight(name, module):
        w = module.weight.data
        if not w.is_contiguous():
            raise RuntimeError('weight of %s is not contiguous' % name)
        return w

    # ------------------------------------------------------------------ rank prune
    def _krange_exit(self):
        # the reference dies in kthvalue(0) here; the project's convention for "too few weights" is utils/prune.py's exit code
        print("Not enough weights for pruning, that is to say, too little space for new task, need expand the network.")
        sys.exit(2)

    def _rank_prune_layers(self, pruning_ratio):
        """cpg_rank_prune_zero for every covered layer (owners released and weights under owner 0 zeroed in its final pass), then
        the result records in one read."""
        layers = list(self._layers())
        if not layers:
            return []
        dev = layers[0][1].weight.device
        res = torch.zeros(len(layers), _lib.PRUNE_RESULT_BYTES // 8, dtype=torch.int64, device=dev)
        ws, nbytes = _lib.workspace(_lib.lib().cpg_rank_prune_workspace_bytes(), dev)
        s = _lib.stream_ptr()
        for i, (name, module) in enumerate(layers):
            w = self._weight(name, module)
            _lib.call('cpg_rank_prune_zero', _lib.dptr(w, name='weight'), _lib.dptr(self._owner(name, w), torch.uint8, 'mask'),
                      int(self.current_dataset_idx), float(pruning_ratio), w.numel(), ctypes.c_void_p(res[i].data_ptr()), _lib.dptr(ws),
                      nbytes, s)
        self._mutations += 1
        self.prune_events += 1
        raw = res.cpu().numpy().tobytes()
        recs = []
        for i, (name, _) in enumerate(layers):
            r = _lib.PruneResult.from_buffer_copy(raw[i * _lib.PRUNE_RESULT_BYTES:(i + 1) * _lib.PRUNE_RESULT_BYTES])
            recs.append({'layer': name, 'n_candidates': r.n_candidates, 'k': r.k, 'n_released': r.n_released, 'cutoff': r.cutoff,
                         'status': r.status})
        self.last_prune_records = recs
        if any(r['status'] == _lib.CPG_E_KRANGE for r in recs):
            self._krange_exit()
        return recs

    def _pruning_mask(self, weights, mask, layer_name, pruning_ratio):
        """Rank one layer and release the smallest weights of the current task (utils/packnet_prune.py:22-41).  Mutates and returns
        `mask`; the weights are left alone here, as in the reference (its callers zero them)."""
        weights = weights.contiguous()
        res = torch.zeros(_lib.PRUNE_RESULT_BYTES // 8, dtype=torch.int64, device=weights.device)
        ws, nbytes = _lib.workspace(_lib.lib().cpg_rank_prune_workspace_bytes(), weights.device)
        _lib.call('cpg_rank_prune', _lib.dptr(weights, name='weights'), _lib.dptr(mask, torch.uint8, 'mask'), int(self.current_dataset_idx),
                  float(pruning_ratio), weights.numel(), ctypes.c_void_p(res.data_ptr()), _lib.dptr(ws), nbytes, _lib.stream_ptr())
        self._mutations += 1
        if _lib.PruneResult.from_buffer_copy(res.cpu().numpy().tobytes()).status == _lib.CPG_E_KRANGE:
            self._krange_exit()
        return mask

    def _adjust_sparsity(self, curr_prune_step):
        """Cubic sparsity schedule (utils/packnet_prune.py:43-53); python floats."""
        p = min(1.0, max(0.0, ((curr_prune_step - self.begin_prune_step) / (self.end_prune_step - self.begin_prune_step))))
        return self.args.target_sparsity + \
            (self.args.initial_sparsity - self.args.target_sparsity) * pow(1 - p, self.sparsity_func_exponent)

    def _time_to_update_masks(self, curr_prune_step):
        """utils/packnet_prune.py:55-62."""
        in_range = self.begin_prune_step <= curr_prune_step <= self.end_prune_step
        return in_range and (self.last_prune_step + self.args.pruning_frequency) <= curr_prune_step

    def gradually_prune(self, curr_prune_step):
        """utils/packnet_prune.py:64-80: the PackNet form zeroes the released weights at once (:77)."""
        if self._time_to_update_masks(curr_prune_step):
            self.last_prune_step = curr_prune_step
            curr_pruning_ratio = self._adjust_sparsity(curr_prune_step)
            self._rank_prune_layers(curr_pruning_ratio)
        else:
            curr_pruning_ratio = self._adjust_sparsity(self.last_prune_step)
        return curr_pruning_ratio

    def one_shot_prune(self, one_shot_prune_perc):
        """utils/packnet_prune.py:82-99."""
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
            w, gw = self._weight(name, module), module.weight.grad.data
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
        s = _lib.stream_ptr()
        for name, module in self._layers():
            w = self._weight(name, module)
            _lib.call('cpg_zero_pruned', _lib.dptr(w, name='weight'), _lib.dptr(self._owner(name, w), torch.uint8, 'mask'), w.numel(), s)

    def apply_mask(self):
        """Keep only the weights of tasks 1..inference_dataset_idx, destructively (utils/packnet_prune.py:173-183)."""
        s = _lib.stream_ptr()
        for name, module in self._layers():
            w = self._weight(name, module)
            _lib.call('cpg_apply_mask', _lib.dptr(w, name='weight'), _lib.dptr(self._owner(name, w), torch.uint8, 'mask'),
                      int(self.inference_dataset_idx), w.numel(), s)

    def make_finetuning_mask(self):
        """Hand every free slot to the next task (utils/packnet_prune.py:185-198)."""
        assert self.masks
        self.current_dataset_idx += 1
        s = _lib.stream_ptr()
        for name, module in self._layers():
            owner = self._owner(name, module.weight.data)
            _lib.call('cpg_claim_free', _lib.dptr(owner, torch.uint8, 'mask'), int(self.current_dataset_idx), owner.numel(), s)
        self._mutations += 1
