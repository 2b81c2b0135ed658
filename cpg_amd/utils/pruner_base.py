"""The mechanics the two SparsePruners share (utils.prune: CPG, utils.packnet_prune: the PackNet baseline): owner-mask hygiene, the
rank-prune launch loop with its one read-back, the sparsity schedule and its gate, and the elementwise mask passes.  What the
reference makes different -- the layers covered, the `current_dataset_idx` rule, the statistics, the gradient routing and what a
prune leaves in the weights -- stays in the subclasses; nothing here asks which of the two it is serving.
"""
import ctypes
import sys

import torch

from .. import _lib


class PrunerBase(object):
    RANK_PRUNE = None                # the entry point of _rank_prune_layers: cpg_rank_prune, or cpg_rank_prune_zero (zeroes the released weights)

    def __init__(self, model, masks, args, begin_prune_step, end_prune_step, inference_dataset_idx):
        self.model = model
        self.args = args
        self.sparsity_func_exponent = 3
        self.begin_prune_step = begin_prune_step
        self.end_prune_step = end_prune_step
        self.last_prune_step = begin_prune_step
        self.masks = masks
        self.inference_dataset_idx = inference_dataset_idx
        self.fused_weight_step = False   # set by the utils.fused_sgd optimizer that takes the covered weights' part of the step over
        self._mutations = 0              # bumped whenever a kernel of ours rewrites a mask in place
        self._hist_key = None
        self._hist = None
        self.last_prune_records = []
        self.prune_events = 0            # rank-prune events executed (gradually_prune + one_shot_prune)

    def _layers(self):
        """(name, module) of every layer this pruner covers."""
        raise NotImplementedError

    def _owner(self, name, like):
        m = self.masks[name]
        if m.dtype != torch.uint8:
            raise TypeError('mask %s must be uint8 (torch.ByteTensor), got %s' % (name, m.dtype))
        if m.device != like.device or not m.is_contiguous():
            m = m.to(like.device).contiguous()          # (the reference moves masks next to the weights lazily, utils/prune.py:228)
            self.masks[name] = m
        if m.shape != like.shape:
            raise RuntimeError('mask %s has shape %s, weight has %s' % (name, tuple(m.shape), tuple(like.shape)))
        return m

    # ------------------------------------------------------------------ rank prune
    def _rank_prune(self, entry, w, owner, pruning_ratio, res, ws, nbytes, s):
        _lib.call(entry, _lib.dptr(w, name='weight'), _lib.dptr(owner, torch.uint8, 'mask'), int(self.current_dataset_idx),
                  float(pruning_ratio), w.numel(), ctypes.c_void_p(res.data_ptr()), _lib.dptr(ws), nbytes, s)

    def _check_krange(self, statuses):
        if _lib.CPG_E_KRANGE in statuses:
            # utils/prune.py:38-42 (the PackNet reference dies in kthvalue(0) here: one convention for "too few weights")
            print("Not enough weights for pruning, that is to say, too little space for new task, need expand the network.")
            sys.exit(2)

    def _rank_prune_layers(self, pruning_ratio):
        """Launch RANK_PRUNE for every covered layer, then read the result records once."""
        layers = list(self._layers())
        if not layers:
            return []
        dev = layers[0][1].weight.device
        res = torch.zeros(len(layers), _lib.PRUNE_RESULT_BYTES // 8, dtype=torch.int64, device=dev)
        ws, nbytes = _lib.workspace(_lib.lib().cpg_rank_prune_workspace_bytes(), dev)
        s = _lib.stream_ptr()
        for i, (name, module) in enumerate(layers):
            w = module.weight.data
            self._rank_prune(self.RANK_PRUNE, w, self._owner(name, w), pruning_ratio, res[i], ws, nbytes, s)
        self._mutations += 1
        self.prune_events += 1
        raw = res.cpu().numpy().tobytes()
        recs = []
        for i, (name, _) in enumerate(layers):
            r = _lib.PruneResult.from_buffer_copy(raw[i * _lib.PRUNE_RESULT_BYTES:(i + 1) * _lib.PRUNE_RESULT_BYTES])
            recs.append({'layer': name, 'n_candidates': r.n_candidates, 'k': r.k, 'n_released': r.n_released,
                         'cutoff': r.cutoff, 'status': r.status})
        self.last_prune_records = recs
        self._check_krange([r['status'] for r in recs])
        return recs

    def _pruning_mask(self, weights, mask, layer_name, pruning_ratio):
        """Rank one layer by magnitude and release the smallest weights of the current task (utils/prune.py:30-53,
        utils/packnet_prune.py:22-41).  Mutates and returns `mask`; the weights are left alone."""
        weights = weights.contiguous()
        res = torch.zeros(_lib.PRUNE_RESULT_BYTES // 8, dtype=torch.int64, device=weights.device)
        ws, nbytes = _lib.workspace(_lib.lib().cpg_rank_prune_workspace_bytes(), weights.device)
        self._rank_prune('cpg_rank_prune', weights, mask, pruning_ratio, res, ws, nbytes, _lib.stream_ptr())
        self._mutations += 1
        self._check_krange([_lib.PruneResult.from_buffer_copy(res.cpu().numpy().tobytes()).status])
        return mask

    def _adjust_sparsity(self, curr_prune_step):
        """Cubic sparsity schedule (utils/prune.py:55-66, utils/packnet_prune.py:43-53); python floats, bit-identical."""
        p = min(1.0, max(0.0, ((curr_prune_step - self.begin_prune_step)
                               / (self.end_prune_step - self.begin_prune_step))))
        return self.args.target_sparsity + \
            (self.args.initial_sparsity - self.args.target_sparsity) * pow(1 - p, self.sparsity_func_exponent)

    def _time_to_update_masks(self, curr_prune_step):
        """Update gate (utils/prune.py:68-76, utils/packnet_prune.py:55-62)."""
        in_range = self.begin_prune_step <= curr_prune_step <= self.end_prune_step
        due = (self.last_prune_step + self.args.pruning_frequency) <= curr_prune_step
        return in_range and due

    def gradually_prune(self, curr_prune_step):
        """utils/prune.py:78-92, utils/packnet_prune.py:64-80.  Whether the released weights are zeroed at once is RANK_PRUNE's
        business: CPG leaves them stale until the next apply_mask, the PackNet form zeroes them (:77)."""
        if self._time_to_update_masks(curr_prune_step):
            self.last_prune_step = curr_prune_step
            curr_pruning_ratio = self._adjust_sparsity(curr_prune_step)
            self._rank_prune_layers(curr_pruning_ratio)
        else:
            curr_pruning_ratio = self._adjust_sparsity(self.last_prune_step)
        return curr_pruning_ratio

    # ------------------------------------------------------------------ mask application
    def _for_each_layer(self, entry, *args, weights=True):
        """`entry(weight, owner, *args, n, stream)` over every covered layer; weights=False: `entry(owner, *args, n, stream)`."""
        s = _lib.stream_ptr()
        for name, module in self._layers():
            w = module.weight.data
            owner = _lib.dptr(self._owner(name, w), torch.uint8, 'mask')
            if weights:
                _lib.call(entry, _lib.dptr(w, name='weight'), owner, *args, w.numel(), s)
            else:
                _lib.call(entry, owner, *args, w.numel(), s)

    def make_pruned_zero(self):
        """Makes pruned weights 0 (utils/prune.py:213-221, utils/packnet_prune.py:161-171)."""
        assert self.masks
        self._for_each_layer('cpg_zero_pruned')

    def apply_mask(self):
        """Keep only the weights of tasks 1..inference_dataset_idx, destructively (utils/prune.py:223-231, utils/packnet_prune.py:173-183)."""
        self._for_each_layer('cpg_apply_mask', int(self.inference_dataset_idx))

    def make_finetuning_mask(self):
        """Hand every free slot to the next task (utils/prune.py:233-243, utils/packnet_prune.py:185-198)."""
        assert self.masks
        self.current_dataset_idx += 1
        self._for_each_layer('cpg_claim_free', int(self.current_dataset_idx), weights=False)
        self._mutations += 1
