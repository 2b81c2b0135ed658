"""Manager: the per-minibatch train / validate loops of the reference's utils/manager.py:16-152,
driving the HIP-backed SparsePruner and masked layers.

Op order per step is the reference's (utils/manager.py:50-75): zero_grad -> forward -> accuracy ->
loss -> backward -> do_weight_decay_and_make_grads_zero -> optimizers.step -> (prune mode)
gradually_prune -> statistics.  `validate` calls apply_mask() FIRST and leaves the weights mutated,
as the reference does (utils/manager.py:105).

What is not reproduced is the reference's per-step host stall: loss / accuracy accumulate on the
device and the progress line (tqdm postfix with the mask statistics) is refreshed on a wall-clock
interval instead of forcing `.item()` + 15 reductions + `.cpu()` every step; the statistics themselves
ARE evaluated every step / validation batch (one cached histogram pass).  Returned values are identical.  Checkpoint save / load (utils/manager.py:198-320) delegate to
utils/checkpoint.py and keep the reference's file format.  LFW evaluation (evalLFW, :156-195) scores the pair embeddings on the
device (cpg_amd/utils/metrics.py).
"""
import logging
import time

import numpy as np
import torch
import torch.nn as nn

from . import Metric, classification_accuracy
from . import checkpoint as ckpt
from .prune import SparsePruner

try:                                    # progress bar is cosmetic; tqdm is present in the image
    from tqdm import tqdm
except ImportError:                     # pragma: no cover
    tqdm = None


class _NullBar(object):
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def set_postfix(self, *a, **k):
        pass

    def update(self, n=1):
        pass


def make_criterion(args):
    """The task's loss (utils/manager.py:29-36).  OPT-IN (args.fused_loss; default off): loss, accuracy and the first gradient from the
    library's loss-head kernels (cpg_amd/models/losses.py) instead of stock torch; same values to rounding, same criterion state."""
    if getattr(args, 'fused_loss', False):
        from ..models.losses import FusedAngleLoss as AngleLoss, FusedCrossEntropyLoss as CrossEntropyLoss
    else:
        from ..models.spherenet import AngleLoss
        CrossEntropyLoss = nn.CrossEntropyLoss
    if args.dataset == 'face_verification':
        return AngleLoss()
    if args.dataset == 'emotion':
        counts = torch.from_numpy(np.array([74874, 134415, 25459, 14090, 6378, 3803, 24882]).astype(np.float32))
        weights = (torch.sum(counts) - counts) / counts
        return CrossEntropyLoss(weight=weights.cuda() if getattr(args, 'cuda', True) else weights)
    return CrossEntropyLoss()


class ManagerBase(object):
    """What the CPG and PackNet Managers share outside their train / validate loops: the fields both set, the progress line, the
    checkpoint path, the criterion with the forward + loss + accuracy of one batch, and the scoring half of evalLFW."""

    def __init__(self, args, model, shared_layer_info, train_loader, val_loader):
        self.args = args
        self.model = model
        self.shared_layer_info = shared_layer_info
        self.inference_dataset_idx = self._root().datasets.index(args.dataset) + 1
        self.train_loader = train_loader
        self.val_loader = val_loader
        self.progress = bool(getattr(args, 'progress', True)) and tqdm is not None
        self.postfix_interval = float(getattr(args, 'postfix_interval', 0.5))
        self.last_stats = {}
        self.last_lfw = None
        # AngleLoss / class-weighted / plain cross-entropy; stock torch unless args.fused_loss
        self.fused_loss = bool(getattr(args, 'fused_loss', False))
        self.criterion = make_criterion(args)
        # OPT-IN (args.telemetry / args.stop_on_nonfinite; default off, no counterpart in the reference): the masked optimizers handed to
        # train() step through the `_stats` twins of their passes (utils/telemetry.py) -- per-layer records of the epoch's last step in
        # `last_telemetry`, and, with stop_on_nonfinite, TrainingDiverged out of train() once a step went non-finite
        self.stop_on_nonfinite = bool(getattr(args, 'stop_on_nonfinite', False))
        self.telemetry = None
        self.last_telemetry = None
        if getattr(args, 'telemetry', False) or self.stop_on_nonfinite:
            from .telemetry import StepTelemetry
            self.telemetry = StepTelemetry()

    def _telemetry_attach(self, optimizers):
        if self.telemetry is not None:
            self.telemetry.attach(optimizers)

    def _telemetry_guard(self):
        """Raise TrainingDiverged if a step so far went non-finite.  Reads the device: called where the progress line is refreshed and
        at the end of an epoch, never per step."""
        if self.stop_on_nonfinite:
            self.telemetry.check()

    def _telemetry_epoch_end(self):
        if self.telemetry is not None:
            self.last_telemetry = self.telemetry.read()
            self._telemetry_guard()

    def _root(self):
        return ckpt._root(self.model)

    def _bar(self, total, desc):
        return tqdm(total=total, desc=desc, ascii=True) if self.progress else _NullBar()

    def _postfix_due(self, last_post, batch_idx, nbatches):
        """Refresh the progress line now?  On a wall-clock interval since `last_post`, and at the last batch."""
        return self.progress and (time.time() - last_post >= self.postfix_interval or batch_idx + 1 == nbatches)

    def _to_device(self, data, target):
        if getattr(self.args, 'cuda', True):
            data, target = data.cuda(non_blocking=True), target.cuda(non_blocking=True)
        return data, target

    def _path(self, folder, epoch):
        return self.args.checkpoint_format.format(save_folder=folder, epoch=epoch)

    def _loss_and_accuracy(self, data, target, train):
        """(loss, accuracy of the batch or None), in the reference's order of calls: train computes the accuracy before the loss (and none
        for the face task), validate the loss before the accuracy.  Fused: the accuracy comes out of the loss kernel, and in train the face
        task's head takes the embeddings -- the trunk and the 512-wide linear layer in front of AngleLinear are the calls `model(data)` makes."""
        face = self.args.dataset == 'face_verification'
        if self.fused_loss and face and train:
            root = self._root()
            return self.criterion.head_loss(root.forward_to_embeddings(data), root.classifier[1], target), None
        output = self.model(data)
        if self.fused_loss and not face:
            loss = self.criterion(output, target)
            return loss, self.criterion.accuracy
        if train:
            accuracy = None if face else classification_accuracy(output, target)
            return self.criterion(output, target), accuracy
        loss = self.criterion(output, target)
        return loss, classification_accuracy(output, target)

    def score_pairs(self, embeddings, epoch_idx=0, full=False, subtract_mean=False):
        """The scoring half of evalLFW on eval_embeddings' list of (emb_a, emb_p, issame) batches.  By default the 10-fold accuracy
        alone, as evalLFW uses it.  full=True also fills `last_lfw` with VAL@FAR = 1e-3 over the reference's fine table
        np.arange(0, 4, 0.001): 'val_train' / 'far_train' (every fold's training table), 'val', 'val_std', 'far' by the reference's
        rule -- NaN, with the reason in 'val_error', where the reference raises (its interpolation, or a test fold without a "same"
        or a "different" pair: cpg_amd/utils/metrics.py) -- and 'val_first', 'val_first_std', 'far_first' ('val_first_error') at
        each fold's largest threshold whose training FAR stays within the target."""
        from . import metrics
        if not embeddings or not all(isinstance(b, tuple) and len(b) == 3 for b in embeddings):
            raise ValueError('evalLFW needs a validation loader of (a, p, issame) batches')
        emb_a = torch.cat([b[0] for b in embeddings])
        emb_p = torch.cat([b[1] for b in embeddings])
        labels = torch.cat([torch.as_tensor(b[2]).reshape(-1).to(emb_a.device) for b in embeddings])
        dtype = getattr(self.args, 'lfw_threshold_dtype', 'float64')
        # calculate_roc's three steps (the distances are kept for VAL@FAR)
        dist = metrics.fold_distances(emb_a, emb_p, labels, 10, True, subtract_mean)
        tpr, fpr, accuracy = metrics.roc_from_counts(*metrics.roc_counts(np.arange(0, 4, 0.01), dist, labels, 10, dtype))
        extra = self._val_at_far(metrics, dist, labels, dtype) if full else {}
        mean, std = np.mean(accuracy), np.std(accuracy)
        self.last_lfw = dict(extra, tpr=tpr, fpr=fpr, accuracy=accuracy)
        self.last_stats = dict(self.last_stats, accuracy=float(mean), accuracy_std=float(std))
        if self.progress:
            print('In evalLFW(): Test set: Accuracy: {:.5f}+-{:.5f}'.format(mean, std))
        if getattr(self.args, 'log_path', None):
            logging.info(('In evalLFW()-> Validate Epoch #{} '.format(epoch_idx + 1)
                          + 'Test set: Accuracy: {:.5f}+-{:.5f}, '.format(mean, std)
                          + 'task_ratio: {:.2f}'.format(self.pruner.calculate_curr_task_ratio())))
        return mean

    @staticmethod
    def _val_at_far(metrics, dist, labels, dtype, far_target=1e-3):
        thr = metrics._thresholds(np.arange(0, 4, 0.001), dtype)
        val_train, far_train = metrics.val_tables(thr, dist, labels, 10)
        out = {'val_train': val_train, 'far_train': far_train, 'far_target': far_target}
        nan = float('nan')
        for rule, keys in ((metrics.threshold_at_far, ('val', 'val_std', 'far', 'val_error')),
                           (metrics.first_at_far, ('val_first', 'val_first_std', 'far_first', 'val_first_error'))):
            try:        # the interpolation's ValueError, or a test fold without a "same" / "different" pair (ZeroDivisionError)
                val, far = metrics.val_far_at([rule(f, thr, far_target) for f in far_train], dist, labels, 10, dtype)
                out.update(zip(keys, (np.mean(val), np.std(val), np.mean(far))))
            except (ValueError, ZeroDivisionError) as e:
                out.update(zip(keys, (nan, nan, nan, '%s: %s' % (type(e).__name__, e))))
        return out


class Manager(ManagerBase):
    """Handles training and pruning (utils/manager.py:16-37)."""

    def __init__(self, args, model, shared_layer_info, masks, train_loader, val_loader, begin_prune_step, end_prune_step):
        super().__init__(args, model, shared_layer_info, train_loader, val_loader)
        self.pruner = SparsePruner(self.model, masks, self.args, begin_prune_step, end_prune_step,
                                   self.inference_dataset_idx)
        if hasattr(model, 'set_gradient_filter'):
            # data parallel: exchange only the gradient slots that survive the routing below (it runs right after the sync)
            model.set_gradient_filter(self.pruner)
        if getattr(args, 'freeze_gc', False):
            # OPT-IN (args.freeze_gc; no counterpart in the reference): the model, its masks and the pruner exist now -- one full collection,
            # then gc.freeze(): removes the 80 ms generation-2 collector pauses from the step loop (cpg_amd.utils.settle_host_gc: process-wide)
            from . import settle_host_gc
            settle_host_gc()

    def train(self, optimizers, epoch_idx, curr_lrs, curr_prune_step):
        """One epoch of the hot loop (utils/manager.py:39-100). Returns (avg_train_acc, curr_prune_step)."""
        self.model.train()
        self._telemetry_attach(optimizers)
        train_loss = Metric('train_loss')
        train_accuracy = Metric('train_accuracy')
        last_post = 0.0
        nbatches = len(self.train_loader)
        with self._bar(nbatches, 'Train Ep. #{}: '.format(epoch_idx + 1)) as t:
            for batch_idx, (data, target) in enumerate(self.train_loader):
                data, target = self._to_device(data, target)
                optimizers.zero_grad()
                num = data.size(0)
                loss, accuracy = self._loss_and_accuracy(data, target, train=True)
                if accuracy is not None:
                    train_accuracy.update(accuracy, num)
                train_loss.update(loss, num)
                loss.backward()
                # Set fixed param grads to 0 (after the data-parallel all-reduce hooks have filled .grad)
                if hasattr(self.model, 'finish_gradient_sync'):
                    self.model.finish_gradient_sync()
                self.pruner.do_weight_decay_and_make_grads_zero()
                optimizers.step()
                if self.args.mode == 'prune':
                    self.pruner.gradually_prune(curr_prune_step)
                    curr_prune_step += 1
                # the mask statistic of the progress line is computed EVERY step, as the reference does
                # (utils/manager.py:77-88); it is one histogram pass that is cached until a mask mutates
                self.last_stats = {'sparsity': self.pruner.calculate_sparsity()}
                if self._postfix_due(last_post, batch_idx, nbatches):
                    last_post = time.time()
                    t.set_postfix({'loss': train_loss.avg.item(),
                                   'accuracy': '{:.2f}'.format(100. * train_accuracy.avg.item()),
                                   'lr': curr_lrs[0],
                                   'sparsity': self.last_stats['sparsity'],
                                   'network_width_mpl': self.args.network_width_multiplier})
                    self._telemetry_guard()
                t.update(1)
        self._telemetry_epoch_end()
        if getattr(self.model, '_world', 1) > 1:        # data parallel: metrics of the GLOBAL batches, the same on every rank
            pg = getattr(self.model, 'process_group', None)
            train_loss.all_reduce_(pg)
            if self.args.dataset != 'face_verification':
                train_accuracy.all_reduce_(pg)
        summary = {'loss': '{:.3f}'.format(train_loss.avg.item()),
                   'accuracy': '{:.2f}'.format(100. * train_accuracy.avg.item()),
                   'lr': curr_lrs[0],
                   'sparsity': '{:.3f}'.format(self.pruner.calculate_sparsity()),
                   'network_width_mpl': self.args.network_width_multiplier}
        if getattr(self.args, 'log_path', None):
            logging.info(('In train()-> Train Ep. #{} '.format(epoch_idx + 1)
                          + ', '.join(['{}: {}'.format(k, v) for k, v in summary.items()])))
        return train_accuracy.avg.item(), curr_prune_step

    def validate(self, epoch_idx, biases=None):
        """Evaluation (utils/manager.py:103-152): apply_mask() first, then an eval-mode forward pass."""
        self.pruner.apply_mask()
        if hasattr(self.model, 'sync_buffers'):
            self.model.sync_buffers()            # data parallel: evaluate with rank 0's BN running statistics
        self.model.eval()
        val_loss = Metric('val_loss')
        val_accuracy = Metric('val_accuracy')
        idx = self.inference_dataset_idx
        last_post = 0.0
        nbatches = len(self.val_loader)
        with self._bar(nbatches, 'Val Ep. #{}: '.format(epoch_idx + 1)) as t:
            with torch.no_grad():
                for bi, (data, target) in enumerate(self.val_loader):
                    data, target = self._to_device(data, target)
                    num = data.size(0)
                    loss, accuracy = self._loss_and_accuracy(data, target, train=False)
                    val_loss.update(loss, num)
                    val_accuracy.update(accuracy, num)
                    # statistics per validation batch, as the reference (utils/manager.py:126-136); cached histogram
                    stats = {'sparsity': self.pruner.calculate_sparsity(),
                             'task{} ratio'.format(idx): self.pruner.calculate_curr_task_ratio(),
                             'zero ratio': self.pruner.calculate_zero_ratio()}
                    if idx != 1:
                        stats['shared_ratio'] = self.pruner.calculate_shared_part_ratio()
                    self.last_stats = stats
                    if self._postfix_due(last_post, bi, nbatches):
                        last_post = time.time()
                        post = {'loss': val_loss.avg.item(),
                                'accuracy': '{:.2f}'.format(100. * val_accuracy.avg.item())}
                        post.update(stats)
                        post['mpl'] = self.args.network_width_multiplier
                        t.set_postfix(post)
                    t.update(1)
        if getattr(self.model, '_world', 1) > 1:        # data parallel: every rank returns the same accuracy (sharded or replicated loader)
            pg = getattr(self.model, 'process_group', None)
            val_loss.all_reduce_(pg)
            val_accuracy.all_reduce_(pg)
        summary = {'loss': '{:.3f}'.format(val_loss.avg.item()),
                   'accuracy': '{:.2f}'.format(100. * val_accuracy.avg.item()),
                   'sparsity': '{:.3f}'.format(self.pruner.calculate_sparsity()),
                   'task{} ratio'.format(idx): '{:.3f}'.format(self.pruner.calculate_curr_task_ratio()),
                   'zero ratio': '{:.3f}'.format(self.pruner.calculate_zero_ratio()),
                   'mpl': self.args.network_width_multiplier}
        if idx != 1:
            summary['shared_ratio'] = '{:.3f}'.format(self.pruner.calculate_shared_part_ratio())
        if getattr(self.args, 'log_path', None):
            logging.info(('In validate()-> Val Ep. #{} '.format(epoch_idx + 1)
                          + ', '.join(['{}: {}'.format(k, v) for k, v in summary.items()])))
        return val_accuracy.avg.item()

    def eval_embeddings(self, epoch_idx=0):
        """The device half of the reference's evalLFW (utils/manager.py:156-175), which is what CPG_face_main.py runs instead of
        `validate` for the `face_verification` task (:337-341,:370-373,:417): apply_mask() first, eval mode, then
        `forward_to_embeddings` of every validation batch.  Returns the list of embedding tensors (on the device).  A loader
        that yields (a, p, label) pairs, as the reference's LFWDataset does, gives a list of (emb_a, emb_p, label), which evalLFW
        scores."""
        self.pruner.apply_mask()
        if hasattr(self.model, 'sync_buffers'):
            self.model.sync_buffers()
        self.model.eval()
        root = self._root()
        out = []
        with torch.no_grad():
            for batch in self.val_loader:
                if len(batch) == 3:
                    a, p, label = batch
                    a, p = self._to_device(a, p)
                    out.append((root.forward_to_embeddings(a), root.forward_to_embeddings(p), label))
                else:
                    data, _ = self._to_device(*batch)
                    out.append(root.forward_to_embeddings(data))
                self.last_stats = {'sparsity': self.pruner.calculate_sparsity(),
                                   'task{} ratio'.format(self.inference_dataset_idx): self.pruner.calculate_curr_task_ratio()}
        return out

    def evalLFW(self, epoch_idx, full=False, subtract_mean=False):
        """utils/manager.py:156-195: apply_mask(), eval mode, `forward_to_embeddings` of both images of every (a, p, issame) batch
        (eval_embeddings), then fv_evaluate(distance_metric=True, subtract_mean=False) over the reference's thresholds
        np.arange(0, 4, 0.01) -- distances and the 10-fold threshold search on the device, the embeddings never leave it.  Logs
        `Accuracy mean+-std` as the reference does and returns np.mean(accuracy).  args.lfw_threshold_dtype = 'float32' compares
        as numpy 1.x did (cpg_amd/utils/metrics.py); the default is numpy >= 2's fp64 comparison.  Under data parallelism with a
        replicated pair loader every rank scores every pair and returns the same value.  full=True also leaves VAL@FAR = 1e-3 and
        the folds' training tables in `last_lfw`, subtract_mean=True centres every fold on its training mean (score_pairs); the
        return value stays np.mean(accuracy)."""
        return self.score_pairs(self.eval_embeddings(epoch_idx), epoch_idx, full=full, subtract_mean=subtract_mean)

    # ------------------------------------------------------------------ checkpoints (utils/manager.py:198-320)
    def save_checkpoint(self, optimizers, epoch_idx, save_folder):
        """Same dict layout as the reference; optimizer state is not saved (momentum restarts each phase)."""
        ckpt.save_checkpoint(self.model, self.pruner.masks, self.shared_layer_info, self.args.dataset,
                             self._path(save_folder, epoch_idx + 1))

    def load_checkpoint(self, optimizers, resume_from_epoch, save_folder):
        if resume_from_epoch > 0:
            state = torch.load(self._path(save_folder, resume_from_epoch), map_location='cpu', weights_only=False)
            ckpt.load_state(self.model, state['model_state_dict'], for_evaluate=False)

    def load_checkpoint_only_for_evaluate(self, resume_from_epoch, save_folder):
        if resume_from_epoch > 0:
            state = torch.load(self._path(save_folder, resume_from_epoch), map_location='cpu', weights_only=False)
            ckpt.load_state(self.model, state['model_state_dict'], for_evaluate=True)
            ckpt.attach_task_layers(self.model, self.shared_layer_info, self.args.dataset)
