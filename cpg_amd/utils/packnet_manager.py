"""Manager of the PackNet baseline stack: the train / validate loops and checkpoint format of the reference's utils/packnet_manager.py,
driving utils.packnet_prune.SparsePruner and the packnet_models.

Op order per step is the reference's (utils/packnet_manager.py:46-75): zero_grad -> forward -> accuracy -> loss -> backward ->
do_weight_decay_and_make_grads_zero -> optimizers.step -> make_pruned_zero -> sparsity.  With a utils.fused_sgd.PackNetSGD as the
optimizer the two pruner calls leave the covered weights to its one fused pass.  `validate` calls apply_mask() FIRST and leaves the
weights mutated (:81).  As in utils.manager.Manager, loss and accuracy accumulate on the device and the progress line is refreshed on a
wall-clock interval; returned values are the reference's.

Checkpoints keep the reference's dictionary (:175-182) and its `shared_layer_info[dataset]` keys -- conv_bias, bn_layer_running_mean /
_var / _weight / _bias, fc_bias (and prelu_layer_weight where the dictionary has it) -- so files written by either implementation load
in the other.  BatchNorm, conv bias and fc bias are trained by every task and stashed per task there; COPIES are stored and copied
back (utils/checkpoint.py explains why one process needs that).  `args.fused_loss` (opt-in, off by default) selects the loss-head
kernels exactly as in utils.manager.Manager.  evalLFW (:109-144) scores LFW pairs through cpg_amd/utils/metrics.py on the device.
"""
import logging
import time
import torch
import torch.nn as nn

from . import Metric
from .checkpoint import _HEAD_ALIAS, _put, _snap, restore_norm, stash_norm
from .manager import ManagerBase
from .packnet_prune import SparsePruner

TASK_KEYS = ('conv_bias', 'bn_layer_running_mean', 'bn_layer_running_var', 'bn_layer_weight', 'bn_layer_bias', 'fc_bias')


def new_task_info(prelu=False):
    """shared_layer_info[dataset] as the reference creates it (packnet_cifar100_main_normal.py:143-151, packnet_imagenet_main.py:199-207);
    prelu: with the `prelu_layer_weight` key of the face flow (packnet_face_main.py:175-184)."""
    return {k: {} for k in TASK_KEYS + (('prelu_layer_weight',) if prelu else ())}


def has_prelu(model):
    return any(isinstance(m, nn.PReLU) for m in model.modules())


def make_masks(model):
    """All-free owner masks for every covered layer, keyed as `model.named_modules()` names them (:178-186)."""
    return {name: torch.zeros(m.weight.shape, dtype=torch.uint8, device=m.weight.device) for name, m in model.named_modules()
            if isinstance(m, (nn.Conv2d, nn.Linear)) and 'classifiers' not in name}


class Manager(ManagerBase):
    """Handles training and pruning (utils/packnet_manager.py:13-33)."""

    def __init__(self, args, model, shared_layer_info, masks, train_loader, val_loader):
        super().__init__(args, model, shared_layer_info, train_loader, val_loader)
        self.pruner = SparsePruner(self.model, masks, self.args, None, None, self.inference_dataset_idx)

    def train(self, optimizers, epoch_idx, curr_lrs):
        """One epoch (utils/packnet_manager.py:35-76).  Returns the average train accuracy."""
        self.model.train()
        self._telemetry_attach(optimizers)
        train_loss, train_accuracy = Metric('train_loss'), Metric('train_accuracy')
        last_post, nbatches = 0.0, len(self.train_loader)
        with self._bar(nbatches, 'Train Epoch #{}: '.format(epoch_idx + 1)) as t:
            for batch_idx, (data, target) in enumerate(self.train_loader):
                data, target = self._to_device(data, target)
                optimizers.zero_grad()
                num = data.size(0)
                loss, accuracy = self._loss_and_accuracy(data, target, train=True)
                if accuracy is not None:
                    train_accuracy.update(accuracy, num)
                train_loss.update(loss, num)
                loss.backward()
                self.pruner.do_weight_decay_and_make_grads_zero()
                optimizers.step()
                self.pruner.make_pruned_zero()
                self.last_stats = {'sparsity': self.pruner.calculate_sparsity()}
                if self._postfix_due(last_post, batch_idx, nbatches):
                    last_post = time.time()
                    t.set_postfix({'loss': train_loss.avg.item(), 'accuracy': '{:.2f}'.format(100. * train_accuracy.avg.item()),
                                   'lr': curr_lrs[0], 'sparsity': self.last_stats['sparsity']})
                    self._telemetry_guard()
                t.update(1)
        self._telemetry_epoch_end()
        acc = train_accuracy.avg.item()
        if getattr(self.args, 'log_path', None):
            logging.info('In train()-> Train Ep. #{} loss: {:.3f}, accuracy: {:.2f}, lr: {}'.format(
                epoch_idx + 1, train_loss.avg.item(), 100. * acc, curr_lrs[0]))
        return acc

    def validate(self, epoch_idx, biases=None):
        """Evaluation (utils/packnet_manager.py:79-105): apply_mask() first, then an eval-mode forward pass."""
        self.pruner.apply_mask()
        self.model.eval()
        val_loss, val_accuracy = Metric('val_loss'), Metric('val_accuracy')
        idx = self.inference_dataset_idx
        last_post, nbatches = 0.0, len(self.val_loader)
        with self._bar(nbatches, 'Validate Epoch  #{}: '.format(epoch_idx + 1)) as t:
            with torch.no_grad():
                for bi, (data, target) in enumerate(self.val_loader):
                    data, target = self._to_device(data, target)
                    num = data.size(0)
                    loss, accuracy = self._loss_and_accuracy(data, target, train=False)
                    val_loss.update(loss, num)
                    val_accuracy.update(accuracy, num)
                    self.last_stats = {'sparsity': self.pruner.calculate_sparsity(),
                                       'task{} ratio'.format(idx): self.pruner.calculate_curr_task_ratio(),
                                       'zero ratio': self.pruner.calculate_zero_ratio()}
                    if self._postfix_due(last_post, bi, nbatches):
                        last_post = time.time()
                        t.set_postfix(dict({'loss': val_loss.avg.item(), 'accuracy': '{:.2f}'.format(100. * val_accuracy.avg.item())},
                                           **self.last_stats))
                    t.update(1)
        return val_accuracy.avg.item()

    def eval_embeddings(self, epoch_idx=0):
        """The device half of evalLFW (utils/packnet_manager.py:112-136): eval mode and `forward_to_embeddings` of both images of every
        (a, p, issame) batch.  Unlike `validate` -- and unlike the CPG Manager's evalLFW -- the reference applies NO mask here: the live
        weights are scored.  Returns [(emb_a, emb_p, issame)], embeddings on the device."""
        self.model.eval()
        root = self._root()
        out = []
        with torch.no_grad():
            for a, p, label in self.val_loader:
                a, p = self._to_device(a, p)
                out.append((root.forward_to_embeddings(a), root.forward_to_embeddings(p), label))
        return out

    def evalLFW(self, epoch_idx, full=False, subtract_mean=False):
        """utils/packnet_manager.py:109-144: fv_evaluate(distance_metric=True, subtract_mean=False) over the pair embeddings, on the
        scoring path of utils.manager.Manager.evalLFW (cpg_amd/utils/metrics.py: distances and the 10-fold threshold search on the device;
        args.lfw_threshold_dtype as there; full and subtract_mean as there too).  Returns np.mean(accuracy)."""
        return self.score_pairs(self.eval_embeddings(epoch_idx), epoch_idx, full=full, subtract_mean=subtract_mean)

    def one_shot_prune(self, one_shot_prune_perc):
        self.pruner.one_shot_prune(one_shot_prune_perc)

    # ------------------------------------------------------------------ checkpoints (utils/packnet_manager.py:151-239)
    def collect_task_layers(self):
        """Refresh shared_layer_info[dataset] from the live modules (:155-173)."""
        info = self.shared_layer_info.setdefault(self.args.dataset, new_task_info(has_prelu(self._root())))
        for name, module in self._root().named_modules():
            if isinstance(module, nn.Conv2d):
                if module.bias is not None:
                    info['conv_bias'][name] = _snap(module.bias)
            elif isinstance(module, nn.Linear):
                if 'features' in name:
                    info['fc_bias'][name] = _snap(module.bias)
            else:
                stash_norm(info, name, module)       # (prelu_layer_weight: KeyError without the key, as in the reference)
        return info

    def attach_task_layers(self):
        """Give the model the task's own BatchNorm, conv bias, fc bias and PReLU slopes (:221-239)."""
        info = self.shared_layer_info[self.args.dataset]
        for name, module in self._root().named_modules():
            if isinstance(module, nn.Conv2d):
                if module.bias is not None:
                    _put(module.bias, info['conv_bias'][name])
            elif isinstance(module, nn.Linear):
                if 'features' in name:
                    _put(module.bias, info['fc_bias'][name])
            else:
                restore_norm(info, name, module)

    def checkpoint_dict(self):
        self.collect_task_layers()
        root = self._root()
        return {'model_state_dict': root.state_dict(), 'dataset_history': root.datasets, 'dataset2num_classes': root.dataset2num_classes,
                'masks': self.pruner.masks, 'shared_layer_info': self.shared_layer_info}

    def save_checkpoint(self, optimizers, epoch_idx, save_folder):
        torch.save(self.checkpoint_dict(), self._path(save_folder, epoch_idx + 1))

    def _load_state(self, state_dict):
        cur = self._root().state_dict()
        with torch.no_grad():
            for name, param in state_dict.items():
                if name in _HEAD_ALIAS:              # the `classifier.*` alias of the active head (:196-199)
                    continue
                cur[name].copy_(param)

    def load_checkpoint(self, optimizers, resume_from_epoch, save_folder):
        if resume_from_epoch > 0:
            state = torch.load(self._path(save_folder, resume_from_epoch), map_location='cpu', weights_only=False)
            self._load_state(state['model_state_dict'])

    def load_checkpoint_for_inference(self, resume_from_epoch, save_folder):
        if resume_from_epoch > 0:
            state = torch.load(self._path(save_folder, resume_from_epoch), map_location='cpu', weights_only=False)
            self._load_state(state['model_state_dict'])
            self.attach_task_layers()
