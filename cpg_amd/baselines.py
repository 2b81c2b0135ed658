"""The baselines of the reference's result tables in one process: what cpg_amd.driver.CPGSession is for the CPG loop.

The reference runs one `python packnet_cifar100_main_normal.py` per phase and passes state through checkpoint files; BaselineSession
keeps the models, owner masks and `shared_layer_info` resident and runs the same phases back to back:

    scratch_task    experiment1/baseline_cifar100.sh   a fresh model per task, `--mode finetune`; its validation accuracies are the
                                                       goals CPG grows the network against (logs/baseline_cifar100_acc.txt)
    finetune_task   experiment1/finetune_cifar100.sh   the same, warm-started from another task's model
                                                       (packnet_cifar100_main_normal.py:155-176: every tensor but num_batches_tracked)
    packnet_task    experiment1/PackNet_cifar100.sh    all tasks in ONE network: claim the free slots -> finetune -> validate ->
                                                       one-shot prune -> retrain at the fixed mask
    evaluate        `--mode inference`

Per phase, as in packnet_cifar100_main_normal.py: a fresh SGD(momentum 0.9, nesterov, weight_decay 0) over everything but the other
tasks' heads (:216-230) -- utils.fused_sgd.PackNetSGD, the decay is applied with the gradient routing --, the learning rate times 0.1
after epochs 50 and 80 in finetune and after epoch 25 in prune (:258-268), a validate after every epoch, the last epoch's numbers
recorded.  The pruned stage of a PackNet task is kept only if its train accuracy exceeds `min_train_acc` (0.97, :297); otherwise the
session goes back to the finetuned stage and records kept=False (the reference then has no checkpoint in the task's one_shot_prune
folder at all, and its next task would start from nothing; here a further packnet_task raises: no free slot is left).  Data loading
is whatever iterable of (images, labels) the caller provides.  Multi-GPU baselines are out of scope.

    goals = session.accuracy_goals()                      # {dataset: '0.8123'}, the logfile's content (:283-290)
    session.write_logfile(path); goals = read_goals(path)
    cpg_session.run_task(dataset, ..., accuracy_goal=float(goals[dataset]))
"""
import copy
import json
import os
import types

import torch

from . import packnet_models
from .driver import _Plain
from .utils import Optimizers
from .utils.fused_sgd import PackNetSGD
from .utils.packnet_manager import Manager, make_masks, new_task_info

LR_DROPS = {'finetune': (50, 80), 'prune': (25,)}          # packnet_cifar100_main_normal.py:258-268


def lr_after_epoch(lr, mode, epoch_idx):
    """The learning rate after epoch `epoch_idx` (0-based) has run."""
    return lr * 0.1 if epoch_idx + 1 in LR_DROPS[mode] else lr


def lr_schedule(lr, mode, epochs):
    """The learning rate each of `epochs` epochs trains with."""
    out = []
    for e in range(epochs):
        out.append(lr)
        lr = lr_after_epoch(lr, mode, e)
    return out


def read_goals(path):
    """{dataset: '%.4f'} of a baseline logfile."""
    with open(path) as f:
        return json.load(f)


def default_args(**over):
    """The flags the PackNet hot path reads, with experiment1's values."""
    a = dict(mode='finetune', dataset='task1', weight_decay=4e-5, cuda=True, log_path=None, progress=False, lr=1e-2,
             checkpoint_format='{save_folder}/checkpoint-{epoch}.pth.tar')
    a.update(over)
    return types.SimpleNamespace(**a)


class TaskRecord(object):
    def __init__(self, flow, dataset):
        self.flow, self.dataset = flow, dataset
        self.train_acc = self.val_acc = None              # the finetune phase's last epoch
        self.baseline_acc = None                          # packnet: validate before the prune (:248)
        self.prune_train_acc = self.prune_val_acc = None
        self.kept = None                                  # packnet: the pruned stage survived the min_train_acc test


class _Net(object):
    """A model with what travels with it between phases: owner masks and shared_layer_info."""

    def __init__(self, net, device):
        self.net = net.to(device)
        self.model = _Plain(self.net)                     # keeps the `module.` prefix of the reference's owner-mask keys
        self.masks = make_masks(self.model)
        self.shared_layer_info = {}

    def snapshot(self):
        return ({k: v.detach().clone() for k, v in self.net.state_dict().items()}, {k: v.clone() for k, v in self.masks.items()},
                copy.deepcopy(self.shared_layer_info))

    def restore(self, snap):
        state, masks, info = snap
        cur = self.net.state_dict()
        with torch.no_grad():
            for k, v in state.items():
                cur[k].copy_(v)
        for k, v in masks.items():
            self.masks[k].copy_(v)
        self.shared_layer_info.clear()
        self.shared_layer_info.update(copy.deepcopy(info))


class BaselineSession(object):
    def __init__(self, arch='vgg16_bn_cifar100', device='cuda', seed=None, sgd_mode='fused', args=None):
        """arch: a factory name of cpg_amd.packnet_models, or a callable (dataset_history=, dataset2num_classes=) -> model with the
        packnet_models.VGG interface.  seed: torch.manual_seed before every model construction (the reference seeds each process, :60).
        sgd_mode: utils.fused_sgd.PackNetSGD's mode."""
        self.factory = getattr(packnet_models, arch) if isinstance(arch, str) else arch
        self.device = torch.device(device)
        self.seed, self.sgd_mode = seed, sgd_mode
        self.args = args or default_args()
        self.models = {}            # dataset -> _Net of the scratch / finetune flows (one model per task)
        self.packnet = None         # the one shared _Net of the packnet flow
        self.records = {}           # dataset -> TaskRecord of the last flow run for it
        self._goals = {}

    # ------------------------------------------------------------------ pieces
    def _fresh(self):
        if self.seed is not None:
            torch.manual_seed(self.seed)
        return _Net(self.factory(dataset_history=[], dataset2num_classes={}), self.device)

    def _start(self, holder, dataset, num_classes):
        holder.net.add_dataset(dataset, num_classes)
        holder.net.classifiers.to(self.device)
        holder.net.set_dataset(dataset)
        holder.shared_layer_info.setdefault(dataset, new_task_info())

    def _manager(self, holder, dataset, mode, train_loader, val_loader):
        args = copy.copy(self.args)
        args.dataset, args.mode = dataset, mode
        return Manager(args, holder.model, holder.shared_layer_info, holder.masks, train_loader, val_loader)

    def make_optimizers(self, holder, mgr, lr):
        """SGD over the trunk and the active head only (packnet_cifar100_main_normal.py:210-233)."""
        active = '.{}.'.format(holder.net.datasets.index(mgr.args.dataset))
        params = [p for n, p in holder.model.named_parameters() if 'classifiers' not in n or active in n]
        opts = Optimizers()
        opts.add(PackNetSGD(params, pruner=mgr.pruner, lr=lr, momentum=0.9, nesterov=True, mode=self.sgd_mode), lr)
        return opts

    def _epochs(self, mgr, opts, mode, epochs):
        lrs = list(opts.lrs)
        tr = va = 0.0
        for epoch in range(epochs):
            tr = mgr.train(opts, epoch, lrs)
            va = mgr.validate(epoch)
            for g in opts[0].param_groups:
                g['lr'] = lr_after_epoch(g['lr'], mode, epoch)
            lrs[0] = opts[0].param_groups[0]['lr']
        return tr, va

    def _finetune(self, holder, dataset, train_loader, val_loader, epochs, lr):
        mgr = self._manager(holder, dataset, 'finetune', train_loader, val_loader)
        mgr.pruner.make_finetuning_mask()
        tr, va = self._epochs(mgr, self.make_optimizers(holder, mgr, lr), 'finetune', epochs)
        mgr.collect_task_layers()                        # (save_checkpoint's stash, :281-282)
        return mgr, tr, va

    # ------------------------------------------------------------------ flows
    def scratch_task(self, dataset, num_classes, train_loader, val_loader, epochs=100, lr=1e-2):
        return self.finetune_task(dataset, num_classes, train_loader, val_loader, epochs, lr, initial_from=None, _flow='scratch')

    def finetune_task(self, dataset, num_classes, train_loader, val_loader, epochs=100, lr=1e-2, initial_from=None, record_goal=None,
                      _flow='finetune'):
        """initial_from: the dataset name of a model of this session, or a state_dict."""
        holder = self._fresh()
        self._start(holder, dataset, num_classes)
        if initial_from is not None:
            src = self.models[initial_from].net.state_dict() if isinstance(initial_from, str) else initial_from
            cur = holder.net.state_dict()
            with torch.no_grad():
                for name, param in src.items():
                    if 'num_batches_tracked' in name:
                        continue
                    cur[name][:].copy_(param)
        rec = TaskRecord(_flow, dataset)
        _, rec.train_acc, rec.val_acc = self._finetune(holder, dataset, train_loader, val_loader, epochs, lr)
        self.models[dataset] = holder
        self.records[dataset] = rec
        if record_goal if record_goal is not None else _flow == 'scratch':
            self._goals[dataset] = '{:.4f}'.format(rec.val_acc)
        return rec

    def packnet_task(self, dataset, num_classes, train_loader, val_loader, epochs=100, lr=1e-2, one_shot_prune_perc=0.6, prune_epochs=30,
                     prune_lr=1e-3, min_train_acc=0.97):
        if self.packnet is None:
            self.packnet = self._fresh()
        holder = self.packnet
        if holder.net.datasets and dataset not in holder.net.datasets and not any(bool((m == 0).any()) for m in holder.masks.values()):
            # (after a task whose pruned stage was not kept; the reference's next run finds no checkpoint and starts from nothing)
            raise RuntimeError('packnet_task(%r): no free slot is left to claim -- the last task (%r) kept every weight; the task would '
                               'train BatchNorm, biases and its head only' % (dataset, holder.net.datasets[-1]))
        self._start(holder, dataset, num_classes)
        rec = TaskRecord('packnet', dataset)
        _, rec.train_acc, rec.val_acc = self._finetune(holder, dataset, train_loader, val_loader, epochs, lr)
        finetuned = holder.snapshot()
        mgr = self._manager(holder, dataset, 'prune', train_loader, val_loader)
        rec.baseline_acc = mgr.validate(-1)
        mgr.one_shot_prune(one_shot_prune_perc)
        rec.prune_train_acc, rec.prune_val_acc = self._epochs(mgr, self.make_optimizers(holder, mgr, prune_lr), 'prune', prune_epochs)
        rec.kept = bool(rec.prune_train_acc > min_train_acc)
        if rec.kept:
            mgr.collect_task_layers()
        else:
            print('Pruning too much!')
            holder.restore(finetuned)
        self.records[dataset] = rec
        return rec

    def evaluate(self, dataset, val_loader):
        """`--mode inference` (:203-206): the task's own BatchNorm / biases attached, apply_mask with its index, validate -- on a copy,
        the live model is not touched.  Returns (accuracy, logits of every batch)."""
        holder = self.models.get(dataset)
        if holder is None:
            holder = self.packnet
        if holder is None or dataset not in holder.net.datasets:
            raise KeyError('no model of this session has learned %r' % (dataset,))
        twin = copy.copy(holder)
        twin.net = copy.deepcopy(holder.net)
        twin.model = _Plain(twin.net)
        twin.masks = {k: v.clone() for k, v in holder.masks.items()}
        twin.net.set_dataset(dataset)
        mgr = self._manager(twin, dataset, 'inference', None, val_loader)
        mgr.attach_task_layers()
        outs = []
        h = twin.model.register_forward_hook(lambda m, i, o: outs.append(o.detach()))
        acc = mgr.validate(0)
        h.remove()
        return acc, outs

    # ------------------------------------------------------------------ the goals hand-off
    def accuracy_goals(self):
        return dict(self._goals)

    def write_logfile(self, path):
        """Merge the goals into the JSON logfile, as successive runs of the reference do (:283-290)."""
        data = read_goals(path) if os.path.isfile(path) else {}
        data.update(self._goals)
        with open(path, 'w') as f:
            json.dump(data, f)
        return data
