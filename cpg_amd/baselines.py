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

packnet_imagenet_main.py (ResNet-50, VGG16-BN at 224x224) and packnet_face_main.py (SphereNet-20) differ from the cifar main in four
places, selected by `policy` ('imagenet' / 'face'; the default for arch resnet50 / resnet101 / resnet152 and spherenet20):

    pretrained first task   `imagenet` resp. `face_verification` is not trained in finetune mode: the free slots are claimed, the
                            pretrained weights are validated and recorded (packnet_face_main.py:303-320, packnet_imagenet_main.py:278-293);
                            the weights come from the caller (`pretrained=`, a state_dict in the names of the checkpoints those mains load)
    face_verification       is scored by Manager.evalLFW over a loader of (a, p, issame) batches, and has no train accuracy
                            (packnet_face_main.py:329-332, utils/packnet_manager.py:55)
    learning rate           finetune: times 0.1 after 10 epochs in a row without a new best validation accuracy, training stops at
                            the end of the first epoch after the third decay; the best epoch is what is kept and recorded
                            (packnet_face_main.py:334-378, packnet_imagenet_main.py:303-347).  prune: times 0.1 after epoch 40 (:380-384)
    keeping a pruned stage  train accuracy above 0.97 AND validation accuracy no more than 0.01 below the task's goal -- the baseline
                            logfile's value (packnet_face_main.py:294-296,386-389).  Read literally the face task can never pass: its
                            train accuracy is 0 / 0.  Here the train-accuracy clause applies to tasks that have one.

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
from .utils.packnet_manager import Manager, has_prelu, make_masks, new_task_info

LR_DROPS = {'finetune': (50, 80), 'prune': (25,)}          # packnet_cifar100_main_normal.py:258-268
# packnet_face_main.py:380-384 = packnet_imagenet_main.py:349-353; their finetune mode follows the validation accuracy (PlateauRule)
PLATEAU_LR_DROPS = {'finetune': (), 'prune': (40,)}
PLATEAU_PATIENCE, PLATEAU_MAX_DECAYS = 10, 3               # packnet_face_main.py:362,369

# what the three mains do differently (module docstring); `pretrained`: the first task that finetune mode records without training
POLICIES = {'cifar': dict(drops=LR_DROPS, plateau=False, pretrained=None, max_val_drop=None),
            'imagenet': dict(drops=PLATEAU_LR_DROPS, plateau=True, pretrained='imagenet', max_val_drop=0.01),
            'face': dict(drops=PLATEAU_LR_DROPS, plateau=True, pretrained='face_verification', max_val_drop=0.01)}
ARCH_POLICY = {'resnet50': 'imagenet', 'resnet101': 'imagenet', 'resnet152': 'imagenet', 'spherenet20': 'face'}


def lr_after_epoch(lr, mode, epoch_idx, drops=LR_DROPS):
    """The learning rate after epoch `epoch_idx` (0-based) has run."""
    return lr * 0.1 if epoch_idx + 1 in drops[mode] else lr


def lr_schedule(lr, mode, epochs, drops=LR_DROPS):
    """The learning rate each of `epochs` epochs trains with."""
    out = []
    for e in range(epochs):
        out.append(lr)
        lr = lr_after_epoch(lr, mode, e, drops)
    return out


class PlateauRule(object):
    """The finetune-mode learning-rate rule of packnet_face_main.py:322-324,334-378 (= packnet_imagenet_main.py:295-347), in its
    order of statements, fed one validation accuracy per epoch."""

    def __init__(self, patience=PLATEAU_PATIENCE, max_decays=PLATEAU_MAX_DECAYS):
        self.patience, self.max_decays = patience, max_decays
        self.best, self.stale, self.decays = 0.0, 0, 0

    def update(self, val_acc):
        """(improved, stop, factor): this epoch is the new best one (the reference replaces its checkpoint and logfile entry, :335-358);
        training ends after this epoch (:362-367, tested BEFORE this epoch's own decay); the learning rate is multiplied by `factor`
        (:369-374)."""
        improved = bool(val_acc > self.best)
        if improved:
            self.stale, self.best = 0, val_acc
        else:
            self.stale += 1
        if self.decays >= self.max_decays:
            return improved, True, 1.0
        if self.stale >= self.patience:
            self.decays += 1
            self.stale = 0
            return improved, False, 0.1
        return improved, False, 1.0


def plateau_schedule(lr, val_accs):
    """The learning rate each epoch trains with under PlateauRule, given the validation accuracies the epochs will reach; shorter than
    `val_accs` when the rule stops the run."""
    rule, out = PlateauRule(), []
    for va in val_accs:
        out.append(lr)
        _, stop, factor = rule.update(va)
        if stop:
            break
        lr = lr * factor
    return out


def keep_pruned_stage(train_acc, val_acc, min_train_acc=0.97, goal=None, max_val_drop=None):
    """The test a pruned stage has to pass to be kept: packnet_cifar100_main_normal.py:297 (train accuracy alone), and with `goal` and
    `max_val_drop` packnet_face_main.py:386-389.  train_acc None / NaN (the face task has none): that clause is skipped."""
    if train_acc is not None and train_acc == train_acc and not train_acc > min_train_acc:
        return False
    return bool(max_val_drop is None or goal is None or (val_acc - goal) >= -max_val_drop)


def map_pretrained(arch_policy, state_dict, first_dataset):
    """{name in the packnet model: tensor} of a pretrained state_dict in the names the mains load: torchvision's resnet50
    (packnet_imagenet_main.py:177-184: everything but `fc`, which becomes the `imagenet` head) or the face weights
    (packnet_face_main.py:196-203: everything but `fc*`; fc5 / fc6 become the embedding layer and AngleLinear of `face_verification`)."""
    out = {k: v for k, v in state_dict.items() if 'fc' not in k}
    if arch_policy == 'imagenet' and first_dataset == 'imagenet':
        out.update({'classifiers.0.weight': state_dict['fc.weight'], 'classifiers.0.bias': state_dict['fc.bias']})
    if arch_policy == 'face' and first_dataset == 'face_verification':
        out.update({'classifiers.0.0.weight': state_dict['fc5.weight'], 'classifiers.0.0.bias': state_dict['fc5.bias'],
                    'classifiers.0.1.weight': state_dict['fc6.weight']})
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
        self.train_acc = self.val_acc = None              # the finetune phase's last epoch (its best one under the plateau rule)
        self.pretrained = False                           # the finetune phase was the pretrained pass-through: no training
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
    def __init__(self, arch='vgg16_bn_cifar100', device='cuda', seed=None, sgd_mode='fused', args=None, policy=None, telemetry=False,
                 stop_on_nonfinite=False):
        """arch: a name cpg_amd.packnet_models.factory knows, or a callable (dataset_history=, dataset2num_classes=) -> model with the
        packnet_models.VGG interface.  seed: torch.manual_seed before every model construction (the reference seeds each process, :60).
        sgd_mode: utils.fused_sgd.PackNetSGD's mode.  policy: a key of POLICIES; default ARCH_POLICY's entry for `arch`, else 'cifar'.
        telemetry / stop_on_nonfinite: OPT-IN, every Manager of this session trains with step telemetry (utils/telemetry.py; needs a
        fused sgd_mode) and, with the second, raises TrainingDiverged out of the flows once a step went non-finite."""
        self.factory = packnet_models.factory(arch) if isinstance(arch, str) else arch
        self.policy_name = policy or (ARCH_POLICY.get(arch, 'cifar') if isinstance(arch, str) else 'cifar')
        self.policy = POLICIES[self.policy_name]
        self.device = torch.device(device)
        self.seed, self.sgd_mode = seed, sgd_mode
        self.args = args or default_args()
        self.telemetry, self.stop_on_nonfinite = bool(telemetry), bool(stop_on_nonfinite)
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
        holder.shared_layer_info.setdefault(dataset, new_task_info(has_prelu(holder.net)))

    def _manager(self, holder, dataset, mode, train_loader, val_loader):
        args = copy.copy(self.args)
        args.dataset, args.mode = dataset, mode
        args.telemetry = self.telemetry or getattr(args, 'telemetry', False)
        args.stop_on_nonfinite = self.stop_on_nonfinite or getattr(args, 'stop_on_nonfinite', False)
        return Manager(args, holder.model, holder.shared_layer_info, holder.masks, train_loader, val_loader)

    def make_optimizers(self, holder, mgr, lr):
        """SGD over the trunk and the active head only (packnet_cifar100_main_normal.py:210-233)."""
        active = '.{}.'.format(holder.net.datasets.index(mgr.args.dataset))
        params = [p for n, p in holder.model.named_parameters() if 'classifiers' not in n or active in n]
        opts = Optimizers()
        opts.add(PackNetSGD(params, pruner=mgr.pruner, lr=lr, momentum=0.9, nesterov=True, mode=self.sgd_mode), lr)
        return opts

    @staticmethod
    def _validate(mgr, epoch):
        """packnet_face_main.py:329-332: LFW pairs for the face task, `validate` for every other."""
        return mgr.evalLFW(epoch) if mgr.args.dataset == 'face_verification' else mgr.validate(epoch)

    def _epochs(self, holder, mgr, opts, mode, epochs):
        """(train accuracy, validation accuracy) of the epoch that is kept: the last one, or under the plateau rule the best one, to
        which the model is put back (the reference keeps that epoch's checkpoint only)."""
        lrs = list(opts.lrs)
        tr = va = 0.0
        rule = PlateauRule() if (mode == 'finetune' and self.policy['plateau']) else None
        best = None
        for epoch in range(epochs):
            tr = mgr.train(opts, epoch, lrs)
            va = self._validate(mgr, epoch)
            if rule is None:
                stop, factor = False, lr_after_epoch(1.0, mode, epoch, self.policy['drops'])
            else:
                improved, stop, factor = rule.update(va)
                if improved:
                    best = (holder.snapshot(), tr, va)
            if stop:
                break
            if factor != 1.0:
                for g in opts[0].param_groups:
                    g['lr'] = g['lr'] * factor
                lrs[0] = opts[0].param_groups[0]['lr']
        if best is not None:
            holder.restore(best[0])
            tr, va = best[1:]
        return tr, va

    def _finetune(self, holder, dataset, train_loader, val_loader, epochs, lr, rec):
        mgr = self._manager(holder, dataset, 'finetune', train_loader, val_loader)
        mgr.pruner.make_finetuning_mask()
        rec.pretrained = dataset == self.policy['pretrained'] and holder.net.datasets.index(dataset) == 0
        if rec.pretrained:
            # the pretrained first task: validated and recorded, not trained (packnet_face_main.py:303-320)
            rec.train_acc, rec.val_acc = None, self._validate(mgr, 0)
        else:
            rec.train_acc, rec.val_acc = self._epochs(holder, mgr, self.make_optimizers(holder, mgr, lr), 'finetune', epochs)
            if dataset == 'face_verification':
                rec.train_acc = None                     # (never accumulated: utils/packnet_manager.py:55)
        mgr.collect_task_layers()                        # (save_checkpoint's stash, :281-282)
        return mgr

    def _load_pretrained(self, holder, dataset, pretrained):
        if pretrained is None:
            return
        cur = holder.net.state_dict()
        with torch.no_grad():
            for name, param in map_pretrained(self.policy_name, pretrained, dataset).items():
                cur[name].copy_(param)

    # ------------------------------------------------------------------ flows
    def scratch_task(self, dataset, num_classes, train_loader, val_loader, epochs=100, lr=1e-2, pretrained=None):
        return self.finetune_task(dataset, num_classes, train_loader, val_loader, epochs, lr, initial_from=None, _flow='scratch',
                                  pretrained=pretrained)

    def finetune_task(self, dataset, num_classes, train_loader, val_loader, epochs=100, lr=1e-2, initial_from=None, record_goal=None,
                      _flow='finetune', pretrained=None):
        """initial_from: the dataset name of a model of this session, or a state_dict.  pretrained: see map_pretrained."""
        holder = self._fresh()
        self._start(holder, dataset, num_classes)
        self._load_pretrained(holder, dataset, pretrained)
        if initial_from is not None:
            src = self.models[initial_from].net.state_dict() if isinstance(initial_from, str) else initial_from
            cur = holder.net.state_dict()
            with torch.no_grad():
                for name, param in src.items():
                    if 'num_batches_tracked' in name:
                        continue
                    cur[name][:].copy_(param)
        rec = TaskRecord(_flow, dataset)
        self._finetune(holder, dataset, train_loader, val_loader, epochs, lr, rec)
        self.models[dataset] = holder
        self.records[dataset] = rec
        if record_goal if record_goal is not None else _flow == 'scratch':
            self._goals[dataset] = '{:.4f}'.format(rec.val_acc)
        return rec

    def packnet_task(self, dataset, num_classes, train_loader, val_loader, epochs=100, lr=1e-2, one_shot_prune_perc=0.6, prune_epochs=30,
                     prune_lr=1e-3, min_train_acc=0.97, goal=None, pretrained=None):
        """goal ('imagenet' / 'face' policies): the accuracy the pruned stage is held against (the mains' --jsonfile entry); default
        this session's recorded goal for the dataset, else the finetuned stage's own validation accuracy."""
        first = self.packnet is None
        if first:
            self.packnet = self._fresh()
        holder = self.packnet
        if holder.net.datasets and dataset not in holder.net.datasets and not any(bool((m == 0).any()) for m in holder.masks.values()):
            # (after a task whose pruned stage was not kept; the reference's next run finds no checkpoint and starts from nothing)
            raise RuntimeError('packnet_task(%r): no free slot is left to claim -- the last task (%r) kept every weight; the task would '
                               'train BatchNorm, biases and its head only' % (dataset, holder.net.datasets[-1]))
        self._start(holder, dataset, num_classes)
        if first:
            self._load_pretrained(holder, dataset, pretrained)
        rec = TaskRecord('packnet', dataset)
        self._finetune(holder, dataset, train_loader, val_loader, epochs, lr, rec)
        finetuned = holder.snapshot()
        mgr = self._manager(holder, dataset, 'prune', train_loader, val_loader)
        if self.policy['max_val_drop'] is None:
            rec.baseline_acc = mgr.validate(-1)          # (:248)
        else:                                            # (read from the goal file instead: packnet_face_main.py:294-297)
            rec.baseline_acc = float(goal if goal is not None else self._goals.get(dataset, rec.val_acc))
        mgr.one_shot_prune(one_shot_prune_perc)
        rec.prune_train_acc, rec.prune_val_acc = self._epochs(holder, mgr, self.make_optimizers(holder, mgr, prune_lr), 'prune', prune_epochs)
        if dataset == 'face_verification':
            rec.prune_train_acc = None
        rec.kept = keep_pruned_stage(rec.prune_train_acc, rec.prune_val_acc, min_train_acc, rec.baseline_acc, self.policy['max_val_drop'])
        if rec.kept:
            mgr.collect_task_layers()
        else:
            print('Pruning too much!')
            holder.restore(finetuned)
        self.records[dataset] = rec
        return rec

    def evaluate(self, dataset, val_loader, flow=None):
        """`--mode inference` (:203-206): the task's own BatchNorm / biases / PReLU slopes attached, apply_mask with its index, validate
        -- on a copy, the live model is not touched.  flow: 'packnet' evaluates the shared PackNet net, 'scratch' the task's own model;
        default: the task's own model where the session has one, else the shared net.  Returns (accuracy, logits of every batch).  `face_verification` is scored over LFW
        pairs and returns (accuracy, [(embeddings a, embeddings p) of every batch]); the mask is applied first here, because
        Manager.evalLFW scores the live weights (the reference's inference mode calls `validate` and cannot score the face head)."""
        holder = self.packnet if flow == 'packnet' else self.models.get(dataset)
        if holder is None and flow is None:
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
        if dataset == 'face_verification':
            mgr.pruner.apply_mask()
            embeddings = mgr.eval_embeddings(0)
            return mgr.score_pairs(embeddings, 0), [(a, p) for a, p, _ in embeddings]
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
