"""The PackNet ResNet-50 and SphereNet-20 on the GPU: that they run the CPG models' kernels (bit identity with the CPG twin holding the
same weights), and that they compute what the reference's PackNet stack computes (tests/golden/packnet_nets_*; generator:
tests/golden/make_packnet_nets_golden.py): eval outputs, the one-shot prune, a train / prune / retrain trajectory inside the band of
the reference's own twin run, evalLFW, the BaselineSession flows of the two mains, and the opt-in fused loss.

Inputs and weights are regenerated from the seeds the fixtures carry (and checked against their crc32): the nets cannot be narrowed.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _verify as V
from _packnet_nets import GOLDEN, build, covered, crc, topology

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
THR = np.arange(0, 4, 0.01)


def load(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)


def batch_x(shape, seed, want_crc=None):
    x = torch.randn(*[int(v) for v in shape], generator=torch.Generator().manual_seed(int(seed)))
    if want_crc is not None:
        assert crc(x) == int(want_crc), 'the seeded input differs from the one the fixture was made with'
    return x


def batch_t(n, classes, seed):
    return torch.randint(0, int(classes), (int(n),), generator=torch.Generator().manual_seed(int(seed)))


def twin_of(arch, net):
    """The CPG model of the same topology at width 1.0 with no piggymask, holding `net`'s tensors."""
    import cpg_amd.models as M
    twin = getattr(M, arch)(dataset_history=[], dataset2num_classes={}, network_width_multiplier=1.0, shared_layer_info={})
    for dataset, n in net.dataset2num_classes.items():
        twin.add_dataset(dataset, n)
    twin.to(DEV)
    twin.load_state_dict({k: v for k, v in net.state_dict().items() if not k.startswith('classifier.')}, strict=True)
    return twin


def _plain(net):
    from cpg_amd.driver import _Plain
    return _Plain(net)


def packnet_manager(net, dataset, train=None, val=None, **over):
    from cpg_amd.baselines import default_args
    from cpg_amd.utils.packnet_manager import Manager, make_masks
    net.set_dataset(dataset)
    model = _plain(net)
    return Manager(default_args(dataset=dataset, **over), model, {}, make_masks(model), train, val)


def cpg_manager(net, dataset, train=None, val=None, **over):
    from cpg_amd.driver import default_args, masked_layers
    from cpg_amd.utils.manager import Manager
    net.set_dataset(dataset)
    model = _plain(net)
    masks = {n: torch.ones(m.weight.shape, dtype=torch.uint8, device=DEV) for n, m in masked_layers(model)}
    return Manager(default_args(dataset=dataset, **over), model, {}, masks, train, val, 0, 1)


# ================================================================ G1: the kernels are the library's
def _train_pass(net, x, t, criterion):
    net.train()
    net.zero_grad(set_to_none=True)
    out = net(x)
    criterion(out, t).backward()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    buffers = {n: b.detach().clone() for n, b in net.named_buffers()}
    return out, grads, buffers


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize('arch,shape', [('resnet50', (4, 3, 64, 64)), ('resnet50', (2, 3, 224, 224)), ('spherenet20', (4, 3, 112, 112))])
def test_twin_identity(arch, shape):
    """One train-mode forward / backward of the PackNet net and of the CPG twin on the same batch: logits, every parameter gradient and
    every BatchNorm buffer are bit-identical -- a layer that fell back to a stock op, or a block that missed its fused form, would
    round differently.  The heads are the same classes in both (nn.Linear / HeadLinear / AngleLinear), so the whole nets are compared."""
    net = build(arch).to(DEV)
    dataset, classes = next(iter(net.dataset2num_classes.items()))
    twin = twin_of(arch, net)
    net.set_dataset(dataset), twin.set_dataset(dataset)
    x, t = batch_x(shape, 7).to(DEV), batch_t(shape[0], classes, 8).to(DEV)
    ce = nn.CrossEntropyLoss()
    out_a, grads_a, buf_a = _train_pass(net, x, t, ce)
    out_b, grads_b, buf_b = _train_pass(twin, x, t, ce)
    assert _same_bits(out_a, out_b), 'logits differ by %g' % float((out_a - out_b).abs().max())
    assert set(grads_a) == set(grads_b) and len(grads_a) == len([p for n, p in net.named_parameters() if 'classifiers' not in n]) + 2
    bad = [n for n in grads_a if not _same_bits(grads_a[n], grads_b[n])]
    assert not bad, '%d gradients differ, first %s' % (len(bad), bad[:4])
    assert set(buf_a) == set(buf_b) and all(_same_bits(buf_a[n], buf_b[n]) for n in buf_a)
    if arch == 'spherenet20':
        # the A-Softmax head in train mode, and the embeddings in eval mode
        from cpg_amd.models.spherenet import AngleLoss
        net.set_dataset('face_verification'), twin.set_dataset('face_verification')
        tf = batch_t(shape[0], net.dataset2num_classes['face_verification'], 9).to(DEV)
        (cos_a, phi_a), grads_a, _ = _train_pass(net, x, tf, AngleLoss())
        (cos_b, phi_b), grads_b, _ = _train_pass(twin, x, tf, AngleLoss())
        assert _same_bits(cos_a, cos_b) and _same_bits(phi_a, phi_b)
        assert set(grads_a) == set(grads_b) and all(_same_bits(grads_a[n], grads_b[n]) for n in grads_a)
        net.eval(), twin.eval()
        with torch.no_grad():
            assert _same_bits(net.forward_to_embeddings(x), twin.forward_to_embeddings(x))


# ================================================================ G2: eval outputs of the reference
@pytest.mark.parametrize('arch', ['resnet50', 'spherenet20'])
def test_eval_outputs_match_the_reference(arch):
    """Eval-mode outputs of seeded batches at 1e-4 of each output's scale (the bar of the first_forward_* fixtures)."""
    fx = load('packnet_nets_topology')
    net = build(arch).to(DEV).eval()
    i = 0
    while '%s/eval%d/shape' % (arch, i) in fx.files:
        pre = '%s/eval%d/' % (arch, i)
        x = batch_x(fx[pre + 'shape'], fx[pre + 'x_seed'], fx[pre + 'x_crc']).to(DEV)
        for dataset in net.datasets:
            net.set_dataset(dataset)
            with torch.no_grad():
                out = net(x)
            got = dict(zip(('cos', 'phi'), out)) if isinstance(out, tuple) else {'logits': out}
            if isinstance(out, tuple):
                with torch.no_grad():
                    got['embeddings'] = net.forward_to_embeddings(x)
            for key, v in got.items():
                want = fx[pre + dataset + '/' + key]
                err = float(np.abs(v.cpu().numpy() - want).max()) / float(np.abs(want).max())
                print('%s%s/%s: %.3g of the scale' % (pre, dataset, key, err))
                assert err <= 1e-4, (pre, dataset, key, err)
        i += 1
    assert i == {'resnet50': 2, 'spherenet20': 1}[arch]


# ================================================================ G3: claim + one-shot prune
@pytest.mark.parametrize('arch', ['resnet50', 'spherenet20'])
def test_one_shot_prune_matches_the_reference(arch):
    """make_finetuning_mask + one_shot_prune(0.6) on the seeded-init weights: the reference's CPU kthvalue and cpg_rank_prune_zero see
    identical bits, so rank, cutoff, released count, owner mask and zeroed weights are exact for every covered layer."""
    fx = load('packnet_nets_prune')
    net = build(arch).to(DEV)
    mgr = packnet_manager(net, topology()[arch]['heads'][0][0])
    mgr.pruner.make_finetuning_mask()
    mgr.one_shot_prune(float(fx[arch + '/ratio']))
    layers = covered(net)
    assert [n for n, _ in layers] == [str(n) for n in fx[arch + '/layers']] and len(layers) == {'resnet50': 53, 'spherenet20': 20}[arch]
    recs = mgr.pruner.last_prune_records
    assert [r['layer'] for r in recs] == [n for n, _ in layers] and all(r['status'] == 0 for r in recs)
    assert [r['k'] for r in recs] == fx[arch + '/k'].tolist()
    assert [r['n_released'] for r in recs] == fx[arch + '/released'].tolist()
    assert np.array_equal(np.array([r['cutoff'] for r in recs], dtype=np.float32), fx[arch + '/cutoff'])
    assert [crc(mgr.pruner.masks[n]) for n, _ in layers] == fx[arch + '/mask_crc'].tolist()
    assert [crc(m.weight.data) for _, m in layers] == fx[arch + '/weight_crc'].tolist()


# ================================================================ G4: the step trajectory
# our distance to the reference's run over the reference's own band, worst quantity and step of the first GPU run with this fixture
# (profiles/packnet.md): 1.271 for ResNet-50 (the loss of the last retrain step), 1.092 for SphereNet-20 (a weight sample after the last
# retrain step); the margin is the next power of two above it
MARGIN = {'resnet50': 2.0, 'spherenet20': 2.0}


@pytest.mark.parametrize('arch', ['resnet50', 'spherenet20'])
def test_step_trajectory_inside_the_reference_band(arch, monkeypatch):
    """The reference Manager's run from the seed -- claim, 3 train steps, validate, one_shot_prune(0.6), 2 retrain steps, validate -- on
    our Manager with the session's PackNetSGD.  Every loss, logit tensor and sampled weight lies within the band the fixture carries
    (the largest distance between the reference's run and its own twins on inputs perturbed by 1e-6) times MARGIN; the statistics, which depend
    on mask counts only, are exact; w[owner == 0] == 0 after every step; what the current task does not own is bit-unchanged by the
    retrain steps."""
    import cpg_amd.utils.packnet_manager as pm_mod
    from cpg_amd.utils import Metric, Optimizers
    from cpg_amd.utils.fused_sgd import PackNetSGD
    fx = load('packnet_nets_steps_' + arch)
    dataset, classes, lr, shape = str(fx['dataset']), int(fx['classes']), float(fx['lr']), fx['shape']
    losses = []

    class Recording(Metric):
        def update(self, val, num):
            if self.name in ('train_loss',):
                losses.append(float(val))
            super().update(val, num)
    monkeypatch.setattr(pm_mod, 'Metric', Recording)
    net = build(arch).to(DEV)
    val = (batch_x(shape, fx['val_x_seed']), batch_t(shape[0], classes, fx['val_t_seed']))
    mgr = packnet_manager(net, dataset, val=[val], lr=lr)
    layers = covered(net)
    assert [n for n, _ in layers] == [str(n) for n in fx['layers']]
    idx = [torch.randperm(m.weight.numel(), generator=torch.Generator().manual_seed(int(fx['idx_seed']) + i))[:int(fx['sample'])]
           for i, (_, m) in enumerate(layers)]
    assert [crc(i) for i in idx] == fx['idx_crc'].tolist()
    idx = [i.to(DEV) for i in idx]
    offs = fx['offsets']
    logits = []
    mgr.model.register_forward_hook(lambda m, i, o: logits.append(o.detach().cpu().numpy()))
    active = '.{}.'.format(net.datasets.index(dataset))
    params = [p for n, p in mgr.model.named_parameters() if 'classifiers' not in n or active in n]
    ratios, missed = {}, []

    def within(tag, got, want, band):
        dist = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())
        ratio = dist / float(band) if band > 0 else (0.0 if dist == 0 else float('inf'))
        key = ':'.join(tag.split(':')[:2])                # (quantity:step)
        ratios[key] = max(ratios.get(key, 0.0), ratio)
        if not ratio <= MARGIN[arch]:
            missed.append('%s: distance %.3g, band %.3g (x%.2f)' % (tag, dist, band, ratio))

    def stats():
        return [mgr.pruner.calculate_sparsity(), mgr.pruner.calculate_curr_task_ratio(), mgr.pruner.calculate_zero_ratio()]

    def free_slots_hold_zero(step):
        bad = [n for n, m in layers if bool((m.weight.data[mgr.pruner.masks[n] == 0].view(torch.int32) != 0).any())]
        assert not bad, 'step %d: weights under owner 0 in %s' % (step, bad[:3])

    def phase(nsteps, first, vi):
        opts = Optimizers()
        opts.add(PackNetSGD(params, pruner=mgr.pruner, lr=lr, momentum=0.9, nesterov=True, mode='fused'), lr)
        for s in range(first, first + nsteps):
            x = batch_x(shape, int(fx['x_seed0']) + s, fx['x_crc'][s])
            mgr.train_loader = [(x, batch_t(shape[0], classes, int(fx['t_seed0']) + s))]
            mgr.train(opts, s, [lr])
            within('loss:%d' % s, losses[-1], fx['loss'][s], fx['band/loss'][s])
            within('logits:%d' % s, logits[-1], fx['logits'][s], fx['band/logits'][s])
            assert stats() == fx['stats'][s].tolist(), (s, stats(), fx['stats'][s])
            free_slots_hold_zero(s)
            want = load('packnet_nets_steps_%s_w%d' % (arch, s))['w']
            got = torch.cat([m.weight.data.reshape(-1)[i] for (_, m), i in zip(layers, idx)]).cpu().numpy()
            if s >= 3:
                # after the prune: over the slots whose owner we and the reference agree on -- a weight next to the cutoff that one run
                # releases and the other keeps differs by its whole value; those slots are counted (owner_moved), as the fixture's band does
                got, want = got * agree, want * agree
            for j, (n, _) in enumerate(layers):
                within('w:%d:%s' % (s, n), got[offs[j]:offs[j + 1]], want[offs[j]:offs[j + 1]], fx['band/w'][s][j])
        mgr.validate(first + nsteps - 1)
        within('val_logits:%d' % vi, logits[-1], fx['val_logits'][vi], fx['band/val_logits'][vi])
        assert stats() == fx['val_stats'][vi].tolist()

    mgr.pruner.make_finetuning_mask()
    phase(3, 0, 0)
    mgr.one_shot_prune(float(fx['ratio']))
    assert stats() == fx['stats_after_prune'].tolist()
    owner = torch.cat([mgr.pruner.masks[n].reshape(-1)[i] for (n, _), i in zip(layers, idx)]).cpu().numpy()
    agree = (owner == fx['owner']).astype(np.float32)
    moved = int((owner != fx['owner']).sum())
    ratios['owner_moved'] = moved / max(int(fx['band/owner_moved']), 1)
    if moved > MARGIN[arch] * int(fx['band/owner_moved']):
        missed.append('owner sample: %d slots on the other side, the reference twin %d' % (moved, int(fx['band/owner_moved'])))
    cur = int(mgr.pruner.current_dataset_idx)
    frozen = {n: m.weight.data[mgr.pruner.masks[n] != cur].clone() for n, m in layers}
    phase(2, 3, 1)
    assert all(_same_bits(m.weight.data[mgr.pruner.masks[n] != cur], frozen[n]) for n, m in layers)
    print('%s: distance over the reference band, worst per quantity and step: %s' % (arch, {k: round(v, 3) for k, v in ratios.items()}))
    assert not missed, '%d outside %gx the band: %s' % (len(missed), MARGIN[arch], '; '.join(missed[:6]))


# ================================================================ G5: evalLFW
def _pair_batches(seed=21, pairs=40, per_batch=8):
    """A PairLoader-shaped iterable: `pairs` pairs at 3x112x112 in batches of (a, p, issame), half of them `same` (the second image is
    the first plus a little noise), half different."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(pairs, 3, 112, 112, generator=g)
    same = torch.arange(pairs) % 2 == 0
    p = torch.where(same.view(-1, 1, 1, 1), a + 0.05 * torch.randn(a.shape, generator=g), torch.randn(a.shape, generator=g))
    assert int(same.sum()) == pairs // 2
    return [(a[i:i + per_batch].to(DEV), p[i:i + per_batch].to(DEV), same[i:i + per_batch]) for i in range(0, pairs, per_batch)]


def _face_net():
    import cpg_amd.packnet_models as pm
    torch.manual_seed(1)
    net = pm.factory('spherenet20')(dataset_history=[], dataset2num_classes={})
    net.add_dataset('face_verification', 10)
    net.set_dataset('face_verification')
    return net.to(DEV)


def test_evalLFW_equals_the_cpg_managers_and_the_restatement():
    loader = _pair_batches()
    net = _face_net()
    mgr = packnet_manager(net, 'face_verification', val=loader)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    acc = mgr.evalLFW(0)
    assert isinstance(acc, np.floating) and 0.0 <= acc <= 1.0 and mgr.last_stats['accuracy'] == float(acc)
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())              # (no apply_mask: utils/packnet_manager.py:109-144)
    embs = mgr.eval_embeddings(0)
    a = np.concatenate([b[0].cpu().numpy() for b in embs])
    p = np.concatenate([b[1].cpu().numpy() for b in embs])
    same = np.concatenate([np.asarray(b[2]).reshape(-1) for b in embs])
    counts, best = V.sweep(V.distance(a, p, 1), same, THR, 10)
    want = V.roc(counts, best)[2]
    assert np.array_equal(mgr.last_lfw['accuracy'], want) and acc == np.mean(want)
    twin = cpg_manager(twin_of('spherenet20', net), 'face_verification', val=loader)
    assert twin.evalLFW(0) == acc and np.array_equal(twin.last_lfw['accuracy'], mgr.last_lfw['accuracy'])


# ================================================================ G6: the sessions of the two mains
def _class_loader(seed, size, classes, batches=2, n=4):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, 3, size, size, generator=g), torch.randint(0, classes, (n,), generator=g)) for _ in range(batches)]


def _shared_net_moved(s, first, keys):
    """The second task really changed the shared net: it owns slots (owner 2) in every covered layer and they hold values, and the live
    per-task tensors named by `keys` are no longer the ones stashed for `first` -- so what `evaluate(first)` reproduces is not trivial."""
    holder = s.packnet
    for name, m in covered(holder.net):
        mine = holder.masks[name] == 2
        assert bool(mine.any()) and bool((m.weight.data[mine] != 0).any()), name
    live = dict(holder.net.named_modules())
    info = holder.shared_layer_info[first]
    for key, attr in keys:
        assert info[key] and any(not torch.equal(getattr(live[n], attr).detach(), t.detach().to(DEV)) for n, t in info[key].items()), key


def test_face_session_pretrained_first_task_then_gender_never_forgets():
    from cpg_amd.baselines import BaselineSession
    s = BaselineSession('spherenet20', device=DEV, seed=1)
    assert s.policy_name == 'face'
    pairs = _pair_batches(seed=22)
    face_train = _class_loader(30, 112, 10)
    # the baseline of the first task: validated and recorded, not trained -- the weights are the seeded initialisation's, bit for bit
    rec = s.scratch_task('face_verification', 10, face_train, pairs, epochs=3)
    assert rec.pretrained and rec.train_acc is None and 0.0 <= rec.val_acc <= 1.0
    fresh = _face_net().state_dict()
    assert all(torch.equal(v, fresh[k]) for k, v in s.models['face_verification'].net.state_dict().items())
    # the PackNet run: the same pass-through, then one-shot prune and one retrain epoch, scored by evalLFW, no train accuracy
    # (goal=0.0: random weights on synthetic pairs -- the stage is held against a goal it reaches; the rule itself: test_keeping_a_pruned_stage)
    rec = s.packnet_task('face_verification', 10, face_train, pairs, epochs=3, one_shot_prune_perc=0.6, prune_epochs=1, prune_lr=1e-4, goal=0.0)
    assert rec.pretrained and rec.train_acc is None and rec.prune_train_acc is None and rec.baseline_acc == 0.0 and rec.kept
    assert 0.0 <= rec.prune_val_acc <= 1.0
    # the shared PackNet net, not the one-task model of scratch_task above
    acc0, emb0 = s.evaluate('face_verification', pairs, flow='packnet')
    gender = (_class_loader(31, 112, 2), _class_loader(32, 112, 2))
    s.scratch_task('gender', 2, gender[0], gender[1], epochs=1, lr=1e-4)
    rec = s.packnet_task('gender', 2, gender[0], gender[1], epochs=1, lr=1e-4, prune_epochs=1, prune_lr=1e-4, min_train_acc=-1.0, goal=0.0)
    assert not rec.pretrained and rec.train_acc is not None and rec.kept
    info = s.packnet.shared_layer_info
    assert len(info['gender']['prelu_layer_weight']) == 20 and len(info['face_verification']['conv_bias']) == 20
    _shared_net_moved(s, 'face_verification', [('conv_bias', 'bias'), ('prelu_layer_weight', 'weight')])
    acc1, emb1 = s.evaluate('face_verification', pairs, flow='packnet')
    assert len(emb0) == len(emb1) == len(pairs)
    assert acc1 == acc0 and all(torch.equal(a0, a1) and torch.equal(p0, p1) for (a0, p0), (a1, p1) in zip(emb0, emb1))
    goals = s.accuracy_goals()
    assert set(goals) == {'face_verification', 'gender'} and all(g == '%.4f' % float(g) for g in goals.values())


def test_imagenet_session_pretrained_first_task_then_a_second_never_forgets():
    from cpg_amd.baselines import BaselineSession
    s = BaselineSession('resnet50', device=DEV, seed=1)
    assert s.policy_name == 'imagenet'
    first = (_class_loader(40, 64, 10), _class_loader(41, 64, 10))
    rec = s.scratch_task('imagenet', 10, first[0], first[1], epochs=3)
    assert rec.pretrained and rec.train_acc is None
    torch.manual_seed(1)
    import cpg_amd.packnet_models as pm
    fresh = pm.factory('resnet50')(dataset_history=[], dataset2num_classes={})
    fresh.add_dataset('imagenet', 10)
    got = s.models['imagenet'].net.state_dict()
    assert all(torch.equal(got[k].cpu(), v) for k, v in fresh.state_dict().items())
    rec = s.packnet_task('imagenet', 10, first[0], first[1], epochs=3, prune_epochs=1, prune_lr=1e-4, min_train_acc=-1.0, goal=0.0)
    assert rec.pretrained and rec.kept and rec.prune_train_acc is not None
    acc0, out0 = s.evaluate('imagenet', first[1], flow='packnet')
    second = (_class_loader(42, 64, 5), _class_loader(43, 64, 5))
    s.scratch_task('flowers', 5, second[0], second[1], epochs=1, lr=1e-4)
    rec = s.packnet_task('flowers', 5, second[0], second[1], epochs=1, lr=1e-4, prune_epochs=1, prune_lr=1e-4, min_train_acc=-1.0, goal=0.0)
    assert not rec.pretrained and rec.kept
    assert len(s.packnet.shared_layer_info['flowers']['bn_layer_running_mean']) == 53
    _shared_net_moved(s, 'imagenet', [('bn_layer_weight', 'weight'), ('bn_layer_bias', 'bias'), ('bn_layer_running_mean', 'running_mean'),
                                      ('bn_layer_running_var', 'running_var')])
    acc1, out1 = s.evaluate('imagenet', first[1], flow='packnet')
    assert len(out0) == len(out1) == len(first[1])
    assert acc1 == acc0 and all(torch.equal(a, b) for a, b in zip(out0, out1))
    goals = s.accuracy_goals()
    assert set(goals) == {'imagenet', 'flowers'} and all(g == '%.4f' % float(g) for g in goals.values())


# ================================================================ G7: the opt-in fused loss
@pytest.mark.parametrize('arch,dataset,classes,shape', [('spherenet20', 'face_verification', 10, (4, 3, 112, 112)),
                                                       ('resnet50', 't1', 5, (4, 3, 64, 64))])
def test_fused_loss_step_equals_the_cpg_managers(arch, dataset, classes, shape, monkeypatch):
    """args.fused_loss: the first train step's loss and the gradients `backward` leaves (taken before the pruner routes them) equal those
    of utils.manager.Manager's fused-loss step on the CPG twin, bit for bit."""
    import cpg_amd.utils.manager as cm_mod
    import cpg_amd.utils.packnet_manager as pm_mod
    from cpg_amd.models.losses import FusedAngleLoss, FusedCrossEntropyLoss
    from cpg_amd.utils import Metric, Optimizers
    seen = {}

    class Recording(Metric):
        def update(self, val, num):
            seen.setdefault(self.name, []).append(val.detach().clone() if isinstance(val, torch.Tensor) else val)
            super().update(val, num)
    monkeypatch.setattr(pm_mod, 'Metric', Recording)
    monkeypatch.setattr(cm_mod, 'Metric', Recording)
    net = build(arch).to(DEV)
    twin = twin_of(arch, net)
    batch = [(batch_x(shape, 7), batch_t(shape[0], classes, 8))]
    results = []
    for which, mgr in (('packnet', packnet_manager(net, dataset, train=batch, fused_loss=True)),
                       ('cpg', cpg_manager(twin, dataset, train=batch, fused_loss=True))):
        assert isinstance(mgr.criterion, FusedAngleLoss if dataset == 'face_verification' else FusedCrossEntropyLoss)
        grads = {}
        route = mgr.pruner.do_weight_decay_and_make_grads_zero

        def snapshot_then_route(mgr=mgr, grads=grads, route=route):
            grads.update({n: p.grad.detach().clone() for n, p in mgr._root().named_parameters() if p.grad is not None})
            route()
        monkeypatch.setattr(mgr.pruner, 'do_weight_decay_and_make_grads_zero', snapshot_then_route)
        opts = Optimizers()
        opts.add(torch.optim.SGD(list(mgr.model.parameters()), lr=1e-4, momentum=0.9, nesterov=True), 1e-4)
        seen.clear()
        if which == 'packnet':
            mgr.pruner.make_finetuning_mask()
            mgr.train(opts, 0, [1e-4])
        else:
            mgr.train(opts, 0, [1e-4], 0)
        results.append((seen['train_loss'][0], grads, seen.get('train_accuracy')))
    (loss_a, grads_a, acc_a), (loss_b, grads_b, acc_b) = results
    assert _same_bits(loss_a.reshape(1), loss_b.reshape(1))
    assert set(grads_a) == set(grads_b) and len(grads_a) > 20
    bad = [n for n in grads_a if not _same_bits(grads_a[n], grads_b[n])]
    assert not bad, '%d gradients differ, first %s' % (len(bad), bad[:4])
    assert (acc_a is None) == (acc_b is None) == (dataset == 'face_verification')
    if acc_a is not None:
        assert torch.equal(acc_a[0], acc_b[0])
    # off by default: the stock criterion
    assert type(packnet_manager(net, dataset).criterion).__name__ in ('AngleLoss', 'CrossEntropyLoss')
