"""Host-side restatement of the PackNet pruner and train step (numpy / torch-CPU), pinned to the fixtures that the reference's own
SparsePruner / Manager produced (tests/golden/packnet_ops.npz, packnet_steps*.npz; generator: tests/golden/make_packnet_golden.py).
It states, independently of cpg_amd, what utils/packnet_prune.py and utils/packnet_manager.py compute; the GPU tests compare the HIP
path with the same fixtures.  Also the small net of packnet_steps, in a stock-torch form (CPU) and on the library's layers (HIP).
"""
import os

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
HEAD_IN = 64
STEP_FILES = ['packnet_steps_%02d' % i for i in range(6)]


def load(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)


def prune_tags(fx):
    return sorted(k[len('prune_'):-len('_status')] for k in fx.files if k.startswith('prune_') and k.endswith('_status'))


# ---------------------------------------------------------------- the pruner (utils/packnet_prune.py)
def rank_prune_zero(w, owner, cur, ratio):
    """_pruning_mask (:22-41) + `weight[mask.eq(0)] = 0.0` (:77, :98).  Returns (status, owner_out, w_out); status 2 is the reference's
    failing kthvalue(0) (k rounds to 0, or exceeds the candidates): nothing is touched."""
    cand = (owner == cur) | (owner == 0)
    k = round(float(ratio) * int(cand.sum()))                   # python round(): half to even (:29)
    if k < 1 or k > int(cand.sum()):
        return 2, owner.copy(), w.copy()
    cutoff = np.sort(np.abs(w[cand]))[k - 1]                     # NaN sorts last, as in kthvalue (:30)
    with np.errstate(invalid='ignore'):
        remove = (np.abs(w) <= cutoff) & (owner == cur)          # (:34) a NaN compares false
    owner_out = owner.copy()
    owner_out[remove] = 0
    w_out = w.copy()
    w_out[owner_out == 0] = 0.0
    return 0, owner_out, w_out


def statistics(first_mask, idx):
    """(sparsity, task ratio, zero ratio) over the FIRST layer's mask only (:101-143)."""
    ge, gt = int((first_mask >= idx).sum()), int((first_mask > idx).sum())
    sparsity = float(gt) / float(ge) if ge != 0 else 0.0
    return sparsity, float((first_mask == idx).sum()) / first_mask.size, float((first_mask == 0).sum()) / first_mask.size


def route(g, w, owner, cur, wd):
    """grad += wd * w; grad[owner != cur] = 0 (:146-159)."""
    out = (torch.from_numpy(g.copy()).add_(torch.from_numpy(w), alpha=float(wd))).numpy()
    out[owner != cur] = 0
    return out


def zero_pruned(w, owner):
    out = w.copy()
    out[owner == 0] = 0.0                                        # (:161-171)
    return out


def apply_mask(w, owner, idx):
    out = w.copy()
    out[(owner == 0) | (owner > idx)] = 0.0                      # (:173-183)
    return out


def claim_free(owner, cur):
    out = owner.copy()
    out[out == 0] = cur + 1                                      # (:185-198)
    return out, cur + 1


# ---------------------------------------------------------------- the small net of packnet_steps
class View(nn.Module):
    def __init__(self, *shape):
        super().__init__()
        self.shape = shape

    def forward(self, x):
        return x.view(*self.shape)


def _trunk(conv, linear):
    return [conv(3, 16, 3, padding=1, bias=False), nn.BatchNorm2d(16), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2),
            conv(16, 32, 3, padding=1, bias=True), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2), nn.MaxPool2d(2, 2),
            View(-1, 512), linear(512, HEAD_IN), nn.ReLU(True), linear(HEAD_IN, HEAD_IN), nn.ReLU(True)]


class CpuNet(nn.Module):
    """Stock torch; `ntasks` heads of 5 classes, head `active` in use."""

    def __init__(self, ntasks, active):
        super().__init__()
        self.features = nn.Sequential(*_trunk(nn.Conv2d, nn.Linear))
        self.classifiers = nn.ModuleList([nn.Linear(HEAD_IN, 5) for _ in range(ntasks)])
        self.active = active

    def forward(self, x):
        return self.classifiers[self.active](self.features(x))


def hip_net(datasets=None, dataset2num_classes=None):
    """The same net on cpg_amd.packnet_models' layers and VGG bookkeeping (GPU tests, BaselineSession factory)."""
    from cpg_amd.models.fused_bn import FusedSequential
    from cpg_amd.packnet_models import vgg as pv
    from cpg_amd.packnet_models.layers import PlainConv2d, PlainLinear

    class Small(pv.VGG):
        head_in = HEAD_IN
    return Small(FusedSequential(*_trunk(PlainConv2d, PlainLinear)), [] if datasets is None else datasets,
                 {} if dataset2num_classes is None else dataset2num_classes)


def covered(net, prefix='module.'):
    """(mask key, module) of every layer the PackNet pruner covers."""
    return [(prefix + n, m) for n, m in net.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear)) and 'classifiers' not in n]


def step_state(fx, which):
    """{state_dict key: tensor} stored `which` ('before' / 'after') the step."""
    pre = which + '_state_'
    return {k[len(pre):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(pre)}


def step_named(fx, prefix):
    """{parameter name without 'module.': tensor} of the arrays stored under `prefix` (before_momentum_, after_grad_, ...)."""
    return {k[len(prefix) + len('module.'):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(prefix)}


def step_masks(fx):
    return {k[len('mask_'):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith('mask_')}


def optimised(net, active):
    """Names and parameters packnet_cifar100_main_normal.py:216-224 hands to SGD: all but the other tasks' heads."""
    return [(n, p) for n, p in net.named_parameters() if 'classifiers' not in n or '.%d.' % active in n]


def cpu_step(fx):
    """One train step of utils/packnet_manager.py:46-69 from the fixture's own state, on stock torch.  Returns a dict shaped like
    the fixture's `after` half."""
    state = step_state(fx, 'before')
    active = int(fx['dataset_index'])
    ntasks = len({k.split('.')[1] for k in state if k.startswith('classifiers.')})
    net = CpuNet(ntasks, active)
    net.load_state_dict(state, strict=True)
    masks = {k[len('module.'):]: v.numpy() for k, v in step_masks(fx).items()}
    cur, lr, wd = int(fx['cur']), float(fx['lr']), 4e-5
    params = optimised(net, active)
    sgd = torch.optim.SGD([p for _, p in params], lr=lr, weight_decay=0.0, momentum=0.9, nesterov=True)
    for n, p in params:
        if n in (mom := step_named(fx, 'before_momentum_')):
            sgd.state[p]['momentum_buffer'] = mom[n].clone()
    net.train()
    sgd.zero_grad()
    logits = net(torch.from_numpy(fx['x']))
    loss = nn.functional.cross_entropy(logits, torch.from_numpy(fx['t']))
    loss.backward()
    with torch.no_grad():
        for key, m in covered(net, ''):
            m.weight.grad.copy_(torch.from_numpy(route(m.weight.grad.numpy(), m.weight.detach().numpy(), masks[key], cur, wd)))
    sgd.step()
    with torch.no_grad():
        for key, m in covered(net, ''):
            m.weight.copy_(torch.from_numpy(zero_pruned(m.weight.numpy(), masks[key])))
    return {'logits': logits.detach(), 'loss': float(loss), 'state': {k: v.detach() for k, v in net.state_dict().items()},
            'grad': {n: p.grad for n, p in net.named_parameters() if p.grad is not None},
            'momentum': {n: sgd.state[p]['momentum_buffer'] for n, p in params}}


def scale_err(got, want):
    """max |got - want| over the scale of `want` (at least 1e-30)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30) if want.size else 0.0


def check_step(got, fx, tol):
    """Compare one replayed step with the fixture: floating tensors within `tol` of each tensor's scale, zero patterns of the routed
    gradients and of the weights exactly.  Every check runs; all misses are reported together.  Returns the worst relative error per
    group of tensors (tests print it)."""
    worst, missed = {}, []

    def need(ok, text):
        if not ok:
            missed.append(text)

    def cmp(tag, a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return need(False, '%s: shape %s vs %s' % (tag, a.shape, b.shape))
        if b.dtype.kind in 'iu':
            return need(np.array_equal(a, b), '%s differs' % tag)
        e = scale_err(a, b)
        worst[tag.split(':')[0]] = max(worst.get(tag.split(':')[0], 0.0), e)
        need(e <= tol, '%s differs by %.3g of its scale (bar %.1g)' % (tag, e, tol))

    cmp('logits', got['logits'].cpu().numpy(), fx['logits'])
    need(abs(got['loss'] - float(fx['loss'])) <= tol * max(1.0, abs(float(fx['loss']))), 'loss %r vs %r' % (got['loss'], float(fx['loss'])))
    want_state, want_grad, want_mom = step_state(fx, 'after'), step_named(fx, 'after_grad_'), step_named(fx, 'after_momentum_')
    masks = {k[len('module.'):]: v.numpy() for k, v in step_masks(fx).items()}
    assert set(got['grad']) == set(want_grad) and set(got['momentum']) == set(want_mom)
    for k, v in want_state.items():
        cmp('state:' + k, got['state'][k].cpu().numpy(), v.numpy())
    for k, v in want_grad.items():
        g = got['grad'][k].cpu().numpy()
        cmp('grad:' + k, g, v.numpy())
        if k[:-len('.weight')] in masks:
            need(np.array_equal(g == 0, v.numpy() == 0), 'zero pattern of the routed gradient of %s' % k)
    for k, v in want_mom.items():
        cmp('momentum:' + k, got['momentum'][k].cpu().numpy(), v.numpy())
    for key, owner in masks.items():
        w = got['state'][key + '.weight'].cpu().numpy()
        need(np.array_equal(w == 0, want_state[key + '.weight'].numpy() == 0), 'zero pattern of %s.weight' % key)
        need(not np.signbit(w[owner == 0]).any() and not w[owner == 0].any(), '%s: weights under owner 0 must be +0.0' % key)
    assert not missed, '; '.join(missed) + ' -- worst per group: %r' % (worst,)
    return worst
