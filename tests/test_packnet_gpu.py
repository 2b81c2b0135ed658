"""PackNet baseline stack on the GPU: the two new entry points against the compositions they replace (bit for bit), the HIP path
against the reference's fixtures (tests/golden/packnet_*; tolerances: 1e-4 of each tensor's scale, the project's bar for contractions
on identical inputs), and the BaselineSession flows on the small net of the fixtures with synthetic loaders."""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import _packnet as pk

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lib():
    from cpg_amd import _lib as L
    return L


def _u8(t):
    return _lib().dptr(t, torch.uint8, 'mask')


# ================================================================ raw ABI: the fused step
SIZES = [0, 1, 3, 4, 5, 4096, 4097, 8191, 1 << 20, 1300001]


@pytest.fixture(scope='module')
def ragged():
    """70 ragged layers cut out of flat buffers: 16-byte aligned starts, except every seventh layer (one element off: the scalar path)."""
    rng = np.random.RandomState(5)
    sizes = SIZES + [int(v) for v in rng.randint(1, 20000, size=60)]
    offs, at = [], 0
    for i, n in enumerate(sizes):
        at = (at + 15) // 16 * 16 + (1 if i % 7 == 6 else 0)      # in elements: multiples of 16 keep fp32 AND uint8 storage aligned
        offs.append(at)
        at += n
    g = torch.Generator().manual_seed(6)
    total = at + 16
    w = torch.randn(total, generator=g)
    gw = torch.randn(total, generator=g)
    buf = torch.randn(total, generator=g)
    owner = torch.randint(0, 4, (total,), generator=g, dtype=torch.uint8)
    w[::97] = -0.0                                                # a negative zero under every owner id: pinned slots must read +0.0
    return sizes, offs, (w.to(DEV), gw.to(DEV), buf.to(DEV), owner.to(DEV))


def _views(flat, sizes, offs):
    return [flat[o:o + n] for n, o in zip(sizes, offs)]


def _rows(L, ws, gs, bs, os_):
    rows = [(w.data_ptr() if w.numel() else None, g.data_ptr() if w.numel() else None, b.data_ptr() if w.numel() else None,
             o.data_ptr() if w.numel() else None, w.numel()) for w, g, b, o in zip(ws, gs, bs, os_)]
    return (L.SgdItem * len(rows))(*rows), len(rows)


@pytest.mark.parametrize('cur', [2, 5])
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('nesterov', [0, 1])
def test_route_zero_step_bit_equals_step_then_zero(ragged, cur, first, nesterov):
    """cpg_sgd_route_zero_step == cpg_sgd_route_step + cpg_zero_pruned in w, gw and buf, per layer and in the multi form; cur = 5 owns
    nothing."""
    L = _lib()
    sizes, offs, flats = ragged
    s = L.stream_ptr()
    hyper = (cur, 4e-5, 1e-2, 0.9, nesterov, first)
    outs = []
    for arm in ('step+zero', 'fused', 'fused_multi'):
        w, gw, buf, owner = (t.clone() for t in flats)
        ws, gs, bs, os_ = (_views(t, sizes, offs) for t in (w, gw, buf, owner))
        assert all((x.data_ptr() % 16 == 0) == (i % 7 != 6) for i, x in enumerate(ws))
        if arm == 'fused_multi':
            items, n = _rows(L, ws, gs, bs, os_)
            L.call('cpg_sgd_route_zero_step_multi', items, n, *hyper, s)
        else:
            for a, b, c, d in zip(ws, gs, bs, os_):
                n = a.numel()
                p = [ctypes.c_void_p(x.data_ptr()) if n else None for x in (a, b, c, d)]
                if arm == 'fused':
                    L.call('cpg_sgd_route_zero_step', *p, *hyper, n, s)
                else:
                    L.call('cpg_sgd_route_step', *p, *hyper, n, s)
                    L.call('cpg_zero_pruned', p[0], p[3], n, s)
        outs.append((w.cpu().numpy(), gw.cpu().numpy(), buf.cpu().numpy()))
        assert torch.equal(owner, flats[3])
    for name, other in zip(('per layer', 'multi'), outs[1:]):
        for what, a, b in zip(('w', 'gw', 'buf'), outs[0], other):
            assert a.tobytes() == b.tobytes(), '%s: %s differs from step + zero in %d elements' % (name, what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    # pinned slots: +0.0 with the sign bit clear, inside the layers; nothing written between them
    w_out, owner = outs[1][0], flats[3].cpu().numpy()
    inside = np.zeros(w_out.size, dtype=bool)
    for n, o in zip(sizes, offs):
        inside[o:o + n] = True
    assert not w_out.view(np.uint32)[inside & (owner == 0)].any()
    w_in = flats[0].cpu().numpy()
    assert w_out[~inside].tobytes() == w_in[~inside].tobytes()
    if first:      # another task's slot: g = 0 and no momentum yet, so the step is exactly 0
        frozen = inside & (owner != 0) & (owner != cur)
        assert w_out[frozen].tobytes() == w_in[frozen].tobytes()


@pytest.mark.parametrize('entry', ['cpg_sgd_route_zero_step_multi', 'cpg_sgd_route_step_multi', 'cpg_adam_route_step_multi'])
def test_route_zero_step_multi_rejects_a_bad_table_before_any_launch(ragged, entry):
    """All three multi-tensor entry points check every row before their first launch: a null pointer in the last of 69 rows, past the
    first launch's 48, returns CPG_E_INVALID and leaves every tensor bytewise as it was.  (Adam's two moments: buf and |buf|.)"""
    L = _lib()
    sizes, offs, flats = ragged
    adam = entry == 'cpg_adam_route_step_multi'
    before = list(flats[:3]) + ([flats[2].abs()] if adam else [])
    tensors = [t.clone() for t in before]
    views = [_views(t, sizes, offs) for t in tensors + [flats[3]]]
    rows = [tuple(v.data_ptr() for v in row) + (row[0].numel(),) for row in zip(*views) if row[0].numel()]
    rows[-1] = (rows[-1][0], None) + rows[-1][2:]                                  # the 69th row: after the first launch's worth of layers
    assert len(rows) > L.lib().cpg_multi_tensor_max()
    items = (L.AdamItem if adam else L.SgdItem) * len(rows)
    hyper = (2, L.MODE_FINETUNE, 5e-4, 0.9, 0.999, 1e-8, 3) if adam else (2, 4e-5, 1e-2, 0.9, 1, 0)
    with pytest.raises(L.CpgHipError) as e:
        L.call(entry, items(*rows), len(rows), *hyper, L.stream_ptr())
    assert e.value.code == L.CPG_E_INVALID
    with pytest.raises(L.CpgHipError):
        L.call('cpg_sgd_route_zero_step', None, None, None, None, 2, 4e-5, 1e-2, 0.9, 1, 0, 8, L.stream_ptr())
    torch.cuda.synchronize()
    assert all(torch.equal(t, t0) for t, t0 in zip(tensors, before))


# ================================================================ raw ABI: the zeroing prune
def _rank_prune(L, entry, w, owner, cur, ratio):
    res = torch.zeros(L.PRUNE_RESULT_BYTES // 8, dtype=torch.int64, device=DEV)
    ws, nbytes = L.workspace(L.lib().cpg_rank_prune_workspace_bytes(), DEV)
    L.call(entry, L.dptr(w), _u8(owner), cur, ratio, w.numel(), ctypes.c_void_p(res.data_ptr()), L.dptr(ws), nbytes, L.stream_ptr())
    return L.PruneResult.from_buffer_copy(res.cpu().numpy().tobytes())


def test_rank_prune_zero_equals_composition_and_reference():
    L = _lib()
    ops = pk.load('packnet_ops')
    tags = pk.prune_tags(ops)
    assert len(tags) >= 10
    for tag in tags:
        g = lambda k: ops['prune_%s_%s' % (tag, k)]      # noqa: E731
        cur, ratio = int(g('cur')), float(g('ratio'))
        w0, o0 = torch.from_numpy(g('w')).to(DEV), torch.from_numpy(g('owner')).to(DEV)
        w1, o1 = w0.clone(), o0.clone()
        r1 = _rank_prune(L, 'cpg_rank_prune_zero', w1, o1, cur, ratio)
        w2, o2 = w0.clone(), o0.clone()
        r2 = _rank_prune(L, 'cpg_rank_prune', w2, o2, cur, ratio)
        if r2.status == L.CPG_OK:
            L.call('cpg_zero_pruned', L.dptr(w2), _u8(o2), w2.numel(), L.stream_ptr())
        assert (r1.status, r1.k, r1.n_candidates, r1.n_released) == (r2.status, r2.k, r2.n_candidates, r2.n_released), tag
        assert r1.status == int(g('status')), tag
        assert torch.equal(o1, o2) and w1.cpu().numpy().tobytes() == w2.cpu().numpy().tobytes(), tag
        assert int((o1.cpu().numpy() != g('owner_out')).sum()) == 0, tag
        assert w1.cpu().numpy().tobytes() == g('w_out').tobytes(), '%s: weights differ from the reference' % tag
        if r1.status == L.CPG_E_KRANGE:
            assert torch.equal(o1, o0) and w1.cpu().numpy().tobytes() == w0.cpu().numpy().tobytes(), tag
    assert int(ops['prune_k_zero_status']) == L.CPG_E_KRANGE


def test_pruner_methods_reproduce_the_reference_ops():
    """utils.packnet_prune.SparsePruner on the crafted cases of packnet_ops.npz: statistics equal as floats, masks and zero patterns exact,
    SystemExit(2) where the reference's kthvalue(0) fails."""
    from cpg_amd.utils.packnet_prune import SparsePruner
    ops = pk.load('packnet_ops')

    class Flat(nn.Module):
        def __init__(self, weights):
            super().__init__()
            for i, w in enumerate(weights):
                w = torch.from_numpy(np.ascontiguousarray(w))
                lin = nn.Linear(w.numel(), 1, bias=False)
                lin.weight.data = w.reshape(1, -1).clone()
                setattr(self, 'l%d' % i, lin)
            self.classifiers = nn.ModuleList([nn.Linear(3, 2)])

    def pruner(weights, owners, cur, idx):
        model = Flat(weights).to(DEV)
        masks = {'l%d' % i: torch.from_numpy(o).reshape(1, -1).clone() for i, o in enumerate(owners)}      # on the host: moved lazily
        p = SparsePruner(model, masks, types.SimpleNamespace(weight_decay=float(ops['route_wd'])), None, None, idx)
        p.current_dataset_idx = cur
        return model, p

    for tag in sorted(k[len('stats_'):-len('_values')] for k in ops.files if k.startswith('stats_') and k.endswith('_values')):
        a, b = ops['stats_%s_first' % tag], ops['stats_%s_second' % tag]
        _, p = pruner([np.zeros(a.size, np.float32), np.zeros(b.size, np.float32)], [a, b], 3, int(ops['stats_%s_idx' % tag]))
        got = [p.calculate_sparsity(), p.calculate_curr_task_ratio(), p.calculate_zero_ratio()]
        assert got == list(ops['stats_%s_values' % tag]), tag
    w, owner = ops['route_w'], ops['route_owner']
    _, p = pruner([np.zeros(8, np.float32)], [np.array([0, 1, 2, 3, 3, 1, 0, 2], dtype=np.uint8)], 0, 1)
    assert SparsePruner(p.model, p.masks, p.args, None, None, 1).current_dataset_idx == int(ops['init_cur_from_first_mask']) == 3
    model, p = pruner([w], [owner], int(ops['route_cur']), 2)
    model.l0.weight.grad = torch.from_numpy(ops['route_g']).reshape(1, -1).to(DEV)
    p.do_weight_decay_and_make_grads_zero()
    got = model.l0.weight.grad.cpu().numpy().reshape(-1)
    assert np.array_equal(got == 0, ops['route_g_out'] == 0) and pk.scale_err(got, ops['route_g_out']) <= 1e-6
    p.make_pruned_zero()
    assert model.l0.weight.data.cpu().numpy().tobytes() == ops['zero_w_out'].tobytes()
    for idx in (1, 2, 3):
        model, p = pruner([w], [owner], 3, idx)
        p.apply_mask()
        assert model.l0.weight.data.cpu().numpy().tobytes() == ops['apply_idx%d_w_out' % idx].tobytes()
    model, p = pruner([w], [owner], 3, 3)
    p.make_finetuning_mask()
    assert np.array_equal(p.masks['l0'].cpu().numpy().reshape(-1), ops['claim_owner_out']) and p.current_dataset_idx == int(ops['claim_cur_out'])
    model, p = pruner([ops['prune_mixed_w']], [ops['prune_mixed_owner']], int(ops['prune_mixed_cur']), 2)
    assert p.calculate_zero_ratio() == float((ops['prune_mixed_owner'] == 0).mean())
    p.one_shot_prune(float(ops['prune_mixed_ratio']))
    assert np.array_equal(p.masks['l0'].cpu().numpy().reshape(-1), ops['prune_mixed_owner_out'])
    assert model.l0.weight.data.cpu().numpy().tobytes() == ops['prune_mixed_w_out'].tobytes()
    assert p.calculate_zero_ratio() == float((ops['prune_mixed_owner_out'] == 0).mean())       # the cached histogram was dropped
    model, p = pruner([ops['prune_k_zero_w']], [ops['prune_k_zero_owner']], 1, 1)
    with pytest.raises(SystemExit) as e:
        p.one_shot_prune(float(ops['prune_k_zero_ratio']))
    assert e.value.code == 2


# ================================================================ against the reference: stored steps
class _Recording(object):
    """Optimizers that notes the gradients of the parameters torch's own SGD path steps, right before it does: torch's foreach Nesterov
    update overwrites those .grad tensors in place (the routed gradients of the covered weights are left as the reference leaves them)."""

    def __init__(self, opt, named):
        self.opt, self.named, self.grads = opt, named, {}

    def zero_grad(self):
        self.opt.zero_grad()

    def step(self):
        self.grads = {n: p.grad.detach().clone() for n, p in self.named if p.grad is not None}
        self.opt.step()


def _hip_step(fx, mode='fused'):
    from cpg_amd.utils.fused_sgd import PackNetSGD
    from cpg_amd.utils.packnet_manager import Manager
    state = pk.step_state(fx, 'before')
    active = int(fx['dataset_index'])
    ntasks = len({k.split('.')[1] for k in state if k.startswith('classifiers.')})
    names = ['t%d' % (i + 1) for i in range(ntasks)]
    net = pk.hip_net(list(names), {n: 5 for n in names})
    net.set_dataset(names[active])
    _load(net, state)
    net.to(DEV)
    model = pk_wrap(net)
    masks = {k: v.clone() for k, v in pk.step_masks(fx).items()}
    args = types.SimpleNamespace(dataset=names[active], cuda=True, weight_decay=4e-5, progress=False, mode='finetune')
    mgr = Manager(args, model, {}, masks, [(torch.from_numpy(fx['x']), torch.from_numpy(fx['t']))], None)
    assert mgr.pruner.current_dataset_idx == int(fx['cur'])
    params = pk.optimised(net, active)
    sgd = PackNetSGD([p for _, p in params], pruner=mgr.pruner, lr=float(fx['lr']), momentum=0.9, nesterov=True, mode=mode)
    mom = pk.step_named(fx, 'before_momentum_')
    for n, p in params:
        if n in mom:
            sgd.state[p]['momentum_buffer'] = mom[n].to(DEV)
    covered = {id(m.weight) for _, m in pk.covered(net)}
    opts = _Recording(sgd, params)
    logits = []
    model.register_forward_hook(lambda m, i, o: logits.append(o.detach()))
    crit, losses = mgr.criterion, []
    mgr.criterion = lambda o, t: (lambda l: (losses.append(l.detach()), l)[1])(crit(o, t))
    mgr.train(opts, 0, [float(fx['lr'])])
    grads = dict(opts.grads)
    if mode != 'unfused':      # (unfused: torch's SGD steps the covered weights too, and its foreach update reuses their .grad)
        grads.update({n: p.grad for n, p in params if id(p) in covered})
    return {'logits': logits[-1], 'loss': float(losses[-1]), 'state': {k: v.detach() for k, v in net.state_dict().items()},
            'grad': grads, 'momentum': {n: sgd.state[p]['momentum_buffer'] for n, p in params}}, mgr


def _load(net, state):
    """The stored state_dict (the fixture leaves out the `classifier.*` alias of the active head: same tensors as classifiers.i)."""
    r = net.load_state_dict(state, strict=False)
    assert not r.unexpected_keys and all(k.startswith('classifier.') for k in r.missing_keys), r


def pk_wrap(net):
    from cpg_amd.driver import _Plain
    return _Plain(net)


@pytest.mark.parametrize('name', pk.STEP_FILES)
def test_stored_step_matches_the_reference(name):
    fx = pk.load(name)
    got, _ = _hip_step(fx)
    print(name, pk.check_step(got, fx, 1e-4))


def test_unfused_composition_matches_the_reference_step():
    fx = pk.load(pk.STEP_FILES[4])               # task 2, second finetune step: momentum, three owner ids
    got, _ = _hip_step(fx, mode='unfused')
    print(pk.check_step(got, fx, 1e-4))
    got, _ = _hip_step(fx, mode='step+zero')
    print(pk.check_step(got, fx, 1e-4))


@pytest.mark.parametrize('after_step,tag', [(1, 't1_prune'), (4, 't2_prune')])
def test_one_shot_prune_masks_equal_the_reference(after_step, tag):
    """The reference prunes the weights its last finetune step left (its validate in between zeroes nothing: no owner is 0 or above the
    task): from the stored state after that step, one_shot_prune(0.6) must give its owner masks byte for byte."""
    from cpg_amd.utils.packnet_manager import Manager
    fx, index = pk.load(pk.STEP_FILES[after_step]), pk.load('packnet_steps')
    state = pk.step_state(fx, 'after')
    ntasks = len({k.split('.')[1] for k in state if k.startswith('classifiers.')})
    names = ['t%d' % (i + 1) for i in range(ntasks)]
    net = pk.hip_net(list(names), {n: 5 for n in names})
    net.set_dataset(names[-1])
    _load(net, state)
    net.to(DEV)
    masks = {k: v.clone() for k, v in pk.step_masks(fx).items()}
    mgr = Manager(types.SimpleNamespace(dataset=names[-1], cuda=True, weight_decay=4e-5, progress=False, mode='prune'), pk_wrap(net), {}, masks,
                  None, [(torch.from_numpy(index[tag + '_val0_x']), torch.from_numpy(index[tag + '_val0_t']))])
    logits = []
    mgr.model.register_forward_hook(lambda m, i, o: logits.append(o.detach()))
    mgr.validate(-1)
    assert pk.scale_err(logits[-1].cpu().numpy(), index[tag + '_val0_logits']) <= 1e-4
    mgr.one_shot_prune(0.6)
    for key, m in pk.covered(net):
        want = index['%s_pruned_%s' % (tag, key)]
        assert int((mgr.pruner.masks[key].cpu().numpy() != want).sum()) == 0, key
        w = m.weight.data.cpu().numpy()
        assert not w.view(np.uint32)[want == 0].any(), key
    assert mgr.pruner.calculate_sparsity() == float(index[tag + '_sparsity_after_prune']) == 0.0
    assert mgr.pruner.calculate_zero_ratio() == float(index[tag + '_zero_ratio_after_prune'])


# ================================================================ PackNetSGD against the unfused composition
@pytest.mark.parametrize('nesterov', [True, False])
def test_packnet_sgd_equals_routing_then_torch_sgd_then_zeroing(nesterov, libopt):
    """4 steps on two copies of the small net, as test_masked_sgd_equals_routing_then_torch_sgd: direct conv kernels (the test is about
    the optimizer arithmetic), the same 2e-6 band; weights under owner 0 are +0.0 after every step in both."""
    from cpg_amd.utils.fused_sgd import PackNetSGD
    from cpg_amd.utils.packnet_prune import SparsePruner
    libopt.set('CPG_NO_WINO', '1')
    nets, pruners, opts = [], [], []
    for mode in ('unfused', 'fused'):
        torch.manual_seed(3)
        net = pk.hip_net()
        net.add_dataset('t1', 5)
        net.set_dataset('t1')
        model = pk_wrap(net.to(DEV))
        g = torch.Generator().manual_seed(11)
        masks = {n: torch.randint(0, 4, m.weight.shape, generator=g, dtype=torch.uint8).to(DEV) for n, m in pk.covered(net)}
        pruner = SparsePruner(model, masks, types.SimpleNamespace(weight_decay=4e-5), None, None, 2)
        pruner.current_dataset_idx = 2
        opt = PackNetSGD(model.parameters(), pruner=pruner, lr=1e-2, momentum=0.9, nesterov=nesterov, mode=mode)
        assert pruner.fused_weight_step == (mode == 'fused')
        nets.append(model); pruners.append(pruner); opts.append(opt)      # noqa: E702
    g = torch.Generator().manual_seed(12)
    for step in range(4):
        x = torch.randn(8, 3, 32, 32, generator=g).to(DEV)
        t = torch.randint(0, 5, (8,), generator=g).to(DEV)
        for model, pruner, opt in zip(nets, pruners, opts):
            model.train()
            opt.zero_grad()
            nn.functional.cross_entropy(model(x), t).backward()
            pruner.do_weight_decay_and_make_grads_zero()
            opt.step()
            pruner.make_pruned_zero()
            for key, m in pk.covered(model.module):
                w = m.weight.data.cpu().numpy()
                assert not w.view(np.uint32)[pruner.masks[key].cpu().numpy() == 0].any(), '%s step %d' % (key, step)
        for (n, p), (_, q) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
            sc = float(p.abs().max()) + 1e-12
            np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().cpu().numpy(), rtol=0, atol=2e-6 * sc, err_msg='%s step %d' % (n, step))
    covered = {id(m.weight) for model in nets for _, m in pk.covered(model.module)}
    for (n, p), (_, q) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        b0, b1 = opts[0].state[p]['momentum_buffer'], opts[1].state[q]['momentum_buffer']
        np.testing.assert_allclose(b1.cpu().numpy(), b0.cpu().numpy(), rtol=2e-3, atol=1e-5 * (float(b0.abs().max()) + 1e-20), err_msg=n)
        if id(q) in covered:      # the fused pass leaves the routed gradient: zero exactly where the current task does not own the slot
            key = 'module.' + n[len('module.'):-len('.weight')]
            assert not q.grad[pruners[1].masks[key] != 2].any()


# ================================================================ models and checkpoints against the reference
def test_vgg16_bn_cifar100_eval_logits_match_the_reference():
    import cpg_amd.packnet_models as pm
    fx = pk.load('packnet_topology')
    torch.manual_seed(1)
    net = pm.vgg16_bn_cifar100(pretrained=False, dataset_history=[], dataset2num_classes={})
    net.add_dataset('t1', 5)
    net.set_dataset('t1')
    net.to(DEV).eval()
    with torch.no_grad():
        out = net(torch.from_numpy(fx['x']).to(DEV))
    e = pk.scale_err(out.cpu().numpy(), fx['logits'])
    print('eval logits: %.3g of scale' % e)
    assert e <= 1e-4


def test_reference_checkpoint_serves_both_tasks():
    from cpg_amd.utils.packnet_manager import Manager
    index = pk.load('packnet_steps')
    ck = torch.load(os.path.join(pk.GOLDEN, 'packnet_checkpoint-1.pth.tar'), map_location='cpu', weights_only=False)
    fmt = '{save_folder}/packnet_checkpoint-{epoch}.pth.tar'
    for d in ('t1', 't2'):
        net = pk.hip_net(list(ck['dataset_history']), dict(ck['dataset2num_classes']))
        net.set_dataset(d)
        net.to(DEV)
        model = pk_wrap(net)
        val = [(torch.from_numpy(index['infer_%s_x' % d]), torch.from_numpy(index['infer_%s_t' % d]))]
        args = types.SimpleNamespace(dataset=d, cuda=True, weight_decay=4e-5, progress=False, mode='inference', checkpoint_format=fmt)
        mgr = Manager(args, model, copy.deepcopy(ck['shared_layer_info']), {k: v.clone() for k, v in ck['masks'].items()}, None, val)
        assert mgr.pruner.current_dataset_idx == 2
        mgr.load_checkpoint_for_inference(1, pk.GOLDEN)
        logits = []
        model.register_forward_hook(lambda m, i, o: logits.append(o.detach()))
        acc = mgr.validate(0)
        e = pk.scale_err(logits[-1].cpu().numpy(), index['infer_%s_logits' % d])
        print(d, 'logits: %.3g of scale' % e)
        assert e <= 1e-4 and abs(acc - float(index['infer_%s_acc' % d])) < 1e-6
        got = [mgr.pruner.calculate_sparsity(), mgr.pruner.calculate_curr_task_ratio(), mgr.pruner.calculate_zero_ratio()]
        assert got == list(index['infer_%s_stats' % d])
        # a checkpoint written here has the reference's key sets
        mine = mgr.checkpoint_dict()
        assert set(mine) == set(ck)
        assert sorted(mine['model_state_dict']) == sorted(ck['model_state_dict']) and set(mine['masks']) == set(ck['masks'])
        assert mine['dataset_history'] == ck['dataset_history'] and mine['dataset2num_classes'] == ck['dataset2num_classes']
        for task, info in ck['shared_layer_info'].items():
            assert set(mine['shared_layer_info'][task]) == set(info)
            for key, entries in info.items():
                assert set(mine['shared_layer_info'][task][key]) == set(entries), (task, key)


# ================================================================ the flows
def _loader(seed, batches=3, n=8):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, 3, 32, 32, generator=g), torch.randint(0, 5, (n,), generator=g)) for _ in range(batches)]


def _session(**kw):
    from cpg_amd.baselines import BaselineSession
    return BaselineSession(arch=lambda dataset_history, dataset2num_classes: pk.hip_net(dataset_history, dataset2num_classes), device=DEV, seed=1, **kw)


def _hist(mask):
    return torch.bincount(mask.reshape(-1).to(torch.int64).cpu(), minlength=4).tolist()


def test_packnet_task_three_tasks_never_forgets(monkeypatch):
    from cpg_amd.utils.packnet_prune import SparsePruner
    seen = []
    prune = SparsePruner.one_shot_prune

    def recording_prune(self, perc):      # what each one-shot prune was given, for the host restatement below
        seen.append((int(self.current_dataset_idx), perc, {k: m.weight.data.cpu().numpy().copy() for k, m in self._layers()},
                     {k: v.cpu().numpy().copy() for k, v in self.masks.items()}))
        return prune(self, perc)
    monkeypatch.setattr(SparsePruner, 'one_shot_prune', recording_prune)
    # Inside the flow, at the end of EVERY train step (Manager.train's make_pruned_zero call: after optimizers.step, before any validate,
    # whose apply_mask would zero the free slots anyway): the step's optimizer is a PackNetSGD attached to THIS phase's pruner, and every
    # weight under owner 0 reads +0.0.
    from cpg_amd.utils.fused_sgd import PackNetSGD
    from cpg_amd.utils.packnet_manager import Manager
    steps = {'total': 0, 'with_free_slots': 0}
    zero, train = SparsePruner.make_pruned_zero, Manager.train

    def checked_zero(self, force=False):
        zero(self, force)
        steps['total'] += 1
        free_slots = 0
        for key, m in self._layers():
            free_mask = self.masks[key].cpu().numpy() == 0
            free_slots += int(free_mask.sum())
            assert not m.weight.data.cpu().numpy().view(np.uint32)[free_mask].any(), 'step %d: %s holds a value under owner 0' % (steps['total'], key)
        steps['with_free_slots'] += free_slots > 0

    def checked_train(self, optimizers, epoch_idx, curr_lrs):
        opt = optimizers[0]
        assert isinstance(opt, PackNetSGD) and opt.mode == 'fused' and opt.pruner is self.pruner and self.pruner.fused_weight_step
        assert self.pruner.masks is s.packnet.masks and self.pruner.current_dataset_idx == self.inference_dataset_idx
        return train(self, optimizers, epoch_idx, curr_lrs)
    monkeypatch.setattr(SparsePruner, 'make_pruned_zero', checked_zero)
    monkeypatch.setattr(Manager, 'train', checked_train)
    s = _session()
    loaders = {d: (_loader(20 + i), _loader(40 + i, batches=2)) for i, d in enumerate(('a', 'b', 'c'))}
    logits, free = {}, None
    for ti, d in enumerate(('a', 'b', 'c')):
        rec = s.packnet_task(d, 5, loaders[d][0], loaders[d][1], epochs=2, lr=1e-2, one_shot_prune_perc=0.6, prune_epochs=1, prune_lr=1e-3,
                             min_train_acc=-1.0)
        assert rec.kept is True and rec.baseline_acc is not None
        # owner histograms follow claim -> prune(0.6): the task claimed every free slot and nothing else, and the prune released what the
        # reference's rule releases of them (tests/_packnet.py: the k smallest magnitudes, k = round(0.6 * claimed), and every tie of the k-th)
        cur, perc, w_before, m_before = seen[-1]
        assert (cur, perc, len(seen)) == (ti + 1, 0.6, ti + 1)
        new_free = {}
        for key, m in pk.covered(s.packnet.net):
            n = m.weight.numel()
            claimed = n if free is None else free[key]
            hb = np.bincount(m_before[key].reshape(-1), minlength=5)
            assert hb[0] == 0 and hb[cur] == claimed, (d, key, hb)
            status, want, _ = pk.rank_prune_zero(w_before[key].reshape(-1), m_before[key].reshape(-1), cur, 0.6)
            got = s.packnet.masks[key].cpu().numpy().reshape(-1)
            assert status == 0 and int((got != want).sum()) == 0, (d, key)
            h = _hist(s.packnet.masks[key])
            assert h[0] >= round(0.6 * claimed) and h[cur] == claimed - h[0] and sum(h) == n, (d, key, h)
            new_free[key] = h[0]
            w = m.weight.data.cpu().numpy()
            assert not w.view(np.uint32)[s.packnet.masks[key].cpu().numpy() == 0].any()
        free = new_free
        for old in list(logits) + [d]:
            acc, outs = s.evaluate(old, loaders[old][1])
            if old in logits:
                assert all(torch.equal(a, b) for a, b in zip(outs, logits[old])), 'task %s changed after task %s' % (old, d)
            else:
                logits[old] = outs
    # 3 tasks x (2 finetune + 1 retrain epochs) x 3 batches; the retrain steps (and the finetune steps of no task: it claimed every free slot)
    # run with free slots in the masks
    assert steps == {'total': 27, 'with_free_slots': 9}, steps
    rec = s.packnet_task('d', 5, _loader(60), _loader(61, batches=2), epochs=1, prune_epochs=1, min_train_acc=1.5)
    assert rec.kept is False and rec.prune_train_acc is not None
    for key, _ in pk.covered(s.packnet.net):      # back at the finetuned stage: the task owns what it claimed, nothing is released
        h = _hist(s.packnet.masks[key])
        assert h[0] == 0 and h[4] == free[key], (key, h)
    with pytest.raises(RuntimeError, match='no free slot'):      # nothing left to claim: a further task says so instead of training the head only
        s.packnet_task('e', 5, _loader(62), _loader(63, batches=2), epochs=1, prune_epochs=1)
    assert s.packnet.net.datasets == ['a', 'b', 'c', 'd']


def test_scratch_and_finetune_tasks_and_the_goals_hand_off(tmp_path):
    from cpg_amd.baselines import read_goals
    from cpg_amd.driver import CPGSession
    s = _session()
    la, lb = (_loader(70), _loader(71, batches=2)), (_loader(72), _loader(73, batches=2))
    ra = s.scratch_task('a', 5, la[0], la[1], epochs=2, lr=1e-2)
    rb = s.scratch_task('b', 5, lb[0], lb[1], epochs=2, lr=1e-2)
    na, nb = s.models['a'].net, s.models['b'].net
    assert na is not nb and na.datasets == ['a'] and nb.datasets == ['b']
    assert all(p.data_ptr() != q.data_ptr() for p, q in zip(na.parameters(), nb.parameters()))
    assert all(bool((m == 1).all()) for m in s.models['a'].masks.values())
    goals = s.accuracy_goals()
    assert goals == {'a': '{:.4f}'.format(ra.val_acc), 'b': '{:.4f}'.format(rb.val_acc)}
    path = str(tmp_path / 'acc.txt')
    s.write_logfile(path)
    assert read_goals(path) == goals
    acc, _ = s.evaluate('a', la[1])
    assert abs(acc - ra.val_acc) < 1e-6
    # finetune_task: starts from the other task's tensors, num_batches_tracked excepted
    src = {k: v.clone() for k, v in na.state_dict().items()}
    rc = s.finetune_task('c', 5, la[0], la[1], epochs=0, initial_from='a')
    assert rc.flow == 'finetune' and 'c' not in s.accuracy_goals()
    for k, v in s.models['c'].net.state_dict().items():
        if 'num_batches_tracked' in k:
            assert int(v) == 0 and int(src[k]) > 0
        else:
            assert torch.equal(v, src[k]), k
    # the goal feeds the CPG loop
    cpg = CPGSession(width=0.125, data_parallel=False, seed=1)
    res = cpg.run_task('a', 5, la[0], la[1], accuracy_goal=float(goals['a']), finetune_epochs=1, prune_epochs=1, sparsities=(0.1,))
    assert res.finetune_acc is not None
