"""Step telemetry on the GPU: the three `_stats` entry points against their plain twins (every updated tensor bit for bit), their
records against the fp64 restatement of tests/_step_stats.py (counts, maxima, flips and picked EQUAL; every sum within n * 2^-52
relative of math.fsum: the squares are exact in fp64, so only the order of at most n non-negative additions differs, and that is
bounded by (n - 1) * 2^-53), run-to-run determinism of stats and partials, the sticky health record, and the whole path through
MaskedSGD / MaskedAdam / PackNetSGD, Manager and CPGSession with the divergence guard.  A NaN here is data: nothing faults."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _step_stats as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [1, 3, 4, 5, 255, 4095, 4096, 4097, 8193, 3 * 4096 + 7]
PATTERNS = ('mixed', 'all', 'none')
THR = 5e-3


def _lib():
    from cpg_amd import _lib as L
    return L


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


# ================================================================ raw ABI
def _layout(nonempty):
    """`nonempty` rows over SIZES in turn (49 / 97: one / two launches past the 48-row limit), an n == 0 row after every fourth, every
    row 16-byte aligned except each seventh, which starts one element later (the scalar path).  -> sizes, offsets, elements in all."""
    sizes = []
    for i in range(nonempty):
        sizes.append(SIZES[i % len(SIZES)])
        if nonempty > 1 and i % 4 == 3:
            sizes.append(0)
    offs, at = [], 0
    for i, n in enumerate(sizes):
        at = (at + 15) // 16 * 16 + (1 if i % 7 == 3 else 0)
        offs.append(at)
        at += n
    return sizes, offs, at + 16


def _single_layouts():
    """Tables of one row: every size, aligned and one element off."""
    return [([n], [off], n + 32) for n in SIZES for off in (0, 1)]


def _owner_flat(sizes, offs, total, cur, seed, shift=0):
    """Row i takes owner pattern PATTERNS[(i + shift) % 3] (shift: the table's number, so that one-row tables meet all three)."""
    owner = np.zeros(total, dtype=np.uint8)
    for i, (n, o) in enumerate(zip(sizes, offs)):
        owner[o:o + n] = S.owners(n, PATTERNS[(i + shift) % 3], cur, seed + i)
    return owner


def _items(L, kind, tensors, sizes, offs):
    rows = [tuple((t.data_ptr() + o * t.element_size()) if n else None for t in tensors) + (n,) for n, o in zip(sizes, offs)]
    return (kind * len(rows))(*rows), len(rows)


def _run(L, entry, kind, flats, sizes, offs, before, stats=False, step=1):
    """One call of `entry` (its `_stats` twin when stats) on clones of `flats` (the last one, the owner mask, is shared).  -> dict of
    numpy arrays: the tensors after the call, and stats [rows][8], partials, health."""
    tensors = [t.clone() for t in flats[:-1]] + [flats[-1]]
    items, n = _items(L, kind, tensors, sizes, offs)
    out = {}
    if stats:
        need = S.workspace_bytes(sizes)
        assert L.lib().cpg_step_stats_workspace_bytes((ctypes.c_int64 * n)(*sizes), n) == need
        st = torch.full((n, 8), 7.0, dtype=torch.float64, device=DEV)                 # (garbage: every row must be written, n == 0 rows too)
        pa = torch.full((max(need // 8, 8),), -1.0, dtype=torch.float64, device=DEV)
        he = torch.zeros(4, dtype=torch.int64, device=DEV)
        L.call(entry + '_stats', items, n, *before, step, _vp(st), _vp(pa), need, _vp(he), L.stream_ptr())
        out.update(stats=st.cpu().numpy(), partials=pa[:need // 8].cpu().numpy(), health=he.cpu().numpy())
    else:
        L.call(entry, items, n, *(before[:-1] if entry.startswith('cpg_adam') else before), L.stream_ptr())       # (the plain Adam form takes no thr)
    torch.cuda.synchronize()
    out['tensors'] = [t.cpu().numpy() for t in tensors[:-1]]
    return out


def _same_bits(a, b, names, what):
    for name, x, y in zip(names, a, b):
        assert x.tobytes() == y.tobytes(), '%s: %s differs in %d elements' % (what, name, int((x.view(np.uint32) != y.view(np.uint32)).sum()))


def _sgd_inputs(sizes, offs, total, cur, seed, shift=0):
    w, gw, buf = (S.values(total, seed + k, 0.02) for k in range(3))
    owner = _owner_flat(sizes, offs, total, cur, seed + 10, shift)
    return [torch.from_numpy(a).to(DEV) for a in (w, gw, buf, owner)]


def _check_sgd_records(got, flats, sizes, offs, cur, what, shift=0):
    w0, owner = flats[0].cpu().numpy(), flats[3].cpu().numpy()
    w1, g1 = got['tensors'][0], got['tensors'][1]
    for i, (n, o) in enumerate(zip(sizes, offs)):
        rec = dict(zip(S.SGD_FIELDS, got['stats'][i].tolist()))
        sl = slice(o, o + n)
        S.assert_record(rec, S.sgd_record(w0[sl], w1[sl], g1[sl], owner[sl], cur), n,
                        '%s row %d (n = %d, %s)' % (what, i, n, PATTERNS[(i + shift) % 3]))


@pytest.mark.parametrize('nesterov', [0, 1])
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('nonempty', [1, 49, 97])
@pytest.mark.parametrize('entry', ['cpg_sgd_route_step_multi', 'cpg_sgd_route_zero_step_multi'])
def test_sgd_stats_update_is_bit_equal_and_records_are_right(entry, nonempty, first, nesterov):
    L = _lib()
    cur = 2
    hyper = (cur, 4e-5, 1e-2, 0.9, nesterov, first)
    seen = np.zeros(len(S.SGD_FIELDS))
    for li, (sizes, offs, total) in enumerate(_single_layouts() if nonempty == 1 else [_layout(nonempty)]):
        flats = _sgd_inputs(sizes, offs, total, cur, 100 * nonempty + li, li)
        if nonempty > 1:
            assert sum(1 for n in sizes if n) == nonempty > L.lib().cpg_multi_tensor_max() and 0 in sizes
            assert any((flats[0].data_ptr() + 4 * o) % 16 for o in offs)
        plain = _run(L, entry, L.SgdItem, flats, sizes, offs, hyper)
        got = _run(L, entry, L.SgdItem, flats, sizes, offs, hyper, stats=True)
        _same_bits(plain['tensors'], got['tensors'], ('w', 'gw', 'momentum'), '%s table %d' % (entry, li))
        _check_sgd_records(got, flats, sizes, offs, cur, entry, li)
        for i, n in enumerate(sizes):
            if n == 0:
                assert not got['stats'][i].any()
        seen = np.maximum(seen, got['stats'].max(axis=0))
        again = _run(L, entry, L.SgdItem, flats, sizes, offs, hyper, stats=True)
        assert again['stats'].tobytes() == got['stats'].tobytes() and again['partials'].tobytes() == got['partials'].tobytes()
    assert (seen > 0).all(), dict(zip(S.SGD_FIELDS, seen))                          # every field was exercised, the two non-finite counts too


def _adam_inputs(sizes, offs, total, cur, adam_step, seed, shift=0):
    pm, g = S.values(total, seed, 0.02), S.values(total, seed + 1, 0.02)
    for i, (n, o) in enumerate(zip(sizes, offs)):
        if (i + shift) % 2 == 0:                                # piggymasks at / one ulp above / one ulp below the threshold, gradient +-1
            pm[o:o + n], g[o:o + n] = S.threshold_masks(n, THR, seed + 20 + i)
    if adam_step == 1:
        m1, m2 = np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.float32)
    else:
        m1, m2 = S.values(total, seed + 2), np.abs(S.values(total, seed + 3))
    owner = _owner_flat(sizes, offs, total, cur, seed + 10, shift)
    return [torch.from_numpy(a).to(DEV) for a in (pm, g, m1, m2, owner)]


@pytest.mark.parametrize('adam_step', [1, 3])
@pytest.mark.parametrize('mode', [S.MODE_FINETUNE, S.MODE_PRUNE])
@pytest.mark.parametrize('nonempty', [1, 49, 97])
def test_adam_stats_update_is_bit_equal_and_records_are_right(nonempty, mode, adam_step):
    L = _lib()
    entry, cur = 'cpg_adam_route_step_multi', 3
    before = (cur, mode, 5e-4, 0.9, 0.999, 1e-8, adam_step, THR)
    seen = np.zeros(len(S.PM_FIELDS))
    for li, (sizes, offs, total) in enumerate(_single_layouts() if nonempty == 1 else [_layout(nonempty)]):
        flats = _adam_inputs(sizes, offs, total, cur, adam_step, 1000 * nonempty + li, li)
        plain = _run(L, entry, L.AdamItem, flats, sizes, offs, before)
        got = _run(L, entry, L.AdamItem, flats, sizes, offs, before, stats=True)
        _same_bits(plain['tensors'], got['tensors'], ('pm', 'gpm', 'exp_avg', 'exp_avg_sq'), 'adam table %d' % li)
        pm0, owner = flats[0].cpu().numpy(), flats[4].cpu().numpy()
        pm1, g1 = got['tensors'][0], got['tensors'][1]
        for i, (n, o) in enumerate(zip(sizes, offs)):
            rec = dict(zip(S.PM_FIELDS, got['stats'][i].tolist()))
            sl = slice(o, o + n)
            want = S.pm_record(pm0[sl], pm1[sl], g1[sl], owner[sl], cur, mode, THR)
            S.assert_record(rec, want, n, 'adam row %d (n = %d, %s)' % (i, n, PATTERNS[(i + li) % 3]))
            if mode == S.MODE_FINETUNE and adam_step == 1 and (i + li) % 2 == 0 and want['n_routed'] >= 64:
                # the known-sign step: +1 pushes the masks above the threshold under it, -1 those at or under it above it
                assert rec['flips_on'] > 0 and rec['flips_off'] > 0 and 0 < rec['picked'] < rec['n_routed']
        seen = np.maximum(seen, got['stats'].max(axis=0))
        again = _run(L, entry, L.AdamItem, flats, sizes, offs, before, stats=True)
        assert again['stats'].tobytes() == got['stats'].tobytes() and again['partials'].tobytes() == got['partials'].tobytes()
    fields = dict(zip(S.PM_FIELDS, seen))
    if mode == S.MODE_FINETUNE:
        assert all(v > 0 for v in fields.values()), fields
    else:       # prune mode keeps no slot: the non-finite count remains, and the step's size once the moments are not zero (Adam step 3)
        assert fields['pm_nonfinite'] > 0 and (fields['dpm_sumsq'] > 0) == (adam_step == 3), fields
        assert all(fields[k] == 0 for k in ('n_routed', 'g_sumsq', 'g_absmax', 'flips_on', 'flips_off', 'picked')), fields


def test_a_refused_stats_call_changes_nothing():
    L = _lib()
    sizes, offs, total = _layout(49)
    flats = _sgd_inputs(sizes, offs, total, 2, 7)
    tensors = [t.clone() for t in flats]
    items, n = _items(L, L.SgdItem, tensors, sizes, offs)
    need = S.workspace_bytes(sizes)
    st = torch.full((n, 8), 7.0, dtype=torch.float64, device=DEV)
    pa = torch.full((need // 8,), -1.0, dtype=torch.float64, device=DEV)
    he = torch.zeros(4, dtype=torch.int64, device=DEV)
    for kw, code in ((dict(nbytes=need - 1), -3), (dict(step=0), -1), (dict(stats=ctypes.c_void_p(st.data_ptr() + 8)), -1)):
        with pytest.raises(L.CpgHipError) as e:
            L.call('cpg_sgd_route_step_multi_stats', items, n, 2, 4e-5, 1e-2, 0.9, 1, 0, kw.get('step', 1), kw.get('stats', _vp(st)), _vp(pa),
                   kw.get('nbytes', need), _vp(he), L.stream_ptr())
        assert e.value.code == code
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(tensors, flats))       # (bytes: the inputs hold NaNs)
    assert bool((st == 7.0).all()) and bool((pa == -1.0).all()) and not bool(he.any())


def test_health_record_is_sticky_and_picks_the_lowest_item():
    L = _lib()
    cur = 2
    sizes, offs = [300, 5000, 0, 4097, 77], [0, 304, 5312, 5312, 9424]
    total = 9520
    rng = np.random.RandomState(3)
    w, gw, buf = ((rng.standard_normal(total) * 1e-2).astype(np.float32) for _ in range(3))
    owner = _owner_flat(sizes, offs, total, cur, 5)
    owner[[offs[0] + 1, offs[1] + 4500, offs[3] + 9]] = cur                          # slots of the current task to plant a NaN in
    flats = [torch.from_numpy(a).to(DEV) for a in (w, gw, buf, owner)]
    items, n = _items(L, L.SgdItem, flats, sizes, offs)
    need = S.workspace_bytes(sizes)
    st = torch.zeros(n, 8, dtype=torch.float64, device=DEV)
    pa = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    he = torch.zeros(4, dtype=torch.int64, device=DEV)

    def step(k, first):
        L.call('cpg_sgd_route_step_multi_stats', items, n, cur, 0.0, 1e-2, 0.9, 1, first, k, _vp(st), _vp(pa), need, _vp(he), L.stream_ptr())
        return he.cpu().tolist()
    assert step(1, 1) == [0, 0, 0, 0]                                                # a clean step
    flats[1][offs[3] + 9] = float('nan')                                             # item 3 ...
    flats[1][offs[1] + 4500] = float('nan')                                          # ... and item 1 (its second piece), both at step 2
    assert step(2, 0) == [2, 1, 1, 1]
    rec = dict(zip(S.SGD_FIELDS, st.cpu().numpy()[1].tolist()))
    assert rec['g_nonfinite'] == 1 and rec['w_nonfinite'] == 1
    flats[1].normal_(0, 1e-2)
    flats[1][offs[0] + 1] = float('inf')                                             # a later bad step, in a lower item: only bad_steps moves
    assert step(3, 0) == [2, 1, 1, 2]
    # kind 2: a non-finite weight whose routed gradient is fine -- a slot of ANOTHER task (its gradient is routed to 0, never formed from w)
    kw, kg, kb = torch.ones(100, device=DEV), torch.full((100,), 0.5, device=DEV), torch.zeros(100, device=DEV)
    kown = torch.ones(100, dtype=torch.uint8, device=DEV)
    kown[50:] = cur
    kw[5] = float('nan')
    kitems, kn = _items(L, L.SgdItem, [kw, kg, kb, kown], [100], [0])
    fresh = torch.zeros(4, dtype=torch.int64, device=DEV)
    L.call('cpg_sgd_route_step_multi_stats', kitems, kn, cur, 4e-5, 1e-2, 0.9, 1, 1, 7, _vp(st), _vp(pa), 64, _vp(fresh), L.stream_ptr())
    assert fresh.cpu().tolist() == [7, 0, 2, 1] and he.cpu().tolist() == [2, 1, 1, 2]
    rec = dict(zip(S.SGD_FIELDS, st.cpu().numpy()[0].tolist()))
    assert (rec['n_routed'], rec['g_nonfinite'], rec['w_nonfinite'], rec['w_absmax']) == (50, 0, 1, 1.0)
    # the piggymask form has no gradient count: a NaN gradient in a kept slot shows as a non-finite piggymask, kind 2
    asz, aoff = [100, 4200], [0, 112]
    pm = torch.full((4400,), 0.01, device=DEV)
    g, m1, m2 = torch.zeros_like(pm), torch.zeros_like(pm), torch.zeros_like(pm)
    own = torch.ones(4400, dtype=torch.uint8, device=DEV)
    g[aoff[1] + 4100] = float('nan')
    aitems, an = _items(L, L.AdamItem, [pm, g, m1, m2, own], asz, aoff)
    ast = torch.zeros(an, 8, dtype=torch.float64, device=DEV)
    ahe = torch.zeros(4, dtype=torch.int64, device=DEV)
    L.call('cpg_adam_route_step_multi_stats', aitems, an, 2, S.MODE_FINETUNE, 5e-4, 0.9, 0.999, 1e-8, 1, THR, 9, _vp(ast), _vp(pa),
           S.workspace_bytes(asz), _vp(ahe), L.stream_ptr())
    assert ahe.cpu().tolist() == [9, 1, 2, 1]
    assert dict(zip(S.PM_FIELDS, ast.cpu().numpy()[1].tolist()))['pm_nonfinite'] == 1


# ================================================================ through the optimizers, Manager and CPGSession
def _batches(seed, n=3, ncls=5):
    g = torch.Generator().manual_seed(seed)
    return [((0.5 * torch.randn(4, 3, 32, 32, generator=g)).to(DEV), torch.randint(0, ncls, (4,), generator=g).to(DEV)) for _ in range(n)]


def _masked(sess):
    from cpg_amd.driver import masked_layers
    return masked_layers(sess.net)


def _layer_names():
    from cpg_amd.driver import CPGSession
    return [n for n, _ in _masked(CPGSession('custom_vgg_cifar100', 0.125, device='cpu', seed=1, data_parallel=False))]


class _Loop(object):
    """Three steps of Manager.train on a width-0.125 custom_vgg_cifar100 at batch 4, with the tensors around the LAST optimizer step."""

    def __init__(self, mode, task2, telemetry=False, stop=False, poison=None, multi=True, monkeypatch=None):
        from cpg_amd.driver import CPGSession, default_args
        from cpg_amd.utils import Optimizers, fused_sgd
        if monkeypatch is not None:
            monkeypatch.setattr(fused_sgd, 'MULTI_TENSOR', multi)
        sess = self.sess = CPGSession('custom_vgg_cifar100', 0.125, device=DEV, seed=1, data_parallel=False, telemetry=telemetry,
                                      stop_on_nonfinite=stop)
        args = default_args(lr=5e-2, lr_mask=5e-4, pruning_frequency=1, pruning_interval=1, prune_lr=1e-2, dataset='t1')
        def claim():                                   # what a finetune phase does first: the task takes every free slot
            sess._manager(args, [], [], 0, 0).pruner.make_finetuning_mask()
        sess.start_task('t1', 5)
        if task2:
            # task 1 claims everything, then gives a third of its slots back (a prune without the training); task 2 works in them
            claim()
            g = torch.Generator().manual_seed(2)
            for k, v in sess.masks.items():
                v[(torch.rand(v.shape, generator=g) < 0.33).to(DEV)] = 0
            sess.commit_task('t1')
            args.dataset = 't2'
            sess.start_task('t2', 5)
        if mode == 'prune':                            # (a prune phase follows a finetune phase: the slots are the task's already)
            claim()
            args.mode, args.initial_sparsity, args.target_sparsity, args.lr, args.lr_mask = 'prune', 0.0, 0.3, 1e-2, 0.0
        mgr = self.mgr = sess._manager(args, _batches(11), [], 0, 3 if mode == 'prune' else 0)
        if mode == 'finetune':
            mgr.pruner.make_finetuning_mask()
        opts = sess.make_optimizers(args, mgr.pruner)
        layers = self.layers = _masked(sess)
        self.names = [n for n, _ in layers]
        if poison is not None:                         # one NaN in one layer's weight gradient at step 2, as the backward pass hands it over
            calls = []

            def hook(grad):
                calls.append(1)
                if len(calls) == 2:
                    grad = grad.clone()
                    grad.view(-1)[3] = float('nan')
                    return grad
            dict(layers)[poison].weight.register_hook(hook)
        loop = self

        class Capture(Optimizers):
            def step(self):
                loop.before = loop._snap()
                Optimizers.step(self)
                loop.after = loop._snap(grads=True)
        cap = Capture()
        cap.optimizers, cap.lrs = opts.optimizers, opts.lrs
        self.opts = cap
        self.cur = int(mgr.pruner.current_dataset_idx)
        self.mode = mode
        mgr.train(cap, 0, list(opts.lrs), 0)
        torch.cuda.synchronize()

    def _snap(self, grads=False):
        out = {}
        for n, m in self.layers:
            out[n] = dict(w=m.weight.detach().cpu().numpy().copy(), owner=self.sess.masks[n].cpu().numpy().copy(),
                          pm=None if m.piggymask is None else m.piggymask.detach().cpu().numpy().copy())
            if grads:
                out[n]['gw'] = m.weight.grad.cpu().numpy().copy()
                out[n]['gpm'] = None if m.piggymask is None or m.piggymask.grad is None else m.piggymask.grad.cpu().numpy().copy()
        return out

    def final(self):
        out = {n: m.weight.detach().cpu().numpy().tobytes() for n, m in self.layers}
        out.update({n + '.pm': m.piggymask.detach().cpu().numpy().tobytes() for n, m in self.layers if m.piggymask is not None})
        out.update({n + '.owner': self.sess.masks[n].cpu().numpy().tobytes() for n, _ in self.layers})
        return out


@pytest.mark.parametrize('mode,task2', [('finetune', False), ('prune', False), ('finetune', True)])
def test_manager_telemetry_leaves_training_alone_and_reports_the_last_step(mode, task2):
    off = _Loop(mode, task2)
    on = _Loop(mode, task2, telemetry=True)
    assert off.mgr.last_telemetry is None and off.mgr.telemetry is None
    assert on.final() == off.final()                                                # weights, piggymasks and owner masks, bit for bit
    tel = on.mgr.last_telemetry
    assert sorted(tel) == sorted(on.names) and len(tel) == 15
    owners = {n: on.before[n]['owner'] for n in on.names}          # (as the step saw them: a prune-mode step is followed by a rank prune)
    picked = kept = 0
    for n in on.names:
        rec, b, a = tel[n], on.before[n], on.after[n]
        size = b['w'].size
        S.assert_record(rec, S.sgd_record(b['w'], a['w'], a['gw'], owners[n], on.cur), size, n)
        assert rec['g_norm'] == rec['g_sumsq'] ** 0.5 and rec['update_ratio'] == (rec['dw_sumsq'] / rec['w_sumsq']) ** 0.5
        assert rec['g_nonfinite'] == rec['w_nonfinite'] == 0 and rec['n_routed'] > 0 and 0 < rec['update_ratio'] < 1
        if task2:
            want = S.pm_record(b['pm'], a['pm'], a['gpm'], owners[n], on.cur, S.MODE_FINETUNE, THR)
            S.assert_record({k: rec[k if k in rec and k not in S.SGD_FIELDS else 'pm_' + k] for k in S.PM_FIELDS}, want, size, n + ' piggymask')
            older = (owners[n] > 0) & (owners[n] < on.mgr.pruner.inference_dataset_idx)
            num, den = int(((a['pm'] > np.float32(0.005)) & older).sum()), int(older.sum())
            assert (rec['picked'], rec['pm_n_routed']) == (num, den) and rec['picked_ratio'] == num / den
            assert rec['flips'] == rec['flips_on'] + rec['flips_off']
            picked, kept = picked + num, kept + den
        else:
            assert 'picked' not in rec
    if task2:
        assert on.mgr.pruner.calculate_shared_part_ratio() == picked / kept
    assert on.mgr.telemetry.health() == {'first_bad_step': 0, 'layer': None, 'kind': 0, 'bad_steps': 0}


def test_prune_phase_piggymasks_report_the_idle_record_without_a_launch(monkeypatch):
    """Task 2 in prune mode: MaskedAdam's idle shortcut runs no kernel; the piggymask records are the all-zero record the STATS kernel
    gives any prune-mode step (no slot is kept outside finetune mode)."""
    L = _lib()
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    on = _Loop('prune', True, telemetry=True)
    assert 'cpg_adam_route_step_multi_stats' not in calls and 'cpg_adam_route_step_multi' not in calls
    assert calls.count('cpg_sgd_route_step_multi_stats') == 3 and 'cpg_sgd_route_step_multi' not in calls
    for n in on.names:
        rec = on.mgr.last_telemetry[n]
        assert rec['picked'] == rec['pm_n_routed'] == rec['flips'] == rec['pm_nonfinite'] == 0 and rec['picked_ratio'] is None
        assert rec['n_routed'] > 0


def test_one_row_per_call_without_multi_tensor(monkeypatch):
    """CPG_MULTI_TENSOR=0: the `_stats` entry points still run, one row per call; same weights, same records, same guard."""
    names = _layer_names()
    ref = _Loop('finetune', True, telemetry=True, monkeypatch=monkeypatch, multi=True)
    one = _Loop('finetune', True, telemetry=True, monkeypatch=monkeypatch, multi=False)
    assert one.final() == ref.final() and one.mgr.last_telemetry == ref.mgr.last_telemetry
    bad = _Loop('finetune', False, telemetry=True, poison=names[4], monkeypatch=monkeypatch, multi=False)
    h = bad.mgr.telemetry.health()
    assert (h['first_bad_step'], h['layer'], h['kind']) == (2, names[4], 1)


def test_the_guard_names_the_layer_the_step_and_the_kind():
    from cpg_amd.utils.telemetry import TrainingDiverged
    layer = _layer_names()[6]
    with pytest.raises(TrainingDiverged) as e:
        _Loop('finetune', False, stop=True, poison=layer)
    assert (e.value.step, e.value.layer, e.value.kind) == (2, layer, 1)
    # without the switch nothing raises, and health() reports it: step 3 ran on the poisoned weights, so it counts as bad too
    quiet = _Loop('finetune', False, telemetry=True, poison=layer)
    h = quiet.mgr.telemetry.health()
    assert h == {'first_bad_step': 2, 'layer': layer, 'kind': 1, 'bad_steps': 2}
    with pytest.raises(TrainingDiverged):
        quiet.mgr.telemetry.check()


def test_a_diverged_finetune_leaves_run_task_as_an_exception_and_never_grows():
    """A finetune with an unreachable accuracy goal and room to grow: without the guard its chance accuracy reads as "capacity exhausted"
    and run_task widens the network.  With stop_on_nonfinite the NaN step ends run_task with TrainingDiverged, at the width it had."""
    from cpg_amd.driver import CPGSession, default_args
    from cpg_amd.utils.telemetry import TrainingDiverged
    args = default_args(lr=5e-2, lr_mask=5e-4, pruning_frequency=1, pruning_interval=1, prune_lr=1e-2)
    sess = CPGSession('custom_vgg_cifar100', 0.125, device=DEV, seed=1, data_parallel=False, stop_on_nonfinite=True)
    layer, module = _masked(sess)[2]
    calls = []

    def hook(grad):
        calls.append(1)
        if len(calls) == 2:
            grad = grad.clone()
            grad.view(-1)[0] = float('nan')
            return grad
    module.weight.register_hook(hook)
    with pytest.raises(TrainingDiverged) as e:
        sess.run_task('t1', 5, _batches(21), _batches(22, n=1), accuracy_goal=2.0, finetune_epochs=1, prune_epochs=1, sparsities=(0.3,),
                      args=args, min_train_acc=-1.0, max_width_multiplier=0.0625, width_step=0.046875)
    assert (e.value.step, e.value.layer, e.value.kind) == (2, layer, 1)
    assert sess.width == 0.125 and sess.width_multiplier == 0.015625 and len(calls) == 3


def test_packnet_sgd_feeds_the_telemetry():
    """PackNetSGD(telemetry=...): the zeroing pass's `_stats` twin; same weights as without, records of the last step."""
    from cpg_amd.utils.fused_sgd import PackNetSGD
    from cpg_amd.utils.telemetry import StepTelemetry
    import torch.nn as nn
    outs = []
    for tel in (None, StepTelemetry()):
        torch.manual_seed(4)
        net = nn.Sequential(nn.Conv2d(3, 8, 3, bias=False), nn.ReLU(), nn.Flatten(), nn.Linear(8 * 36, 5)).to(DEV)
        layers = [('0', net[0]), ('3', net[3])]
        masks = {n: torch.randint(0, 3, m.weight.shape, dtype=torch.uint8, device=DEV) for n, m in layers}
        pruner = types.SimpleNamespace(_layers=lambda: layers, _owner=lambda name, like: masks[name], current_dataset_idx=2,
                                       args=types.SimpleNamespace(weight_decay=4e-5), fused_weight_step=False)
        opt = PackNetSGD(net.parameters(), pruner=pruner, lr=1e-2, telemetry=tel)
        x = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
        for _ in range(2):
            opt.zero_grad()
            before = [m.weight.detach().cpu().numpy().copy() for _, m in layers]
            net(x).square().mean().backward()
            opt.step()
        outs.append([m.weight.detach().cpu().numpy().tobytes() for _, m in layers])
        if tel is not None:
            got = tel.read()
            for (n, m), w0 in zip(layers, before):
                S.assert_record(got[n], S.sgd_record(w0, m.weight.detach().cpu().numpy(), m.weight.grad.cpu().numpy(), masks[n].cpu().numpy(), 2),
                                w0.size, 'packnet ' + n)
                assert not m.weight.detach()[masks[n] == 0].any()
    assert outs[0] == outs[1]
    with pytest.raises(ValueError):
        PackNetSGD(net.parameters(), pruner=pruner, lr=1e-2, mode='unfused', telemetry=StepTelemetry())
