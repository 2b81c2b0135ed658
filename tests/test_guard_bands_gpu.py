"""The fp64 / oracle parity tests once more with every buffer between guard bands (tests/_guarded.py).

Each case builds its const inputs as guarded, frozen tensors, runs a body shared with the plain test of the same name
(tests/_parity_cases.py, _eval_*_cases.py, _loss_cases.py) inside guarding(), so that every output and workspace the Python mirror
allocates is a NaN-filled window of exactly the requested size between two 64 KiB guards, and then asks the ledger whether anything
outside a payload, or any const input, changed.  The numeric check is the shared body's own: no tolerance is introduced here.  A
case is not allowed to be vacuous: what the body returned must lie in ledger memory, the route must have asked the interposed
workspace allocator and not the original one, and no allocation may have slipped past the interposer.

Shapes are the smallest that reach each kernel class.  Known limit: a stray access further than 64 KiB from its buffer is not seen."""
import ctypes

import numpy as np
import pytest
import torch

import _conv_space_cases as CS
import _eval_block_cases as EB
import _eval_conv_cases as EC
import _guarded as G
import _loss_cases as LC
import _parity_cases as PC
import _prelu_eval_cases as PE
from _guarded import GUARD_BYTES, GuardedBuffers, guarding
from oracle import ops

pytestmark = pytest.mark.gpu

from cpg_amd import _lib as L                    # noqa: E402

DEV = PC.DEV
BUF = GuardedBuffers(DEV)


def finish(ledger, outs=(), asked_workspace=True, assembled_by_torch=False):
    """The guards, then the not-vacuous part.  assembled_by_torch: the route hands torch per-group pieces to concatenate, so what the
    body returned is torch's; the pieces the kernels wrote must then number at least as many."""
    ledger.verify()
    if assembled_by_torch:
        assert ledger.intercepted >= len(outs) >= 1
    for i, t in enumerate(outs):
        assert assembled_by_torch or ledger.holds(t), 'output %d of the body is not in guarded memory' % i
    if asked_workspace:
        assert ledger.workspace_requests >= 1
    assert ledger.original_workspace_calls == 0
    assert ledger.passed_through == [], ledger.passed_through
    assert ledger.arenas


# --------------------------------------------------------------------------- the harness itself, on the device
def test_detection_on_the_device():
    """tests/test_guarded_host.py's detection cases with the arenas in device memory: the compare that runs on the device sees a torch
    write into the arena on either side of the payload, and passes a write that stays inside."""
    led = G.Ledger()
    t = led.guarded((4, 6), torch.float32, DEV, label='before')
    assert t.is_cuda and t.data_ptr() % 512 == 0 and bool(torch.isnan(t).all())
    t.fill_(1.0)
    led.verify()
    led.arena_of(t).raw[GUARD_BYTES - 4: GUARD_BYTES].view(torch.float32)[0] = 1.0
    a = led.guarded((4, 6), torch.float32, DEV, label='after')
    led.arena_of(a).raw[GUARD_BYTES + 96: GUARD_BYTES + 100].view(torch.float32)[0] = 0.0
    o = led.guarded((4097,), torch.uint8, DEV, label='owner')
    o.fill_(3)
    led.arena_of(o).raw[GUARD_BYTES + 4097] = 0
    f = led.guarded((10,), torch.float32, DEV, label='far')
    led.arena_of(f).raw[-1] = 0
    x = led.guarded((6, 7), torch.float32, DEV, init=torch.randn(6, 7), frozen=True, label='frozen')
    x.view(torch.int32)[2, 3] ^= 1 << 9
    led.guarded((5,), torch.float32, DEV, label='clean')
    assert led.check() == [G.Violation('before', (4, 6), 'front', -4, 4), G.Violation('after', (4, 6), 'back', 96, 4),
                           G.Violation('owner', (4097,), 'back', 4097, 1), G.Violation('far', (10,), 'back', 40 + GUARD_BYTES - 1, 1),
                           G.Violation('frozen', (6, 7), 'payload', (2 * 7 + 3) * 4 + 1, 1)]
    with pytest.raises(G.GuardViolation):
        led.verify()


def test_interposer_on_the_device():
    from cpg_amd.models import layers as nl
    real = L.workspace
    with guarding() as led:
        ws, nb = L.workspace(10, DEV)
        assert led.owns(ws) and nb == 12 and led.arena_of(ws).nbytes == 12 and bool(torch.isnan(ws).all())
        y = nl.torch.empty((3, 5), dtype=torch.float32, device=DEV)
        z = nl.torch.zeros_like(y)
        assert led.owns(y) and led.owns(z) and bool(torch.isnan(y).all()) and not bool(z.any())
        assert not led.owns(torch.empty(3, device=DEV))
        real(8, DEV)
        assert led.original_workspace_calls == 1 and led.workspaces == 1 and led.workspace_requests == 1
        led.verify()
    assert L.workspace is real and nl.torch is torch


# --------------------------------------------------------------------------- convolutions
def _conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _small(row):
    N, C, H, W, K, k, s, p = row[:8]
    return N * C * H * W <= 1 << 21 and N * K * _conv_out(H, k, s, p) * _conv_out(W, k, s, p) <= 1 << 21


CONV_ROWS = [r for r in PC.CONV_ORACLE_CASES if _small(r)]
NO_WINO = {'CPG_NO_WINO': 1, 'CPG_NO_WINO_WGRAD': 1}
CONV_CASES = ([(r, {}) for r in CONV_ROWS] + [(r, NO_WINO) for r in CONV_ROWS] + [(r, {'CPG_NO_STEM': 1}) for r in CONV_ROWS if r[1] <= 3]
              + [(r, {'CPG_WINO_KERNEL': v}) for v in ('wave', 'pair', '64', 'block') for r in CONV_ROWS
                 if r[5:8] == (3, 1, 1) and r[1] >= 16 and r[4] >= 16])
CONV_REFS = {}          # the oracle's results per row, shared by the option tables


def _conv_id(case):
    row, opts = case
    return '-'.join(str(int(v)) for v in row) + ''.join('-%s=%s' % (k[4:], v) for k, v in sorted(opts.items()))


def test_the_conv_table_kept_its_ragged_rows():
    rows = {r[:8] for r in CONV_ROWS}
    for must in [(2, 4, 1, 1, 8, 3, 1, 1), (1, 16, 2, 3, 16, 3, 1, 1), (6, 32, 7, 7, 160, 3, 1, 1), (4, 16, 14, 14, 72, 3, 1, 1),
                 (2, 32, 12, 28, 128, 3, 1, 1), (2, 24, 11, 56, 130, 3, 1, 1), (3, 64, 28, 28, 256, 1, 1, 0), (3, 256, 28, 28, 512, 1, 2, 0),
                 (2, 20, 15, 17, 24, 3, 2, 1), (1, 8, 20, 20, 8, 5, 3, 2), (3, 3, 64, 70, 64, 7, 2, 3), (5, 3, 30, 64, 64, 3, 2, 1),
                 (3, 18, 12, 20, 19, 3, 1, 1), (2, 67, 14, 14, 61, 3, 1, 1)]:
        assert must in rows, must
    assert not any(r[2] == 224 and r[5] == 3 for r in CONV_ROWS)          # the 224-wide 3x3 rows are the plain test's
    assert len(CONV_ROWS) >= 40


@pytest.mark.parametrize('case', CONV_CASES, ids=_conv_id)
def test_conv_oracle_guarded(case, libopt):
    row, opts = case
    for name, v in opts.items():
        libopt.set(name, v)
    with guarding() as led:
        outs = PC.conv_oracle(*row, buf=BUF, refs=CONV_REFS)
        finish(led, outs)


@pytest.mark.parametrize('row', PC.GROUPED_CONV_CASES, ids=lambda r: '-'.join(str(int(v)) for v in r))
def test_grouped_conv_guarded(row):
    from cpg_amd.models import layers as nl
    N, C, K, H, W, k, s, p, G = row[:9]
    per_group = nl.SharableConv2d(C, K, k, stride=s, padding=p, groups=G)._per_group()       # one groups == 1 launch per group + torch.cat
    with guarding() as led:
        finish(led, PC.grouped_conv_vs_oracle(*row, buf=BUF), assembled_by_torch=per_group)


@pytest.mark.parametrize('cid', list(CS.CASE_BY_ID))
def test_conv_descriptor_space_guarded(cid):
    """The hand table of tests/_conv_space_cases.py -- near misses of every fast class, the generic family's branches, degenerate
    geometry, grouped layers off the templates -- between guard bands: a workspace query that under-sizes an unusual descriptor, or a
    tile that assumes its class's geometry, writes outside its payload."""
    from cpg_amd.models import layers as nl
    c = CS.CASE_BY_ID[cid]
    per_group = c.G > 1 and nl.SharableConv2d(c.C, c.K, (c.R, c.S), stride=(c.sh, c.sw), padding=(c.ph, c.pw), dilation=(c.dh, c.dw),
                                              groups=c.G)._per_group()
    with guarding() as led:
        finish(led, CS.conv_space(c, buf=BUF), assembled_by_torch=per_group)


def test_winograd_tail_guarded(libopt):
    N, C, K, H, bias = PC.WINOGRAD_TAIL_CASES[0]
    assert (N, C, K, H, bias) == (256, 256, 256, 14, True)
    with guarding() as led:
        finish(led, PC.winograd_tail_pieces_equal_the_single_launch(N, C, K, H, bias, libopt, buf=BUF))


def test_winograd_tail_degrade_guarded(libopt):
    """... and the launch in a workspace that ends behind the packed filter writes no tail piece past it."""
    with guarding() as led:
        finish(led, PC.winograd_tail_degrades_to_the_single_launch(libopt, buf=BUF))


# --------------------------------------------------------------------------- linear
@pytest.mark.parametrize('B,I,O,pm', [(7, 513, 129, True), (1, 64, 5, False)])
def test_linear_oracle_guarded(B, I, O, pm):
    assert (B, I, O, pm) in PC.LINEAR_ORACLE_CASES
    with guarding() as led:
        finish(led, PC.linear_oracle(B, I, O, pm, buf=BUF))


@pytest.mark.parametrize('seed', PC.LINEAR_SMALL_BATCH_SEEDS)
def test_linear_small_batch_guarded(seed):
    with guarding() as led:
        finish(led, PC.linear_small_batch_random_shapes(seed, buf=BUF))


# --------------------------------------------------------------------------- BatchNorm, PReLU, fused stem
BN_RELU_SMALL = [c for c in PC.bn_relu_cases() if np.prod(c.values[1:5]) <= 1 << 16]


@pytest.mark.parametrize('training,N,C,H,W,misaligned', BN_RELU_SMALL)
def test_bn_relu_guarded(training, N, C, H, W, misaligned):
    with guarding() as led:
        finish(led, PC.fused_bn_relu_matches_torch(N, C, H, W, training, misaligned, buf=BUF))


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('N,C,H,W', [(3, 5, 6, 10), (2, 3, 2, 2)])
def test_bn_relu_pool_guarded(N, C, H, W, training):
    assert (N, C, H, W) in PC.BN_RELU_POOL_SHAPES
    with guarding() as led:
        finish(led, PC.fused_bn_relu_pool_matches_torch(N, C, H, W, training, buf=BUF))


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('N,C,H,W', [(3, 5, 7, 9), (2, 3, 1, 1), (2, 8, 16, 15)])
def test_bn_relu_pool3_guarded(N, C, H, W, training):
    assert (N, C, H, W) in PC.BN_RELU_POOL3_SHAPES
    with guarding() as led:
        finish(led, PC.fused_bn_relu_pool3_matches_torch(N, C, H, W, training, buf=BUF))


@pytest.mark.parametrize('N,C,H,W,relu,add', PC.BN_SMALL_PLANES_CASES)
def test_bn_small_planes_guarded(N, C, H, W, relu, add):
    with guarding() as led:
        finish(led, PC.fused_bn_small_planes_fp64(N, C, H, W, relu, add, buf=BUF))


@pytest.mark.parametrize('N,C,H,W', [(5, 8, 14, 14), (2, 8, 7, 7), (130, 4, 12, 20)])
def test_bn_add_relu_byte_mask_guarded(N, C, H, W, monkeypatch):
    assert (N, C, H, W) in PC.BN_ADD_RELU_MASK_SHAPES
    with guarding() as led:
        finish(led, PC.bn_add_relu_byte_mask_equals_reading_the_output(N, C, H, W, monkeypatch, buf=BUF))


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('N,C,H,W', [(5, 12, 7, 9), (2, 3, 1, 1)])
def test_prelu_backward_guarded(N, C, H, W, shared):
    with guarding() as led:
        finish(led, PC.prelu_backward_matches_torch(N, C, H, W, shared, buf=BUF))


@pytest.mark.parametrize('K', [64, 65, 78])
@pytest.mark.parametrize('wgrad_in_pass', [True, False])
@pytest.mark.parametrize('N,C,H,W,pm', [(5, 1, 17, 33, False), (3, 3, 40, 70, False)])
def test_fused_stem_guarded(N, C, H, W, pm, wgrad_in_pass, K, monkeypatch):
    assert (N, C, H, W, pm) in PC.FUSED_STEM_SHAPES and K in PC.FUSED_STEM_K
    with guarding() as led:
        finish(led, PC.fused_stem_conv_bn_relu_matches_unfused(N, C, H, W, pm, wgrad_in_pass, K, monkeypatch, buf=BUF))


# --------------------------------------------------------------------------- inference epilogues (raw C ABI)
def _raw_abi_finish(led, ws_bytes):
    """y and skip_stats came from BUF.full, the inputs from BUF.put: all in the ledger by construction -- so count them."""
    finish(led, asked_workspace=True)
    assert any(a.label.startswith('full(') for a in led.arenas) and any(a.label.startswith('input') for a in led.arenas)
    assert (led.workspaces > 0) == (ws_bytes > 0), (led.workspaces, ws_bytes)


@pytest.mark.parametrize('cid', [c[0] for c in EC.CASES])
def test_eval_conv_guarded(cid, libopt):
    with guarding() as led:
        EC.eval_conv_case(cid, libopt, buf=BUF)
        _raw_abi_finish(led, EC._ws_bytes(EC.CASE_BY_ID[cid][3]))


@pytest.mark.parametrize('cid', list(EB.CASES))
def test_eval_block_guarded(cid, libopt):
    with guarding() as led:
        EB.eval_block_case(cid, libopt, buf=BUF)
        _, k, (N, C, H, W, K, s), _, _ = EB.CASES[cid]
        _raw_abi_finish(led, int(L.lib().cpg_conv2d_workspace_bytes(ctypes.byref(EB._desc(N, C, H, W, K, k, s)))))


@pytest.mark.parametrize('cid', list(PE.CASES))
def test_prelu_eval_guarded(cid, libopt):
    with guarding() as led:
        PE.prelu_eval_case(cid, libopt, buf=BUF)
        shape, s, _ = PE.CASES[cid]
        _raw_abi_finish(led, int(L.lib().cpg_conv2d_workspace_bytes(ctypes.byref(PE._desc(shape, s)))))


# --------------------------------------------------------------------------- loss heads
@pytest.mark.parametrize('B,C,weights', LC.XENT_CASES)
def test_cross_entropy_guarded(B, C, weights):
    """Forward-backward: the shared body.  Forward only (no_grad): the loss against the same fp64 arbiter at the same bar."""
    with guarding() as led:
        LC.cross_entropy_case(B, C, weights, buf=BUF)
        made = []
        LC.fused_xent(*LC.xent_inputs(B, C, weights), buf=BUF, made=made)
        finish(led, made)
    from cpg_amd.models.losses import FusedCrossEntropyLoss
    z, t, w = LC.xent_inputs(B, C, weights)
    l64, _ = LC.stock_xent(z, t, w, torch.float64)
    l32, _ = LC.stock_xent(z, t, w, torch.float32)
    with guarding() as led:
        crit = BUF.rehome(FusedCrossEntropyLoss(weight=w).to(DEV), const_buffers=True)
        with torch.no_grad():
            loss = crit(BUF.put(z), BUF.put(t))
        LC.hold('forward-only loss %dx%d %s' % (B, C, weights), loss.cpu().numpy(), l32, l64)
        assert float(crit.correct) == int((z.argmax(1) == t).sum())
        finish(led, [loss, crit.correct])


@pytest.mark.parametrize('B,D,C', LC.ANGLE_SWEEP_SHAPES)
def test_angle_head_guarded(B, D, C):
    with guarding() as led:
        LC.angle_head_margin_sweep(B, D, C, 3000, buf=BUF)
        x, w, t = LC.sweep_reference(B, D, C, 3000)[:3]
        made = []
        LC.fused_angle(x, w, t, 3000, buf=BUF, made=made)
        finish(led, made)


# --------------------------------------------------------------------------- in-place element-wise kernels (raw C ABI)
ELEMENTWISE_SIZES = [1, 3, 5, 1023, 1025, 4099]
CUR, WD = 3, 4e-5


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _elementwise_inputs(n, seed=0):
    g = torch.Generator().manual_seed(1009 * n + seed)
    w = torch.randn(n, generator=g) * 0.05
    owner = torch.randint(0, 5, (n,), generator=g, dtype=torch.uint8)         # 0 free, 1 / 2 older tasks, 3 the current one, 4 a later one
    pm = torch.rand(n, generator=g) * 0.012
    return g, w, owner, pm


@pytest.mark.parametrize('mode', ['finetune', 'prune'])
@pytest.mark.parametrize('n', ELEMENTWISE_SIZES)
def test_route_grads_guarded(n, mode):
    g, w, owner, _ = _elementwise_inputs(n)
    gw, gpm = torch.randn(n, generator=g), torch.randn(n, generator=g)
    with guarding() as led:
        dgw, dgpm = BUF.copy(gw), BUF.copy(gpm)
        L.call('cpg_route_grads', _ptr(dgw), _ptr(BUF.put(w)), _ptr(BUF.put(owner)), CUR, WD, _ptr(dgpm),
               L.MODE_PRUNE if mode == 'prune' else L.MODE_FINETUNE, n, L.stream_ptr())
        wg, wp = ops.route_grads(gw.numpy(), w.numpy(), owner.numpy(), CUR, WD, gpm.numpy(), mode)
        np.testing.assert_allclose(dgw.cpu().numpy(), wg, rtol=3e-7, atol=0)          # (test_owner_id_uint8_extremes_vs_oracle's bar)
        np.testing.assert_array_equal(dgpm.cpu().numpy(), wp)
        finish(led, [dgw, dgpm], asked_workspace=False)


def _sgd_oracle(w, owner, grads, zero):
    """The CPU oracle's routing followed by torch-CPU SGD-nesterov (test_fused_optimizer_steps_full_size_vs_oracle's reference), one
    entry per step: (routed gradient, weights, momentum buffer)."""
    p = torch.nn.Parameter(w.clone())
    opt = torch.optim.SGD([p], lr=1e-2, momentum=0.9, nesterov=True)
    out = []
    for grad in grads:
        routed, _ = ops.route_grads(grad.numpy(), p.detach().numpy(), owner.numpy(), CUR, WD)
        p.grad = torch.from_numpy(routed)
        opt.step()
        if zero:
            with torch.no_grad():
                p.copy_(torch.from_numpy(ops.zero_pruned(p.detach().numpy(), owner.numpy())))
        out.append((p.grad.clone(), p.detach().clone(), opt.state[p]['momentum_buffer'].clone()))
    return out


def _near(got, want, rel, what):
    """|got - want| <= rel * max|want|, the bars of test_fused_optimizer_steps_full_size_vs_oracle."""
    got = got.cpu()
    assert float((got - want).abs().max()) <= rel * float(want.abs().max() + 1e-30), what


@pytest.mark.parametrize('zero', [False, True], ids=['sgd', 'sgd-zero'])
def test_sgd_route_step_guarded(zero):
    """cpg_sgd_route_step / cpg_sgd_route_zero_step at every size, two steps each (the first allocates the state and must not read the
    NaN the buffer holds), then the same layers through one cpg_sgd_route_(zero_)step_multi table: bit-equal to the per-layer calls."""
    entry = 'cpg_sgd_route_zero_step' if zero else 'cpg_sgd_route_step'
    with guarding() as led:
        per_layer, rows, keep = [], [], []
        for n in ELEMENTWISE_SIZES:
            g, w, owner, _ = _elementwise_inputs(n, 1)
            grads = [torch.randn(n, generator=g) * 1e-3 for _ in range(2)]
            want = _sgd_oracle(w, owner, grads, zero)
            do = BUF.put(owner)
            dw, mom = BUF.copy(w), BUF.empty((n,))
            mw, mmom, mgs = BUF.copy(w), BUF.empty((n,)), []
            for step, grad in enumerate(grads):
                dg = BUF.copy(grad)
                L.call(entry, _ptr(dw), _ptr(dg), _ptr(mom), _ptr(do), CUR, WD, 1e-2, 0.9, 1, int(step == 0), n, L.stream_ptr())
                rg, rw, rm = want[step]
                assert torch.equal(dg.cpu() == 0, rg == 0), (n, step)                  # the routing decision, bit-exact
                _near(dg, rg, 1e-6, ('grad', n, step))
                _near(dw, rw, 2e-6, ('w', n, step))
                _near(mom, rm, 2e-6, ('momentum', n, step))
                if zero:
                    assert not bool(dw[do == 0].any())
                mgs.append(BUF.copy(grad))
                keep.append(dg)
            per_layer.append((dw, mom, keep[-2:]))
            rows.append((mw, mmom, mgs, do, n))
        for step in range(2):
            items = (L.SgdItem * len(rows))(*[(w_.data_ptr(), gs[step].data_ptr(), m_.data_ptr(), o_.data_ptr(), n_) for w_, m_, gs, o_, n_ in rows])
            L.call(entry + '_multi', items, len(rows), CUR, WD, 1e-2, 0.9, 1, int(step == 0), L.stream_ptr())
        for (dw, mom, dgs), (mw, mmom, mgs, _, n) in zip(per_layer, rows):
            assert torch.equal(dw, mw) and torch.equal(mom, mmom) and all(torch.equal(a, b) for a, b in zip(dgs, mgs)), n
        finish(led, [t for dw, mom, dgs in per_layer for t in (dw, mom)] + [r[0] for r in rows], asked_workspace=False)


@pytest.mark.parametrize('mode', ['finetune', 'prune'])
def test_adam_route_step_guarded(mode):
    """cpg_adam_route_step at every size, two steps, against the oracle's routing + torch-CPU Adam; then cpg_adam_route_step_multi."""
    md = L.MODE_PRUNE if mode == 'prune' else L.MODE_FINETUNE
    with guarding() as led:
        per_layer, rows = [], []
        for n in ELEMENTWISE_SIZES:
            g, _, owner, pmv = _elementwise_inputs(n, 2)
            grads = [torch.randn(n, generator=g) * 1e-3 for _ in range(2)]
            p = torch.nn.Parameter(pmv.clone())
            opt = torch.optim.Adam([p], lr=5e-4)
            do = BUF.put(owner)
            dp, m1, m2 = BUF.copy(pmv), BUF.zeros((n,)), BUF.zeros((n,))
            mp, mm1, mm2, mgs = BUF.copy(pmv), BUF.zeros((n,)), BUF.zeros((n,)), []
            for step, grad in enumerate(grads):
                _, routed = ops.route_grads(grad.numpy(), grad.numpy(), owner.numpy(), CUR, 0.0, gpm=grad.numpy(), mode=mode)
                p.grad = torch.from_numpy(routed)
                opt.step()
                dg = BUF.copy(grad)
                L.call('cpg_adam_route_step', _ptr(dp), _ptr(dg), _ptr(m1), _ptr(m2), _ptr(do), CUR, md, 5e-4, 0.9, 0.999, 1e-8, step + 1, n,
                       L.stream_ptr())
                assert torch.equal(dg.cpu() == 0, p.grad == 0), (n, step)
                _near(dg, p.grad, 1e-6, ('grad', n, step))
                _near(dp, p.detach(), 2e-6, ('pm', n, step))
                mgs.append(BUF.copy(grad))
            for got, key in ((m1, 'exp_avg'), (m2, 'exp_avg_sq')):
                _near(got, opt.state[p][key], 2e-6, (key, n))
            if mode == 'prune':                         # every piggymask gradient is zeroed: Adam's state stays 0, nothing moves
                assert not bool(m1.any()) and torch.equal(dp.cpu(), pmv)
            per_layer.append((dp, m1, m2))
            rows.append((mp, mgs, mm1, mm2, do, n))
        for step in range(2):
            items = (L.AdamItem * len(rows))(*[(p_.data_ptr(), gs[step].data_ptr(), a_.data_ptr(), b_.data_ptr(), o_.data_ptr(), n_)
                                               for p_, gs, a_, b_, o_, n_ in rows])
            L.call('cpg_adam_route_step_multi', items, len(rows), CUR, md, 5e-4, 0.9, 0.999, 1e-8, step + 1, L.stream_ptr())
        for (dp, m1, m2), (mp, _, mm1, mm2, _, n) in zip(per_layer, rows):
            assert torch.equal(dp, mp) and torch.equal(m1, mm1) and torch.equal(m2, mm2), n
        finish(led, [t for row in per_layer for t in row], asked_workspace=False)


@pytest.mark.parametrize('n', ELEMENTWISE_SIZES)
def test_mask_ops_guarded(n):
    """apply_mask, claim_free, zero_pruned and mask_hist, the tensors themselves guarded, against the oracle bit for bit."""
    _, w, owner, pm = _elementwise_inputs(n, 3)
    s = L.stream_ptr()
    with guarding() as led:
        do = BUF.put(owner)
        for idx in (2, 3):
            dw = BUF.copy(w)
            L.call('cpg_apply_mask', _ptr(dw), _ptr(do), idx, n, s)
            np.testing.assert_array_equal(dw.cpu().numpy(), ops.apply_mask(w.numpy(), owner.numpy(), idx))
        dz = BUF.copy(w)
        L.call('cpg_zero_pruned', _ptr(dz), _ptr(do), n, s)
        np.testing.assert_array_equal(dz.cpu().numpy(), ops.zero_pruned(w.numpy(), owner.numpy()))
        dc = BUF.copy(owner)
        L.call('cpg_claim_free', _ptr(dc), 4, n, s)
        np.testing.assert_array_equal(dc.cpu().numpy(), ops.claim_free(owner.numpy(), 4))
        hist = BUF.zeros((257,), torch.int64)
        L.call('cpg_mask_hist', _ptr(do), _ptr(BUF.put(pm)), CUR, n, _ptr(hist), s)
        np.testing.assert_array_equal(hist[:256].cpu().numpy(), np.bincount(owner.numpy(), minlength=256))
        shared = (owner.numpy() > 0) & (owner.numpy() < CUR) & (pm.numpy() > np.float32(0.005))
        assert int(hist[256]) == int(shared.sum())
        hist2 = BUF.zeros((257,), torch.int64)                                       # without a piggymask: the owner counts alone
        L.call('cpg_mask_hist', _ptr(do), None, CUR, n, _ptr(hist2), s)
        assert torch.equal(hist2[:256], hist[:256]) and int(hist2[256]) == 0
        finish(led, [dw, dz, dc, hist, hist2], asked_workspace=False)


@pytest.mark.parametrize('select', [0, 1])
@pytest.mark.parametrize('n', [1, 3, 1023, 1025])
def test_pack_unpack_guarded(n, select):
    assert n in PC.PACK_UNPACK_SIZES
    with guarding() as led:
        finish(led, PC.gradient_pack_unpack_equals_boolean_indexing(n, select, buf=BUF), asked_workspace=False)


@pytest.mark.parametrize('zero', [False, True], ids=['rank-prune', 'rank-prune-zero'])
@pytest.mark.parametrize('n', [1, 3, 1025, 70001])
def test_rank_prune_guarded(n, zero):
    """The 32-byte result record, the workspace, the owner bytes (and, for the zeroing form, the weights) all between guards."""
    g = torch.Generator().manual_seed(n)
    w = torch.randn(n, generator=g) * 0.05
    owner = torch.randint(0, 3, (n,), generator=g, dtype=torch.uint8)
    owner[0] = 1                                        # at least one candidate: k = round(0.7 * candidates) >= 1
    with guarding() as led:
        outs = PC.rank_prune_vs_oracle(w, owner, 1, 0.7, buf=BUF, zero=zero)
        assert led.arena_of(outs[1]).nbytes == L.PRUNE_RESULT_BYTES == 32
        assert led.arena_of(outs[2]).nbytes == (int(L.lib().cpg_rank_prune_workspace_bytes()) + 3) // 4 * 4
        finish(led, outs)
