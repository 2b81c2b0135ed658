"""The guard-band harness (tests/_guarded.py) proves itself on CPU tensors: layout, detection of writes on either side of a payload,
frozen inputs, and the interposer on stand-in modules.  A careless kernel is played by a torch write into the arena itself, so the
write stays inside the allocation."""
import types

import numpy as np
import pytest
import torch

import _guarded as G
from _guarded import GUARD_BYTES, Ledger, guarded, guarding

CPU = torch.device('cpu')


def _arena(ledger, t):
    a = ledger.arena_of(t)
    assert a is not None and a.payload is None
    return a


# --------------------------------------------------------------------------- layout
@pytest.mark.parametrize('shape,dtype', [((3, 5), torch.float32), ((7,), torch.float32), ((4097,), torch.uint8), ((2, 2), torch.int64),
                                         ((), torch.float32)])
def test_layout(shape, dtype):
    led = Ledger()
    t = led.guarded(shape, dtype, CPU)
    a = _arena(led, t)
    nbytes = int(np.prod(shape, dtype=np.int64)) * t.element_size()
    assert GUARD_BYTES == 64 * 1024 and GUARD_BYTES % 512 == 0
    assert t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.dtype == dtype
    off = t.storage_offset() * t.element_size()
    assert t.data_ptr() - a.raw.data_ptr() == off == GUARD_BYTES and off % 512 == 0                       # payload offset: the front guard, a multiple of 512
    assert a.nbytes == nbytes and t.numel() * t.element_size() == nbytes
    assert a.raw.numel() == 2 * GUARD_BYTES + (nbytes + 3) // 4 * 4    # exact size, rounded to the 4 bytes _lib.workspace rounds to
    assert a.raw.numel() - off - nbytes - GUARD_BYTES in (0, 1, 2, 3)
    raw = a.raw.numpy()
    pat = np.frombuffer(np.array([G.GUARD_WORD], dtype='<i4').tobytes(), dtype=np.uint8)
    assert (pat != 0).all()                                            # works behind uint8 owner tensors too
    assert np.isnan(np.array([G.GUARD_WORD], dtype='<i4').view('<f4')[0]) and (G.GUARD_WORD >> 22) & 1      # a quiet NaN as fp32
    assert np.isnan(np.array([G.EMPTY_WORD], dtype='<i4').view('<f4')[0]) and G.EMPTY_WORD != G.GUARD_WORD
    assert (raw[:GUARD_BYTES].reshape(-1, 4) == pat).all()
    assert (raw[off + nbytes:] == np.tile(pat, GUARD_BYTES // 4 + 1)[(nbytes % 4 or 4):]).all()
    assert led.check() == [] and led.owns(t) and not led.owns(torch.zeros(3))
    assert led.holds(t) and led.holds(t.clone()) and not led.holds(torch.zeros(shape, dtype=dtype))
    assert not led.owns(led.guarded((0,), dtype, CPU)) and led.check() == []       # no elements: nothing to own, guards all the same


def test_payload_contents():
    led = Ledger()
    e = led.guarded((5, 3), torch.float32, CPU)
    assert bool(torch.isnan(e).all())                                  # "empty": all NaN, and not the guards' NaN
    assert (e.view(torch.int32) == G.EMPTY_WORD).all()
    z = led.guarded((5, 3), torch.float32, CPU, zero=True)
    assert (z.view(torch.int32) == 0).all()
    o = led.guarded((9,), torch.uint8, CPU)
    assert (o != 0).all()
    src = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    c = led.guarded((5, 3), torch.float32, CPU, init=src)
    assert torch.equal(c, src) and c.data_ptr() != src.data_ptr()
    with pytest.raises(ValueError):
        led.guarded((5, 3), torch.float32, CPU, init=src.reshape(3, 5))
    led.verify()


# --------------------------------------------------------------------------- detection
def test_a_write_inside_the_payload_passes():
    led = Ledger()
    t = led.guarded((4, 6), torch.float32, CPU)
    t.fill_(3.0)
    t[3, 5] = float('nan')
    u = led.guarded((4097,), torch.uint8, CPU)
    u.fill_(0)
    led.verify()


def test_one_element_before_the_payload():
    led = Ledger()
    t = led.guarded((4, 6), torch.float32, CPU, label='victim')
    a = _arena(led, t)
    a.raw[GUARD_BYTES - 4: GUARD_BYTES].view(torch.float32)[0] = 1.0
    (v,) = led.check()
    assert v == G.Violation('victim', (4, 6), 'front', -4, 4)
    with pytest.raises(G.GuardViolation) as e:
        led.verify()
    assert 'victim' in str(e.value) and 'front' in str(e.value) and 'payload-4' in str(e.value)


def test_one_element_after_the_payload():
    led = Ledger()
    t = led.guarded((4, 6), torch.float32, CPU, label='victim')
    a = _arena(led, t)
    a.raw[GUARD_BYTES + 96: GUARD_BYTES + 100].view(torch.float32)[0] = 0.0
    (v,) = led.check()
    assert v == G.Violation('victim', (4, 6), 'back', 96, 4)


def test_one_byte_after_a_byte_payload_that_ends_inside_a_word():
    led = Ledger()
    t = led.guarded((4097,), torch.uint8, CPU, label='owner')         # 4k + 1
    a = _arena(led, t)
    t.fill_(2)                                                         # the payload itself may be written, to its last byte
    assert led.check() == []
    a.raw[GUARD_BYTES + 4097] = 0
    (v,) = led.check()
    assert v == G.Violation('owner', (4097,), 'back', 4097, 1)


def test_the_last_byte_of_the_back_guard():
    led = Ledger()
    t = led.guarded((10,), torch.float32, CPU, label='far')
    a = _arena(led, t)
    a.raw[-1] = 0
    (v,) = led.check()
    assert v == G.Violation('far', (10,), 'back', 40 + GUARD_BYTES - 1, 1)
    led2 = Ledger()
    t2 = led2.guarded((10,), torch.float32, CPU, label='near')
    _arena(led2, t2).raw[0] = 0                                        # and the first byte of the front guard
    (v2,) = led2.check()
    assert v2 == G.Violation('near', (10,), 'front', -GUARD_BYTES, 1)


def test_both_sides_and_several_arenas_are_all_reported():
    led = Ledger()
    a = _arena(led, led.guarded((3,), torch.float32, CPU, label='a'))
    led.guarded((3,), torch.float32, CPU, label='clean')
    b = _arena(led, led.guarded((3,), torch.float32, CPU, label='b'))
    a.raw[GUARD_BYTES - 1] = 0
    a.raw[GUARD_BYTES + 12: GUARD_BYTES + 20] = 0
    b.raw[GUARD_BYTES + 13] = 0
    got = led.check()
    assert got == [G.Violation('a', (3,), 'front', -1, 1), G.Violation('a', (3,), 'back', 12, 8), G.Violation('b', (3,), 'back', 13, 1)]


def test_the_call_site_labels_an_unnamed_buffer():
    led = Ledger()
    t = led.guarded((3,), torch.float32, CPU)
    assert _arena(led, t).label.startswith('tests/test_guarded_host.py:')


# --------------------------------------------------------------------------- frozen inputs
def test_one_changed_bit_of_a_frozen_input_is_reported():
    led = Ledger()
    src = torch.randn(6, 7)
    t = led.guarded((6, 7), torch.float32, CPU, init=src, frozen=True, label='x')
    free = led.guarded((6, 7), torch.float32, CPU, init=src, label='y')
    led.verify()
    free.view(torch.int32)[2, 3] ^= 1                                  # not frozen: may change
    led.verify()
    t.view(torch.int32)[2, 3] ^= 1 << 9
    (v,) = led.check()
    assert v == G.Violation('x', (6, 7), 'payload', (2 * 7 + 3) * 4 + 1, 1)
    nan = led.guarded((2,), torch.float32, CPU, init=torch.tensor([float('nan'), 1.0]), frozen=True, label='nan')
    assert len(led.check()) == 1                                       # a NaN that stayed the same NaN is unchanged (bits, not values)
    nan.view(torch.int32)[0] ^= 1
    assert [w.label for w in led.check()] == ['x', 'nan']


# --------------------------------------------------------------------------- interposer, on CPU stand-ins
def _stand_in(name):
    m = types.ModuleType(name)
    m.torch = torch
    exec('def make(n, like):\n'
         '    a = torch.empty((n, 3), dtype=torch.float32, device=like.device)\n'
         '    b = torch.empty_like(like)\n'
         '    c = torch.zeros(n, dtype=torch.int64, device=like.device)\n'
         '    d = torch.zeros_like(like, memory_format=torch.contiguous_format)\n'
         '    return a, b, c, d\n'
         'def odd(like):\n'
         '    return torch.empty(4, device=like.device, pin_memory=False), torch.empty_like(like.t()), torch.ones(3)\n'
         'def workspace(nbytes, device):\n'
         '    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device), (nbytes + 3) // 4 * 4\n'
         'def use_workspace(n):\n'
         '    import sys\n'
         '    return sys.modules[__name__].workspace(n, "cpu")\n', m.__dict__)
    return m


def test_interposer_guards_the_patched_modules_allocations_and_only_those():
    import sys
    mod, other, bind = _stand_in('_guarded_stand_in'), _stand_in('_guarded_other'), _stand_in('_guarded_binding')
    sys.modules[bind.__name__] = bind
    try:
        like = torch.randn(4, 5)
        orig_ws = bind.workspace
        with guarding(modules=[mod], binding=bind, device_types=('cpu',)) as led:
            assert G.active() is led
            outs = mod.make(6, like)
            assert all(led.owns(t) for t in outs) and led.intercepted == 4
            a, b, c, d = outs
            assert a.shape == (6, 3) and b.shape == like.shape and c.dtype == torch.int64 and d.dtype == torch.float32
            assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()) and not c.any() and not d.any()
            assert not any(led.owns(t) for t in other.make(6, like))          # from elsewhere: torch's own
            assert not led.owns(torch.empty(3)) and led.intercepted == 4
            ws, nb = bind.use_workspace(10)
            assert led.owns(ws) and nb == 12 and ws.numel() == 3 and led.workspaces == 1 and bool(torch.isnan(ws).all())
            assert led.arena_of(ws).nbytes == 12 and bind.use_workspace(0) == (None, 0)
            assert led.original_workspace_calls == 0
            orig_ws(8, 'cpu')                                                  # a kept reference to the old allocator is noticed
            assert led.original_workspace_calls == 1
            assert led.passed_through == []
            odd = mod.odd(like)                                                # an unknown keyword, a non-contiguous model: untouched, counted
            assert not any(led.owns(t) for t in odd) and [f for _, f in led.passed_through] == ['empty', 'empty_like']
            assert odd[1].shape == (5, 4)
            inp = guarded((4, 5), torch.float32, CPU, init=like, frozen=True)  # the free function lands in the enclosing block's ledger
            assert led.owns(inp)
            led.verify()
            led.arena_of(b).raw[GUARD_BYTES + 80] = 0
            with pytest.raises(G.GuardViolation) as e:
                led.verify()
            assert 'empty_like @' in str(e.value) and e.value.violations[0].side == 'back' and e.value.violations[0].offset == 80
        assert mod.torch is torch and bind.torch is torch and bind.workspace is orig_ws and G.active() is None
        assert not Ledger().owns(mod.make(2, like)[0])
    finally:
        del sys.modules[bind.__name__]


def test_interposer_restores_after_an_exception_and_nests():
    mod = _stand_in('_guarded_stand_in2')
    like = torch.randn(2, 2)
    with pytest.raises(KeyError):
        with guarding(modules=[mod], binding=None, device_types=('cpu',)):
            assert mod.torch is not torch
            raise KeyError('boom')
    assert mod.torch is torch and G.active() is None
    with guarding(modules=[mod], binding=None, device_types=('cpu',)) as outer:
        with guarding(modules=[mod], binding=None, device_types=('cpu',)) as inner:
            t = mod.make(1, like)[0]
            assert inner.owns(t) and not outer.owns(t)
        assert outer.owns(mod.make(1, like)[0])
    assert mod.torch is torch
    with pytest.raises(RuntimeError):
        guarded((2,), torch.float32, CPU)                              # no enclosing block, no ledger given


def test_the_real_modules_are_patched_and_restored_without_a_gpu():
    import importlib
    mods = [importlib.import_module(n) for n in G.PATCHED_MODULES]
    from cpg_amd import _lib
    ws = _lib.workspace
    with guarding() as led:
        assert all(type(m.torch).__name__ == '_TorchProxy' for m in mods) and _lib.workspace is not ws
        # a host-side allocation of a patched module (a layer's Parameter) is none of the interposer's business
        from cpg_amd.models import layers as nl
        layer = nl.SharableLinear(5, 3)
        assert not led.owns(layer.weight) and led.passed_through == [] and led.intercepted == 0
    assert all(m.torch is torch for m in mods) and _lib.workspace is ws and _lib.torch is torch
