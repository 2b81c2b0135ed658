"""Guard bands round the buffers a kernel is handed, and an interposer that puts the Python mirror's own allocations into them.

Every GPU test compares the tensor a kernel was asked to fill with a reference; none looks at the bytes on either side of it, and
none controls what a workspace holds on entry.  Here a buffer is a window into a private arena

    [ front guard, 64 KiB | payload, exactly the bytes asked for (rounded up to 4 only) | back guard, 64 KiB ]

whose guards hold a fixed 32-bit pattern (a quiet NaN as fp32, every byte non-zero) and whose payload holds a copy of `init`,
zeros, or a second NaN pattern for "uninitialised".  `Ledger.verify()` compares every guard bit for bit, and the payload of every
`frozen` (const) input with what it was made from.  A guard is a multiple of 512 bytes, so the payload keeps the alignment torch's
caching allocator gives in production and no kernel's choice of a vector or scalar path changes.

Inside `with guarding() as ledger:` the mirror's allocations are intercepted in two places: `cpg_amd._lib.workspace` (the one
workspace allocator of the binding) and the module global `torch` of the modules that allocate outputs, which becomes a forwarding
proxy whose empty / empty_like / zeros / zeros_like come from the ledger.  Calls the proxy does not understand pass through and
are counted.  Everything is put back on exit.

Known limit: a stray access further than 64 KiB from its buffer is not seen.

No GPU is needed to import this module or to test it (tests/test_guarded_host.py runs it on CPU tensors)."""
import collections
import contextlib
import importlib
import os
import sys

import numpy as np
import pytest
import torch

GUARD_BYTES = 64 * 1024
GUARD_WORD = 0x7FC5A371         # fp32: quiet NaN; bytes 71 A3 C5 7F, none zero
EMPTY_WORD = 0x7FE6B2D9         # another quiet NaN: what an "uninitialised" payload holds on entry
_GUARD_LE = np.frombuffer(np.array([GUARD_WORD], dtype='<i4').tobytes(), dtype=np.uint8)

PATCHED_MODULES = ('cpg_amd.models.layers', 'cpg_amd.models.fused_bn', 'cpg_amd.models.losses', 'cpg_amd.utils.pruner_base',
                   'cpg_amd.utils.prune', 'cpg_amd.utils.fused_sgd', 'cpg_amd.utils.packnet_prune')

Violation = collections.namedtuple('Violation', 'label shape side offset nbytes')
# side: 'front' | 'back' | 'payload' (a frozen input that changed); offset: first differing byte, relative to the payload's first byte
# (negative in the front guard, >= the payload's size in the back guard); nbytes: how many bytes differ on that side


class GuardViolation(AssertionError):
    def __init__(self, violations):
        self.violations = list(violations)
        super().__init__('%d guarded region(s) were written:\n' % len(self.violations) + '\n'.join(
            '  %s shape %s: %s, first byte at payload%+d, %d byte(s) differ' % (v.label, tuple(v.shape), v.side, v.offset, v.nbytes)
            for v in self.violations))


def _itemsize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _call_site(skip_files):
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) in skip_files:
        f = f.f_back
    if f is None:
        return '?'
    return '%s:%d' % (os.path.relpath(f.f_code.co_filename, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), f.f_lineno)


_THIS = {os.path.abspath(__file__)}


class Arena(object):
    """One guarded buffer.  `raw` is the whole arena as bytes (tests of the harness write into it to play a careless kernel);
    the payload tensor goes to whoever asked for the buffer."""

    def __init__(self, shape, dtype, device, init, zero, frozen, label):
        shape = tuple(int(s) for s in shape)
        self.shape, self.dtype, self.label = shape, dtype, label
        isz = _itemsize(dtype)
        numel = 1
        for s in shape:
            numel *= s
        self.nbytes = numel * isz
        self.padded = (self.nbytes + 3) // 4 * 4
        words = torch.empty((2 * GUARD_BYTES + self.padded) // 4, dtype=torch.int32, device=device)
        words.fill_(GUARD_WORD)
        self.words = words
        self.raw = words.view(torch.uint8)
        strides, st = [], 1
        for s in reversed(shape):
            strides.append(st)
            st *= max(s, 1)
        # set_ on the arena's storage: the payload is an ordinary tensor to autograd (no view bookkeeping), as an allocator's would be
        # (and the arena keeps no reference to it: autograd takes over a gradient buffer only when nobody else holds the tensor)
        t = torch.empty(0, dtype=dtype, device=device).set_(words.untyped_storage(), GUARD_BYTES // isz, shape, tuple(reversed(strides)))
        if init is not None:
            if tuple(init.shape) != shape or init.dtype != dtype:
                raise ValueError('guarded: init is %s %s, asked for %s %s' % (tuple(init.shape), init.dtype, shape, dtype))
            t.copy_(init)
        elif zero:
            t.zero_()
        elif self.nbytes:
            body = self.words[GUARD_BYTES // 4: (GUARD_BYTES + self.nbytes) // 4]
            body.fill_(EMPTY_WORD)
            tail = self.nbytes % 4              # a byte payload that ends inside a word: its last 1..3 bytes, non-zero like the rest
            if tail:
                self.raw[GUARD_BYTES + self.nbytes - tail: GUARD_BYTES + self.nbytes].fill_(0xD9)
        self.frozen = self.payload_bytes().clone() if frozen else None
        self.payload = t                    # handed to the caller by Ledger.guarded, then dropped

    def payload_bytes(self):
        return self.raw[GUARD_BYTES: GUARD_BYTES + self.nbytes]

    def owns(self, ptr):
        lo = self.raw.data_ptr() + GUARD_BYTES
        return lo <= ptr < lo + max(self.nbytes, 1)

    def _side(self, side, lo, hi, want):
        """Bytes [lo, hi) of the arena against `want` (numpy bytes), after the cheap word compare on the device said they differ."""
        got = self.raw[lo:hi].cpu().numpy()
        bad = np.flatnonzero(got != want)
        return Violation(self.label, self.shape, side, int(bad[0]) + lo - GUARD_BYTES, int(bad.size))

    def check(self):
        out = []
        gw = GUARD_BYTES // 4
        if bool((self.words[:gw] != GUARD_WORD).any()):
            out.append(self._side('front', 0, GUARD_BYTES, np.tile(_GUARD_LE, gw)))
        back_lo = GUARD_BYTES + self.nbytes
        pad = self.padded - self.nbytes
        dirty = bool((self.words[(GUARD_BYTES + self.padded) // 4:] != GUARD_WORD).any())
        if pad and not dirty:
            dirty = not np.array_equal(self.raw[back_lo: back_lo + pad].cpu().numpy(), _GUARD_LE[4 - pad:])
        if dirty:
            out.append(self._side('back', back_lo, 2 * GUARD_BYTES + self.padded, np.tile(_GUARD_LE, gw + 1)[4 - pad if pad else 4:]))
        if self.frozen is not None and not torch.equal(self.payload_bytes(), self.frozen):
            out.append(self._side('payload', GUARD_BYTES, GUARD_BYTES + self.nbytes, self.frozen.cpu().numpy()))
        return out


class Ledger(object):
    def __init__(self):
        self.arenas = []
        self.workspace_requests = 0         # calls of the interposed _lib.workspace, those for 0 bytes (no buffer) included
        self.workspaces = 0                 # guarded workspaces handed out by the interposed _lib.workspace
        self.original_workspace_calls = 0   # allocations the binding's own workspace() made while it should have been replaced
        self.intercepted = 0                # allocations of the patched modules that came back guarded
        self.passed_through = []            # (call site, function) of calls the proxy did not understand

    def guarded(self, shape, dtype, device, init=None, label=None, zero=False, frozen=False):
        if isinstance(shape, int):
            shape = (shape,)
        a = Arena(shape, dtype, torch.device(device), init, zero, frozen, label or _call_site(_THIS))
        self.arenas.append(a)
        t, a.payload = a.payload, None
        return t

    def arena_of(self, t):
        p = t.data_ptr()                    # (0 for a tensor of no elements: nobody owns those)
        for a in reversed(self.arenas):
            if p and a.owns(p):
                return a
        return None

    def owns(self, t):
        return isinstance(t, torch.Tensor) and self.arena_of(t) is not None

    def holds(self, t):
        """`t` lies in a payload, or is a bit-for-bit copy of one of its own shape and type (a gradient autograd chose to copy
        out of the buffer the kernel wrote)."""
        if self.owns(t):
            return True
        if not isinstance(t, torch.Tensor) or not t.numel():
            return False
        b = t.detach().contiguous().reshape(-1).view(torch.uint8)
        return any(a.dtype == t.dtype and a.shape == tuple(t.shape) and a.raw.device == t.device and torch.equal(a.payload_bytes(), b)
                   for a in self.arenas)

    def check(self):
        """Synchronise, then every violation of every arena (empty list: nothing outside a payload, and no frozen payload, changed)."""
        if any(a.raw.is_cuda for a in self.arenas):
            torch.cuda.synchronize()
        out = []
        for a in self.arenas:
            out.extend(a.check())
        return out

    def verify(self):
        bad = self.check()
        if bad:
            raise GuardViolation(bad)


_ACTIVE = []


def active():
    return _ACTIVE[-1] if _ACTIVE else None


def guarded(shape, dtype, device, init=None, label=None, zero=False, frozen=False, ledger=None):
    """A contiguous tensor of exactly this shape between two guards, registered with `ledger` (default: the enclosing guarding()
    block's).  Payload: a copy of `init`, zeros (zero=True), or NaN.  frozen=True: verify() also holds the payload to `init`."""
    ledger = ledger or active()
    if ledger is None:
        raise RuntimeError('guarded() outside a guarding() block needs ledger=')
    return ledger.guarded(shape, dtype, device, init=init, label=label or _call_site(_THIS), zero=zero, frozen=frozen)


def frozen_copy(t, device=None, label=None):
    """`t` (any device) as a guarded, frozen tensor on `device`: how a test hands a kernel a const argument."""
    t = t.detach()
    return guarded(t.shape, t.dtype, device or t.device, init=t.contiguous(), label=label or _call_site(_THIS), frozen=True)


class GuardedBuffers(object):
    """The buffer factory of the shared test bodies (tests/_parity_cases.py: PlainBuffers) with every buffer in the enclosing
    guarding() block's ledger: const inputs frozen, outputs and scratch between guards."""
    guarded = True

    def __init__(self, device='cuda:0'):
        self.device = torch.device(device)

    def put(self, t, offset=0):
        if t is None:
            return None
        t = t.detach()
        if not offset:
            return guarded(t.shape, t.dtype, self.device, init=t.contiguous(), label='input @ ' + _call_site(_THIS), frozen=True)
        flat = torch.cat([torch.zeros(offset, dtype=t.dtype, device=t.device), t.reshape(-1)])
        whole = guarded(flat.shape, t.dtype, self.device, init=flat, label='input+%d @ %s' % (offset, _call_site(_THIS)), frozen=True)
        return whole[offset:].view(t.shape)

    def copy(self, t):
        t = t.detach()
        return guarded(t.shape, t.dtype, self.device, init=t.contiguous(), label='in-place @ ' + _call_site(_THIS))

    def full(self, shape, value, dtype=torch.float32):
        shape = tuple(shape)
        return guarded(shape, dtype, self.device, init=torch.full(shape, value, dtype=dtype, device=self.device),
                       label='full(%r) @ %s' % (value, _call_site(_THIS)))

    def empty(self, shape, dtype=torch.float32):
        return guarded(tuple(shape), dtype, self.device, label='empty @ ' + _call_site(_THIS))

    def zeros(self, shape, dtype=torch.float32):
        return guarded(tuple(shape), dtype, self.device, zero=True, label='zeros @ ' + _call_site(_THIS))

    def rehome(self, module, const_buffers=False):
        """Every parameter of `module` into a frozen guarded buffer (no body steps an optimizer), every buffer (running statistics)
        into a guarded one, frozen where the mode makes it an input only."""
        for name, p in module.named_parameters():
            p.data = guarded(p.shape, p.dtype, self.device, init=p.data.contiguous(), label='parameter ' + name, frozen=True)
        for name, b in module.named_buffers():
            b.data = guarded(b.shape, b.dtype, self.device, init=b.data.contiguous(), label='buffer ' + name, frozen=const_buffers)
        return module


class _TorchProxy(object):
    """Stands in for the module global `torch` of one patched module: everything forwards to torch except the four allocating
    functions, which come from the ledger when the request is one the proxy understands (a dense, contiguous tensor on a guarded
    device type)."""

    def __init__(self, ledger, device_types):
        object.__setattr__(self, '_ledger', ledger)
        object.__setattr__(self, '_types', tuple(device_types))

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    def _through(self, fn, args, kw):
        self._ledger.passed_through.append((_call_site(_THIS), fn.__name__))
        return fn(*args, **kw)

    def _new(self, fn, zero, args, kw):
        kw2 = dict(kw)
        dtype = kw2.pop('dtype', None) or torch.get_default_dtype()
        device = kw2.pop('device', None)
        mf = kw2.pop('memory_format', torch.contiguous_format)
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            shape = tuple(args[0])
        else:
            shape = tuple(args)
        device = torch.device(device) if device is not None else torch.device('cpu')
        if device.type not in self._types:
            return fn(*args, **kw)                # not a device allocation (a Parameter made on the host, say): none of our business
        if kw2 or mf != torch.contiguous_format or not all(isinstance(s, int) and s >= 0 for s in shape):
            return self._through(fn, args, kw)
        self._ledger.intercepted += 1
        return self._ledger.guarded(shape, dtype, device, zero=zero, label='%s @ %s' % (fn.__name__, _call_site(_THIS)))

    def _like(self, fn, zero, args, kw):
        kw2 = dict(kw)
        mf = kw2.pop('memory_format', torch.preserve_format)
        dtype = kw2.pop('dtype', None)
        if len(args) != 1 or not isinstance(args[0], torch.Tensor):
            return self._through(fn, args, kw)
        t = args[0]
        if t.device.type not in self._types:
            return fn(*args, **kw)
        if kw2 or t.layout != torch.strided or (mf != torch.contiguous_format and not (mf == torch.preserve_format and t.is_contiguous())):
            return self._through(fn, args, kw)
        self._ledger.intercepted += 1
        return self._ledger.guarded(tuple(t.shape), dtype or t.dtype, t.device, zero=zero, label='%s @ %s' % (fn.__name__, _call_site(_THIS)))

    def empty(self, *args, **kw):
        return self._new(torch.empty, False, args, kw)

    def zeros(self, *args, **kw):
        return self._new(torch.zeros, True, args, kw)

    def empty_like(self, *args, **kw):
        return self._like(torch.empty_like, False, args, kw)

    def zeros_like(self, *args, **kw):
        return self._like(torch.zeros_like, True, args, kw)


class _CountingTorch(object):
    """The binding's own `torch` while its workspace() is replaced: an allocation from there means something kept a reference to the
    original allocator."""

    def __init__(self, ledger):
        object.__setattr__(self, '_ledger', ledger)

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kw):
        self._ledger.original_workspace_calls += 1
        return torch.empty(*args, **kw)


@contextlib.contextmanager
def guarding(modules=PATCHED_MODULES, binding='cpg_amd._lib', device_types=('cuda',)):
    """Route the allocations of `modules` (names or module objects) and the workspaces of `binding` (None: leave it) through a new
    Ledger for the duration of the block."""
    ledger = Ledger()
    mp = pytest.MonkeyPatch()
    _ACTIVE.append(ledger)
    try:
        proxy = _TorchProxy(ledger, device_types)
        for m in modules:
            m = importlib.import_module(m) if isinstance(m, str) else m
            mp.setattr(m, 'torch', proxy)
        if binding is not None:
            b = importlib.import_module(binding) if isinstance(binding, str) else binding

            def workspace(nbytes, device):
                ledger.workspace_requests += 1
                if nbytes == 0:
                    return None, 0
                buf = ledger.guarded(((nbytes + 3) // 4,), torch.float32, device, label='workspace(%d) @ %s' % (nbytes, _call_site(_THIS)))
                ledger.workspaces += 1
                return buf, buf.numel() * 4

            mp.setattr(b, 'workspace', workspace)
            mp.setattr(b, 'torch', _CountingTorch(ledger))
        yield ledger
    finally:
        _ACTIVE.pop()
        mp.undo()
