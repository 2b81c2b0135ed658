"""Step telemetry and the divergence guard (no counterpart in the reference, which trains blind: a run whose loss went non-finite
reports chance accuracy, and the task loop reads that as "capacity exhausted" and widens the network for good).

The fused optimizer passes stream every masked weight, its routed gradient, its momentum and every piggymask through one kernel per
step.  Their STATS twins (include/cpg_hip.h: cpg_sgd_route_step_multi_stats, cpg_sgd_route_zero_step_multi_stats,
cpg_adam_route_step_multi_stats) perform the same update bit for bit and reduce, in the same pass, one record per layer and a sticky
health record -- all on the device, deterministically, without a synchronisation.  OPT-IN: an optimizer of utils.fused_sgd given
`telemetry=StepTelemetry()` calls the twins; nothing here is touched otherwise.

    tel = StepTelemetry()
    opt = MaskedSGD(params, pruner=pruner, lr=1e-2, telemetry=tel)
    ... loss.backward(); pruner.do_weight_decay_and_make_grads_zero(); opt.step() ...
    tel.read()      # {layer: {'g_norm': ..., 'update_ratio': ..., ...}} of the last step   (the only call that waits for the GPU
    tel.check()     # raises TrainingDiverged(step, layer, kind) once a step went non-finite  besides health() / check())
"""
import ctypes
import math

import torch

from .. import _lib

SGD_FIELDS = ('n_routed', 'g_nonfinite', 'g_sumsq', 'g_absmax', 'w_nonfinite', 'dw_sumsq', 'w_sumsq', 'w_absmax')      # cpg_sgd_step_stats
PM_FIELDS = ('n_routed', 'g_sumsq', 'g_absmax', 'dpm_sumsq', 'flips_on', 'flips_off', 'picked', 'pm_nonfinite')        # cpg_pm_step_stats
_COUNTS = frozenset(('n_routed', 'pm_n_routed', 'g_nonfinite', 'w_nonfinite', 'flips_on', 'flips_off', 'picked', 'pm_nonfinite'))      # integers
# a layer's weight record keeps the header's field names; its piggymask record carries 'pm_' where the two would collide
_PM_KEYS = tuple(f if f in ('dpm_sumsq', 'flips_on', 'flips_off', 'picked', 'pm_nonfinite') else 'pm_' + f for f in PM_FIELDS)
PICK_THRESHOLD = 5e-3            # the Binarizer's default threshold (models/layers.py), the literal of calculate_shared_part_ratio
KIND_GRADIENT, KIND_VALUE = 1, 2
_KIND_TEXT = {KIND_GRADIENT: 'a non-finite routed gradient', KIND_VALUE: 'a non-finite weight or piggymask after the step'}


class TrainingDiverged(RuntimeError):
    """A step left a non-finite routed gradient (kind 1) or a non-finite weight / piggymask (kind 2) in `layer` at optimizer step `step`."""

    def __init__(self, step, layer, kind):
        super().__init__('training diverged at step %d in %s: %s (kind %d)' % (step, layer, _KIND_TEXT.get(kind, 'unknown'), kind))
        self.step, self.layer, self.kind = step, layer, kind


class _Tables(object):
    """The device tables of ONE optimizer: a record per row of the last step's calls, the partials workspace, and a health record per
    call slot (a step is one call per (param group, first-step) batch -- one in every flow of this package --, or one call per layer
    under CPG_MULTI_TENSOR=0; a slot's item index is relative to its call, `offsets` puts it back into the step's row order)."""

    def __init__(self, kind):
        self.kind = kind                     # 'sgd' | 'pm'
        self.step = 0                        # 1-based count of this optimizer's steps
        self.stats = self.partials = self.health = None
        self.names = []                      # layer name per row of the last step
        self.idle = []                       # piggymasks of the last step that took MaskedAdam's idle shortcut (no kernel ran)
        self.slots = {}                      # slot key -> row of `health`
        self.offsets = {}                    # slot key -> (first row of its last call, the names of that call)

    def begin(self):
        self.step += 1
        self.names, self.idle = [], []

    def _grow(self, t, rows, cols, dtype, device, keep):
        if t is not None and t.shape[0] >= rows:
            return t
        new = torch.zeros(max(rows, 2 * (t.shape[0] if t is not None else 0)), cols, dtype=dtype, device=device)
        if t is not None and keep:
            new[:t.shape[0]].copy_(t)
        return new

    def call(self, entry, table, rows, names, args_before, args_after, slot, device):
        """One _stats call: `rows` of (pointers..., n) with their layer names; entry(table, len, *args_before, step, stats, partials,
        bytes, health, *args_after)."""
        first = len(self.names)
        ns = (ctypes.c_int64 * len(rows))(*[r[-1] for r in rows])
        need = int(_lib.lib().cpg_step_stats_workspace_bytes(ns, len(rows)))
        self.stats = self._grow(self.stats, first + len(rows), len(SGD_FIELDS), torch.float64, device, keep=True)
        self.partials = self._grow(self.partials, max(need // 64, 1), 8, torch.float64, device, keep=False)
        if slot not in self.slots:
            self.slots[slot] = len(self.slots)
        self.health = self._grow(self.health, len(self.slots), 4, torch.int64, device, keep=True)
        self.offsets[slot] = (first, list(names))
        self.names.extend(names)
        _lib.call(entry, table, len(rows), *args_before, self.step, ctypes.c_void_p(self.stats.data_ptr() + 64 * first),
                  ctypes.c_void_p(self.partials.data_ptr()), self.partials.numel() * 8,
                  ctypes.c_void_p(self.health.data_ptr() + 32 * self.slots[slot]), *args_after)

    def read(self):
        fields = SGD_FIELDS if self.kind == 'sgd' else _PM_KEYS
        out = {}
        if self.names:
            for name, row in zip(self.names, self.stats[:len(self.names)].cpu().tolist()):
                out[name] = {f: int(v) if f in _COUNTS else v for f, v in zip(fields, row)}
        for name in self.idle:
            out[name] = {f: 0 if f in _COUNTS else 0.0 for f in fields}
        return out

    def read_health(self):
        """(first_bad_step, layer, kind, bad_steps) merged over the slots, or None while every step was clean."""
        if self.health is None:
            return None
        rows = self.health[:len(self.slots)].cpu().tolist()
        best, bad_steps = None, 0
        for slot, at in self.slots.items():
            step, item, kind, bad = rows[at]
            bad_steps = max(bad_steps, bad)
            if step == 0:
                continue
            first, names = self.offsets[slot]
            key = (step, first + item)
            if best is None or key < best[0]:
                best = (key, names[item] if item < len(names) else '#%d' % item, kind)
        return None if best is None else (best[0][0], best[1], best[2], bad_steps)


class StepTelemetry(object):
    """Owns the device tables (sized on first use, reused afterwards), one set per optimizer it is attached to, and maps rows to layer
    names.  `thr`: the threshold of the piggymask flip / picked counts."""

    def __init__(self, thr=PICK_THRESHOLD):
        self.thr = float(thr)
        self._tables = {}                    # id(optimizer) -> _Tables, in attachment order (SGD before Adam)

    def tables(self, optimizer, kind):
        t = self._tables.get(id(optimizer))
        if t is None:
            t = self._tables[id(optimizer)] = _Tables(kind)
            t.owner = optimizer              # (kept alive with its tables: an id is unique only among live objects)
        return t

    def attach(self, optimizers):
        """Give this object to every optimizer of `optimizers` (an utils.Optimizers, or an iterable) that can feed it."""
        for opt in getattr(optimizers, 'optimizers', optimizers):
            if hasattr(opt, 'telemetry'):
                opt.telemetry = self
        return self

    def read(self):
        """{layer: {field: value}} of every optimizer's LAST step -- the header's fields (a piggymask's n_routed / g_sumsq / g_absmax as
        pm_n_routed / ...), and derived: g_norm = sqrt(g_sumsq), update_ratio = sqrt(dw_sumsq / w_sumsq) (None for all-zero weights),
        pm_g_norm, flips = flips_on + flips_off, picked_ratio = picked / pm_n_routed (None where no slot is kept: task 1, prune mode).
        Waits for the GPU."""
        out = {}
        for t in self._tables.values():
            for name, rec in t.read().items():
                out.setdefault(name, {}).update(rec)
        for rec in out.values():
            if 'g_sumsq' in rec:
                rec['g_norm'] = math.sqrt(rec['g_sumsq'])
                rec['update_ratio'] = math.sqrt(rec['dw_sumsq'] / rec['w_sumsq']) if rec['w_sumsq'] > 0 else None
            if 'picked' in rec:
                rec['pm_g_norm'] = math.sqrt(rec['pm_g_sumsq'])
                rec['flips'] = rec['flips_on'] + rec['flips_off']
                rec['picked_ratio'] = rec['picked'] / rec['pm_n_routed'] if rec['pm_n_routed'] else None
        return out

    def health(self):
        """The sticky record: {'first_bad_step', 'layer', 'kind', 'bad_steps'} of the earliest bad step any attached optimizer saw (the
        weight optimizer's before the piggymask optimizer's within one step), or the all-zero record {0, None, 0, 0}.  Waits for the GPU."""
        found = [h for h in (t.read_health() for t in self._tables.values()) if h is not None]
        if not found:
            return {'first_bad_step': 0, 'layer': None, 'kind': 0, 'bad_steps': 0}
        step, layer, kind, _ = min(found, key=lambda h: h[0])
        return {'first_bad_step': step, 'layer': layer, 'kind': kind, 'bad_steps': max(h[3] for h in found)}

    def check(self):
        h = self.health()
        if h['first_bad_step']:
            raise TrainingDiverged(h['first_bad_step'], h['layer'], h['kind'])
