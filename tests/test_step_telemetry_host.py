"""Step telemetry without a GPU: the workspace query against its arithmetic, every refusal of the three _stats entry points (made-up
pointers: all of these calls return before anything is launched), the ABI triple with the new symbols in it, and the numpy
restatement of the two records (tests/_step_stats.py) against itself."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _step_stats as S

CPG_E_INVALID, CPG_E_WORKSPACE = -1, -3
SGD_ENTRIES = ('cpg_sgd_route_step_multi_stats', 'cpg_sgd_route_zero_step_multi_stats')
ADAM_ENTRY = 'cpg_adam_route_step_multi_stats'
ENTRIES = SGD_ENTRIES + (ADAM_ENTRY,)
NEW_SYMBOLS = ENTRIES + ('cpg_step_stats_workspace_bytes',)


@pytest.fixture(scope='module')
def L():
    from cpg_amd import _lib
    _lib.lib()
    return _lib


def _query(L, ns):
    arr = (ctypes.c_int64 * len(ns))(*ns) if ns else None
    return L.lib().cpg_step_stats_workspace_bytes(arr, len(ns))


# --------------------------------------------------------------------------- the workspace query
SIZES = [0, 1, 4095, 4096, 4097, 3 * 4096 + 7]


@pytest.mark.parametrize('n', SIZES)
def test_workspace_query_of_one_row(L, n):
    assert _query(L, [n]) == S.workspace_bytes([n]) == 64 * ((n + 4095) // 4096)


def test_workspace_query_of_tables(L):
    assert _query(L, []) == 0 and _query(L, [0, 0, 0]) == 0
    assert _query(L, SIZES) == S.workspace_bytes(SIZES) == 64 * (0 + 1 + 1 + 1 + 2 + 4)
    mixed = [0, 5, 0, 4097, 1 << 20, 0, 1300001, 1, 0]
    assert _query(L, mixed) == S.workspace_bytes(mixed)
    long = list(range(0, 97 * 911, 911))                          # 97 rows: more than two launches' worth
    assert _query(L, long) == S.workspace_bytes(long)


# --------------------------------------------------------------------------- refusals (nothing is launched)
P, Q = 0x10000, 0x20000                                            # made-up device pointers, 16-byte aligned; never dereferenced
NS = [4097, 0, 5]
NEED = S.workspace_bytes(NS)


def _table(L, entry, ns=NS, spoil=None):
    adam = entry == ADAM_ENTRY
    rows = []
    for i, n in enumerate(ns):
        ptrs = [P + 64 * i if n else None] * (5 if adam else 4)
        if spoil == i:
            ptrs[1] = None
        rows.append(tuple(ptrs) + (n,))
    return ((L.AdamItem if adam else L.SgdItem) * len(rows))(*rows), len(rows)


def _call(L, entry, items=None, hyper=None, step=1, stats=Q, partials=Q + 4096, nbytes=NEED, health=Q + 8192):
    """One _stats entry point on made-up pointers: its status.  Callers pass only arguments that a check refuses."""
    table, n = items if items is not None else _table(L, entry)
    if hyper is None:
        hyper = (2, L.MODE_FINETUNE, 5e-4, 0.9, 0.999, 1e-8, 1, 5e-3) if entry == ADAM_ENTRY else (2, 4e-5, 1e-2, 0.9, 1, 0)
    return getattr(L.lib(), entry)(table, n, *hyper, step, stats, partials, nbytes, health, None)


@pytest.mark.parametrize('entry', ENTRIES)
def test_entry_points_refuse_before_they_launch(L, entry):
    assert NEED == 64 * 3
    # a partials buffer shorter than the query's answer
    assert _call(L, entry, nbytes=NEED - 1) == CPG_E_WORKSPACE
    assert _call(L, entry, nbytes=0) == CPG_E_WORKSPACE
    assert b'partials' in L.lib().cpg_last_error()
    # null or misaligned stats / partials, a null health, step < 1
    for kw in (dict(stats=None), dict(stats=Q + 8), dict(partials=None), dict(partials=Q + 4096 + 8), dict(partials=Q + 4), dict(health=None),
               dict(step=0), dict(step=-3)):
        assert _call(L, entry, **kw) == CPG_E_INVALID, kw
    # the empty table and the all-empty table need no workspace, and still a stats, a partials and a health pointer
    for ns in ([], [0, 0]):
        items = _table(L, entry, ns)
        assert _call(L, entry, items=items, nbytes=0, stats=None) == CPG_E_INVALID
        assert _call(L, entry, items=items, nbytes=0, health=None) == CPG_E_INVALID
    # the plain twin's checks: a bad row (after good ones), a negative n, a bad owner id, a negative count
    assert _call(L, entry, items=_table(L, entry, spoil=2)) == CPG_E_INVALID
    assert _call(L, entry, items=_table(L, entry, [5, -1])) == CPG_E_INVALID
    assert _call(L, entry, items=(None, 3)) == CPG_E_INVALID
    assert _call(L, entry, items=(_table(L, entry)[0], -1)) == CPG_E_INVALID
    if entry == ADAM_ENTRY:
        assert _call(L, entry, hyper=(256, L.MODE_FINETUNE, 5e-4, 0.9, 0.999, 1e-8, 1, 5e-3)) == CPG_E_INVALID
        assert _call(L, entry, hyper=(2, 7, 5e-4, 0.9, 0.999, 1e-8, 1, 5e-3)) == CPG_E_INVALID             # unknown mode
        assert _call(L, entry, hyper=(2, L.MODE_PRUNE, 5e-4, 0.9, 0.999, 1e-8, 0, 5e-3)) == CPG_E_INVALID    # Adam's own step count
    else:
        assert _call(L, entry, hyper=(256, 4e-5, 1e-2, 0.9, 1, 0)) == CPG_E_INVALID
    # a long table (three launches' worth) is sized as a whole: one byte short of it is refused
    ns = [4096 * (1 + i % 3) + i for i in range(97)]
    assert _call(L, entry, items=_table(L, entry, ns), nbytes=S.workspace_bytes(ns) - 1) == CPG_E_WORKSPACE


# --------------------------------------------------------------------------- the ABI triple
def test_abi_triple_holds_with_the_new_symbols(L):
    """Header == binding == exported symbols, slot by slot, through the suite's own checks; and the new names are in all three."""
    import test_abi_and_host as abi
    abi.test_library_exports_every_declared_symbol()
    header = open(os.path.join(abi.ROOT, 'include', 'cpg_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS and re.search(r'\b%s\(' % name, header) and hasattr(L.lib(), name)
    assert L.ABI_VERSION == L.lib().cpg_version() == 3
    for struct, fields in (('cpg_sgd_step_stats', S.SGD_FIELDS), ('cpg_pm_step_stats', S.PM_FIELDS)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), header, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', ' ', body, flags=re.S)
        assert tuple(re.findall(r'(\w+)\s*[,;]', body)) == fields and len(fields) * 8 == S.RECORD_BYTES


def test_library_still_exports_nothing_but_the_header():
    import test_abi_and_host as abi
    abi.test_library_exports_nothing_but_the_header()


def test_telemetry_tables_match_the_header():
    from cpg_amd.utils import telemetry as T
    assert T.SGD_FIELDS == S.SGD_FIELDS and T.PM_FIELDS == S.PM_FIELDS
    assert issubclass(T.TrainingDiverged, RuntimeError)
    e = T.TrainingDiverged(7, 'features.3', 1)
    assert (e.step, e.layer, e.kind) == (7, 'features.3', 1) and 'features.3' in str(e) and 'step 7' in str(e)


# --------------------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize('n', [1, 5, 4097, 3 * 4096 + 7])
@pytest.mark.parametrize('pattern', ['all', 'none', 'mixed'])
def test_restatement_meets_its_own_bound(n, pattern):
    """math.fsum against fp64 additions in index order on the GPU tests' inputs: the bound n * 2^-52 is attainable by a plain sum;
    counts, maxima and flips do not depend on how the sums are taken."""
    cur = 2
    w0, g1, w1 = S.values(n, 1, 0.05), S.values(n, 2, 0.05), S.values(n, 3, 0.05)
    owner = S.owners(n, pattern, cur, 4)
    a, b = S.sgd_record(w0, w1, g1, owner, cur), S.sgd_record(w0, w1, g1, owner, cur, total=S.plain)
    S.assert_record(b, a, n, 'sgd n=%d %s' % (n, pattern))
    assert a['n_routed'] == int((owner == cur).sum()) == (n if pattern == 'all' else 0 if pattern == 'none' else a['n_routed'])
    assert all(math.isfinite(v) for v in a.values())
    pm0, g = S.threshold_masks(n, 5e-3, 5)
    pm1 = (pm0 - np.float32(5e-4) * g).astype(np.float32)
    for mode in (S.MODE_FINETUNE, S.MODE_PRUNE):
        a = S.pm_record(pm0, pm1, g, owner, cur, mode, 5e-3)
        S.assert_record(S.pm_record(pm0, pm1, g, owner, cur, mode, 5e-3, total=S.plain), a, n, 'pm n=%d %s' % (n, pattern))
        kept = int(((owner != 0) & (owner < cur)).sum()) if mode == S.MODE_FINETUNE else 0
        assert a['n_routed'] == kept and a['flips_on'] + a['flips_off'] <= kept and a['picked'] <= kept
        if kept >= 64:
            assert a['flips_on'] > 0 and a['flips_off'] > 0 and 0 < a['picked'] < kept


def test_restatement_on_hand_made_values():
    f = np.float32
    w0 = np.array([1.0, np.nan, 2.0, 3e30, -0.0, np.inf], dtype=f)
    w1 = np.array([0.5, 1.0, np.nan, -3e30, 1e-45, 4.0], dtype=f)
    g1 = np.array([2.0, np.inf, 1e25, -3e30, 0.0, np.nan], dtype=f)
    owner = np.array([2, 2, 2, 2, 0, 1], dtype=np.uint8)
    r = S.sgd_record(w0, w1, g1, owner, 2)
    assert (r['n_routed'], r['g_nonfinite'], r['w_nonfinite']) == (4, 1, 1)
    assert r['g_absmax'] == float(f(3e30)) and r['w_absmax'] == float(f(3e30))
    assert r['g_sumsq'] == math.fsum(float(v) ** 2 for v in (f(2.0), f(1e25), f(-3e30)))         # finite although 9e60 overflows fp32
    assert r['dw_sumsq'] == math.fsum([0.25, (2.0 * float(f(3e30))) ** 2, float(f(1e-45)) ** 2])  # pairs with a NaN / Inf side are left out
    pm0 = np.array([5e-3, 5e-3, 6e-3, 4e-3, np.nan, 6e-3], dtype=f)
    pm1 = np.array([6e-3, 4e-3, 4e-3, np.nan, 6e-3, 7e-3], dtype=f)
    p = S.pm_record(pm0, pm1, g1, np.array([1, 1, 1, 1, 1, 3], dtype=np.uint8), 3, S.MODE_FINETUNE, 5e-3)
    assert (p['n_routed'], p['flips_on'], p['flips_off'], p['picked'], p['pm_nonfinite']) == (5, 2, 1, 2, 1)
