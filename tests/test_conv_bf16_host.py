"""tests/_bf16_cases.py without a GPU: the table against the selection predicates of csrc/conv3x3_bf16.hip, the oracle against itself
(the fp32 emulation sits well inside the a-priori bound; three wrong kernels sit further from it than any admissible M), and the
planner and the refusals of the six bf16 entry points, which launch nothing."""
import ctypes

import pytest
import torch

import _bf16_cases as B

ROW_IDS = list(B.ROWS)


# --------------------------------------------------------------------------- the table
def _fwd_passes(row, math):
    """(configuration, channels read, channels produced) of the forward and of the input gradient."""
    N, C, H, W, K = B.ROWS[row]
    return [(B.fwd_config(math, K, H, W), C, K), (B.fwd_config(math, C, H, W), K, C)]


def _edges(row):
    """What the row's last column in the issue's table says it reaches, as predicates on the restated plans."""
    N, C, H, W, K = B.ROWS[row]
    F, G = B.FWD_CFG, B.WG_CFG
    f16, fx3 = B.fwd_config('bf16', K, H, W), B.fwd_config('bf16x3', K, H, W)
    d16 = B.fwd_config('bf16', C, H, W)
    g16 = G[B.wgrad_config('bf16', W)]
    unit_cols = [min(g16.TW, W - u * g16.TW) for u in range(B._ceil(W, g16.TW))]          # valid columns per unit of a row
    masked = [(u, c % 8) for u, c in enumerate(unit_cols) if c % 8]                       # (unit, valid pixels of its straddling group)
    return {
        'a': [H % F[f16].TH != 0, C % 16 != 0, F[fx3].BM == 64 and B._ceil(K, 64) == 2, g16.TW == 64 and unit_cols == [56]],
        'b': [H < F[f16].TH, g16.TW == 64 and unit_cols == [64, 48]],
        'c': [f16 == 'B16S16' and H == F[f16].TH - 1 and W == F[f16].TW - 2],
        'd': [d16 == 'B16N128' and W <= 16 and H == 15 and H % 7 != 0],
        'e': [B._ceil(K, F[f16].BM) == 2 and K % F[f16].BM == 8, g16.MASKW and masked == [(0, 4)] and len(unit_cols) == 1],
        'f': [B._ceil(C, 64) == 3 and C % 64 == 8],
        'g': [B._ceil(C, 16) == 1, W % F[f16].TW == 5, masked == [(1, 5)]],
        'h': [W > 56 and W % 8 != 0 and g16.MASKW and masked == [(1, 4)], C % 64 == 1 and C % 16 == 1],
        'i': [W % 8 == 0 and W % 56 != 0 and g16.TW == 64 and not g16.MASKW, H == g16.TH],
        'j': [all(B.wplan(B.wgrad_config(m, W), N, C, H, W, K)['nsplit'] > B.wplan(B.wgrad_config(m, W), N, C, H, W, K)['units'] for m in B.MATHS)],
    }[row]


def test_the_rows_reach_every_configuration_and_edge():
    fwd_seen, wg_seen = set(), set()
    for row in B.ROWS:
        N, C, H, W, K = B.ROWS[row]
        (f, d, g) = B.CLAIMS[row]
        for i, math in enumerate(B.MATHS):
            got = _fwd_passes(row, math)
            assert (got[0][0], got[1][0]) == (f[i], d[i]), (row, math, got)
            wg = B.wgrad_config(math, W)
            assert wg == ('B16', 'X3')[i] + g, (row, math, wg)
            fwd_seen.update(c for c, _, _ in got)
            wg_seen.add(wg)
        assert all(_edges(row)), (row, _edges(row))
    assert fwd_seen == set(B.FWD_CFG) and len(fwd_seen) == 10
    assert wg_seen == set(B.WG_CFG) and len(wg_seen) == 6
    # the two weight-gradient cases no earlier test ran (tests/test_hip_parity.py has W in 9, 11, 14, 28, 37, 56, 112, 224 only)
    assert any(B.wgrad_config('bf16', r[3]) == 'B16G64' and r[3] % 64 and r[3] != 56 for r in B.ROWS.values())
    assert any(B.wgrad_config('bf16', r[3]) == 'B16G32' and r[3] > 56 and r[3] % 8 for r in B.ROWS.values())


# --------------------------------------------------------------------------- the oracle against itself
@pytest.mark.parametrize('variant', B.VARIANTS)
@pytest.mark.parametrize('row', ROW_IDS)
def test_oracle_self_checks(row, variant):
    """On every row, math and tensor: the fp32 emulation meets the a-priori bound with r <= 1/4, and each wrong kernel is more than
    64 times the emulation's r from the model, so no admissible M hides it."""
    ref = B.reference(row, variant)
    ins = ref['in']
    N, C, H, W, K = B.ROWS[row]
    for math in B.MATHS:
        m = ref[math]
        mutants = {'drop' if math == 'bf16x3' else 'trunc': B.arithmetic(math, *ins, dt=torch.float32, mutant='drop' if math == 'bf16x3' else 'trunc'),
                   'tail': B.tail_mutant(math, *ins)}
        assert set(mutants['tail']) == {n for n, t in (('y', C % 16), ('gx', K % 16)) if t}
        for name in m.model:
            r_emu, hard = B.ratios(m.emu[name], m, name)
            print('row %s %s %s %s: emulation r %.3e (%.3e of the bound)' % (row, variant, math, name, r_emu, hard))
            assert 0 < r_emu <= 0.25 and hard <= 0.25, (row, variant, math, name, r_emu, hard)
            hit = 0
            for kind, res in mutants.items():
                if name in res:
                    r_mut, _ = B.ratios(res[name], m, name)
                    print('row %s %s %s %s: mutant %s r %.3e = %.1f x emulation' % (row, variant, math, name, kind, r_mut, r_mut / r_emu))
                    assert r_mut > B.M_CAP * r_emu, (row, variant, math, name, kind, r_mut, r_emu)
                    hit += 1
            assert hit >= 1
    assert B.M <= B.M_CAP and B.M & (B.M - 1) == 0


def test_the_tail_mutant_is_defined_where_the_table_says_there_is_a_tail():
    """Rows a, b, c, e, f, h have a channel tail in the forward's last chunk, rows a, b, d, e, f, g in the input gradient's."""
    assert [r for r, v in B.ROWS.items() if v[1] % 16] == ['a', 'b', 'c', 'e', 'f', 'h']
    assert [r for r, v in B.ROWS.items() if v[4] % 16] == ['a', 'b', 'd', 'e', 'f', 'g']


# --------------------------------------------------------------------------- planner and refusals (nothing is launched)
CPG_E_INVALID, CPG_E_UNSUPPORTED, CPG_E_WORKSPACE = -1, -2, -3
UNSUPPORTED = [dict(C=15), dict(K=15), dict(stride_h=2, stride_w=2), dict(pad_h=0, pad_w=0), dict(dil_h=2, dil_w=2), dict(groups=2)]


@pytest.fixture(scope='module')
def lib():
    from cpg_amd import _lib
    return _lib.lib()


def _entry_calls(lib, d, ws, nb, nbw):
    """The six entry points on made-up tensor pointers: name -> status.  Every call made through here must be refused BEFORE anything
    is launched (the descriptor, the workspace's size and its alignment are checked first, in that order): the pointers are never
    dereferenced, on a machine with a GPU either.  Callers pass only arguments that one of those three checks refuses."""
    p = ctypes.c_void_p(0x10000)
    r = ctypes.byref(d)
    out = {}
    for sfx in ('', 'x3'):
        out['fwd_bf16' + sfx] = getattr(lib, 'cpg_conv2d_fwd_bf16' + sfx)(r, p, p, None, B.THR, None, p, ws, nb, None)
        out['dgrad_bf16' + sfx] = getattr(lib, 'cpg_conv2d_dgrad_bf16' + sfx)(r, p, p, None, B.THR, p, ws, nb, None)
        out['wgrad_bf16' + sfx] = getattr(lib, 'cpg_conv2d_wgrad_bf16' + sfx)(r, p, p, p, None, B.THR, p, None, ws, nbw, None)
    assert len(out) == 6
    return out


@pytest.mark.parametrize('row', ROW_IDS)
def test_planner_answers(row, lib):
    N, C, H, W, K = B.ROWS[row]
    d = B.desc_of(row)
    assert lib.cpg_conv2d_bf16_supported(ctypes.byref(d)) == 1 and lib.cpg_conv2d_wgrad_bf16_supported(ctypes.byref(d)) == 1
    nb, nbw = lib.cpg_conv2d_bf16_workspace_bytes(ctypes.byref(d)), lib.cpg_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d))
    need = max(B.pack_bytes(c_read, m, B.FWD_CFG[cfg].NP) for math in B.MATHS for cfg, c_read, m in _fwd_passes(row, math))
    needw = max(B.wplan(B.wgrad_config(math, W), N, C, H, W, K)['ws_bytes'] for math in B.MATHS)
    print('row %s: pack workspace %d (plans need %d), split-K workspace %d (plans need %d)' % (row, nb, need, nbw, needw))
    assert nb >= need and nbw >= needw
    assert nb == need and nbw == needw          # ... and no more: what the guard-band test hands out is what the kernels may use
    for over in UNSUPPORTED:
        d2 = B.desc_of(row, **over)
        if over == dict(groups=2) and (C % 2 or K % 2):
            d2 = B.desc_of(row, groups=2, C=C + C % 2, K=K + K % 2)
        assert lib.cpg_conv2d_bf16_supported(ctypes.byref(d2)) == 0 and lib.cpg_conv2d_wgrad_bf16_supported(ctypes.byref(d2)) == 0, over
        assert lib.cpg_conv2d_bf16_workspace_bytes(ctypes.byref(d2)) == 0 and lib.cpg_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d2)) == 0
        big = ctypes.c_void_p(0x20000)
        assert set(_entry_calls(lib, d2, big, 1 << 30, 1 << 30).values()) == {CPG_E_UNSUPPORTED}, over


@pytest.mark.parametrize('row', ROW_IDS)
def test_entry_points_refuse_a_short_or_misaligned_workspace(row, lib):
    d = B.desc_of(row)
    nb, nbw = lib.cpg_conv2d_bf16_workspace_bytes(ctypes.byref(d)), lib.cpg_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d))
    aligned, off4 = ctypes.c_void_p(0x20000), ctypes.c_void_p(0x20004)
    short = _entry_calls(lib, d, aligned, nb - 1, nbw - 1)
    assert set(short.values()) == {CPG_E_WORKSPACE}, short
    assert set(_entry_calls(lib, d, None, nb, nbw).values()) == {CPG_E_WORKSPACE}
    crooked = _entry_calls(lib, d, off4, nb, nbw)
    assert set(crooked.values()) == {CPG_E_INVALID}, crooked
