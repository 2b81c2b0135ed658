"""The descriptor-space table and sampler of tests/_conv_space_cases.py without a GPU: that they are what they claim, that the
tolerances of the GPU body are attainable by a plain float32 convolution with room to spare, what the planner queries answer on
every near miss of a fast class (needs the built library, launches nothing), and what the entry points refuse."""
import collections
import ctypes

import pytest
import torch

import _conv_space_cases as CS
import cpg_amd._lib as L

SWEEP = CS.sweep_cases()
UNSUPPORTED = -2
ONE = ctypes.c_void_p(16)           # a non-null pointer nothing reads: the refused calls return before anything is launched
BYTES = 1 << 20


# --------------------------------------------------------------------------- the table and the sampler are what they claim
def test_table_ids_limits_and_outputs():
    ids = [c.id for c in CS.SPACE_CASES]
    assert len(set(ids)) == len(ids)
    for c in CS.SPACE_CASES:
        OH, OW = CS.out_hw(c)
        assert OH >= 1 and OW >= 1, c.id
        # (80 output channels -- the pointwise kernels' other tile, K > 64 -- is the one width beyond the limit, on pointwise rows only)
        wide_pw = c.cls == 'pointwise' and c.K == 80 and c.C <= CS.LIMIT_CH
        assert c.N <= CS.LIMIT_N and (max(c.C, c.K) <= CS.LIMIT_CH or wide_pw) and max(c.H, c.W) <= CS.LIMIT_MAP, c.id
        assert c.C % c.G == 0 and c.K % c.G == 0, c.id
        assert set(c.plan) <= set(CS.PLAN_KEYS), c.id
    assert len(CS.SPACE_CASES) >= 75


def test_table_gives_every_class_a_bias_and_a_piggymask():
    for cls in {c.cls for c in CS.SPACE_CASES}:
        rows = [c for c in CS.SPACE_CASES if c.cls == cls]
        assert any(c.bias for c in rows) and any(c.pm for c in rows) and any(not c.bias and not c.pm for c in rows), cls


def test_table_holds_the_rows_it_was_built_for():
    """The geometry each block of the table is about, restated from the descriptors (a row edited away from its branch fails here)."""
    by = CS.CASE_BY_ID
    # a misroute of a near miss would land on the fast kernel: Winograd's channel counts and even maps; the stems' 3 -> 64
    for c in CS.SPACE_CASES:
        if c.id.startswith(('n3-', 'ns2-')) and c.id != 'ns2-c8':
            assert c.C >= 16 and c.K >= 16 and c.C % 4 == 0 and c.K % 4 == 0 and c.H % 2 == 0 and c.W % 2 == 0, c.id
        if c.id.startswith(('nv-', 'nst-')) and c.id != 'nst-7c4':
            assert c.C <= 3 and c.K == 64, c.id
        if c.cls == 'pointwise':
            assert c.C % 16 == 0 and c.K % 16 == 0 and (c.R, c.S) == (1, 1), c.id
    pw = [c for c in CS.SPACE_CASES if c.cls == 'pointwise']
    assert {(c.sh, c.sw) for c in pw} >= {(2, 1), (1, 2), (3, 2)} and {(c.ph, c.pw) for c in pw} >= {(1, 1), (0, 1)}
    assert any(c.K <= 64 for c in pw) and any(c.K == 80 for c in pw) and {(c.H, c.W) for c in pw} == {(12, 12), (15, 14)}
    # the generic input gradient: a residue class without taps (rho >= R), h_start >= H, strided + dilated
    c = by['dg-k23-s31']
    assert c.sh > c.R and c.sw == 1
    c = by['dg-s4-2x3']
    assert ((0 - c.ph) % c.sh) >= c.H
    assert all(by[i].sh * by[i].sw > 1 and by[i].dh * by[i].dw > 1 for i in ('dg-s2d2', 'dg-s21-d12'))
    # degenerate geometry: outputs that see padding only, kernel extents beyond the map, one output
    for cid in ('dz-p3', 'dz-k5-3x3', 'dz-k7d2-9x9', 'pw-p11', 'pw-p01-k80'):
        assert bool(CS.padding_only_mask(by[cid]).any()) == (cid in ('dz-p3', 'pw-p11', 'pw-p01-k80')), cid
    assert by['dz-k5-3x3'].R > by['dz-k5-3x3'].H and by['dz-k13-h1'].H == 1 and by['dz-k31-w1'].W == 1
    assert by['dz-k7d2-9x9'].dh * (by['dz-k7d2-9x9'].R - 1) + 1 > by['dz-k7d2-9x9'].H
    assert CS.out_hw(by['dz-keqmap']) == (1, 1) and (by['dz-keqmap'].ph, by['dz-keqmap'].pw) == (0, 0)
    # grouped: depthwise, multiplier 2, 16 and 15 channels per group
    assert by['g-dw3'].G == by['g-dw3'].C == by['g-dw3'].K and by['g-mult2'].K == 2 * by['g-mult2'].C == 2 * by['g-mult2'].G
    assert all(by[i].C // by[i].G == 16 and by[i].K // by[i].G == 16 for i in ('g16-s21', 'g16-k13', 'g16-p10')) and by['g15'].C // by['g15'].G == 15


def test_padding_only_mask_against_a_convolution_of_ones():
    """The mask computed from the descriptor is where a convolution of an all-ones map with an all-ones kernel gives 0."""
    for c in list(CS.SPACE_CASES) + SWEEP:
        seen = torch.nn.functional.conv2d(torch.ones(1, 1, c.H, c.W), torch.ones(1, 1, c.R, c.S), None, (c.sh, c.sw), (c.ph, c.pw), (c.dh, c.dw))
        assert torch.equal(CS.padding_only_mask(c), seen[0, 0] == 0), c.id


def test_sweep_strata_are_exact_and_every_draw_is_valid():
    assert len(SWEEP) == 160 and len({c.id for c in SWEEP}) == 160
    counts = collections.Counter(c.cls for c in SWEEP)
    assert [counts[s] for s in CS.STRATA] == CS.strata_counts(160) == [27, 27, 27, 27, 26, 26]
    assert CS.sweep_cases() == SWEEP                        # seeded
    for c in SWEEP:
        OH, OW = CS.out_hw(c)
        assert OH >= 1 and OW >= 1 and 1 <= c.N <= 3, c.id
        assert 1 <= c.R <= 7 and 1 <= c.S <= 7 and 1 <= c.sh <= 3 and 1 <= c.sw <= 3 and 1 <= c.dh <= 3 and 1 <= c.dw <= 3, c.id
        assert 0 <= c.ph <= c.dh * (c.R - 1) + 1 and 0 <= c.pw <= c.dw * (c.S - 1) + 1, c.id
        assert c.C % c.G == 0 and c.K % c.G == 0 and 1 <= c.C // c.G <= 40 and 1 <= c.K // c.G <= 40, c.id
    by = lambda s: [c for c in SWEEP if c.cls == s]         # noqa: E731
    assert all((c.R, c.S) == (3, 3) for c in by('3x3-like')) and all((c.R, c.S) == (1, 1) for c in by('1x1'))
    assert all(c.R != c.S for c in by('rect')) and all(c.sh * c.sw > 1 for c in by('strided'))
    assert all(c.dh * c.dw > 1 and min(c.R, c.S) >= 2 for c in by('dilated')) and all(c.G > 1 for c in by('grouped'))
    assert all(c.G == 1 for c in SWEEP if c.cls != 'grouped')
    # the sweep reaches what the table cannot list one by one
    assert any(bool(CS.padding_only_mask(c).any()) for c in SWEEP) and any(c.H == 1 or c.W == 1 for c in SWEEP)
    assert any(c.sh != c.sw for c in by('strided')) and any(c.dh != c.dw for c in by('dilated'))


# --------------------------------------------------------------------------- the yardstick is attainable
@pytest.mark.parametrize('c', list(CS.SPACE_CASES) + SWEEP, ids=lambda c: c.id)
def test_float32_reference_conv_meets_half_the_tolerance(c):
    """torch's float32 CPU convolution and its gradients stay within HALF of every tolerance the GPU body applies: the inputs are
    well conditioned, and the thresholds are not what a wrong kernel could hide behind."""
    ins, ref = CS.reference(c)
    got = CS.conv_and_grads(c, *ins, dtype=torch.float32)
    assert set(got) == set(ref)
    for name, (rtol, atol) in CS.tolerances(ref).items():
        if name in ref:
            err, ratio = CS.worst(got[name], ref[name], rtol / 2, atol / 2)
            assert ratio <= 1.0, (c.id, name, err, ratio)


# --------------------------------------------------------------------------- planner answers on the near misses
def _answers(c):
    lib, d = L.lib(), ctypes.byref(CS.desc_of(c))
    return collections.OrderedDict([
        ('wino0', lib.cpg_conv2d_winograd(d, 0)), ('wino1', lib.cpg_conv2d_winograd(d, 1)), ('wino2', lib.cpg_conv2d_winograd(d, 2)),
        ('wino3', lib.cpg_conv2d_winograd(d, 3)), ('bn_eval', lib.cpg_conv2d_fwd_bn_eval_supported(d)),
        ('bn_eval_add', lib.cpg_conv2d_fwd_bn_eval_add_supported(d)), ('prelu_eval0', lib.cpg_conv2d_fwd_prelu_eval_supported(d, 0)),
        ('prelu_eval1', lib.cpg_conv2d_fwd_prelu_eval_supported(d, 1)), ('dgrad_add', lib.cpg_conv2d_dgrad_add_supported(d)),
        ('rider', lib.cpg_conv2d_wgrad_rider_supported(d)), ('pool_max', lib.cpg_conv2d_fwd_pool_max_supported(d)),
        ('stem_bn', lib.cpg_stem_bn_supported(d)), ('bf16', lib.cpg_conv2d_bf16_supported(d)),
        ('wgrad_bf16', lib.cpg_conv2d_wgrad_bf16_supported(d)), ('bnstats_tiles', lib.cpg_conv2d_bnstats_tiles(d)),
        ('bnbwd_tiles', lib.cpg_conv2d_dgrad_bnbwd_tiles(d))])


@pytest.mark.parametrize('c', [c for c in CS.SPACE_CASES if c.cls in CS.NEAR_MISS_CLASSES + ('fast',)], ids=lambda c: c.id)
def test_planner_answers(c):
    """Every query answers what its class in include/cpg_hip.h says: 0 on a near miss, except where the table records that the
    near miss is legitimately still inside that query's class (a 1x1 with dilation or unequal strides)."""
    got = _answers(c)
    assert tuple(got) == CS.PLAN_KEYS
    for key, v in got.items():
        want = c.plan.get(key, 0)
        if want is True:
            assert v > 0, (c.id, key, v)
        else:
            assert v == want, (c.id, key, v, want)


def test_the_other_classes_of_the_table_have_no_fused_path():
    """Generic, degenerate and grouped rows: no query claims them."""
    for c in CS.SPACE_CASES:
        if c.cls not in CS.NEAR_MISS_CLASSES + ('fast',):
            assert not any(_answers(c).values()), (c.id, _answers(c))


# --------------------------------------------------------------------------- refusals
def _entry_points(d):
    """Every conv entry point on descriptor d with pointers nothing reads -> {name: status}."""
    lib, p = L.lib(), ctypes.byref(d)
    return {
        'fwd': lib.cpg_conv2d_fwd(p, ONE, ONE, None, 0.0, None, ONE, ONE, BYTES, None),
        'dgrad': lib.cpg_conv2d_dgrad(p, ONE, ONE, None, 0.0, ONE, ONE, BYTES, None),
        'wgrad': lib.cpg_conv2d_wgrad(p, ONE, ONE, ONE, None, 0.0, ONE, None, None, ONE, BYTES, None),
        'fwd_bnstats': lib.cpg_conv2d_fwd_bnstats(p, ONE, ONE, None, 0.0, None, ONE, ONE, BYTES, ONE, BYTES, None),
        'fwd_bn_eval': lib.cpg_conv2d_fwd_bn_eval(p, ONE, ONE, None, 0.0, None, ONE, ONE, ONE, ONE, 1e-5, 1, ONE, None, ONE, BYTES, None),
        'fwd_bn_eval_add': lib.cpg_conv2d_fwd_bn_eval_add(p, ONE, ONE, None, 0.0, None, ONE, ONE, ONE, ONE, 1e-5, ONE, 1, ONE, ONE, BYTES, None),
        'fwd_prelu_eval': lib.cpg_conv2d_fwd_prelu_eval(p, ONE, ONE, None, 0.0, None, ONE, 1, None, ONE, None, ONE, BYTES, None),
        'dgrad_bnbwd': lib.cpg_conv2d_dgrad_bnbwd(p, ONE, ONE, None, 0.0, ONE, ONE, ONE, ONE, ONE, ONE, ONE, BYTES, ONE, BYTES, None),
    }


def _bad_descriptors():
    base = CS.CASE_BY_ID['n3-p00']
    out = {}
    for name, kw in (('empty-oh', dict(H=2, ph=0)), ('empty-ow', dict(W=1, pw=0, S=3)), ('empty-dilated', dict(dh=4, dw=4, ph=0, pw=0)),
                     ('groups-not-dividing-c', dict(G=3, K=18)), ('groups-not-dividing-k', dict(G=4, K=18)), ('groups-zero', dict(G=0)),
                     ('zero-stride', dict(sh=0)), ('negative-pad', dict(pw=-1))):
        out[name] = base._replace(**kw)
    return out


@pytest.mark.parametrize('name', sorted(_bad_descriptors()))
def test_refusals(name):
    """An empty output, or groups that do not divide C and K: CPG_E_INVALID from every entry point, 0 bytes from the workspace query,
    0 from every planner query."""
    c = _bad_descriptors()[name]
    if name.startswith('empty'):
        assert min(CS.out_hw(c)) <= 0
    d = CS.desc_of(c)
    # This file also runs where there is a GPU, and the pointers below are fakes (device memory cannot be faked from the host): an
    # entry point that stopped validating would launch on address 16.  So the two queries that launch nothing and share make_geom's
    # verdict go first and fail cleanly; the calls are made only once they agree that the descriptor is refused.
    assert L.lib().cpg_conv2d_workspace_bytes(ctypes.byref(d)) == 0
    assert L.lib().cpg_conv2d_fwd_bn_eval_supported(ctypes.byref(d)) == 0 and L.lib().cpg_conv2d_pack_bytes(ctypes.byref(d), 0) == 0
    for entry, rc in _entry_points(d).items():
        assert rc == L.CPG_E_INVALID, (name, entry, rc, L.lib().cpg_last_error())
    assert not any(_answers(c).values()), _answers(c)
