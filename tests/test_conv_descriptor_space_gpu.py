"""Every descriptor the conv entry points accept runs a kernel that computes THAT descriptor: the hand table and the seeded sweep of
tests/_conv_space_cases.py through SharableConv2d against torch's float64 conv2d and its autograd (the body and its tolerances live
there); the fused entry points on the near misses that are legitimately still inside their class (a 1x1 with unequal strides or with
dilation); and the same layers, and the linear layers, on pointers that are only element-aligned.

The fast families' own fused entry points on their own shapes (the `fast` rows of the table) are their own tests' business
(test_hip_parity.py, test_eval_*_gpu.py): no near miss answers non-zero to cpg_conv2d_dgrad_bnbwd_tiles, so that entry point has no
row here."""
import pytest
import torch

import _conv_space_cases as CS
import _eval_block_cases as EB
import _evalres as R
import _parity_cases as PC
from cpg_amd import _lib

pytestmark = pytest.mark.gpu
DEV = PC.DEV
SWEEP = CS.sweep_cases()


@pytest.mark.parametrize('cid', list(CS.CASE_BY_ID))
def test_space_table(cid):
    CS.conv_space(CS.CASE_BY_ID[cid])


@pytest.mark.parametrize('c', SWEEP, ids=lambda c: c.id)
def test_space_sweep(c):
    CS.conv_space(c)


# --------------------------------------------------------------------------- fused entry points on the legitimate non-zero answers
BN_EVAL_ROWS = [c.id for c in CS.SPACE_CASES if c.cls in CS.NEAR_MISS_CLASSES and c.plan.get('bn_eval')]
DGRAD_ADD_ROWS = [c.id for c in CS.SPACE_CASES if c.cls in CS.NEAR_MISS_CLASSES and c.plan.get('dgrad_add')]


def test_the_fused_rows_are_the_pointwise_near_misses():
    assert set(BN_EVAL_ROWS) == {c.id for c in CS.SPACE_CASES if c.cls == 'pointwise' and (c.ph, c.pw) == (0, 0)} and len(BN_EVAL_ROWS) == 7
    assert set(DGRAD_ADD_ROWS) == {'pw-d23', 'pw-d23-k80', 'pw-d21-k48'}
    assert all(CS.CASE_BY_ID[i].plan.get('bn_eval_add') and CS.CASE_BY_ID[i].plan.get('bnstats_tiles') for i in BN_EVAL_ROWS)
    # (cpg_conv2d_fwd_bnstats on these rows: the body of test_space_table, which holds the statistics to the float64 sums)
    assert not any(c.plan.get('bnbwd_tiles') for c in CS.SPACE_CASES if c.cls in CS.NEAR_MISS_CLASSES)


@pytest.mark.parametrize('cid', BN_EVAL_ROWS)
def test_space_fused_bn_eval(cid):
    """cpg_conv2d_fwd_bn_eval and cpg_conv2d_fwd_bn_eval_add on a 1x1 with unequal strides / dilation, as eval_block_case holds them on
    the isotropic shapes: the identity BatchNorm is the plain forward bit for bit; a general one stays inside the a-priori bound of
    tests/_evalres.py round the float64 reference."""
    c = CS.CASE_BY_ID[cid]
    d = CS.desc_of(c)
    (x, w, b, pm, _), ref = CS.reference(c)
    g = torch.Generator().manual_seed(len(cid) * 131 + c.K)
    bn = EB.make_bn(c.K, g)
    res = torch.randn(ref['y'].shape, generator=g)
    put = PC.PLAIN.put
    xd, wd, pd, bd, resd = put(x), put(w), put(pm), put(b), put(res)
    bnd = tuple(put(t) for t in bn)
    ident = tuple(put(t) for t in (torch.ones(c.K), torch.zeros(c.K), torch.zeros(c.K), torch.ones(c.K)))
    y0 = EB.run_fwd(d, xd, wd, pd, bd)
    PC.close(y0, ref['y'].numpy(), rtol=CS.RTOL, atol=CS.ATOL_Y, msg=cid)
    for relu in (0, 1):
        rc, y, st = EB.run_eval(d, xd, wd, pd, bd, ident, 0.0, relu)
        assert rc == 0 and st == [0, 0], (cid, _lib.lib().cpg_last_error(), st)
        assert EB._bits_equal(y, y0.clamp_min(0.0) if relu else y0), (cid, relu)
        rc, y, _ = EB.run_eval(d, xd, wd, pd, bd, ident, 0.0, relu, resd, add=True)
        assert rc == 0, (cid, _lib.lib().cpg_last_error())
        assert EB._bits_equal(y, (y0 + resd).clamp_min(0.0) if relu else y0 + resd), (cid, relu, 'add')
    parts = R.conv_parts(x, w, pm, (c.sh, c.sw), 0, CS.THR)
    for residual in (None, res):
        ref0, conv_term, shift_term = R.eval_res_terms(parts, b, *bn, EB.EPS, residual)
        for relu in (0, 1):
            rc, y, _ = EB.run_eval(d, xd, wd, pd, bd, bnd, EB.EPS, relu, resd if residual is not None else None, add=residual is not None)
            assert rc == 0, (cid, _lib.lib().cpg_last_error())
            want = ref0.clamp_min(0.0) if relu else ref0
            ratio = R.error_ratio(y.cpu(), want, conv_term, shift_term)
            print('%s relu=%d residual=%d: ratio %.4f' % (cid, relu, residual is not None, ratio))
            bad = ~((y.cpu().double() - want).abs() <= conv_term + shift_term)
            assert not bool(bad.any()), (cid, relu, residual is not None, int(bad.sum()), ratio)


@pytest.mark.parametrize('cid', DGRAD_ADD_ROWS)
def test_space_fused_dgrad_add(cid):
    """cpg_conv2d_dgrad_add on a dense 1x1 with dilation, by test_skip_gradient_in_the_input_gradient_epilogue's own body (the fused
    entry point really runs; y, gx, gw and gpm agree with the plain composition to 1e-6 of the scale); then the fused run against
    float64 at conv_oracle's bars, gx with the addend."""
    c = CS.CASE_BY_ID[cid]
    (x, w, b, pm, gy), ref = CS.reference(c)
    gs = torch.randn(x.shape, generator=torch.Generator().manual_seed(c.C + c.K))
    layer = CS.make_layer(c, w, b, pm, PC.PLAIN)
    fused = PC.skip_gradient_fused_equals_plain(layer, x.to(DEV), gy.to(DEV), gs.to(DEV))
    tol = CS.tolerances(ref)
    for name, got in zip(('y', 'gx', 'gw', 'gpm'), fused):
        want = ref[name] + gs.double() if name == 'gx' else ref[name]
        PC.close(got, want.numpy(), rtol=tol[name][0], atol=tol[name][1], msg='%s %s' % (cid, name))


# --------------------------------------------------------------------------- pointers that are only element-aligned
MIS_ROWS = [c.id for c in CS.SPACE_CASES if c.mis]


OUT_OFFSETS = (1, 3)


def test_the_misaligned_rows_cover_every_predicate_and_family():
    """What each `& 15` predicate needs in order to flip, restated from the code, and which of the two misaligned tests moves the pointer
    it looks at: test_space_table_misaligned moves x, gy, w, pm, bias; test_space_outputs_misplaced moves y, the statistics, gx, gw,
    gpm, gb."""
    rows = [CS.CASE_BY_ID[i] for i in MIS_ROWS]
    plane = lambda c: CS.out_hw(c)[0] * CS.out_hw(c)[1]          # noqa: E731
    fams = {c.id for c in rows if c.cls == 'fast'}
    assert fams == {'f-wino', 'f-direct', 'f-wino-wgrad', 'f-s2', 'f-vgg-stem', 'f-stem7', 'f-stem3'}
    pw = [c for c in rows if c.cls == 'pointwise' and (c.ph, c.pw) == (0, 0)]
    dense4 = [c for c in pw if (c.sh, c.sw) == (1, 1) and plane(c) % 4 == 0]
    # pointwise.hip pw_fwd_tile (x) and cpg_conv1x1_dgrad (gy): float4 <-> per-pixel staging needs a dense layer with 4 | plane, on the
    # narrow tile (K <= 64 forward, C <= 64 input gradient) and on the wide one -- jointly
    assert any(c.K <= 64 for c in dense4) and any(c.K > 64 for c in dense4) and any(c.C <= 64 for c in dense4)
    assert any(plane(c) % 4 for c in pw) and any(c.sh * c.sw > 1 for c in pw)                      # ... and rows that never take float4
    # igemm_conv.hip k_conv_bias_partial (gy): a bias and 4 | plane
    assert any(c.bias and c.bitexact and plane(c) % 4 == 0 for c in rows)
    # conv_grouped.hip launch_gd_ocb (`out`: y forward, gx input gradient): four outputs per lane from 16 columns, 4 | width, and the
    # OUTPUT off alignment -- only the direct calls of test_space_outputs_misplaced do that; template and run-time path
    wide = [c for c in rows if c.G > 1 and CS.out_hw(c)[1] >= 16 and CS.out_hw(c)[1] % 4 == 0 and c.W >= 16 and c.W % 4 == 0]
    assert any((c.R, c.S) == (3, 3) and (c.sh, c.sw, c.dh, c.dw) == (1, 1, 1, 1) for c in wide) and any((c.R, c.S) != (3, 3) for c in wide)
    assert all(off % 4 for off in OUT_OFFSETS)
    # fc_small.hip cpg_fc_small_dgrad_ok (w, pm through the layer; gx directly): <= 64 rows, 4 | in_features
    assert [s for s in CS.LINEAR_MISALIGNED if s[0] <= 64 and s[1] % 4 == 0] == FC_SMALL_SHAPES
    assert [v for v in CS.PLACEMENTS.values()] == [(1, 0), (0, 1), (3, 3)]


@pytest.mark.parametrize('place', list(CS.PLACEMENTS))
@pytest.mark.parametrize('cid', MIS_ROWS)
def test_space_table_misaligned(cid, place):
    """The body with the activations, the parameters or everything moved off 16-byte alignment (PlacedBuffers asserts
    data_ptr() % 16): the same float64 checks; the same bits as the aligned run where the route has no alignment predicate; and
    the aligned layer afterwards is bit-equal to itself before (no packed operand armed for the misplaced call survived it)."""
    c = CS.CASE_BY_ID[cid]
    act, _ = CS.PLACEMENTS[place]
    before, moved, after = {}, {}, {}
    CS.conv_space(c, named=before)
    CS.conv_space(c, place=place, named=moved)
    CS.conv_space(c, named=after)
    OH, OW = CS.out_hw(c)
    for name in before:
        assert torch.equal(before[name], after[name]), (cid, place, name, 'the aligned layer changed after the misplaced call')
        if c.bitexact and not (name == 'gb' and act and (OH * OW) % 4 == 0):
            assert torch.equal(before[name], moved[name]), (cid, place, name)


@pytest.mark.parametrize('place', list(CS.PLACEMENTS))
@pytest.mark.parametrize('pm', [False, True], ids=['w', 'pm'])
@pytest.mark.parametrize('B,I,O', CS.LINEAR_MISALIGNED)
def test_linear_misaligned(B, I, O, pm, place):
    """SharableLinear at the shapes that sit on fc_small.hip's and the pointwise GEMMs' alignment predicates, through linear_oracle's own
    checks."""
    PC.linear_oracle(B, I, O, pm, buf=CS.placed(place))


@pytest.mark.parametrize('off', OUT_OFFSETS)
@pytest.mark.parametrize('cid', MIS_ROWS)
def test_space_outputs_misplaced(cid, off):
    """The entry points called directly with every OUTPUT one / three floats off alignment (abi_outputs: float64 checks, nothing
    written outside a tensor, nothing left unwritten); the same bits as with aligned outputs where the route has no alignment
    predicate."""
    c = CS.CASE_BY_ID[cid]
    aligned = CS.abi_outputs(c, 0)
    moved = CS.abi_outputs(c, off)
    assert set(aligned) == set(moved)
    if c.bitexact:
        for name in aligned:
            assert torch.equal(aligned[name], moved[name]), (cid, off, name)


FC_SMALL_SHAPES = [(8, 132, 18), (40, 256, 128), (33, 4100, 1000)]


@pytest.mark.parametrize('off', (0,) + OUT_OFFSETS)
@pytest.mark.parametrize('pm', [False, True], ids=['w', 'pm'])
@pytest.mark.parametrize('B,I,O', FC_SMALL_SHAPES)
def test_linear_dgrad_output_misplaced(B, I, O, pm, off):
    """cpg_linear_dgrad with gx off alignment: the weight-streaming kernel of fc_small.hip refuses it and the GEMM takes the call."""
    CS.linear_dgrad_output(B, I, O, pm, off)
