"""tests/_special.py does what it claims -- on the arbiter alone, no GPU: the builders' poison is where they say, ties are ties in the
arbiter, both signs of bn(x) occur, the exclusion cap holds for every case tests/test_special_values_gpu.py runs, and no decision of
the arbiter (sign of bn(x), winner of a pooling window) is so close that fp32 could legitimately decide it the other way."""
import pytest
import torch

import _special as S

CASES = S.cases()
# fp32 evaluates bn(x) of these inputs (|z| of order 1) to a few 1e-7: a sign or an order decided by more than this is decided alike
MARGIN = 2e-6


def _pair(case):
    op, pattern, train, shape = case
    t = S.build(op, pattern, shape)
    return t, S.stock(op, t, train)


@pytest.mark.parametrize('case', CASES, ids=S.case_id)
def test_exclusion_cap_and_margins(case):
    op, pattern, train, shape = case
    t, ref = _pair(case)
    assert S.cap_holds(t, ref, train)
    bad, chan = S.exclusions(ref, train)
    assert int(chan.sum()) <= 1 or pattern == 'inf_x'
    # the clean twin differs from the case in the pattern's own elements only
    clean = S.build(op, 'plain', shape)
    if pattern in ('nan_x', 'inf_x', 'nan_gy', 'nan_res'):
        key = {'nan_x': 'x', 'inf_x': 'x', 'nan_gy': 'gy', 'nan_res': 'res'}[pattern]
        for k in ('x', 'gy', 'res'):
            if t[k] is not None:
                differ = int((t[k].view(torch.int32) != clean[k].view(torch.int32)).sum())
                assert differ == ((2 if pattern == 'inf_x' else 1) if k == key else 0), (k, differ)
    # decisions with a margin: the sign of z wherever the ReLU looks at it, the winner of every window that is not an exact tie
    z = ref['z']
    live = torch.isfinite(z) & (z != 0)
    if op != 'bn_norelu' and bool(live.any()):
        assert float(z[live].abs().min()) > MARGIN, float(z[live].abs().min())
    if op in ('pool2', 'pool3'):
        a = torch.nan_to_num(ref['act'], nan=0.0, posinf=1e30)
        top = S.windows(op, a).topk(2, dim=2).values
        gap = top[:, :, 0] - top[:, :, 1]
        close = gap[(gap > 0) & torch.isfinite(gap)]
        assert close.numel() == 0 or float(close.min()) > MARGIN, float(close.min())


@pytest.mark.parametrize('case', [c for c in CASES if c[1] == 'ties'], ids=S.case_id)
def test_ties_are_ties_in_the_arbiter(case):
    op, pattern, train, shape = case
    t, ref = _pair(case)
    w = S.windows(op, ref['act'])
    maximal = (w == w.max(dim=2, keepdim=True).values).sum(dim=2)
    assert int(maximal.min()) >= 2, 'a window with a single maximal element'
    for kind in (0, 1):                      # gamma > 0 and gamma < 0: both signs of z, so routed and ReLU-masked windows both occur
        z = ref['z'][:, kind::4]
        assert bool((z > 0).any()) and bool((z < 0).any())
    assert bool((ref['z'][:, 2::4] == t['beta'][2]).all()) and bool((ref['z'][:, 3::4] == 0).all())
    # the routed gradient really lands on one element per window (the first): in eval mode it is the arbiter's gx support
    if not train:
        first = ref['gx'][:, 0::4] != 0
        assert 0 < int(first.sum()) <= w.shape[3] * shape[0] * (shape[1] // 4)


@pytest.mark.parametrize('case', [c for c in CASES if c[1] == 'nan_x'], ids=S.case_id)
def test_nan_x_poisons_one_element_or_one_channel(case):
    op, pattern, train, shape = case
    t, ref = _pair(case)
    nan_act, nan_y = torch.isnan(ref['act']), torch.isnan(ref['y'])
    if train:
        for a in (nan_act, nan_y):
            assert bool(a[:, 0].all()) and not bool(a[:, 1:].any())
        assert torch.isnan(ref['running_mean']).tolist() == [True] + [False] * (shape[1] - 1)
        assert torch.isnan(ref['running_var']).tolist() == [True] + [False] * (shape[1] - 1)
    else:
        assert int(nan_act.sum()) == 1 and bool(nan_act[0, 0, shape[2] // 2, shape[3] // 2])
        if op in ('pool2', 'pool3'):
            hit = torch.isnan(S.windows(op, ref['act'])).any(dim=2).view(nan_y.shape)
            assert bool((hit == nan_y).all()) and int(nan_y.sum()) == {'pool2': 1, 'pool3': int(hit.sum())}[op]
            assert 1 <= int(nan_y.sum()) <= 4
        else:
            assert int(nan_y.sum()) == 1


def test_inf_and_zero_patterns():
    for op in S.OPS:
        shape = S.SHAPES[op][0]
        t = S.build(op, 'inf_x', shape)
        ref = S.stock(op, t, False)
        assert int(torch.isinf(t['x']).sum()) == 2 and not bool(torch.isnan(ref['act']).any())
        assert int(torch.isinf(ref['act']).sum()) == 2          # +Inf under gamma > 0 and -Inf under gamma < 0 both come out as +Inf
        t = S.build(op, 'zeros', shape)
        ref = S.stock(op, t, False)
        assert bool((ref['z'] == 0).all())
        if op != 'bn_norelu':                 # relu'(0) = 0: nothing comes back
            assert bool((ref['gx'] == 0).all()) and bool((ref['dbeta'] == 0).all()) and bool((ref['dgamma'] == 0).all())


@pytest.mark.parametrize('slopes', S.PRELU_SLOPES)
def test_prelu_builders(slopes):
    shape = (2, 4, 6, 10)
    t = S.build_prelu('zeros', slopes, shape, False)
    assert bool((t['x'] == 0).all()) and bool(torch.signbit(t['x']).any()) and not bool(torch.signbit(t['x']).all())
    assert t['alpha'].numel() == (1 if slopes == 'shared' else 4)
    if slopes == 'zero':
        assert bool((t['alpha'] == 0).all())
    if slopes == 'negative':
        assert bool((t['alpha'] < 0).all())
    ref = S.stock_prelu(S.build_prelu('nan_x', slopes, shape, True))
    assert int(torch.isnan(ref['y']).sum()) == 1
    ref = S.stock_prelu(S.build_prelu('nan_res', slopes, shape, True))
    assert int(torch.isnan(ref['y']).sum()) == 1 and not bool(torch.isnan(ref['gx']).any())


def test_comparison_helpers():
    a = torch.tensor([1.0, S.NAN, S.INF, -S.INF, 0.0])
    assert S.same_nonfinite(a, a.double())
    assert not S.same_nonfinite(torch.tensor([1.0, 0.0, S.INF, -S.INF, 0.0]), a)          # a NaN turned into 0
    assert not S.same_nonfinite(torch.tensor([1.0, S.NAN, -S.INF, -S.INF, 0.0]), a)       # the sign of an Inf
    assert S.finite_err(torch.tensor([1.0, 5.0, 5.0, 5.0, 0.0]), a) == 0.0
    assert S.finite_err(torch.tensor([1.5, 0.0, 0.0, 0.0, 0.0]), a) == 0.5
    assert S.finite_err(torch.tensor([S.NAN, 0.0, 0.0, 0.0, 0.0]), a) == S.INF
    assert S.finite_err(torch.tensor([1.5, 0.0, 0.0, 0.0, 0.0]), a, skip=torch.tensor([True, False, False, False, False])) == 0.0
