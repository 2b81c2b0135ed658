"""tests/_evalconv.py's fp64 reference of the inference conv pinned to torch's own fp32 operators on the CPU: F.conv2d with the
effective weight, F.batch_norm(training=False), relu.  Covers bias / no bias, relu / no relu, a piggymask whose values sit on the
threshold, and a zero running variance (eps alone under the square root)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _evalconv as E
from oracle import ops

THR = ops.DEFAULT_THRESHOLD


def _torch_fp32(x, w, pm, bias, gamma, beta, mean, var, eps, relu):
    weff = w if pm is None else w * (pm > THR).float()
    y = F.conv2d(x, weff, bias, padding=1)
    y = F.batch_norm(y, mean, var, gamma, beta, training=False, eps=eps)
    return F.relu(y) if relu else y


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('piggymask', [False, True])
@pytest.mark.parametrize('N,C,H,W,K', [(2, 6, 9, 7, 5), (1, 13, 8, 8, 11)])
def test_reference_matches_torch_fp32(N, C, H, W, K, bias, relu, piggymask):
    g = torch.Generator().manual_seed(N + C + H + W + K + 2 * bias + 4 * relu + 8 * piggymask)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * 0.3
    b = torch.randn(K, generator=g) * 0.3 if bias else None
    pm = None
    if piggymask:
        pm = torch.where(torch.rand(K, C, 3, 3, generator=g) < 0.5, 0.01, 0.001).float()
        pm[0] = THR                                                         # on the threshold: bin = 0 (x <= thr)
        pm[1] = float(np.nextafter(np.float32(THR), np.float32(1.0)))       # one ulp above: bin = 1
    gamma = torch.rand(K, generator=g) + 0.5
    beta = torch.rand(K, generator=g) - 0.5
    mean = torch.randn(K, generator=g) * 0.3
    var = torch.rand(K, generator=g) + 0.5
    var[K - 1] = 0.0
    eps = 1e-3
    ref, bound = E.eval_conv_ref(x, w, pm, b, gamma, beta, mean, var, eps=eps, relu=relu, threshold=THR, family=E.GAMMA_DIRECT)
    got = _torch_fp32(x, w, pm, b, gamma, beta, mean, var, eps, relu).double()
    assert ref.dtype == torch.float64 and ref.shape == (N, K, H, W)
    assert bool(((got - ref).abs() <= bound).all()), float((got - ref).abs().max())
    # the bound is tight enough to tell the operation apart from its near misses
    s = gamma.double() / torch.sqrt(var.double() + eps)
    assert float(s[K - 1]) == pytest.approx(float(gamma[K - 1]) / np.sqrt(eps))
    if piggymask:
        flipped = pm.clone()
        flipped[0] = 1.0                                                    # channel 0 with bin = 1 instead of 0
        wrong, _ = E.eval_conv_ref(x, w, flipped, b, gamma, beta, mean, var, eps=eps, relu=relu, threshold=THR)
        assert not bool(((got - wrong).abs() <= bound).all())
        assert not bool(((got - E.eval_conv_ref(x, w, pm, b, gamma, beta, mean, var, eps=eps, relu=relu,
                                                threshold=float(np.nextafter(np.float32(THR), np.float32(1.0))))[0]).abs()
                         <= bound).all())
    wrong_eps = (got - E.eval_conv_ref(x, w, pm, b, gamma, beta, mean, var, eps=eps * 2, relu=relu, threshold=THR)[0]).abs()
    assert not bool((wrong_eps <= bound).all())


def test_bound_of_a_dead_channel_is_the_shift_term():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 6, 6, generator=g)
    w = torch.randn(3, 4, 3, 3, generator=g)
    w[1] = 0.0
    w[2] = -0.0
    b = torch.tensor([0.1, -0.4, 0.25])
    gamma, beta = torch.tensor([1.0, 1.5, 0.7]), torch.tensor([0.0, 0.2, -0.1])
    mean, var = torch.tensor([0.0, 0.3, -0.2]), torch.tensor([1.0, 2.0, 0.5])
    ref, conv_term, shift_term = E.eval_conv_terms(x, w, None, b, gamma, beta, mean, var, eps=1e-5, relu=False)
    assert bool((conv_term[:, 1:] == 0).all()) and bool((conv_term[:, 0] > 0).all())
    s = gamma.double() / torch.sqrt(var.double() + 1e-5)
    want = (b.double() - mean.double()) * s + beta.double()
    assert torch.equal(ref[:, 1:], want[1:, None, None].expand(2, 2, 6, 6))
    assert E.live_input_extent(w) == 4 and E.dead_output_channels(w).tolist() == [False, True, True]


@pytest.mark.parametrize('C,live,want', [(78, [77], 80), (78, [75], 76), (78, [76], 80), (78, [], 0), (3, [0], 4), (8, [3], 4),
                                         (8, [4], 8)])
def test_live_input_extent(C, live, want):
    w = torch.zeros(5, C, 3, 3)
    for c in live:
        w[4, c, 0, 2] = 1.0
    assert E.live_input_extent(w) == want
