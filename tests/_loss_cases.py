"""Inputs, references, bars and the case bodies of tests/test_loss_heads_gpu.py (the loss heads against stock torch in fp64), shared
with tests/test_guard_bands_gpu.py.  fused_xent / fused_angle take a buffer factory (tests/_parity_cases.py: PLAIN is today's .to(DEV));
every assertion lives here."""
import numpy as np
import torch
import torch.nn.functional as F

from _parity_cases import PLAIN

DEV = 'cuda:0'
FLOOR = 4 * 2.0 ** -23
EMOTION_COUNTS = [74874, 134415, 25459, 14090, 6378, 3803, 24882]          # cpg_amd/utils/manager.py: the emotion task's class counts


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max()
    diff = np.abs(a - b).max()
    if scale == 0.0:
        return 0.0 if diff == 0.0 else np.inf
    return diff / scale


def hold(what, fused, stock32, ref64):
    e, bar = err(fused, ref64), max(4 * err(stock32, ref64), FLOOR)
    print('%-40s err %.3e  bar %.3e (stock fp32 %.3e)' % (what, e, bar, err(stock32, ref64)))
    assert e <= bar, (what, e, bar)          # (a NaN error fails too)
    return e


def emotion_weights():
    counts = torch.tensor(EMOTION_COUNTS, dtype=torch.float32)
    return (torch.sum(counts) - counts) / counts


# ------------------------------------------------------------------------------------------------------------ cross-entropy
def stock_xent(z, t, w, dtype):
    z = z.detach().clone().to(dtype).requires_grad_(True)
    loss = F.cross_entropy(z, t, weight=None if w is None else w.to(dtype))
    loss.backward()
    return loss.detach().numpy(), z.grad.numpy()


def fused_xent(z, t, w, buf=PLAIN, made=None):
    from cpg_amd.models.losses import FusedCrossEntropyLoss
    crit = buf.rehome(FusedCrossEntropyLoss(weight=w).to(DEV), const_buffers=True)
    zd = buf.put(z.detach()).requires_grad_(True)
    loss = crit(zd, buf.put(t))
    loss.backward()
    if made is not None:
        made += [loss, zd.grad]
    return loss.detach().cpu().numpy(), zd.grad.cpu().numpy(), float(crit.correct), float(crit.accuracy)


def xent_inputs(B, C, weights, seed=0):
    g = torch.Generator().manual_seed(1000 * B + C + seed)
    z = torch.randn(B, C, generator=g) * 3
    t = torch.randint(0, C, (B,), generator=g)
    w = {'none': None, 'random': torch.rand(C, generator=g) + 0.25, 'emotion': emotion_weights()}[weights]
    return z, t, w


# the issue's shapes, the emotion task's seven classes, and both sides of the two kernel thresholds (512 and 8 192 classes)
XENT_SHAPES = [(1, 1), (7, 2), (4, 5), (3, 63), (3, 64), (5, 65), (33, 257), (5, 4630), (3, 512), (3, 513), (2, 8192), (2, 8193)]
XENT_CASES = [(B, C, w) for B, C in XENT_SHAPES for w in ('none', 'random')] + [(9, 7, 'emotion')]


def cross_entropy_case(B, C, weights, buf=PLAIN):
    z, t, w = xent_inputs(B, C, weights)
    l64, g64 = stock_xent(z, t, w, torch.float64)
    l32, g32 = stock_xent(z, t, w, torch.float32)
    loss, grad, correct, accuracy = fused_xent(z, t, w, buf)
    hold('loss %dx%d %s' % (B, C, weights), loss, l32, l64)
    hold('dlogits %dx%d %s' % (B, C, weights), grad, g32, g64)
    want = int((z.argmax(1) == t).sum())
    assert correct == want and accuracy == np.float32(want) / np.float32(B)


# ------------------------------------------------------------------------------------------------------------ angular head
def stock_angle(x, w, t, it, dtype):
    from cpg_amd.models.spherenet import AngleLinear, AngleLoss
    lin = AngleLinear(w.shape[0], w.shape[1]).to(dtype)
    lin.weight.data.copy_(w)
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    crit = AngleLoss()
    crit.it = it - 1
    cos, phi = lin(xx)
    loss = crit((cos, phi), t)
    loss.backward()
    assert crit.it == it
    return loss.detach().numpy(), xx.grad.numpy(), lin.weight.grad.numpy(), cos.detach(), phi.detach()


def fused_angle(x, w, t, it, buf=PLAIN, made=None):
    from cpg_amd.models.losses import FusedAngleLoss
    from cpg_amd.models.spherenet import AngleLinear
    lin = AngleLinear(w.shape[0], w.shape[1])
    lin.weight.data.copy_(w)
    lin = buf.rehome(lin.to(DEV))
    xd = buf.put(x.detach()).requires_grad_(True)
    crit = FusedAngleLoss()
    crit.it = it - 1
    loss = crit.head_loss(xd, lin, buf.put(t))
    loss.backward()
    if made is not None:
        made += [loss, xd.grad, lin.weight.grad]
    assert crit.it == it and crit.lamb == max(5.0, 1500.0 / (1 + 0.1 * it))
    return loss.detach().cpu().numpy(), xd.grad.cpu().numpy(), lin.weight.grad.cpu().numpy(), float(crit.correct)


def sweep_inputs(B, D, C):
    """x_i = a_i (c_i what_t + sqrt(1 - c_i^2) u_i): rows whose cosine to their target column sweeps [-0.95, 0.95]."""
    g = torch.Generator().manual_seed(B * 7 + C)
    w = (torch.rand(D, C, generator=g, dtype=torch.float64) * 2 - 1)
    t = torch.randint(0, C, (B,), generator=g)
    what = w[:, t].T / w[:, t].norm(dim=0).view(-1, 1)                       # [B][D]
    u = torch.randn(B, D, generator=g, dtype=torch.float64)
    u = u - (u * what).sum(1, keepdim=True) * what
    u = u / u.norm(dim=1, keepdim=True)
    c = torch.linspace(-0.95, 0.95, B, dtype=torch.float64)[torch.randperm(B, generator=g)].view(-1, 1)
    a = 5 + 20 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    x = a * (c * what + torch.sqrt(1 - c * c) * u)
    return x.float(), w.float(), t


SWEEP = {}


def sweep_reference(B, D, C, it):
    """Inputs and the stock fp64 / fp32 results, computed once per case and shared (never modified)."""
    key = (B, D, C, it)
    if key not in SWEEP:
        x, w, t = sweep_inputs(B, D, C)
        SWEEP[key] = (x, w, t, stock_angle(x, w, t, it, torch.float64), stock_angle(x, w, t, it, torch.float32))
    return SWEEP[key]


ANGLE_SWEEP_SHAPES = [(64, 512, 200), (37, 512, 4630)]


def angle_head_margin_sweep(B, D, C, it, buf=PLAIN):
    x, w, t, r64, r32 = sweep_reference(B, D, C, it)
    cos = (r64[3] / x.double().norm(dim=1, keepdim=True))
    ct = cos.gather(1, t.view(-1, 1)).view(-1)
    k = torch.floor(4 * torch.acos(ct) / 3.14159265).long()
    counts = torch.bincount(k, minlength=4).tolist()
    print('k counts', counts, 'max |cos|', float(cos.abs().max()))
    assert len(counts) == 4 and min(counts) >= 1
    assert float(cos.abs().max()) <= 0.95 + 1e-6          # (x and w were rounded to fp32 after the construction)
    loss, gx, gw, correct = fused_angle(x, w, t, it, buf)
    tag = '%dx%dx%d it %d' % (B, D, C, it)
    hold('loss ' + tag, loss, r32[0], r64[0])
    hold('gx ' + tag, gx, r32[1], r64[1])
    hold('gw ' + tag, gw, r32[2], r64[2])
    # the head's correct count: rows whose first maximum of f (AngleLoss's `output`, fp64) is the target
    scale = 1.0 / (1 + max(5.0, 1500.0 / (1 + 0.1 * it)))
    onehot = torch.zeros_like(r64[3]).scatter_(1, t.view(-1, 1), 1.0)
    f64 = r64[3] - r64[3] * onehot * scale + r64[4] * onehot * scale
    top2 = f64.topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3          # no near tie that fp32 could resolve the other way
    want = int((f64.argmax(1) == t).sum())
    print('correct', correct, 'argmax count of f', want)
    assert correct == want
