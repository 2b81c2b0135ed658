"""The two step-telemetry records of include/cpg_hip.h (cpg_sgd_step_stats, cpg_pm_step_stats) restated in numpy, from the tensors
before and after a step.  Sums go through `total`: math.fsum (the correctly rounded sum, the reference of the GPU tests) or `plain`
(fp64 additions in index order).  Every term is the fp64 square of an fp32 value (exact) or of an fp64 difference of two fp32 values,
formed the same way in the kernels; so any fp64 summation of the n non-negative terms is within (n - 1) * 2^-53 relative of the exact
sum, and within n * 2^-52 of its correctly rounded value -- the bound the tests hold the kernels to."""
import math

import numpy as np

SGD_FIELDS = ('n_routed', 'g_nonfinite', 'g_sumsq', 'g_absmax', 'w_nonfinite', 'dw_sumsq', 'w_sumsq', 'w_absmax')
PM_FIELDS = ('n_routed', 'g_sumsq', 'g_absmax', 'dpm_sumsq', 'flips_on', 'flips_off', 'picked', 'pm_nonfinite')
SUMS = ('g_sumsq', 'dw_sumsq', 'w_sumsq', 'dpm_sumsq')       # every other field must be EQUAL
KCHUNK = 4096
RECORD_BYTES = 64
MODE_FINETUNE, MODE_PRUNE = 0, 1


def plain(terms):
    s = np.float64(0.0)
    for t in terms:
        s = s + t
    return float(s)


def pieces(n):
    return (n + KCHUNK - 1) // KCHUNK


def workspace_bytes(ns):
    return sum(pieces(n) for n in ns) * RECORD_BYTES


def _f32(a):
    a = np.ascontiguousarray(np.asarray(a).reshape(-1))
    assert a.dtype == np.float32
    return a


def _sumsq_absmax(x, total):
    """(sum x^2 in fp64, max |x|) over the finite entries of the fp32 vector x; (0, 0) if there is none."""
    x = x[np.isfinite(x)]
    x64 = x.astype(np.float64)
    return float(total(x64 * x64)), float(np.abs(x).max()) if x.size else 0.0


def _diff_sumsq(a1, a0, total):
    both = np.isfinite(a1) & np.isfinite(a0)
    d = a1[both].astype(np.float64) - a0[both].astype(np.float64)
    return float(total(d * d))


def sgd_record(w0, w1, g1, owner, cur, total=math.fsum):
    """w0 / w1: the weight before / after the step, g1: the routed gradient the step wrote back."""
    w0, w1, g1 = _f32(w0), _f32(w1), _f32(g1)
    routed = np.asarray(owner).reshape(-1) == cur
    g = g1[routed]
    g_sumsq, g_absmax = _sumsq_absmax(g, total)
    w_sumsq, w_absmax = _sumsq_absmax(w1, total)
    return dict(n_routed=int(routed.sum()), g_nonfinite=int((~np.isfinite(g)).sum()), g_sumsq=g_sumsq, g_absmax=g_absmax,
                w_nonfinite=int((~np.isfinite(w1)).sum()), dw_sumsq=_diff_sumsq(w1, w0, total), w_sumsq=w_sumsq, w_absmax=w_absmax)


def pm_record(pm0, pm1, g1, owner, cur, mode, thr, total=math.fsum):
    pm0, pm1, g1 = _f32(pm0), _f32(pm1), _f32(g1)
    owner = np.asarray(owner).reshape(-1).astype(np.int64)
    keep = (owner != 0) & (owner < cur) if mode == MODE_FINETUNE else np.zeros(owner.shape, dtype=bool)
    g_sumsq, g_absmax = _sumsq_absmax(g1[keep], total)
    with np.errstate(invalid='ignore'):
        on0, on1 = pm0[keep] > np.float32(thr), pm1[keep] > np.float32(thr)          # fp32 compares, False for NaN
    return dict(n_routed=int(keep.sum()), g_sumsq=g_sumsq, g_absmax=g_absmax, dpm_sumsq=_diff_sumsq(pm1, pm0, total),
                flips_on=int((~on0 & on1).sum()), flips_off=int((on0 & ~on1).sum()), picked=int(on1.sum()),
                pm_nonfinite=int((~np.isfinite(pm1)).sum()))


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -3e-42, 1.1754942e-38, 3e30, -2.5e25, 1e19, 3.4028235e38],
                    dtype=np.float32)       # NaN, +-Inf, zeros, denormals, and finite values whose square overflows fp32


def values(n, seed, specials=0.0):
    """n fp32 values around 1e-2; a fraction `specials` of them drawn from SPECIALS."""
    rng = np.random.RandomState(seed)
    v = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    if specials:
        hit = rng.rand(n) < specials
        v[hit] = SPECIALS[rng.randint(0, len(SPECIALS), size=int(hit.sum()))]
    return v


def owners(n, pattern, cur, seed):
    """all: every slot is cur's; none: nobody's is (0, 1, 255); mixed: 0 .. cur + 1 and 255."""
    rng = np.random.RandomState(seed)
    pool = {'all': [cur], 'none': [0, 1, 255] if cur != 1 else [0, 2, 255], 'mixed': list(range(0, cur + 2)) + [255]}[pattern]
    return np.array(pool, dtype=np.uint8)[rng.randint(0, len(pool), size=n)]


def threshold_masks(n, thr, seed):
    """(piggymask, gradient): every value sits exactly at thr, one ulp above or one ulp below; the gradient is +-1, so that Adam's
    first step (pm -= lr * g / (|g| + eps), lr = 5e-4 >> one ulp) moves each by a known sign across or away from the threshold."""
    rng = np.random.RandomState(seed)
    t = np.float32(thr)
    pool = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(-1))], dtype=np.float32)
    return pool[rng.randint(0, 3, size=n)], np.where(rng.rand(n) < 0.5, 1.0, -1.0).astype(np.float32)


def assert_record(got, want, n, what=''):
    """got: the kernel's record (field -> float), want: the math.fsum restatement of an n-element item."""
    for k, v in want.items():
        if k in SUMS:
            print('%s %s: kernel %.17g, fsum %.17g, |diff| / fsum %.3e (bound %.3e)' % (
                what, k, got[k], v, abs(got[k] - v) / v if v else abs(got[k] - v), n * 2.0 ** -52))
            assert abs(got[k] - v) <= n * 2.0 ** -52 * v, (what, k, got[k], v)
        else:
            assert got[k] == v, (what, k, got[k], v)
