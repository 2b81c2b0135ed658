// The pair verification kernels (include/cpg_hip.h, "pair verification"): the reference's LFW scoring, utils/metrics.py
// `distance` (:11-27) and the fold / threshold sweep of `calculate_roc` (:29-61) with `calculate_accuracy`'s counts (:63-74).
//
//  cpg_pair_distance : one wave per pair.  Every row sum is numpy's float32 pairwise summation (pairwise_sum_FLOAT: blocks of at
//                      most 128 elements summed by eight accumulators, a recursive split at n/2 - (n/2 % 8) above 128, the result
//                      added to the reduction's identity 0) -- the order np.sum(axis=1) and np.linalg.norm(axis=1) use on a
//                      C-contiguous float32 matrix.  Lanes run the eight accumulator chains of every block; lanes 0..2 fold the
//                      chains of one sum each in numpy's order.
//  cpg_pair_sweep    : one block per fold.  Every pair's upper-bound index j in the threshold table goes into an LDS histogram
//                      (this fold's pairs and all pairs, by label); an inclusive scan gives the test counts at every threshold and
//                      the train counts as the totals minus the fold's.  Integer work only.
#include <math.h>

#include <algorithm>

#include "cpg_common.h"

// numpy rounds every product before it is added; one contracted a * b + c changes the sum's last bit.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDim = 4096;
constexpr int kBlockSize = 128;                 // numpy's PW_BLOCKSIZE
constexpr int kLeafMax = 40;                    // blocks of a row of <= 4096 elements: at most 33
constexpr int kOpsMax = 2 * kLeafMax;
constexpr int kStackMax = 8;                    // split depth of <= 4096 elements: 6
constexpr int kThrMax = 480;                    // threshold table entries (travel in the launch arguments)
constexpr float kPi = 3.14159265358979323846f;  // float32(math.pi)

// The blocks of a row and the order numpy adds them in, as a postfix program: op >= 0 pushes block op's sum, op < 0 adds the two
// sums on top of the stack (left + right).  Built on the host from d alone.
struct Plan {
    int start[kLeafMax];
    int len[kLeafMax];
    int8_t op[kOpsMax];
    int leaves, ops;
};

struct SweepArgs {
    double thr[kThrMax];
    int T;
};
static_assert(sizeof(Plan) + 96 <= 4096 && sizeof(SweepArgs) + 96 <= 4096, "kernel arguments are limited to 4 KB");

void plan_rec(Plan &p, int start, int n, int depth) {
    if (n <= kBlockSize) {
        p.start[p.leaves] = start;
        p.len[p.leaves] = n;
        p.op[p.ops++] = (int8_t)p.leaves++;
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    plan_rec(p, start, n2, depth + 1);
    plan_rec(p, start + n2, n - n2, depth + 1);
    p.op[p.ops++] = -1;
}

// quantity q of element t: metric 0 (a - b)^2; metric 1 a * b, a * a, b * b
__device__ __forceinline__ float term(int metric, int q, float x, float y) {
    if (metric == 0) {
        const float d = x - y;
        return d * d;
    }
    return q == 0 ? x * y : q == 1 ? x * x : y * y;
}

// Sum of quantity q over the row in numpy's order, from the accumulator chains in `part` (d >= 8) or directly (d < 8).
__device__ float row_sum(int metric, int q, const float *__restrict__ ra, const float *__restrict__ rb, int d, const Plan &p,
                         const float *part) {
    if (d < 8) {                                // pairwise_sum's n < 8 branch: res = 0, then in order
        float r = 0.0f;
        for (int t = 0; t < d; ++t) r = r + term(metric, q, ra[t], rb[t]);
        return 0.0f + r;
    }
    float st[kStackMax];
    int sp = 0;
    for (int o = 0; o < p.ops; ++o) {
        const int op = p.op[o];
        if (op >= 0) {
            const float *r = part + op * 8;
            float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            const int end = p.start[op] + p.len[op];
            for (int t = end - p.len[op] % 8; t < end; ++t) res = res + term(metric, q, ra[t], rb[t]);
            st[sp++] = res;
        } else {
            const float right = st[--sp];
            st[sp - 1] = st[sp - 1] + right;
        }
    }
    return 0.0f + st[0];                        // the reduction's identity, then the row's pairwise sum
}

__global__ __launch_bounds__(kThreads) void k_pair_distance(const float *__restrict__ a, int64_t lda, const float *__restrict__ b, int64_t ldb,
                                                            int64_t n, int d, int metric, const Plan p, float *__restrict__ dist,
                                                            float *__restrict__ sim) {
    __shared__ float part[kWaves][3][kLeafMax * 8];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = metric == 0 ? 1 : 3;
    const int chains = d >= 8 ? p.leaves * 8 : 0;
    for (int64_t base = (int64_t)blockIdx.x * kWaves; base < n; base += (int64_t)gridDim.x * kWaves) {
        const int64_t i = base + w;
        const bool live = i < n;
        const float *ra = a + (live ? i : 0) * lda;
        const float *rb = b + (live ? i : 0) * ldb;
        if (live) {
            // chain c = 8 * block + j: elements start + j, start + j + 8, ... of the block's multiple-of-8 part
            for (int c = lane; c < chains; c += 64) {
                const int k = c >> 3, s = p.start[k] + (c & 7), m = p.len[k] >> 3;
                float x = ra[s], y = rb[s];
                float r0 = term(metric, 0, x, y), r1 = term(metric, 1, x, y), r2 = term(metric, 2, x, y);
                for (int t = 1; t < m; ++t) {
                    x = ra[s + 8 * t];
                    y = rb[s + 8 * t];
                    r0 = r0 + term(metric, 0, x, y);
                    r1 = r1 + term(metric, 1, x, y);
                    r2 = r2 + term(metric, 2, x, y);
                }
                part[w][0][c] = r0;
                part[w][1][c] = r1;
                part[w][2][c] = r2;
            }
        }
        __syncthreads();
        float v = 0.0f;
        if (live && lane < nq) v = row_sum(metric, lane, ra, rb, d, p, part[w][lane]);
        const float s0 = __shfl(v, 0), s1 = __shfl(v, 1), s2 = __shfl(v, 2);
        if (live && lane == 0) {
            if (metric == 0) {
                dist[i] = s0;
            } else {
                const float norm = sqrtf(s1) * sqrtf(s2);
                const float sm = s0 / norm;     // a zero row: 0 / 0 = NaN, as numpy
                if (sim) sim[i] = sm;
                float c = sm;                   // np.clip(., 0, 1) keeps NaN (fminf / fmaxf would drop it)
                if (c < 0.0f) c = 0.0f;
                if (c > 1.0f) c = 1.0f;
                const float ang = (float)acos((double)c);
                dist[i] = ang * 4.0f / kPi;
            }
        }
        __syncthreads();                        // `part` is reused by the next pair of this wave
    }
}

// first t with thr[t] > x; T when there is none or x is NaN (a NaN distance is never "same")
__device__ __forceinline__ int upper_bound(const double *thr, int T, double x) {
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// KFold(n_splits=F, shuffle=False): fold f is [f * q + min(f, r), ...) with q = n / F, r = n % F, the first r folds one longer
__device__ __forceinline__ int64_t fold_start(int64_t n, int F, int f) {
    const int64_t q = n / F, r = n % F;
    return f * q + (f < r ? f : r);
}

// grid: one block per fold.  LDS: hist[4][T + 1] = {fold same, fold different, all same, all different} by upper-bound index.
__global__ __launch_bounds__(kThreads) void k_pair_sweep(const float *__restrict__ dist, const uint8_t *__restrict__ issame, int64_t n,
                                                         int F, const SweepArgs a, int64_t *__restrict__ counts, int64_t *__restrict__ best) {
    __shared__ double thr[kThrMax];
    __shared__ int hist[4][kThrMax + 1];
    __shared__ int carry[4][kThreads];
    __shared__ int64_t red_v[kThreads];
    __shared__ int red_i[kThreads];
    const int T = a.T, T1 = a.T + 1, f = blockIdx.x, tid = threadIdx.x;
    for (int t = tid; t < T; t += kThreads) thr[t] = a.thr[t];
    for (int t = tid; t < 4 * (kThrMax + 1); t += kThreads) (&hist[0][0])[t] = 0;
    __syncthreads();
    const int64_t lo = fold_start(n, F, f), hi = fold_start(n, F, f + 1);
    for (int64_t i = tid; i < n; i += kThreads) {
        const int j = upper_bound(thr, T, (double)dist[i]);
        const int same = issame[i] != 0;
        atomicAdd(&hist[same ? 2 : 3][j], 1);
        if (i >= lo && i < hi) atomicAdd(&hist[same ? 0 : 1][j], 1);
    }
    __syncthreads();
    // inclusive scan over j: thread tid owns the contiguous run [c0, c1)
    const int per = (T1 + kThreads - 1) / kThreads;
    const int c0 = std::min(tid * per, T1), c1 = std::min(c0 + per, T1);
    for (int h = 0; h < 4; ++h) {
        int s = 0;
        for (int j = c0; j < c1; ++j) s += hist[h][j];
        carry[h][tid] = s;
    }
    __syncthreads();
    if (tid < 4) {                              // exclusive offsets of the runs (4 x 256 adds)
        int s = 0;
        for (int k = 0; k < kThreads; ++k) {
            const int v = carry[tid][k];
            carry[tid][k] = s;
            s += v;
        }
    }
    __syncthreads();
    // totals: the whole histogram, bucket T (never "same") included
    int tot[4];
    for (int h = 0; h < 4; ++h) tot[h] = 0;
    for (int h = 0; h < 4; ++h) {
        const int last = kThreads - 1;
        const int lc0 = std::min(last * per, T1), lc1 = std::min(lc0 + per, T1);
        int s = carry[h][last];
        for (int j = lc0; j < lc1; ++j) s += hist[h][j];
        tot[h] = s;
    }
    int64_t bv = -1;
    int bi = T;
    int run[4];
    for (int h = 0; h < 4; ++h) run[h] = carry[h][tid];
    for (int t = c0; t < c1; ++t) {
        for (int h = 0; h < 4; ++h) run[h] += hist[h][t];
        if (t >= T) break;
        // predicted "same" at threshold t: every pair whose upper bound is <= t
        const int tp = run[0], fp = run[1], tn = tot[1] - run[1], fn = tot[0] - run[0];
        int64_t *o = counts + ((int64_t)f * T + t) * 4;
        o[0] = tp;
        o[1] = fp;
        o[2] = tn;
        o[3] = fn;
        const int64_t train = (int64_t)(run[2] - run[0]) + (int64_t)((tot[3] - run[3]) - tn);     // train tp + train tn
        if (train > bv) {
            bv = train;
            bi = t;
        }
    }
    red_v[tid] = bv;
    red_i[tid] = bi;
    __syncthreads();
    if (tid == 0) {                             // first maximum: runs are in threshold order
        int64_t v = -1;
        int idx = 0;
        for (int k = 0; k < kThreads; ++k)
            if (red_v[k] > v) {
                v = red_v[k];
                idx = red_i[k];
            }
        best[f] = idx;
    }
}

inline unsigned distance_blocks(int64_t n) {
    const int64_t b = (n + kWaves - 1) / kWaves;
    return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

}  // namespace

extern "C" int cpg_pair_distance(const float *a, int64_t lda, const float *b, int64_t ldb, int64_t n, int32_t d, int32_t metric, float *dist,
                                 float *sim, void *stream) {
    CPG_REQUIRE(metric == 0 || metric == 1, "cpg_pair_distance: metric must be 0 (squared Euclidean) or 1 (angular), got %d", metric);
    CPG_REQUIRE(d >= 1 && d <= kMaxDim, "cpg_pair_distance: embedding width %d outside [1, %d]", d, kMaxDim);
    CPG_REQUIRE(n >= 0, "cpg_pair_distance: negative pair count %lld", (long long)n);
    CPG_REQUIRE(lda >= d && ldb >= d, "cpg_pair_distance: leading dimensions %lld / %lld below the width %d", (long long)lda, (long long)ldb, d);
    if (n == 0) return CPG_OK;
    CPG_REQUIRE(a && b && dist, "cpg_pair_distance: null embeddings or output");
    Plan p;
    p.leaves = p.ops = 0;
    plan_rec(p, 0, d, 0);
    hipLaunchKernelGGL(k_pair_distance, dim3(distance_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, a, lda, b, ldb, n, (int)d,
                       (int)metric, p, dist, sim);
    CPG_CHECK_LAUNCH("cpg_pair_distance");
    return CPG_OK;
}

extern "C" int cpg_pair_sweep(const float *dist, const uint8_t *issame, int64_t n, const double *thr_host, int32_t n_thr, int32_t nfolds,
                              int64_t *counts, int64_t *best, void *stream) {
    CPG_REQUIRE(n_thr >= 1 && n_thr <= kThrMax, "cpg_pair_sweep: %d thresholds outside [1, %d]", n_thr, kThrMax);
    CPG_REQUIRE(thr_host, "cpg_pair_sweep: null threshold table");
    CPG_REQUIRE(nfolds >= 2, "cpg_pair_sweep: nfolds must be at least 2, got %d", nfolds);
    CPG_REQUIRE(n >= nfolds && n <= INT32_MAX, "cpg_pair_sweep: %lld pairs for %d folds (need nfolds <= n <= 2^31 - 1)", (long long)n, nfolds);
    SweepArgs a;
    a.T = n_thr;
    for (int32_t t = 0; t < n_thr; ++t) {
        CPG_REQUIRE(t == 0 ? !isnan(thr_host[0]) : thr_host[t] > thr_host[t - 1],
                    "cpg_pair_sweep: the threshold table is not strictly ascending at entry %d", t);
        a.thr[t] = thr_host[t];
    }
    CPG_REQUIRE(dist && issame && counts && best, "cpg_pair_sweep: null distances, labels or outputs");
    hipLaunchKernelGGL(k_pair_sweep, dim3(nfolds), dim3(kThreads), 0, (hipStream_t)stream, dist, issame, n, (int)nfolds, a, counts, best);
    CPG_CHECK_LAUNCH("cpg_pair_sweep");
    return CPG_OK;
}
