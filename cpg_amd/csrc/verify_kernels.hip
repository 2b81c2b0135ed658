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
//
// With subtract_mean the reference centres both embeddings on the mean of the fold's training rows before every distance, so the
// distances differ per fold (calculate_roc / calculate_val, :43-49 and :89-94):
//  cpg_pair_fold_mean        : one thread per (fold, column) walks the fold's training rows in order -- numpy's np.mean(axis=0).
//  cpg_pair_distance_centred : k_pair_distance's body with every element read as fp32(e - mean_f); grid.y runs over the folds.
//  cpg_pair_sweep_folds      : k_pair_sweep reading row f of the distance matrix for fold f.
//  cpg_pair_val_table        : calculate_val's train-set true / false accepts at every threshold of its (much longer) table;
//                              the LDS histograms are sized from the table, which lives in the workspace.
//  cpg_pair_val_at           : calculate_val_far's counts of every fold's test pairs at one threshold per fold.
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

// Element t of a row: as stored, or centred on the fold's mean and rounded to fp32 (embeddings - mean is a float32 array).
template <bool kCentred>
__device__ __forceinline__ float elem(const float *__restrict__ r, const float *__restrict__ mu, int t) {
    if (kCentred) return r[t] - mu[t];
    return r[t];
}

// Sum of quantity q over the row in numpy's order, from the accumulator chains in `part` (d >= 8) or directly (d < 8).
template <bool kCentred>
__device__ float row_sum(int metric, int q, const float *__restrict__ ra, const float *__restrict__ rb, const float *__restrict__ mu, int d,
                         const Plan &p, const float *part) {
    if (d < 8) {                                // pairwise_sum's n < 8 branch: res = 0, then in order
        float r = 0.0f;
        for (int t = 0; t < d; ++t) r = r + term(metric, q, elem<kCentred>(ra, mu, t), elem<kCentred>(rb, mu, t));
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
            for (int t = end - p.len[op] % 8; t < end; ++t) res = res + term(metric, q, elem<kCentred>(ra, mu, t), elem<kCentred>(rb, mu, t));
            st[sp++] = res;
        } else {
            const float right = st[--sp];
            st[sp - 1] = st[sp - 1] + right;
        }
    }
    return 0.0f + st[0];                        // the reduction's identity, then the row's pairwise sum
}

// kCentred: blockIdx.y is the fold; its mean is row blockIdx.y of `mean` [folds][d], its distances row blockIdx.y of dist / sim [folds][n].
template <bool kCentred>
__global__ __launch_bounds__(kThreads) void k_pair_distance(const float *__restrict__ a, int64_t lda, const float *__restrict__ b, int64_t ldb,
                                                            int64_t n, int d, int metric, const Plan p, const float *__restrict__ mean,
                                                            float *__restrict__ dist, float *__restrict__ sim) {
    __shared__ float part[kWaves][3][kLeafMax * 8];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float *mu = nullptr;
    if (kCentred) {
        mu = mean + (int64_t)blockIdx.y * d;
        dist += (int64_t)blockIdx.y * n;
        if (sim) sim += (int64_t)blockIdx.y * n;
    }
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
                float x = elem<kCentred>(ra, mu, s), y = elem<kCentred>(rb, mu, s);
                float r0 = term(metric, 0, x, y), r1 = term(metric, 1, x, y), r2 = term(metric, 2, x, y);
                for (int t = 1; t < m; ++t) {
                    x = elem<kCentred>(ra, mu, s + 8 * t);
                    y = elem<kCentred>(rb, mu, s + 8 * t);
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
        if (live && lane < nq) v = row_sum<kCentred>(metric, lane, ra, rb, mu, d, p, part[w][lane]);
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
// kRows: fold f reads row f of a distance matrix with leading dimension ldd (the centred distances differ per fold).
template <bool kRows>
__global__ __launch_bounds__(kThreads) void k_pair_sweep(const float *__restrict__ dist, int64_t ldd, const uint8_t *__restrict__ issame,
                                                         int64_t n, int F, const SweepArgs a, int64_t *__restrict__ counts,
                                                         int64_t *__restrict__ best) {
    __shared__ double thr[kThrMax];
    __shared__ int hist[4][kThrMax + 1];
    __shared__ int carry[4][kThreads];
    __shared__ int64_t red_v[kThreads];
    __shared__ int red_i[kThreads];
    const int T = a.T, T1 = a.T + 1, f = blockIdx.x, tid = threadIdx.x;
    if (kRows) dist += (int64_t)f * ldd;
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

// ---------------------------------------------------------------------------------------------- subtract_mean and VAL@FAR
constexpr int kMeanThreads = 64;                // one wave: lanes run over columns, so every row load coalesces
constexpr int kFoldChunk = 256;                 // per-fold thresholds of one cpg_pair_val_at launch (by value)
constexpr size_t kLdsBytes = 64 * 1024;         // what one block may have without asking the runtime for more
constexpr int kPwDepth = 40;                    // pairwise split depth of < 2^33 elements: 26

struct FoldThr {
    double thr[kFoldChunk];
};
static_assert(sizeof(FoldThr) + 96 <= 4096, "kernel arguments are limited to 4 KB");

// LDS of k_pair_val_table for a table of T entries: hist[2][T + 1] and the scan's carry[2][kThreads]
inline size_t val_table_lds(int64_t T) { return (size_t)(2 * (T + 1) + 2 * kThreads) * sizeof(int); }
inline int val_table_max_thr() { return (int)((kLdsBytes / sizeof(int) - 2 * kThreads) / 2 - 1); }

// Row k of np.concatenate([a[train], b[train]]) for the fold [lo, hi): column c of that row.
struct TrainRows {
    const float *a, *b;
    int64_t lda, ldb, lo, skip, m;              // skip = hi - lo; m = n - skip training pairs
    __device__ __forceinline__ float at(int64_t k, int c) const {
        const float *base = k < m ? a : b;
        const int64_t ld = k < m ? lda : ldb;
        int64_t r = k < m ? k : k - m;
        if (r >= lo) r += skip;
        return base[r * ld + c];
    }
};

// numpy's pairwise_sum of one block of n <= 128 elements starting at row s of column 0
__device__ float pw_leaf(const TrainRows &tr, int64_t s, int n) {
    if (n < 8) {
        float res = 0.0f;
        for (int i = 0; i < n; ++i) res = res + tr.at(s + i, 0);
        return res;
    }
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = tr.at(s + j, 0);
    int i = 8;
    for (; i < n - n % 8; i += 8)
        for (int j = 0; j < 8; ++j) r[j] = r[j] + tr.at(s + i + j, 0);
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + tr.at(s + i, 0);
    return res;
}

// numpy's pairwise_sum over all rows of column 0 (what an axis-0 reduction of an [m][1] matrix becomes: one contiguous run)
__device__ float pw_column(const TrainRows &tr, int64_t rows) {
    int64_t fs[kPwDepth], fn[kPwDepth];
    int8_t ph[kPwDepth];
    float val[kPwDepth];
    int sp = 0, vp = 0;
    fs[0] = 0;
    fn[0] = rows;
    ph[0] = 0;
    sp = 1;
    while (sp > 0) {
        const int t = sp - 1;
        if (fn[t] <= kBlockSize) {
            val[vp++] = pw_leaf(tr, fs[t], (int)fn[t]);
            --sp;
            continue;
        }
        int64_t n2 = fn[t] / 2;
        n2 -= n2 % 8;
        if (ph[t] == 0) {                       // left half first
            ph[t] = 1;
            fs[sp] = fs[t];
            fn[sp] = n2;
            ph[sp++] = 0;
        } else if (ph[t] == 1) {
            ph[t] = 2;
            fs[sp] = fs[t] + n2;
            fn[sp] = fn[t] - n2;
            ph[sp++] = 0;
        } else {
            const float right = val[--vp];
            val[vp - 1] = val[vp - 1] + right;
            --sp;
        }
    }
    return val[0];
}

// grid: (ceil(d / 64), folds).  mean[f][c] = np.mean(np.concatenate([a[train_f], b[train_f]]), axis=0)[c]: the add reduction starts
// from its identity 0 and takes the rows one after another (d == 1: the rows are one contiguous run and numpy sums it pairwise),
// then one division by float32(row count).
__global__ __launch_bounds__(kMeanThreads) void k_fold_mean(const float *__restrict__ a, int64_t lda, const float *__restrict__ b, int64_t ldb,
                                                            int64_t n, int d, int F, float *__restrict__ mean) {
    const int f = blockIdx.y, c = blockIdx.x * kMeanThreads + threadIdx.x;
    if (c >= d) return;
    TrainRows tr;
    tr.a = a;
    tr.b = b;
    tr.lda = lda;
    tr.ldb = ldb;
    tr.lo = fold_start(n, F, f);
    tr.skip = fold_start(n, F, f + 1) - tr.lo;
    tr.m = n - tr.skip;
    const int64_t rows = 2 * tr.m;
    float s = 0.0f;
    if (d == 1) {
        s = s + pw_column(tr, rows);
    } else {
        for (int half = 0; half < 2; ++half) {
            const float *base = (half == 0 ? a : b) + c;
            const int64_t ld = half == 0 ? lda : ldb;
#pragma unroll 8
            for (int64_t r = 0; r < tr.lo; ++r) s = s + base[r * ld];
#pragma unroll 8
            for (int64_t r = tr.lo + tr.skip; r < n; ++r) s = s + base[r * ld];
        }
    }
    mean[(int64_t)f * d + c] = s / (float)rows;
}

// Writes 480 table entries a launch into the workspace: a host table of any length reaches the device without a copy engine.
__global__ void k_store_thresholds(const SweepArgs a, double *__restrict__ dst) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.T) dst[t] = a.thr[t];
}

// grid: one block per fold.  Dynamic LDS: hist[2][T + 1] = {train same, train different} by upper-bound index, carry[2][kThreads].
// table[f][t] = {true accepts, false accepts} of the fold's TRAIN pairs at threshold t; totals[f] = {n_same, n_diff} of them.
__global__ __launch_bounds__(kThreads) void k_pair_val_table(const float *__restrict__ dist, int64_t ldd, const uint8_t *__restrict__ issame,
                                                             int64_t n, int F, const double *__restrict__ thr, int T,
                                                             int64_t *__restrict__ table, int64_t *__restrict__ totals) {
    extern __shared__ int lds[];
    const int T1 = T + 1, f = blockIdx.x, tid = threadIdx.x;
    int *hist = lds, *carry = lds + 2 * T1;
    dist += (int64_t)f * ldd;
    for (int t = tid; t < 2 * T1; t += kThreads) hist[t] = 0;
    __syncthreads();
    const int64_t lo = fold_start(n, F, f), hi = fold_start(n, F, f + 1);
    for (int64_t i = tid; i < n; i += kThreads) {
        if (i >= lo && i < hi) continue;
        const int j = upper_bound(thr, T, (double)dist[i]);
        atomicAdd(&hist[(issame[i] != 0 ? 0 : T1) + j], 1);
    }
    __syncthreads();
    const int per = (T1 + kThreads - 1) / kThreads;
    const int c0 = std::min(tid * per, T1), c1 = std::min(c0 + per, T1);
    for (int h = 0; h < 2; ++h) {
        int s = 0;
        for (int j = c0; j < c1; ++j) s += hist[h * T1 + j];
        carry[h * kThreads + tid] = s;
    }
    __syncthreads();
    if (tid < 2) {
        int s = 0;
        for (int k = 0; k < kThreads; ++k) {
            const int v = carry[tid * kThreads + k];
            carry[tid * kThreads + k] = s;
            s += v;
        }
        totals[(int64_t)f * 2 + tid] = s;       // every train pair of this label, bucket T (never accepted) included
    }
    __syncthreads();
    int run[2] = {carry[tid], carry[kThreads + tid]};
    for (int t = c0; t < c1 && t < T; ++t) {
        run[0] += hist[t];
        run[1] += hist[T1 + t];
        int64_t *o = table + ((int64_t)f * T + t) * 2;
        o[0] = run[0];
        o[1] = run[1];
    }
}

// grid: one block per fold of this chunk.  out[f] = {true accepts, false accepts, n_same, n_diff} of the fold's TEST pairs at a.thr[f].
__global__ __launch_bounds__(kThreads) void k_pair_val_at(const float *__restrict__ dist, int64_t ldd, const uint8_t *__restrict__ issame,
                                                          int64_t n, int F, int f0, const FoldThr a, int64_t *__restrict__ out) {
    __shared__ int acc[4];
    const int f = f0 + blockIdx.x, tid = threadIdx.x;
    const double thr = a.thr[blockIdx.x];
    if (tid < 4) acc[tid] = 0;
    __syncthreads();
    dist += (int64_t)f * ldd;
    const int64_t lo = fold_start(n, F, f), hi = fold_start(n, F, f + 1);
    int c[4] = {0, 0, 0, 0};
    for (int64_t i = lo + tid; i < hi; i += kThreads) {
        const bool same = issame[i] != 0, accept = (double)dist[i] < thr;    // false for a NaN distance or threshold
        c[same ? 2 : 3] += 1;
        if (accept) c[same ? 0 : 1] += 1;
    }
    for (int k = 0; k < 4; ++k)
        if (c[k]) atomicAdd(&acc[k], c[k]);
    __syncthreads();
    if (tid < 4) out[(int64_t)f * 4 + tid] = acc[tid];
}

int distance_args(const char *fn, int64_t lda, int64_t ldb, int64_t n, int32_t d, int32_t metric) {
    CPG_REQUIRE(metric == 0 || metric == 1, "%s: metric must be 0 (squared Euclidean) or 1 (angular), got %d", fn, metric);
    CPG_REQUIRE(d >= 1 && d <= kMaxDim, "%s: embedding width %d outside [1, %d]", fn, d, kMaxDim);
    CPG_REQUIRE(n >= 0, "%s: negative pair count %lld", fn, (long long)n);
    CPG_REQUIRE(lda >= d && ldb >= d, "%s: leading dimensions %lld / %lld below the width %d", fn, (long long)lda, (long long)ldb, d);
    return CPG_OK;
}

int fold_args(const char *fn, int64_t n, int32_t nfolds, int32_t min_folds) {
    CPG_REQUIRE(nfolds >= min_folds, "%s: nfolds must be at least %d, got %d", fn, min_folds, nfolds);
    CPG_REQUIRE(n >= nfolds && n <= INT32_MAX, "%s: %lld pairs for %d folds (need nfolds <= n <= 2^31 - 1)", fn, (long long)n, nfolds);
    return CPG_OK;
}

int ascending(const char *fn, const double *thr_host, int32_t n_thr) {
    CPG_REQUIRE(thr_host, "%s: null threshold table", fn);
    for (int32_t t = 0; t < n_thr; ++t)
        CPG_REQUIRE(t == 0 ? !isnan(thr_host[0]) : thr_host[t] > thr_host[t - 1], "%s: the threshold table is not strictly ascending at entry %d",
                    fn, t);
    return CPG_OK;
}

template <bool kRows>
int sweep_run(const char *fn, const float *dist, int64_t ldd, const uint8_t *issame, int64_t n, const double *thr_host, int32_t n_thr,
              int32_t nfolds, int64_t *counts, int64_t *best, void *stream) {
    CPG_REQUIRE(n_thr >= 1 && n_thr <= kThrMax, "%s: %d thresholds outside [1, %d]", fn, n_thr, kThrMax);
    CPG_REQUIRE(thr_host, "%s: null threshold table", fn);
    int rc = fold_args(fn, n, nfolds, 2);
    if (rc != CPG_OK) return rc;
    CPG_REQUIRE(!kRows || ldd >= n, "%s: leading dimension %lld of the distance matrix below the %lld pairs", fn, (long long)ldd, (long long)n);
    rc = ascending(fn, thr_host, n_thr);
    if (rc != CPG_OK) return rc;
    SweepArgs a;
    a.T = n_thr;
    for (int32_t t = 0; t < n_thr; ++t) a.thr[t] = thr_host[t];
    CPG_REQUIRE(dist && issame && counts && best, "%s: null distances, labels or outputs", fn);
    hipLaunchKernelGGL(k_pair_sweep<kRows>, dim3(nfolds), dim3(kThreads), 0, (hipStream_t)stream, dist, ldd, issame, n, (int)nfolds, a, counts,
                       best);
    CPG_CHECK_LAUNCH(fn);
    return CPG_OK;
}

}  // namespace

extern "C" int cpg_pair_distance(const float *a, int64_t lda, const float *b, int64_t ldb, int64_t n, int32_t d, int32_t metric, float *dist,
                                 float *sim, void *stream) {
    const int rc = distance_args("cpg_pair_distance", lda, ldb, n, d, metric);
    if (rc != CPG_OK) return rc;
    if (n == 0) return CPG_OK;
    CPG_REQUIRE(a && b && dist, "cpg_pair_distance: null embeddings or output");
    Plan p;
    p.leaves = p.ops = 0;
    plan_rec(p, 0, d, 0);
    hipLaunchKernelGGL(k_pair_distance<false>, dim3(distance_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, a, lda, b, ldb, n, (int)d,
                       (int)metric, p, (const float *)nullptr, dist, sim);
    CPG_CHECK_LAUNCH("cpg_pair_distance");
    return CPG_OK;
}

extern "C" int cpg_pair_sweep(const float *dist, const uint8_t *issame, int64_t n, const double *thr_host, int32_t n_thr, int32_t nfolds,
                              int64_t *counts, int64_t *best, void *stream) {
    return sweep_run<false>("cpg_pair_sweep", dist, 0, issame, n, thr_host, n_thr, nfolds, counts, best, stream);
}

extern "C" int cpg_pair_fold_mean(const float *a, int64_t lda, const float *b, int64_t ldb, int64_t n, int32_t d, int32_t nfolds, float *mean,
                                  void *stream) {
    int rc = distance_args("cpg_pair_fold_mean", lda, ldb, n, d, 0);
    if (rc != CPG_OK) return rc;
    rc = fold_args("cpg_pair_fold_mean", n, nfolds, 2);
    if (rc != CPG_OK) return rc;
    CPG_REQUIRE(nfolds <= 65535, "cpg_pair_fold_mean: %d folds exceed the 65535 of one launch", nfolds);
    CPG_REQUIRE(a && b && mean, "cpg_pair_fold_mean: null embeddings or output");
    hipLaunchKernelGGL(k_fold_mean, dim3((d + kMeanThreads - 1) / kMeanThreads, nfolds), dim3(kMeanThreads), 0, (hipStream_t)stream, a, lda, b,
                       ldb, n, (int)d, (int)nfolds, mean);
    CPG_CHECK_LAUNCH("cpg_pair_fold_mean");
    return CPG_OK;
}

extern "C" int cpg_pair_distance_centred(const float *a, int64_t lda, const float *b, int64_t ldb, int64_t n, int32_t d, int32_t metric,
                                         const float *mean, int32_t nfolds, float *dist, float *sim, void *stream) {
    const int rc = distance_args("cpg_pair_distance_centred", lda, ldb, n, d, metric);
    if (rc != CPG_OK) return rc;
    CPG_REQUIRE(nfolds >= 1 && nfolds <= 65535, "cpg_pair_distance_centred: %d folds outside [1, 65535]", nfolds);
    if (n == 0) return CPG_OK;
    CPG_REQUIRE(a && b && mean && dist, "cpg_pair_distance_centred: null embeddings, means or output");
    Plan p;
    p.leaves = p.ops = 0;
    plan_rec(p, 0, d, 0);
    hipLaunchKernelGGL(k_pair_distance<true>, dim3(distance_blocks(n), nfolds), dim3(kThreads), 0, (hipStream_t)stream, a, lda, b, ldb, n, (int)d,
                       (int)metric, p, mean, dist, sim);
    CPG_CHECK_LAUNCH("cpg_pair_distance_centred");
    return CPG_OK;
}

extern "C" int cpg_pair_sweep_folds(const float *dist, int64_t ldd, const uint8_t *issame, int64_t n, const double *thr_host, int32_t n_thr,
                                    int32_t nfolds, int64_t *counts, int64_t *best, void *stream) {
    return sweep_run<true>("cpg_pair_sweep_folds", dist, ldd, issame, n, thr_host, n_thr, nfolds, counts, best, stream);
}

extern "C" int32_t cpg_pair_val_max_thresholds(void) { return val_table_max_thr(); }

extern "C" size_t cpg_pair_val_workspace_bytes(int32_t n_thr) {
    return n_thr >= 1 && n_thr <= val_table_max_thr() ? (size_t)n_thr * sizeof(double) : 0;
}

extern "C" int cpg_pair_val_table(const float *dist, int64_t ldd, const uint8_t *issame, int64_t n, const double *thr_host, int32_t n_thr,
                                  int32_t nfolds, int64_t *table, int64_t *totals, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "cpg_pair_val_table";
    CPG_REQUIRE(n_thr >= 1 && n_thr <= val_table_max_thr(),
                "%s: %d thresholds outside [1, %d] (two histograms of n_thr + 1 counters must fit a block's %zu bytes of LDS)", fn, n_thr,
                val_table_max_thr(), kLdsBytes);
    int rc = fold_args(fn, n, nfolds, 2);
    if (rc != CPG_OK) return rc;
    CPG_REQUIRE(ldd == 0 || ldd >= n, "%s: leading dimension %lld of the distance matrix is neither 0 (one row for every fold) nor >= %lld",
                fn, (long long)ldd, (long long)n);
    rc = ascending(fn, thr_host, n_thr);
    if (rc != CPG_OK) return rc;
    CPG_REQUIRE(dist && issame && table && totals, "%s: null distances, labels or outputs", fn);
    CPG_REQUIRE(workspace && workspace_bytes >= (size_t)n_thr * sizeof(double) && ((uintptr_t)workspace & 7) == 0,
                "%s: workspace of %zu bytes (need %zu, 8-byte aligned)", fn, workspace_bytes, (size_t)n_thr * sizeof(double));
    double *thr = (double *)workspace;
    for (int32_t at = 0; at < n_thr; at += kThrMax) {
        SweepArgs a;
        a.T = std::min(kThrMax, n_thr - at);
        for (int t = 0; t < a.T; ++t) a.thr[t] = thr_host[at + t];
        hipLaunchKernelGGL(k_store_thresholds, dim3((kThrMax + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, a, thr + at);
    }
    CPG_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(k_pair_val_table, dim3(nfolds), dim3(kThreads), val_table_lds(n_thr), (hipStream_t)stream, dist, ldd, issame, n,
                       (int)nfolds, (const double *)thr, (int)n_thr, table, totals);
    CPG_CHECK_LAUNCH(fn);
    return CPG_OK;
}

extern "C" int cpg_pair_val_at(const float *dist, int64_t ldd, const uint8_t *issame, int64_t n, const double *thr_host, int32_t nfolds,
                               int64_t *out, void *stream) {
    const char *fn = "cpg_pair_val_at";
    const int rc = fold_args(fn, n, nfolds, 1);
    if (rc != CPG_OK) return rc;
    CPG_REQUIRE(ldd == 0 || ldd >= n, "%s: leading dimension %lld of the distance matrix is neither 0 (one row for every fold) nor >= %lld",
                fn, (long long)ldd, (long long)n);
    CPG_REQUIRE(thr_host, "%s: null threshold table", fn);
    CPG_REQUIRE(dist && issame && out, "%s: null distances, labels or output", fn);
    for (int32_t f0 = 0; f0 < nfolds; f0 += kFoldChunk) {
        FoldThr a;
        const int count = std::min(kFoldChunk, nfolds - f0);
        for (int k = 0; k < kFoldChunk; ++k) a.thr[k] = k < count ? thr_host[f0 + k] : 0.0;
        hipLaunchKernelGGL(k_pair_val_at, dim3(count), dim3(kThreads), 0, (hipStream_t)stream, dist, ldd, issame, n, (int)nfolds, (int)f0, a,
                           out);
    }
    CPG_CHECK_LAUNCH(fn);
    return CPG_OK;
}
