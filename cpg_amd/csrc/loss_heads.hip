// Loss heads: the step from the network's output to the loss, the accuracy and the gradient that starts the backward pass.
//
//   (a) row softmax cross-entropy = nn.CrossEntropyLoss(weight) with its mean reduction + classification_accuracy
//       (utils/manager.py:29-36,58-62,120-121; utils/__init__.py:46-49).  One pass over the logits up to 8 192 classes: a row lives in registers (one wave per row up to
//       512 classes, one block per row up to 8 192; WIDER rows are streamed from global memory two to three times), its maximum, first
//       argmax and sum of exponentials are reduced with wave shuffles (+ LDS across the four waves of a block), and with a gradient the
//       same registers give dz.  Per-row results go to the workspace and ONE block adds them in a fixed order (fp64): no atomics, two
//       runs give the same bytes.
//   (b) the angular-margin head, m = 4, gamma = 0 = AngleLinear + AngleLoss (models/spherenet.py:24-98) restated so that phi(theta) is
//       evaluated in the target column only:  what = w / |w_j|,  z = x . what,  f = z except f[i][t_i] = (1 - s) z + s |x_i| phi_i,
//       loss = CE(f, t); backward: dz = df except dz[i][t_i] = df ((1 - s) + s phi'), r_i = df s (phi - c phi'),
//       gx = dz . what^T + r_i x_i / |x_i|,  G = x^T . dz,  gw_j = (G_j - what_j (what_j . G_j)) / |w_j|.
//       The three products are the library's linear GEMMs with `what` read as an (out = D, in = C) weight: x . what has the operand
//       roles of cpg_linear_dgrad, dz . what^T those of cpg_linear_fwd, x^T . dz those of cpg_linear_wgrad.  New here: the column
//       norms, the column scale, the per-row margin pass (one wave per row), the dz / r fix-up and the tangent projection of G.
// Caller's stream, no allocation, no floating-point atomics; the planners below size the workspace AND lay it out for the launches.
#include <algorithm>
#include "cpg_common.h"

using namespace cpg;

namespace {

constexpr int XE_WAVE_VPT = 8;      // classes per lane of the one-wave-per-row kernel (<= 512 classes)
constexpr int XE_BLOCK_VPT = 32;    // classes per thread of the one-block-per-row kernel (<= 8 192 classes)

__device__ __forceinline__ float wave_sum(float v) {       // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// running maximum with the FIRST index that attains it (torch.max(1)[1]); a NaN never becomes the maximum
struct Best {
    float v;
    int i;
};
__device__ __forceinline__ Best better(Best a, Best b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

// sum of `v` over the 256 threads of a block in a fixed order (every thread returns it)
__device__ __forceinline__ double block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

__device__ __forceinline__ bool target_ok(int64_t t, int C) { return t >= 0 && t < (int64_t)C; }

// wsum[0] = W = sum_i cw[t_i] over the rows whose target lies in [0, C) (cw == null: their number)
__global__ __launch_bounds__(256) void k_xent_wsum(const int64_t *__restrict__ target, const float *__restrict__ cw, float *__restrict__ wsum,
                                                   int B, int C) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const int64_t t = target[i];
        if (target_ok(t, C)) acc += cw ? (double)cw[t] : 1.0;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) wsum[0] = (float)acc;
}

// WPR waves share a row (1: four rows per block, 4: one row per block); VPT > 0: the row in VPT registers per thread, 0: streamed.
// rowstat[row] = {cw[t] * nll, argmax == t}; GRAD: dz[row][:] = g * cw[t] / W * (softmax - onehot), exactly 0 for a row without a target.
template <int WPR, int VPT, bool GRAD>
__global__ __launch_bounds__(256) void k_xent_rows(const float *__restrict__ z, const int64_t *__restrict__ target, const float *__restrict__ cw,
                                                   const float *__restrict__ gscale, const float *__restrict__ wsum,
                                                   float *__restrict__ rowstat, float *__restrict__ dz, int B, int C) {
    constexpr int TPR = 64 * WPR;
    __shared__ float s_max[4], s_sum[4];
    __shared__ int s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = WPR == 1 ? (int64_t)blockIdx.x * 4 + wave : (int64_t)blockIdx.x;
    const int tr = WPR == 1 ? lane : tid;
    if (WPR == 1 && row >= B) return;                 // whole waves leave; this path has no barrier
    const float *zr = z + row * C;
    float v[VPT > 0 ? VPT : 1];
    if constexpr (VPT > 0) {
#pragma unroll
        for (int q = 0; q < VPT; ++q) {
            const int j = tr + q * TPR;
            v[q] = j < C ? zr[j] : 0.0f;
        }
    }
    auto for_each = [&](auto f) {                      // f(value slot, class) over this thread's classes
        if constexpr (VPT > 0) {
#pragma unroll
            for (int q = 0; q < VPT; ++q) {
                const int j = tr + q * TPR;
                if (j < C) f(v[q], j);
            }
        } else {
            for (int j = tr; j < C; j += TPR) {
                float x = zr[j];
                f(x, j);
            }
        }
    };

    Best best{-INFINITY, INT32_MAX};
    for_each([&](float &x, int j) { best = better(best, Best{x, j}); });
#pragma unroll
    for (int o = 32; o; o >>= 1) best = better(best, Best{__shfl_xor(best.v, o), __shfl_xor(best.i, o)});
    if constexpr (WPR > 1) {
        if (lane == 0) s_max[wave] = best.v, s_idx[wave] = best.i;
        __syncthreads();
        best = Best{s_max[0], s_idx[0]};
#pragma unroll
        for (int k = 1; k < 4; ++k) best = better(best, Best{s_max[k], s_idx[k]});
    }
    const float m = best.v;

    float sum = 0.0f;
    for_each([&](float &x, int) { x = expf(x - m), sum += x; });          // (register path: the slot now holds the exponential)
    sum = wave_sum(sum);
    if constexpr (WPR > 1) {
        if (lane == 0) s_sum[wave] = sum;
        __syncthreads();
        sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    }

    const int64_t t = target[row];
    const bool ok = target_ok(t, C);
    const float wt = ok ? (cw ? cw[t] : 1.0f) : 0.0f;
    if (tr == 0) {
        const float nll = ok ? logf(sum) + (m - zr[t]) : 0.0f;
        rowstat[2 * row] = ok ? wt * nll : 0.0f;
        rowstat[2 * row + 1] = (ok && best.i == (int)t) ? 1.0f : 0.0f;
    }
    if constexpr (GRAD) {
        float *dr = dz + row * C;
        if (!ok) {
            for (int j = tr; j < C; j += TPR) dr[j] = 0.0f;
            return;
        }
        const float coef = (gscale ? gscale[0] : 1.0f) * wt / wsum[0];
        const int tj = (int)t;
        for_each([&](float &x, int j) {
            const float e = VPT > 0 ? x : expf(x - m);
            dr[j] = coef * (e / sum - (j == tj ? 1.0f : 0.0f));
        });
    }
}

// out: loss = sum_i rowstat[i][0] / W, correct = sum_i rowstat[i][1]
__global__ __launch_bounds__(256) void k_xent_final(const float *__restrict__ rowstat, const float *__restrict__ wsum, float *__restrict__ loss,
                                                    float *__restrict__ correct, int B) {
    __shared__ double red[256];
    double a = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) a += (double)rowstat[2 * (int64_t)i], c += (double)rowstat[2 * (int64_t)i + 1];
    a = block_sum(a, red);
    c = block_sum(c, red);
    if (threadIdx.x == 0) {
        loss[0] = (float)(a / (double)wsum[0]);
        correct[0] = (float)c;
    }
}

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

struct XentPlan {
    size_t off_rowstat, bytes;       // the workspace: W at its head, then rowstat[B][2]
};
XentPlan xent_plan(int B) {
    XentPlan p;
    p.off_rowstat = 256;
    p.bytes = p.off_rowstat + round256((size_t)B * 2 * sizeof(float));
    return p;
}

int xent_run(const float *z, const int64_t *target, const float *cw, const float *gscale, int B, int C, float *loss, float *correct, float *dz,
             void *ws, size_t ws_bytes, hipStream_t stream, const char *what) {
    const XentPlan p = xent_plan(B);
    if (ws == nullptr || ws_bytes < p.bytes || (((uintptr_t)ws) & 15) != 0)
        return fail(CPG_E_WORKSPACE, "%s: workspace %zu < %zu bytes (or not 16-byte aligned)", what, ws_bytes, p.bytes);
    float *wsum = (float *)ws, *rowstat = (float *)((char *)ws + p.off_rowstat);
    hipLaunchKernelGGL(k_xent_wsum, dim3(1), dim3(256), 0, stream, target, cw, wsum, B, C);
#define XE_LAUNCH(WPR_, VPT_, GRID_)                                                                                                   \
    do {                                                                                                                               \
        if (dz) {                                                                                                                      \
            hipLaunchKernelGGL((k_xent_rows<WPR_, VPT_, true>), dim3((unsigned)(GRID_)), dim3(256), 0, stream, z, target, cw, gscale,  \
                               wsum, rowstat, dz, B, C);                                                                               \
        } else {                                                                                                                       \
            hipLaunchKernelGGL((k_xent_rows<WPR_, VPT_, false>), dim3((unsigned)(GRID_)), dim3(256), 0, stream, z, target, cw, gscale, \
                               wsum, rowstat, dz, B, C);                                                                               \
        }                                                                                                                              \
    } while (0)
    if (C <= 64 * XE_WAVE_VPT) XE_LAUNCH(1, XE_WAVE_VPT, (B + 3) / 4);
    else if (C <= 256 * XE_BLOCK_VPT) XE_LAUNCH(4, XE_BLOCK_VPT, B);
    else XE_LAUNCH(4, 0, B);
#undef XE_LAUNCH
    if (loss) hipLaunchKernelGGL(k_xent_final, dim3(1), dim3(256), 0, stream, rowstat, wsum, loss, correct, B);      // (null: gradient only)
    CPG_CHECK_LAUNCH(what);
    return CPG_OK;
}

// ---- angular-margin head -------------------------------------------------------------------------------------------------------------------

// part[split][j] = sum over the split's rows d of a[d][j] * b[d][j] (a == b: squared column norms); 64 columns x 4 row phases per block
__global__ __launch_bounds__(256) void k_col_dot_partial(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ part, int D,
                                                         int C, int rows_per_split) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + cl;
    const int d0 = blockIdx.y * rows_per_split, d1 = min(D, d0 + rows_per_split);
    float acc = 0.0f;
    if (j < C)
        for (int d = d0 + rl; d < d1; d += 4) acc = fmaf(a[(int64_t)d * C + j], b[(int64_t)d * C + j], acc);
    red[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && j < C) part[(int64_t)blockIdx.y * C + j] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

__device__ __forceinline__ float col_total(const float *__restrict__ part, int nsplit, int C, int64_t j) {
    float s = part[j];
    for (int k = 1; k < nsplit; ++k) s += part[(int64_t)k * C + j];
    return s;
}

constexpr int COL_ROWS = 16;        // rows per thread of the two column passes below

// what[d][j] = w[d][j] / n_j, n_j = sqrt(sum of the partial squared norms); colnorm[j] = n_j
__global__ __launch_bounds__(256) void k_col_normalize(const float *__restrict__ w, const float *__restrict__ part, int nsplit,
                                                       float *__restrict__ what, float *__restrict__ colnorm, int D, int C) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= C) return;
    const float n = sqrtf(col_total(part, nsplit, C, j));
    if (blockIdx.y == 0) colnorm[j] = n;
    const int d0 = blockIdx.y * COL_ROWS, d1 = min(D, d0 + COL_ROWS);
    for (int d = d0; d < d1; ++d) what[(int64_t)d * C + j] = w[(int64_t)d * C + j] / n;
}

// gw[d][j] = (gw[d][j] - what[d][j] * dot_j) / n_j in place, dot_j = what_j . G_j from the partial sums
__global__ __launch_bounds__(256) void k_col_project(const float *__restrict__ what, const float *__restrict__ part, int nsplit,
                                                     const float *__restrict__ colnorm, float *__restrict__ gw, int D, int C) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= C) return;
    const float dot = col_total(part, nsplit, C, j), n = colnorm[j];
    const int d0 = blockIdx.y * COL_ROWS, d1 = min(D, d0 + COL_ROWS);
    for (int d = d0; d < d1; ++d) {
        const int64_t e = (int64_t)d * C + j;
        gw[e] = (gw[e] - what[e] * dot) / n;
    }
}

// One wave per row: |x_i|, c = clamp(z_iy / |x_i|), k = floor(4 acos(c) / 3.14159265), phi = (-1)^k (8 c^4 - 8 c^2 + 1) - 2 k,
// phi' = (-1)^k (32 c^3 - 16 c) (0 where the clamp bit); f_iy = (1 - s) z_iy + s |x_i| phi.  saved[i] = {|x_i|, c, phi, phi'}.
// A row whose target is outside [0, C) keeps f = z (the cross-entropy gives it weight 0).
__global__ __launch_bounds__(256) void k_margin_fwd(const float *__restrict__ x, const int64_t *__restrict__ target, float *__restrict__ f,
                                                    float *__restrict__ saved, float s, int B, int D, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float *xr = x + row * D;
    float acc = 0.0f;
    for (int d = lane; d < D; d += 64) acc = fmaf(xr[d], xr[d], acc);
    const float xlen = sqrtf(wave_sum(acc));
    if (lane != 0) return;
    const int64_t t = target[row];
    float c = 0.0f, phi = 0.0f, dphi = 0.0f;
    if (target_ok(t, C)) {
        const float zt = f[row * C + t], q = zt / xlen;
        c = fminf(fmaxf(q, -1.0f), 1.0f);
        const float k = floorf(4.0f * acosf(c) / 3.14159265f);
        const float sign = ((int)k & 1) ? -1.0f : 1.0f, c2 = c * c;
        phi = sign * (8.0f * c2 * c2 - 8.0f * c2 + 1.0f) - 2.0f * k;
        dphi = (q >= -1.0f && q <= 1.0f) ? sign * (32.0f * c2 * c - 16.0f * c) : 0.0f;
        f[row * C + t] = (1.0f - s) * zt + s * xlen * phi;
    }
    float *sv = saved + 4 * row;
    sv[0] = xlen, sv[1] = c, sv[2] = phi, sv[3] = dphi;
}

// One thread per row: dz_iy = df_iy ((1 - s) + s phi'), rr_i = df_iy s (phi - c phi') / |x_i| (the factor of x_i in gx_i)
__global__ __launch_bounds__(256) void k_margin_bwd(const int64_t *__restrict__ target, const float *__restrict__ saved, float *__restrict__ df,
                                                    float *__restrict__ rr, float s, int B, int C) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= B) return;
    const int64_t t = target[row];
    float r = 0.0f;
    if (target_ok(t, C)) {
        const float *sv = saved + 4 * row;
        const float xlen = sv[0], c = sv[1], phi = sv[2], dphi = sv[3], dfy = df[row * C + t];
        df[row * C + t] = dfy * ((1.0f - s) + s * dphi);
        r = dfy * s * (phi - c * dphi) / xlen;
    }
    rr[row] = r;
}

// gx[i][d] += rr[i] * x[i][d]
__global__ __launch_bounds__(256) void k_add_radial(const float *__restrict__ x, const float *__restrict__ rr, float *__restrict__ gx, int64_t total,
                                                    int D) {
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += nthreads) gx[e] = fmaf(rr[e / D], x[e], gx[e]);
}

struct HeadPlan {
    int nsplit, rows_per_split;      // row splits of the column reductions
    size_t off_part, off_df, off_rr, off_xent, off_lin, lin_bytes, bytes;
};
HeadPlan head_plan(int B, int D, int C) {
    HeadPlan p;
    p.rows_per_split = std::max(64, ((D + 15) / 16 + 3) / 4 * 4);       // <= 16 splits of >= 64 rows
    p.nsplit = (D + p.rows_per_split - 1) / p.rows_per_split;
    p.off_part = 0;
    p.off_df = p.off_part + round256((size_t)p.nsplit * C * sizeof(float));
    p.off_rr = p.off_df + round256((size_t)B * C * sizeof(float));
    p.off_xent = p.off_rr + round256((size_t)B * sizeof(float));
    p.off_lin = p.off_xent + xent_plan(B).bytes;
    p.lin_bytes = round256(cpg_linear_workspace_bytes(B, C, D));
    p.bytes = p.off_lin + p.lin_bytes;
    return p;
}

int head_check(const char *what, const void *ws, size_t ws_bytes, const HeadPlan &p) {
    if (ws == nullptr || ws_bytes < p.bytes || (((uintptr_t)ws) & 15) != 0)
        return fail(CPG_E_WORKSPACE, "%s: workspace %zu < %zu bytes (or not 16-byte aligned)", what, ws_bytes, p.bytes);
    return CPG_OK;
}

}  // namespace

extern "C" size_t cpg_loss_heads_workspace_bytes(int32_t B, int32_t D, int32_t C) {
    if (B <= 0 || C <= 0 || D < 0) return 0;
    return D == 0 ? xent_plan(B).bytes : head_plan(B, D, C).bytes;
}

extern "C" int cpg_softmax_xent_fwd(const float *logits, const int64_t *target, const float *class_weight, int32_t B, int32_t C, float *loss,
                                    float *correct, void *ws, size_t ws_bytes, void *stream) {
    CPG_REQUIRE(logits && target && loss && correct && B > 0 && C > 0, "cpg_softmax_xent_fwd: bad argument");
    return xent_run(logits, target, class_weight, nullptr, B, C, loss, correct, nullptr, ws, ws_bytes, (hipStream_t)stream,
                    "cpg_softmax_xent_fwd");
}

extern "C" int cpg_softmax_xent_fwd_bwd(const float *logits, const int64_t *target, const float *class_weight, const float *gscale, int32_t B,
                                        int32_t C, float *loss, float *correct, float *dlogits, void *ws, size_t ws_bytes, void *stream) {
    CPG_REQUIRE(logits && target && dlogits && (loss == nullptr) == (correct == nullptr) && B > 0 && C > 0,
                "cpg_softmax_xent_fwd_bwd: bad argument");
    return xent_run(logits, target, class_weight, gscale, B, C, loss, correct, dlogits, ws, ws_bytes, (hipStream_t)stream,
                    "cpg_softmax_xent_fwd_bwd");
}

#define HEAD_REQUIRE_MARGIN(name)                                                                                                          \
    CPG_REQUIRE(m == 4 && gamma == 0.0f, name ": only m = 4 and gamma = 0 are implemented (got m = %d, gamma = %g)", (int)m, (double)gamma); \
    CPG_REQUIRE(lamb >= 0.0, name ": lambda must be >= 0")

extern "C" int cpg_angle_head_fwd(const float *x, const float *w, const int64_t *target, int32_t B, int32_t D, int32_t C, int32_t m, float gamma,
                                  double lamb, float *what, float *colnorm, float *f, float *saved, float *loss, float *correct, void *ws,
                                  size_t ws_bytes, void *stream) {
    HEAD_REQUIRE_MARGIN("cpg_angle_head_fwd");
    CPG_REQUIRE(x && w && target && what && colnorm && f && saved && loss && correct && B > 0 && D > 0 && C > 0,
                "cpg_angle_head_fwd: bad argument");
    const HeadPlan p = head_plan(B, D, C);
    if (int rc = head_check("cpg_angle_head_fwd", ws, ws_bytes, p)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)ws;
    float *part = (float *)(base + p.off_part);
    const float s = (float)(1.0 / (1.0 + lamb));
    hipLaunchKernelGGL(k_col_dot_partial, dim3((unsigned)((C + 63) / 64), (unsigned)p.nsplit), dim3(256), 0, st, w, w, part, D, C, p.rows_per_split);
    hipLaunchKernelGGL(k_col_normalize, dim3((unsigned)((C + 255) / 256), (unsigned)((D + COL_ROWS - 1) / COL_ROWS)), dim3(256), 0, st, w, part,
                       p.nsplit, what, colnorm, D, C);
    CPG_CHECK_LAUNCH("cpg_angle_head_fwd(norm)");
    // z[b][j] = sum_d x[b][d] what[d][j]: `what` as an (out = D, in = C) weight, x in the place of the output gradient
    if (int rc = cpg_linear_dgrad(x, what, nullptr, 0.0f, f, B, C, D, base + p.off_lin, p.lin_bytes, stream)) return rc;
    hipLaunchKernelGGL(k_margin_fwd, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, x, target, f, saved, s, B, D, C);
    CPG_CHECK_LAUNCH("cpg_angle_head_fwd(margin)");
    return xent_run(f, target, nullptr, nullptr, B, C, loss, correct, nullptr, base + p.off_xent, xent_plan(B).bytes, st, "cpg_angle_head_fwd");
}

extern "C" int cpg_angle_head_bwd(const float *x, const float *what, const float *colnorm, const float *f, const float *saved,
                                  const int64_t *target, const float *gscale, int32_t B, int32_t D, int32_t C, int32_t m, float gamma, double lamb,
                                  float *gx, float *gw, void *ws, size_t ws_bytes, void *stream) {
    HEAD_REQUIRE_MARGIN("cpg_angle_head_bwd");
    CPG_REQUIRE(x && what && colnorm && f && saved && target && gx && gw && B > 0 && D > 0 && C > 0, "cpg_angle_head_bwd: bad argument");
    const HeadPlan p = head_plan(B, D, C);
    if (int rc = head_check("cpg_angle_head_bwd", ws, ws_bytes, p)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)ws;
    float *part = (float *)(base + p.off_part), *df = (float *)(base + p.off_df), *rr = (float *)(base + p.off_rr);
    const float s = (float)(1.0 / (1.0 + lamb));
    if (int rc = xent_run(f, target, nullptr, gscale, B, C, nullptr, nullptr, df, base + p.off_xent, xent_plan(B).bytes, st, "cpg_angle_head_bwd"))
        return rc;
    hipLaunchKernelGGL(k_margin_bwd, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, target, saved, df, rr, s, B, C);
    CPG_CHECK_LAUNCH("cpg_angle_head_bwd(margin)");
    // gx[b][d] = sum_j dz[b][j] what[d][j]: the forward of that (out = D, in = C) layer on dz
    if (int rc = cpg_linear_fwd(df, what, nullptr, 0.0f, nullptr, gx, B, C, D, base + p.off_lin, p.lin_bytes, stream)) return rc;
    hipLaunchKernelGGL(k_add_radial, dim3(stream_grid((int64_t)B * D, 256)), dim3(256), 0, st, x, rr, gx, (int64_t)B * D, D);
    // G[d][j] = sum_b x[b][d] dz[b][j]: its weight gradient, x in the place of the output gradient
    if (int rc = cpg_linear_wgrad(df, x, nullptr, nullptr, 0.0f, gw, nullptr, nullptr, B, C, D, base + p.off_lin, p.lin_bytes, stream)) return rc;
    hipLaunchKernelGGL(k_col_dot_partial, dim3((unsigned)((C + 63) / 64), (unsigned)p.nsplit), dim3(256), 0, st, what, gw, part, D, C,
                       p.rows_per_split);
    hipLaunchKernelGGL(k_col_project, dim3((unsigned)((C + 255) / 256), (unsigned)((D + COL_ROWS - 1) / COL_ROWS)), dim3(256), 0, st, what, part,
                       p.nsplit, colnorm, gw, D, C);
    CPG_CHECK_LAUNCH("cpg_angle_head_bwd(project)");
    return CPG_OK;
}
