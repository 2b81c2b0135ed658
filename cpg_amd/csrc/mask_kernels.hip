// HBM-bound mask / gradient-routing kernels (K1, K4e, K7, K8 of SURVEY.md section 2).
// Each is a single streaming pass: 16 B per lane per access for fp32, 4 owner bytes as one
// dword, grid capped at 8 blocks per CU with a grid-stride loop.  gfx950 only.
#include <cmath>
#include "cpg_common.h"

using namespace cpg;

namespace {

constexpr int kThreads = 256;

struct alignas(16) F4 { float x, y, z, w; };

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
inline bool aligned4(const void *p) { return (((uintptr_t)p) & 3) == 0; }

// ---------------------------------------------------------------- K1
__global__ __launch_bounds__(kThreads) void k_binarize_mul(const float *__restrict__ w,
                                                           const float *__restrict__ pm, float thr,
                                                           float *__restrict__ out, int64_t n, int vec_ok) {
    // w == nullptr: plain Binarizer (out = bin(pm)); else out = w * bin(pm)
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    const bool has_w = (w != nullptr);
    if (vec_ok) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += nthreads) {
            const F4 m = reinterpret_cast<const F4 *>(pm)[i];
            F4 r = {binarize(m.x, thr), binarize(m.y, thr), binarize(m.z, thr), binarize(m.w, thr)};
            if (has_w) {
                const F4 a = reinterpret_cast<const F4 *>(w)[i];
                r = F4{a.x * r.x, a.y * r.y, a.z * r.z, a.w * r.w};
            }
            reinterpret_cast<F4 *>(out)[i] = r;
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += nthreads) out[i] = (has_w ? w[i] : 1.0f) * binarize(pm[i], thr);
    } else {
        for (int64_t i = tid; i < n; i += nthreads) out[i] = (has_w ? w[i] : 1.0f) * binarize(pm[i], thr);
    }
}

// ---------------------------------------------------------------- K4e
// utils/prune.py:203-210 in one pass.  MODE: 0 finetune, 1 prune.
template <bool HAS_PM>
__global__ __launch_bounds__(kThreads) void k_route(float *__restrict__ gw, const float *__restrict__ w,
                                                    const uint8_t *__restrict__ owner, int cur, float wd,
                                                    float *__restrict__ gpm, int mode, int64_t n, int vec_ok) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    auto route1 = [&](int64_t i) {
        const int o = owner[i];
        gw[i] = (o == cur) ? fmaf(wd, w[i], gw[i]) : 0.0f;
        if (HAS_PM) {
            if (mode == CPG_MODE_PRUNE || o == 0 || o >= cur) gpm[i] = 0.0f;
        }
    };
    if (vec_ok) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += nthreads) {
            const uint32_t o4 = reinterpret_cast<const uint32_t *>(owner)[i];
            const int o0 = o4 & 255, o1 = (o4 >> 8) & 255, o2 = (o4 >> 16) & 255, o3 = o4 >> 24;
            F4 g = {0.f, 0.f, 0.f, 0.f};
            if (o0 == cur || o1 == cur || o2 == cur || o3 == cur) {      // frozen quads: no gw / w read at all
                const F4 gi = reinterpret_cast<const F4 *>(gw)[i];
                const F4 wi = reinterpret_cast<const F4 *>(w)[i];
                g.x = (o0 == cur) ? fmaf(wd, wi.x, gi.x) : 0.0f;
                g.y = (o1 == cur) ? fmaf(wd, wi.y, gi.y) : 0.0f;
                g.z = (o2 == cur) ? fmaf(wd, wi.z, gi.z) : 0.0f;
                g.w = (o3 == cur) ? fmaf(wd, wi.w, gi.w) : 0.0f;
            }
            reinterpret_cast<F4 *>(gw)[i] = g;
            if (HAS_PM) {
                if (mode == CPG_MODE_PRUNE) {
                    reinterpret_cast<F4 *>(gpm)[i] = F4{0.f, 0.f, 0.f, 0.f};
                } else {
                    const bool z0 = (o0 == 0 || o0 >= cur), z1 = (o1 == 0 || o1 >= cur);
                    const bool z2 = (o2 == 0 || o2 >= cur), z3 = (o3 == 0 || o3 >= cur);
                    if (z0 || z1 || z2 || z3) {
                        F4 p = {0.f, 0.f, 0.f, 0.f};
                        if (!(z0 && z1 && z2 && z3)) {
                            p = reinterpret_cast<const F4 *>(gpm)[i];
                            if (z0) p.x = 0.f;
                            if (z1) p.y = 0.f;
                            if (z2) p.z = 0.f;
                            if (z3) p.w = 0.f;
                        }
                        reinterpret_cast<F4 *>(gpm)[i] = p;
                    }
                }
            }
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += nthreads) route1(i);
    } else {
        for (int64_t i = tid; i < n; i += nthreads) route1(i);
    }
}

// ---------------------------------------------------------------- K7
// Owner-id histogram.  Owner ids take very few distinct values per layer, so plain LDS atomics
// would serialise 64-way on one bin; instead each wave peels off one distinct value per
// iteration with readfirstlane + ballot + popcount and issues ONE LDS atomic for it.
__device__ __forceinline__ void wave_count_byte(unsigned v, unsigned *hist_lds) {
    for (;;) {
        const unsigned u = __builtin_amdgcn_readfirstlane(v);
        const unsigned long long m = __ballot(v == u);
        if (v == u) {
            const int first = __ffsll((long long)m) - 1;
            if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist_lds[u], (unsigned)__popcll(m));
            break;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_mask_hist(const uint8_t *__restrict__ owner,
                                                        const float *__restrict__ pm, int idx, int64_t n,
                                                        unsigned long long *__restrict__ hist, int vec_ok) {
    __shared__ unsigned h[257];
    for (int i = threadIdx.x; i < 257; i += kThreads) h[i] = 0;
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    unsigned shared_cnt = 0;
    const float pick_thr = 0.005f;                 // literal of utils/prune.py:188
    if (vec_ok) {
        const int64_t n4 = n >> 2;
        // all lanes of a wave iterate together (uniform trip count) so ballots see whole waves
        const int64_t iters = (n4 + nthreads - 1) / nthreads;
        for (int64_t it = 0; it < iters; ++it) {
            const int64_t i = tid + it * nthreads;
            if (i < n4) {
                const uint32_t o4 = reinterpret_cast<const uint32_t *>(owner)[i];
                if (pm != nullptr) {
                    const bool a0 = (o4 & 255) > 0 && (int)(o4 & 255) < idx;
                    const bool a1 = ((o4 >> 8) & 255) > 0 && (int)((o4 >> 8) & 255) < idx;
                    const bool a2 = ((o4 >> 16) & 255) > 0 && (int)((o4 >> 16) & 255) < idx;
                    const bool a3 = (o4 >> 24) > 0 && (int)(o4 >> 24) < idx;
                    if (a0 || a1 || a2 || a3) {
                        const F4 p = reinterpret_cast<const F4 *>(pm)[i];
                        shared_cnt += (a0 && p.x > pick_thr) + (a1 && p.y > pick_thr) + (a2 && p.z > pick_thr) +
                                      (a3 && p.w > pick_thr);
                    }
                }
                wave_count_byte(o4 & 255, h);
                wave_count_byte((o4 >> 8) & 255, h);
                wave_count_byte((o4 >> 16) & 255, h);
                wave_count_byte(o4 >> 24, h);
            }
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += nthreads) {
            const unsigned o = owner[i];
            atomicAdd(&h[o], 1u);
            if (pm != nullptr && o > 0 && (int)o < idx && pm[i] > pick_thr) shared_cnt++;
        }
    } else {
        for (int64_t i = tid; i < n; i += nthreads) {
            const unsigned o = owner[i];
            atomicAdd(&h[o], 1u);
            if (pm != nullptr && o > 0 && (int)o < idx && pm[i] > pick_thr) shared_cnt++;
        }
    }
    if (shared_cnt) atomicAdd(&h[256], shared_cnt);
    __syncthreads();
    for (int i = threadIdx.x; i < 257; i += kThreads)
        if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// ---------------------------------------------------------------- K8
// zero w where owner == 0 (zero_pruned) or additionally owner > idx (apply_mask, idx < 256)
__global__ __launch_bounds__(kThreads) void k_zero_by_owner(float *__restrict__ w, const uint8_t *__restrict__ owner,
                                                            int idx, int64_t n, int vec_ok) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    auto dead = [idx](int o) { return o == 0 || o > idx; };
    if (vec_ok) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += nthreads) {
            const uint32_t o4 = reinterpret_cast<const uint32_t *>(owner)[i];
            const bool d0 = dead(o4 & 255), d1 = dead((o4 >> 8) & 255), d2 = dead((o4 >> 16) & 255), d3 = dead(o4 >> 24);
            if (d0 && d1 && d2 && d3) {
                reinterpret_cast<F4 *>(w)[i] = F4{0.f, 0.f, 0.f, 0.f};
            } else if (d0 || d1 || d2 || d3) {
                F4 v = reinterpret_cast<const F4 *>(w)[i];
                if (d0) v.x = 0.f;
                if (d1) v.y = 0.f;
                if (d2) v.z = 0.f;
                if (d3) v.w = 0.f;
                reinterpret_cast<F4 *>(w)[i] = v;
            }
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += nthreads)
            if (dead(owner[i])) w[i] = 0.0f;
    } else {
        for (int64_t i = tid; i < n; i += nthreads)
            if (dead(owner[i])) w[i] = 0.0f;
    }
}

__global__ __launch_bounds__(kThreads) void k_claim_free(uint8_t *__restrict__ owner, unsigned new_idx, int64_t n,
                                                         int vec_ok) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    if (vec_ok) {
        const int64_t n16 = n >> 4;
        for (int64_t i = tid; i < n16; i += nthreads) {
            uint4 v = reinterpret_cast<const uint4 *>(owner)[i];
            auto fix = [new_idx](uint32_t x) {
                // bytes that are zero -> new_idx.  exact zero-byte detect (no borrow artefacts)
                uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
                t = ~(t | x | 0x7F7F7F7Fu);            // 0x80 in every zero byte
                return x | ((t >> 7) * new_idx);
            };
            const uint4 r = {fix(v.x), fix(v.y), fix(v.z), fix(v.w)};
            if (r.x != v.x || r.y != v.y || r.z != v.z || r.w != v.w) reinterpret_cast<uint4 *>(owner)[i] = r;
        }
        for (int64_t i = (n16 << 4) + tid; i < n; i += nthreads)
            if (owner[i] == 0) owner[i] = (uint8_t)new_idx;
    } else {
        for (int64_t i = tid; i < n; i += nthreads)
            if (owner[i] == 0) owner[i] = (uint8_t)new_idx;
    }
}

// ---------------------------------------------------------------- the walk of the two fused optimizer passes
// float4 body plus scalar tail over the elements [begin, end) of one layer: `quad(i)` handles elements 4i .. 4i+3, `single(i)`
// element i; this thread takes index `first` of every `stride`.  begin is a multiple of 4.  Serves the grid-stride per-layer
// kernels (0, n, global thread id, threads of the grid) and the block-per-chunk multi kernels (chunk, threadIdx.x, kThreads).
template <class Quad, class Single>
__device__ __forceinline__ void walk4(int64_t begin, int64_t end, int64_t first, int64_t stride, int vec_ok, Quad quad, Single single) {
    if (vec_ok) {
        const int64_t e4 = end >> 2;
        for (int64_t i = (begin >> 2) + first; i < e4; i += stride) quad(i);
        for (int64_t i = (e4 << 2) + first; i < end; i += stride) single(i);
    } else {
        for (int64_t i = begin + first; i < end; i += stride) single(i);
    }
}

// ---------------------------------------------------------------- fused masked SGD
// utils/prune.py:203-205 + torch.optim.SGD(momentum, nesterov, dampening 0, weight_decay 0) in ONE pass:
//   g   = owner == cur ? gw + wd * w : 0            (gradient routing; written back so .grad is what the reference leaves)
//   buf = first ? g : momentum * buf + g            (two roundings, as torch's _foreach_mul_ / _foreach_add_)
//   d   = nesterov ? g + momentum * buf : buf
//   w  -= lr * d
// 13 B read + 12 B written per element instead of the 13 + 36 B of the routing pass plus torch's three foreach passes.
// ZERO (the PackNet step, utils/packnet_prune.py:146-171 + utils/packnet_manager.py:69): the weight of a slot nobody owns is pinned to
// +0.0f in the same store (make_pruned_zero after every step); its gradient and momentum are written as above -- the reference's
// momentum keeps decaying on pruned slots.
struct SgdHyper {
    int cur;
    float wd, lr, momentum;
    int nesterov, first;
};

template <bool ZERO>
__device__ __forceinline__ void sgd_route_one(float &wv, float &gv, float &bv, int o, const SgdHyper h) {
    const float g = (o == h.cur) ? fmaf(h.wd, wv, gv) : 0.0f;
    const float b = h.first ? g : __fadd_rn(__fmul_rn(h.momentum, bv), g);
    const float d = h.nesterov ? fmaf(h.momentum, b, g) : b;
    wv = (ZERO && o == 0) ? 0.0f : fmaf(-h.lr, d, wv);
    gv = g;
    bv = b;
}

// (The span functions take plain pointers and the hyper-parameters by value: the per-layer kernels' __restrict__ parameters carry
// through the inlining, and the multi kernels, whose pointers come out of the argument struct, keep the schedule and the register
// count they had before the two forms shared this code -- with __restrict__ here k_adam_route_multi goes from 56 to 85 VGPRs.)
template <bool ZERO>
__device__ __forceinline__ void sgd_route_span(float *w, float *gw, float *buf, const uint8_t *owner, int64_t begin, int64_t end,
                                               int64_t first, int64_t stride, int vec_ok, const SgdHyper h) {
    walk4(begin, end, first, stride, vec_ok,
          [&](int64_t i) {
              const uint32_t o4 = reinterpret_cast<const uint32_t *>(owner)[i];
              F4 wv = reinterpret_cast<F4 *>(w)[i], gv = reinterpret_cast<F4 *>(gw)[i];
              F4 bv = h.first ? F4{0.f, 0.f, 0.f, 0.f} : reinterpret_cast<F4 *>(buf)[i];
              sgd_route_one<ZERO>(wv.x, gv.x, bv.x, o4 & 255, h);
              sgd_route_one<ZERO>(wv.y, gv.y, bv.y, (o4 >> 8) & 255, h);
              sgd_route_one<ZERO>(wv.z, gv.z, bv.z, (o4 >> 16) & 255, h);
              sgd_route_one<ZERO>(wv.w, gv.w, bv.w, o4 >> 24, h);
              reinterpret_cast<F4 *>(w)[i] = wv;
              reinterpret_cast<F4 *>(gw)[i] = gv;
              reinterpret_cast<F4 *>(buf)[i] = bv;
          },
          [&](int64_t i) {
              float bv = h.first ? 0.f : buf[i];
              sgd_route_one<ZERO>(w[i], gw[i], bv, owner[i], h);
              buf[i] = bv;
          });
}

template <bool ZERO>
__global__ __launch_bounds__(kThreads) void k_sgd_route(float *__restrict__ w, float *__restrict__ gw, float *__restrict__ buf,
                                                        const uint8_t *__restrict__ owner, int cur, float wd, float lr,
                                                        float momentum, int nesterov, int first, int64_t n, int vec_ok) {
    sgd_route_span<ZERO>(w, gw, buf, owner, 0, n, (int64_t)blockIdx.x * kThreads + threadIdx.x, (int64_t)gridDim.x * kThreads, vec_ok,
                         SgdHyper{cur, wd, lr, momentum, nesterov, first});
}

// Fused piggymask step (CPG_cifar100_main_normal.py:342-346 Adam on the piggymasks + utils/prune.py:206-210 routing):
//   g   = finetune: (owner == 0 || owner >= cur) ? 0 : gpm ; prune: 0        (only older tasks' slots learn to be picked)
//   m   = m + (1 - beta1) * (g - m);   v = beta2 * v + (1 - beta2) * g * g    (torch.optim.Adam, amsgrad = False, wd = 0)
//   pm -= step_size * m / (sqrt(v) / sqrt(bias_correction2) + eps),  step_size = lr / bias_correction1
// and the routed g is written back to .grad.  21 B read + 16 B written per element in one pass.
struct AdamHyper {
    int cur, mode;
    float step_size, omb1, beta2, omb2, eps, bc2_sqrt;
};

__device__ __forceinline__ void adam_route_one(float &p, float &g, float &a, float &b, int o, const AdamHyper h) {
    const bool keep = h.mode == CPG_MODE_FINETUNE && o != 0 && o < h.cur;
    const float gr = keep ? g : 0.0f;
    a = fmaf(h.omb1, gr - a, a);                   // exp_avg.lerp_(grad, 1 - beta1)
    b = fmaf(h.omb2, gr * gr, h.beta2 * b);        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(b) / h.bc2_sqrt + h.eps;
    p = fmaf(-h.step_size, a / denom, p);
    g = gr;
}

__device__ __forceinline__ void adam_route_span(float *pm, float *gpm, float *m1, float *m2, const uint8_t *owner, int64_t begin, int64_t end,
                                                int64_t first, int64_t stride, int vec_ok, const AdamHyper h) {
    walk4(begin, end, first, stride, vec_ok,
          [&](int64_t i) {
              const uint32_t o4 = reinterpret_cast<const uint32_t *>(owner)[i];
              F4 pv = reinterpret_cast<F4 *>(pm)[i], gv = reinterpret_cast<F4 *>(gpm)[i];
              F4 av = reinterpret_cast<F4 *>(m1)[i], bv = reinterpret_cast<F4 *>(m2)[i];
              adam_route_one(pv.x, gv.x, av.x, bv.x, o4 & 255, h);
              adam_route_one(pv.y, gv.y, av.y, bv.y, (o4 >> 8) & 255, h);
              adam_route_one(pv.z, gv.z, av.z, bv.z, (o4 >> 16) & 255, h);
              adam_route_one(pv.w, gv.w, av.w, bv.w, o4 >> 24, h);
              reinterpret_cast<F4 *>(pm)[i] = pv;
              reinterpret_cast<F4 *>(gpm)[i] = gv;
              reinterpret_cast<F4 *>(m1)[i] = av;
              reinterpret_cast<F4 *>(m2)[i] = bv;
          },
          [&](int64_t i) { adam_route_one(pm[i], gpm[i], m1[i], m2[i], owner[i], h); });
}

__global__ __launch_bounds__(kThreads) void k_adam_route(float *__restrict__ pm, float *__restrict__ gpm, float *__restrict__ m1,
                                                         float *__restrict__ m2, const uint8_t *__restrict__ owner, int cur, int mode,
                                                         float step_size, float omb1, float beta2, float omb2, float eps, float bc2_sqrt,
                                                         int64_t n, int vec_ok) {
    adam_route_span(pm, gpm, m1, m2, owner, 0, n, (int64_t)blockIdx.x * kThreads + threadIdx.x, (int64_t)gridDim.x * kThreads, vec_ok,
                    AdamHyper{cur, mode, step_size, omb1, beta2, omb2, eps, bc2_sqrt});
}

// ---------------------------------------------------------------- multi-tensor forms of the two fused optimizer passes (ABI 3)
// One launch for up to kMultiMax layers: the per-layer pointers travel BY VALUE in the kernel arguments (no device table, no copy),
// a block owns one kChunk-element piece of one layer and finds it by walking the (block-uniform, scalar) prefix of pieces per layer.
// The arithmetic per element is sgd_route_one / adam_route_one, as in the per-layer kernels: results do not depend on how the work is cut.
constexpr int kMultiMax = 48;
constexpr int kChunk = kThreads * 16;           // elements per block: 4 float4 per thread
struct SgdItems {
    float *w[kMultiMax], *gw[kMultiMax], *buf[kMultiMax];
    const uint8_t *owner[kMultiMax];
    long long n[kMultiMax];
    int first_block[kMultiMax + 1];             // pieces before layer i; [count] = grid size
    unsigned char vec[kMultiMax];
    int count;
};
struct AdamItems {
    float *pm[kMultiMax], *gpm[kMultiMax], *m1[kMultiMax], *m2[kMultiMax];
    const uint8_t *owner[kMultiMax];
    long long n[kMultiMax];
    int first_block[kMultiMax + 1];
    unsigned char vec[kMultiMax];
    int count;
};
static_assert(sizeof(SgdItems) <= 4096 && sizeof(AdamItems) <= 4096, "kernel arguments are limited to 4 KB");

// this block's piece of the table: the layer, and [begin, end) inside it (begin is a multiple of kChunk, hence of 4)
template <class Items>
__device__ __forceinline__ int find_piece(const Items &it, int64_t &begin, int64_t &end) {
    const int block = (int)blockIdx.x;
    int i = 0;
    while (i + 1 < it.count && it.first_block[i + 1] <= block) ++i;
    begin = (int64_t)(block - it.first_block[i]) * kChunk;
    end = begin + kChunk < it.n[i] ? begin + kChunk : it.n[i];
    return i;
}

template <bool ZERO>
__global__ __launch_bounds__(kThreads) void k_sgd_route_multi(const SgdItems it, int cur, float wd, float lr, float momentum, int nesterov,
                                                              int first) {
    int64_t begin, end;
    const int item = find_piece(it, begin, end);
    sgd_route_span<ZERO>(it.w[item], it.gw[item], it.buf[item], it.owner[item], begin, end, threadIdx.x, kThreads, it.vec[item],
                         SgdHyper{cur, wd, lr, momentum, nesterov, first});
}

__global__ __launch_bounds__(kThreads) void k_adam_route_multi(const AdamItems it, int cur, int mode, float step_size, float omb1, float beta2,
                                                               float omb2, float eps, float bc2_sqrt) {
    int64_t begin, end;
    const int item = find_piece(it, begin, end);
    adam_route_span(it.pm[item], it.gpm[item], it.m1[item], it.m2[item], it.owner[item], begin, end, threadIdx.x, kThreads, it.vec[item],
                    AdamHyper{cur, mode, step_size, omb1, beta2, omb2, eps, bc2_sqrt});
}

// ---------------------------------------------------------------- STATS forms of the multi-tensor passes (step telemetry)
// The same update, element for element (sgd_route_one / adam_route_one are called, never restated), and a reduction of what the pass
// has in registers anyway into one record of kStatFields doubles per piece (include/cpg_hip.h: cpg_sgd_step_stats / cpg_pm_step_stats).
// Separate kernels: the plain ones above keep their registers and their schedule.  Three stages, no atomics anywhere, so a record is
// bit-reproducible:  thread (sums in fp64 -- the square of an fp32 value is exact there --, maxima fp32, counts integers; the
// thread's elements in ascending order)  ->  block (xor butterfly over the wave, then the four waves in order through LDS; one
// record per piece, plain stores to partials[piece])  ->  k_step_stats_finalize (one wave per item: lane l adds pieces l, l + 64, ...,
// then the same butterfly) and k_step_health (the sticky record).
constexpr int kStatFields = 8;
constexpr unsigned kSgdMaxFields = (1u << 3) | (1u << 7);       // g_absmax, w_absmax: merged by maximum, every other field by sum
constexpr unsigned kPmMaxFields = 1u << 2;                      // g_absmax

struct SgdAcc {
    double g_sumsq = 0, dw_sumsq = 0, w_sumsq = 0;
    float g_absmax = 0, w_absmax = 0;
    unsigned n_routed = 0, g_nonfinite = 0, w_nonfinite = 0;
    __device__ __forceinline__ void record(double (&r)[kStatFields]) const {
        r[0] = n_routed, r[1] = g_nonfinite, r[2] = g_sumsq, r[3] = g_absmax, r[4] = w_nonfinite, r[5] = dw_sumsq, r[6] = w_sumsq, r[7] = w_absmax;
    }
};
struct PmAcc {
    double g_sumsq = 0, dpm_sumsq = 0;
    float g_absmax = 0;
    unsigned n_routed = 0, flips_on = 0, flips_off = 0, picked = 0, pm_nonfinite = 0;
    __device__ __forceinline__ void record(double (&r)[kStatFields]) const {
        r[0] = n_routed, r[1] = g_sumsq, r[2] = g_absmax, r[3] = dpm_sumsq, r[4] = flips_on, r[5] = flips_off, r[6] = picked, r[7] = pm_nonfinite;
    }
};

// sum of x^2 and max |x| over the finite values: the square is formed in fp64 (a finite fp32 whose square overflows fp32 still counts)
__device__ __forceinline__ void add_square(double &sumsq, double x) {
#pragma clang fp contract(off)
    const double sq = x * x;
    sumsq += sq;
}

template <bool ZERO>
__device__ __forceinline__ void sgd_route_one_stats(float &wv, float &gv, float &bv, int o, const SgdHyper h, SgdAcc &a) {
    const float w0 = wv;
    sgd_route_one<ZERO>(wv, gv, bv, o, h);
    if (o == h.cur) {
        a.n_routed++;
        if (__builtin_isfinite(gv)) {
            add_square(a.g_sumsq, (double)gv);
            a.g_absmax = fmaxf(a.g_absmax, fabsf(gv));
        } else {
            a.g_nonfinite++;
        }
    }
    if (__builtin_isfinite(wv)) {
        add_square(a.w_sumsq, (double)wv);
        a.w_absmax = fmaxf(a.w_absmax, fabsf(wv));
        if (__builtin_isfinite(w0)) add_square(a.dw_sumsq, (double)wv - (double)w0);
    } else {
        a.w_nonfinite++;
    }
}

__device__ __forceinline__ void adam_route_one_stats(float &p, float &g, float &m1, float &m2, int o, const AdamHyper h, float thr, PmAcc &a) {
    const float p0 = p;
    adam_route_one(p, g, m1, m2, o, h);
    if (h.mode == CPG_MODE_FINETUNE && o != 0 && o < h.cur) {
        a.n_routed++;
        if (__builtin_isfinite(g)) {
            add_square(a.g_sumsq, (double)g);
            a.g_absmax = fmaxf(a.g_absmax, fabsf(g));
        }
        const bool on0 = p0 > thr, on1 = p > thr;      // the Binarizer's compare: false for NaN
        a.flips_on += !on0 && on1;
        a.flips_off += on0 && !on1;
        a.picked += on1;
    }
    if (__builtin_isfinite(p)) {
        if (__builtin_isfinite(p0)) add_square(a.dpm_sumsq, (double)p - (double)p0);
    } else {
        a.pm_nonfinite++;
    }
}

template <bool ZERO>
__device__ __forceinline__ void sgd_route_span_stats(float *w, float *gw, float *buf, const uint8_t *owner, int64_t begin, int64_t end,
                                                     int64_t first, int64_t stride, int vec_ok, const SgdHyper h, SgdAcc &a) {
    walk4(begin, end, first, stride, vec_ok,
          [&](int64_t i) {
              const uint32_t o4 = reinterpret_cast<const uint32_t *>(owner)[i];
              F4 wv = reinterpret_cast<F4 *>(w)[i], gv = reinterpret_cast<F4 *>(gw)[i];
              F4 bv = h.first ? F4{0.f, 0.f, 0.f, 0.f} : reinterpret_cast<F4 *>(buf)[i];
              sgd_route_one_stats<ZERO>(wv.x, gv.x, bv.x, o4 & 255, h, a);
              sgd_route_one_stats<ZERO>(wv.y, gv.y, bv.y, (o4 >> 8) & 255, h, a);
              sgd_route_one_stats<ZERO>(wv.z, gv.z, bv.z, (o4 >> 16) & 255, h, a);
              sgd_route_one_stats<ZERO>(wv.w, gv.w, bv.w, o4 >> 24, h, a);
              reinterpret_cast<F4 *>(w)[i] = wv;
              reinterpret_cast<F4 *>(gw)[i] = gv;
              reinterpret_cast<F4 *>(buf)[i] = bv;
          },
          [&](int64_t i) {
              float bv = h.first ? 0.f : buf[i];
              sgd_route_one_stats<ZERO>(w[i], gw[i], bv, owner[i], h, a);
              buf[i] = bv;
          });
}

__device__ __forceinline__ void adam_route_span_stats(float *pm, float *gpm, float *m1, float *m2, const uint8_t *owner, int64_t begin,
                                                      int64_t end, int64_t first, int64_t stride, int vec_ok, const AdamHyper h, float thr,
                                                      PmAcc &a) {
    walk4(begin, end, first, stride, vec_ok,
          [&](int64_t i) {
              const uint32_t o4 = reinterpret_cast<const uint32_t *>(owner)[i];
              F4 pv = reinterpret_cast<F4 *>(pm)[i], gv = reinterpret_cast<F4 *>(gpm)[i];
              F4 av = reinterpret_cast<F4 *>(m1)[i], bv = reinterpret_cast<F4 *>(m2)[i];
              adam_route_one_stats(pv.x, gv.x, av.x, bv.x, o4 & 255, h, thr, a);
              adam_route_one_stats(pv.y, gv.y, av.y, bv.y, (o4 >> 8) & 255, h, thr, a);
              adam_route_one_stats(pv.z, gv.z, av.z, bv.z, (o4 >> 16) & 255, h, thr, a);
              adam_route_one_stats(pv.w, gv.w, av.w, bv.w, o4 >> 24, h, thr, a);
              reinterpret_cast<F4 *>(pm)[i] = pv;
              reinterpret_cast<F4 *>(gpm)[i] = gv;
              reinterpret_cast<F4 *>(m1)[i] = av;
              reinterpret_cast<F4 *>(m2)[i] = bv;
          },
          [&](int64_t i) { adam_route_one_stats(pm[i], gpm[i], m1[i], m2[i], owner[i], h, thr, a); });
}

// every lane ends with the wave's merged record: partner lanes add (or take the maximum of) the same two values, so all agree bit for bit
template <unsigned MAXMASK>
__device__ __forceinline__ void wave_merge(double (&r)[kStatFields]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int f = 0; f < kStatFields; ++f) {
            const double other = __shfl_xor(r[f], m);
            r[f] = ((MAXMASK >> f) & 1) ? fmax(r[f], other) : r[f] + other;
        }
    }
}

// the block's record (kThreads = 4 waves) to out[0 .. kStatFields): the waves are merged in order 0, 1, 2, 3 by threads 0 .. 7, one field each
template <unsigned MAXMASK>
__device__ __forceinline__ void block_merge_store(double (&r)[kStatFields], double *out) {
    __shared__ double red[kThreads / 64][kStatFields];
    wave_merge<MAXMASK>(r);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int f = 0; f < kStatFields; ++f) red[threadIdx.x >> 6][f] = r[f];
    }
    __syncthreads();
    if (threadIdx.x < kStatFields) {
        const int f = threadIdx.x;
        double v = red[0][f];
        for (int wv = 1; wv < kThreads / 64; ++wv) v = ((MAXMASK >> f) & 1) ? fmax(v, red[wv][f]) : v + red[wv][f];
        out[f] = v;
    }
}

template <bool ZERO>
__global__ __launch_bounds__(kThreads) void k_sgd_route_multi_stats(const SgdItems it, int cur, float wd, float lr, float momentum, int nesterov,
                                                                    int first, double *partials, int piece_base) {
    int64_t begin, end;
    const int item = find_piece(it, begin, end);
    SgdAcc a;
    sgd_route_span_stats<ZERO>(it.w[item], it.gw[item], it.buf[item], it.owner[item], begin, end, threadIdx.x, kThreads, it.vec[item],
                               SgdHyper{cur, wd, lr, momentum, nesterov, first}, a);
    double r[kStatFields];
    a.record(r);
    block_merge_store<kSgdMaxFields>(r, partials + ((size_t)piece_base + blockIdx.x) * kStatFields);
}

__global__ __launch_bounds__(kThreads) void k_adam_route_multi_stats(const AdamItems it, int cur, int mode, float step_size, float omb1,
                                                                     float beta2, float omb2, float eps, float bc2_sqrt, float thr,
                                                                     double *partials, int piece_base) {
    int64_t begin, end;
    const int item = find_piece(it, begin, end);
    PmAcc a;
    adam_route_span_stats(it.pm[item], it.gpm[item], it.m1[item], it.m2[item], it.owner[item], begin, end, threadIdx.x, kThreads, it.vec[item],
                          AdamHyper{cur, mode, step_size, omb1, beta2, omb2, eps, bc2_sqrt}, thr, a);
    double r[kStatFields];
    a.record(r);
    block_merge_store<kPmMaxFields>(r, partials + ((size_t)piece_base + blockIdx.x) * kStatFields);
}

// Finalize: block b (one wave) merges the pieces [first_piece[b], first_piece[b + 1]) of item item_base + b, in a fixed order, into
// stats[item]; an item without pieces (n == 0) gets the all-zero record.  The table travels by value, kFinMax items per launch.
constexpr int kFinMax = 256;
struct FinItems {
    int first_piece[kFinMax + 1];
    int count, item_base;
};

template <unsigned MAXMASK>
__global__ __launch_bounds__(64) void k_step_stats_finalize(const FinItems it, const double *__restrict__ partials, double *__restrict__ stats) {
    const int row = blockIdx.x;
    double r[kStatFields] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int p = it.first_piece[row] + (int)threadIdx.x; p < it.first_piece[row + 1]; p += 64) {
#pragma unroll
        for (int f = 0; f < kStatFields; ++f) {
            const double v = partials[(size_t)p * kStatFields + f];
            r[f] = ((MAXMASK >> f) & 1) ? fmax(r[f], v) : r[f] + v;
        }
    }
    wave_merge<MAXMASK>(r);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int f = 0; f < kStatFields; ++f) stats[(size_t)(it.item_base + row) * kStatFields + f] = r[f];
    }
}

// The sticky health record {first_bad_step, first_bad_item, kind, bad_steps} from the finalized records of one step: the lowest bad
// item of the step; kind 1 = a non-finite routed gradient (SGD records: g_nonfinite), 2 = a non-finite weight / piggymask after the step.
template <bool SGD>
__global__ __launch_bounds__(kThreads) void k_step_health(const double *__restrict__ stats, int n_items, long long step,
                                                          long long *__restrict__ health) {
    __shared__ int lowest[kThreads / 64];
    auto bad = [&](int i) {
        const double *s = stats + (size_t)i * kStatFields;
        return SGD ? (s[1] > 0 || s[4] > 0) : s[7] > 0;
    };
    int best = INT32_MAX;
    for (int i = threadIdx.x; i < n_items; i += kThreads)
        if (i < best && bad(i)) best = i;
    for (int m = 32; m >= 1; m >>= 1) best = min(best, __shfl_xor(best, m));
    if ((threadIdx.x & 63) == 0) lowest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < kThreads / 64; ++wv) best = min(best, lowest[wv]);
        if (best != INT32_MAX) {
            if (health[0] == 0) {
                health[0] = step;
                health[1] = best;
                health[2] = (SGD && stats[(size_t)best * kStatFields + 1] > 0) ? 1 : 2;
            }
            health[3] += 1;
        }
    }
}

// one row of a multi-tensor table: is it usable, and its copy into slot i of the kernel's argument struct with its float4 flag
inline bool row_ok(const cpg_sgd_item &s) { return s.n >= 0 && (s.n == 0 || (s.w && s.gw && s.momentum_buf && s.owner)); }
inline bool row_ok(const cpg_adam_item &s) { return s.n >= 0 && (s.n == 0 || (s.pm && s.gpm && s.exp_avg && s.exp_avg_sq && s.owner)); }
inline void set_row(SgdItems &it, int i, const cpg_sgd_item &s) {
    it.w[i] = s.w, it.gw[i] = s.gw, it.buf[i] = s.momentum_buf, it.owner[i] = s.owner, it.n[i] = s.n;
    it.vec[i] = aligned16(s.w) && aligned16(s.gw) && aligned16(s.momentum_buf) && aligned4(s.owner);
}
inline void set_row(AdamItems &it, int i, const cpg_adam_item &s) {
    it.pm[i] = s.pm, it.gpm[i] = s.gpm, it.m1[i] = s.exp_avg, it.m2[i] = s.exp_avg_sq, it.owner[i] = s.owner, it.n[i] = s.n;
    it.vec[i] = aligned16(s.pm) && aligned16(s.gpm) && aligned16(s.exp_avg) && aligned16(s.exp_avg_sq) && aligned4(s.owner);
}

// The table walk of the three multi entry points: kMultiMax non-empty rows per `launch(items, blocks)`.  Every row is checked before
// the first launch (pointers, sizes, and the grid of the launch it will fall into, cut as below): a bad table changes nothing.
template <class Row>
int check_rows(const char *fn, const Row *rows, int32_t n_rows) {
    CPG_REQUIRE(n_rows >= 0 && (n_rows == 0 || rows), "%s: null item table or negative count", fn);
    for (int32_t at = 0, count = 0, blocks = 0; at < n_rows; ++at) {
        const Row &s = rows[at];
        CPG_REQUIRE(row_ok(s), "%s: item %d: null pointer or negative n", fn, at);
        if (s.n == 0) continue;
        if (count == kMultiMax) count = 0, blocks = 0;
        const int64_t pieces = (s.n + kChunk - 1) / kChunk;
        CPG_REQUIRE(blocks + pieces < (1ll << 30), "%s: item %d is too large for one launch", fn, at);
        blocks += (int)pieces, ++count;
    }
    return CPG_OK;
}

template <class Items, class Row, class Launch>
int launch_rows(const char *fn, const Row *rows, int32_t n_rows, Launch launch) {
    for (int32_t at = 0; at < n_rows;) {
        Items it;
        int blocks = 0;
        it.count = 0;
        for (; at < n_rows && it.count < kMultiMax; ++at) {
            const Row &s = rows[at];
            if (s.n == 0) continue;
            const int i = it.count++;
            set_row(it, i, s);
            it.first_block[i] = blocks;
            blocks += (int)((s.n + kChunk - 1) / kChunk);
        }
        if (it.count == 0) continue;
        it.first_block[it.count] = blocks;
        launch(it, blocks);
        CPG_CHECK_LAUNCH(fn);
    }
    return CPG_OK;
}

template <class Items, class Row, class Launch>
int route_multi(const char *fn, const Row *rows, int32_t n_rows, Launch launch) {
    if (const int rc = check_rows(fn, rows, n_rows)) return rc;
    return launch_rows<Items>(fn, rows, n_rows, launch);
}

template <bool ZERO>
int sgd_route_multi(const char *fn, const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                    int32_t nesterov, int32_t first_step, void *stream) {
    CPG_REQUIRE(cur >= 0 && cur <= 255, "%s: owner id %d out of uint8 range", fn, cur);
    return route_multi<SgdItems>(fn, items_host, n_items, [&](const SgdItems &it, int blocks) {
        hipLaunchKernelGGL(k_sgd_route_multi<ZERO>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, it, cur, wd, lr, momentum, nesterov,
                           first_step);
    });
}

// ---- the host side of the STATS entry points
struct StatsArgs {
    int64_t step;
    void *stats, *partials;
    size_t partials_bytes;
    int64_t *health;
};

inline int64_t pieces_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

// what a _stats call adds to its plain twin's checks; runs after check_rows (every n is >= 0) and before the first launch
template <class Row>
int check_stats(const char *fn, const Row *rows, int32_t n_rows, const StatsArgs &a) {
    CPG_REQUIRE(a.step >= 1, "%s: step %lld: the 1-based number of the step", fn, (long long)a.step);
    CPG_REQUIRE(a.health != nullptr, "%s: null health record", fn);
    int64_t pieces = 0;
    for (int32_t at = 0; at < n_rows; ++at) pieces += pieces_of(rows[at].n);
    CPG_REQUIRE(pieces < (1ll << 31), "%s: %lld pieces are too many for one call", fn, (long long)pieces);
    const size_t need = (size_t)pieces * kStatFields * sizeof(double);
    if (a.partials_bytes < need) return fail(CPG_E_WORKSPACE, "%s: partials buffer %zu < %zu bytes", fn, a.partials_bytes, need);
    CPG_REQUIRE(a.stats && aligned16(a.stats) && a.partials && aligned16(a.partials), "%s: stats / partials null or not 16-byte aligned", fn);
    return CPG_OK;
}

// after the step's launches, on the same stream: the records of all rows, then the health record
template <unsigned MAXMASK, bool SGD, class Row>
int finalize_stats(const char *fn, const Row *rows, int32_t n_rows, const StatsArgs &a, void *stream) {
    int piece = 0;
    for (int32_t at = 0; at < n_rows;) {
        FinItems f;
        f.count = 0, f.item_base = at;
        for (; at < n_rows && f.count < kFinMax; ++at) {
            f.first_piece[f.count++] = piece;
            piece += (int)pieces_of(rows[at].n);
        }
        f.first_piece[f.count] = piece;
        hipLaunchKernelGGL(k_step_stats_finalize<MAXMASK>, dim3(f.count), dim3(64), 0, (hipStream_t)stream, f, (const double *)a.partials,
                           (double *)a.stats);
        CPG_CHECK_LAUNCH(fn);
    }
    if (n_rows == 0) return CPG_OK;
    hipLaunchKernelGGL(k_step_health<SGD>, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double *)a.stats, (int)n_rows,
                       (long long)a.step, (long long *)a.health);
    CPG_CHECK_LAUNCH(fn);
    return CPG_OK;
}

template <bool ZERO>
int sgd_route_multi_stats(const char *fn, const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                          int32_t nesterov, int32_t first_step, const StatsArgs &a, void *stream) {
    CPG_REQUIRE(cur >= 0 && cur <= 255, "%s: owner id %d out of uint8 range", fn, cur);
    if (const int rc = check_rows(fn, items_host, n_items)) return rc;
    if (const int rc = check_stats(fn, items_host, n_items, a)) return rc;
    int piece_base = 0;                          // one running piece index over the launches of a long table
    const int rc = launch_rows<SgdItems>(fn, items_host, n_items, [&](const SgdItems &it, int blocks) {
        hipLaunchKernelGGL(k_sgd_route_multi_stats<ZERO>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, it, cur, wd, lr, momentum,
                           nesterov, first_step, (double *)a.partials, piece_base);
        piece_base += blocks;
    });
    return rc ? rc : finalize_stats<kSgdMaxFields, true>(fn, items_host, n_items, a, stream);
}

template <bool ZERO>
int sgd_route(const char *fn, float *w, float *gw, float *momentum_buf, const uint8_t *owner, int32_t cur, float wd, float lr, float momentum,
              int32_t nesterov, int32_t first_step, int64_t n, void *stream) {
    CPG_REQUIRE(n >= 0 && (n == 0 || (w && gw && momentum_buf && owner)), "%s: null pointer or negative n", fn);
    CPG_REQUIRE(cur >= 0 && cur <= 255, "%s: owner id %d out of uint8 range", fn, cur);
    if (n == 0) return CPG_OK;
    const int vec = aligned16(w) && aligned16(gw) && aligned16(momentum_buf) && aligned4(owner);
    hipLaunchKernelGGL(k_sgd_route<ZERO>, dim3(stream_grid(n, kThreads * 4)), dim3(kThreads), 0, (hipStream_t)stream, w, gw, momentum_buf,
                       owner, cur, wd, lr, momentum, nesterov, first_step, n, vec);
    CPG_CHECK_LAUNCH(fn);
    return CPG_OK;
}

}  // namespace

extern "C" int32_t cpg_multi_tensor_max(void) { return kMultiMax; }

extern "C" int cpg_sgd_route_step_multi(const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                                        int32_t nesterov, int32_t first_step, void *stream) {
    return sgd_route_multi<false>("cpg_sgd_route_step_multi", items_host, n_items, cur, wd, lr, momentum, nesterov, first_step, stream);
}

extern "C" int cpg_sgd_route_zero_step_multi(const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                                             int32_t nesterov, int32_t first_step, void *stream) {
    return sgd_route_multi<true>("cpg_sgd_route_zero_step_multi", items_host, n_items, cur, wd, lr, momentum, nesterov, first_step, stream);
}

extern "C" int cpg_adam_route_step_multi(const cpg_adam_item *items_host, int32_t n_items, int32_t cur, int32_t mode, double lr, double beta1,
                                         double beta2, double eps, int32_t step, void *stream) {
    CPG_REQUIRE(mode == CPG_MODE_FINETUNE || mode == CPG_MODE_PRUNE, "cpg_adam_route_step_multi: unknown mode %d", mode);
    CPG_REQUIRE(cur >= 0 && cur <= 255 && step >= 1, "cpg_adam_route_step_multi: owner id %d / step %d out of range", cur, step);
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    return route_multi<AdamItems>("cpg_adam_route_step_multi", items_host, n_items, [&](const AdamItems &it, int blocks) {
        hipLaunchKernelGGL(k_adam_route_multi, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, it, cur, mode, (float)(lr / bc1),
                           (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)sqrt(bc2));
    });
}

extern "C" size_t cpg_step_stats_workspace_bytes(const int64_t *n_host, int32_t n_items) {
    size_t pieces = 0;
    for (int32_t i = 0; n_host && i < n_items; ++i)
        if (n_host[i] > 0) pieces += (size_t)pieces_of(n_host[i]);
    return pieces * kStatFields * sizeof(double);
}

extern "C" int cpg_sgd_route_step_multi_stats(const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                                              int32_t nesterov, int32_t first_step, int64_t step, void *stats, void *partials,
                                              size_t partials_bytes, int64_t *health, void *stream) {
    return sgd_route_multi_stats<false>("cpg_sgd_route_step_multi_stats", items_host, n_items, cur, wd, lr, momentum, nesterov, first_step,
                                        StatsArgs{step, stats, partials, partials_bytes, health}, stream);
}

extern "C" int cpg_sgd_route_zero_step_multi_stats(const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr,
                                                   float momentum, int32_t nesterov, int32_t first_step, int64_t step, void *stats,
                                                   void *partials, size_t partials_bytes, int64_t *health, void *stream) {
    return sgd_route_multi_stats<true>("cpg_sgd_route_zero_step_multi_stats", items_host, n_items, cur, wd, lr, momentum, nesterov, first_step,
                                       StatsArgs{step, stats, partials, partials_bytes, health}, stream);
}

// (`adam_step` is cpg_adam_route_step_multi's `step`, Adam's bias-correction count; `step` the telemetry's step number)
extern "C" int cpg_adam_route_step_multi_stats(const cpg_adam_item *items_host, int32_t n_items, int32_t cur, int32_t mode, double lr,
                                               double beta1, double beta2, double eps, int32_t adam_step, float thr, int64_t step, void *stats,
                                               void *partials, size_t partials_bytes, int64_t *health, void *stream) {
    const char *fn = "cpg_adam_route_step_multi_stats";
    CPG_REQUIRE(mode == CPG_MODE_FINETUNE || mode == CPG_MODE_PRUNE, "%s: unknown mode %d", fn, mode);
    CPG_REQUIRE(cur >= 0 && cur <= 255 && adam_step >= 1, "%s: owner id %d / step %d out of range", fn, cur, adam_step);
    const StatsArgs a{step, stats, partials, partials_bytes, health};
    if (const int rc = check_rows(fn, items_host, n_items)) return rc;
    if (const int rc = check_stats(fn, items_host, n_items, a)) return rc;
    const double bc1 = 1.0 - pow(beta1, (double)adam_step), bc2 = 1.0 - pow(beta2, (double)adam_step);
    int piece_base = 0;
    const int rc = launch_rows<AdamItems>(fn, items_host, n_items, [&](const AdamItems &it, int blocks) {
        hipLaunchKernelGGL(k_adam_route_multi_stats, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, it, cur, mode, (float)(lr / bc1),
                           (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)sqrt(bc2), thr, (double *)partials,
                           piece_base);
        piece_base += blocks;
    });
    return rc ? rc : finalize_stats<kPmMaxFields, false>(fn, items_host, n_items, a, stream);
}

extern "C" int cpg_adam_route_step(float *pm, float *gpm, float *exp_avg, float *exp_avg_sq, const uint8_t *owner, int32_t cur,
                                   int32_t mode, double lr, double beta1, double beta2, double eps, int32_t step, int64_t n, void *stream) {
    CPG_REQUIRE(n >= 0 && (n == 0 || (pm && gpm && exp_avg && exp_avg_sq && owner)), "cpg_adam_route_step: null pointer or negative n");
    CPG_REQUIRE(mode == CPG_MODE_FINETUNE || mode == CPG_MODE_PRUNE, "cpg_adam_route_step: unknown mode %d", mode);
    CPG_REQUIRE(cur >= 0 && cur <= 255 && step >= 1, "cpg_adam_route_step: owner id %d / step %d out of range", cur, step);
    if (n == 0) return CPG_OK;
    // every derived constant is formed in double and rounded once, as torch does with its python-float hyper-parameters
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const int vec = aligned16(pm) && aligned16(gpm) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned4(owner);
    hipLaunchKernelGGL(k_adam_route, dim3(stream_grid(n, kThreads * 4)), dim3(kThreads), 0, (hipStream_t)stream, pm, gpm, exp_avg,
                       exp_avg_sq, owner, cur, mode, (float)(lr / bc1), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                       (float)sqrt(bc2), n, vec);
    CPG_CHECK_LAUNCH("cpg_adam_route_step");
    return CPG_OK;
}

extern "C" int cpg_sgd_route_step(float *w, float *gw, float *momentum_buf, const uint8_t *owner, int32_t cur, float wd, float lr,
                                  float momentum, int32_t nesterov, int32_t first_step, int64_t n, void *stream) {
    return sgd_route<false>("cpg_sgd_route_step", w, gw, momentum_buf, owner, cur, wd, lr, momentum, nesterov, first_step, n, stream);
}

extern "C" int cpg_sgd_route_zero_step(float *w, float *gw, float *momentum_buf, const uint8_t *owner, int32_t cur, float wd, float lr,
                                       float momentum, int32_t nesterov, int32_t first_step, int64_t n, void *stream) {
    return sgd_route<true>("cpg_sgd_route_zero_step", w, gw, momentum_buf, owner, cur, wd, lr, momentum, nesterov, first_step, n, stream);
}


extern "C" int cpg_binarize_mask_weight(const float *w, const float *pm, float thr, float *w_eff, int64_t n,
                                        void *stream) {
    CPG_REQUIRE(n >= 0 && (n == 0 || (pm && w_eff)), "cpg_binarize_mask_weight: null pointer or negative n");
    if (n == 0) return CPG_OK;
    const int vec = (!w || aligned16(w)) && aligned16(pm) && aligned16(w_eff);
    hipLaunchKernelGGL(k_binarize_mul, dim3(stream_grid(n, kThreads * 4)), dim3(kThreads), 0, (hipStream_t)stream, w, pm,
                       thr, w_eff, n, vec);
    CPG_CHECK_LAUNCH("cpg_binarize_mask_weight");
    return CPG_OK;
}

extern "C" int cpg_route_grads(float *gw, const float *w, const uint8_t *owner, int32_t cur, float wd, float *gpm,
                               int32_t mode, int64_t n, void *stream) {
    CPG_REQUIRE(n >= 0 && (n == 0 || (gw && w && owner)), "cpg_route_grads: null pointer or negative n");
    CPG_REQUIRE(mode == CPG_MODE_FINETUNE || mode == CPG_MODE_PRUNE, "cpg_route_grads: unknown mode %d", mode);
    CPG_REQUIRE(cur >= 0 && cur <= 255, "cpg_route_grads: owner id %d out of uint8 range", cur);
    if (n == 0) return CPG_OK;
    const int vec = aligned16(gw) && aligned16(w) && aligned4(owner) && (!gpm || aligned16(gpm));
    const dim3 grid(stream_grid(n, kThreads * 4)), block(kThreads);
    if (gpm)
        hipLaunchKernelGGL(k_route<true>, grid, block, 0, (hipStream_t)stream, gw, w, owner, cur, wd, gpm, mode, n, vec);
    else
        hipLaunchKernelGGL(k_route<false>, grid, block, 0, (hipStream_t)stream, gw, w, owner, cur, wd, gpm, mode, n, vec);
    CPG_CHECK_LAUNCH("cpg_route_grads");
    return CPG_OK;
}

extern "C" int cpg_mask_hist(const uint8_t *owner, const float *pm, int32_t inference_idx, int64_t n, uint64_t *hist,
                             void *stream) {
    CPG_REQUIRE(n >= 0 && hist && (n == 0 || owner), "cpg_mask_hist: null pointer or negative n");
    if (n == 0) return CPG_OK;
    const int vec = aligned4(owner) && (!pm || aligned16(pm));
    hipLaunchKernelGGL(k_mask_hist, dim3(stream_grid(n, kThreads * 16)), dim3(kThreads), 0, (hipStream_t)stream, owner, pm,
                       inference_idx, n, (unsigned long long *)hist, vec);
    CPG_CHECK_LAUNCH("cpg_mask_hist");
    return CPG_OK;
}

extern "C" int cpg_apply_mask(float *w, const uint8_t *owner, int32_t inference_idx, int64_t n, void *stream) {
    CPG_REQUIRE(n >= 0 && (n == 0 || (w && owner)), "cpg_apply_mask: null pointer or negative n");
    if (n == 0) return CPG_OK;
    const int vec = aligned16(w) && aligned4(owner);
    hipLaunchKernelGGL(k_zero_by_owner, dim3(stream_grid(n, kThreads * 4)), dim3(kThreads), 0, (hipStream_t)stream, w,
                       owner, inference_idx, n, vec);
    CPG_CHECK_LAUNCH("cpg_apply_mask");
    return CPG_OK;
}

extern "C" int cpg_zero_pruned(float *w, const uint8_t *owner, int64_t n, void *stream) {
    return cpg_apply_mask(w, owner, 255, n, stream);      // no uint8 owner exceeds 255: only owner == 0 dies
}

extern "C" int cpg_claim_free(uint8_t *owner, int32_t new_idx, int64_t n, void *stream) {
    CPG_REQUIRE(n >= 0 && (n == 0 || owner), "cpg_claim_free: null pointer or negative n");
    CPG_REQUIRE(new_idx >= 1 && new_idx <= 255, "cpg_claim_free: owner id %d out of uint8 range", new_idx);
    if (n == 0) return CPG_OK;
    const int vec = aligned16(owner);
    hipLaunchKernelGGL(k_claim_free, dim3(stream_grid(n, kThreads * 16)), dim3(kThreads), 0, (hipStream_t)stream, owner,
                       (unsigned)new_idx, n, vec);
    CPG_CHECK_LAUNCH("cpg_claim_free");
    return CPG_OK;
}
