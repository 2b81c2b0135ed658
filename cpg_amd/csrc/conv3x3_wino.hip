// Masked 3x3 / stride 1 / pad 1 convolution by Winograd F(2x2, 3x3) on fp32 MFMA: forward and input gradient.
//
//   Y(2x2 tile) = A^T [ (G g G^T) .* (B^T d B) ] A        (d: 4x4 input patch, g: 3x3 filter; Lavin & Gray 2015)
//
// 16 multiplies per 2x2 output tile and (c, k) pair instead of 36: the contraction over input channels becomes 16
// independent GEMMs  M_p[k][t] = sum_c U_p[k][c] * V_p[c][t]  (p = transform-domain position, t = tile), 2.25x fewer MFMAs
// than the direct kernels of conv3x3.hip for the same result up to fp32 rounding (the transforms only add, subtract and
// halve; measured 1-4e-6 of the output scale against fp64, the direct kernels 0.5-1e-6).  docs/LAB_NOTEBOOK.md section 4.9 has the
// measurements behind the choices below.
//
//   k_wg_pack   U = G (W .* bin(piggymask)) G^T per (k, c), written in the order the conv kernel streams it:
//               Up[k block of BK][channel chunk of 4][p][k][c]  (one contiguous record per block and chunk)
//   k_wg_fwd    block = NW waves = BK output channels x 64 tiles (256 output pixels); a tile run is 64 consecutive tiles in
//               (image, tile row, tile column) order, whatever the map size -- no padding tiles, blocks may straddle rows and
//               images.  NW = 4 (the default): BK = 32, two blocks per CU; NW = 8: BK = 64, one block per CU (every
//               transformed input element feeds twice the MFMAs, less staging work per MFMA -- but measured slower, see
//               WinoPlan::nw).  Wave (tq, ph, kq) owns tiles tq*32..+31, positions ph*8..+7 and
//               channels kq*32..+31: 8 accumulators of 32 x 32.  Per chunk of 4 input channels:
//     G  global -> registers.  A vector-memory instruction occupies the texture addresser for 16 cycles whatever its width
//        (gathering every tile's 4 x 4 patch with 16 dword loads made the kernel TA-bound), so the patch rows are fetched
//        ONCE, as aligned column pairs: per channel and patch row one buffer_load_dwordx2 (lane t = columns 2 tx, 2 tx + 1 of
//        tile t; range-checked: rows outside the image read as zeros), plus one dword load for the two halo columns left /
//        right of the tile run.  U: two float4 per thread.
//     W  registers -> LDS raw[c][row][slot 1 + t][2]  (slot 0 / 65: halos; their unused halves hold zeros that the tiles on
//        the image's left / right border read instead of a neighbour)
//     T  every thread reads a tile's patch back (own pair + the neighbours' halves), transforms it in registers and writes the
//        positions to LDS V[p][c][t].  NW = 8: two threads share a tile, positions 0-7 (patch rows 0-2) / 8-15 (rows 1-3).
//     M  16 MFMAs per wave; operands: lanes 0-31 take channels (0, 1), lanes 32-63 channels (2, 3) of the chunk.
//   Main-loop iteration `it` runs M(it), T(it + 1), W(it + 2), G(it + 5) -- three register sets -- software-pipelined ACROSS its
//   one barrier: every LDS write the other waves wait for and every LDS read of this chunk's operands is issued by position 3;
//   positions 4-7 run from registers after the barrier while the wave issues G and already reads the next chunk's first operands
//   and raw patch.  sched_barrier fences pin that order (left alone, the compiler clumps the MFMAs at the top).
//   Epilogue: the output transform is linear, so each wave reduces its 8 positions to partial 2x2 outputs, the two waves of a
//   tile swap halves through LDS (row 0 of every tile is finished by ph = 0, row 1 by ph = 1) and store float2 per lane.
//   STATS: per-channel sum / sum of squares of the block's outputs for the BatchNorm that follows (as k_c3_fwd<.., STATS>).
//   dgrad       the same kernel on gy with the filter transposed and spatially flipped (k_wg_pack's dgrad flavour).
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include "cpg_dispatch.h"
#include "wino_acc.h"

using namespace cpg;

namespace {

constexpr int WG_T = 64;                      // tiles per block
constexpr int WG_CK = 4;                      // input channels per chunk
constexpr int WG_V = 16 * WG_T * WG_CK;       // floats of V per chunk
constexpr int WG_RAWC = 4 * 66 * 2;           // raw floats per channel: [row][slot][2]
constexpr int WG_RAW = WG_CK * WG_RAWC;

struct WgGeom {
    int N, C, H, W, M;        // C: channels read, M: channels produced
    int th, tw;               // tiles per image column / row (H / 2, W / 2)
    int tiles_img;            // th * tw
    int64_t tiles_total;      // N * th * tw
    int nkb, nch;             // blocks of BK output channels, chunks of 4 input channels
    int span;                 // images a block's 64 consecutive tiles can touch
    unsigned nblocks;         // k_wg1 / k_wg3: logical blocks of the launch (the grid may be smaller: blocks loop over them)
    float inv_timg, inv_tw;   // 1 / tiles_img, 1 / tw (wg_divmod)
    // k_wg3<.., SPLIT> (the tail launch of wg3_run): logical blocks split_first .. of the layer, each cut into split_s pieces of split_nch
    // channel chunks; piece s writes its partial outputs to y + s * split_stride
    unsigned split_first;
    int split_s, split_nch;
    int64_t split_stride;
};

// rel / d and rel % d for rel < 2^24 (exact in fp32) and a small quotient: a multiply by the reciprocal and one correction step, ~10
// vector instructions where the compiler's generic 32-bit division is ~30 -- a unit's set-up did eight of those, its epilogue four,
// and on this chip every vector instruction of the single resident wave is MFMA time (the twin of pointwise.hip's divmod_small).
__device__ __forceinline__ void wg_divmod(unsigned rel, unsigned d, float inv, unsigned &qt, unsigned &rm) {
    const unsigned n = (unsigned)((float)rel * inv);
    const int r = (int)(rel - n * d);
    const int lt = r < 0 ? 1 : 0, ge = r >= (int)d ? 1 : 0;            // (selects, no branches)
    qt = n + ge - lt;
    rm = (unsigned)(r + (lt - ge) * (int)d);
}

// First input channel of chunk `ch`.  A channel count that is not a multiple of the chunk (the reference's grown networks: 78 / 313 /
// 627 channels, models/vgg.py:124-154 with sqrt(1.5)) makes the LAST chunk start at C - 4 instead of past the end: it overlaps the chunk
// before it, and the pack kernels give the overlapped channels (already contracted there) zero filters.  The conv kernels then never read
// a channel that does not exist -- no range check, no predicate in the main loop, one scalar min per chunk.
__host__ __device__ __forceinline__ int wg_chunk_base(int ch, int C) {
    const int b = ch * WG_CK;
    return b < C - WG_CK ? b : C - WG_CK;
}

// ------------------------------------------------------------------------------ weight transform
__global__ __launch_bounds__(256) void k_wg_pack(const float *__restrict__ w, const float *__restrict__ pm, float thr,
                                                 float *__restrict__ up, int K, int C, int M, int Cin, int nch, int dgrad, int BK) {
    // one thread per (kb, ch, kl, cl); writes 16 values at stride BK * 4 floats
    const int64_t total = (int64_t)((M + BK - 1) / BK) * nch * BK * WG_CK;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int cl = (int)(o % WG_CK);
        const int kl = (int)((o / WG_CK) % BK);
        const int64_t rec = o / (WG_CK * BK);                // kb * nch + ch
        const int ch = (int)(rec % nch), kb = (int)(rec / nch);
        const int m = kb * BK + kl, c = wg_chunk_base(ch, Cin) + cl;     // produced / read channel (the last chunk may overlap the one before)
        float g[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) g[r][s] = 0.0f;
        if (m < M && c >= ch * WG_CK) {
            const int co = dgrad ? c : m, ci = dgrad ? m : c;
            const int64_t off = ((int64_t)co * C + ci) * 9;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int tap = dgrad ? 8 - (r * 3 + s) : r * 3 + s;
                    float v = w[off + tap];
                    if (pm != nullptr) v *= binarize(pm[off + tap], thr);
                    g[r][s] = v;
                }
        }
        float t[4][3];                                        // G g
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            t[0][s] = g[0][s];
            t[1][s] = 0.5f * (g[0][s] + g[1][s] + g[2][s]);
            t[2][s] = 0.5f * (g[0][s] - g[1][s] + g[2][s]);
            t[3][s] = g[2][s];
        }
        float *dst = up + rec * (16 * BK * WG_CK) + kl * WG_CK + cl;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dst[(i * 4 + 0) * (BK * WG_CK)] = t[i][0];
            dst[(i * 4 + 1) * (BK * WG_CK)] = 0.5f * (t[i][0] + t[i][1] + t[i][2]);
            dst[(i * 4 + 2) * (BK * WG_CK)] = 0.5f * (t[i][0] - t[i][1] + t[i][2]);
            dst[(i * 4 + 3) * (BK * WG_CK)] = t[i][2];
        }
    }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

template <int NW_>
struct WgCfg {
    static constexpr int NW = NW_, NT = 64 * NW, BK = 8 * NW;
    static constexpr int U = 16 * BK * WG_CK;              // floats of U per chunk
    // LDS map (floats): V[2 stages] | U[3 stages] | raw[2 stages]
    static constexpr int OFF_U = 2 * WG_V, OFF_RAW = OFF_U + 3 * U, SMEM = OFF_RAW + 2 * WG_RAW;   // 72.5 KB (NW = 4) / 96.5 KB (NW = 8)
    static constexpr int NROW = NW == 4 ? 4 : 2;           // patch rows a wave fetches per chunk
    static constexpr int ND = NW == 4 ? 16 : 12;           // patch elements a thread transforms (4 or 3 rows)
    static_assert(NW == 4 || NW == 8, "4 or 8 waves");
};

// ------------------------------------------------------------------------------ forward / input gradient
template <int NW, bool DGRAD, bool STATS>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void k_wg_fwd(WgGeom g, const float *__restrict__ x,
                                                                      const float *__restrict__ up,
                                                                      const float *__restrict__ bias, float *__restrict__ y,
                                                                      float *__restrict__ stats) {
    using Cfg = WgCfg<NW>;
    constexpr int BK = Cfg::BK;
    __shared__ __attribute__((aligned(16))) float smem[Cfg::SMEM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tq = wave & 1, ph = (wave >> 1) & 1, kq = wave >> 2;
    const int li = lane & 31, lh = lane >> 5;
    const int HW = g.H * g.W;
    // staging roles: channel of the chunk, first patch row fetched (G / W), position half transformed (T)
    const int sc = NW == 4 ? wave : wave >> 1;
    const int srow = NW == 4 ? 0 : 2 * (wave & 1);
    const int half = NW == 4 ? 0 : wave & 1;               // NW = 8: positions 8 * half .. + 7 = transform rows 2 * half, + 1

    unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int kb = lb % g.nkb;
    const unsigned tb = lb / g.nkb;
    const int64_t t0 = (int64_t)tb * WG_T;                  // first tile of the block
    const int n0 = (int)(t0 / g.tiles_img);                 // first image the block touches

    // ---- G descriptors: tile `lane`, channel `sc` of the chunk ----
    constexpr int kOutOfRange = (int)0x80000000;
    int roff[Cfg::NROW];                                    // byte offset of (row, column 2 tx), or out of range (-> zeros)
    int hoff;
    int lo, ro;                                             // raw-row float index of the patch's column 0 / 3 (a zero slot on the image border)
    {
        const int64_t tg = t0 + lane;
        const bool tv = tg < g.tiles_total;
        const int n = (int)(tg / g.tiles_img), r = (int)(tg % g.tiles_img);
        const int ty = r / g.tw, tx = r % g.tw;
        const int cbase = ((n - n0) * g.C + sc) * HW;
#pragma unroll
        for (int i = 0; i < Cfg::NROW; ++i) {
            const int gh = 2 * ty - 1 + srow + i;
            roff[i] = (tv && (unsigned)gh < (unsigned)g.H) ? (cbase + gh * g.W + 2 * tx) * 4 : kOutOfRange;
        }
        lo = tx == 0 ? 0 : (lane + 1) * 2 - 1;
        ro = tx == g.tw - 1 ? 65 * 2 + 1 : (lane + 1) * 2 + 2;
        // halo loads, one instruction: lanes 0-3 fetch row (lane) of the column LEFT of tile t0 (slot 0, element 1), lanes 4-7 row
        // (lane - 4) of the column RIGHT of tile t0 + 63 (slot 65, element 0); out of range when that tile sits on the image border
        const int side = (lane >> 2) & 1, hi = lane & 3;
        const int64_t th = side ? t0 + WG_T - 1 : t0;
        const int nh = (int)(th / g.tiles_img), rh = (int)(th % g.tiles_img);
        const int tyh = rh / g.tw, txh = rh % g.tw;
        const int ghh = 2 * tyh - 1 + hi, gwh = side ? 2 * txh + 2 : 2 * txh - 1;
        const bool okh = lane < 8 && th < g.tiles_total && (unsigned)ghh < (unsigned)g.H && (unsigned)gwh < (unsigned)g.W;
        hoff = okh ? (((nh - n0) * g.C + sc) * HW + ghh * g.W + gwh) * 4 : kOutOfRange;
    }
    const bool halo_wave = NW == 4 || (wave & 1) == 0;
    const int nimg_here = min(g.span, g.N - n0);
    const __amdgpu_buffer_rsrc_t srd_x =
        __builtin_amdgcn_make_buffer_rsrc((void *)(x + (int64_t)n0 * g.C * HW), 0, nimg_here * g.C * HW * 4, 0x00020000);
    const float *ubase = up + (int64_t)kb * g.nch * Cfg::U + tid * 4;

    struct Regs {
        f32x4 u[2];
        i32x2 row[Cfg::NROW];
        float halo;
    };
    Regs rs[3];
    auto G = [&](int ch, Regs &r) {
        r.u[0] = *reinterpret_cast<const f32x4 *>(ubase + (int64_t)ch * Cfg::U);
        r.u[1] = *reinterpret_cast<const f32x4 *>(ubase + (int64_t)ch * Cfg::U + Cfg::NT * 4);
        const int soff = wg_chunk_base(ch, g.C) * HW * 4;
#pragma unroll
        for (int i = 0; i < Cfg::NROW; ++i) r.row[i] = __builtin_amdgcn_raw_buffer_load_b64(srd_x, roff[i], soff, 0);
        if (halo_wave) r.halo = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_x, hoff, soff, 0));
    };
    // raw[c][row][slot][2]: slot 0 = left halo, 1 + t = tile t, 65 = right halo
    const int raw_c = Cfg::OFF_RAW + sc * WG_RAWC;
    const int raw_w = raw_c + srow * 132 + (lane + 1) * 2;
    const int halo_w = raw_c + (lane & 3) * 132 + ((lane >> 2) & 1 ? 65 * 2 : 1);
    // (stage indices are compile-time constants at every call site of the 6-fold unrolled main loop: LDS addresses are a
    //  per-thread base register + an immediate)
    auto W = [&](int rstage, int ustage, const Regs &r) {
        float *us = smem + Cfg::OFF_U + ustage * Cfg::U;
        *reinterpret_cast<f32x4 *>(us + tid * 4) = r.u[0];
        *reinterpret_cast<f32x4 *>(us + tid * 4 + Cfg::NT * 4) = r.u[1];
        float *raw = smem + rstage * WG_RAW;
#pragma unroll
        for (int i = 0; i < Cfg::NROW; ++i) *reinterpret_cast<i32x2 *>(raw + raw_w + i * 132) = r.row[i];
        if (halo_wave && lane < 8) raw[halo_w] = r.halo;
    };
    // T in pieces, so that the main loop can spread it between its MFMAs.  d holds patch rows half .. half + ND / 4 - 1.
    const int t_row0 = raw_c + half * 132;
    auto T_read = [&](int rstage, float (&d)[Cfg::ND]) {
        const float *raw = smem + rstage * WG_RAW + t_row0;
#pragma unroll
        for (int i = 0; i < Cfg::ND / 4; ++i) {
            const f32x2 own = *reinterpret_cast<const f32x2 *>(raw + i * 132 + (lane + 1) * 2);
            d[i * 4 + 0] = raw[i * 132 + lo];
            d[i * 4 + 1] = own[0];
            d[i * 4 + 2] = own[1];
            d[i * 4 + 3] = raw[i * 132 + ro];
        }
    };
    // V = B^T d B,  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]: column pass of columns j0, j0 + 1, in place.  NW = 4: all four
    // transform rows; NW = 8: rows 2 * half, 2 * half + 1 land in d[0..3], d[4..7].  (Written on register pairs to get packed
    // v_pk_add_f32 the compiler spent more v_mov on forming the pairs than it saved: 110 VALU per chunk instead of 45.)
    auto T_col = [&](float (&d)[Cfg::ND], int j0) {
#pragma unroll
        for (int j = j0; j < j0 + 2; ++j) {
            if (NW == 4) {
                const float d0 = d[0 * 4 + j], d1 = d[1 * 4 + j], d2 = d[2 * 4 + j], d3 = d[3 * 4 + j];
                d[0 * 4 + j] = d0 - d2;
                d[1 * 4 + j] = d1 + d2;
                d[2 * 4 + j] = d2 - d1;
                d[3 * 4 + j] = d1 - d3;
            } else {
                const float e0 = d[0 * 4 + j], e1 = d[1 * 4 + j], e2 = d[2 * 4 + j];
                // half 0 holds patch rows 0, 1, 2: rows 0, 1 of B^T d = d0 - d2, d1 + d2;  half 1 holds 1, 2, 3: rows 2, 3 = d2 - d1, d1 - d3
                d[0 * 4 + j] = half ? e1 - e0 : e0 - e2;
                d[1 * 4 + j] = half ? e0 - e2 : e1 + e2;
            }
        }
    };
    // ... row pass of transform rows i0, i0 + 1 (as stored in d) and their 8 positions to V[p][c][t]
    const int v_w = (half * 8) * (WG_T * WG_CK) + sc * WG_T + lane;
    auto T_row = [&](int vstage, const float (&t)[Cfg::ND], int i0) {
        float *v = smem + vstage * WG_V + v_w;
#pragma unroll
        for (int i = i0; i < i0 + 2; ++i) {
            v[(i * 4 + 0) * (WG_T * WG_CK)] = t[i * 4 + 0] - t[i * 4 + 2];
            v[(i * 4 + 1) * (WG_T * WG_CK)] = t[i * 4 + 1] + t[i * 4 + 2];
            v[(i * 4 + 2) * (WG_T * WG_CK)] = t[i * 4 + 2] - t[i * 4 + 1];
            v[(i * 4 + 3) * (WG_T * WG_CK)] = t[i * 4 + 1] - t[i * 4 + 3];
        }
    };

    // operand lane bases (floats): position p = ph * 8 + pp
    const int a_base = Cfg::OFF_U + (ph * 8) * (BK * WG_CK) + (kq * 32 + li) * WG_CK + lh * 2;
    const int b_base = (ph * 8) * (WG_T * WG_CK) + (2 * lh) * WG_T + tq * 32 + li;
    struct Ops {
        f32x2 a;
        float b0, b1;
    };
    auto read_ops = [&](int vstage, int k, int pp, Ops &o) {
        o.a = *reinterpret_cast<const f32x2 *>(smem + k * Cfg::U + a_base + pp * (BK * WG_CK));
        const float *vs = smem + vstage * WG_V + b_base + pp * (WG_T * WG_CK);
        o.b0 = vs[0], o.b1 = vs[WG_T];
    };

    f32x16 acc[8];
#pragma unroll
    for (int pp = 0; pp < 8; ++pp)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[pp][e] = 0.0f;

    // zero slots of the raw rows (never written by W): slot 0 element 0, slot 65 element 1 -- 2 stages x 4 channels x 4 rows x 2
    if (tid < 64) smem[Cfg::OFF_RAW + (tid >> 1) * 132 + (tid & 1 ? 65 * 2 + 1 : 0)] = 0.0f;

    const int last = g.nch - 1;
    auto clampc = [&](int c) { return min(c, last); };
    float d[Cfg::ND];                  // the raw patch of T(it + 1), read before iteration `it` starts
    Ops o0, o1;                        // operands of M(it)'s first two positions, likewise
    G(0, rs[0]);
    G(clampc(1), rs[1]);
    G(clampc(2), rs[2]);
    W(0, 0, rs[0]);
    G(clampc(3), rs[0]);
    __syncthreads();
    T_read(0, d);
    T_col(d, 0);
    T_col(d, 2);
    T_row(0, d, 0);
    if (NW == 4) T_row(0, d, 2);
    W(1, 1, rs[1]);
    G(clampc(4), rs[1]);
    __syncthreads();
    T_read(1, d);
    read_ops(0, 0, 0, o0);
    read_ops(0, 0, 1, o1);
#define WG_MMA(pp, o)                                                                        \
    acc[pp] = __builtin_amdgcn_mfma_f32_32x32x2f32((o).a[0], (o).b0, acc[pp], 0, 0, 0);      \
    acc[pp] = __builtin_amdgcn_mfma_f32_32x32x2f32((o).a[1], (o).b1, acc[pp], 0, 0, 0)
    // iteration `it`: k = it % 3 (U stage, register set), p = it & 1 (V / raw stage) -- constants at the six call sites.
    // (operands are read two positions = 256 MFMA cycles before their MFMAs)
    auto iter = [&](int it, int k, int p, Regs &r) {
        Ops o2, o3, o4, o5, o6, o7;
        read_ops(p, k, 2, o2);
        WG_MMA(0, o0);
        T_col(d, 0);
        WACC_FENCE();
        read_ops(p, k, 3, o3);
        WG_MMA(1, o1);
        T_col(d, 2);
        WACC_FENCE();
        read_ops(p, k, 4, o4);
        WG_MMA(2, o2);
        T_row(p ^ 1, d, 0);                                // T(it + 1) -> V stage of it + 1
        WACC_FENCE();
        read_ops(p, k, 5, o5);
        read_ops(p, k, 6, o6);
        read_ops(p, k, 7, o7);
        WG_MMA(3, o3);
        if (NW == 4) T_row(p ^ 1, d, 2);
        W(p, (k + 2) % 3, r);                              // W(it + 2) -> raw stage of it + 2, U stage (it + 2) % 3
        WACC_FENCE();
        __syncthreads();
        WACC_FENCE();
        WG_MMA(4, o4);
        G(clampc(it + 5), r);
        WACC_FENCE();
        WG_MMA(5, o5);
        T_read(p, d);                                      // raw patch of T(it + 2)
        WACC_FENCE();
        WG_MMA(6, o6);
        read_ops(p ^ 1, (k + 1) % 3, 0, o0);
        WACC_FENCE();
        WG_MMA(7, o7);
        read_ops(p ^ 1, (k + 1) % 3, 1, o1);
        WACC_FENCE();
    };
    for (int it = 0; it < g.nch; it += 6) {
        iter(it, 0, 0, rs[2]);
        if (it + 1 < g.nch) iter(it + 1, 1, 1, rs[0]);
        if (it + 2 < g.nch) iter(it + 2, 2, 0, rs[1]);
        if (it + 3 < g.nch) iter(it + 3, 0, 1, rs[2]);
        if (it + 4 < g.nch) iter(it + 4, 1, 0, rs[0]);
        if (it + 5 < g.nch) iter(it + 5, 2, 1, rs[1]);
    }
    __syncthreads();                   // (the trailing prefetch reads are done before the epilogue reuses the LDS)

    // ---- epilogue: output transform  Y = A^T M A,  A^T = [1 1 1 0; 0 1 -1 -1];  position p = 4 i + j, this wave holds i = 2 ph, 2 ph + 1
    f32x16 own[2], give[2];                    // [b]: the output row this wave finishes (a = ph) / the other row's partial
    {
        f32x16 r0[2], r1[2];                   // R[il][b] = sum_j A^T[b][j] M[i][j]
        r0[0] = acc[0] + acc[1] + acc[2];
        r0[1] = acc[1] - acc[2] - acc[3];
        r1[0] = acc[4] + acc[5] + acc[6];
        r1[1] = acc[5] - acc[6] - acc[7];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (ph == 0) {                     // i = 0, 1:  Y0 += R0 + R1,  Y1 += R1
                own[b] = r0[b] + r1[b];
                give[b] = r1[b];
            } else {                           // i = 2, 3:  Y0 += R2,  Y1 += -R2 - R3
                own[b] = -r0[b] - r1[b];
                give[b] = r0[b];
            }
        }
    }
    // exchange buffer [wave][b * 16 + e][lane]; the partner of wave w is w ^ 2
    float *xch = smem;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) xch[(wave * 32 + b * 16 + e) * 64 + lane] = give[b][e];
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) own[b][e] += xch[((wave ^ 2) * 32 + b * 16 + e) * 64 + lane];

    const int64_t tg = t0 + tq * 32 + li;
    const bool tv = tg < g.tiles_total;
    const int n = (int)(tg / g.tiles_img), r = (int)(tg % g.tiles_img);
    const int ty = r / g.tw, tx = r % g.tw;
    float *yout = y + ((int64_t)n * g.M) * HW + (2 * ty + ph) * g.W + 2 * tx;
    float s1[16], s2[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int co = kb * BK + kq * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        float v0 = own[0][e], v1 = own[1][e];
        if (bias != nullptr) {
            const float bv = bias[co < g.M ? co : 0];
            v0 += bv, v1 += bv;
        }
        if (tv && co < g.M) {
            f32x2 o;
            o[0] = v0, o[1] = v1;
            *reinterpret_cast<f32x2 *>(yout + (int64_t)co * HW) = o;
        }
        if (STATS) {
            s1[e] = tv ? v0 + v1 : 0.0f;
            s2[e] = tv ? v0 * v0 + v1 * v1 : 0.0f;
        }
    }
    if (STATS) {
#pragma unroll
        for (int e = 0; e < 16; ++e)
#pragma unroll
            for (int off = 1; off < 32; off <<= 1) {
                s1[e] += __shfl_xor(s1[e], off);
                s2[e] += __shfl_xor(s2[e], off);
            }
        __syncthreads();                       // the exchange buffer has been read
        float *red = smem;                     // [wave][32 channels][2]
        if (li == 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int cl = (e & 3) + 8 * (e >> 2) + 4 * lh;
                red[(wave * 32 + cl) * 2 + 0] = s1[e];
                red[(wave * 32 + cl) * 2 + 1] = s2[e];
            }
        }
        __syncthreads();
        if (tid < BK && kb * BK + tid < g.M) {  // channel tid: waves kq = tid / 32, (tq, ph) = 0..3
            float a = 0.0f, b = 0.0f;
#pragma unroll
            for (int w2 = 0; w2 < 4; ++w2) {
                a += red[(((tid >> 5) * 4 + w2) * 32 + (tid & 31)) * 2 + 0];
                b += red[(((tid >> 5) * 4 + w2) * 32 + (tid & 31)) * 2 + 1];
            }
            const unsigned ntb = gridDim.x / g.nkb;
            float *dst = stats + ((int64_t)(kb * BK + tid) * ntb + tb) * 2;
            dst[0] = a;
            dst[1] = b;
        }
    }
}

// ------------------------------------------------------------------------------ one wave = one unit ("k_wg1")
// A wave computes 32 output channels x 32 tiles for ALL 16 positions by itself: 256 accumulator registers (one wave per SIMD, the
// whole 512-entry register file), no cooperation between waves, hence NO barrier and no V / U staging through LDS:
//   * lane (li, lh) transforms the patches of tile li for channels 2 lh, 2 lh + 1 of the chunk -- and those 2 x 16 values ARE
//     its B operands (lanes 0-31 feed k = channel 0 / 1, lanes 32-63 channel 2 / 3 of the two MFMAs of a position);
//   * the A operands come straight from global memory in per-lane order: Up1[k block][chunk][q][lane][4] (positions 2q, 2q + 1 x
//     channels 2 lh, 2 lh + 1 of output channel li), 8 float4 per lane and chunk, L1 / L2 resident (the four waves of a block
//     share the k block);
//   * only the raw patch rows go through LDS, inside the wave (no synchronisation: a wave's LDS operations complete in order):
//     8 buffer_load_dwordx2 (4 rows x 2 channels, lane = aligned column pair of its tile) + 1 dword load for the 32 halo values,
//     written to raw[c][row][slot][2], read back with the neighbours' halves.
// Per chunk and wave: 32 MFMAs against 17 vector-memory, 25 LDS and ~70 vector-ALU instructions (the 4-wave block: 16 MFMAs
// against 7 + 33 + 50) -- and nothing to wait for at a barrier.
constexpr int W1_T = 32;                                  // tiles per wave
constexpr int W1_ROW = (W1_T + 2) * 2;                    // floats of a raw row: slot 0 = left halo, 1 + t, 33 = right halo
constexpr int W1_RAW = 4 * 4 * W1_ROW;                    // one stage: [channel][row][slot][2] = 1088 floats
constexpr int W1_U = 16 * 32 * WG_CK;                     // floats of U per (k block, chunk)

// U in per-lane order (see above); rec = kb * nch + ch
__device__ __forceinline__ void wg1_pack_one(int64_t o, const float *__restrict__ w, const float *__restrict__ pm, float thr,
                                             float *__restrict__ up, int C, int M, int Cin, int nch, int dgrad,
                                             int *__restrict__ live, int Mp) {
    {
        const int cl = (int)(o % WG_CK);
        const int kl = (int)((o / WG_CK) % 32);
        const int64_t rec = o / (WG_CK * 32);
        const int ch = (int)(rec % nch), kb = (int)(rec / nch);
        const int m = kb * 32 + kl, c = wg_chunk_base(ch, Cin) + cl;     // (the last chunk may overlap the one before: wg_chunk_base)
        float g[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) g[r][s] = 0.0f;
        if (m < M && c >= ch * WG_CK) {
            const int co = dgrad ? c : m, ci = dgrad ? m : c;
            const int64_t off = ((int64_t)co * C + ci) * 9;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int tap = dgrad ? 8 - (r * 3 + s) : r * 3 + s;
                    float v = w[off + tap];
                    if (pm != nullptr) v *= binarize(pm[off + tap], thr);
                    g[r][s] = v;
                }
        }
        if (live != nullptr) {                  // liveness flags (zeroed by the caller): plain stores of 1, same-value races are benign
            bool nz = false;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) nz |= g[r][s] != 0.0f;
            if (nz) {
                live[m] = 1;
                live[Mp + 4 + ch] = 1;
            }
        }
        float t[4][3], u[16];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            t[0][s] = g[0][s];
            t[1][s] = 0.5f * (g[0][s] + g[1][s] + g[2][s]);
            t[2][s] = 0.5f * (g[0][s] - g[1][s] + g[2][s]);
            t[3][s] = g[2][s];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u[i * 4 + 0] = t[i][0];
            u[i * 4 + 1] = 0.5f * (t[i][0] + t[i][1] + t[i][2]);
            u[i * 4 + 2] = 0.5f * (t[i][0] - t[i][1] + t[i][2]);
            u[i * 4 + 3] = t[i][2];
        }
        // lane = (lh = cl / 2) * 32 + kl; float (p & 1) * 2 + (cl & 1) of float4 q = p / 2
        float *dst = up + rec * W1_U + ((cl >> 1) * 32 + kl) * 4 + (cl & 1);
#pragma unroll
        for (int p = 0; p < 16; ++p) dst[(p >> 1) * 256 + (p & 1) * 2] = u[p];
    }
}

__global__ __launch_bounds__(256) void k_wg1_pack(const float *__restrict__ w, const float *__restrict__ pm, float thr,
                                                  float *__restrict__ up, int K, int C, int M, int Cin, int nch, int dgrad,
                                                  int *__restrict__ live, int Mp) {
    const int64_t total = (int64_t)((M + 31) / 32) * nch * 32 * WG_CK;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x)
        wg1_pack_one(o, w, pm, thr, up, C, M, Cin, nch, dgrad, live, Mp);
}

// Up to two pack jobs in ONE launch (cpg_conv2d_pack: a training step's forward and input-gradient operands of a layer -- the same
// weights in two layouts): work items [0, a.total) are job a's, [a.total, a.total + b.total) job b's.  Family 1 is pointwise.hip's
// k_pw_pack (Wp[c][m] = W[co][ci] * bin(pm), fwd: c = ci, m = co; dgrad: c = co, m = ci), family 2 wg1_pack_one above.
struct PackArgs {
    int family, K, C, a, b, c, d;
    long long total;
    float *out;
};
__device__ __forceinline__ void pack_job_one(const PackArgs &j, int64_t o, const float *__restrict__ w, const float *__restrict__ pm, float thr) {
    if (j.family == 1) {
        const int Mp = j.b, dgrad = j.c;
        const int m = (int)(o % Mp), c = (int)(o / Mp);
        const int co = dgrad ? c : m, ci = dgrad ? m : c;
        float v = 0.0f;
        if (co < j.K && ci < j.C) {
            const int64_t off = (int64_t)co * j.C + ci;
            v = w[off];
            if (pm != nullptr) v *= binarize(pm[off], thr);
        }
        j.out[o] = v;
    } else {
        wg1_pack_one(o, w, pm, thr, j.out, j.C, j.a, j.b, j.c, j.d, nullptr, 0);
    }
}
__global__ __launch_bounds__(256) void k_pack_jobs(const PackArgs a, const PackArgs b, const float *__restrict__ w,
                                                   const float *__restrict__ pm, float thr) {
    const int64_t total = a.total + b.total;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        if (o < a.total)
            pack_job_one(a, o, w, pm, thr);
        else
            pack_job_one(b, o - a.total, w, pm, thr);
    }
}

// Inference: eval-mode BatchNorm (+ ReLU) in the epilogue -- the expression of conv3x3.hip's C3BnEval -- and the dead-channel skip:
// `live` (may be null) are the flags k_wg1_pack wrote, same layout as k_c3_pack's (live[m]: output channel m has a non-zero
// weight; live[Mp + 4 + q]: input chunk q has one; live[Mp] receives 4 x the chunks up to the last live one, live[Mp + 1] counts
// the waves that skipped their MFMA loop).
// One parameter block for both inference epilogues (cpg::EvalEpilogue, filled by wg_epilogue): the BNE instances read the members, the PRE
// instances (y = prelu(conv + bias) [+ residual], cpg_common.h's prelu_one / prelu_sum) slope(), residual() and per_channel(); `live`, Mp
// are common.  (Accessors, where conv3x3.hip's C3BnEval has unions: a read through a union member loses its struct-path alias
// information, and k_wg3<ODD, PRE> then compiles to other code -- tools/build_digest.py.)
struct WgBnEval {
    const float *gamma, *beta, *mean, *var;
    float eps;
    int relu;
    int *live;
    int Mp;
    __host__ __device__ const float *slope() const { return gamma; }
    __host__ __device__ const float *residual() const { return beta; }
    __host__ __device__ int per_channel() const { return relu; }
};

// -DWG_TIMING (development builds only, tools/attic/diag_wg_timing.py): every wave of k_wg1 leaves the constant-clock time of its
// entry / prologue start / main loop start / epilogue start / exit and its hardware slot in wg_dbg.
#ifdef WG_TIMING
__device__ unsigned long long wg_dbg[65536 * 8];
#define WG_STAMP(i) do { if (lane == 0 && dbg_u < 65536) wg_dbg[dbg_u * 8 + (i)] = wall_clock64(); } while (0)
#else
#define WG_STAMP(i)
#endif
// POOL (inference launches, with BNE: the same skip; even maps): the MaxPool2d(2, 2) behind the BatchNorm (+ ReLU) too.  A tile's 2x2 outputs ARE
// one pool window and this wave holds all four in one lane: `y` is the POOLED tensor [N][M][H/2][W/2], one dword per (channel, tile) at the
// tile's own index inside its image; the full-resolution activation is never written.
template <bool DGRAD, bool STATS, bool BNE = false, bool PRE = false, bool POOL = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_wg1(WgGeom g, const float *__restrict__ x, const float *__restrict__ up, const float *__restrict__ bias,
           float *__restrict__ y, float *__restrict__ stats, WgBnEval bn) {
    static_assert(!PRE || (BNE && !DGRAD && !STATS), "the PReLU epilogue is an inference epilogue");
    static_assert(!POOL || (BNE && !PRE && !DGRAD && !STATS), "the pooled epilogue is the BatchNorm inference epilogue's");
    __shared__ __attribute__((aligned(16))) float smem_all[4 * 2 * W1_RAW];
    // (readfirstlane: tells the compiler the wave index is wave-uniform, so that everything derived from it -- the tile run, the
    //  buffer descriptor of its first image -- lives in scalar registers; without it every buffer load became a waterfall loop)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int HW = g.H * g.W;
    float *smem = smem_all + wave * 2 * W1_RAW;               // this wave's private raw stages
    // PERSISTENT blocks: the grid is at most a few times what the chip holds (one block per CU: 512 registers per wave; see
    // wino_grids) and every wave walks over the logical blocks base + blockIdx, base += gridDim -- no dispatch gap between
    // units (0.6 us of 27 on the 64-channel layers), the kernel arguments and the code stay where they are.
    for (unsigned base = 0; base < g.nblocks; base += gridDim.x) {
    // (virtual block v runs on XCD v % 8 = blockIdx % 8 -- the grid is a multiple of 8 blocks whenever there is more than one
    //  round -- and XCD x owns the x-th eighth of ALL logical blocks, walking through it round after round: consecutive tile runs,
    //  which share half of their input rows, stay in one XCD's L2 as with one block per logical block)
    const unsigned v = base + blockIdx.x;
    if (v >= g.nblocks) break;
    const unsigned lb = xcd_remap(v, g.nblocks);
    const int kb = lb % g.nkb;
    // (32-bit tile arithmetic: the host refuses N * tiles >= 2^31; 64-bit divisions cost the prologue ~1.5 us per wave)
    const unsigned ttot = (unsigned)g.tiles_total, timg = (unsigned)g.tiles_img, twu = (unsigned)g.tw;
    const unsigned run = (lb / g.nkb) * 4 + wave;             // tile run of 32
    const unsigned t0 = run * W1_T;
    if (t0 >= ttot) continue;                                 // (no barriers anywhere: a wave may skip)
#ifdef WG_TIMING
    const unsigned dbg_u = lb * 4 + wave;
    WG_STAMP(0);
    if (lane == 0 && dbg_u < 65536) wg_dbg[dbg_u * 8 + 6] = __builtin_amdgcn_s_getreg(63492), wg_dbg[dbg_u * 8 + 7] = __builtin_amdgcn_s_getreg(63508);
#endif
    const int n0 = (int)(t0 / timg);

    constexpr int kOutOfRange = (int)0x80000000;
    int roff[4], hoff, lo, ro;
    {
        const unsigned tg = t0 + li;
        const bool tv = tg < ttot;
        const int n = (int)(tg / timg), r = (int)(tg % timg);
        const int ty = (int)((unsigned)r / twu), tx = (int)((unsigned)r % twu);
        const int cbase = ((n - n0) * g.C + 2 * lh) * HW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gh = 2 * ty - 1 + i;
            roff[i] = (tv && (unsigned)gh < (unsigned)g.H) ? (cbase + gh * g.W + 2 * tx) * 4 : kOutOfRange;
        }
        lo = tx == 0 ? 0 : (li + 1) * 2 - 1;
        ro = tx == g.tw - 1 ? (W1_T + 1) * 2 + 1 : (li + 1) * 2 + 2;
        // halo: lanes 0-31 = (side, row, channel): the column left of tile t0 / right of tile t0 + 31
        const int side = (lane >> 4) & 1, hi = (lane >> 2) & 3, hc = lane & 3;
        const unsigned th = side ? t0 + W1_T - 1 : t0;
        const int nh = (int)(th / timg), rh = (int)(th % timg);
        const int tyh = (int)((unsigned)rh / twu), txh = (int)((unsigned)rh % twu);
        const int ghh = 2 * tyh - 1 + hi, gwh = side ? 2 * txh + 2 : 2 * txh - 1;
        const bool okh = lane < 32 && th < ttot && (unsigned)ghh < (unsigned)g.H && (unsigned)gwh < (unsigned)g.W;
        hoff = okh ? (((nh - n0) * g.C + hc) * HW + ghh * g.W + gwh) * 4 : kOutOfRange;
    }
    const int span = (W1_T + g.tiles_img - 1) / g.tiles_img + 1;
    const int nimg_here = min(span, g.N - n0);
    // byte offset of the LAST chunk's first channel, set once the chunk count is known: min(last chunk * 4, C - 4) channels.  Every row load
    // takes min(chunk * stride, x_last_off): chunks past the end re-read the last one (what clampc did for them), and with a channel count
    // that is no multiple of 4 the last chunk starts at C - 4, overlapping its neighbour (wg_chunk_base; the pack kernel zeroes its filters
    // for the channels the neighbour already contracted) -- one scalar multiply and one min per chunk, as before.
    int x_last_off = 0, x_last = 0;
    const __amdgpu_buffer_rsrc_t srd_x =
        __builtin_amdgcn_make_buffer_rsrc((void *)(x + (int64_t)n0 * g.C * HW), 0, nimg_here * g.C * HW * 4, 0x00020000);
    // (U through a buffer descriptor: two per-lane byte offsets per unit, the chunk in the scalar offset, q in the instruction offset)
    const __amdgpu_buffer_rsrc_t srd_u = __builtin_amdgcn_make_buffer_rsrc((void *)up, 0, (int)((int64_t)g.nkb * g.nch * W1_U * 4), 0x00020000);
    const int ubase = (kb * g.nch * W1_U + lane * 4) * 4;

    // raw[c][row][slot][2] offsets of this lane (channels 2 lh + j)
    const int raw_own = (2 * lh) * 4 * W1_ROW + (li + 1) * 2;
    const int halo_w = ((lane & 3) * 4 + ((lane >> 2) & 3)) * W1_ROW + (((lane >> 4) & 1) ? (W1_T + 1) * 2 : 1);
    // zero slots (never written): slot 0 element 0, slot 33 element 1 of the 2 x 16 rows
    if (lane < 32) {
        smem[lane * W1_ROW] = 0.0f;
        smem[lane * W1_ROW + (W1_T + 1) * 2 + 1] = 0.0f;
    }

    struct Rows {
        i32x2 r[2][4];
        float halo;
    };
    auto G_row1 = [&](int ch, Rows &q, int k) {             // k = 0..7: row k & 3 of channel 2 lh + k / 4;  k = 8: the halo values
        // (the inference instance has no scalar register left for x_last_off -- it spilled a vector register pair to scratch --: it clamps the
        //  chunk index with `last`, which its filter loads keep live anyway)
        const int soff = BNE ? wg_chunk_base(min(ch, x_last), g.C) * HW * 4 : min(ch * (WG_CK * HW * 4), x_last_off);      // (see x_last_off)
        if (k < 8)
            q.r[k >> 2][k & 3] = __builtin_amdgcn_raw_buffer_load_b64(srd_x, roff[k & 3], soff + (k >> 2) * HW * 4, 0);
        else
            q.halo = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_x, hoff, soff, 0));
    };
    auto G_rows = [&](int ch, Rows &q) {
#pragma unroll
        for (int k = 0; k < 9; ++k) G_row1(ch, q, k);
    };
    auto W_row1 = [&](int stage, const Rows &q, int k) {
        float *raw = smem + stage * W1_RAW;
        if (k < 8)
            *reinterpret_cast<i32x2 *>(raw + raw_own + k * W1_ROW) = q.r[k >> 2][k & 3];
        else if (lane < 32)
            raw[halo_w] = q.halo;
    };
    auto W_rows = [&](int stage, const Rows &q) {
#pragma unroll
        for (int k = 0; k < 9; ++k) W_row1(stage, q, k);
    };
    const int ubase4 = ubase + 4 * 256 * 4;                   // (the instruction offset has 12 bits: q = 4 .. 7 from a second base)
    auto G_u1 = [&](int ch, f32x4 (&u)[8], int q) {
        u[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_u, (q < 4 ? ubase : ubase4) + (q & 3) * 256 * 4, ch * (W1_U * 4), 0));
    };
    auto G_u = [&](int ch, f32x4 (&u)[8]) {
#pragma unroll
        for (int q = 0; q < 8; ++q) G_u1(ch, u, q);
    };
    // patch of (tile li, channel 2 lh + j) -> the 16 transform-domain values, in place
    auto T_read2 = [&](int stage, int j, float (&d)[16], int i0) {       // patch rows i0, i0 + 1
        const float *raw = smem + stage * W1_RAW + (2 * lh + j) * 4 * W1_ROW;
#pragma unroll
        for (int i = i0; i < i0 + 2; ++i) {
            const f32x2 own = *reinterpret_cast<const f32x2 *>(raw + i * W1_ROW + (li + 1) * 2);
            d[i * 4 + 0] = raw[i * W1_ROW + lo];
            d[i * 4 + 1] = own[0];
            d[i * 4 + 2] = own[1];
            d[i * 4 + 3] = raw[i * W1_ROW + ro];
        }
    };
    auto T_read = [&](int stage, int j, float (&d)[16]) {
        const float *raw = smem + stage * W1_RAW + (2 * lh + j) * 4 * W1_ROW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 own = *reinterpret_cast<const f32x2 *>(raw + i * W1_ROW + (li + 1) * 2);
            d[i * 4 + 0] = raw[i * W1_ROW + lo];
            d[i * 4 + 1] = own[0];
            d[i * 4 + 2] = own[1];
            d[i * 4 + 3] = raw[i * W1_ROW + ro];
        }
    };
    auto T_col = [&](float (&d)[16], int j0) {
#pragma unroll
        for (int j = j0; j < j0 + 2; ++j) {
            const float d0 = d[0 * 4 + j], d1 = d[1 * 4 + j], d2 = d[2 * 4 + j], d3 = d[3 * 4 + j];
            d[0 * 4 + j] = d0 - d2;
            d[1 * 4 + j] = d1 + d2;
            d[2 * 4 + j] = d2 - d1;
            d[3 * 4 + j] = d1 - d3;
            asm volatile("" : "+v"(d[0 * 4 + j]), "+v"(d[1 * 4 + j]), "+v"(d[2 * 4 + j]), "+v"(d[3 * 4 + j]));
        }
    };
    // (the asm "uses" pin the results where they are computed: their only consumers are the NEXT iteration's MFMAs, and the
    //  optimizer otherwise sinks the whole transform -- 64 adds -- in front of them, where nothing runs in its shadow)
    auto T_rowp = [&](float (&d)[16], int i) {
        const float t0_ = d[i * 4 + 0], t1 = d[i * 4 + 1], t2 = d[i * 4 + 2], t3 = d[i * 4 + 3];
        d[i * 4 + 0] = t0_ - t2;
        d[i * 4 + 1] = t1 + t2;
        d[i * 4 + 2] = t2 - t1;
        d[i * 4 + 3] = t1 - t3;
        asm volatile("" : "+v"(d[i * 4 + 0]), "+v"(d[i * 4 + 1]), "+v"(d[i * 4 + 2]), "+v"(d[i * 4 + 3]));
    };


    int nch = g.nch;
    if (BNE && bn.live != nullptr) {                          // inference: skip what apply_mask killed (wave-uniform decisions)
        const int alive = (kb * 32 + li < g.M) ? bn.live[kb * 32 + li] : 0;
        const bool dead = __ballot(alive != 0) == 0ull;
        int lastc = g.nch;
        while (lastc > 0 && bn.live[bn.Mp + 4 + lastc - 1] == 0) --lastc;
        nch = dead ? 0 : lastc;
        if (lane == 0) {
            if (dead) atomicAdd(&bn.live[bn.Mp + 1], 1);
            if (blockIdx.x == 0 && wave == 0) bn.live[bn.Mp] = lastc * WG_CK;
        }
    }
    const int last = nch - 1;
    x_last = last;
    if (!BNE) x_last_off = __builtin_amdgcn_readfirstlane(min(last * WG_CK, g.C - WG_CK) * HW * 4);
    auto clampc = [&](int c) { return min(c, last); };
    f32x4 u0[8], u1[8], u2[8];             // U of chunks it, it + 1, it + 2 (three rotating sets: requested two iterations ahead)
    float b0[16], b1[16];                  // B operands of the current chunk: V of channels 2 lh, 2 lh + 1
    float n0v[16], n1v[16];                // ... of the next chunk, transformed while the current chunk's MFMAs run
    Rows rw0, rw1;                         // raw rows in flight: chunk c uses set c & 1, requested FOUR iterations before its MFMAs
    // With one wave per SIMD a wait is an idle MFMA pipe: the loads that miss L2 (the transformed filter of a 512 x 512 layer is
    // 16 MB, the input's first touch) take longer than one iteration (0.85 us), so everything is requested two iterations early.
    WG_STAMP(1);
    // prologue: chunk 0 operands, chunks 0 / 1 raw rows in LDS, chunks 2 / 3 rows and U(0), U(1) in flight
    if (nch > 0) {
    G_rows(0, rw0);
    G_rows(clampc(1), rw1);
    G_u(0, u0);
    G_u(clampc(1), u1);
    }
    // the accumulators are cleared while those loads fly (256 instructions, 0.4 us)
    __builtin_amdgcn_sched_barrier(0);
    WACC_ZERO_ALL();
    __builtin_amdgcn_sched_barrier(0);
    if (nch > 0) {
    W_rows(0, rw0);
    W_rows(1, rw1);
    G_rows(clampc(2), rw0);
    G_rows(clampc(3), rw1);
    T_read(0, 0, b0);
    T_read(0, 1, b1);
    T_col(b0, 0); T_col(b0, 2); T_col(b1, 0); T_col(b1, 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) { T_rowp(b0, i); T_rowp(b1, i); }
    }

    // The 256 accumulators live in fixed accumulation registers, behind the WACC_* macros of wino_acc.h (which says why).
// MFMA h (0: channels 0 / 2 of the chunk, 1: channels 1 / 3) of position p, then a slice of the staging work, then a fence.  ONE
// MFMA per slot: a wave issues in order, so whatever stands behind an MFMA pair only gets the second one's 64-cycle shadow --
// with 9 loads or 9 LDS writes in one slot the matrix pipe waited for the memory pipelines' issue
#define W1_SLOT(p, h, U, B, work)                                                      \
    WACC_MMA_##p((U)[(p) >> 1][((p) & 1) * 2 + (h)], (B)[p]);                            \
    work;                                                                              \
    WACC_FENCE()
    // iteration it (par = it & 1): M(it) from (ucur, c0, c1); T(it + 1) from raw stage (it + 1) & 1 into (x0, x1); W(it + 2) from
    // the row set of this parity, which is then re-used for the loads of chunk it + 4; U(it + 2) is requested at the top
    auto iter = [&](int it, int par, f32x4 (&ucur)[8], f32x4 (&ufar)[8], Rows &rows, float (&c0)[16], float (&c1)[16],
                    float (&x0)[16], float (&x1)[16]) {
        const int cu = clampc(it + 2), cr = it + 4;
        W1_SLOT(0, 0, ucur, c0, T_read2(par ^ 1, 0, x0, 0));
        W1_SLOT(0, 1, ucur, c1, T_read2(par ^ 1, 0, x0, 2));
        W1_SLOT(1, 0, ucur, c0, T_read2(par ^ 1, 1, x1, 0));
        W1_SLOT(1, 1, ucur, c1, T_read2(par ^ 1, 1, x1, 2));
        W1_SLOT(2, 0, ucur, c0, T_col(x0, 0));
        W1_SLOT(2, 1, ucur, c1, T_col(x0, 2));
        W1_SLOT(3, 0, ucur, c0, T_col(x1, 0));
        W1_SLOT(3, 1, ucur, c1, T_col(x1, 2));
        W1_SLOT(4, 0, ucur, c0, T_rowp(x0, 0));
        W1_SLOT(4, 1, ucur, c1, T_rowp(x0, 1));
        W1_SLOT(5, 0, ucur, c0, T_rowp(x0, 2));
        W1_SLOT(5, 1, ucur, c1, T_rowp(x0, 3));
        W1_SLOT(6, 0, ucur, c0, T_rowp(x1, 0));
        W1_SLOT(6, 1, ucur, c1, T_rowp(x1, 1));
        W1_SLOT(7, 0, ucur, c0, T_rowp(x1, 2));
        W1_SLOT(7, 1, ucur, c1, T_rowp(x1, 3));
        W1_SLOT(8, 0, ucur, c0, G_u1(cu, ufar, 0));
        W1_SLOT(8, 1, ucur, c1, G_u1(cu, ufar, 1));
        W1_SLOT(9, 0, ucur, c0, G_u1(cu, ufar, 2));
        W1_SLOT(9, 1, ucur, c1, G_u1(cu, ufar, 3));
        W1_SLOT(10, 0, ucur, c0, G_u1(cu, ufar, 4));
        W1_SLOT(10, 1, ucur, c1, G_u1(cu, ufar, 5));
        W1_SLOT(11, 0, ucur, c0, G_u1(cu, ufar, 6));
        W1_SLOT(11, 1, ucur, c1, G_u1(cu, ufar, 7));
        // rows of chunk it + 2 -> raw stage (it + 2) & 1, each register pair re-requested for chunk it + 4 right after its store
        W1_SLOT(12, 0, ucur, c0, W_row1(par, rows, 0); W_row1(par, rows, 1); G_row1(cr, rows, 0));
        W1_SLOT(12, 1, ucur, c1, W_row1(par, rows, 2); G_row1(cr, rows, 1));
        W1_SLOT(13, 0, ucur, c0, W_row1(par, rows, 3); G_row1(cr, rows, 2));
        W1_SLOT(13, 1, ucur, c1, W_row1(par, rows, 4); G_row1(cr, rows, 3));
        W1_SLOT(14, 0, ucur, c0, W_row1(par, rows, 5); G_row1(cr, rows, 4));
        W1_SLOT(14, 1, ucur, c1, W_row1(par, rows, 6); G_row1(cr, rows, 5));
        W1_SLOT(15, 0, ucur, c0, W_row1(par, rows, 7); G_row1(cr, rows, 6));
        W1_SLOT(15, 1, ucur, c1, W_row1(par, rows, 8); G_row1(cr, rows, 7); G_row1(cr, rows, 8));
    };
    WG_STAMP(2);
    for (int it = 0; it < nch; it += 6) {
        iter(it, 0, u0, u2, rw0, b0, b1, n0v, n1v);
        if (it + 1 < nch) iter(it + 1, 1, u1, u0, rw1, n0v, n1v, b0, b1);
        if (it + 2 < nch) iter(it + 2, 0, u2, u1, rw0, b0, b1, n0v, n1v);
        if (it + 3 < nch) iter(it + 3, 1, u0, u2, rw1, n0v, n1v, b0, b1);
        if (it + 4 < nch) iter(it + 4, 0, u1, u0, rw0, b0, b1, n0v, n1v);
        if (it + 5 < nch) iter(it + 5, 1, u2, u1, rw1, n0v, n1v, b0, b1);
    }

    WG_STAMP(3);
    // ---- epilogue: Y = A^T M A in registers (M[i][j] = acc[4 i + j]),  A^T = [1 1 1 0; 0 1 -1 -1]
    WACC_DRAIN();
    const unsigned tg = t0 + li;
    const bool tv = tg < ttot;
    const int n = (int)(tg / timg), r = (int)(tg % timg);
    const int ty = (int)((unsigned)r / twu), tx = (int)((unsigned)r % twu);
    float *yout = y + ((int64_t)n * g.M) * HW + (2 * ty) * g.W + 2 * tx;
    float *pout = y + ((int64_t)n * g.M) * g.tiles_img + r;       // (POOL) window (ty, tx) of image n, channel 0
    float s1[16], s2[16];
    // (PRE) the residual, at the store's own address + the uniform distance between the two tensors: nothing new for the compiler to keep
    // per lane across the main loop (this kernel's loop owns all 256 vector registers)
    const bool has_res = PRE && bn.residual() != nullptr;
    const intptr_t rdelta = has_res ? reinterpret_cast<intptr_t>(bn.residual()) - reinterpret_cast<intptr_t>(y) : 0;
    // hb: with / without a conv bias, decided ONCE outside (the two epilogues are separate code).  With the bias load behind a
    // branch inside the per-channel code the compiler's s_waitcnt vmcnt(0) for it sat in the common path: every channel waited for
    // the previous channel's stores to be acknowledged, 16 round trips = 3.9 us of a 29 us unit on the 64-channel layers
    // (tools/attic/diag_wg_timing.py); without it 2.7 us.
    auto out_e = [&](auto hb, int e, const float (&m)[16]) {       // m[4 i + j] = M[i][j] of output channel element e
        float r_[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r_[i][0] = m[i * 4 + 0] + m[i * 4 + 1] + m[i * 4 + 2];
            r_[i][1] = m[i * 4 + 1] - m[i * 4 + 2] - m[i * 4 + 3];
        }
        const int co = kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        float bv = 0.0f;
        if constexpr (decltype(hb)::value) bv = bias[co < g.M ? co : 0];
        float v00 = r_[0][0] + r_[1][0] + r_[2][0] + bv, v01 = r_[0][1] + r_[1][1] + r_[2][1] + bv;
        float v10 = r_[1][0] - r_[2][0] - r_[3][0] + bv, v11 = r_[1][1] - r_[2][1] - r_[3][1] + bv;
        if constexpr (PRE) {                   // y = prelu(conv + bias) [+ residual]
            const float a = bn.slope()[bn.per_channel() && co < g.M ? co : 0];
            v00 = prelu_one(v00, a), v01 = prelu_one(v01, a), v10 = prelu_one(v10, a), v11 = prelu_one(v11, a);
            if (has_res && tv && co < g.M) {
                const char *rp = reinterpret_cast<const char *>(yout + (int64_t)co * HW) + rdelta;
                const f32x2 r0 = *reinterpret_cast<const f32x2 *>(rp), r1 = *reinterpret_cast<const f32x2 *>(rp + (int64_t)g.W * 4);
                v00 = prelu_sum(v00, r0[0]), v01 = prelu_sum(v01, r0[1]);
                v10 = prelu_sum(v10, r1[0]), v11 = prelu_sum(v11, r1[1]);
            }
        } else if (BNE) {                      // y = [max(0,] (conv + bias - mean) * invstd * gamma + beta [)]
            const int cc = co < g.M ? co : 0;
            const float mu = bn.mean[cc], is = 1.0f / sqrtf(bn.var[cc] + bn.eps), ga = bn.gamma[cc], be = bn.beta[cc];
            v00 = (v00 - mu) * is * ga + be, v01 = (v01 - mu) * is * ga + be;
            v10 = (v10 - mu) * is * ga + be, v11 = (v11 - mu) * is * ga + be;
            if (bn.relu) v00 = relu_keep(v00), v01 = relu_keep(v01), v10 = relu_keep(v10), v11 = relu_keep(v11);
        }
        if constexpr (POOL) {                  // the two row maxima, then the window's: the order the two-wave kernels combine them in
            if (tv && co < g.M) pout[(int64_t)co * g.tiles_img] = max_keep(max_keep(v10, v11), max_keep(v00, v01));
        } else
        if (tv && co < g.M) {
            f32x2 o;
            o[0] = v00, o[1] = v01;
            *reinterpret_cast<f32x2 *>(yout + (int64_t)co * HW) = o;
            o[0] = v10, o[1] = v11;
            *reinterpret_cast<f32x2 *>(yout + (int64_t)co * HW + g.W) = o;
        }
        if (STATS) {
            s1[e] = tv ? (v00 + v01) + (v10 + v11) : 0.0f;
            s2[e] = tv ? (v00 * v00 + v01 * v01) + (v10 * v10 + v11 * v11) : 0.0f;
        }
    };
    auto out_all = [&](auto hb) {
        float m[16];
#define W1_OUT(e) WACC_RD16_##e(m); out_e(hb, e, m);
        WACC_EACH16(W1_OUT)
#undef W1_OUT
    };
    if (bias != nullptr) out_all(std::true_type{}); else out_all(std::false_type{});
    if (STATS) {
#pragma unroll
        for (int e = 0; e < 16; e += 8) half_wave_sum8(s1 + e), half_wave_sum8(s2 + e);
        if (li == kHalfSumLane) {
            const unsigned nruns = (ttot + W1_T - 1) / W1_T;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (co < g.M) {
                    float *dst = stats + ((int64_t)co * nruns + run) * 2;
                    f32x2 o;
                    o[0] = s1[e], o[1] = s2[e];
                    *reinterpret_cast<f32x2 *>(dst) = o;
                }
            }
        }
    }
    WG_STAMP(4);
    }   // next logical block
}

// ------------------------------------------------------------------------------ two waves = one unit ("k_wg2")
// k_wg1 split over the transform positions, built to test whether a SECOND wave per SIMD would fill the gaps the staging
// instructions leave in k_wg1's MFMA stream: a block is two waves that share a unit of 32 channels x 32 tiles, wave ph owns the
// positions of transform rows 2 ph, 2 ph + 1 -- 8 accumulators = 128 AGPRs, so two waves fit a SIMD (four independent blocks per
// CU).  Per chunk a wave fetches the three patch rows its positions need (ph .. ph + 2), does half of the input transform (16 adds
// per patch instead of 32: nothing is computed twice) and 16 MFMAs; the two waves meet once, in the epilogue, to swap the halves of
// the (linear) output transform through LDS.  RESULT: the same speed as k_wg1 within 1 % on every layer (34.5 vs 34.4 ms per VGG16
// pass) -- the time the other instructions take is not hidden by a second wave either; on this chip an fp32 MFMA and the fp32 vector
// adds / the memory instructions' register traffic share what they run on (the fp32 matrix and packed-vector peaks are the same
// number), so the cost is additive: MFMA time + ~4 cycles per vector add + ~8-16 per LDS / vector-memory instruction.  Kept behind
// CPG_WINO_KERNEL=pair (tested); not the default.
constexpr int W2_RAW = 4 * 3 * W1_ROW;                    // one stage of one wave: [channel][row 3][slot 34][2] = 816 floats



// POOL (see k_wg1): a wave ends the epilogue with output row ph of the tile.  It leaves max(v0, v1) in the exchange slot it has just read (the
// other wave's, consumed, nobody else looks at it); after one more barrier wave ph combines the two row maxima of accumulator elements
// 8 ph .. 8 ph + 7 (16 of the block's 32 channels) and stores them to the pooled tensor `y`.
template <bool DGRAD, bool STATS, bool BNE = false, bool PRE = false, bool POOL = false>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_wg2(WgGeom g, const float *__restrict__ x, const float *__restrict__ up, const float *__restrict__ bias,
           float *__restrict__ y, float *__restrict__ stats, WgBnEval bn) {
    static_assert(!POOL || (BNE && !PRE && !DGRAD && !STATS), "the pooled epilogue is the BatchNorm inference epilogue's");
    __shared__ __attribute__((aligned(16))) float smem_all[2 * 32 * 64];       // 2 x 2 raw stages (3264 floats) / the exchange buffer
    const int tid = threadIdx.x, lane = tid & 63, ph = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int HW = g.H * g.W;
    float *smem = smem_all + ph * 2 * W2_RAW;                 // this wave's private raw stages

    unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int kb = lb % g.nkb;
    const unsigned ttot = (unsigned)g.tiles_total, timg = (unsigned)g.tiles_img, twu = (unsigned)g.tw;
    const unsigned run = lb / g.nkb;                          // tile run of 32
    const unsigned t0 = run * W1_T;
    if (t0 >= ttot) return;                                   // (uniform for the block)
    const int n0 = (int)(t0 / timg);

    constexpr int kOutOfRange = (int)0x80000000;
    int roff[3], hoff, lo, ro;
    {
        const unsigned tg = t0 + li;
        const bool tv = tg < ttot;
        const int n = (int)(tg / timg), r = (int)(tg % timg);
        const int ty = (int)((unsigned)r / twu), tx = (int)((unsigned)r % twu);
        const int cbase = ((n - n0) * g.C + 2 * lh) * HW;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int gh = 2 * ty - 1 + ph + i;
            roff[i] = (tv && (unsigned)gh < (unsigned)g.H) ? (cbase + gh * g.W + 2 * tx) * 4 : kOutOfRange;
        }
        lo = tx == 0 ? 0 : (li + 1) * 2 - 1;
        ro = tx == g.tw - 1 ? (W1_T + 1) * 2 + 1 : (li + 1) * 2 + 2;
        // halo: lanes 0-23 = (side, row, channel): the column left of tile t0 / right of tile t0 + 31
        const int side = lane >= 12 ? 1 : 0, hl = lane - 12 * side, hi = hl >> 2, hc = hl & 3;
        const unsigned th = side ? t0 + W1_T - 1 : t0;
        const int nh = (int)(th / timg), rh = (int)(th % timg);
        const int tyh = (int)((unsigned)rh / twu), txh = (int)((unsigned)rh % twu);
        const int ghh = 2 * tyh - 1 + ph + hi, gwh = side ? 2 * txh + 2 : 2 * txh - 1;
        const bool okh = lane < 24 && th < ttot && (unsigned)ghh < (unsigned)g.H && (unsigned)gwh < (unsigned)g.W;
        hoff = okh ? (((nh - n0) * g.C + hc) * HW + ghh * g.W + gwh) * 4 : kOutOfRange;
    }
    const int span = (W1_T + g.tiles_img - 1) / g.tiles_img + 1;
    const int nimg_here = min(span, g.N - n0);
    // byte offset of the LAST chunk's first channel, set once the chunk count is known: min(last chunk * 4, C - 4) channels.  Every row load
    // takes min(chunk * stride, x_last_off): chunks past the end re-read the last one (what clampc did for them), and with a channel count
    // that is no multiple of 4 the last chunk starts at C - 4, overlapping its neighbour (wg_chunk_base; the pack kernel zeroes its filters
    // for the channels the neighbour already contracted) -- one scalar multiply and one min per chunk, as before.
    int x_last_off = 0;
    const __amdgpu_buffer_rsrc_t srd_x =
        __builtin_amdgcn_make_buffer_rsrc((void *)(x + (int64_t)n0 * g.C * HW), 0, nimg_here * g.C * HW * 4, 0x00020000);
    const float *ubase = up + (int64_t)kb * g.nch * W1_U + ph * 1024 + lane * 4;     // this wave's four float4 of a chunk: q = 4 ph .. + 3

    // raw[c][row][slot][2] offsets of this lane (channels 2 lh + j)
    const int raw_own = (2 * lh) * 3 * W1_ROW + (li + 1) * 2;
    const int hside = lane >= 12 ? 1 : 0, hrem = lane - 12 * hside;
    const int halo_w = ((hrem & 3) * 3 + (hrem >> 2)) * W1_ROW + (hside ? (W1_T + 1) * 2 : 1);
    if (lane < 24) {                                          // zero slots of the 2 x 12 rows (never written)
        smem[lane * W1_ROW] = 0.0f;
        smem[lane * W1_ROW + (W1_T + 1) * 2 + 1] = 0.0f;
    }

    struct Rows {
        i32x2 r[2][3];
        float halo;
    };
    auto G_row1 = [&](int ch, Rows &q, int k) {             // k = 0..5: row k % 3 of channel 2 lh + k / 3;  k = 6: the halo values
        const int soff = min(ch * (WG_CK * HW * 4), x_last_off);      // (see x_last_off)
        if (k < 6)
            q.r[k / 3][k % 3] = __builtin_amdgcn_raw_buffer_load_b64(srd_x, roff[k % 3], soff + (k / 3) * HW * 4, 0);
        else
            q.halo = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_x, hoff, soff, 0));
    };
    auto W_row1 = [&](int stage, const Rows &q, int k) {
        float *raw = smem + stage * W2_RAW;
        if (k < 6)
            *reinterpret_cast<i32x2 *>(raw + raw_own + k * W1_ROW) = q.r[k / 3][k % 3];
        else if (lane < 24)
            raw[halo_w] = q.halo;
    };
    auto G_u1 = [&](int ch, f32x4 (&u)[4], int q) { u[q] = *reinterpret_cast<const f32x4 *>(ubase + (int64_t)ch * W1_U + q * 256); };
    // half patch of (tile li, channel 2 lh + j): rows ph .. ph + 2 -> the 8 values of transform rows 2 ph, 2 ph + 1 in d[0..7]
    auto T_read1 = [&](int stage, int j, float (&d)[12], int i) {
        const float *raw = smem + stage * W2_RAW + ((2 * lh + j) * 3 + i) * W1_ROW;
        const f32x2 own = *reinterpret_cast<const f32x2 *>(raw + (li + 1) * 2);
        d[i * 4 + 0] = raw[lo], d[i * 4 + 1] = own[0], d[i * 4 + 2] = own[1], d[i * 4 + 3] = raw[ro];
    };
    // B^T d: ph = 0 holds patch rows 0, 1, 2 -> rows 0, 1 = d0 - d2, d1 + d2;  ph = 1 holds 1, 2, 3 -> rows 2, 3 = d2 - d1, d1 - d3
    auto T_col = [&](float (&d)[12], int j0) {
#pragma unroll
        for (int j = j0; j < j0 + 2; ++j) {
            const float e0 = d[0 * 4 + j], e1 = d[1 * 4 + j], e2 = d[2 * 4 + j];
            d[0 * 4 + j] = ph ? e1 - e0 : e0 - e2;
            d[1 * 4 + j] = ph ? e0 - e2 : e1 + e2;
            asm volatile("" : "+v"(d[0 * 4 + j]), "+v"(d[1 * 4 + j]));
        }
    };
    auto T_rowp = [&](float (&d)[12], int i) {
        const float t0_ = d[i * 4 + 0], t1 = d[i * 4 + 1], t2 = d[i * 4 + 2], t3 = d[i * 4 + 3];
        d[i * 4 + 0] = t0_ - t2, d[i * 4 + 1] = t1 + t2, d[i * 4 + 2] = t2 - t1, d[i * 4 + 3] = t1 - t3;
        asm volatile("" : "+v"(d[i * 4 + 0]), "+v"(d[i * 4 + 1]), "+v"(d[i * 4 + 2]), "+v"(d[i * 4 + 3]));
    };

    WACC_ZERO_LOW8();

    int nch = g.nch;
    if (BNE && bn.live != nullptr) {                          // inference: skip what apply_mask killed (wave-uniform decisions)
        const int alive = (kb * 32 + li < g.M) ? bn.live[kb * 32 + li] : 0;
        const bool dead = __ballot(alive != 0) == 0ull;
        int lastc = g.nch;
        while (lastc > 0 && bn.live[bn.Mp + 4 + lastc - 1] == 0) --lastc;
        nch = dead ? 0 : lastc;
        if (lane == 0 && ph == 0) {
            if (dead) atomicAdd(&bn.live[bn.Mp + 1], 1);
            if (blockIdx.x == 0) bn.live[bn.Mp] = lastc * WG_CK;
        }
    }
    const int last = nch - 1;
    x_last_off = __builtin_amdgcn_readfirstlane(min(last * WG_CK, g.C - WG_CK) * HW * 4);
    auto clampc = [&](int c) { return min(c, last); };
    f32x4 ua[4], ub[4];                    // U of the current / next chunk
    float c0[12], c1[12], x0[12], x1[12];  // B operands ([0..7]) of the current chunk for channels 2 lh, 2 lh + 1 / the next chunk's, being transformed
    Rows rows;
    if (nch > 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) G_row1(0, rows, k);
#pragma unroll
        for (int q = 0; q < 4; ++q) G_u1(0, ua, q);
#pragma unroll
        for (int k = 0; k < 7; ++k) W_row1(0, rows, k);
#pragma unroll
        for (int k = 0; k < 7; ++k) G_row1(clampc(1), rows, k);
#pragma unroll
        for (int i = 0; i < 3; ++i) { T_read1(0, 0, c0, i); T_read1(0, 1, c1, i); }
        T_col(c0, 0); T_col(c0, 2); T_col(c1, 0); T_col(c1, 2);
        T_rowp(c0, 0); T_rowp(c0, 1); T_rowp(c1, 0); T_rowp(c1, 1);
#pragma unroll
        for (int k = 0; k < 7; ++k) W_row1(1, rows, k);
#pragma unroll
        for (int k = 0; k < 7; ++k) G_row1(clampc(2), rows, k);
    }
#define W2_SLOT(p, h, U, B, work)                                                      \
    WACC_MMA_##p((U)[(p) >> 1][((p) & 1) * 2 + (h)], (B)[p]);                            \
    work;                                                                              \
    WACC_FENCE()
    // iteration it (par = it & 1): M(it); T(it + 1) from raw stage (it + 1) & 1; U(it + 1) requested; W(it + 2) stores the rows
    // requested one iteration ago, whose registers then take the loads of chunk it + 3
    auto iter = [&](int it, int par, f32x4 (&ucur)[4], f32x4 (&unext)[4], float (&b0)[12], float (&b1)[12], float (&n0v)[12], float (&n1v)[12]) {
        const int cu = clampc(it + 1), cr = it + 3;
        W2_SLOT(0, 0, ucur, b0, T_read1(par ^ 1, 0, n0v, 0); T_read1(par ^ 1, 0, n0v, 1));
        W2_SLOT(0, 1, ucur, b1, T_read1(par ^ 1, 0, n0v, 2); T_read1(par ^ 1, 1, n1v, 0));
        W2_SLOT(1, 0, ucur, b0, T_read1(par ^ 1, 1, n1v, 1); T_read1(par ^ 1, 1, n1v, 2));
        W2_SLOT(1, 1, ucur, b1, G_u1(cu, unext, 0));
        W2_SLOT(2, 0, ucur, b0, T_col(n0v, 0); G_u1(cu, unext, 1));
        W2_SLOT(2, 1, ucur, b1, T_col(n0v, 2); G_u1(cu, unext, 2));
        W2_SLOT(3, 0, ucur, b0, T_col(n1v, 0); G_u1(cu, unext, 3));
        W2_SLOT(3, 1, ucur, b1, T_col(n1v, 2));
        W2_SLOT(4, 0, ucur, b0, T_rowp(n0v, 0));
        W2_SLOT(4, 1, ucur, b1, T_rowp(n0v, 1));
        W2_SLOT(5, 0, ucur, b0, T_rowp(n1v, 0));
        W2_SLOT(5, 1, ucur, b1, T_rowp(n1v, 1));
        W2_SLOT(6, 0, ucur, b0, W_row1(par, rows, 0); W_row1(par, rows, 1); G_row1(cr, rows, 0));
        W2_SLOT(6, 1, ucur, b1, W_row1(par, rows, 2); W_row1(par, rows, 3); G_row1(cr, rows, 1); G_row1(cr, rows, 2));
        W2_SLOT(7, 0, ucur, b0, W_row1(par, rows, 4); W_row1(par, rows, 5); G_row1(cr, rows, 3); G_row1(cr, rows, 4));
        W2_SLOT(7, 1, ucur, b1, W_row1(par, rows, 6); G_row1(cr, rows, 5); G_row1(cr, rows, 6));
    };
    for (int it = 0; it < nch; it += 2) {
        iter(it, 0, ua, ub, c0, c1, x0, x1);
        if (it + 1 < nch) iter(it + 1, 1, ub, ua, x0, x1, c0, c1);
    }

    // ---- epilogue: this wave's 8 positions (transform rows i = 2 ph, 2 ph + 1) -> partial 2x2 outputs; the output transform is linear
    WACC_DRAIN();
    float own0[16], own1[16];                  // the output row this wave finishes (a = ph), columns 0 / 1, per accumulator element
    __syncthreads();                           // both waves are done with their raw stages: the LDS becomes the exchange buffer
    float *xch = smem_all;
    auto part_e = [&](int e, const float (&m)[8]) {
        const float r00 = m[0] + m[1] + m[2], r01 = m[1] - m[2] - m[3];       // R[il][b] = sum_j A^T[b][j] M[i][j]
        const float r10 = m[4] + m[5] + m[6], r11 = m[5] - m[6] - m[7];
        float g0, g1;
        if (ph == 0) {                         // i = 0, 1:  Y0 += R0 + R1 (own),  Y1 += R1 (given to the other wave)
            own0[e] = r00 + r10, own1[e] = r01 + r11, g0 = r10, g1 = r11;
        } else {                               // i = 2, 3:  Y1 += -R2 - R3 (own),  Y0 += R2 (given)
            own0[e] = -r00 - r10, own1[e] = -r01 - r11, g0 = r00, g1 = r01;
        }
        xch[((ph * 2 + 0) * 16 + e) * 64 + lane] = g0;
        xch[((ph * 2 + 1) * 16 + e) * 64 + lane] = g1;
    };
    {
        float m[8];
#define W2_PART(e) WACC_RD8_0_##e(m); part_e(e, m);
        WACC_EACH16(W2_PART)
#undef W2_PART

    }
    __syncthreads();
    const unsigned tg = t0 + li;
    const bool tv = tg < ttot;
    const int n = (int)(tg / timg), r = (int)(tg % timg);
    const int ty = (int)((unsigned)r / twu), tx = (int)((unsigned)r % twu);
    float *yout = y + ((int64_t)n * g.M) * HW + (2 * ty + ph) * g.W + 2 * tx;
    float s1[16], s2[16];
    auto out_all = [&](auto hb) {                // (hb: with / without a conv bias -- two separate epilogues, see k_wg1)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int co = kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        float v0 = own0[e] + xch[(((ph ^ 1) * 2 + 0) * 16 + e) * 64 + lane];
        float v1 = own1[e] + xch[(((ph ^ 1) * 2 + 1) * 16 + e) * 64 + lane];
        if constexpr (decltype(hb)::value) {
            const float bv = bias[co < g.M ? co : 0];
            v0 += bv, v1 += bv;
        }
        if constexpr (PRE) {                   // y = prelu(conv + bias) [+ residual]
            const float a = bn.slope()[bn.per_channel() && co < g.M ? co : 0];
            v0 = prelu_one(v0, a), v1 = prelu_one(v1, a);
            if (bn.residual() != nullptr && tv && co < g.M) {
                const f32x2 rr = *reinterpret_cast<const f32x2 *>(bn.residual() + (yout - y) + (int64_t)co * HW);
                v0 = prelu_sum(v0, rr[0]), v1 = prelu_sum(v1, rr[1]);
            }
        } else if (BNE) {                      // y = [max(0,] (conv + bias - mean) * invstd * gamma + beta [)]
            const int cc = co < g.M ? co : 0;
            const float mu = bn.mean[cc], is = 1.0f / sqrtf(bn.var[cc] + bn.eps), ga = bn.gamma[cc], be = bn.beta[cc];
            v0 = (v0 - mu) * is * ga + be, v1 = (v1 - mu) * is * ga + be;
            if (bn.relu) v0 = relu_keep(v0), v1 = relu_keep(v1);
        }
        if constexpr (POOL) {                  // this wave's row maximum, into the slot v0's partial came from (see POOL)
            xch[(((ph ^ 1) * 2 + 0) * 16 + e) * 64 + lane] = max_keep(v0, v1);
        } else
        if (tv && co < g.M) {
            f32x2 o;
            o[0] = v0, o[1] = v1;
            *reinterpret_cast<f32x2 *>(yout + (int64_t)co * HW) = o;
        }
        if (STATS) {
            s1[e] = tv ? v0 + v1 : 0.0f;
            s2[e] = tv ? v0 * v0 + v1 * v1 : 0.0f;
        }
    }
    };
    if (bias != nullptr) out_all(std::true_type{}); else out_all(std::false_type{});
    if constexpr (POOL) {
        __syncthreads();                       // both waves' row maxima are in the exchange buffer
        float *pout = y + ((int64_t)n * g.M) * g.tiles_img + r;       // window (ty, tx) of image n, channel 0
#pragma unroll
        for (int e8 = 0; e8 < 8; ++e8) {
            const int e = ph * 8 + e8;
            const int co = kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            const float a = xch[((0 * 2 + 0) * 16 + e) * 64 + lane], b = xch[((1 * 2 + 0) * 16 + e) * 64 + lane];      // left by wave 1 / by wave 0
            if (tv && co < g.M) pout[(int64_t)co * g.tiles_img] = max_keep(a, b);
        }
    }
    if (STATS) {                               // every wave is its own statistics tile: stats[k][2 run + ph][2]
#pragma unroll
        for (int e = 0; e < 16; e += 8) half_wave_sum8(s1 + e), half_wave_sum8(s2 + e);
        if (li == kHalfSumLane) {
            const unsigned ntile = 2 * ((ttot + W1_T - 1) / W1_T);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (co < g.M) {
                    float *dst = stats + ((int64_t)co * ntile + 2 * run + ph) * 2;
                    f32x2 o;
                    o[0] = s1[e], o[1] = s2[e];
                    *reinterpret_cast<f32x2 *>(dst) = o;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------ two waves = one unit of 64 channels ("k_wg3")
// k_wg2 with 64 output channels per wave: the transformed input (whose adds and LDS round trip are paid in MFMA time, see k_wg2) feeds
// twice the MFMAs.  Wave ph owns the positions of transform rows 2 ph, 2 ph + 1 for the channel halves kq = 0, 1: 16 accumulators =
// 256 AGPRs, one wave per SIMD, two 2-wave blocks per CU.  Per chunk: 32 MFMAs against 32 (not 64) transform adds, 7 (not 9) row
// loads and 8 float4 of U.

// ODD: maps with an odd height and / or width (7 x 7: ResNet-50 layer4, SphereNet conv4_x) as ceil(H/2) x ceil(W/2) tiles -- the last tile
// row / column hangs over the edge by one pixel.  Rows past the map are range-checked to zero as ever; a tile in the last column of an
// odd-width map fetches the pair (W-2, W-1) instead of (W-1, W) -- nothing past the tensor is touched -- and stores (x[W-1], 0); its
// outputs past the edge are not stored (one dword instead of the pair; the odd row of the last tile row not at all) and stay out of
// the BatchNorm statistics.
struct Bop {                                  // k_wg3's B operands of one channel: patch rows as register pairs (see T_read1)
    f32x2 P[3], Q[3];
};
// SH (round 4; even maps, training launches, a multiple of 128 output channels): a block is FOUR waves = TWO units on the SAME tile run
// (output-channel blocks 2 j, 2 j + 1).  The B operands of a chunk -- the transformed patch of the lane's tile for channels 2 lh, 2 lh + 1 --
// are the same for both units, so the waves (unit 0, ph) and (unit 1, ph) split them: unit u fetches, stages and transforms channel
// 2 lh + u only (3 + 1 instead of 6 + 1 row loads and LDS stores, 9 instead of 18 raw reads, 8 instead of 16 packed transform
// instructions per chunk), leaves its eight operand values in a shared double-buffered LDS array (two 16-byte stores) and both read
// all sixteen back after a barrier that waits for LDS traffic only (four 16-byte reads).  Everything else -- filter operands,
// accumulators, the epilogue and its exchange between the two waves of a unit -- is per unit, as before; every sum is bit for bit
// what the two-wave block computes.
// SPLIT (round 5): the TAIL launch of a layer whose units do not fill their last round (SphereNet-20's 256 -> 256 @14 at batch 256: 784
// four-wave blocks on 256 CUs = 3.06 rounds -- the last 16 blocks ran alone for a whole round).  wg3_run() launches the full rounds as
// before and the leftover logical blocks here, each cut into split_s pieces along the channel loop (piece s contracts chunks
// s * split_nch .. and stores its partial outputs -- the output transform is linear -- to its own slice of a workspace); k_wg_tail_reduce
// adds the slices in a fixed order (+ bias) into y.  No statistics / inference epilogue, even maps.
// ADD (round 5; input-gradient launches): y = result + addend, elementwise -- the gradient of the OTHER consumer of the conv's input (SphereNet's
// residual units, models/spherenet.py:121-131: `x = x + relu(conv(relu(conv(x))))`: x feeds the first conv and the sum), which autograd would
// otherwise add in a separate 3-pass kernel.  The addend comes in through the `bias` parameter (an input-gradient launch has no bias) and is
// shaped like y.
// PMAX (forward launches with the statistics epilogue, even maps, no bias, M a multiple of 64): the maximum of every 2x2 output tile --
// the window of the MaxPool2d(2, 2) behind the BatchNorm that follows -- also goes out, as E[n][co][H/2][W/2], one dword per (channel,
// tile).  A wave ends the epilogue with output row ph of the tile: it leaves max(v0, v1) in the exchange slot it has just read (that slot is
// the other wave's, already consumed, and nobody else looks at it), and after one more barrier wave ph combines the two row maxima of channel
// half kq = ph and stores them: 32 consecutive tiles = 128 bytes per channel and half-wave.  No further LDS, no value kept in a register
// across the stores.  E comes in through the `bias` parameter (such a launch has no bias), as the addend does under ADD.
// PRE (inference launches, with BNE: the same skip): y = prelu(conv + bias) [+ residual] instead of the BatchNorm expression (see WgBnEval).
// The residual is fetched as ADD fetches its addend -- on the fast path four channels' worth with the group's exchange reads, at y's own
// offsets -- but from bn.residual(): the bias slot holds the conv's bias here.
// POOL (inference launches, with BNE: the same skip; even maps, any channel count): PMAX's exchange behind the BatchNorm (+ ReLU), with NO y store
// at all -- `y` is the POOLED tensor [N][M][H/2][W/2], which wave ph writes for channel half kq = ph after the extra barrier.  One path for
// whole and ragged units: the unit's scalar base + a 32-bit lane offset + the running scalar channel offset, every store guarded by
// tile < tiles_total and co < M.
template <bool DGRAD, bool STATS, bool BNE = false, bool ODD = false, bool SH = false, bool SPLIT = false, bool ADD = false, bool PMAX = false,
          bool PRE = false, bool POOL = false>
__global__ __launch_bounds__(SH ? 256 : 128) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_wg3(WgGeom g, const float *__restrict__ x, const float *__restrict__ up, const float *__restrict__ bias,
           float *__restrict__ y, float *__restrict__ stats, WgBnEval bn) {
    static_assert(!PRE || (BNE && !DGRAD && !STATS), "the PReLU epilogue is an inference epilogue");
    static_assert(!SH || (!BNE && !ODD), "shared B operands: training launches on even maps");
    static_assert(!SPLIT || (!STATS && !BNE && !ODD), "the tail launch has the plain epilogue only");
    static_assert(!ADD || (DGRAD && !STATS && !BNE && !SPLIT), "the addend rides in plain input-gradient launches");
    static_assert(!PMAX || (STATS && !DGRAD && !BNE && !ODD && !SPLIT && !ADD), "the window maxima go out with the statistics of an even map");
    static_assert(!POOL || (BNE && !PRE && !DGRAD && !STATS && !ODD && !SH && !SPLIT && !ADD && !PMAX), "the pooled epilogue is the BatchNorm inference epilogue's, on even maps");
    constexpr int UNITF = 2 * 64 * 64;                       // per unit: 2 x 2 raw stages (3264 floats) / the epilogue's exchange buffer (32 KB)
    constexpr int BXF = 2 * 2 * 2 * 2 * 64 * 4;              // SH: [buffer][ph][channel j][half][lane][4] transformed operands (16 KB)
    __shared__ __attribute__((aligned(16))) float smem_all[SH ? 2 * UNITF + BXF : UNITF];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int un = SH ? wv >> 1 : 0, ph = SH ? wv & 1 : wv;   // unit of the block, wave of the unit
    const int li = lane & 31, lh = lane >> 5;
    const int HW = g.H * g.W;
    float *unit_smem = smem_all + un * UNITF;
    float *smem = unit_smem + ph * 2 * W2_RAW;                // this wave's private raw stages
    float *bx = smem_all + 2 * UNITF;                         // (SH only)

    // persistent blocks, as in k_wg1 (two blocks of two waves per CU are resident)
    const unsigned nlb = SH ? g.nblocks >> 1 : g.nblocks;     // SH: pairs of logical blocks (the host only sends an even number of channel blocks)
    for (unsigned base = 0; base < nlb; base += gridDim.x) {
    // (virtual block v runs on XCD v % 8 = blockIdx % 8 -- the grid is a multiple of 8 blocks whenever there is more than one
    //  round -- and XCD x owns the x-th eighth of ALL logical blocks, walking through it round after round: consecutive tile runs,
    //  which share half of their input rows, stay in one XCD's L2 as with one block per logical block)
    const unsigned v = base + blockIdx.x;
    if (v >= nlb) break;
    // SPLIT: virtual block v = (leftover block or pair v / split_s, piece v % split_s); g.nblocks counts the pieces
    const int piece = SPLIT ? (int)(v % (unsigned)g.split_s) : 0;
    const unsigned lb = SPLIT ? g.split_first + (SH ? 2 * (v / (unsigned)g.split_s) + (unsigned)un : v / (unsigned)g.split_s)
                              : (SH ? 2 * xcd_remap(v, nlb) + (unsigned)un : xcd_remap(v, nlb));
    const int ch0 = SPLIT ? piece * g.split_nch : 0;          // first channel chunk of this unit's contraction
    float *const yy = SPLIT ? y + (int64_t)piece * g.split_stride : y;
    const int nkb64 = (g.nkb + 1) / 2;                        // (g.nkb counts blocks of 32 channels)
    const int kb = lb % nkb64;                                // block of 64 output channels
    const unsigned ttot = (unsigned)g.tiles_total, timg = (unsigned)g.tiles_img, twu = (unsigned)g.tw;
    const unsigned run = lb / nkb64;                          // tile run of 32
    const unsigned t0 = run * W1_T;
    if (t0 >= ttot) continue;                                 // (uniform for the block)
#ifdef WG_TIMING
    const unsigned dbg_u = lb * 2 + ph;
    WG_STAMP(0);
    if (lane == 0 && dbg_u < 65536) wg_dbg[dbg_u * 8 + 6] = __builtin_amdgcn_s_getreg(63492), wg_dbg[dbg_u * 8 + 7] = __builtin_amdgcn_s_getreg(63508);
#endif
    const unsigned n0u = t0 / timg, r0 = t0 - n0u * timg;      // (uniform: the one generic division of a unit)
    const int n0 = (int)n0u;
    // tile t0 + add (add < 64) -> image relative to n0, tile row, tile column: r0 + add < tiles_img + 64 < 2^24 (cpg_conv3x3_wino_ok)
    auto locate = [&](unsigned add, int &nrel, int &ty, int &tx) {
        unsigned dn, r, tyu, txu;
        wg_divmod(r0 + add, timg, g.inv_timg, dn, r);
        wg_divmod(r, twu, g.inv_tw, tyu, txu);
        nrel = (int)dn, ty = (int)tyu, tx = (int)txu;
    };

    constexpr int kOutOfRange = (int)0x80000000;
    int roff[3], hoff, lo, ro;
    bool oddcol = false;                                     // ODD: this lane's tile hangs over the right edge of an odd-width map
    {
        const unsigned tg = t0 + li;
        const bool tv = tg < ttot;
        int nrel, ty, tx;
        locate((unsigned)li, nrel, ty, tx);
        const int n = n0 + nrel;
        const int cbase = ((n - n0) * g.C + 2 * lh) * HW;
        if (ODD) oddcol = (g.W & 1) && tx == g.tw - 1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int gh = 2 * ty - 1 + ph + (ph ? 2 - i : i);          // wave 1 holds its rows 3, 2, 1 (see T_col)
            roff[i] = (tv && (unsigned)gh < (unsigned)g.H) ? (cbase + gh * g.W + 2 * tx - (oddcol ? 1 : 0)) * 4 : kOutOfRange;
        }
        lo = tx == 0 ? 0 : (li + 1) * 2 - 1;
        ro = tx == g.tw - 1 ? (W1_T + 1) * 2 + 1 : (li + 1) * 2 + 2;
        // halo: lanes 0-23 = (side, row, channel): the column left of tile t0 / right of tile t0 + 31
        const int side = lane >= 12 ? 1 : 0, hl = lane - 12 * side, hi = hl >> 2, hc = hl & 3;
        const unsigned th = side ? t0 + W1_T - 1 : t0;
        int nhrel, tyh, txh;
        locate(side ? W1_T - 1 : 0, nhrel, tyh, txh);
        const int nh = n0 + nhrel;
        const int ghh = 2 * tyh - 1 + ph + (ph ? 2 - hi : hi), gwh = side ? 2 * txh + 2 : 2 * txh - 1;
        const bool okh = lane < 24 && th < ttot && (unsigned)ghh < (unsigned)g.H && (unsigned)gwh < (unsigned)g.W;
        hoff = okh ? (((nh - n0) * g.C + hc) * HW + ghh * g.W + gwh) * 4 : kOutOfRange;
    }
    const int span = (W1_T + g.tiles_img - 1) / g.tiles_img + 1;
    const int nimg_here = min(span, g.N - n0);
    // byte offset of the LAST chunk's first channel, set once the chunk count is known: min(last chunk * 4, C - 4) channels.  Every row load
    // takes min(chunk * stride, x_last_off): chunks past the end re-read the last one (what clampc did for them), and with a channel count
    // that is no multiple of 4 the last chunk starts at C - 4, overlapping its neighbour (wg_chunk_base; the pack kernel zeroes its filters
    // for the channels the neighbour already contracted) -- one scalar multiply and one min per chunk, as before.
    int x_last_off = 0;
    const __amdgpu_buffer_rsrc_t srd_x =
        __builtin_amdgcn_make_buffer_rsrc((void *)(x + ((int64_t)n0 * g.C + ch0 * WG_CK) * HW), 0, (nimg_here * g.C - ch0 * WG_CK) * HW * 4, 0x00020000);
    // U records are per block of 32 channels: this wave reads float4 q = 4 ph .. + 3 of the records of blocks 2 kb, 2 kb + 1
    // (through a buffer descriptor: four per-lane byte offsets computed once per unit, the chunk in the scalar offset, the float4 pair
    //  in the instruction offset -- no vector instruction per load; 64-bit pointer arithmetic was four per chunk)
    const __amdgpu_buffer_rsrc_t srd_u = __builtin_amdgcn_make_buffer_rsrc((void *)up, 0, (int)(((int64_t)g.nkb + 1) / 2 * 2 * g.nch * W1_U * 4), 0x00020000);
    const int ubase = (((2 * kb) * g.nch + ch0) * W1_U + ph * 1024 + lane * 4) * 4;
    const int ukq = g.nch * W1_U * 4;

    // raw[c][row][slot][2] offsets of this lane (channels 2 lh + j)
    const int raw_own = (2 * lh) * 3 * W1_ROW + (li + 1) * 2;
    const int hside = lane >= 12 ? 1 : 0, hrem = lane - 12 * hside;
    const int halo_w = ((hrem & 3) * 3 + (hrem >> 2)) * W1_ROW + (hside ? (W1_T + 1) * 2 : 1);
    if (lane < 24) {                                          // zero slots of the 2 x 12 rows (never written)
        smem[lane * W1_ROW] = 0.0f;
        smem[lane * W1_ROW + (W1_T + 1) * 2 + 1] = 0.0f;
    }

    struct Rows {
        i32x2 r[2][3];
        float halo;
    };
    auto G_row1 = [&](int ch, Rows &q, int k) {             // k = 0..5: row k % 3 of channel 2 lh + k / 3;  k = 6: the halo values
        const int soff = min(ch * (WG_CK * HW * 4), x_last_off);      // (see x_last_off)
        if (k < 6)
            q.r[k / 3][k % 3] = __builtin_amdgcn_raw_buffer_load_b64(srd_x, roff[k % 3], soff + (k / 3) * HW * 4, 0);
        else
            q.halo = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_x, hoff, soff, 0));
    };
    auto W_row1 = [&](int stage, const Rows &q, int k) {
        float *raw = smem + stage * W2_RAW;
        if (k < 6) {
            i32x2 v = q.r[k / 3][k % 3];
            if (ODD) {                                       // the pair fetched was (W-2, W-1): keep x[W-1], the column past the edge is 0
                v[0] = oddcol ? v[1] : v[0];
                v[1] = oddcol ? 0 : v[1];
            }
            *reinterpret_cast<i32x2 *>(raw + raw_own + k * W1_ROW) = v;
        } else if (lane < 24)
            raw[halo_w] = q.halo;
    };
    // SH: this wave stages channel 2 lh + un only (k = 0..2: its three patch rows; k = 3: the halo values, all four channels as before)
    const int un_goff = un * HW * 4;
    const int raw_own_s = raw_own + un * 3 * W1_ROW, tr_base = ((2 * lh + un) * 3) * W1_ROW;
    auto G_rows = [&](int ch, Rows &q, int k) {
        const int soff = min(ch * (WG_CK * HW * 4), x_last_off);      // (see x_last_off)
        if (k < 3)
            q.r[0][k] = __builtin_amdgcn_raw_buffer_load_b64(srd_x, roff[k], soff + un_goff, 0);
        else
            q.halo = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_x, hoff, soff, 0));
    };
    auto W_rows = [&](int stage, const Rows &q, int k) {
        float *raw = smem + stage * W2_RAW;
        if (k < 3)
            *reinterpret_cast<i32x2 *>(raw + raw_own_s + k * W1_ROW) = q.r[0][k];
        else if (lane < 24)
            raw[halo_w] = q.halo;
    };
    // Wave ph = 1 keeps its two transform rows in REVERSE order (local row 0 = row 3, local row 1 = row 2) AND its three patch rows
    // in reverse order (e0, e1, e2 = patch rows 3, 2, 1; wave 0: 0, 1, 2): then local row 0 of B^T d is e0 - e2 for both waves
    // (= row 0 = d0 - d2 for wave 0, = -(row 3) = d3 - d1 for wave 1) and local row 1 is e1 + sgn e2 (row 1 = d1 + d2, row 2 =
    // d2 - d1) -- ONE fused multiply-add with the wave's sign where a select between two operands was two instructions: 2 instead
    // of 3 vector instructions per column.  The negated row 3 is put right where the two waves' rows meet in the epilogue (own =
    // r1 + sgn r0 instead of r0 + r1): every value is bit for bit what it was.  The row a wave GIVES the other is local row 1 for both.
    const float sgn = ph ? -1.0f : 1.0f;
    f32x2 sgn2;
    sgn2[0] = sgn, sgn2[1] = sgn;
    const int urow = ph * 512 * 4;                            // float4 q ^ 2 of the wave's four: + 512 floats for q = 0, 1, - 512 for q = 2, 3
    const int uoff[4] = {ubase + urow, ubase - urow + 512 * 4, ubase + ukq + urow, ubase + ukq - urow + 512 * 4};   // [(q >> 2) * 2 + ((q >> 1) & 1)]
    auto G_u1 = [&](int ch, f32x4 (&u)[8], int q) {
        u[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_u, uoff[(q >> 2) * 2 + ((q >> 1) & 1)] + (q & 1) * 256 * 4, ch * (W1_U * 4), 0));
    };
    // half patch of (tile li, channel 2 lh + j): the wave's three patch rows as register PAIRS, P[i] = columns (1, 2) -- the lane's own
    // pixel pair, one 8-byte LDS read -- and Q[i] = columns (0, 3).  The transforms below are packed fp32 instructions (two results per
    // vector instruction: v_pk_add_f32 / v_pk_fma_f32 with op_sel / neg picking the halves and signs), 16 per chunk where the scalar
    // form was 30 -- on this chip every vector instruction of the wave is MFMA time (profiles/r03_pmc_step_vgg16.md).
    // After T_col and T_rowp rows 0, 1 hold the B operands: position il * 4 + j -> j = 0: Q[il][0], 1: P[il][0], 2: P[il][1], 3: Q[il][1].
    auto T_read1 = [&](int stage, int j, Bop &d, int i) {
        const float *raw = smem + stage * W2_RAW + ((2 * lh + j) * 3 + i) * W1_ROW;
        d.P[i] = *reinterpret_cast<const f32x2 *>(raw + (li + 1) * 2);
        d.Q[i][0] = raw[lo], d.Q[i][1] = raw[ro];
    };
    auto T_reads = [&](int stage, Bop &d, int i) {            // SH: patch row i of this wave's channel 2 lh + un
        const float *raw = smem + stage * W2_RAW + tr_base + i * W1_ROW;
        d.P[i] = *reinterpret_cast<const f32x2 *>(raw + (li + 1) * 2);
        d.Q[i][0] = raw[lo], d.Q[i][1] = raw[ro];
    };
    // SH: the transformed operands of channel 2 lh + un (local rows 0, 1: P and Q pairs) go to bx[buffer][ph][un]; both waves with this ph
    // then read channel j's from bx[buffer][ph][j]
    auto X_put = [&](int buf, const Bop &d) {
        float *dst = bx + ((((buf * 2 + ph) * 2 + un) * 2) * 64 + lane) * 4;
        f32x4 a, b;
        a[0] = d.P[0][0], a[1] = d.P[0][1], a[2] = d.Q[0][0], a[3] = d.Q[0][1];
        b[0] = d.P[1][0], b[1] = d.P[1][1], b[2] = d.Q[1][0], b[3] = d.Q[1][1];
        *reinterpret_cast<f32x4 *>(dst) = a;
        *reinterpret_cast<f32x4 *>(dst + 256) = b;
    };
    auto X_get = [&](int buf, int j, Bop &d, int half) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(bx + ((((buf * 2 + ph) * 2 + j) * 2 + half) * 64 + lane) * 4);
        d.P[half][0] = v[0], d.P[half][1] = v[1], d.Q[half][0] = v[2], d.Q[half][1] = v[3];
    };
    // B^T d on a pair type (half = 0: the P pairs, 1: the Q pairs): local rows (0, 1) = e0 - e2, e1 + sgn e2
    auto T_col = [&](Bop &d, int half) {
        f32x2 &e0 = half ? d.Q[0] : d.P[0], &e1 = half ? d.Q[1] : d.P[1], &e2 = half ? d.Q[2] : d.P[2];
        f32x2 r0, r1;
        asm volatile("v_pk_add_f32 %0, %2, %3 neg_lo:[0,1] neg_hi:[0,1]\n\tv_pk_fma_f32 %1, %4, %3, %5"
                     : "=&v"(r0), "=&v"(r1) : "v"(e0), "v"(e2), "v"(sgn2), "v"(e1));
        e0 = r0, e1 = r1;
    };
    // (B^T d) B on local row i: P = (t1, t2), Q = (t0, t3) -> Q = (t0 - t2, t1 - t3), P = (t1 + t2, t2 - t1)
    auto T_rowp = [&](Bop &d, int i) {
        f32x2 nq, np;
        asm volatile("v_pk_add_f32 %0, %2, %3 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[1,0]\n\t"
                     "v_pk_add_f32 %1, %3, %3 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[0,1]"
                     : "=&v"(nq), "=&v"(np) : "v"(d.Q[i]), "v"(d.P[i]));
        d.Q[i] = nq, d.P[i] = np;
    };


    WG_STAMP(1);
    int nch = SPLIT ? min(g.split_nch, g.nch - ch0) : g.nch;
    if (BNE && bn.live != nullptr) {                          // inference: skip what apply_mask killed (wave-uniform decisions)
        const int alive = (kb * 64 + lane < g.M) ? bn.live[kb * 64 + lane] : 0;
        const bool dead = __ballot(alive != 0) == 0ull;
        int lastc = g.nch;
        while (lastc > 0 && bn.live[bn.Mp + 4 + lastc - 1] == 0) --lastc;
        nch = dead ? 0 : lastc;
        if (lane == 0 && ph == 0) {
            if (dead) atomicAdd(&bn.live[bn.Mp + 1], 1);
            if (blockIdx.x == 0) bn.live[bn.Mp] = lastc * WG_CK;
        }
    }
    const int last = nch - 1;
    x_last_off = __builtin_amdgcn_readfirstlane(min(last * WG_CK, g.C - WG_CK - ch0 * WG_CK) * HW * 4);
    auto clampc = [&](int c) { return min(c, last); };
    // U of the current / next chunk: [kq * 4 + q].  U3 (every variant but the one with the statistics epilogue, which has no registers
    // left): a third buffer -- the loads of chunk it + 2 go out during chunk it, two chunks (2 us) ahead of their first use instead of
    // one; the wait counters showed the waves stalled on vector-memory data 13 % of the time with one chunk of distance
    constexpr bool U3 = true;
    f32x4 ua[8], ub[8], uc[U3 ? 8 : 1];
    Bop c0, c1, x0, x1;                    // B operands of the current chunk for channels 2 lh, 2 lh + 1 / the next chunk's, being transformed
    Bop mine;                              // SH: the half this wave transforms
    Rows rows;
    if (nch > 0) {
        if constexpr (SH) {
#pragma unroll
            for (int k = 0; k < 4; ++k) G_rows(0, rows, k);
        } else {
#pragma unroll
            for (int k = 0; k < 7; ++k) G_row1(0, rows, k);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) G_u1(0, ua, q);
        if constexpr (U3) {
#pragma unroll
            for (int q = 0; q < 8; ++q) G_u1(min(1, nch - 1), ub, q);
        }
    }
    // the accumulators are cleared while those loads fly (256 instructions, 0.4 us)
    __builtin_amdgcn_sched_barrier(0);
    WACC_ZERO_ALL();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SH) {
        if (nch > 0) {                        // (nch is the same for the two units of a block: the barriers pair up)
#pragma unroll
            for (int k = 0; k < 4; ++k) W_rows(0, rows, k);
#pragma unroll
            for (int k = 0; k < 4; ++k) G_rows(clampc(1), rows, k);
#pragma unroll
            for (int i = 0; i < 3; ++i) T_reads(0, mine, i);
            T_col(mine, 0); T_col(mine, 1);
            T_rowp(mine, 0); T_rowp(mine, 1);
            X_put(0, mine);
            WACC_LDS_BARRIER();
            X_get(0, 0, c0, 0); X_get(0, 0, c0, 1); X_get(0, 1, c1, 0); X_get(0, 1, c1, 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) W_rows(1, rows, k);
#pragma unroll
            for (int k = 0; k < 4; ++k) G_rows(clampc(2), rows, k);
        }
    } else if (nch > 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) W_row1(0, rows, k);
#pragma unroll
        for (int k = 0; k < 7; ++k) G_row1(clampc(1), rows, k);
#pragma unroll
        for (int i = 0; i < 3; ++i) { T_read1(0, 0, c0, i); T_read1(0, 1, c1, i); }
        T_col(c0, 0); T_col(c0, 1); T_col(c1, 0); T_col(c1, 1);
        T_rowp(c0, 0); T_rowp(c0, 1); T_rowp(c1, 0); T_rowp(c1, 1);
#pragma unroll
        for (int k = 0; k < 7; ++k) W_row1(1, rows, k);
#pragma unroll
        for (int k = 0; k < 7; ++k) G_row1(clampc(2), rows, k);
    }
// accumulator a = kq * 8 + pp (channel half kq, local position pp = il * 4 + j: see T_read1 for where the operand sits)
#define W3_B(B, pp) (((pp) & 3) == 0 ? (B).Q[(pp) >> 2][0] : ((pp) & 3) == 1 ? (B).P[(pp) >> 2][0] : ((pp) & 3) == 2 ? (B).P[(pp) >> 2][1] : (B).Q[(pp) >> 2][1])
#define W3_SLOT(a, h, U, B, work)                                                                  \
    WACC_MMA_##a((U)[((a) >> 3) * 4 + (((a) & 7) >> 1)][((a) & 1) * 2 + (h)], W3_B(B, (a) & 7));     \
    work;                                                                                          \
    WACC_FENCE()
    // iteration it (par = it & 1): M(it); T(it + 1) from raw stage (it + 1) & 1; U(it + 1) requested; W(it + 2) stores the rows
    // requested one iteration ago, whose registers then take the loads of chunk it + 3
    auto iter = [&](int it, int par, f32x4 (&ucur)[8], f32x4 (&unext)[8], Bop &b0, Bop &b1, Bop &n0v, Bop &n1v) {
        const int cu = clampc(it + (U3 ? 2 : 1)), cr = it + 3;
        if constexpr (SH) {
            // the next chunk's operands: this wave's channel, the barrier, both channels read back; then the rows of chunk it + 2 / it + 3
            W3_SLOT(0, 0, ucur, b0, G_u1(cu, unext, 0));
            W3_SLOT(0, 1, ucur, b1, G_u1(cu, unext, 1));
            W3_SLOT(8, 0, ucur, b0, G_u1(cu, unext, 2));
            W3_SLOT(8, 1, ucur, b1, G_u1(cu, unext, 3));
            W3_SLOT(1, 0, ucur, b0, G_u1(cu, unext, 4));
            W3_SLOT(1, 1, ucur, b1, G_u1(cu, unext, 5));
            W3_SLOT(9, 0, ucur, b0, G_u1(cu, unext, 6));
            W3_SLOT(9, 1, ucur, b1, G_u1(cu, unext, 7));
            W3_SLOT(2, 0, ucur, b0, T_reads(par ^ 1, mine, 0));
            W3_SLOT(2, 1, ucur, b1, T_reads(par ^ 1, mine, 1));
            W3_SLOT(10, 0, ucur, b0, T_reads(par ^ 1, mine, 2));
            W3_SLOT(10, 1, ucur, b1, T_col(mine, 0));
            W3_SLOT(3, 0, ucur, b0, T_col(mine, 1));
            W3_SLOT(3, 1, ucur, b1, T_rowp(mine, 0));
            W3_SLOT(11, 0, ucur, b0, T_rowp(mine, 1));
            W3_SLOT(11, 1, ucur, b1, X_put(par ^ 1, mine));
            // (the barrier sits ten slots behind the stores it waits for: its s_waitcnt then finds them done -- right behind them the wave
            //  stood at the wait for an LDS latency per chunk while the MFMA pipe drained -- and the two units may drift by that much)
            W3_SLOT(4, 0, ucur, b0, W_rows(par, rows, 0); G_rows(cr, rows, 0));
            W3_SLOT(4, 1, ucur, b1, W_rows(par, rows, 1); G_rows(cr, rows, 1));
            W3_SLOT(12, 0, ucur, b0, W_rows(par, rows, 2); G_rows(cr, rows, 2));
            W3_SLOT(12, 1, ucur, b1, W_rows(par, rows, 3); G_rows(cr, rows, 3));
            W3_SLOT(5, 0, ucur, b0, );
            W3_SLOT(5, 1, ucur, b1, );
            W3_SLOT(13, 0, ucur, b0, );
            W3_SLOT(13, 1, ucur, b1, );
            W3_SLOT(6, 0, ucur, b0, );
            W3_SLOT(6, 1, ucur, b1, WACC_LDS_BARRIER());
            W3_SLOT(14, 0, ucur, b0, X_get(par ^ 1, 0, n0v, 0));
            W3_SLOT(14, 1, ucur, b1, X_get(par ^ 1, 0, n0v, 1));
            W3_SLOT(7, 0, ucur, b0, X_get(par ^ 1, 1, n1v, 0));
            W3_SLOT(7, 1, ucur, b1, X_get(par ^ 1, 1, n1v, 1));
            W3_SLOT(15, 0, ucur, b0, );
            W3_SLOT(15, 1, ucur, b1, );
            return;
        }
        W3_SLOT(0, 0, ucur, b0, G_u1(cu, unext, 0));
        W3_SLOT(0, 1, ucur, b1, G_u1(cu, unext, 1));
        W3_SLOT(8, 0, ucur, b0, G_u1(cu, unext, 2));
        W3_SLOT(8, 1, ucur, b1, G_u1(cu, unext, 3));
        W3_SLOT(1, 0, ucur, b0, G_u1(cu, unext, 4));
        W3_SLOT(1, 1, ucur, b1, G_u1(cu, unext, 5));
        W3_SLOT(9, 0, ucur, b0, G_u1(cu, unext, 6));
        W3_SLOT(9, 1, ucur, b1, G_u1(cu, unext, 7));
        W3_SLOT(2, 0, ucur, b0, T_read1(par ^ 1, 0, n0v, 0));
        W3_SLOT(2, 1, ucur, b1, T_read1(par ^ 1, 0, n0v, 1));
        W3_SLOT(10, 0, ucur, b0, T_read1(par ^ 1, 0, n0v, 2));
        W3_SLOT(10, 1, ucur, b1, T_read1(par ^ 1, 1, n1v, 0));
        W3_SLOT(3, 0, ucur, b0, T_read1(par ^ 1, 1, n1v, 1));
        W3_SLOT(3, 1, ucur, b1, T_read1(par ^ 1, 1, n1v, 2));
        W3_SLOT(11, 0, ucur, b0, T_col(n0v, 0));
        W3_SLOT(11, 1, ucur, b1, T_col(n0v, 1));
        W3_SLOT(4, 0, ucur, b0, T_col(n1v, 0));
        W3_SLOT(4, 1, ucur, b1, T_col(n1v, 1));
        W3_SLOT(12, 0, ucur, b0, T_rowp(n0v, 0));
        W3_SLOT(12, 1, ucur, b1, T_rowp(n0v, 1));
        W3_SLOT(5, 0, ucur, b0, T_rowp(n1v, 0));
        W3_SLOT(5, 1, ucur, b1, T_rowp(n1v, 1));
        W3_SLOT(13, 0, ucur, b0, W_row1(par, rows, 0); G_row1(cr, rows, 0));
        W3_SLOT(13, 1, ucur, b1, W_row1(par, rows, 1); G_row1(cr, rows, 1));
        W3_SLOT(6, 0, ucur, b0, W_row1(par, rows, 2); G_row1(cr, rows, 2));
        W3_SLOT(6, 1, ucur, b1, W_row1(par, rows, 3); G_row1(cr, rows, 3));
        W3_SLOT(14, 0, ucur, b0, W_row1(par, rows, 4); G_row1(cr, rows, 4));
        W3_SLOT(14, 1, ucur, b1, W_row1(par, rows, 5); G_row1(cr, rows, 5));
        W3_SLOT(7, 0, ucur, b0, W_row1(par, rows, 6); G_row1(cr, rows, 6));
        W3_SLOT(7, 1, ucur, b1, );
        W3_SLOT(15, 0, ucur, b0, );
        W3_SLOT(15, 1, ucur, b1, );
    };
    WG_STAMP(2);
    if constexpr (U3) {                       // (U buffers rotate with period 3, the operand sets with period 2: six iterations per trip)
        for (int it = 0; it < nch; it += 6) {
            iter(it, 0, ua, uc, c0, c1, x0, x1);
            if (it + 1 < nch) iter(it + 1, 1, ub, ua, x0, x1, c0, c1);
            if (it + 2 < nch) iter(it + 2, 0, uc, ub, c0, c1, x0, x1);
            if (it + 3 < nch) iter(it + 3, 1, ua, uc, x0, x1, c0, c1);
            if (it + 4 < nch) iter(it + 4, 0, ub, ua, c0, c1, x0, x1);
            if (it + 5 < nch) iter(it + 5, 1, uc, ub, x0, x1, c0, c1);
        }
    } else {
        for (int it = 0; it < nch; it += 2) {
            iter(it, 0, ua, ub, c0, c1, x0, x1);
            if (it + 1 < nch) iter(it + 1, 1, ub, ua, x0, x1, c0, c1);
        }
    }

    WG_STAMP(3);
    // ---- epilogue: this wave's 8 positions (transform rows i = 2 ph, 2 ph + 1) -> partial 2x2 outputs; the output transform is linear
    WACC_DRAIN();
    float own0[32], own1[32];                  // the output row this wave finishes (a = ph), columns 0 / 1, per channel half and accumulator element
    // (the epilogue's lane constants are derived from an opaque copy: computed from `lh` itself they are invariant in the persistent loop,
    //  the compiler hoists all 32 channel offsets in front of it and spills them)
    int lh_e = lh;
    asm volatile("" : "+v"(lh_e));
    __syncthreads();                           // both waves are done with their raw stages: the LDS becomes the exchange buffer
    float *xch = unit_smem;
    // local rows: wave 0 holds R0, R1, wave 1 holds -R3, R2 (reversed; row 3 negated, see T_col).  Y0 = R0 + R1 + R2, Y1 = R1 - R2 - R3: a wave owns
    // +-(its two rows) and gives its local row 1 (R1 to Y1, R2 to Y0) to the other wave; the sign is applied when the two meet.
    auto part_e = [&](int kq, int e, const float (&m)[8]) {
        const float r00 = m[0] + m[1] + m[2], r01 = m[1] - m[2] - m[3];       // R[il][b] = sum_j A^T[b][j] M[i][j]
        const float r10 = m[4] + m[5] + m[6], r11 = m[5] - m[6] - m[7];
        own0[kq * 16 + e] = fmaf(sgn, r00, r10), own1[kq * 16 + e] = fmaf(sgn, r01, r11);   // wave 1's local row 0 is -R3 (T_col): R2 + R3
        f32x2 gv;                              // (one 8-byte LDS store / load per channel: xch[wave][kq][e][lane][2])
        gv[0] = r10, gv[1] = r11;
        *reinterpret_cast<f32x2 *>(xch + (((ph * 2 + kq) * 16 + e) * 64 + lane) * 2) = gv;
    };
    {
        float m[8];
#define W3_PART_0(e) WACC_RD8_0_##e(m); part_e(0, e, m);
#define W3_PART_1(e) WACC_RD8_1_##e(m); part_e(1, e, m);
        WACC_EACH16(W3_PART_0)
        WACC_EACH16(W3_PART_1)
#undef W3_PART_0
#undef W3_PART_1

    }
    __syncthreads();
    const unsigned tg = t0 + li;
    int nrel, ty, tx;
    locate((unsigned)li, nrel, ty, tx);
    const int n = n0 + nrel;
    // (ODD: the odd row of the last tile row of an odd-height map does not exist -- the wave that owns it stores nothing for that tile)
    const bool tv = tg < ttot && (!ODD || 2 * ty + ph < g.H);
    float *yout = yy + ((int64_t)n * g.M) * HW + (2 * ty + ph) * g.W + 2 * tx;
    // FAST (all 32 tiles of the unit exist, all 64 channels of the block exist, even map -- a wave-uniform test): plain stores at the unit's
    // (scalar) base + a 32-bit lane offset + the running scalar channel offset, one vector add per store.  The general path computes a
    // 64-bit address per store (a multiply-add and two shift-adds), compares and branches around it: 1 us of a unit for the few units
    // on the ragged end of a launch that need it.
    const bool fast_u = !ODD && t0 + W1_T <= ttot && g.M - kb * 64 >= 64;
    char *ybase = reinterpret_cast<char *>(yy + (int64_t)n0 * g.M * HW);
    // (ADD) the addend at the same offsets as y: `bias` IS the addend tensor
    const char *abase = reinterpret_cast<const char *>(bias + (ADD ? (int64_t)n0 * g.M * HW : 0));
    const float *aout = bias + (ADD ? ((int64_t)n * g.M) * HW + (2 * ty + ph) * g.W + 2 * tx : 0);
    // (PRE) the residual at the same offsets as y; null: none (a wave-uniform test)
    const bool has_res = PRE && bn.residual() != nullptr;
    const char *rbase = reinterpret_cast<const char *>(bn.residual() + (has_res ? (int64_t)n0 * g.M * HW : 0));
    const float *rout = bn.residual() + (has_res ? ((int64_t)n * g.M) * HW + (2 * ty + ph) * g.W + 2 * tx : 0);
    const unsigned yoff = (unsigned)(((nrel * g.M + kb * 64 + 4 * lh_e) * HW + (2 * ty + ph) * g.W + 2 * tx) * 4);
    // (the scalar channel offsets are a running sum behind an opaque barrier: as multiples of HW they are invariant in the persistent
    //  loop, the compiler would compute all 32 in front of it and spill scalar registers into vector lanes)
    int HW4 = HW * 4;
    asm volatile("" : "+s"(HW4));
    // (the statistics go out per 32-channel half: with all 32 + 32 sums live next to own0 / own1 the kernel is past 256 vector registers and the
    //  allocator parks values in scratch and in an accumulation register -- tests/test_abi_and_host.py checks the compiled code for both)
    auto out_half = [&](auto hb, auto kqc, auto fastc) {     // (hb: with / without a conv bias -- two separate epilogues, see k_wg1)
    constexpr int kq = decltype(kqc)::value;
    constexpr bool FAST = decltype(fastc)::value;
    float s1[16], s2[16];
    constexpr int GR = STATS ? 2 : 4;          // (the statistics variant has no registers for four)
    f32x2 got4[GR];
    f32x2 ad4[((ADD || PRE) && FAST) ? GR : 1];         // (ADD / PRE, fast path) the addend of the group's GR channels, requested with the exchange reads
    int soff = kq * 32 * HW4;                  // (kq * 32 + (e & 3) + 8 * (e >> 2)) * HW4, stepped
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int ke = kq * 16 + e;
        const int co = kb * 64 + kq * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh_e;
        if ((e & (GR - 1)) == 0) {             // (the exchange reads of GR channels go out together: one LDS latency per GR stores)
#pragma unroll
            for (int j = 0; j < GR; ++j)
                got4[j] = *reinterpret_cast<const f32x2 *>(xch + ((((ph ^ 1) * 2 + kq) * 16 + e + j) * 64 + lane) * 2);
            if constexpr (ADD && FAST && decltype(hb)::value) {
                static_assert(!ADD || GR == 4, "a group is the four channels between two 5 HW jumps of the running offset");
#pragma unroll
                for (int j = 0; j < GR; ++j)
                    ad4[j] = *reinterpret_cast<const f32x2 *>(abase + (size_t)(yoff + (unsigned)(soff + j * HW4)));
            }
            if constexpr (PRE && FAST) {
                static_assert(!PRE || GR == 4, "a group is the four channels between two 5 HW jumps of the running offset");
                if (has_res) {
#pragma unroll
                    for (int j = 0; j < GR; ++j)
                        ad4[j] = *reinterpret_cast<const f32x2 *>(rbase + (size_t)(yoff + (unsigned)(soff + j * HW4)));
                }
            }
        }
        const f32x2 got = got4[e & (GR - 1)];
        float v0 = fmaf(own0[ke], sgn, got[0]);             // (+- own + got, exactly)
        float v1 = fmaf(own1[ke], sgn, got[1]);
        if constexpr (decltype(hb)::value) {
            if constexpr (ADD) {
                if constexpr (FAST) {
                    v0 += ad4[e & (GR - 1)][0], v1 += ad4[e & (GR - 1)][1];
                } else if (tv && co < g.M) {
                    if (ODD && oddcol) {
                        v0 += aout[(int64_t)co * HW];
                    } else {
                        const f32x2 ad = *reinterpret_cast<const f32x2 *>(aout + (int64_t)co * HW);
                        v0 += ad[0], v1 += ad[1];
                    }
                }
            } else {
                const float bv = bias[co < g.M ? co : 0];
                v0 += bv, v1 += bv;
            }
        }
        if constexpr (PRE) {                   // y = prelu(conv + bias) [+ residual]
            const float a = bn.slope()[bn.per_channel() && co < g.M ? co : 0];
            v0 = prelu_one(v0, a), v1 = prelu_one(v1, a);
            if (has_res) {
                if constexpr (FAST) {
                    v0 = prelu_sum(v0, ad4[e & (GR - 1)][0]), v1 = prelu_sum(v1, ad4[e & (GR - 1)][1]);
                } else if (tv && co < g.M) {
                    if (ODD && oddcol) {
                        v0 = prelu_sum(v0, rout[(int64_t)co * HW]);
                    } else {
                        const f32x2 rr = *reinterpret_cast<const f32x2 *>(rout + (int64_t)co * HW);
                        v0 = prelu_sum(v0, rr[0]), v1 = prelu_sum(v1, rr[1]);
                    }
                }
            }
        } else if (BNE) {                      // y = [max(0,] (conv + bias - mean) * invstd * gamma + beta [)]
            const int cc = co < g.M ? co : 0;
            const float mu = bn.mean[cc], is = 1.0f / sqrtf(bn.var[cc] + bn.eps), ga = bn.gamma[cc], be = bn.beta[cc];
            v0 = (v0 - mu) * is * ga + be, v1 = (v1 - mu) * is * ga + be;
            if (bn.relu) v0 = relu_keep(v0), v1 = relu_keep(v1);
        }
        if constexpr (PMAX || POOL)            // this wave's row maximum, into the slot `got` came from (see PMAX)
            xch[((((ph ^ 1) * 2 + kq) * 16 + e) * 64 + lane) * 2] = max_keep(v0, v1);
        if constexpr (POOL) {                  // (no y store; the fence keeps the exchange reads in their groups, as on the fast path)
            if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        } else
        if constexpr (FAST) {
            f32x2 o;
            o[0] = v0, o[1] = v1;
            *reinterpret_cast<f32x2 *>(ybase + (size_t)(yoff + (unsigned)soff)) = o;
            soff += (e & 3) == 3 ? 5 * HW4 : HW4;
            asm volatile("" : "+s"(soff));
            if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (with no branch between them the scheduler hoists every exchange read: spills)
            if (STATS) s1[e] = v0 + v1, s2[e] = v0 * v0 + v1 * v1;
        } else {
            if (ODD && oddcol) {               // the second column is past the edge: one dword, and it stays out of the statistics
                if (tv && co < g.M) yout[(int64_t)co * HW] = v0;
                v1 = 0.0f;
            } else if (tv && co < g.M) {
                f32x2 o;
                o[0] = v0, o[1] = v1;
                *reinterpret_cast<f32x2 *>(yout + (int64_t)co * HW) = o;
            }
            if (STATS) {
                s1[e] = tv ? v0 + v1 : 0.0f;
                s2[e] = tv ? v0 * v0 + v1 * v1 : 0.0f;
            }
        }
    }
    if (STATS) {                               // every wave is its own statistics tile: stats[k][2 run + ph][2]
#pragma unroll
        for (int e = 0; e < 16; e += 8) half_wave_sum8(s1 + e), half_wave_sum8(s2 + e);
        if (li == kHalfSumLane) {
            const unsigned ntile = 2 * ((ttot + W1_T - 1) / W1_T);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = kb * 64 + kq * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh_e;
                if (co < g.M) {
                    float *dst = stats + ((int64_t)co * ntile + 2 * run + ph) * 2;
                    f32x2 o;
                    o[0] = s1[e], o[1] = s2[e];
                    *reinterpret_cast<f32x2 *>(dst) = o;
                }
            }
        }
    }
    };
    auto out_all = [&](auto hb) {
        if constexpr (!ODD) {
            if (fast_u) {
                out_half(hb, std::integral_constant<int, 0>{}, std::true_type{}), out_half(hb, std::integral_constant<int, 1>{}, std::true_type{});
                return;
            }
        }
        out_half(hb, std::integral_constant<int, 0>{}, std::false_type{}), out_half(hb, std::integral_constant<int, 1>{}, std::false_type{});
    };
    if constexpr (PMAX) {
        out_all(std::false_type{});            // (`bias` is E)
        __syncthreads();                       // both waves' row maxima are in the exchange buffer
        // wave ph: channel half kq = ph.  The tile index inside the image IS the window index: E[n][co][ty][tx]
        float *ebase = const_cast<float *>(bias) + (int64_t)n0 * g.M * g.tiles_img;
        const unsigned eoff = (unsigned)((nrel * g.M + kb * 64 + ph * 32 + 4 * lh_e) * g.tiles_img + ty * g.tw + tx);
        int timg1 = g.tiles_img;               // (a running scalar channel offset behind an opaque barrier, as HW4 above)
        asm volatile("" : "+s"(timg1));
        int esoff = 0;
        const float *rowmax = xch + (ph * 16 * 64 + lane) * 2;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float a = rowmax[e * 64 * 2], b = rowmax[(2 * 16 + e) * 64 * 2];      // left by wave 1 / by wave 0
            if (tg < ttot) ebase[eoff + (unsigned)esoff] = max_keep(a, b);
            esoff += (e & 3) == 3 ? 5 * timg1 : timg1;
            asm volatile("" : "+s"(esoff));
        }
    } else if constexpr (POOL) {
        auto rows = [&](auto hb) {             // (the general out_half: it differs from the fast one in the y stores only, and there are none)
            out_half(hb, std::integral_constant<int, 0>{}, std::false_type{}), out_half(hb, std::integral_constant<int, 1>{}, std::false_type{});
        };
        if (bias != nullptr) rows(std::true_type{}); else rows(std::false_type{});
        __syncthreads();                       // both waves' row maxima are in the exchange buffer
        // wave ph: channel half kq = ph.  The tile index inside the image IS the window index: y[n][co][ty][tx]
        float *ebase = yy + (int64_t)n0 * g.M * g.tiles_img;
        const unsigned eoff = (unsigned)((nrel * g.M + kb * 64 + ph * 32 + 4 * lh_e) * g.tiles_img + ty * g.tw + tx);
        const int co0 = kb * 64 + ph * 32 + 4 * lh_e;
        int timg1 = g.tiles_img;               // (a running scalar channel offset behind an opaque barrier, as HW4 above)
        asm volatile("" : "+s"(timg1));
        int esoff = 0;
        const float *rowmax = xch + (ph * 16 * 64 + lane) * 2;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float a = rowmax[e * 64 * 2], b = rowmax[(2 * 16 + e) * 64 * 2];      // left by wave 1 / by wave 0
            if (tg < ttot && co0 + (e & 3) + 8 * (e >> 2) < g.M) ebase[eoff + (unsigned)esoff] = max_keep(a, b);
            esoff += (e & 3) == 3 ? 5 * timg1 : timg1;
            asm volatile("" : "+s"(esoff));
        }
    } else {
        if (bias != nullptr) out_all(std::true_type{}); else out_all(std::false_type{});
    }
    WG_STAMP(4);
    __syncthreads();                           // the exchange buffer becomes the next unit's raw stages
    }   // next logical block
}

// y = bias + sum over the pieces of k_wg3<.., SPLIT>'s partial outputs, for the logical blocks lb_first .. lb_end - 1 of the layer (each: 64 output
// channels x 32 tiles x 2 x 2 pixels).  The pieces are added in index order: the result does not depend on which piece finished first.
// `part` is piece 0's slice, addressed like y (image n at (n * M + m) * H W); piece s lies s * stride floats further.
// PMAX (see k_wg3): the tail's share of the window maxima; E comes in through the `addend` parameter (a forward launch has no addend).
template <bool STATS, bool PMAX = false>
__global__ __launch_bounds__(256) void k_wg_tail_reduce(WgGeom g, const float *__restrict__ part, const float *__restrict__ bias,
                                                        float *__restrict__ y, unsigned lb_first, unsigned lb_end, float *__restrict__ stats,
                                                        const float *__restrict__ addend) {
    // one half-wave = the 32 tiles of one (unit, channel): total is a multiple of 32, so a half-wave is never split by the loop bound
    const int64_t total = (int64_t)(lb_end - lb_first) * 64 * W1_T;
    const int nkb64 = (g.nkb + 1) / 2, HW = g.H * g.W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(i & (W1_T - 1)), kl = (int)((i >> 5) & 63);
        const unsigned lb = lb_first + (unsigned)(i >> 11);
        const int m = (int)(lb % (unsigned)nkb64) * 64 + kl;
        const unsigned run = lb / (unsigned)nkb64;
        const int64_t tile = (int64_t)run * W1_T + t;
        const bool ok = m < g.M && tile < g.tiles_total;
        f32x2 a0, a1;
        a0[0] = a0[1] = a1[0] = a1[1] = 0.0f;
        int64_t off = 0;
        if (ok) {
            const int n = (int)(tile / g.tiles_img), r = (int)(tile % g.tiles_img);
            const int ty = r / g.tw, tx = r % g.tw;
            off = ((int64_t)n * g.M + m) * HW + (int64_t)(2 * ty) * g.W + 2 * tx;
            const float b = bias != nullptr ? bias[m] : 0.0f;
            a0[0] = a0[1] = a1[0] = a1[1] = b;
            for (int sidx = 0; sidx < g.split_s; ++sidx) {
                const float *p = part + (int64_t)sidx * g.split_stride + off;
                const f32x2 v0 = *reinterpret_cast<const f32x2 *>(p), v1 = *reinterpret_cast<const f32x2 *>(p + g.W);
                a0[0] += v0[0], a0[1] += v0[1], a1[0] += v1[0], a1[1] += v1[1];
            }
            if constexpr (PMAX) {
                const_cast<float *>(addend)[((int64_t)n * g.M + m) * g.tiles_img + r] = max_keep(max_keep(a0[0], a0[1]), max_keep(a1[0], a1[1]));
            } else if (addend != nullptr) {                          // (the fused skip gradient of an input-gradient launch: k_wg3<.., ADD>)
                const f32x2 d0 = *reinterpret_cast<const f32x2 *>(addend + off), d1 = *reinterpret_cast<const f32x2 *>(addend + off + g.W);
                a0[0] += d0[0], a0[1] += d0[1], a1[0] += d1[0], a1[1] += d1[1];
            }
            *reinterpret_cast<f32x2 *>(y + off) = a0;
            *reinterpret_cast<f32x2 *>(y + off + g.W) = a1;
        }
        if constexpr (STATS) {
            // the BatchNorm partial sums of the unit, in k_wg3's layout: statistics tile 2 run + ph holds output row ph of the unit's 32 tiles
            // (a wave of the main kernel is its own tile).  Sum over the half-wave's 32 lanes (xor shuffles below 32 stay inside it); a
            // lane without a tile / channel contributes zeros.
            float s[4] = {a0[0] + a0[1], a0[0] * a0[0] + a0[1] * a0[1], a1[0] + a1[1], a1[0] * a1[0] + a1[1] * a1[1]};
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1)
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], d, 64);
            if (t == 0 && m < g.M) {
                const unsigned ntile = 2 * (unsigned)((g.tiles_total + W1_T - 1) / W1_T);
                float *dst = stats + ((int64_t)m * ntile + 2 * run) * 2;
                dst[0] = s[0], dst[1] = s[1], dst[2] = s[2], dst[3] = s[3];
            }
        }
    }
}

inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// The tail of a k_wg3 launch (see k_wg3<.., SPLIT>): `units` blocks (SH: four-wave blocks of two units, one resident per CU; otherwise
// two-wave blocks, two per CU) = some full rounds + `left` blocks that would run a whole round alone.  When they are at most half a round,
// each is cut into S <= 16 pieces along the channel loop (>= 2 chunks per piece) so that the pieces fill (at most) one round of 1 / S length.
struct WgTail {
    bool on;
    unsigned first_lb, end_lb;    // logical blocks of the tail
    int64_t left;
    int S, nch_per, n_first;
    int64_t stride;               // floats per piece: images n_first .. N - 1 of the output
    size_t off, bytes;            // the pieces in the workspace: behind the packed filter (pack_bytes of it), 256-byte aligned
    WgGeom g;                     // the pieces' launch: the layer's geometry with the split filled in, nblocks = the pieces
};
static WgTail wino_tail_plan(const WgGeom &g0, int64_t nblocks, bool sh, size_t pack_bytes) {
    WgTail t{};
    if (opt_or(OPT_WINO_TAIL, 1) == 0) return t;
    const int64_t units = sh ? nblocks / 2 : nblocks, slots = sh ? kCUs : 2 * kCUs;
    const int64_t full = units / slots * slots, left = units - full;
    if (full == 0 || left == 0 || left * 2 > slots) return t;
    int S = (int)std::min<int64_t>(slots / left, 16);
    S = std::min(S, g0.nch / 2);
    if (S < 2) return t;
    const int per = (g0.nch + S - 1) / S;
    S = (g0.nch + per - 1) / per;
    if (S < 2) return t;
    t.first_lb = (unsigned)(sh ? 2 * full : full), t.end_lb = (unsigned)nblocks;
    t.left = left, t.S = S, t.nch_per = per;
    const int nkb64 = (g0.nkb + 1) / 2;
    t.n_first = (int)(((int64_t)(t.first_lb / (unsigned)nkb64) * W1_T) / g0.tiles_img);
    t.stride = (int64_t)(g0.N - t.n_first) * g0.M * g0.H * g0.W;
    t.off = (pack_bytes + 255) / 256 * 256, t.bytes = (size_t)S * t.stride * sizeof(float);
    t.on = t.bytes <= ((size_t)64 << 20) && t.stride > 0;
    t.g = g0;
    t.g.split_first = t.first_lb, t.g.split_s = S, t.g.split_nch = per, t.g.split_stride = t.stride;
    t.g.nblocks = (unsigned)((sh ? 2 : 1) * left * S);
    return t;
}

// the cooperative block kernel (CPG_WINO_KERNEL=block only): NW waves per block, `blocks` of them -- one per (tile run, channel block)
template <int NW>
void wino_launch(bool dgrad, const WgGeom &g, unsigned blocks, const float *x, const float *up, const float *bias, float *y, float *stats,
                 hipStream_t stream) {
    if (dgrad)
        hipLaunchKernelGGL((k_wg_fwd<NW, true, false>), dim3(blocks), dim3(64 * NW), 0, stream, g, x, up, bias, y, nullptr);
    else if (stats != nullptr)
        hipLaunchKernelGGL((k_wg_fwd<NW, false, true>), dim3(blocks), dim3(64 * NW), 0, stream, g, x, up, bias, y, stats);
    else
        hipLaunchKernelGGL((k_wg_fwd<NW, false, false>), dim3(blocks), dim3(64 * NW), 0, stream, g, x, up, bias, y, nullptr);
}

// ---- host side: the plan ---------------------------------------------------------------------------------------------
// Which Winograd forward / input-gradient kernel a launch uses.  Default: k_wg3 (two waves per unit, 64 output channels each) when the
// layer reads and produces at least 64 channels, else k_wg1 (one wave per unit).  (Until round 4 the launches WITH the BatchNorm-statistics
// epilogue switched at 128 channels read: k_wg3's statistics epilogue was the heavier one.  After round 3's work on it -- sums per
// 32-channel half, scalar-base stores, the third filter buffer -- the interleaved A/B (tools/conv_bench.py --only fwdstats --ab
// CPG_WINO_KERNEL=-,64) reads 64 -> 64 @224 4.716 -> 4.546 ms and 64 -> 128 @112 2.277 -> 2.217 ms for k_wg3.)
// CPG_WINO_KERNEL = wave | pair | 64 | block forces k_wg1 / k_wg2 / k_wg3 / the cooperative block kernel (A/B experiments, tests).
enum { WV_BLOCK = 0, WV_WAVE = 1, WV_PAIR = 2, WV_PAIR64 = 3 };
int wino_variant(int c_read, int m) {
    if (const int forced = opt(OPT_WINO_KERNEL); forced != OPT_UNSET)      // (block | wave | pair | 64 -> WV_*)
        return forced >= WV_BLOCK && forced <= WV_PAIR64 ? forced : WV_WAVE;
    if (c_read < 64 || m < 64) return WV_WAVE;
    // Channel counts that are no multiple of 64 (the grown networks: 78 / 156 / 313 / 627 outputs): a unit of k_wg3 produces 64 channels, one
    // of k_wg1 32, and the padding of the last block is MFMA time.  At equal padding k_wg3 is the faster kernel by 5-8 % (shared transform),
    // so the one-wave kernel takes the layer when its blocks waste at least 10 % less: m = 78 (96 vs 128 computed) 9.88 -> 7.73 ms,
    // m = 156 (160 vs 192) 6.37 -> 5.81 ms; m = 313 / 627 (both 320 / 640) stay on k_wg3: 5.21 vs 5.49 ms  (conv_bench --width-multiplier 1.5).
    const int p64 = (m + 63) / 64 * 64, p32 = (m + 31) / 32 * 32;
    return p64 * 10 > p32 * 11 ? WV_WAVE : WV_PAIR64;
}

// eligibility of one launch (c_read channels contracted, m produced): the staging offsets of the images a block can touch fit 31 bits.
// Odd maps (7 x 7: ResNet-50 layer4, SphereNet conv4_x): only the two-wave kernel k_wg3 has the edge handling (its ODD instances), and it
// only pays with a long channel loop -- >= 128 channels read, >= 64 produced, no forced kernel choice
bool wino_eligible(int N, int c_read, int m, int H, int W) {
    if (opt_on(OPT_NO_WINO)) return false;
    if (c_read < 16 || m < 16 || N < 1) return false;           // (any channel count: wg_chunk_base)
    if (((H | W) & 1) && !(H >= 3 && W >= 3 && c_read >= 128 && m >= 64 && opt(OPT_WINO_KERNEL) == OPT_UNSET && !opt_on(OPT_NO_WINO_ODD)))
        return false;
    const int tiles_img = ((H + 1) / 2) * ((W + 1) / 2);
    const int span = (WG_T + tiles_img - 1) / tiles_img + 1;    // (the widest unit's, whichever kernel runs)
    if ((int64_t)N * tiles_img + 64 >= (1ll << 31)) return false;               // 32-bit tile indices in the kernels
    return (int64_t)span * std::max(c_read, m) * H * W * 4 < (1ll << 31);   // (a unit's images behind one buffer descriptor: read and written)
}

// What differs between launches of one shape: the direction (the pack job), an inference launch (neither shared transforms nor a tail),
// and whether the tail may be planned at all (false: the single launch of a caller whose workspace ends behind the packed filter).
struct WinoWant {
    bool dgrad, eval, tail;
};
constexpr WinoWant kWinoTrain{false, false, true};      // what the shape queries ask: direction-free answers of a training launch

// Everything a launch or a query needs, from the shape and the option table alone: no pointer, no workspace, no thread state.
struct WinoPlan {
    bool ok;                  // the shape is eligible; the rest describes the launch an eligible shape gets
    bool odd;                 // an odd map: k_wg3's ODD instances
    int variant, nw;          // WV_*; waves per block of the block kernel (4, or 8: 64 channels per block -- it does half the staging work per
                              // MFMA, but its eight waves run in lock step behind one barrier and it measured 3-4 % SLOWER than two independent
                              // 4-wave blocks per CU on every VGG16 layer (docs/LAB_NOTEBOOK.md section 4.9): CPG_WINO_NW=8 only)
    WgGeom g;                 // nblocks: the logical blocks of the main launch (the whole launch's, less the tail's)
    int64_t blocks;           // logical blocks of the whole launch
    bool grid_ok;             // ... fit a grid; false: "grid too large", nothing below is filled in
    unsigned grid, threads;   // the main launch, after the persistent clamp
    bool sh;                  // k_wg3<.., SH>: two units per four-wave block share the input transform
    WgTail tail;              // k_wg3<.., SPLIT> + k_wg_tail_reduce behind the main launch (on: planned)
    size_t pack_bytes;        // the transformed filter at the head of the workspace
    PackJob job;              // ... as k_wg1_pack writes it (the block kernel packs another layout for itself)
    int tiles;                // BatchNorm-statistics tiles per channel of a forward launch
    // what the launch can carry: the inference epilogues, the pooled one, the window maxima, an addend, a caller-packed operand
    bool eval, eval_pool, pool_max, addend, takes_packed;
};

// CPG_WINO_PERSIST=0: one block per logical block instead of the persistent grid (A/B experiments).
// How many resident grids' worth of persistent blocks a launch gets: 8.  One grid (every block resident from the start, ~200 units
// per wave on the big layers) and 4, 8 or 16 grids measured the same within 0.5 % on every VGG16 layer -- a block that runs a
// dozen units has amortised its dispatch --, but with one exactly-resident grid a launch that finds some CUs taken (RCCL's
// kernels on the communication stream) would run its last blocks alone afterwards; with 8 the dispatcher balances whatever
// share of the chip is free to within 1/8 of a round.  CPG_WINO_GRIDS overrides (A/B experiments).
unsigned wino_persistent_grid(int64_t units, int resident) {
    if (opt_or(OPT_WINO_PERSIST, 1) == 0) return (unsigned)units;
    return (unsigned)std::min<int64_t>(units, (int64_t)std::max(1, opt_or(OPT_WINO_GRIDS, 8)) * resident);
}

WinoPlan wino_plan(WinoWant want, int N, int c_read, int m, int H, int W) {
    WinoPlan p{};
    p.ok = wino_eligible(N, c_read, m, H, W);
    p.odd = ((H | W) & 1) != 0;
    p.variant = p.odd ? WV_PAIR64 : wino_variant(c_read, m);
    p.nw = opt_or(OPT_WINO_NW, 4) == 8 ? 8 : 4;
    const bool block = p.variant == WV_BLOCK, pair64 = p.variant == WV_PAIR64;
    p.eval = p.ok && !block, p.eval_pool = p.eval && !p.odd, p.takes_packed = p.eval;
    p.addend = p.ok && pair64;           // (k_wg3<.., ADD>: >= 64 channels on both sides, or an odd map)
    p.pool_max = p.ok && pair64 && !p.odd && m % 64 == 0 && !opt_on(OPT_NO_POOL_MAX);      // (k_wg3<.., PMAX>: whole 64-channel blocks)
    // The geometry.  The block kernel differs from the one- and two-wave kernels in two numbers: its unit is a run of WG_T = 64 consecutive
    // tiles, theirs W1_T = 32 (`span`, the images a run can touch, follows), and its channel blocks are 8 * nw wide, theirs 32 (`nkb`).
    // (It runs even maps only, so th = (H + 1) / 2 is its H / 2.)
    const int run = block ? WG_T : W1_T, bk = block ? 8 * p.nw : 32;
    WgGeom &g = p.g;
    g.N = N, g.C = c_read, g.H = H, g.W = W, g.M = m;
    g.th = (H + 1) / 2, g.tw = (W + 1) / 2, g.tiles_img = g.th * g.tw;
    g.inv_timg = 1.0f / (float)g.tiles_img, g.inv_tw = 1.0f / (float)g.tw;
    g.tiles_total = (int64_t)N * g.tiles_img;
    g.nkb = pad_to(m, bk) / bk, g.nch = pad_to(c_read, WG_CK) / WG_CK;
    g.span = (run + g.tiles_img - 1) / g.tiles_img + 1;
    const int64_t runs = (g.tiles_total + run - 1) / run;
    p.tiles = (int)(block || p.variant == WV_WAVE ? runs : 2 * runs);       // (every wave of a pair is its own statistics tile)
    // the packed operand: the per-lane transformed filter U in k_wg1_pack's layout (the 64-channel blocking pads m further: covers both);
    // the layer's weight is [K][C][3][3], whichever side the launch reads
    p.pack_bytes = cpg_conv3x3_wino_pack_bytes(c_read, m);
    p.job = PackJob{2, want.dgrad ? c_read : m, want.dgrad ? m : c_read, m, c_read, g.nch, want.dgrad ? 1 : 0,
                    (long long)((m + 31) / 32) * g.nch * 32 * WG_CK, p.pack_bytes};
    // logical blocks: one per (run, channel block) -- k_wg1's four waves take four runs, k_wg3's unit two channel blocks
    p.blocks = pair64 ? runs * ((g.nkb + 1) / 2) : p.variant == WV_WAVE ? (runs + 3) / 4 * g.nkb : runs * g.nkb;
    p.grid_ok = p.blocks <= 0x7FFFFFFFll;
    if (!p.grid_ok) return p;
    g.nblocks = (unsigned)p.blocks;
    if (pair64 && !p.odd && !want.eval) {       // (inference launches: no SH instance with an epilogue, and no tail)
        p.sh = ((g.nkb + 1) / 2) % 2 == 0 && opt_or(OPT_WG3_SHARE, 1) != 0;       // training launches whose 64-channel blocks pair up
        if (want.tail) p.tail = wino_tail_plan(g, p.blocks, p.sh, p.pack_bytes);
        if (p.tail.on) g.nblocks = p.tail.first_lb;      // the full rounds run as before on logical blocks 0 .. first_lb - 1
    }
    // k_wg1 and k_wg3 are persistent: one four-wave block per CU is resident, or two two-wave blocks
    if (pair64)
        p.threads = p.sh ? 256 : 128, p.grid = wino_persistent_grid(p.sh ? g.nblocks / 2 : g.nblocks, p.sh ? kCUs : 2 * kCUs);
    else if (p.variant == WV_WAVE)
        p.threads = 256, p.grid = wino_persistent_grid(g.nblocks, kCUs);
    else
        p.threads = block ? 64 * p.nw : 128, p.grid = g.nblocks;
    return p;
}

}  // namespace

// ---- the queries: each reads the plan ------------------------------------------------------------------------------------
extern "C" int cpg_conv3x3_wino_ok(int N, int c_read, int m, int H, int W) { return wino_plan(kWinoTrain, N, c_read, m, H, W).ok ? 1 : 0; }

extern "C" size_t cpg_conv3x3_wino_pack_bytes(int c_read, int m) {
    return (size_t)pad_to(m, 64) * pad_to(c_read, WG_CK) * 16 * sizeof(float);
}

// workspace behind the packed filter for the partial outputs of a tail launch (0: this launch has none) -- part of cpg_conv2d_workspace_bytes
size_t cpg_conv3x3_wino_tail_bytes(int N, int c_read, int m, int H, int W) {
    const WinoPlan p = wino_plan(kWinoTrain, N, c_read, m, H, W);
    return p.ok && p.tail.on ? p.tail.bytes + 256 : 0;
}

// number of BatchNorm-statistics tiles per channel of a forward launch (stats[m][tiles][2])
extern "C" int cpg_conv3x3_wino_tiles(int N, int c_read, int m, int H, int W) { return wino_plan(kWinoTrain, N, c_read, m, H, W).tiles; }

// the packed operand of the launch cpg_conv3x3_wino_launch would make; false: that launch streams no operand a caller could hand in -- a
// shape that is not eligible, or the cooperative block kernel (CPG_WINO_KERNEL=block), which packs for itself
bool cpg_conv3x3_wino_pack_job(int dgrad, int N, int c_read, int m, int H, int W, cpg::PackJob *job) {
    const WinoPlan p = wino_plan(WinoWant{dgrad != 0, false, true}, N, c_read, m, H, W);
    if (p.takes_packed) *job = p.job;
    return p.takes_packed;
}

int cpg_conv3x3_wino_pool_max_ok(int N, int c_read, int m, int H, int W) { return wino_plan(kWinoTrain, N, c_read, m, H, W).pool_max ? 1 : 0; }
int cpg_conv3x3_wino_eval_ok(int N, int c_read, int m, int H, int W) { return wino_plan(kWinoTrain, N, c_read, m, H, W).eval ? 1 : 0; }
int cpg_conv3x3_wino_eval_pool_ok(int N, int c_read, int m, int H, int W) { return wino_plan(kWinoTrain, N, c_read, m, H, W).eval_pool ? 1 : 0; }
int cpg_conv3x3_wino_dgrad_add_ok(int N, int c_read, int m, int H, int W) { return wino_plan(kWinoTrain, N, c_read, m, H, W).addend ? 1 : 0; }

#ifdef WG_TIMING
extern "C" int cpg_debug_wg_timing(unsigned long long *dst, int n) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(wg_dbg), (size_t)n * 8 * sizeof(unsigned long long));
}
#endif

// ---- the launch ------------------------------------------------------------------------------------------------------
// What a launch of the one- and two-wave kernels computes.  Each kernel family has ONE function that maps a mode to the template
// instance; an instance that does not exist cannot be named, and a mode a family lacks is a status, not a launch.
enum WgMode {
    WG_FWD,           // y = conv(x) (+ bias)
    WG_FWD_STATS,     // ... + the BatchNorm partial sums of y
    WG_FWD_STATS_PMAX,// ... + the 2x2 window maxima of y (E rides in the bias slot; k_wg3 on even maps only)
    WG_FWD_BNE,       // ... + eval-mode BatchNorm (+ ReLU), dead-channel skip: the inference epilogue
    WG_FWD_PRE,       // ... + PReLU (+ residual) instead of the BatchNorm, the same skip: SphereNet's inference epilogue
    WG_DGRAD,         // gx = dgrad(gy)
    WG_DGRAD_ADD,     // ... + addend (rides in the bias slot)
    WG_FWD_BNE_POOL   // WG_FWD_BNE + the MaxPool2d(2, 2) behind it: y is the pooled tensor (even maps; not ODD, SH or SPLIT)
};
struct WgLaunch {     // the arguments every instance takes
    const WgGeom &g;
    const float *x, *up, *bias;      // bias: the kernels' one slot -- wg_slot
    float *y, *stats;                // stats: passed under WG_FWD_STATS only
    const WgBnEval &bne;             // read under WG_FWD_BNE / WG_FWD_PRE only
    hipStream_t stream;
};
// The mode of a call, and what rides in the kernels' one slot under it: the addend, the window maxima E a caller attached
// (cpg_conv2d_fwd_attach_pool_max), else the bias.  ep->pool has no slot in the parameter block: the pooled epilogue is other code, not a
// run-time branch -- it picks the POOL instances, whose `y` is the pooled tensor.
static WgMode wg_mode(const cpg::WinoCall &c) {
    if (c.ep != nullptr) return c.ep->kind == cpg::EvalEpilogue::PRELU ? WG_FWD_PRE : c.ep->pool ? WG_FWD_BNE_POOL : WG_FWD_BNE;
    if (c.dgrad) return c.addend != nullptr ? WG_DGRAD_ADD : WG_DGRAD;
    return c.stats == nullptr ? WG_FWD : c.pool_max != nullptr ? WG_FWD_STATS_PMAX : WG_FWD_STATS;
}
static const float *wg_slot(WgMode mode, const cpg::WinoCall &c) {
    return mode == WG_DGRAD_ADD ? c.addend : mode == WG_FWD_STATS_PMAX ? c.pool_max : c.bias;
}
// The kernels' parameter block from the descriptor (null: no inference epilogue) -- the one place that knows which name of a pair each kind fills.
static WgBnEval wg_epilogue(const cpg::EvalEpilogue *ep, int *live, int m) {
    WgBnEval bn{};
    if (ep == nullptr) return bn;
    if (ep->kind == cpg::EvalEpilogue::PRELU)      // (the slots behind slope(), residual() and per_channel())
        bn.gamma = ep->slope, bn.beta = ep->residual, bn.relu = ep->per_channel ? 1 : 0;
    else
        bn.gamma = ep->gamma, bn.beta = ep->beta, bn.mean = ep->mean, bn.var = ep->var, bn.eps = ep->eps, bn.relu = ep->relu;
    bn.live = live, bn.Mp = pad_to(m, 128);
    return bn;
}
#define WG_GO(kernel, blocks, threads, a, stats_arg) \
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, (a).stream, (a).g, (a).x, (a).up, (a).bias, (a).y, stats_arg, (a).bne)

// k_wg3<DGRAD, STATS, BNE, ODD, SH, SPLIT, ADD, PMAX, PRE, POOL>: 23 instances (PRE: where BNE exists; POOL: the even-map BNE one).  ODD (odd maps) and SH (two units per four-wave block) exclude each
// other; SPLIT (a tail piece: raw partial output) exists for the plain forward and input gradient of even maps; SH has no BNE; PMAX
// (window maxima) exists for the statistics forward of even maps, SH or not.
template <bool ODD, bool SH, bool SPLIT>
static int wg3_launch(WgMode mode, unsigned blocks, const WgLaunch &a) {
    static_assert(!(ODD && (SH || SPLIT)), "k_wg3: the odd-map instances neither share the transform nor split the channel loop");
    constexpr int threads = SH ? 256 : 128;
    if constexpr (!SH && !SPLIT) {
        if (mode == WG_FWD_BNE) { WG_GO((k_wg3<false, false, true, ODD>), blocks, threads, a, nullptr); return CPG_OK; }
    }
    if constexpr (!SPLIT) {
        if (mode == WG_DGRAD_ADD) { WG_GO((k_wg3<true, false, false, ODD, SH, false, true>), blocks, threads, a, nullptr); return CPG_OK; }
    }
    if (mode == WG_DGRAD) { WG_GO((k_wg3<true, false, false, ODD, SH, SPLIT>), blocks, threads, a, nullptr); return CPG_OK; }
    if constexpr (!SPLIT) {
        if (mode == WG_FWD_STATS) { WG_GO((k_wg3<false, true, false, ODD, SH>), blocks, threads, a, a.stats); return CPG_OK; }
    }
    if constexpr (!SPLIT && !ODD) {
        if (mode == WG_FWD_STATS_PMAX) { WG_GO((k_wg3<false, true, false, false, SH, false, false, true>), blocks, threads, a, a.stats); return CPG_OK; }
    }
    if (mode == WG_FWD) { WG_GO((k_wg3<false, false, false, ODD, SH, SPLIT>), blocks, threads, a, nullptr); return CPG_OK; }
    if constexpr (!SH && !SPLIT) {
        if (mode == WG_FWD_PRE) { WG_GO((k_wg3<false, false, true, ODD, false, false, false, false, true>), blocks, threads, a, nullptr); return CPG_OK; }
    }
    if constexpr (!ODD && !SH && !SPLIT) {
        if (mode == WG_FWD_BNE_POOL) { WG_GO((k_wg3<false, false, true, false, false, false, false, false, false, true>), blocks, threads, a, nullptr); return CPG_OK; }
    }
    return fail(CPG_E_UNSUPPORTED, "conv3x3 (winograd): k_wg3 has no instance for mode %d (odd %d, shared %d, split %d)", (int)mode, ODD, SH, SPLIT);
}

// (The four launchers below stand in this order, and name their instances in this order, on purpose: the compiler emits kernels in the order
// of their first reference from host code, and host-side edits keep this file's device code byte-identical -- tools/build_digest.py.)

// The two-wave kernel's launch as planned: the main launch, then -- where the plan has a tail -- the leftover units of the last round as
// pieces of the channel loop (k_wg3<.., SPLIT>, raw partial outputs into the workspace behind the packed filter) and k_wg_tail_reduce,
// which adds the pieces (+ bias, + addend; with the BatchNorm statistics and the window maxima too) into y.
static int wg3_run(const WinoPlan &p, WgMode mode, const WgLaunch &whole, const cpg::WinoCall &c) {
    if (p.odd) return wg3_launch<true, false, false>(mode, p.grid, whole);
    const WgTail &t = p.tail;
    // piece 0's slice, addressed like y: its first image is n_first
    float *const part0 = reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(c.ws) + t.off) - (int64_t)t.n_first * p.g.M * p.g.H * p.g.W;
    auto reduce = [&]() {
        const dim3 rg(stream_grid((int64_t)(t.end_lb - t.first_lb) * 64 * W1_T, 256));
        if (mode == WG_FWD_STATS_PMAX)
            hipLaunchKernelGGL((k_wg_tail_reduce<true, true>), rg, dim3(256), 0, c.stream, t.g, part0, c.bias, c.y, t.first_lb, t.end_lb, c.stats, (const float *)c.pool_max);
        else if (c.stats != nullptr)
            hipLaunchKernelGGL(k_wg_tail_reduce<true>, rg, dim3(256), 0, c.stream, t.g, part0, c.bias, c.y, t.first_lb, t.end_lb, c.stats, (const float *)nullptr);
        else
            hipLaunchKernelGGL(k_wg_tail_reduce<false>, rg, dim3(256), 0, c.stream, t.g, part0, c.bias, c.y, t.first_lb, t.end_lb, (float *)nullptr, c.addend);
    };
    auto go = [&](bool split, WgMode md, unsigned blocks, const WgLaunch &a) {
        if (p.sh) return !split ? wg3_launch<false, true, false>(md, blocks, a) : wg3_launch<false, true, true>(md, blocks, a);
        return !split ? wg3_launch<false, false, false>(md, blocks, a) : wg3_launch<false, false, true>(md, blocks, a);
    };
    int rc = go(false, mode, p.grid, whole);
    if (rc != CPG_OK || !t.on) return rc;
    const WgBnEval none{};
    const WgLaunch pieces{t.g, c.x, whole.up, nullptr, part0, nullptr, none, c.stream};      // (forward or input gradient, nothing else)
    if ((rc = go(true, c.dgrad ? WG_DGRAD : WG_FWD, (unsigned)(t.left * t.S), pieces)) == CPG_OK) reduce();
    return rc;
}
// k_wg2<DGRAD, STATS, BNE, PRE, POOL> and k_wg1<DGRAD, STATS, BNE, PRE, POOL>: 6 instances each, no addend
static int wg2_launch(WgMode mode, unsigned blocks, const WgLaunch &a) {
    switch (mode) {
        case WG_FWD_BNE: WG_GO((k_wg2<false, false, true>), blocks, 128, a, nullptr); return CPG_OK;
        case WG_DGRAD: WG_GO((k_wg2<true, false>), blocks, 128, a, nullptr); return CPG_OK;
        case WG_FWD_STATS: WG_GO((k_wg2<false, true>), blocks, 128, a, a.stats); return CPG_OK;
        case WG_FWD: WG_GO((k_wg2<false, false>), blocks, 128, a, nullptr); return CPG_OK;
        case WG_FWD_PRE: WG_GO((k_wg2<false, false, true, true>), blocks, 128, a, nullptr); return CPG_OK;
        case WG_FWD_BNE_POOL: WG_GO((k_wg2<false, false, true, false, true>), blocks, 128, a, nullptr); return CPG_OK;
        default: return fail(CPG_E_UNSUPPORTED, "conv3x3 (winograd): k_wg2 takes no addend");
    }
}
static int wg1_launch(WgMode mode, unsigned blocks, const WgLaunch &a) {
    switch (mode) {
        case WG_FWD_BNE: WG_GO((k_wg1<false, false, true>), blocks, 256, a, nullptr); return CPG_OK;
        case WG_DGRAD: WG_GO((k_wg1<true, false>), blocks, 256, a, nullptr); return CPG_OK;
        case WG_FWD_STATS: WG_GO((k_wg1<false, true>), blocks, 256, a, a.stats); return CPG_OK;
        case WG_FWD: WG_GO((k_wg1<false, false>), blocks, 256, a, nullptr); return CPG_OK;
        case WG_FWD_PRE: WG_GO((k_wg1<false, false, true, true>), blocks, 256, a, nullptr); return CPG_OK;
        case WG_FWD_BNE_POOL: WG_GO((k_wg1<false, false, true, false, true>), blocks, 256, a, nullptr); return CPG_OK;
        default: return fail(CPG_E_UNSUPPORTED, "conv3x3 (winograd): k_wg1 takes no addend");
    }
}
#undef WG_GO
// the cooperative block kernel k_wg_fwd: its own pack (k_wg_pack's layout, `bk` channels per block), bias and statistics only
static void wg_block_run(const WinoPlan &p, const cpg::WinoCall &c) {
    const int bk = 8 * p.nw;
    float *up = (float *)c.ws;
    hipLaunchKernelGGL(k_wg_pack, dim3(stream_grid((int64_t)p.g.nkb * p.g.nch * bk * WG_CK, 256)), dim3(256), 0, c.stream, c.w, c.pm, c.thr, up,
                       c.K, c.C, c.m, c.c_read, p.g.nch, c.dgrad ? 1 : 0, bk);
    if (p.nw == 8) wino_launch<8>(c.dgrad != 0, p.g, p.grid, c.x, up, c.bias, c.y, c.stats, c.stream);
    else wino_launch<4>(c.dgrad != 0, p.g, p.grid, c.x, up, c.bias, c.y, c.stats, c.stream);
}

// The one entry (cpg_dispatch.h: cpg::WinoCall): validate, plan, take or pack the operand, launch the plan.
int cpg_conv3x3_wino_launch(const cpg::WinoCall &c) {
    char what[96];
    snprintf(what, sizeof what, "%s(winograd)", c.what);
    const cpg::EvalEpilogue *const ep = c.ep;
    // ---- validate: what the call asks for, then what the plan can carry
    CPG_REQUIRE(c.K == (c.dgrad ? c.c_read : c.m) && c.C == (c.dgrad ? c.m : c.c_read), "%s: the weight is [K][C][3][3], K x C = %d x %d here", what,
                c.dgrad ? c.c_read : c.m, c.dgrad ? c.m : c.c_read);
    if (ep != nullptr && ep->kind == cpg::EvalEpilogue::PRELU && ep->slope == nullptr) return fail(CPG_E_INVALID, "%s: null slope", what);
    if (ep != nullptr && ep->kind == cpg::EvalEpilogue::BN_EVAL && ep->residual != nullptr)
        return fail(CPG_E_UNSUPPORTED, "%s: no residual behind the BatchNorm", what);
    // addend: added to the result in the epilogue (k_wg3<.., ADD>; the tail pieces' share in k_wg_tail_reduce)
    if (c.addend != nullptr && (!c.dgrad || c.bias != nullptr || ep != nullptr || c.stats != nullptr))
        return fail(CPG_E_INVALID, "%s: an addend rides in plain input-gradient launches only", what);
    WinoWant want{c.dgrad != 0, ep != nullptr, true};
    WinoPlan p = wino_plan(want, c.N, c.c_read, c.m, c.H, c.W);
    if (!p.ok || (c.addend != nullptr && !p.addend)) return fail(CPG_E_UNSUPPORTED, "%s: shape not supported", what);
    if (ep != nullptr && !p.eval) return fail(CPG_E_UNSUPPORTED, "%s: the block kernels have no inference epilogue", what);
    if (ep != nullptr && ep->pool && (ep->kind != cpg::EvalEpilogue::BN_EVAL || !p.eval_pool))
        return fail(CPG_E_UNSUPPORTED, "%s: the pooled epilogue is the BatchNorm epilogue's, on the one- and two-wave kernels of an even map", what);
    if (c.ws == nullptr || c.ws_bytes < p.pack_bytes) return fail(CPG_E_WORKSPACE, "%s: workspace %zu < %zu bytes", what, c.ws_bytes, p.pack_bytes);
    CPG_REQUIRE((((uintptr_t)c.ws) & 15) == 0, "%s: workspace must be 16-byte aligned", what);
    if (!p.grid_ok) return fail(CPG_E_UNSUPPORTED, "%s: grid too large", what);
    // The run-time degrade: a caller whose workspace holds the packed filter but not the tail pieces (cpg_conv2d_workspace_bytes of an
    // older release) gets the plan without a tail -- the single launch.
    if (p.tail.on && c.ws_bytes < p.tail.off + p.tail.bytes) want.tail = false, p = wino_plan(want, c.N, c.c_read, c.m, c.H, c.W);
    // ---- the operand: the caller's, or packed here.  (The inference epilogue's pack also writes the liveness flags -- zeroed first --: never
    // taken from a caller's operand.)
    const WgBnEval bne = wg_epilogue(ep, c.live, c.m);
    if (c.live != nullptr) {
        hipError_t e = hipMemsetAsync(c.live, 0, c.live_words * sizeof(int), c.stream);
        if (e != hipSuccess) return hip_status(e, what);
    }
    const float *up = (const float *)c.ws;
    if (p.variant != WV_BLOCK) {
        const cpg::PackedOperand pre = ep == nullptr ? c.packed : cpg::PackedOperand();
        if (const int rc = cpg::packed_fits(pre, p.pack_bytes, what)) return rc;
        if (pre.data != nullptr)
            up = pre.data;
        else
            hipLaunchKernelGGL(k_wg1_pack, dim3(stream_grid(p.job.total, 256)), dim3(256), 0, c.stream, c.w, c.pm, c.thr, (float *)c.ws, c.K, c.C, c.m,
                               c.c_read, p.job.c, p.job.d, bne.live, bne.Mp);
    }
    // ---- the launch
    const WgMode mode = wg_mode(c);
    const WgLaunch whole{p.g, c.x, up, wg_slot(mode, c), c.y, c.stats, bne, c.stream};
    int rc = CPG_OK;
    switch (p.variant) {
        case WV_PAIR64: rc = wg3_run(p, mode, whole, c); break;
        case WV_PAIR: rc = wg2_launch(mode, p.grid, whole); break;
        case WV_WAVE: rc = wg1_launch(mode, p.grid, whole); break;
        default: wg_block_run(p, c);
    }
    if (rc != CPG_OK) return rc;
    CPG_CHECK_LAUNCH(what);
    return CPG_OK;
}

// today's signature, for tools/wino_bench.py in a CPG_EXPORT_ALL build: a plain forward (stats may be null) or input gradient
extern "C" int cpg_conv3x3_wino_run(int dgrad, int N, int c_read, int m, int H, int W, int K, int C, const float *x,
                                    const float *w, const float *pm, float thr, const float *bias, float *y, float *stats,
                                    void *ws, size_t ws_bytes, hipStream_t stream) {
    cpg::WinoCall c{};
    c.dgrad = dgrad, c.N = N, c.c_read = c_read, c.m = m, c.H = H, c.W = W, c.K = K, c.C = C;
    c.x = x, c.w = w, c.pm = pm, c.thr = thr, c.bias = bias, c.y = y, c.stats = stats;
    c.ws = ws, c.ws_bytes = ws_bytes, c.stream = stream, c.what = dgrad ? "cpg_conv2d_dgrad" : "cpg_conv2d_fwd";
    return cpg_conv3x3_wino_launch(c);
}

// cpg_conv2d_pack's launch (declared in cpg_common.h): job b may be null
int cpg::pack_jobs_launch(const cpg::PackJob *ja, float *dst_a, const cpg::PackJob *jb, float *dst_b, const float *w, const float *pm, float thr,
                          hipStream_t stream) {
    auto args = [](const cpg::PackJob *j, float *dst) {
        if (j == nullptr) return PackArgs{0, 0, 0, 0, 0, 0, 0, 0, nullptr};
        return PackArgs{j->family, j->K, j->C, j->a, j->b, j->c, j->d, j->total, dst};
    };
    const PackArgs a = args(ja, dst_a), b = args(jb, dst_b);
    if (a.total + b.total <= 0) return CPG_OK;
    hipLaunchKernelGGL(k_pack_jobs, dim3(stream_grid(a.total + b.total, 256)), dim3(256), 0, stream, a, b, w, pm, thr);
    CPG_CHECK_LAUNCH("cpg_conv2d_pack");
    return CPG_OK;
}
