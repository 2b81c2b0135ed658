// Grouped and depthwise masked conv2d (groups > 1), fp32: forward, input gradient and weight gradient of
// F.conv2d(x, W * bin(pm), bias, stride, padding, dilation, groups) for ANY kernel size / stride / padding / dilation.
//
// Weight, piggymask and their gradients are [K][C/G][R][S]; group g reads input channels [g*C/G, (g+1)*C/G) and writes output
// channels [g*K/G, (g+1)*K/G).  Every pass runs ALL groups in ONE main launch that addresses the NCHW tensors in place (channel
// offset of the group + the full tensor's image stride): no slices, no concatenation.  Two kernel families:
//
//   narrow (C/G < 16 or K/G < 16: depthwise, channel multipliers, ResNeXt-32x4d-style groups) -- direct VALU kernels.  fp32 MFMA runs
//       at the fp32 vector rate on gfx950, so nothing is given up, and a depthwise 3x3 is HBM-bound (9 MACs per 8 bytes) anyway.
//       A wave owns 64 strips of TW adjacent outputs of one (image, group, block of <= 8 output channels) plane, so the masked taps
//       W * bin(pm) are wave-uniform (scalar registers); under stride 1 / dilation 1 a lane reads the TW + S - 1 values of a row that its strip needs
//       once, as separate 4-byte loads (no LDS halo tile and no vector loads: neighbouring lanes' segments overlap by S - 1 values and
//       the caches serve the overlap -- the kernel reaches a fraction of the copy rate, profiles/grouped_conv.md), the outputs leave
//       as 16-byte stores where the row length allows.  The input gradient is the same kernel
//       with the taps flipped and the roles of C/G and K/G swapped (a divisibility test per tap when the stride is > 1).
//       Weight gradient: one block per (output channel, image slice), per-lane partial taps, wave + block reduction in a fixed
//       order, partials to the workspace, then k_split_reduce (igemm_core.h) with the autograd epilogue of bin(pm) * W.
//   wide (>= 16 channels per group on both sides) -- the fp32-MFMA implicit GEMM of igemm_core.h with the group as a grid
//       dimension and the output-channel tile (32 / 64 / 128 rows) chosen by the group's width.
//
// No floating-point atomics anywhere: results are bit-identical run to run.
#include "cpg_dispatch.h"

using namespace cpg;

namespace {

struct GGeom {
    int N, C, H, W, K, R, S, sh, sw, ph, pw, dh, dw, OH, OW;
    int G, Cg, Kg;
};

GGeom make_ggeom(const cpg_conv_desc *d) {
    GGeom g{d->N, d->C, d->H, d->W, d->K, d->R, d->S, d->stride_h, d->stride_w, d->pad_h, d->pad_w, d->dil_h, d->dil_w, 0, 0,
            d->groups, d->C / d->groups, d->K / d->groups};
    g.OH = (d->H + 2 * d->pad_h - d->dil_h * (d->R - 1) - 1) / d->stride_h + 1;
    g.OW = (d->W + 2 * d->pad_w - d->dil_w * (d->S - 1) - 1) / d->stride_w + 1;
    return g;
}

// the measured boundary between the two families (profiles/grouped_conv.md; CPG_GROUPED_WIDE_MIN moves it for A/B runs)
inline bool wide_groups(const GGeom &g) {
    const int lo = std::max(1, opt_or(OPT_GROUPED_WIDE_MIN, 16));
    return g.Cg >= lo && g.Kg >= lo && g.G <= 65535;      // (the group is grid.y / grid.z there)
}

// ================================================================================== narrow groups: direct kernels
// Forward (DGRAD = false): in = x [N][C][H][W], out = y [N][K][OH][OW]; contraction over the group's Cg input channels.
// Input gradient (DGRAD = true): in = gy [N][K][OH][OW], out = gx [N][C][H][W]; contraction over the group's Kg output channels.
// KS > 0: R == S == KS at compile time (taps in registers); KS == 0: any R, S.  OCB: produced channels per wave.
// UNIT: stride 1 and dilation 1 (row segments shared by the TW outputs of a strip).
template <int KS, int OCB, int TW, bool UNIT, bool DGRAD>
__global__ __launch_bounds__(256) void k_gd(GGeom g, const float *__restrict__ in, const float *__restrict__ w,
                                            const float *__restrict__ pm, float thr, const float *__restrict__ bias,
                                            float *__restrict__ out, int vec_ok) {
    const int IH = DGRAD ? g.OH : g.H, IW = DGRAD ? g.OW : g.W;            // plane that is read
    const int OHo = DGRAD ? g.H : g.OH, OWo = DGRAD ? g.W : g.OW;          // plane that is written
    const int ICg = DGRAD ? g.Kg : g.Cg, OCg = DGRAD ? g.Cg : g.Kg;
    const int ICt = DGRAD ? g.K : g.C, OCt = DGRAD ? g.C : g.K;
    const int R = KS ? KS : g.R, S = KS ? KS : g.S, RS = R * S;
    const int spr = (OWo + TW - 1) / TW, nstrip = OHo * spr, wpp = (nstrip + 63) / 64;
    const int nchunk = (OCg + OCB - 1) / OCB;
    // wave-uniform: which plane this wave works on
    const int64_t wid = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t plane = wid / wpp;
    if (plane >= (int64_t)g.N * g.G * nchunk) return;
    const int wq = (int)(wid - plane * wpp);
    const int n = (int)(plane / (g.G * nchunk)), chunk = (int)(plane - (int64_t)n * (g.G * nchunk));
    const int grp = chunk / nchunk, oc0 = (chunk - grp * nchunk) * OCB;
    const int st = wq * 64 + (int)(threadIdx.x & 63);
    const bool valid = st < nstrip;
    const int a = valid ? st / spr : 0;
    const int b0 = valid ? (st - a * spr) * TW : 0;

    float acc[OCB][TW];
#pragma unroll
    for (int oc = 0; oc < OCB; ++oc)
#pragma unroll
        for (int t = 0; t < TW; ++t) acc[oc][t] = 0.0f;

    // masked tap of (produced channel oc0 + oc, contracted channel ic, tap rs); 0 past the group's last channel
    auto tap = [&](int oc, int ic, int rs) -> float {
        const int o = oc0 + oc;
        if (o >= OCg) return 0.0f;
        const int64_t idx = DGRAD ? ((int64_t)(grp * g.Kg + ic) * g.Cg + o) * RS + rs : ((int64_t)(grp * g.Kg + o) * g.Cg + ic) * RS + rs;
        float v = w[idx];
        if (pm != nullptr) v *= binarize(pm[idx], thr);
        return v;
    };

    for (int ic = 0; ic < ICg; ++ic) {
        const float *inp = in + ((int64_t)n * ICt + grp * ICg + ic) * IH * IW;
        if constexpr (KS > 0) {
            float wv[OCB][KS * KS];
#pragma unroll
            for (int oc = 0; oc < OCB; ++oc)
#pragma unroll
                for (int rs = 0; rs < KS * KS; ++rs) wv[oc][rs] = tap(oc, ic, rs);
#pragma unroll
            for (int r = 0; r < KS; ++r) {
                int ia;
                bool rowok = valid;
                if (!DGRAD) {
                    ia = a * g.sh - g.ph + r * g.dh;
                    rowok = rowok && (unsigned)ia < (unsigned)IH;
                } else {
                    const int t = a + g.ph - r * g.dh;
                    ia = t / g.sh;
                    rowok = rowok && t >= 0 && ia * g.sh == t && ia < IH;
                }
                const int rowoff = rowok ? ia * IW : 0;
                if constexpr (UNIT) {
                    constexpr int SEG = TW + KS - 1;
                    const int ib0 = DGRAD ? b0 + g.pw - (KS - 1) : b0 - g.pw;
                    float seg[SEG];
#pragma unroll
                    for (int j = 0; j < SEG; ++j) {
                        const int ib = ib0 + j;
                        const bool ok = rowok && (unsigned)ib < (unsigned)IW;
                        const float v = inp[ok ? rowoff + ib : 0];
                        seg[j] = ok ? v : 0.0f;
                    }
#pragma unroll
                    for (int s = 0; s < KS; ++s)
#pragma unroll
                        for (int t = 0; t < TW; ++t) {
                            const float v = seg[DGRAD ? t + (KS - 1 - s) : t + s];
#pragma unroll
                            for (int oc = 0; oc < OCB; ++oc) acc[oc][t] = fmaf(wv[oc][r * KS + s], v, acc[oc][t]);
                        }
                } else {
#pragma unroll
                    for (int s = 0; s < KS; ++s)
#pragma unroll
                        for (int t = 0; t < TW; ++t) {
                            int ib;
                            bool ok = rowok;
                            if (!DGRAD) {
                                ib = (b0 + t) * g.sw - g.pw + s * g.dw;
                                ok = ok && (unsigned)ib < (unsigned)IW;
                            } else {
                                const int u = b0 + t + g.pw - s * g.dw;
                                ib = u / g.sw;
                                ok = ok && u >= 0 && ib * g.sw == u && ib < IW;
                            }
                            float v = inp[ok ? rowoff + ib : 0];
                            v = ok ? v : 0.0f;
#pragma unroll
                            for (int oc = 0; oc < OCB; ++oc) acc[oc][t] = fmaf(wv[oc][r * KS + s], v, acc[oc][t]);
                        }
                }
            }
        } else {
            for (int r = 0; r < R; ++r) {
                int ia;
                bool rowok = valid;
                if (!DGRAD) {
                    ia = a * g.sh - g.ph + r * g.dh;
                    rowok = rowok && (unsigned)ia < (unsigned)IH;
                } else {
                    const int t = a + g.ph - r * g.dh;
                    ia = t / g.sh;
                    rowok = rowok && t >= 0 && ia * g.sh == t && ia < IH;
                }
                const int rowoff = rowok ? ia * IW : 0;
                for (int s = 0; s < S; ++s) {
                    float wv[OCB];
#pragma unroll
                    for (int oc = 0; oc < OCB; ++oc) wv[oc] = tap(oc, ic, r * S + s);
#pragma unroll
                    for (int t = 0; t < TW; ++t) {
                        int ib;
                        bool ok = rowok;
                        if (!DGRAD) {
                            ib = (b0 + t) * g.sw - g.pw + s * g.dw;
                            ok = ok && (unsigned)ib < (unsigned)IW;
                        } else {
                            const int u = b0 + t + g.pw - s * g.dw;
                            ib = u / g.sw;
                            ok = ok && u >= 0 && ib * g.sw == u && ib < IW;
                        }
                        float v = inp[ok ? rowoff + ib : 0];
                        v = ok ? v : 0.0f;
#pragma unroll
                        for (int oc = 0; oc < OCB; ++oc) acc[oc][t] = fmaf(wv[oc], v, acc[oc][t]);
                    }
                }
            }
        }
    }

    if (!valid) return;
#pragma unroll
    for (int oc = 0; oc < OCB; ++oc) {
        const int o = oc0 + oc;
        if (o >= OCg) break;
        const int ch = grp * OCg + o;
        const float bv = (!DGRAD && bias != nullptr) ? bias[ch] : 0.0f;
        float *dst = out + ((int64_t)n * OCt + ch) * OHo * OWo + (int64_t)a * OWo + b0;
        if (TW == 4 && vec_ok) {            // OWo % 4 == 0 and a 16-byte aligned tensor: the whole strip is inside the row
            f32x4 v = {acc[oc][0] + bv, acc[oc][TW > 1 ? 1 : 0] + bv, acc[oc][TW > 2 ? 2 : 0] + bv, acc[oc][TW > 3 ? 3 : 0] + bv};
            *reinterpret_cast<f32x4 *>(dst) = v;
        } else {
#pragma unroll
            for (int t = 0; t < TW; ++t)
                if (b0 + t < OWo) dst[t] = acc[oc][t] + bv;
        }
    }
}

template <int KS, int OCB, bool DGRAD>
void launch_gd_ocb(const GGeom &g, const float *in, const float *w, const float *pm, float thr, const float *bias, float *out,
                   hipStream_t stream) {
    const int OHo = DGRAD ? g.H : g.OH, OWo = DGRAD ? g.W : g.OW, OCg = DGRAD ? g.Cg : g.Kg;
    const bool unit = g.sh == 1 && g.sw == 1 && g.dh == 1 && g.dw == 1;
    const int tw = OWo >= 16 ? 4 : 1;                   // narrow maps: one output per lane keeps the lanes of a wave busy
    const int spr = (OWo + tw - 1) / tw;
    const int64_t wpp = ((int64_t)OHo * spr + 63) / 64;
    const int64_t waves = (int64_t)g.N * g.G * ((OCg + OCB - 1) / OCB) * wpp;
    const dim3 grid((unsigned)((waves + 3) / 4));
    const int vec_ok = (OWo % 4 == 0 && (((uintptr_t)out) & 15) == 0) ? 1 : 0;
    if constexpr (KS > 0) {
        if (tw == 4 && unit) {
            hipLaunchKernelGGL((k_gd<KS, OCB, 4, true, DGRAD>), grid, dim3(256), 0, stream, g, in, w, pm, thr, bias, out, vec_ok);
            return;
        }
    }
    if (tw == 4)
        hipLaunchKernelGGL((k_gd<KS, OCB, 4, false, DGRAD>), grid, dim3(256), 0, stream, g, in, w, pm, thr, bias, out, vec_ok);
    else
        hipLaunchKernelGGL((k_gd<KS, OCB, 1, false, DGRAD>), grid, dim3(256), 0, stream, g, in, w, pm, thr, bias, out, vec_ok);
}

template <int KS, bool DGRAD>
void launch_gd_ks(const GGeom &g, const float *in, const float *w, const float *pm, float thr, const float *bias, float *out,
                  hipStream_t stream) {
    const int OCg = DGRAD ? g.Cg : g.Kg;
    if (OCg == 1) launch_gd_ocb<KS, 1, DGRAD>(g, in, w, pm, thr, bias, out, stream);
    else if (OCg == 2) launch_gd_ocb<KS, 2, DGRAD>(g, in, w, pm, thr, bias, out, stream);
    else if (OCg <= 4) launch_gd_ocb<KS, 4, DGRAD>(g, in, w, pm, thr, bias, out, stream);
    else launch_gd_ocb<KS, 8, DGRAD>(g, in, w, pm, thr, bias, out, stream);
}

template <bool DGRAD>
void launch_gd(const GGeom &g, const float *in, const float *w, const float *pm, float thr, const float *bias, float *out,
               hipStream_t stream) {
    if (g.R == 3 && g.S == 3) launch_gd_ks<3, DGRAD>(g, in, w, pm, thr, bias, out, stream);
    else if (g.R == 5 && g.S == 5) launch_gd_ks<5, DGRAD>(g, in, w, pm, thr, bias, out, stream);
    else launch_gd_ks<0, DGRAD>(g, in, w, pm, thr, bias, out, stream);
}

// blocks (4 waves each) of the grid launch_gd builds; the entry points refuse a descriptor for which grid.x would not hold them
inline int64_t gd_blocks(const GGeom &g, bool dgrad) {
    const int OHo = dgrad ? g.H : g.OH, OWo = dgrad ? g.W : g.OW, OCg = dgrad ? g.Cg : g.Kg;
    const int ocb = OCg <= 2 ? OCg : OCg <= 4 ? 4 : 8;
    const int tw = OWo >= 16 ? 4 : 1;
    const int64_t wpp = ((int64_t)OHo * ((OWo + tw - 1) / tw) + 63) / 64;
    return ((int64_t)g.N * g.G * ((OCg + ocb - 1) / ocb) * wpp + 3) / 4;
}

// ---- weight gradient: block (output channel co, image slice); part[slice][co][ci][r][s] ----
// Every thread sums its pixels' products per tap, the block adds the 256 partial sums in a fixed order (wave butterfly, then waves 0..3).
template <int KS>
__global__ __launch_bounds__(256) void k_gd_wgrad(GGeom g, const float *__restrict__ x, const float *__restrict__ gy,
                                                  float *__restrict__ part, int ips) {
    constexpr int NT = KS > 0 ? KS * KS : 1;
    __shared__ float red[4][NT];
    const int co = blockIdx.x, grp = co / g.Kg;
    const int n0 = blockIdx.y * ips, n1 = min(g.N, n0 + ips);
    const int S = KS ? KS : g.S, RS = (KS ? KS : g.R) * S;
    const int ohw = g.OH * g.OW;
    const int64_t hw = (int64_t)g.H * g.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *dst = part + ((int64_t)blockIdx.y * g.K + co) * g.Cg * RS;
    for (int ci = 0; ci < g.Cg; ++ci) {
        for (int rs0 = 0; rs0 < RS; rs0 += NT) {              // (KS > 0: one trip)
            float acc[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = 0.0f;
            for (int n = n0; n < n1; ++n) {
                const float *gyp = gy + ((int64_t)n * g.K + co) * ohw;
                const float *xp = x + ((int64_t)n * g.C + grp * g.Cg + ci) * hw;
                for (int q = threadIdx.x; q < ohw; q += 256) {
                    const int oh = q / g.OW, ow = q - oh * g.OW;
                    const float gv = gyp[q];
                    const int ih0 = oh * g.sh - g.ph, iw0 = ow * g.sw - g.pw;
#pragma unroll
                    for (int i = 0; i < NT; ++i) {
                        const int rs = rs0 + i;
                        const int r = rs / S, s = rs - r * S;
                        const int ih = ih0 + r * g.dh, iw = iw0 + s * g.dw;
                        const bool ok = (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
                        const float xv = xp[ok ? ih * g.W + iw : 0];
                        acc[i] = fmaf(gv, ok ? xv : 0.0f, acc[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                float v = acc[i];
                for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
                if (lane == 0) red[wave][i] = v;
            }
            __syncthreads();
            if ((int)threadIdx.x < NT) dst[(int64_t)ci * RS + rs0 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
            __syncthreads();
        }
    }
}

// image slices of the narrow weight gradient: ~8 blocks per CU, at least one image per slice
inline void gd_wgrad_plan(const GGeom &g, int &slices, int &ips) {
    int want = std::max(1, std::min(g.N, (8 * kCUs + g.K - 1) / g.K));
    ips = (g.N + want - 1) / want;
    slices = (g.N + ips - 1) / ips;
}

// ================================================================================== wide groups: fp32-MFMA implicit GEMM
// The loaders of igemm_conv.hip with the group's channel window: the tensor pointer already points at the group's first channel, `istride`
// is the FULL tensor's image stride and the channel loops stop at the group's width.
template <int BN, int BK>
struct GFwdBLoader {      // B[k=(ci,r,s)][j=p]
    static constexpr int N = BN * BK / 256;
    static constexpr int KSTEP = 256 / BN;
    const float *x;
    int H, W, R, S, dh, dw, Kd;
    int ih0, iw0, t_j, t_k;
    int64_t xbase;
    bool jvalid;
    unsigned okmask;
    __device__ __forceinline__ void init(const float *x_, const GGeom &g, int64_t p0, int64_t P) {
        x = x_; H = g.H; W = g.W; R = g.R; S = g.S; dh = g.dh; dw = g.dw; Kd = g.Cg * g.R * g.S;
        t_j = threadIdx.x % BN;
        t_k = threadIdx.x / BN;
        const int64_t p = p0 + t_j;
        jvalid = p < P;
        const int ohw = g.OH * g.OW;
        const int n = jvalid ? (int)(p / ohw) : 0;
        const int q = jvalid ? (int)(p % ohw) : 0;
        const int oh = q / g.OW, ow = q % g.OW;
        ih0 = oh * g.sh - g.ph;
        iw0 = ow * g.sw - g.pw;
        xbase = (int64_t)n * g.C * H * W;
    }
    __device__ __forceinline__ void fetch(int kt, float (&r)[N]) {
        const int RS = R * S;
        okmask = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int k = kt * BK + t_k + KSTEP * i;
            const int ci = k / RS, rs = k - ci * RS;
            const int rr = rs / S, ss = rs - rr * S;
            const int ih = ih0 + rr * dh, iw = iw0 + ss * dw;
            const bool ok = jvalid && k < Kd && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
            okmask |= (ok ? 1u : 0u) << i;
            r[i] = x[ok ? xbase + ((int64_t)ci * H + ih) * W + iw : 0];
        }
    }
    __device__ __forceinline__ void put(const float (&r)[N], float *lds) {
#pragma unroll
        for (int i = 0; i < N; ++i) lds[(t_k + KSTEP * i) * (BN + 1) + t_j] = ((okmask >> i) & 1u) ? r[i] : 0.0f;
    }
};

template <int BN, int BK>
struct GDgradBLoader {    // B[k=(co,r,s)][j=q=(n,h,w)] = gy[n][co][(h+ph-r*dh)/sh][(w+pw-s*dw)/sw] when divisible and in range
    static constexpr int N = BN * BK / 256;
    static constexpr int KSTEP = 256 / BN;
    const float *gy;
    int OH, OW, R, S, dh, dw, sh, sw, Kd;
    int th0, tw0, t_j, t_k;
    int64_t base;
    bool jvalid;
    unsigned okmask;
    __device__ __forceinline__ void init(const float *gy_, const GGeom &g, int64_t q0, int64_t Q) {
        gy = gy_; OH = g.OH; OW = g.OW; R = g.R; S = g.S; dh = g.dh; dw = g.dw; sh = g.sh; sw = g.sw;
        Kd = g.Kg * g.R * g.S;
        t_j = threadIdx.x % BN;
        t_k = threadIdx.x / BN;
        const int64_t q = q0 + t_j;
        jvalid = q < Q;
        const int hw = g.H * g.W;
        const int n = jvalid ? (int)(q / hw) : 0;
        const int rem = jvalid ? (int)(q % hw) : 0;
        th0 = rem / g.W + g.ph;
        tw0 = rem % g.W + g.pw;
        base = (int64_t)n * g.K * OH * OW;
    }
    __device__ __forceinline__ void fetch(int kt, float (&r)[N]) {
        const int RS = R * S;
        okmask = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int k = kt * BK + t_k + KSTEP * i;
            const int co = k / RS, rs = k - co * RS;
            const int rr = rs / S, ss = rs - rr * S;
            const int th = th0 - rr * dh, tw = tw0 - ss * dw;
            bool ok = jvalid && k < Kd && th >= 0 && tw >= 0;
            int oh = th, ow = tw;
            if (sh != 1) { oh = th / sh; ok = ok && (oh * sh == th); }
            if (sw != 1) { ow = tw / sw; ok = ok && (ow * sw == tw); }
            ok = ok && oh < OH && ow < OW;
            okmask |= (ok ? 1u : 0u) << i;
            r[i] = gy[ok ? base + ((int64_t)co * OH + oh) * OW + ow : 0];
        }
    }
    __device__ __forceinline__ void put(const float (&r)[N], float *lds) {
#pragma unroll
        for (int i = 0; i < N; ++i) lds[(t_k + KSTEP * i) * (BN + 1) + t_j] = ((okmask >> i) & 1u) ? r[i] : 0.0f;
    }
};

template <int BM, int BK>
struct GDgradALoader {    // A[k=(co,r,s)][m=ci] = Weff[co][ci][r][s] of the group (w points at the group's first row)
    static constexpr int N = BM * BK / 256;
    static constexpr int MSTEP = 256 / BK;
    const float *w, *pm;
    float thr;
    int Cg, RS, Kd, m0, t_k, t_m;
    unsigned okmask;
    float rp[N];
    __device__ __forceinline__ void init(const float *w_, const float *pm_, float thr_, const GGeom &g, int m0_) {
        w = w_; pm = pm_; thr = thr_; Cg = g.Cg; RS = g.R * g.S; Kd = g.Kg * RS; m0 = m0_;
        t_k = threadIdx.x % BK;
        t_m = threadIdx.x / BK;
    }
    __device__ __forceinline__ void fetch(int kt, float (&r)[N]) {
        const int k = kt * BK + t_k;
        const int co = k / RS, rs = k - co * RS;
        okmask = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int ci = m0 + t_m + MSTEP * i;
            const bool ok = k < Kd && ci < Cg;
            const int64_t off = ok ? ((int64_t)co * Cg + ci) * RS + rs : 0;
            okmask |= (ok ? 1u : 0u) << i;
            r[i] = w[off];
            if (pm != nullptr) rp[i] = pm[off];            // wave-uniform condition
        }
    }
    __device__ __forceinline__ void put(const float (&r)[N], float *lds) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            float v = r[i];
            if (pm != nullptr) v *= binarize(rp[i], thr);
            lds[t_k * (BM + 1) + t_m + MSTEP * i] = ((okmask >> i) & 1u) ? v : 0.0f;
        }
    }
};

template <int BM, int BK>
struct GWgradALoader {    // A[k=p][m=co] = gy[n_p][co][q_p]
    static constexpr int N = BM * BK / 256;
    static constexpr int MSTEP = 256 / BK;
    const float *gy;
    int Kg, OHW, m0, t_k, t_m;
    int64_t istride, P;
    unsigned okmask;
    __device__ __forceinline__ void init(const float *gy_, const GGeom &g, int m0_) {
        gy = gy_; Kg = g.Kg; OHW = g.OH * g.OW; m0 = m0_; P = (int64_t)g.N * OHW; istride = (int64_t)g.K * OHW;
        t_k = threadIdx.x % BK;
        t_m = threadIdx.x / BK;
    }
    __device__ __forceinline__ void fetch(int kt, float (&r)[N]) {
        const int64_t p = (int64_t)kt * BK + t_k;
        const bool pv = p < P;
        const int n = pv ? (int)(p / OHW) : 0;
        const int q = pv ? (int)(p % OHW) : 0;
        const int64_t b = (int64_t)n * istride + q;
        okmask = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int co = m0 + t_m + MSTEP * i;
            const bool ok = pv && co < Kg;
            okmask |= (ok ? 1u : 0u) << i;
            r[i] = gy[ok ? b + (int64_t)co * OHW : 0];
        }
    }
    __device__ __forceinline__ void put(const float (&r)[N], float *lds) {
#pragma unroll
        for (int i = 0; i < N; ++i) lds[t_k * (BM + 1) + t_m + MSTEP * i] = ((okmask >> i) & 1u) ? r[i] : 0.0f;
    }
};

template <int BN, int BK>
struct GWgradBLoader {    // B[k=p][j=(ci,r,s)] = x[n_p][ci][oh*sh-ph+r*dh][ow*sw-pw+s*dw]
    static constexpr int N = BN * BK / 256;
    static constexpr int JSTEP = 256 / BK;
    const float *x;
    int H, W, OW, OHW, sh, sw, ph, pw, t_k, t_j;
    int64_t istride, P;
    unsigned okmask;
    int joff[N];      // ci*H*W + r*dh*W + s*dw, or -1 when j is out of range
    int jrs[N];       // (r*dh) << 16 | (s*dw)
    __device__ __forceinline__ void init(const float *x_, const GGeom &g, int j0) {
        x = x_; H = g.H; W = g.W; OW = g.OW; OHW = g.OH * g.OW; sh = g.sh; sw = g.sw; ph = g.ph; pw = g.pw;
        P = (int64_t)g.N * OHW;
        istride = (int64_t)g.C * H * W;
        t_k = threadIdx.x % BK;
        t_j = threadIdx.x / BK;
        const int RS = g.R * g.S, J = g.Cg * RS;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int j = j0 + t_j + JSTEP * i;
            if (j < J) {
                const int ci = j / RS, rs = j - ci * RS;
                const int rr = (rs / g.S) * g.dh, ss = (rs % g.S) * g.dw;
                joff[i] = ci * H * W + rr * W + ss;
                jrs[i] = (rr << 16) | ss;
            } else {
                joff[i] = -1;
                jrs[i] = 0;
            }
        }
    }
    __device__ __forceinline__ void fetch(int kt, float (&r)[N]) {
        const int64_t p = (int64_t)kt * BK + t_k;
        const bool pv = p < P;
        const int n = pv ? (int)(p / OHW) : 0;
        const int q = pv ? (int)(p % OHW) : 0;
        const int oh = q / OW, ow = q - oh * OW;
        const int ih0 = oh * sh - ph, iw0 = ow * sw - pw;
        const int64_t b = (int64_t)n * istride + (int64_t)ih0 * W + iw0;
        okmask = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int ih = ih0 + (jrs[i] >> 16), iw = iw0 + (jrs[i] & 0xFFFF);
            const bool ok = pv && joff[i] >= 0 && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
            okmask |= (ok ? 1u : 0u) << i;
            r[i] = x[ok ? b + joff[i] : 0];
        }
    }
    __device__ __forceinline__ void put(const float (&r)[N], float *lds) {
#pragma unroll
        for (int i = 0; i < N; ++i) lds[t_k * (BN + 1) + t_j + JSTEP * i] = ((okmask >> i) & 1u) ? r[i] : 0.0f;
    }
};

// blockIdx.y = group
template <class Cfg>
__global__ __launch_bounds__(256) void k_gw_fwd(GGeom g, const float *__restrict__ x, const float *__restrict__ w,
                                                const float *__restrict__ pm, float thr, const float *__restrict__ bias,
                                                float *__restrict__ y, int tiles_m) {
    __shared__ float smem[Cfg::SMEM_FLOATS];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int grp = blockIdx.y;
    const int tm = lb % tiles_m, tn = lb / tiles_m;
    const int Kd = g.Cg * g.R * g.S;
    const int ohw = g.OH * g.OW;
    const int64_t P = (int64_t)g.N * ohw;
    const int m0 = tm * Cfg::BM;
    const int64_t p0 = (int64_t)tn * Cfg::BN;
    const int64_t woff = (int64_t)grp * g.Kg * Kd;
    GFwdBLoader<Cfg::BN, Cfg::BK> lbB;
    lbB.init(x + (int64_t)grp * g.Cg * g.H * g.W, g, p0, P);
    f32x16 acc[Cfg::FM][Cfg::FN];
    const int nkt = (Kd + Cfg::BK - 1) / Cfg::BK;
    if (pm != nullptr) {
        DenseLoader<Cfg::BM, Cfg::BK, true, true> la;
        la.init(w + woff, pm + woff, thr, Kd, m0, g.Kg, Kd);
        igemm_mainloop<Cfg>(la, lbB, 0, nkt, smem, acc);
    } else {
        DenseLoader<Cfg::BM, Cfg::BK, true, false> la0;
        la0.init(w + woff, nullptr, thr, Kd, m0, g.Kg, Kd);
        igemm_mainloop<Cfg>(la0, lbB, 0, nkt, smem, acc);
    }
    int64_t colbase[Cfg::FN];           // n*K*ohw + q per fragment column, -1 when past the end
    col_setup<Cfg>(colbase, [&](int j) -> int64_t {
        const int64_t p = p0 + j;
        if (p >= P) return -1;
        const int n = (int)(p / ohw), q = (int)(p - (int64_t)n * ohw);
        return (int64_t)n * g.K * ohw + q;
    });
    for_each_acc<Cfg>(acc, [&](int m, int j, int fn, float v) {
        const int co = m0 + m;
        if (co < g.Kg && colbase[fn] >= 0) {
            const int ch = grp * g.Kg + co;
            y[colbase[fn] + (int64_t)ch * ohw] = bias != nullptr ? v + bias[ch] : v;
        }
    });
}

template <class Cfg>
__global__ __launch_bounds__(256) void k_gw_dgrad(GGeom g, const float *__restrict__ gy, const float *__restrict__ w,
                                                  const float *__restrict__ pm, float thr, float *__restrict__ gx, int tiles_m) {
    __shared__ float smem[Cfg::SMEM_FLOATS];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int grp = blockIdx.y;
    const int tm = lb % tiles_m, tn = lb / tiles_m;
    const int Kd = g.Kg * g.R * g.S;
    const int hw = g.H * g.W;
    const int64_t Q = (int64_t)g.N * hw;
    const int m0 = tm * Cfg::BM;
    const int64_t q0 = (int64_t)tn * Cfg::BN;
    const int64_t woff = (int64_t)grp * g.Kg * g.Cg * g.R * g.S;
    GDgradALoader<Cfg::BM, Cfg::BK> la;
    la.init(w + woff, pm != nullptr ? pm + woff : nullptr, thr, g, m0);
    GDgradBLoader<Cfg::BN, Cfg::BK> lbB;
    lbB.init(gy + (int64_t)grp * g.Kg * g.OH * g.OW, g, q0, Q);
    f32x16 acc[Cfg::FM][Cfg::FN];
    igemm_mainloop<Cfg>(la, lbB, 0, (Kd + Cfg::BK - 1) / Cfg::BK, smem, acc);
    int64_t colbase[Cfg::FN];
    col_setup<Cfg>(colbase, [&](int j) -> int64_t {
        const int64_t q = q0 + j;
        if (q >= Q) return -1;
        const int n = (int)(q / hw), rem = (int)(q - (int64_t)n * hw);
        return (int64_t)n * g.C * hw + rem;
    });
    for_each_acc<Cfg>(acc, [&](int m, int j, int fn, float v) {
        const int ci = m0 + m;
        if (ci < g.Cg && colbase[fn] >= 0) gx[colbase[fn] + (int64_t)(grp * g.Cg + ci) * hw] = v;
    });
}

// split-K over output pixels; blockIdx.y = split, blockIdx.z = group; raw partials part[split][K][Cg*R*S]
template <class Cfg>
__global__ __launch_bounds__(256) void k_gw_wgrad(GGeom g, const float *__restrict__ x, const float *__restrict__ gy,
                                                  float *__restrict__ part, int tiles_m, int kt_per_split) {
    __shared__ float smem[Cfg::SMEM_FLOATS];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int grp = blockIdx.z;
    const int tm = lb % tiles_m, tn = lb / tiles_m;
    const int J = g.Cg * g.R * g.S;
    const int64_t P = (int64_t)g.N * g.OH * g.OW;
    const int nkt = (int)((P + Cfg::BK - 1) / Cfg::BK);
    const int m0 = tm * Cfg::BM, j0 = tn * Cfg::BN;
    GWgradALoader<Cfg::BM, Cfg::BK> la;
    la.init(gy + (int64_t)grp * g.Kg * g.OH * g.OW, g, m0);
    GWgradBLoader<Cfg::BN, Cfg::BK> lbB;
    lbB.init(x + (int64_t)grp * g.Cg * g.H * g.W, g, j0);
    f32x16 acc[Cfg::FM][Cfg::FN];
    const int kt0 = blockIdx.y * kt_per_split;
    const int kt1 = min(nkt, kt0 + kt_per_split);
    igemm_mainloop<Cfg>(la, lbB, kt0, kt1, smem, acc);
    float *dst = part + ((int64_t)blockIdx.y * g.K + (int64_t)grp * g.Kg) * J;
    for_each_acc<Cfg>(acc, [&](int m, int j, int, float v) {
        const int co = m0 + m, jj = j0 + j;
        if (co < g.Kg && jj < J) dst[(int64_t)co * J + jj] = v;
    });
}

using Cfg32 = TileCfg<32, 256, 16, 1, 4>;       // forward / input gradient: rows x pixels
using Cfg64 = TileCfg<64, 256, 16, 1, 4>;
using Cfg128 = TileCfg<128, 128, 16, 2, 2>;
using CfgW32 = TileCfg<32, 128, 16, 1, 4>;      // weight gradient: K/G rows x (ci, tap) columns
using CfgW64 = TileCfg<64, 128, 16, 2, 2>;

// rows of the output-channel tile for a group `width` channels wide: the least padding, the larger tile on a tie
inline int pick_rows(int width) {
    int best = 128, pad = (width + 127) / 128 * 128;
    if ((width + 63) / 64 * 64 < pad) { best = 64; pad = (width + 63) / 64 * 64; }
    if ((width + 31) / 32 * 32 < pad) best = 32;
    return best;
}

// the split-K plan of the generic weight gradient, with the groups counted among the tiles
inline void gw_wgrad_plan(const GGeom &g, int &bm, int &tm, int &tn, int &nsplit, int &per) {
    bm = pick_rows(g.Kg);
    tm = (g.Kg + bm - 1) / bm;
    tn = (g.Cg * g.R * g.S + 127) / 128;
    const int64_t P = (int64_t)g.N * g.OH * g.OW;
    const int nkt = (int)((P + 15) / 16);
    const int64_t tiles = (int64_t)tm * tn * g.G;
    int64_t want = (4 * kCUs + tiles - 1) / tiles;
    const int64_t max_by_k = (nkt + 7) / 8;
    if (want > max_by_k) want = max_by_k;
    if (want < 1) want = 1;
    if (want > 1024) want = 1024;
    per = (int)((nkt + want - 1) / want);
    nsplit = (nkt + per - 1) / per;
}

}  // namespace

// ================================================================================== host entry points (descriptor validated by the caller)
int cpg_conv_grouped_ok(const cpg_conv_desc *d) {
    return d != nullptr && d->groups > 1 && !opt_on(OPT_NO_GROUPED) ? 1 : 0;
}

int cpg_conv_grouped_fwd(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias, float *y,
                         hipStream_t stream) {
    const GGeom g = make_ggeom(d);
    if (!wide_groups(g)) {
        if (gd_blocks(g, false) > 0x7fffffffLL) return fail(CPG_E_INVALID, "cpg_conv2d_fwd(grouped): %lld blocks exceed the grid", (long long)gd_blocks(g, false));
        launch_gd<false>(g, x, w, pm, thr, bias, y, stream);
    } else {
        const int64_t P = (int64_t)g.N * g.OH * g.OW;
        const int bm = pick_rows(g.Kg), tm = (g.Kg + bm - 1) / bm;
        const int bn = bm == 128 ? 128 : 256;
        const dim3 grid((unsigned)(tm * ((P + bn - 1) / bn)), (unsigned)g.G);
        if (bm == 32) hipLaunchKernelGGL(k_gw_fwd<Cfg32>, grid, dim3(256), 0, stream, g, x, w, pm, thr, bias, y, tm);
        else if (bm == 64) hipLaunchKernelGGL(k_gw_fwd<Cfg64>, grid, dim3(256), 0, stream, g, x, w, pm, thr, bias, y, tm);
        else hipLaunchKernelGGL(k_gw_fwd<Cfg128>, grid, dim3(256), 0, stream, g, x, w, pm, thr, bias, y, tm);
    }
    CPG_CHECK_LAUNCH("cpg_conv2d_fwd(grouped)");
    return CPG_OK;
}

int cpg_conv_grouped_dgrad(const cpg_conv_desc *d, const float *gy, const float *w, const float *pm, float thr, float *gx,
                           hipStream_t stream) {
    const GGeom g = make_ggeom(d);
    if (!wide_groups(g)) {
        if (gd_blocks(g, true) > 0x7fffffffLL) return fail(CPG_E_INVALID, "cpg_conv2d_dgrad(grouped): %lld blocks exceed the grid", (long long)gd_blocks(g, true));
        launch_gd<true>(g, gy, w, pm, thr, nullptr, gx, stream);
    } else {
        const int64_t Q = (int64_t)g.N * g.H * g.W;
        const int bm = pick_rows(g.Cg), tm = (g.Cg + bm - 1) / bm;
        const int bn = bm == 128 ? 128 : 256;
        const dim3 grid((unsigned)(tm * ((Q + bn - 1) / bn)), (unsigned)g.G);
        if (bm == 32) hipLaunchKernelGGL(k_gw_dgrad<Cfg32>, grid, dim3(256), 0, stream, g, gy, w, pm, thr, gx, tm);
        else if (bm == 64) hipLaunchKernelGGL(k_gw_dgrad<Cfg64>, grid, dim3(256), 0, stream, g, gy, w, pm, thr, gx, tm);
        else hipLaunchKernelGGL(k_gw_dgrad<Cfg128>, grid, dim3(256), 0, stream, g, gy, w, pm, thr, gx, tm);
    }
    CPG_CHECK_LAUNCH("cpg_conv2d_dgrad(grouped)");
    return CPG_OK;
}

// narrow: slices * K * (C/G) * R * S floats (always); wide: nsplit * K * (C/G) * R * S floats
size_t cpg_conv_grouped_wgrad_workspace(const cpg_conv_desc *d) {
    const GGeom g = make_ggeom(d);
    const size_t out_bytes = (size_t)g.K * g.Cg * g.R * g.S * sizeof(float);
    if (!wide_groups(g)) {
        int slices, ips;
        gd_wgrad_plan(g, slices, ips);
        return (size_t)slices * out_bytes;
    }
    int bm, tm, tn, nsplit, per;
    gw_wgrad_plan(g, bm, tm, tn, nsplit, per);
    return (size_t)nsplit * out_bytes;
}

int cpg_conv_grouped_wgrad(const cpg_conv_desc *d, const float *x, const float *gy, const float *w, const float *pm, float thr, float *gw,
                           float *gpm, void *ws, size_t ws_bytes, hipStream_t stream) {
    const GGeom g = make_ggeom(d);
    const size_t need = cpg_conv_grouped_wgrad_workspace(d);
    if (ws == nullptr || ws_bytes < need) return fail(CPG_E_WORKSPACE, "cpg_conv2d_wgrad(grouped): workspace %zu < %zu bytes", ws_bytes, need);
    const int64_t out_elems = (int64_t)g.K * g.Cg * g.R * g.S;
    float *part = (float *)ws;
    int nparts;
    if (!wide_groups(g)) {
        int ips;
        gd_wgrad_plan(g, nparts, ips);
        const dim3 grid((unsigned)g.K, (unsigned)nparts);
        if (g.R == 3 && g.S == 3) hipLaunchKernelGGL(k_gd_wgrad<3>, grid, dim3(256), 0, stream, g, x, gy, part, ips);
        else if (g.R == 5 && g.S == 5) hipLaunchKernelGGL(k_gd_wgrad<5>, grid, dim3(256), 0, stream, g, x, gy, part, ips);
        else hipLaunchKernelGGL(k_gd_wgrad<0>, grid, dim3(256), 0, stream, g, x, gy, part, ips);
    } else {
        int bm, tm, tn, per;
        gw_wgrad_plan(g, bm, tm, tn, nparts, per);
        const dim3 grid((unsigned)(tm * tn), (unsigned)nparts, (unsigned)g.G);
        if (bm == 32) hipLaunchKernelGGL(k_gw_wgrad<CfgW32>, grid, dim3(256), 0, stream, g, x, gy, part, tm, per);
        else if (bm == 64) hipLaunchKernelGGL(k_gw_wgrad<CfgW64>, grid, dim3(256), 0, stream, g, x, gy, part, tm, per);
        else hipLaunchKernelGGL(k_gw_wgrad<Cfg128>, grid, dim3(256), 0, stream, g, x, gy, part, tm, per);
    }
    CPG_CHECK_LAUNCH("cpg_conv2d_wgrad(grouped)");
    const Epilogue ep{gw, nullptr, BIAS_NONE, 1, 1, pm, w, gpm, thr};
    launch_split_reduce(part, nparts, out_elems, 0, ep, stream);
    CPG_CHECK_LAUNCH("cpg_conv2d_wgrad(grouped reduce)");
    return CPG_OK;
}
