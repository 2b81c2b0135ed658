// Every function of libcpg_hip.so that one translation unit defines and another calls, declared ONCE (the C ABI itself is
// include/cpg_hip.h).  The defining file includes this header too, so a definition that drifts from its declaration is a compile
// error (extern "C") or a link error (mangled) instead of a call with its arguments in the wrong slots.  Default arguments live here only.
// Side arguments (cpg_common.h: what a public entry point took from the calling thread) are parameters like any other.  packed: the operand
// a launch may stream instead of packing (none: it packs; not this launch's: CPG_E_INVALID before a launch); families without one stream none.
// The extern "C" helpers are reachable in a CPG_EXPORT_ALL=1 build (tools/wino_bench.py, tools/wino_wgrad_bench.py); the normal
// build exports none of them.  Only the conv / linear translation units include this header: it pulls in igemm_core.h's kernels.
#pragma once
#include "igemm_core.h"

// ---- the inference epilogue: everything an inference forward does behind the conv, named once --------------------------------------------------
// BN_EVAL: y = [relu(] bn(conv + bias) [+ residual] [)] with an eval-mode BatchNorm2d (gamma, beta, mean, var: K floats each);
//          pool = 1: y = max over each 2x2 window of that (no residual), the pooled tensor alone is written.
// PRELU:   y = prelu(conv + bias) [+ residual]; slope: K floats, or one shared (per_channel = 0).
// residual (may be null): dense, shaped like y.  skip_stats (may be null): 2 device words that receive the dead-channel skip's
// {4 * (input chunks up to the last live one), output blocks skipped}: written by cpg_conv3x3_fwd_eval, the only class that skips;
// igemm_conv.hip's fwd_eval zeroes them behind the others.
// Built by igemm_conv.hip's public entry points, read by one cpg_*_eval entry per kernel family, each of which refuses what its kernels
// lack.  One place per file maps these names onto the kernels' parameter struct (c3_epilogue, wg_epilogue, cpg_conv1x1_fwd_eval's PwBn).
// what: the public entry point the caller used, for messages.
namespace cpg {
struct EvalEpilogue {
    enum Kind { BN_EVAL, PRELU } kind;
    const float *gamma, *beta, *mean, *var;     // BN_EVAL
    float eps;
    int relu;
    const float *slope;                         // PRELU
    int per_channel;
    const float *residual;
    int32_t *skip_stats;
    int pool;                                   // BN_EVAL: 1 = the MaxPool2d(2, 2) behind it too, y is [N][K][H/2][W/2]; 0 (and PRELU): none
};
}  // namespace cpg

// ---- conv3x3.hip: 3x3 / stride 1 / pad 1 -----------------------------------------------------------------------------------------------
// 1: the specialised 3x3 kernels take this shape (CPG_DISABLE_CONV3X3: never)
extern "C" int cpg_conv3x3_supported(const cpg_conv_desc *d);
// workspace of the forward / input gradient: packed weights of either direction + the Winograd filter + its tail pieces
size_t cpg_conv3x3_pack_workspace(const cpg_conv_desc *d);
int cpg_conv3x3_fwd(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias,
                    float *y, void *ws, size_t ws_bytes, hipStream_t stream, const cpg::PackedOperand &packed);
// forward that also writes stats[K][tiles][2], the per-(channel, pixel tile) BatchNorm partial sums; tiles = 0: not available.
// pool_max (may be null): receives the 2x2 window maxima of y; the caller has checked cpg_conv2d_fwd_pool_max_supported, no bias, its size
int cpg_conv3x3_bnstats_tiles(const cpg_conv_desc *d);
int cpg_conv3x3_fwd_bnstats(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias,
                            float *y, float *stats, void *ws, size_t ws_bytes, hipStream_t stream, const cpg::PackedOperand &packed, float *pool_max);
// 1: the inference epilogues have a launch for this shape under the current option table (the planner's answer; 0: the channel-split tile)
int cpg_conv3x3_eval_epilogue_ok(const cpg_conv_desc *d);
// 1: ... and the pooled one (ep.pool) too: that launch is a one- or two-wave Winograd kernel on an even map (the direct tiles have none)
int cpg_conv3x3_eval_pool_ok(const cpg_conv_desc *d);
// forward with ep folded into the epilogue, and the dead-channel skip.  Refused: BN_EVAL with a residual; PRELU where cpg_conv3x3_eval_epilogue_ok
// answers 0 (the channel-split tile); ep.pool where cpg_conv3x3_eval_pool_ok answers 0
int cpg_conv3x3_fwd_eval(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias,
                         const cpg::EvalEpilogue &ep, float *y, void *ws, size_t ws_bytes, hipStream_t stream, const char *what);
int cpg_conv3x3_dgrad(const cpg_conv_desc *d, const float *gy, const float *w, const float *pm, float thr, float *gx, void *ws,
                      size_t ws_bytes, hipStream_t stream, const cpg::PackedOperand &packed);
// the packed operand cpg_conv3x3_fwd / _fwd_bnstats (dgrad = 0) or cpg_conv3x3_dgrad streams and a caller may hand in (cpg_conv2d_use_packed);
// false: none (the pass runs a direct kernel, or a Winograd kernel that packs for itself)
bool cpg_conv3x3_pack_job(const cpg_conv_desc *d, int dgrad, cpg::PackJob *job);
// input gradient whose epilogue also does the BatchNorm-backward reduction of the layer below; tiles = 0: this shape has no such path
int cpg_conv3x3_dgrad_bnbwd_tiles(const cpg_conv_desc *d);
int cpg_conv3x3_dgrad_bnbwd(const cpg_conv_desc *d, const float *gy, const float *w, const float *pm, float thr, const float *ypre,
                            const float *gamma, const float *beta, const float *mean, const float *invstd, float *gx, float *partials,
                            void *ws, size_t ws_bytes, hipStream_t stream);
// weight gradient: Winograd (which alone takes a rider), the <= 3-channel stem kernel or k_c3_wgrad's 64-wide input-channel tile (4..15 channels: the generic kernel)
size_t cpg_conv3x3_wgrad_workspace(const cpg_conv_desc *d);
int cpg_conv3x3_wgrad(const cpg_conv_desc *d, const float *x, const float *gy, const float *w, const float *pm, float thr,
                      float *gw, float *gpm, void *ws, size_t ws_bytes, hipStream_t stream, const cpg::WgradRider &rider);

// ---- conv3x3.hip: 3x3 / stride 2 / pad 1, >= 16 channels on both sides (k_c3_fwd's strided tiles, k_c3s2_dgrad, k_c3_wgrad's strided units) ----
// 1: ... take this shape (CPG_DISABLE_CONV3X3, CPG_NO_S2: never)
extern "C" int cpg_conv3x3s2_supported(const cpg_conv_desc *d);
size_t cpg_conv3x3s2_pack_workspace(const cpg_conv_desc *d);
int cpg_conv3x3s2_bnstats_tiles(const cpg_conv_desc *d);
// stats (may be null): [K][tiles][2] BatchNorm partial sums
int cpg_conv3x3s2_fwd(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias, float *y,
                      float *stats, void *ws, size_t ws_bytes, hipStream_t stream);
// forward with ep folded into the epilogue.  Refused: a residual (a strided conv opens a stage), ep.pool.  The strided tiles skip nothing
int cpg_conv3x3s2_fwd_eval(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias,
                           const cpg::EvalEpilogue &ep, float *y, void *ws, size_t ws_bytes, hipStream_t stream, const char *what);
int cpg_conv3x3s2_dgrad(const cpg_conv_desc *d, const float *gy, const float *w, const float *pm, float thr, float *gx, void *ws,
                        size_t ws_bytes, hipStream_t stream);
size_t cpg_conv3x3s2_wgrad_workspace(const cpg_conv_desc *d);
int cpg_conv3x3s2_wgrad(const cpg_conv_desc *d, const float *x, const float *gy, const float *w, const float *pm, float thr, float *gw,
                        float *gpm, void *ws, size_t ws_bytes, hipStream_t stream);

// ---- conv3x3_wino.hip: Winograd F(2x2, 3x3) forward / input gradient.  c_read / m: channels contracted over / produced ----------------------
// Every query below reads the plan (wino_plan) of the launch cpg_conv3x3_wino_launch makes, from the shape and the option table alone.
// eligibility of one launch (CPG_NO_WINO: never; odd maps: the two-wave kernel's ODD instances only)
extern "C" int cpg_conv3x3_wino_ok(int N, int c_read, int m, int H, int W);
// bytes of the transformed filter at the head of the workspace
extern "C" size_t cpg_conv3x3_wino_pack_bytes(int c_read, int m);
// BatchNorm-statistics tiles per channel of a forward launch (stats[m][tiles][2])
extern "C" int cpg_conv3x3_wino_tiles(int N, int c_read, int m, int H, int W);
// workspace behind the packed filter for the partial outputs of a tail launch (0: this launch has none)
size_t cpg_conv3x3_wino_tail_bytes(int N, int c_read, int m, int H, int W);
// the packed operand of that launch; false: none a caller could hand in (a shape that is not eligible; the cooperative block kernel,
// which packs for itself)
bool cpg_conv3x3_wino_pack_job(int dgrad, int N, int c_read, int m, int H, int W, cpg::PackJob *job);
// 1: the launch can carry ... the 2x2 window maxima of a forward with statistics (the two-wave kernel on an even map, m a multiple of 64;
// CPG_NO_POOL_MAX: never); the inference epilogues (not the cooperative block kernel); the pooled one (ep.pool: ... of an even map);
// an addend to the input gradient (the two-wave kernel: >= 64 channels on both sides, or an odd map)
int cpg_conv3x3_wino_pool_max_ok(int N, int c_read, int m, int H, int W);
int cpg_conv3x3_wino_eval_ok(int N, int c_read, int m, int H, int W);
int cpg_conv3x3_wino_eval_pool_ok(int N, int c_read, int m, int H, int W);
int cpg_conv3x3_wino_dgrad_add_ok(int N, int c_read, int m, int H, int W);
// One launch: y[N][m][H][W] = conv3x3(x[N][c_read][H][W], W .* bin(pm)); dgrad: x = gy, the filter transposed and flipped.  Zero-initialise,
// then name what the call carries.  Refused before anything is launched: a null slope (CPG_E_INVALID), a residual behind the BatchNorm,
// ep.pool where cpg_conv3x3_wino_eval_pool_ok answers 0, an addend outside a plain input gradient (CPG_E_INVALID) or where
// cpg_conv3x3_wino_dgrad_add_ok answers 0, a shape cpg_conv3x3_wino_ok refuses.
namespace cpg {
struct WinoCall {
    int dgrad, N, c_read, m, H, W;
    int K, C;                         // the layer's weight w is [K][C][3][3]: (m, c_read), dgrad: (c_read, m)
    const float *x, *w, *pm;
    float thr;
    const float *bias;                // forward only, may be null
    const float *addend;              // plain input gradient only, may be null: gx = dgrad(gy) + addend
    float *pool_max;                  // forward with stats and no bias only, may be null: receives the 2x2 window maxima of y
    float *y, *stats;                 // stats (forward only, may be null): [m][tiles][2] partial sums for the BatchNorm
    const EvalEpilogue *ep;           // forward only, may be null: the inference epilogue (ep->pool: y is the pooled tensor), with the dead-channel skip:
    int *live;                        // ... its liveness words (may be null): live_words ints, zeroed here, layout of k_c3_pack
    size_t live_words;                //     (cpg_conv3x3_fwd_eval copies ep.skip_stats out of them)
    PackedOperand packed;             // launches without ep on the one- and two-wave kernels stream it; the others pack for themselves
    void *ws;                         // cpg_conv3x3_wino_pack_bytes + (for the tail pieces; without: the single launch) cpg_conv3x3_wino_tail_bytes
    size_t ws_bytes;
    hipStream_t stream;
    const char *what;                 // the public entry point the caller used, for messages
};
}  // namespace cpg
int cpg_conv3x3_wino_launch(const cpg::WinoCall &c);
// ... a plain forward (stats may be null) or input gradient, for tools/wino_bench.py
extern "C" int cpg_conv3x3_wino_run(int dgrad, int N, int c_read, int m, int H, int W, int K, int C, const float *x, const float *w,
                                    const float *pm, float thr, const float *bias, float *y, float *stats, void *ws, size_t ws_bytes,
                                    hipStream_t stream);

// ---- conv3x3_wino_wgrad.hip: Winograd F(2x2, 3x3) weight gradient (maps 14 or a multiple of 28 wide, channel counts multiples of 32) -------
extern "C" int cpg_conv3x3_wino_wgrad_ok(const cpg_conv_desc *d);
// 1: cpg_conv2d_wgrad of this shape takes a rider (cpg_conv2d_wgrad_attach_bn_bwd)
extern "C" int cpg_conv3x3_wino_wgrad_rider_ok(const cpg_conv_desc *d);
extern "C" size_t cpg_conv3x3_wino_wgrad_workspace(const cpg_conv_desc *d);
extern "C" int cpg_conv3x3_wino_wgrad(const cpg_conv_desc *d, const float *x, const float *gy, const float *w, const float *pm, float thr,
                                      float *gw, float *gpm, void *ws, size_t ws_bytes, hipStream_t stream);
// ... with the rider (none: the launch above); refused where cpg_conv3x3_wino_wgrad_rider_ok says 0
int cpg_conv3x3_wino_wgrad_side(const cpg_conv_desc *d, const float *x, const float *gy, const float *w, const float *pm, float thr,
                                float *gw, float *gpm, void *ws, size_t ws_bytes, hipStream_t stream, const cpg::WgradRider &rider);

// ---- conv3x3_stem.hip: the <= 3-channel 3x3 s1 p1 stem (one persistent wave per tile, weights in registers, HBM-bound) ---------------------
// 1: cpg_conv2d_fwd / cpg_conv2d_fwd_bnstats run this layer on the stem kernel (CPG_NO_STEM: never)
extern "C" int cpg_conv3x3_stem_ok(int N, int C, int K, int H, int W);
// BatchNorm-statistics tiles per channel (stats[K][tiles][2])
extern "C" int cpg_conv3x3_stem_tiles(int N, int C, int K, int H, int W);
extern "C" int cpg_conv3x3_stem_run(int N, int C, int K, int H, int W, const float *x, const float *w, const float *pm, float thr,
                                    const float *bias, float *y, float *stats, hipStream_t stream);

// ---- conv_stem_s2.hip: the strided image stems (7x7 s2 p3 and 3x3 s2 p1 from <= 3 channels to 64) -----------------------------------------
// 1: cpg_conv2d_fwd / cpg_conv2d_fwd_bnstats / cpg_conv2d_wgrad run this layer on the strided stem kernels (CPG_NO_STEM: never)
extern "C" int cpg_conv_stem2_ok(const cpg_conv_desc *d);
int cpg_conv_stem2_tiles(const cpg_conv_desc *d);
// stats (may be null): [K][tiles][2] BatchNorm partial sums
int cpg_conv_stem2_fwd(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias, float *y,
                       float *stats, hipStream_t stream);
size_t cpg_conv_stem2_wgrad_workspace(const cpg_conv_desc *d);
int cpg_conv_stem2_wgrad(const cpg_conv_desc *d, const float *x, const float *gy, const float *w, const float *pm, float thr, float *gw,
                         float *gpm, void *ws, size_t ws_bytes, hipStream_t stream);

// ---- conv_grouped.hip: groups > 1 (depthwise / narrow groups on direct VALU kernels, wide groups on the fp32-MFMA implicit GEMM) ---------------
// 1: descriptors with groups > 1 run the grouped kernels (CPG_NO_GROUPED: never -- such descriptors are then unsupported).  The entry points
// below take a descriptor the caller has validated (groups > 1 dividing C and K) and non-null tensors.
int cpg_conv_grouped_ok(const cpg_conv_desc *d);
int cpg_conv_grouped_fwd(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias, float *y,
                         hipStream_t stream);
int cpg_conv_grouped_dgrad(const cpg_conv_desc *d, const float *gy, const float *w, const float *pm, float thr, float *gx,
                           hipStream_t stream);
// the split partial sums of the weight gradient: [slices or splits][K][C/G][R][S] floats
size_t cpg_conv_grouped_wgrad_workspace(const cpg_conv_desc *d);
int cpg_conv_grouped_wgrad(const cpg_conv_desc *d, const float *x, const float *gy, const float *w, const float *pm, float thr, float *gw,
                           float *gpm, void *ws, size_t ws_bytes, hipStream_t stream);

// ---- pointwise.hip: 1x1 convolutions ----------------------------------------------------------------------------------------------------
// 1: the pointwise kernels take this shape's forward and input gradient (CPG_DISABLE_CONV1X1: never)
extern "C" int cpg_conv1x1_supported(const cpg_conv_desc *d);
size_t cpg_conv1x1_pack_workspace(const cpg_conv_desc *d);
// the packed operand of cpg_conv1x1_fwd (dgrad = 0) / cpg_conv1x1_dgrad
cpg::PackJob cpg_conv1x1_pack_job(const cpg_conv_desc *d, int dgrad);
// stats (may be null): [K][tiles][2] BatchNorm partial sums, tiles = cpg_conv1x1_bnstats_tiles(d)
int cpg_conv1x1_fwd(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias,
                    float *y, void *ws, size_t ws_bytes, hipStream_t stream, const cpg::PackedOperand &packed, float *stats = nullptr);
int cpg_conv1x1_bnstats_tiles(const cpg_conv_desc *d);
// forward with ep folded into the epilogue: BN_EVAL only (PRELU and ep.pool are refused), with or without a residual.  Nothing is skipped
int cpg_conv1x1_fwd_eval(const cpg_conv_desc *d, const float *x, const float *w, const float *pm, float thr, const float *bias,
                         const cpg::EvalEpilogue &ep, float *y, void *ws, size_t ws_bytes, hipStream_t stream, const cpg::PackedOperand &packed, const char *what);
// addend (may be null; stride 1 only): gx = dgrad(gy) + addend
int cpg_conv1x1_dgrad(const cpg_conv_desc *d, const float *gy, const float *w, const float *pm, float thr, float *gx, void *ws,
                      size_t ws_bytes, hipStream_t stream, const cpg::PackedOperand &packed, const float *addend = nullptr);
// dense pointwise layers whose activations can be staged as aligned float4 and addressed with 31-bit byte offsets
extern "C" int cpg_conv1x1_wgrad_supported(const cpg_conv_desc *d);
size_t cpg_conv1x1_wgrad_workspace(const cpg_conv_desc *d);
int cpg_conv1x1_wgrad(const cpg_conv_desc *d, const float *x, const float *gy, const float *w, const float *pm, float thr,
                      float *gw, float *gpm, void *ws, size_t ws_bytes, hipStream_t stream);

// ---- pointwise.hip: the same kernels as plain GEMMs (the linear layers) -------------------------------------------------------------------
// D[M][C] = A[M][K] . B[C][K]^T, both operands row-major and 16-byte aligned
bool cpg_pw_gemm_nt_ok(const float *A, const float *B, int M, int C, int64_t K);
size_t cpg_pw_gemm_nt_workspace(int M, int C, int64_t K);
int cpg_pw_gemm_nt(const float *A, const float *B, int M, int C, int64_t K, const cpg::Epilogue &ep, void *ws, size_t ws_bytes,
                   hipStream_t stream, const char *what);
// the same product with B masked in staging: D[M][C] = A[M][K] . (B * bin(pmB))[C][K]^T
int cpg_pw_gemm_nt_maskb(const float *A, const float *B, const float *pmB, float thr, int M, int C, int64_t K, const cpg::Epilogue &ep, void *ws,
                         size_t ws_bytes, hipStream_t stream, const char *what);
// masked: the launch that follows is cpg_pw_gemm_nn_masked / _maskx (their pixel tile differs)
bool cpg_pw_gemm_nn_ok(const float *X, int M, int Mp, int Kd, int64_t G, bool masked = false);
// y[M][G] (+ bias[m]) from K-major Wp (row stride Mp >= M, a multiple of 128; rows beyond Kd are never read)
int cpg_pw_gemm_nn(const float *wp, int Mp, const float *X, int M, int Kd, int64_t G, const float *bias, float *y, hipStream_t stream,
                   const char *what);
// the same GEMM with the autograd epilogue of bin(pm) * W: gw[M][G] = D * bin(pm), gpm[M][G] = D * w (pm, w, gpm laid out like gw)
int cpg_pw_gemm_nn_masked(const float *wp, int Mp, const float *X, int M, int Kd, int64_t G, const float *pm, const float *w, float thr,
                          float *gw, float *gpm, hipStream_t stream, const char *what);
// ... and with the operand X * bin(pmX) formed in staging
int cpg_pw_gemm_nn_maskx(const float *wp, int Mp, const float *X, const float *pmX, float thr, int M, int Kd, int64_t G, float *y,
                         hipStream_t stream, const char *what);
// K-major transpose of a row-major [R][Cc] matrix into wp[Cc (padded to 16)][R (padded to 128)]
void cpg_pw_pack_transpose(const float *a, int R, int Cc, float *wp, hipStream_t stream);
size_t cpg_pw_pack_transpose_bytes(int R, int Cc);

// ---- fc_small.hip: the weight-streaming input gradient of linear layers at <= 64 rows ------------------------------------------------------
bool cpg_fc_small_dgrad_ok(const float *w, const float *pm, const float *gx, int batch, int in_f, int out_f);
size_t cpg_fc_small_dgrad_workspace(int batch, int in_f, int out_f);
int cpg_fc_small_dgrad(const float *gy, const float *w, const float *pm, float thr, float *gx, int batch, int in_f, int out_f, void *ws,
                       size_t ws_bytes, hipStream_t stream, const char *what);
