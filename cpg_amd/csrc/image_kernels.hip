// The data path's two kernels (include/cpg_hip.h, "image batches"): the reference's torchvision / PIL transforms on a uint8 RGB
// image store that lives in HBM.
//
//  cpg_image_resample   : crop, then PIL's 8-bit BILINEAR resize (Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
//                         ImagingResampleHorizontal_8bpc / _Vertical_8bpc) -- bit-identical to
//                         PIL.Image.crop(box).resize((out_w, out_h), Image.BILINEAR), which is what RandomSizedCrop, Resize(int),
//                         Scale and CenterCrop-after-Scale compute on PIL images.
//  cpg_image_to_tensor  : window (zero-filled outside the image: RandomCrop's padding), horizontal flip, ToTensor, Normalize and
//                         Cutout in one pass; fp32 NCHW, element for element torchvision's CPU arithmetic.
//
// Item tables are HOST arrays.  Every item is validated on the host before anything is launched, then travels to the kernel by
// value in the launch arguments, kItemsMax per launch (cpg_sgd_route_step_multi's convention), so no kernel can address a byte the
// caller did not hand in and the table may be freed when the call returns.
#include <algorithm>

#include "cpg_common.h"

// The filter coefficients are formed in fp64 exactly as Resample.c forms them.  hipcc contracts a * b + c into an FMA by default;
// one fused multiply-add in `0.5 + k * 2^22` or in the tap position moves a truncation, hence a byte.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kItemsMax = 64;                   // 64 items of 48 bytes + the per-item workspace offsets: < 4 KB of launch arguments
constexpr int kPrecision = 22;                  // PRECISION_BITS = 32 - 8 - 2
constexpr int kMaxSide = 1 << 15;               // image, crop and output sides (int32 accumulators, exact fp64 centres)
constexpr int64_t kMaxWindowShift = 1 << 20;    // |y0|, |x0| of a to-tensor window

struct ResampleArgs {
    cpg_resample_item it[kItemsMax];
    int64_t tmp_off[kItemsMax];                 // horizontal-pass output of items that need both passes
    int count;
};
struct TensorArgs {
    cpg_tensor_item it[kItemsMax];
    int count;
};
static_assert(sizeof(ResampleArgs) + 64 <= 4096 && sizeof(TensorArgs) + 64 <= 4096, "kernel arguments are limited to 4 KB");

// One axis of PIL's precompute_coeffs for a box [0, in) resampled to `out` samples (the crop is taken first, so in0 = 0 and no
// tap ever reads outside the crop).
struct Axis {
    int in;
    double scale, support, ss;
};

__device__ __forceinline__ Axis make_axis(int in, int out) {
    Axis a;
    a.in = in;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 1.0 * fs;                       // bilinear: support 1
    a.ss = 1.0 / fs;
    return a;
}

__device__ __forceinline__ double bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// Taps of output sample o: [xmin, xmin + n).  The weights are recomputed on demand -- the first sweep sums them, the second
// normalises, converts to fixed point and accumulates -- so a 600-to-1 reduction needs no coefficient array.
struct Taps {
    double center, ww;
    int xmin, n;
};

__device__ __forceinline__ Taps make_taps(const Axis &a, int o) {
    Taps t;
    t.center = 0.0 + (o + 0.5) * a.scale;
    int xmin = (int)(t.center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(t.center + a.support + 0.5);
    if (xmax > a.in) xmax = a.in;
    t.xmin = xmin;
    t.n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < t.n; ++x) ww += bilinear((x + xmin - t.center + 0.5) * a.ss);
    t.ww = ww;
    return t;
}

__device__ __forceinline__ int tap_weight(const Axis &a, const Taps &t, int x) {
    double w = bilinear((x + t.xmin - t.center + 0.5) * a.ss);
    if (t.ww != 0.0) w /= t.ww;
    return w < 0 ? (int)(-0.5 + w * (1 << kPrecision)) : (int)(0.5 + w * (1 << kPrecision));
}

__device__ __forceinline__ uint8_t clip8(int v) {
    if (v >= (1 << kPrecision << 8)) return 255;
    if (v <= 0) return 0;
    return (uint8_t)(v >> kPrecision);
}

__device__ __forceinline__ bool need_h(const cpg_resample_item &r) { return r.out_w != r.crop_w; }
__device__ __forceinline__ bool need_v(const cpg_resample_item &r) { return r.out_h != r.crop_h; }

// Horizontal pass (ImagingResampleHorizontal_8bpc) over every row of the crop: into the workspace when a vertical pass follows,
// straight into the destination otherwise.
__global__ __launch_bounds__(kThreads) void k_image_resample_h(const ResampleArgs a, const uint8_t *__restrict__ src,
                                                               uint8_t *__restrict__ dst, uint8_t *__restrict__ tmp) {
    const cpg_resample_item &r = a.it[blockIdx.y];
    if (!need_h(r)) return;
    const Axis ax = make_axis(r.crop_w, r.out_w);
    const uint8_t *in = src + r.src_off + ((int64_t)r.crop_y * r.src_w + r.crop_x) * 3;
    uint8_t *out = need_v(r) ? tmp + a.tmp_off[blockIdx.y] : dst + r.dst_off;
    const int64_t total = (int64_t)r.crop_h * r.out_w;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < total; p += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(p / r.out_w), x = (int)(p - (int64_t)y * r.out_w);
        const Taps t = make_taps(ax, x);
        const uint8_t *row = in + (int64_t)y * r.src_w * 3 + (int64_t)t.xmin * 3;
        int s0 = 1 << (kPrecision - 1), s1 = s0, s2 = s0;
        for (int i = 0; i < t.n; ++i) {
            const int k = tap_weight(ax, t, i);
            s0 += row[i * 3 + 0] * k;
            s1 += row[i * 3 + 1] * k;
            s2 += row[i * 3 + 2] * k;
        }
        uint8_t *o = out + p * 3;
        o[0] = clip8(s0);
        o[1] = clip8(s1);
        o[2] = clip8(s2);
    }
}

// Vertical pass (ImagingResampleVertical_8bpc), from the horizontal pass's rows or from the crop itself; an item that keeps both
// sizes is copied (PIL: ImagingCopy).
__global__ __launch_bounds__(kThreads) void k_image_resample_v(const ResampleArgs a, const uint8_t *__restrict__ src,
                                                               uint8_t *__restrict__ dst, const uint8_t *__restrict__ tmp) {
    const cpg_resample_item &r = a.it[blockIdx.y];
    const bool h = need_h(r), v = need_v(r);
    if (h && !v) return;
    const uint8_t *in;
    int64_t pitch;                              // bytes per row of `in`
    if (h) {
        in = tmp + a.tmp_off[blockIdx.y];
        pitch = (int64_t)r.out_w * 3;
    } else {
        in = src + r.src_off + ((int64_t)r.crop_y * r.src_w + r.crop_x) * 3;
        pitch = (int64_t)r.src_w * 3;
    }
    uint8_t *out = dst + r.dst_off;
    const int64_t total = (int64_t)r.out_h * r.out_w;
    const Axis ax = make_axis(r.crop_h, r.out_h);
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < total; p += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(p / r.out_w), x = (int)(p - (int64_t)y * r.out_w);
        uint8_t *o = out + p * 3;
        if (!v) {
            const uint8_t *s = in + (int64_t)y * pitch + (int64_t)x * 3;
            o[0] = s[0];
            o[1] = s[1];
            o[2] = s[2];
            continue;
        }
        const Taps t = make_taps(ax, y);
        const uint8_t *col = in + (int64_t)t.xmin * pitch + (int64_t)x * 3;
        int s0 = 1 << (kPrecision - 1), s1 = s0, s2 = s0;
        for (int i = 0; i < t.n; ++i) {
            const int k = tap_weight(ax, t, i);
            const uint8_t *s = col + (int64_t)i * pitch;
            s0 += s[0] * k;
            s1 += s[1] * k;
            s2 += s[2] * k;
        }
        o[0] = clip8(s0);
        o[1] = clip8(s1);
        o[2] = clip8(s2);
    }
}

struct Norm {
    float mean[3], sd[3];
};

// ((float)u / 255 - mean) / std with IEEE divisions (torchvision ToTensor + Normalize on the CPU; a multiply by 1/255 differs in
// 126 of the 256 byte values), then `img *= mask` inside the Cutout rectangle: a multiply by 0.0f, so negative values become -0.0.
__device__ __forceinline__ float normalize(uint32_t u, float mean, float sd, bool cut) {
    const float v = ((float)u / 255.0f - mean) / sd;
    return cut ? v * 0.0f : v;
}

// One thread = 4 consecutive output columns of one row, all three channels: 12 gathered bytes in, three 16-byte stores out when
// the width is a multiple of 4 (rows then start 16-byte aligned), scalar stores otherwise.
__global__ __launch_bounds__(kThreads) void k_image_to_tensor(const TensorArgs a, const uint8_t *__restrict__ src, float *__restrict__ dst,
                                                              int out_h, int out_w, const Norm nm, int vec) {
    const cpg_tensor_item &t = a.it[blockIdx.y];
    const int groups = (out_w + 3) >> 2;
    const int64_t plane = (int64_t)out_h * out_w;
    float *out = dst + (int64_t)blockIdx.y * 3 * plane;
    const uint8_t *img = src + t.src_off;
    const int64_t total = (int64_t)out_h * groups;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < total; p += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(p / groups), x0 = (int)(p - (int64_t)y * groups) * 4;
        const int sy = t.y0 + y;
        const bool row_in = sy >= 0 && sy < t.src_h;
        const bool row_cut = y >= t.cut_y0 && y < t.cut_y1;
        float v[3][4];
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            const int wx = t.flip ? out_w - 1 - x : x;
            const int sx = t.x0 + wx;
            uint32_t r = 0, g = 0, b = 0;
            if (x < out_w && row_in && sx >= 0 && sx < t.src_w) {
                const uint8_t *s = img + ((int64_t)sy * t.src_w + sx) * 3;
                r = s[0], g = s[1], b = s[2];
            }
            const bool cut = row_cut && x >= t.cut_x0 && x < t.cut_x1;
            v[0][j] = normalize(r, nm.mean[0], nm.sd[0], cut);
            v[1][j] = normalize(g, nm.mean[1], nm.sd[1], cut);
            v[2][j] = normalize(b, nm.mean[2], nm.sd[2], cut);
        }
        const int64_t at = (int64_t)y * out_w + x0;
        if (vec) {
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4 *>(out + c * plane + at) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
            const int n = out_w - x0 < 4 ? out_w - x0 : 4;
            for (int c = 0; c < 3; ++c)
                for (int j = 0; j < n; ++j) out[c * plane + at + j] = v[c][j];
        }
    }
}

// grid.x: enough blocks for the largest item of the launch, at most 64 (grid-stride beyond); grid.y: one row per item
inline unsigned blocks_for(int64_t work) {
    const int64_t b = (work + kThreads - 1) / kThreads;
    return (unsigned)(b < 1 ? 1 : b > 64 ? 64 : b);
}

inline bool fits(int64_t off, int64_t bytes, int64_t limit) { return off >= 0 && bytes >= 0 && off <= limit && bytes <= limit - off; }

inline int64_t tmp_bytes(const cpg_resample_item &r) {
    return (r.out_w != r.crop_w && r.out_h != r.crop_h) ? ((int64_t)r.crop_h * r.out_w * 3 + 15) / 16 * 16 : 0;
}

int check_resample_item(const cpg_resample_item &r, int32_t i, int64_t src_bytes, int64_t dst_bytes) {
    CPG_REQUIRE(r.src_h >= 1 && r.src_w >= 1 && r.src_h <= kMaxSide && r.src_w <= kMaxSide,
                "cpg_image_resample: item %d: image size %d x %d outside [1, %d]", i, r.src_h, r.src_w, kMaxSide);
    CPG_REQUIRE(fits(r.src_off, (int64_t)r.src_h * r.src_w * 3, src_bytes),
                "cpg_image_resample: item %d: image at byte %lld (%d x %d x 3) is not inside the %lld-byte store", i, (long long)r.src_off,
                r.src_h, r.src_w, (long long)src_bytes);
    CPG_REQUIRE(r.crop_h >= 1 && r.crop_w >= 1 && r.crop_y >= 0 && r.crop_x >= 0 && r.crop_y <= r.src_h - r.crop_h &&
                    r.crop_x <= r.src_w - r.crop_w,
                "cpg_image_resample: item %d: crop (y %d, x %d, %d x %d) is not inside the %d x %d image", i, r.crop_y, r.crop_x, r.crop_h,
                r.crop_w, r.src_h, r.src_w);
    CPG_REQUIRE(r.out_h >= 1 && r.out_w >= 1 && r.out_h <= kMaxSide && r.out_w <= kMaxSide,
                "cpg_image_resample: item %d: output size %d x %d outside [1, %d]", i, r.out_h, r.out_w, kMaxSide);
    CPG_REQUIRE(fits(r.dst_off, (int64_t)r.out_h * r.out_w * 3, dst_bytes),
                "cpg_image_resample: item %d: destination at byte %lld (%d x %d x 3) is not inside the %lld-byte buffer", i,
                (long long)r.dst_off, r.out_h, r.out_w, (long long)dst_bytes);
    return CPG_OK;
}

int check_tensor_item(const cpg_tensor_item &t, int32_t i, int64_t src_bytes, int32_t out_h, int32_t out_w) {
    CPG_REQUIRE(t.src_h >= 1 && t.src_w >= 1 && t.src_h <= kMaxSide && t.src_w <= kMaxSide,
                "cpg_image_to_tensor: item %d: image size %d x %d outside [1, %d]", i, t.src_h, t.src_w, kMaxSide);
    CPG_REQUIRE(fits(t.src_off, (int64_t)t.src_h * t.src_w * 3, src_bytes),
                "cpg_image_to_tensor: item %d: image at byte %lld (%d x %d x 3) is not inside the %lld-byte store", i, (long long)t.src_off,
                t.src_h, t.src_w, (long long)src_bytes);
    CPG_REQUIRE(t.y0 > -kMaxWindowShift && t.y0 < kMaxWindowShift && t.x0 > -kMaxWindowShift && t.x0 < kMaxWindowShift,
                "cpg_image_to_tensor: item %d: window corner (%d, %d) out of range", i, t.y0, t.x0);
    CPG_REQUIRE(t.flip == 0 || t.flip == 1, "cpg_image_to_tensor: item %d: flip must be 0 or 1, got %d", i, t.flip);
    CPG_REQUIRE(t.cut_y0 >= 0 && t.cut_y1 <= out_h && t.cut_x0 >= 0 && t.cut_x1 <= out_w,
                "cpg_image_to_tensor: item %d: cutout [%d, %d) x [%d, %d) is not inside the %d x %d output", i, t.cut_y0, t.cut_y1, t.cut_x0,
                t.cut_x1, out_h, out_w);
    return CPG_OK;
}

}  // namespace

extern "C" size_t cpg_image_resample_workspace_bytes(const cpg_resample_item *items_host, int32_t n_items) {
    if (n_items <= 0 || !items_host) return 0;
    int64_t total = 0;
    for (int32_t i = 0; i < n_items; ++i) {
        const cpg_resample_item &r = items_host[i];
        if (r.crop_h < 1 || r.out_w < 1 || r.crop_h > kMaxSide || r.out_w > kMaxSide) continue;   // refused by the call itself
        total += tmp_bytes(r);
    }
    return (size_t)total;
}

extern "C" int cpg_image_resample(const uint8_t *src, int64_t src_bytes, const cpg_resample_item *items_host, int32_t n_items, uint8_t *dst,
                                  int64_t dst_bytes, void *ws, size_t ws_bytes, void *stream) {
    CPG_REQUIRE(n_items >= 0 && (n_items == 0 || items_host), "cpg_image_resample: null item table or negative count");
    if (n_items == 0) return CPG_OK;
    CPG_REQUIRE(src && dst && src_bytes > 0 && dst_bytes > 0, "cpg_image_resample: null source / destination or empty buffer");
    int64_t need = 0;
    for (int32_t i = 0; i < n_items; ++i) {
        const int rc = check_resample_item(items_host[i], i, src_bytes, dst_bytes);
        if (rc != CPG_OK) return rc;
        need += tmp_bytes(items_host[i]);
    }
    if (need > 0 && (!ws || (int64_t)ws_bytes < need))
        return cpg::fail(CPG_E_WORKSPACE, "cpg_image_resample: workspace of %zu bytes, %lld needed", ws_bytes, (long long)need);
    int64_t off = 0;
    for (int32_t at = 0; at < n_items;) {
        ResampleArgs a;
        a.count = 0;
        int64_t hwork = 0, vwork = 0;
        bool any_h = false;
        for (; at < n_items && a.count < kItemsMax; ++at) {
            const cpg_resample_item &r = items_host[at];
            const int i = a.count++;
            a.it[i] = r;
            a.tmp_off[i] = off;
            off += tmp_bytes(r);
            if (r.out_w != r.crop_w) {
                any_h = true;
                hwork = std::max(hwork, (int64_t)r.crop_h * r.out_w);
            }
            vwork = std::max(vwork, (int64_t)r.out_h * r.out_w);
        }
        uint8_t *tmp = (uint8_t *)ws;
        if (any_h) {
            hipLaunchKernelGGL(k_image_resample_h, dim3(blocks_for(hwork), a.count), dim3(kThreads), 0, (hipStream_t)stream, a, src, dst, tmp);
            CPG_CHECK_LAUNCH("cpg_image_resample (horizontal pass)");
        }
        hipLaunchKernelGGL(k_image_resample_v, dim3(blocks_for(vwork), a.count), dim3(kThreads), 0, (hipStream_t)stream, a, src, dst, tmp);
        CPG_CHECK_LAUNCH("cpg_image_resample (vertical pass)");
    }
    return CPG_OK;
}

extern "C" int cpg_image_to_tensor(const uint8_t *src, int64_t src_bytes, const cpg_tensor_item *items_host, int32_t n_items, int32_t out_h,
                                   int32_t out_w, const float *mean_host, const float *std_host, float *dst, int64_t dst_bytes, void *stream) {
    CPG_REQUIRE(n_items >= 0 && (n_items == 0 || items_host), "cpg_image_to_tensor: null item table or negative count");
    CPG_REQUIRE(out_h >= 1 && out_w >= 1 && out_h <= kMaxSide && out_w <= kMaxSide, "cpg_image_to_tensor: output size %d x %d outside [1, %d]",
                out_h, out_w, kMaxSide);
    CPG_REQUIRE(mean_host && std_host, "cpg_image_to_tensor: null mean / std");
    if (n_items == 0) return CPG_OK;
    CPG_REQUIRE(src && dst && src_bytes > 0, "cpg_image_to_tensor: null source / destination or empty store");
    const int64_t per = (int64_t)3 * out_h * out_w * (int64_t)sizeof(float);
    CPG_REQUIRE(dst_bytes >= 0 && n_items <= dst_bytes / per, "cpg_image_to_tensor: %d items of %lld bytes do not fit the %lld-byte destination",
                n_items, (long long)per, (long long)dst_bytes);
    for (int32_t i = 0; i < n_items; ++i) {
        const int rc = check_tensor_item(items_host[i], i, src_bytes, out_h, out_w);
        if (rc != CPG_OK) return rc;
    }
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        CPG_REQUIRE(std_host[c] != 0.0f, "cpg_image_to_tensor: std[%d] is zero", c);
        nm.mean[c] = mean_host[c];
        nm.sd[c] = std_host[c];
    }
    const int vec = (out_w % 4 == 0) && (((uintptr_t)dst) & 15) == 0;
    const unsigned bx = blocks_for((int64_t)out_h * ((out_w + 3) / 4));
    for (int32_t at = 0; at < n_items;) {
        TensorArgs a;
        a.count = 0;
        const int32_t first = at;
        for (; at < n_items && a.count < kItemsMax; ++at) a.it[a.count++] = items_host[at];
        hipLaunchKernelGGL(k_image_to_tensor, dim3(bx, a.count), dim3(kThreads), 0, (hipStream_t)stream, a, src,
                           dst + (int64_t)first * (per / (int64_t)sizeof(float)), out_h, out_w, nm, vec);
        CPG_CHECK_LAUNCH("cpg_image_to_tensor");
    }
    return CPG_OK;
}
