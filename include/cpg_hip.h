/*
 * cpg_hip.h -- C ABI of libcpg_hip.so, the MI355X (gfx950) implementation of the
 * ivclab/CPG masked-CNN train / prune / retrain hot path.
 *
 * The reference has no FFI layer: its boundary is the Python class contract of
 * models/layers.py + utils/prune.py.  Every entry point below
 * replaces one stock-PyTorch call sequence of the reference and cites it; the
 * reference-side binding (a ctypes stub inside SharableConv2d / SharableLinear /
 * SparsePruner) is shown in INTEGRATION.md, and cpg_amd/_lib.py is that binding.
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HBM) unless named *_host.  The caller (PyTorch)
 *     owns every buffer; kernels borrow them for the duration of the call.
 *   - `stream` is a hipStream_t passed as void*; work is enqueued there and the call
 *     returns without synchronising.  No global mutable state: the library is re-entrant
 *     and may be called concurrently from several host threads on different streams.
 *   - Tensors are dense, contiguous fp32 (NCHW activations, [Cout][Cin/g][R][S] conv
 *     weights, [out][in] linear weights) and uint8 owner ids shaped like the weight
 *     (reference: torch.ByteTensor masks, CPG_cifar100_main_normal.py:204).
 *   - Element-wise entry points accept n == 0 (and then NULL data pointers, as an empty
 *     tensor has no storage) and return CPG_OK without launching anything.
 *   - `pm` is the real-valued piggymask (same shape as the weight) or NULL (task 1,
 *     CPG_cifar100_main_normal.py:263-270).  When non-NULL the effective weight is
 *     W * (pm > thr ? 1 : 0) -- models/layers.py:11-23,99-105.  The linear and generic conv kernels
 *     form it inside their LDS staging pass (never materialised); the 3x3 s1 p1 conv kernels stream it
 *     from a K-major packed copy produced by a fused binarise+mask+transpose pass into the call's
 *     workspace (conv weights are <= 9.4 MB per layer; the 411 MB linear weights are never copied).
 *   - Return value: 0 ok; <0 invalid argument / unsupported; CPG_E_KRANGE is rank-prune's
 *     "not enough weights" (reference: sys.exit(2), utils/prune.py:38-42);
 *     >= CPG_E_HIP_BASE is CPG_E_HIP_BASE + hipError_t.
 *   - Workspaces: query with the *_workspace_bytes function, pass any buffer at least
 *     that large (contents undefined on entry and exit).
 */
#ifndef CPG_HIP_H
#define CPG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPG_ABI_VERSION 3

#define CPG_OK 0
#define CPG_E_INVALID (-1)
#define CPG_E_UNSUPPORTED (-2)
#define CPG_E_WORKSPACE (-3)
#define CPG_E_KRANGE 2
#define CPG_E_HIP_BASE 1000

/* gradient-routing modes (args.mode of utils/prune.py:206-210) */
#define CPG_MODE_FINETUNE 0
#define CPG_MODE_PRUNE 1

/* geometry of one SharableConv2d call (models/layers.py:46-49,108-109) */
typedef struct cpg_conv_desc {
    int32_t N, C, H, W;       /* input  NCHW                                  */
    int32_t K;                /* out_channels                                 */
    int32_t R, S;             /* kernel_size                                  */
    int32_t stride_h, stride_w;
    int32_t pad_h, pad_w;
    int32_t dil_h, dil_w;
    int32_t groups;           /* >= 1, divides C and K; w is [K][C/groups][R][S] */
} cpg_conv_desc;

/* result record of cpg_rank_prune, written to DEVICE memory (one per call) */
typedef struct cpg_prune_result {
    int64_t n_candidates;     /* #(owner == cur || owner == 0)                */
    int64_t k;                /* round-half-even(ratio * n_candidates)        */
    int64_t n_released;       /* #slots whose owner went cur -> 0             */
    float cutoff;             /* k-th smallest |w| among the candidates       */
    int32_t status;           /* CPG_OK or CPG_E_KRANGE (owner left untouched)*/
} cpg_prune_result;

int cpg_version(void);
/* PROCESS-wide scheduling hint (an atomic; default 0): 1 = other streams' kernels share the chip with this process's launches
 * (a data-parallel run: RCCL's all-reduce kernels hold some CUs during the backward pass).  Only changes scheduling and the
 * summation order of split partial sums.  Since round 4 ONE planner reads it: the Winograd weight gradient runs 2 rounds of half-length
 * units per wave slot instead of 1 (a launch that finds CUs taken then grows by half a round instead of a whole one); the pointwise and
 * direct 3x3 weight-gradient planners ignore it (beside RCCL's real kernels their finer splits cost more than they saved).  It changes
 * the workspace a weight-gradient call needs, and it is PROCESS-wide (the planners run inside autograd's backward, on the engine's
 * worker thread, not on the thread that set it): set it once, before the first workspace query, and do not change it while ANY thread
 * is between a workspace query and the launch it sized -- a launch whose plan outgrew its workspace fails with CPG_E_WORKSPACE, it
 * never overruns.  cpg_amd.dist.DataParallel raises it only for >= 256 MB of gradients per step (VGG16).  Replaces nn.DataParallel's
 * implicit "all GPUs are mine" (CPG_cifar100_main_normal.py:199-200). */
int cpg_set_shared_chip_hint(int32_t shared);
int32_t cpg_get_shared_chip_hint(void);
/* Library options.  Every CPG_* switch of the dispatch code (INTEGRATION.md lists them) lives in one process-wide table that is
 * filled from the environment ONCE, when the library is loaded; no launch path calls getenv().  After loading, the table changes
 * only through these two calls.  `name` is the switch's documented name ("CPG_NO_WINO", "CPG_WW_UNITS", ...); `value`: boolean
 * switches 0 / 1, integer switches their number, CPG_WINO_KERNEL 0 = block, 1 = wave, 2 = pair, 3 = 64; CPG_OPT_UNSET = "never
 * given" (the built-in default applies).  The policy switches -- the only ones an integrator should touch -- choose the arithmetic
 * of the 3x3 convolutions: CPG_NO_WINO (direct fp32 MFMA instead of Winograd F(2x2,3x3) in all three passes), CPG_NO_WINO_WGRAD,
 * CPG_NO_WINO_ODD, CPG_NO_STEM, CPG_NO_STEM_FUSE, CPG_NO_DEAD_SKIP; everything else is A/B tooling.  Unknown name: CPG_E_INVALID.
 * There is no counterpart in the reference: F.conv2d takes whichever algorithm cuDNN / MIOpen selects (models/layers.py:106-109).
 *
 * WHICH SWITCHES CHANGE RESULTS.  Every path computes the same fp32 convolution / GEMM; what a switch can change is the rounding
 * (always inside the 1e-4 parity bar, every combination is covered by tests/test_hip_parity.py):
 *   arithmetic (Winograd transforms vs direct taps: differences of 1e-6 of the output scale):
 *       CPG_NO_WINO, CPG_NO_WINO_WGRAD, CPG_NO_WINO_ODD, CPG_DISABLE_CONV3X3, CPG_C3_FORCE (tile shape of the direct kernel = its
 *       channel-split accumulation), CPG_NO_S2, CPG_NO_V14, CPG_W3_PICK, CPG_DISABLE_CONV1X1, CPG_DISABLE_CONV1X1_WGRAD,
 *       CPG_DISABLE_PW_GEMM, CPG_NO_STEM (stem kernel vs general kernel: other k order of the 27 taps),
 *       CPG_NO_GROUPED (groups > 1: the library reports the descriptor as unsupported and the caller runs one groups == 1 launch
 *       per group: another kernel family per group = another summation order), CPG_GROUPED_WIDE_MIN (direct vs MFMA kernels);
 *   summation order only (how a reduction over pixels / tiles / channel blocks is split and added: last-bit differences, mostly in
 *   weight gradients and BatchNorm statistics):
 *       CPG_WW_UNITS, CPG_WW_SHARE, CPG_C3W_BPC, CPG_PWW_BPC, CPG_PW_TILE, CPG_WINO_KERNEL, CPG_WINO_NW, CPG_STEM_BLOCKS, CPG_WINO_TAIL,
 *       CPG_FC_SMALL (linear layers at <= 64 rows: which kernel streams the weight = how the contraction is split),
 *       CPG_NO_STEM_FUSE (fused stem recomputes y instead of reading it back: same bits where the summation order is the same),
 *       and cpg_set_shared_chip_hint (above);
 *   no effect on any result bit (scheduling / mapping of the same work):
 *       CPG_WINO_PERSIST, CPG_WINO_GRIDS, CPG_WW_XCD, CPG_WG3_SHARE, CPG_NO_DEAD_SKIP (skips work whose inputs are exactly zero),
 *       CPG_NO_WW_RIDER (the BatchNorm backward apply as a pass of its own instead of inside the next weight gradient).
 *   CPG_NO_POOL_MAX (cpg_conv2d_fwd_pool_max_supported answers 0: the pooled BatchNorm passes read the conv output, not its window
 *       maxima): no effect on the forward as numbers or on dbeta; dgamma / gx may move by an ulp of one term where two different values
 *       of a window round to the same BatchNorm output.
 * A run is bit-reproducible for a fixed set of switch values and a fixed hint; the defaults are what every committed number used.
 * The table is global state, but not per-call mutable state: no entry point writes it, and a concurrent cpg_set_option only ever
 * changes which of the above equivalent plans a LATER call picks (the workspace caveat of the hint applies to CPG_WW_UNITS,
 * CPG_C3W_BPC, CPG_PWW_BPC, CPG_PW_TILE, CPG_WINO_TAIL and CPG_FC_SMALL as well: a switch that sizes a workspace must not change
 * between the *_workspace_bytes query and the call it sized -- the Winograd tail falls back to one launch on a workspace that is too
 * small, the <= 64-row linear kernels return CPG_E_WORKSPACE). */
#define CPG_OPT_UNSET INT32_MIN
int cpg_set_option(const char *name, int32_t value);
int cpg_get_option(const char *name, int32_t *value);
/* human-readable text for the last non-zero status returned on THIS thread */
const char *cpg_last_error(void);

/* ---- K1: models/layers.py:11-23 + :103 / :190 (Binarizer + elementwise product) ----
 * w_eff[i] = w[i] * (pm[i] > thr ? 1 : pm[i] <= thr ? 0 : pm[i]); w == NULL gives the bare Binarizer
 * output.  Exported for callers that need W_eff itself (tests, checkpoint export); the conv/linear
 * kernels fuse this step. */
int cpg_binarize_mask_weight(const float *w, const float *pm, float thr, float *w_eff,
                             int64_t n, void *stream);

/* ---- K2/K3/K4: F.conv2d of models/layers.py:108-109 and its autograd ----
 * fwd   : y  = conv2d(x, W_eff, bias)                       bias may be NULL
 * dgrad : gx = conv2d_input_grad(gy, W_eff)
 * wgrad : gW_eff = conv2d_weight_grad(x, gy); then, as autograd of `bin(pm) * W`
 *         (models/layers.py:103): gw = gW_eff * bin(pm), gpm = gW_eff * W (gpm NULL when pm
 *         is NULL).  gb (may be NULL) = sum of gy over N,H,W.
 *         gw / gpm / gb are OVERWRITTEN (caller accumulates if it needs to).
 * groups > 1 (desc->groups divides C and K, else CPG_E_INVALID): w, pm, gw and gpm are [K][C/groups][R][S]; group g reads input
 *         channels [g C/groups, (g+1) C/groups) and writes output channels [g K/groups, (g+1) K/groups).  All groups of a pass run
 *         in one launch on the NCHW tensors in place (direct kernels for narrow groups, fp32 MFMA from 16 channels per group on both
 *         sides); the weight gradient sums split partials from the workspace in a fixed order (no atomics: bit-reproducible).  Such
 *         descriptors have no packed operand, no fused BatchNorm statistics / inference epilogue, no addend, no rider: the queries
 *         below answer 0 and cpg_conv2d_fwd_bnstats returns CPG_E_UNSUPPORTED.  With CPG_NO_GROUPED set every entry point reports
 *         them as CPG_E_UNSUPPORTED (workspace 0).  Measured (profiles/grouped_conv.md, batch 256): faster in every pass than one
 *         groups == 1 call per group on channel slices, EXCEPT from 16 channels per group for 3x3 / stride 1 / pad 1 layers (forward
 *         and input gradient 1.2 - 3 x slower: per group those run the Winograd kernels) and for strided layers (input gradient
 *         2.5 - 4.6 x slower).  The library does not reroute these; a caller with such layers is better served by per-group calls,
 *         as cpg_amd's SharableConv2d does.
 * Every entry point validates the descriptor first, then the pointers (NULL: CPG_E_INVALID), then launches.
 * Alignment, the general rule (the entries below state it only where they ask for more):
 *   - ELEMENT alignment (4 bytes) is all the tensors of cpg_conv2d_fwd / _fwd_bnstats / _dgrad / _wgrad and of cpg_linear_fwd /
 *     _dgrad / _wgrad need: x, w, pm, bias, y, gy, gx, gw, gpm, gb and the statistics buffer.  A batch slice of a tensor whose rows
 *     are an odd number of floats long is a legal argument.  The kernels that can use 16-byte accesses (pointwise, grouped, the bias
 *     gradient, the small-batch and GEMM-shaped linear kernels) test the pointer and the row length per call and take their
 *     per-element flavour otherwise: the same contraction, the fp32 sums possibly in another order.  The Winograd, direct 3x3,
 *     3x3 s2, stem and generic implicit-GEMM kernels test nothing and need nothing: the same bits on any element-aligned pointer.
 *   - 16 BYTES are required, and checked, of `workspace` by every conv launch that uses it (CPG_E_INVALID; the linear
 *     entry points take a kernel that needs no workspace instead), of the packed operands of cpg_conv2d_pack /
 *     cpg_conv2d_use_packed, and of the four pointers of cpg_conv2d_wgrad_attach_bn_bwd.  One tensor among the first group can
 *     ask for them: x of cpg_conv2d_fwd_bnstats on a pointwise layer under the wide tile (CPG_PW_TILE=1, A/B tooling, not the
 *     default), whose statistics buffer is sized for that tile -- CPG_E_INVALID otherwise, nothing launched.
 *   - Not covered by this rule: the residual / addend of the fused epilogues (cpg_conv2d_dgrad_add, _fwd_bn_eval_add,
 *     _fwd_prelu_eval) and the BatchNorm, PReLU and loss-head entry points; pass those 16-byte aligned tensors.
 *   tests/test_conv_descriptor_space_gpu.py runs the first group one and three floats off alignment: the inputs (x, gy, w, pm, bias)
 *   through the layers, the outputs (y, the statistics buffer, gx, gw, gpm, gb) through direct calls of the conv entry points and of
 *   cpg_linear_dgrad.  Not run there, so a promise from reading the code alone: y of cpg_linear_fwd and gw / gpm / gb of
 *   cpg_linear_wgrad off alignment, and the linear layers' GEMM routes that need >= 192 output tiles. */
size_t cpg_conv2d_workspace_bytes(const cpg_conv_desc *d);
int cpg_conv2d_fwd(const cpg_conv_desc *d, const float *x, const float *w, const float *pm,
                   float thr, const float *bias, float *y, void *ws, size_t ws_bytes, void *stream);
int cpg_conv2d_dgrad(const cpg_conv_desc *d, const float *gy, const float *w, const float *pm,
                     float thr, float *gx, void *ws, size_t ws_bytes, void *stream);
/* Input gradient with the gradient of the input's OTHER consumer added in the epilogue: gx = dgrad(gy) + addend.  A residual block's
 * input feeds conv1 and the identity branch (models/resnet.py:84-104; models/spherenet.py:121-131: x + relu(conv(relu(conv(x))))); autograd
 * would sum the two gradients in a separate 3-pass kernel.  Dense 1x1 layers, and (round 5) the 3x3 s1 p1 layers whose input gradient
 * runs the two-wave Winograd kernel (>= 64 channels on both sides, or a 7 x 7 map): cpg_conv2d_dgrad_add_supported; addend is shaped
 * like gx and may not alias it. */
int32_t cpg_conv2d_dgrad_add_supported(const cpg_conv_desc *desc);
int cpg_conv2d_dgrad_add(const cpg_conv_desc *desc, const float *gy, const float *w, const float *piggymask, float threshold,
                         const float *addend, float *gx, void *workspace, size_t workspace_bytes, void *stream);
int cpg_conv2d_wgrad(const cpg_conv_desc *d, const float *x, const float *gy, const float *w,
                     const float *pm, float thr, float *gw, float *gpm, float *gb,
                     void *ws, size_t ws_bytes, void *stream);

/* Caller-owned packed weight operands (ABI version 3; SURVEY.md section 8b "an explicit, re-creatable cache (packed keep-bits / W_eff)").
 * The pointwise kernels and the one- / two-wave Winograd kernels stream W_eff = W * bin(pm) from a packed copy (K-major, resp. the
 * transformed filter in per-lane order) that every cpg_conv2d_fwd / _dgrad call otherwise produces into its own workspace first -- one
 * small launch per call, 109 per ResNet-50 step.  With these three calls the caller produces the operands ONCE per weight state -- the
 * forward's and the input gradient's of a layer in ONE launch -- and hands them to the calls that stream them:
 *   cpg_conv2d_pack_bytes(desc, pass): size of the operand of pass 0 (cpg_conv2d_fwd), 1 (cpg_conv2d_dgrad / _dgrad_add) or
 *       2 (cpg_conv2d_fwd_bnstats); 0 = a call of this shape streams no packed operand (it needs no cache).
 *   cpg_conv2d_pack(desc, w, pm, thr, pass_a, packed_a, bytes_a, pass_b, packed_b, bytes_b, stream): packs for one or (packed_b
 *       != NULL) two passes in one launch; bytes_* must equal cpg_conv2d_pack_bytes.  The buffers are the caller's; they are valid
 *       for as long as w, pm, thr, the shape in `desc` and the library options do not change (key them on the tensors' versions).
 *   cpg_conv2d_use_packed(packed, bytes): arms THE CALLING THREAD -- the next cpg_conv2d_fwd / _fwd_bnstats / _dgrad / _dgrad_add /
 *       _dgrad_bnbwd call on this thread streams `packed` instead of packing w / pm (which it still takes: a launch of another kernel
 *       family ignores the operand and packs for itself).  One-shot: that call disarms the thread whether it used the operand or
 *       not; a size that does not match what the launch streams is CPG_E_INVALID.  NULL disarms.
 * cpg_conv2d_pack_bytes, cpg_conv2d_pack and the *_tiles / *_supported queries read no thread state and write none: they answer from the
 * descriptor and the library options alone, launch nothing (the queries) and leave an armed operand armed.
 * Results are bit-equal to the self-packing calls.  Reference: the `W_eff` the reference materialises in every forward
 * (models/layers.py:99-105) and autograd keeps for the backward. */
size_t cpg_conv2d_pack_bytes(const cpg_conv_desc *desc, int32_t pass);
int cpg_conv2d_pack(const cpg_conv_desc *desc, const float *w, const float *piggymask, float threshold, int32_t pass_a, void *packed_a,
                    size_t bytes_a, int32_t pass_b, void *packed_b, size_t bytes_b, void *stream);
int cpg_conv2d_use_packed(const void *packed, size_t bytes);

/* The apply pass of a BatchNorm -> ReLU backward as a SIDE JOB of the next layer's weight gradient (compatible addition: the ABI version
 * stays 3).  The Winograd weight-gradient kernel of the wide layers is bound by its MFMA issue and leaves most of the HBM idle; the
 * backward of conv l launches its input gradient first -- that is gz, the gradient reaching relu(bn(y)) of layer l - 1 -- and its weight
 * gradient, which needs neither that BatchNorm's backward nor its result, second.  So the elementwise pass gy = bn_bwd(y, gz) of layer
 * l - 1 (2 reads + 1 write, otherwise a kernel of its own) runs inside wgrad_l's main loop, every element once, its loads requested four
 * k-steps ahead:
 *   cpg_bn_relu_bwd_reduce(...): the reduce + finalize launches of cpg_bn_relu_bwd(relu = 1, train = 1) alone: dgamma, dbeta, and
 *       table[C][8] = {mean, invstd, gamma, beta, mean(g), mean(g xhat), invstd * gamma, 0} (16-byte aligned) for the rider.
 *   cpg_conv2d_wgrad_rider_supported(desc): 1 = cpg_conv2d_wgrad of this shape takes a rider: fp32 math on the Winograd kernel with the
 *       four waves of a block sharing their input rows (>= 4 output-channel blocks, a multiple of 4), CPG_NO_WW_RIDER unset.
 *   cpg_conv2d_wgrad_attach_bn_bwd(y, gz, gy, table, N, C, HW): arms THE CALLING THREAD -- the next cpg_conv2d_wgrad on it also writes
 *       gy[N][C][HW] (4 | HW, below 2 GiB, all pointers 16-byte aligned, gy aliasing nothing).  One-shot: that call disarms the thread;
 *       when its launch cannot carry the rider it fails with CPG_E_UNSUPPORTED before launching anything.  y == NULL disarms.
 * gy is bit-equal to cpg_bn_relu_bwd's wherever it is a number, signed zeros and infinities included (one shared device function); where it
 * is a NaN the other is a NaN too, but the NaN's sign and payload may differ (the two kernels compile the expression into different
 * instruction sequences, a packed fma against a subtract).  The weight gradient is bit-equal to the call without a rider.
 * DECISION on the version number: these three entries and CPG_NO_WW_RIDER were added WITHOUT raising CPG_ABI_VERSION (no existing
 * signature or behaviour changes, and the version is pinned at 3 by the binding and its tests); cpg_version() therefore does not tell a
 * caller whether they exist -- probe for them with dlsym("cpg_conv2d_wgrad_rider_supported"). */
int cpg_bn_relu_bwd_reduce(const float *x, const float *gz, const float *gamma, const float *beta, const float *mean, const float *invstd,
                           float *dgamma, float *dbeta, float *table, int32_t N, int32_t C, int32_t HW, void *workspace,
                           size_t workspace_bytes, void *stream);
int32_t cpg_conv2d_wgrad_rider_supported(const cpg_conv_desc *desc);
int cpg_conv2d_wgrad_attach_bn_bwd(const float *y, const float *gz, float *gy, const float *table, int32_t N, int32_t C, int32_t HW);

/* The 2x2 window maxima of a conv output from the conv kernel's own epilogue, for the BatchNorm2d -> ReLU -> MaxPool2d(2, 2) group that
 * follows (compatible addition: the ABI version stays 3; probe with dlsym("cpg_conv2d_fwd_pool_max_supported")).  An output tile of the
 * Winograd F(2x2, 3x3) forward IS a pool window, and for a channel with gamma > 0 the pooled output and the backward reduction are
 * functions of the window's maximum E = max(y00, y01, y10, y11) of the raw conv output alone (the BatchNorm affine map is monotone).
 *   cpg_conv2d_fwd_pool_max_supported(desc): 1 = cpg_conv2d_fwd_bnstats of this shape (called WITHOUT a bias) can also write
 *       E[N][K][H/2][W/2]: the two-wave Winograd kernel with the statistics epilogue, H and W even, K a multiple of 64,
 *       CPG_NO_POOL_MAX unset.  Everything else (the one-wave and direct kernels, odd maps, other widths) answers 0.
 *   cpg_conv2d_fwd_attach_pool_max(E, bytes): arms THE CALLING THREAD -- the next cpg_conv2d_fwd_bnstats on it also writes E (bytes >=
 *       N K (H/2) (W/2) floats).  One-shot: that call disarms the thread when it returns, whatever its status; a shape the query refuses,
 *       a bias or a short buffer is CPG_E_INVALID before anything is launched.  E == NULL disarms.
 * y and the statistics are bit-equal to the call without E; E is exactly the maximum over each window of that y. */
int32_t cpg_conv2d_fwd_pool_max_supported(const cpg_conv_desc *desc);
int cpg_conv2d_fwd_attach_pool_max(float *E, size_t bytes);

/* ---- K5: F.linear of models/layers.py:194 and its autograd ----
 * x [batch][in], w [out][in], y [batch][out]; same masking / gradient rules as conv. */
size_t cpg_linear_workspace_bytes(int32_t batch, int32_t in_features, int32_t out_features);
int cpg_linear_fwd(const float *x, const float *w, const float *pm, float thr, const float *bias,
                   float *y, int32_t batch, int32_t in_features, int32_t out_features,
                   void *ws, size_t ws_bytes, void *stream);
int cpg_linear_dgrad(const float *gy, const float *w, const float *pm, float thr, float *gx,
                     int32_t batch, int32_t in_features, int32_t out_features,
                     void *ws, size_t ws_bytes, void *stream);
int cpg_linear_wgrad(const float *x, const float *gy, const float *w, const float *pm, float thr,
                     float *gw, float *gpm, float *gb, int32_t batch, int32_t in_features,
                     int32_t out_features, void *ws, size_t ws_bytes, void *stream);

/* ---- K4e: utils/prune.py:195-211 (do_weight_decay_and_make_grads_zero), one layer ----
 * gw = (owner == cur) ? gw + wd * w : 0.   gpm (may be NULL): FINETUNE -> 0 where owner == 0 or
 * owner >= cur; PRUNE -> 0 everywhere.  One pass, in place. */
int cpg_route_grads(float *gw, const float *w, const uint8_t *owner, int32_t cur, float wd,
                    float *gpm, int32_t mode, int64_t n, void *stream);

/* ---- K6: utils/prune.py:30-53 (_pruning_mask), one layer, fully on device ----
 * candidates = owner in {cur, 0}; k = round-half-even(ratio * n_cand) in fp64 (python round());
 * cutoff = k-th smallest |w| over the candidates (radix select on the fp32 bit pattern);
 * owner[(|w| <= cutoff) & (owner == cur)] = 0.  k < 1 or k > n_cand -> status CPG_E_KRANGE in
 * *result and owner untouched.  `result` is a device pointer; nothing is synchronised. */
size_t cpg_rank_prune_workspace_bytes(void);
int cpg_rank_prune(const float *w, uint8_t *owner, int32_t cur, double ratio, int64_t n,
                   cpg_prune_result *result, void *ws, size_t ws_bytes, void *stream);
/* The PackNet prunes (utils/packnet_prune.py:64-99, one_shot_prune / gradually_prune): cpg_rank_prune's three select passes unchanged, and a
 * final pass that releases owners AND writes +0.0f to w at every slot whose owner is 0 after the update, newly released or not
 * (`module.weight.data[mask.eq(0)] = 0.0`, :77 and :98) -- bit-equal to cpg_rank_prune followed by cpg_zero_pruned, without the second
 * pass over w.  Same result record, same workspace query.  On CPG_E_KRANGE neither owner nor w is touched.  Callers probe for the symbol
 * (CPG_ABI_VERSION stays 3). */
int cpg_rank_prune_zero(float *w, uint8_t *owner, int32_t cur, double ratio, int64_t n,
                        cpg_prune_result *result, void *ws, size_t ws_bytes, void *stream);

/* ---- K7: utils/prune.py:111-193 (the four mask statistics), one layer ----
 * hist[0..255] += #(owner == id); hist[256] += #(0 < owner < inference_idx && pm > 0.005f)
 * (only when pm != NULL).  `hist` = 257 uint64 in device memory, ACCUMULATED so one buffer can
 * collect all layers; the caller zeroes it. */
int cpg_mask_hist(const uint8_t *owner, const float *pm, int32_t inference_idx, int64_t n,
                  uint64_t *hist, void *stream);

/* ---- K8: utils/prune.py:213-243 ---- */
/* apply_mask (:223-231): w[owner == 0 || owner > inference_idx] = 0 */
int cpg_apply_mask(float *w, const uint8_t *owner, int32_t inference_idx, int64_t n, void *stream);
/* make_pruned_zero (:213-221): w[owner == 0] = 0 */
int cpg_zero_pruned(float *w, const uint8_t *owner, int64_t n, void *stream);
/* make_finetuning_mask (:233-243): owner[owner == 0] = new_idx */
int cpg_claim_free(uint8_t *owner, int32_t new_idx, int64_t n, void *stream);

/* ---- data-parallel payload (reference: nn.DataParallel reduces every gradient, CPG_cifar100_main_normal.py:199) ----
 * Gradient routing (K4e) zeroes every slot the current task does not own right after the all-reduce, so only the surviving
 * slots need to cross xGMI: select 0 = owner == cur (weight gradients), select 1 = 0 < owner < cur (piggymask gradients,
 * finetune mode).  cpg_owned_block_counts writes the number of selected slots of every 1024-element block
 * (cpg_owned_num_blocks(n) int32 values); the caller turns them into EXCLUSIVE prefix sums (int64, device) -- cacheable
 * until the owner mask mutates -- and cpg_pack_owned gathers g.flatten()[selected] (natural order) into `packed`,
 * cpg_unpack_owned scatters it back; unselected slots of g are left untouched.  Owner masks are replicated, so packed
 * buffers are element-aligned across ranks. */
int64_t cpg_owned_num_blocks(int64_t n);
int cpg_owned_block_counts(const uint8_t *owner, int32_t cur, int32_t select, int64_t n, int32_t *counts, void *stream);
int cpg_pack_owned(const float *g, const uint8_t *owner, int32_t cur, int32_t select, int64_t n, const int64_t *block_offsets,
                   float *packed, void *stream);
int cpg_unpack_owned(const float *packed, const uint8_t *owner, int32_t cur, int32_t select, int64_t n,
                     const int64_t *block_offsets, float *g, void *stream);

/* ---- fused masked SGD step, one layer ----
 * do_weight_decay_and_make_grads_zero (utils/prune.py:203-205) + torch.optim.SGD(lr, momentum, nesterov,
 * dampening 0, weight_decay 0) (CPG_cifar100_main_normal.py:339-340) in one pass over w / gw / momentum / owner:
 * g = owner == cur ? gw + wd*w : 0;  buf = first_step ? g : momentum*buf + g;  w -= lr * (nesterov ? g + momentum*buf : buf).
 * gw is overwritten with the routed gradient g (the state the reference leaves in .grad). */
int cpg_sgd_route_step(float *w, float *gw, float *momentum_buf, const uint8_t *owner, int32_t cur, float wd,
                       float lr, float momentum, int32_t nesterov, int32_t first_step, int64_t n, void *stream);

/* Fused piggymask step for task >= 2: the piggymask part of do_weight_decay_and_make_grads_zero (utils/prune.py:206-210:
 * finetune -> gradient zeroed where owner == 0 or owner >= cur, prune -> all zero) followed by torch.optim.Adam's update
 * (CPG_cifar100_main_normal.py:342-346; amsgrad = False, weight_decay = 0) in one pass; `step` is the 1-based Adam step
 * count, exp_avg / exp_avg_sq its state (zeros before step 1).  The routed gradient is written back to gpm.
 * The hyper-parameters are DOUBLES, as torch holds them (python floats): torch forms 1 - beta, lr / bias_correction1 and
 * sqrt(bias_correction2) in double and only then rounds to fp32 -- 1 - 0.999 is 0.001 there, but 0.00099998713 when formed from
 * the fp32 value 0.999f (ABI version 2; version 1 took floats and was 1.3e-5 off in exp_avg_sq). */
int cpg_adam_route_step(float *pm, float *gpm, float *exp_avg, float *exp_avg_sq, const uint8_t *owner, int32_t cur,
                        int32_t mode, double lr, double beta1, double beta2, double eps, int32_t step, int64_t n, void *stream);

/* The two fused optimizer passes over MANY layers in one launch (ABI version 3): ResNet-50 has 53 masked layers of 4 k - 2.4 M weights
 * each, and 53 launches of a few microseconds cost the queue more than the bytes they move.  `items_host` is a HOST array (the pointers
 * inside are device pointers, as everywhere else); the library passes them to the kernel by value, cpg_multi_tensor_max() layers per
 * launch, so nothing is copied to the device and the array may be freed or reused when the call returns.  All items share the scalar
 * arguments -- callers group parameters by (lr, momentum, nesterov, first_step) / (lr, betas, eps, step) as torch's own foreach path
 * does.  Element for element the arithmetic is cpg_sgd_route_step's / cpg_adam_route_step's: results are bit-equal to per-layer calls.
 * Every row is checked before the first launch -- null pointers, a negative n, and the 2^30-block limit of the launch the row falls
 * into: a bad table returns CPG_E_INVALID and changes nothing, however many launches' worth of good rows precede the bad one.  This
 * holds for cpg_sgd_route_step_multi, cpg_sgd_route_zero_step_multi and cpg_adam_route_step_multi alike.
 * Replaces the same reference lines: utils/prune.py:195-211 + CPG_cifar100_main_normal.py:339-346. */
typedef struct cpg_sgd_item {
    float *w, *gw, *momentum_buf;
    const uint8_t *owner;
    int64_t n;
} cpg_sgd_item;
typedef struct cpg_adam_item {
    float *pm, *gpm, *exp_avg, *exp_avg_sq;
    const uint8_t *owner;
    int64_t n;
} cpg_adam_item;
int32_t cpg_multi_tensor_max(void);
int cpg_sgd_route_step_multi(const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                             int32_t nesterov, int32_t first_step, void *stream);
int cpg_adam_route_step_multi(const cpg_adam_item *items_host, int32_t n_items, int32_t cur, int32_t mode, double lr, double beta1,
                              double beta2, double eps, int32_t step, void *stream);

/* The PackNet step in one pass: do_weight_decay_and_make_grads_zero (utils/packnet_prune.py:146-159), optim.SGD(momentum, nesterov)
 * (packnet_cifar100_main_normal.py:229-230) and make_pruned_zero (utils/packnet_prune.py:161-171, called after every step at
 * utils/packnet_manager.py:69).  g, buf and the step direction d are cpg_sgd_route_step's; w = (owner == 0) ? +0.0f : w - lr * d.  The routed
 * gradient and the momentum buffer are written as by cpg_sgd_route_step: the reference's momentum keeps decaying on pruned slots and
 * only the weight is pinned to zero.  Bit-equal to cpg_sgd_route_step followed by cpg_zero_pruned at the traffic of the former (w is
 * written anyway).  The multi form takes cpg_sgd_route_step_multi's item rows and follows its conventions.  Callers probe
 * for the symbols (CPG_ABI_VERSION stays 3). */
int cpg_sgd_route_zero_step(float *w, float *gw, float *momentum_buf, const uint8_t *owner, int32_t cur, float wd,
                            float lr, float momentum, int32_t nesterov, int32_t first_step, int64_t n, void *stream);
int cpg_sgd_route_zero_step_multi(const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                                  int32_t nesterov, int32_t first_step, void *stream);

/* ---- step telemetry: the STATS forms of the three multi-tensor passes (no counterpart in the reference, which has no way to see a
 * run diverge while it trains) ----
 * Each performs its plain twin's update, bit for bit, and reduces what the pass holds in registers anyway into one record per item:
 * stats[i] describes row i of the table (a row with n == 0: all zeros).  A record is 8 doubles; counts are integers held in doubles.
 * The reduction is thread (fp64 sums of the fp32 values: a square is exact, only the order of additions can move a bit) -> block
 * (one record per 4096-element piece, plain stores into `partials`) -> a finalize launch on the same stream that merges every item's
 * pieces in a fixed order.  No atomics: stats and partials are bit-reproducible from run to run.
 * `partials`: at least cpg_step_stats_workspace_bytes of the table's n column (64 bytes per piece; 0 for an empty table), contents
 * undefined afterwards.  `step` is the caller's 1-based step number.  `health` is a DEVICE int64[4] the caller owns and zeroes once:
 * {first_bad_step, first_bad_item, kind, bad_steps}.  kind 1: a non-finite routed gradient, 2: a non-finite weight / piggymask after
 * the step (an item with both reports 1; the piggymask record has no gradient count, so the Adam form only ever reports 2).  The
 * first three are written only while first_bad_step == 0, with the lowest bad item of that step; bad_steps grows by one per call
 * that saw any bad item.  Checks, in this order and all before the first launch (a refused call changes nothing): the plain twin's,
 * step < 1 or a null health (CPG_E_INVALID), partials_bytes below the query's answer (CPG_E_WORKSPACE), stats or partials null or not
 * 16-byte aligned (CPG_E_INVALID).  Tables longer than cpg_multi_tensor_max non-empty rows run as several launches with one running
 * piece index.  Callers probe for the symbols (CPG_ABI_VERSION stays 3). */
typedef struct cpg_sgd_step_stats {   /* routed := owner == cur; g: the routed gradient as written back; w': the weight after the step */
    double n_routed;                  /* routed slots                                                     */
    double g_nonfinite;               /* routed slots with a non-finite g                                 */
    double g_sumsq, g_absmax;         /* sum g^2, max |g| over the routed slots with a finite g (0: none) */
    double w_nonfinite;               /* ALL slots with a non-finite w'                                   */
    double dw_sumsq;                  /* sum (w' - w)^2 where both are finite, the difference in fp64     */
    double w_sumsq, w_absmax;         /* over the finite w'                                               */
} cpg_sgd_step_stats;
typedef struct cpg_pm_step_stats {    /* keep := mode == finetune && owner != 0 && owner < cur; on: x > thr in fp32, false for NaN */
    double n_routed;                  /* kept slots                                                       */
    double g_sumsq, g_absmax;         /* over the kept slots with a finite routed gradient                */
    double dpm_sumsq;                 /* sum (pm' - pm)^2 where both are finite                           */
    double flips_on, flips_off;       /* kept slots that went off -> on, on -> off                        */
    double picked;                    /* kept slots that are on after the step                            */
    double pm_nonfinite;              /* ALL slots with a non-finite pm'                                  */
} cpg_pm_step_stats;
size_t cpg_step_stats_workspace_bytes(const int64_t *n_host, int32_t n_items);
int cpg_sgd_route_step_multi_stats(const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                                   int32_t nesterov, int32_t first_step, int64_t step, void *stats, void *partials, size_t partials_bytes,
                                   int64_t *health, void *stream);
int cpg_sgd_route_zero_step_multi_stats(const cpg_sgd_item *items_host, int32_t n_items, int32_t cur, float wd, float lr, float momentum,
                                        int32_t nesterov, int32_t first_step, int64_t step, void *stats, void *partials,
                                        size_t partials_bytes, int64_t *health, void *stream);
/* adam_step: the plain twin's `step` (Adam's 1-based bias-correction count); thr: the Binarizer threshold of flips and picked */
int cpg_adam_route_step_multi_stats(const cpg_adam_item *items_host, int32_t n_items, int32_t cur, int32_t mode, double lr, double beta1,
                                    double beta2, double eps, int32_t adam_step, float thr, int64_t step, void *stats, void *partials,
                                    size_t partials_bytes, int64_t *health, void *stream);

/* ---- nn.BatchNorm2d -> nn.ReLU(inplace) after each masked conv ----
 * (models/vgg.py:137-141: `layers += [conv2d, nn.BatchNorm2d(c), nn.ReLU(inplace=True)]`).
 * x, y, gy, gx: NCHW fp32 with HW = H*W; gamma/beta/mean/invstd/running_*: C floats.
 * fwd_train: batch statistics (biased variance for normalisation; running_var gets the unbiased one,
 *   running = (1 - momentum) * running + momentum * batch, as torch.nn.BatchNorm2d), writes mean and
 *   invstd = 1/sqrt(var + eps) for the backward, then y = [max(0,] (x-mean)*invstd*gamma + beta [)].
 *   running_mean/var may both be NULL.  Reductions are two-stage and deterministic.
 * fwd_eval : same affine map with caller-provided statistics.
 * bwd      : gradient of fwd_train (train != 0) or fwd_eval (train == 0); the ReLU mask is recomputed
 *   from x, so neither y nor a mask tensor is read.  dgamma / dbeta are overwritten. */
size_t cpg_bn_workspace_bytes(int32_t N, int32_t C, int32_t HW);
int cpg_bn_relu_fwd_train(const float *x, const float *gamma, const float *beta, float eps, float momentum,
                          float *running_mean, float *running_var, float *mean, float *invstd, float *y,
                          int32_t N, int32_t C, int32_t HW, int32_t relu, void *ws, size_t ws_bytes, void *stream);
int cpg_bn_relu_fwd_eval(const float *x, const float *gamma, const float *beta, const float *mean,
                         const float *invstd, float *y, int32_t N, int32_t C, int32_t HW, int32_t relu,
                         void *stream);
int cpg_bn_relu_bwd(const float *x, const float *gy, const float *gamma, const float *beta, const float *mean,
                    const float *invstd, float *gx, float *dgamma, float *dbeta, int32_t N, int32_t C,
                    int32_t HW, int32_t relu, int32_t train, void *ws, size_t ws_bytes, void *stream);

/* Which arithmetic a launch of this shape uses (pass: 0 forward, 1 input gradient, 2 weight gradient, 3 the inference entry
 * cpg_conv2d_fwd_bn_eval).
 * cpg_conv2d_fwd, cpg_conv2d_fwd_bnstats (0) and cpg_conv2d_dgrad (1) run 3x3 / stride 1 / pad 1 layers on even-sized maps with >= 16 channels on both sides (a multiple
 * of 4 on the contracted side) by Winograd F(2x2, 3x3): 16 instead of 36 multiplies per 2x2 output tile and channel pair, the
 * same sums in a different association -- 1-4e-6 of the output scale from fp64 where the direct kernels are at 0.5-1e-6; the
 * reference's own F.conv2d (models/layers.py:106-109) takes whichever algorithm cuDNN / MIOpen picks, Winograd included.
 * Returns 1 for such a launch, 0 for the direct / generic kernels.  Setting CPG_NO_WINO in the environment (read per call)
 * forces 0 everywhere.  cpg_conv2d_wgrad (2) uses the adjoint transform for maps that are 14 or a multiple of 28 pixels wide with channel counts that are
 * multiples of 32 (CPG_NO_WINO_WGRAD forces the direct kernels for this pass only).  cpg_conv2d_fwd_bn_eval (3) uses it on the
 * same shapes as the forward pass, with or without a conv bias and the skip statistics (the Winograd kernel's epilogue applies
 * the same expression and honours the same liveness words); the bf16 entry points never do. */
int32_t cpg_conv2d_winograd(const cpg_conv_desc *desc, int32_t pass);

/* Conv forward fused with the statistics pass of the BatchNorm2d that follows it in every CPG topology
 * (models/vgg.py:137-141 `conv2d, BatchNorm2d, ReLU`): the kernel that produces y also writes, per output channel and
 * pixel tile, {sum y, sum y^2} -> stats[K][tiles][2] (fp32), tiles = cpg_conv2d_bnstats_tiles(desc) (0: this shape has
 * no fused path -- use cpg_conv2d_fwd + cpg_bn_relu_fwd_train).  cpg_bn_stats_finalize merges them (fp64, fixed order)
 * into mean / invstd and the running statistics; the normalisation itself is then cpg_bn_relu_fwd_eval or
 * cpg_bn_relu_pool_fwd(train = 0) with those statistics, and backward is unchanged (train = 1). */
int32_t cpg_conv2d_bnstats_tiles(const cpg_conv_desc *desc);
int cpg_conv2d_fwd_bnstats(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                           const float *bias, float *y, float *stats, size_t stats_bytes, void *workspace,
                           size_t workspace_bytes, void *stream);
int cpg_bn_stats_finalize(const float *stats, int32_t tiles, int32_t N, int32_t C, int32_t HW, float eps, float momentum,
                          float *running_mean, float *running_var, float *mean, float *invstd, void *stream);
/* ... and (ABI version 3) nn.BatchNorm2d's `num_batches_tracked += 1` in the same launch (torch.nn.modules.batchnorm: the counter every
 * training-mode forward bumps; one `add<long>` launch per layer in stock torch -- 53 per ResNet-50 step).  num_batches_tracked: one int64
 * in device memory, may be NULL. */
int cpg_bn_stats_finalize_count(const float *stats, int32_t tiles, int32_t N, int32_t C, int32_t HW, float eps, float momentum,
                                float *running_mean, float *running_var, float *mean, float *invstd, int64_t *num_batches_tracked,
                                void *stream);

/* Inference (Manager.validate, utils/manager.py:103-121: apply_mask, then model.eval() forward): conv -> BatchNorm2d in
 * eval mode (-> ReLU) of models/vgg.py:137-141 as ONE kernel -- y = [max(0,] (conv(x, W_eff) + bias - running_mean) /
 * sqrt(running_var + eps) * gamma + beta [)] applied in the conv epilogue, so the raw conv output is never written and no
 * BatchNorm kernel runs.  cpg_conv2d_fwd_bn_eval_supported(desc) == 0: shape has no fused path (use cpg_conv2d_fwd +
 * cpg_bn_relu_fwd_eval).  No gradient counterpart: callers use it under torch.no_grad() only.
 * Dead channels are skipped: after apply_mask (utils/prune.py:223-231) every slot with owner 0 or > the inference task is
 * zero, so a network that was GROWN for later tasks (CPG_cifar100_main_normal.py:208-232) carries whole output channels and
 * trailing input channels that are zero for an earlier task.  The weight-pack pass records per-channel liveness (wave
 * ballots), a block whose output channels are all dead skips its MFMA loop (conv output exactly 0 -> it writes BatchNorm(bias))
 * and every block stops after the last live input channel: serving an old task from the resident wide model costs what
 * the reference's cropped model (CPG_cifar100_main_normal.py:233-249) costs.  skip_stats (device, may be NULL) receives
 * {4 * (number of 4-channel input chunks up to the last one with a live weight) -- 4 * (c_last / 4 + 1) for c_last the last
 * live input channel, 0 when no weight is live (C = 78 with channel 77 live: 80) --, number of output blocks that skipped their
 * MFMA loop (32 output channels per block in the Winograd one-wave kernels, 64 in the two-wave kernel, 64 or 128 in the direct
 * tiles; a block also spans a pixel tile, so the count is a diagnostic, not a channel count)}; {0, 0} with CPG_NO_DEAD_SKIP.
 * One deliberate difference from the reference: a NaN or Inf in an input channel past the last live chunk, or in any input of an
 * output block with no live weight, does not reach the output (that work is skipped; the reference computes 0 * Inf = NaN).
 * CPG_NO_DEAD_SKIP=1 restores the propagation; skipped work otherwise only ever drops exact zeros.
 *
 * Non-finite values, zeros and ties.  Apart from that skip, every fused activation keeps what torch.relu, max_pool2d and F.prelu keep:
 * the ReLU of a NaN is a NaN and a maximum over a window that holds a NaN is a NaN (relu_keep / max_keep of csrc/cpg_common.h -- ONE
 * definition each, used by the BatchNorm passes, the pooled passes, the fused stem, the inference epilogues below and the window
 * maxima of cpg_conv2d_fwd_attach_pool_max), +Inf and -Inf come out where and as torch puts them, and in training mode one NaN makes
 * its channel's batch and running statistics -- and with them that channel, and no other -- NaN.  A network whose activations have
 * overflowed therefore shows a NaN loss on the first bad step, fused or not.  Ties: a pooled gradient goes to the FIRST maximum of its
 * window in row-major order (MaxPool2d(2, 2) and the overlapping windows of MaxPool2d(3, 2, 1) alike), a NaN counting as the maximum;
 * relu'(0) = 0, so a gamma = 0, beta = 0 channel passes nothing back.  The signs of zeros are not specified (relu_keep(-0) = -0).
 * The one difference in the BACKWARD passes: torch's threshold_backward lets gy through where the activation is NaN; these kernels
 * mask by `activation > 0`, which is false for a NaN, so they pass 0 there -- gradients at, and parameter gradients summed over, a
 * non-finite activation are not the reference's.  tests/test_special_values_gpu.py holds all of this to the stock modules in fp64. */
int32_t cpg_conv2d_fwd_bn_eval_supported(const cpg_conv_desc *desc);
int cpg_conv2d_fwd_bn_eval(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                           const float *bias, const float *gamma, const float *beta, const float *running_mean,
                           const float *running_var, float eps, int32_t relu, float *y, int32_t *skip_stats, void *workspace,
                           size_t workspace_bytes, void *stream);
/* ... and the MaxPool2d(2, 2) of models/vgg.py:142-143 behind the group in the same kernel:
 *     y_pooled[N][K][H/2][W/2] = max over each 2x2 window of [max(0,] (conv(x, W_eff) + bias - running_mean) / sqrt(running_var + eps) * gamma + beta [)]
 * Per element the expression of cpg_conv2d_fwd_bn_eval -- the same operation order, invstd formed in the kernel, relu_keep -- and the
 * four values of a window combined with max_keep: bit for bit torch.nn.functional.max_pool2d(y, 2, 2) of cpg_conv2d_fwd_bn_eval's y, a
 * NaN in the window gives a NaN.  The full-resolution activation is never written (one F(2x2, 3x3) Winograd output tile is one window).
 * Shapes: 3x3 / stride 1 / pad 1 / dilation 1 / groups 1 with H and W even whose inference launch is a one- or two-wave Winograd kernel
 * (cpg_conv2d_winograd(desc, 3) == 1), any channel counts those take (78 / 156 / 313 / 627 included).  Everything else -- odd maps, the
 * direct tiles (maps and channel counts the Winograd kernels refuse, CPG_NO_WINO), the cooperative block kernel (CPG_WINO_KERNEL=block),
 * strided, pointwise, grouped and other descriptors -- answers 0 from cpg_conv2d_fwd_bn_eval_pool_supported(desc), the planner's answer
 * under the current option table (no launch code runs for it), and CPG_E_UNSUPPORTED from the call before anything is launched:
 * y_pooled is not touched.  Dead-channel skip and skip_stats: cpg_conv2d_fwd_bn_eval's for the same descriptor and option table (the
 * liveness words are re-zeroed by every call; {0, 0} with CPG_NO_DEAD_SKIP); a block with no live output channel writes [max(0,]
 * BatchNorm(bias) [)] to its pooled outputs.  workspace: cpg_conv2d_workspace_bytes(desc).  Pointers as for cpg_conv2d_fwd_bn_eval
 * (bias and skip_stats may be NULL); y_pooled must not overlap x (CPG_E_INVALID).  No gradient counterpart.  Callers probe for the
 * symbols; CPG_ABI_VERSION is unchanged. */
int32_t cpg_conv2d_fwd_bn_eval_pool_supported(const cpg_conv_desc *desc);
int cpg_conv2d_fwd_bn_eval_pool(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                                const float *bias, const float *gamma, const float *beta, const float *running_mean,
                                const float *running_var, float eps, int32_t relu, float *y_pooled, int32_t *skip_stats, void *workspace,
                                size_t workspace_bytes, void *stream);
/* The residual topologies' inference (models/resnet.py:83-95 under model.eval(): `conv1 -> bn1 -> relu`, `conv2 -> bn2 -> relu`,
 * `conv3 -> bn3`, and the shortcut `downsample = nn.Sequential(conv1x1, norm_layer)` of models/resnet.py:179-182): the two entry points
 * above also take every pointwise shape (1x1, any stride, pad 0, C and K multiples of 16) and every 3x3 / stride 2 / pad 1 shape that
 * cpg_conv2d_fwd runs on its specialised kernels, with the same contract -- y = [max(0,] (conv + bias - running_mean) /
 * sqrtf(running_var + eps) * gamma + beta [)], invstd formed in the kernel.  These shapes have NO dead-channel skip: a non-NULL
 * skip_stats receives {0, 0}, and cpg_conv2d_winograd(desc, 3) is 0 for them.  CPG_DISABLE_CONV1X1 / CPG_DISABLE_CONV3X3 / CPG_NO_S2
 * take the class away from cpg_conv2d_fwd and from this query alike.
 * cpg_conv2d_fwd_bn_eval_add is the block's tail (models/resnet.py:91-98: `out = self.bn3(self.conv3(out)); out += identity;
 * out = self.relu(out)`) as one kernel: y = [max(0,] bn(conv + bias) + residual [)], residual dense NCHW and shaped like y (it may not
 * be NULL: CPG_E_INVALID).  Pointwise shapes only: every other descriptor, 3x3 included, answers 0 / CPG_E_UNSUPPORTED and y is not
 * touched.  workspace: cpg_conv2d_workspace_bytes(desc); a packed operand armed with cpg_conv2d_use_packed is consumed as by
 * cpg_conv2d_fwd (and by cpg_conv2d_fwd_bn_eval on the pointwise shapes). */
int32_t cpg_conv2d_fwd_bn_eval_add_supported(const cpg_conv_desc *desc);
int cpg_conv2d_fwd_bn_eval_add(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                               const float *bias, const float *gamma, const float *beta, const float *running_mean,
                               const float *running_var, float eps, const float *residual, int32_t relu, float *y, void *workspace,
                               size_t workspace_bytes, void *stream);

/* SphereNet's inference (models/spherenet.py: `x = relu1_1(conv1_1(x)); x = x + relu1_3(conv1_3(relu1_2(conv1_2(x))))` with nn.PReLU
 * activations, under model.eval() and torch.no_grad()): conv -> (+ bias) -> PReLU (-> + the unit's residual) as ONE kernel,
 *     v = conv(x, W_eff) + bias;  z = v > 0 ? v : slope[k] * v;  y = z + residual
 * -- the residual is added AFTER the PReLU (unlike cpg_conv2d_fwd_bn_eval_add's tail).  The product is rounded, then selected, then the
 * sum is rounded: bit for bit what cpg_conv2d_fwd_bn_eval with the identity BatchNorm followed by cpg_prelu_fwd computes.
 * slope: n_slopes = K values (one per output channel) or 1 (shared); NULL or another count: CPG_E_INVALID.  bias and residual may be
 * NULL; residual is dense NCHW, shaped like y, and must not overlap y.
 * Classes, by the route cpg_conv2d_fwd takes: 3x3 s1 p1 with or without a residual -- the launch plan (kernel, tile, workspace layout),
 * the dead-channel skip and skip_stats of cpg_conv2d_fwd_bn_eval for the same descriptor and option table; a block with no live output
 * channel writes prelu(bias) + residual -- and 3x3 s2 p1 without a residual (no skip: skip_stats receives {0, 0}).  Everything else
 * (pointwise, generic, grouped descriptors, a residual on the strided class, the channel-split 14 x 14 tile of CPG_C3_FORCE=8) answers 0
 * from cpg_conv2d_fwd_prelu_eval_supported(desc, with_residual) -- the planner's answer, no launch code runs for it -- and
 * CPG_E_UNSUPPORTED from the call, before anything is launched: y is not touched.  workspace: cpg_conv2d_workspace_bytes(desc).
 * No gradient counterpart.  Callers probe for the symbols; CPG_ABI_VERSION is unchanged. */
int32_t cpg_conv2d_fwd_prelu_eval_supported(const cpg_conv_desc *desc, int32_t with_residual);
int cpg_conv2d_fwd_prelu_eval(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                              const float *bias, const float *slope, int32_t n_slopes, const float *residual, float *y,
                              int32_t *skip_stats, void *workspace, size_t workspace_bytes, void *stream);

/* ---- OPT-IN bf16 MFMA path (north_star: "MFMA fp32/bf16 GEMM") of the 3x3 / stride 1 / pad 1 convolution ----
 * Same contraction as cpg_conv2d_fwd / cpg_conv2d_dgrad with the operands (activations, effective weights W * bin(pm))
 * rounded to bf16 on their way into LDS, exact products, fp32 accumulation (v_mfma_f32_32x32x16_bf16) -- the arithmetic of
 * an autocast(bf16) convolution.  All tensors in HBM stay fp32 NCHW.  NOT the default: north_star's 1e-4 parity bar is an
 * fp32 bar; this path has its own tolerance (about 1e-2 of the output scale) and its own roofline (2.5 PFLOP/s).
 * cpg_conv2d_wgrad_bf16: gW_eff from bf16-rounded x and gy, then the same autograd epilogue as cpg_conv2d_wgrad; no bias
 * gradient -- layers with a bias and the 3 -> 64 stem (< 16 channels) use cpg_conv2d_wgrad (fp32).
 * The *_bf16x3 entry points run the same kernels with every operand split into two bf16 terms, v = hi + lo (hi = bf16(v),
 * lo = bf16(v - hi)), and accumulate a_hi*b_hi + a_hi*b_lo + a_lo*b_hi in fp32: ~16 mantissa bits per product instead of 8
 * (measured 5e-6 of the output scale per layer against 2.5e-3 for plain bf16 and 2.5e-7 for fp32 MFMA) at 3/16 of the fp32
 * MFMA cost.  Also opt-in: it meets north_star's 1e-4 logit bar, but it is not the reference's fp32 arithmetic.
 * Non-finite values: bf16x3 turns an Inf operand into NaN (lo = Inf - Inf), where plain bf16 keeps it an Inf
 * (tests/test_conv_bf16_gpu.py test_an_inf_operand_is_nan_under_bf16x3_and_inf_under_bf16).  Both arithmetics round a finite |v|
 * above bf16's largest finite value (about 3.3895e38) to Inf, so such an operand leaves no finite output where fp32 would
 * (test_a_finite_value_above_the_bf16_range_is_not_finite).
 * Workspaces: every bf16 entry point refuses (CPG_E_WORKSPACE) less than its query's answer, whatever part of it the call
 * uses, and (CPG_E_INVALID) a workspace that is not 16-byte aligned. */
int32_t cpg_conv2d_bf16_supported(const cpg_conv_desc *desc);
int32_t cpg_conv2d_wgrad_bf16_supported(const cpg_conv_desc *desc);
size_t cpg_conv2d_wgrad_bf16_workspace_bytes(const cpg_conv_desc *desc);
int cpg_conv2d_wgrad_bf16(const cpg_conv_desc *desc, const float *x, const float *gy, const float *w, const float *piggymask,
                          float threshold, float *gw, float *gpm, void *workspace, size_t workspace_bytes, void *stream);
int cpg_conv2d_fwd_bf16x3(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                          const float *bias, float *y, void *workspace, size_t workspace_bytes, void *stream);
int cpg_conv2d_dgrad_bf16x3(const cpg_conv_desc *desc, const float *gy, const float *w, const float *piggymask, float threshold,
                            float *gx, void *workspace, size_t workspace_bytes, void *stream);
int cpg_conv2d_wgrad_bf16x3(const cpg_conv_desc *desc, const float *x, const float *gy, const float *w, const float *piggymask,
                            float threshold, float *gw, float *gpm, void *workspace, size_t workspace_bytes, void *stream);
size_t cpg_conv2d_bf16_workspace_bytes(const cpg_conv_desc *desc);
int cpg_conv2d_fwd_bf16(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                        const float *bias, float *y, void *workspace, size_t workspace_bytes, void *stream);
int cpg_conv2d_dgrad_bf16(const cpg_conv_desc *desc, const float *gy, const float *w, const float *piggymask, float threshold,
                          float *gx, void *workspace, size_t workspace_bytes, void *stream);

/* The BatchNorm backward reduction riding in the NEXT layer's input-gradient kernel (the backward counterpart of
 * cpg_conv2d_fwd_bnstats): conv_{L+1}'s dgrad produces g = dL/da with a = relu(bn_L(ypre)); its epilogue reads ypre at the
 * same positions, stores gm = g * [bn_L(ypre) > 0] instead of g and writes {sum gm, sum gm * xhat} per (channel, pixel tile) ->
 * partials[C][tiles][2] (fp32), tiles = cpg_conv2d_dgrad_bnbwd_tiles(desc) (0: no fused path for this shape).
 * cpg_bn_bwd_from_partials merges them (fp64, fixed order) into dgamma / dbeta and runs the one remaining pass
 * dx = (gm - mean(gm) - xhat * mean(gm * xhat)) * invstd * gamma.  Saves the 2-read reduction pass of cpg_bn_relu_bwd. */
int32_t cpg_conv2d_dgrad_bnbwd_tiles(const cpg_conv_desc *desc);
int cpg_conv2d_dgrad_bnbwd(const cpg_conv_desc *desc, const float *gy, const float *w, const float *piggymask, float threshold,
                           const float *ypre, const float *gamma, const float *beta, const float *mean, const float *invstd,
                           float *gm, float *partials, size_t partial_bytes, void *workspace, size_t workspace_bytes, void *stream);
int cpg_bn_bwd_from_partials(const float *partials, int32_t tiles, const float *x, const float *gm, const float *gamma,
                             const float *beta, const float *mean, const float *invstd, float *gx, float *dgamma, float *dbeta,
                             int32_t N, int32_t C, int32_t HW, void *workspace, size_t workspace_bytes, void *stream);

/* The merge step of cpg_bn_bwd_from_partials alone: partials[C][tiles][2] = {sum gm, sum gm * xhat} -> dbeta, dgamma and
 * coef[2c] = mean(gm), coef[2c + 1] = mean(gm * xhat) over N * HW elements (fp64, fixed order). */
int cpg_bn_bwd_finalize_partials(const float *partials, int32_t tiles, int32_t N, int32_t C, int32_t HW, float *dgamma, float *dbeta,
                                 float *coef, void *stream);

/* The network stem fused with the training-mode BatchNorm2d -> ReLU behind it (VGG16 features.0-2, models/vgg.py:137-141 `conv2d,
 * nn.BatchNorm2d(v), nn.ReLU(inplace=True)`; SharableConv2d.forward, models/layers.py:98-109): a 3x3 s1 p1 conv from <= 3 channels to
 * 64 whose output y is NEVER written -- every pass recomputes it from the image (27 multiply-adds per output against 4 bytes of
 * HBM traffic per pass).  No conv bias.  Forward: cpg_stem_bn_stats (partial sums stats[64][tiles][2] of y) ->
 * cpg_bn_stats_finalize -> cpg_stem_bn_relu_fwd (z = relu(bn(y))).  Backward: cpg_stem_bn_relu_bwd_reduce (partials[64][tiles][2]
 * = {sum gm, sum gm * xhat}, gm = gz * [z > 0]) -> cpg_bn_bwd_finalize_partials -> cpg_stem_bn_relu_bwd_wgrad (the weight gradient; or
 * cpg_stem_bn_relu_bwd_apply for gy, the gradient w.r.t. the conv output, and cpg_conv2d_wgrad(x, gy)).  The image itself gets no gradient through this path. */
int32_t cpg_stem_bn_supported(const cpg_conv_desc *desc);
int32_t cpg_stem_bn_tiles(const cpg_conv_desc *desc);
int cpg_stem_bn_stats(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                      const float *bias, float *stats, size_t stats_bytes, void *stream);
int cpg_stem_bn_relu_fwd(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                         const float *bias, const float *gamma, const float *beta, const float *mean, const float *invstd, float *z,
                         void *stream);
int cpg_stem_bn_relu_bwd_reduce(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                                const float *bias, const float *gamma, const float *beta, const float *mean, const float *invstd,
                                const float *gz, float *partials, size_t partials_bytes, void *stream);
int cpg_stem_bn_relu_bwd_apply(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                               const float *bias, const float *gamma, const float *beta, const float *mean, const float *invstd,
                               const float *coef, const float *gz, float *gy, void *stream);
/* ... or, instead of cpg_stem_bn_relu_bwd_apply + cpg_conv2d_wgrad: gy contracted with the image patch inside the same pass (gy is
 * never written): gW = g * bin(pm), gPM = g * W as cpg_conv2d_wgrad.  workspace: cpg_stem_bn_wgrad_workspace(desc) bytes. */
size_t cpg_stem_bn_wgrad_workspace(const cpg_conv_desc *desc);
int cpg_stem_bn_relu_bwd_wgrad(const cpg_conv_desc *desc, const float *x, const float *w, const float *piggymask, float threshold,
                               const float *bias, const float *gamma, const float *beta, const float *mean, const float *invstd,
                               const float *coef, const float *gz, float *gw, float *gpm, void *workspace, size_t workspace_bytes,
                               void *stream);

/* y = relu(bn(x) + res): the tail of a residual block (models/resnet.py:69-74 `out = self.bn3(out); out += identity;
 * out = self.relu(out)`).  train != 0: batch statistics (mean / invstd out, running stats updated); train == 0: `mean`
 * / `invstd` are inputs.  relu_mask (may be NULL; cpg_bn_add_relu_mask_bytes() bytes, 0 = no mask for this shape: 4 must divide HW)
 * receives the ReLU mask of y, one byte per four consecutive elements (bit j: element 4 i + j > 0), for cpg_bn_add_relu_bwd. */
size_t cpg_bn_add_relu_mask_bytes(int32_t N, int32_t C, int32_t HW);
int cpg_bn_add_relu_fwd(const float *x, const float *res, const float *gamma, const float *beta, float eps,
                        float momentum, float *running_mean, float *running_var, float *mean, float *invstd, float *y,
                        int32_t N, int32_t C, int32_t HW, int32_t train, void *ws, size_t ws_bytes, void *stream, uint8_t *relu_mask);
/* Backward of cpg_bn_add_relu_fwd (out = relu(bn(x) + residual), the tail of a residual block, models/resnet.py:62-71,96-104 --
 * stock torch: threshold_backward, then the BatchNorm backward, 8 passes): gz = gy * [out > 0] (the residual branch's gradient; must
 * not alias gy) is written by the reduction pass that also needs it, gx is the BatchNorm input gradient.  7 passes -- 6 1/16 with
 * relu_mask (the forward's byte mask; `out` is then not read and may be NULL), 6 % of a ResNet-50 step's BatchNorm traffic. */
int cpg_bn_add_relu_bwd(const float *x, const float *out, const float *gy, const float *gamma, const float *beta,
                        const float *mean, const float *invstd, float *gx, float *gz, float *dgamma, float *dbeta, int32_t N,
                        int32_t C, int32_t HW, int32_t train, void *ws, size_t ws_bytes, void *stream, const uint8_t *relu_mask);

/* BatchNorm2d -> ReLU -> MaxPool2d(2, 2) fused (the 5 VGG blocks that end in 'M', models/vgg.py:131-141).
 * y_pooled / g_pooled: [N][C][H/2][W/2]; H and W even.  train != 0: batch statistics are computed (and
 * running stats updated) first; train == 0: `mean` / `invstd` are inputs.  The un-pooled activation is never
 * written: backward recomputes each window from x and routes the pooled gradient to its first maximum. */
int cpg_bn_relu_pool_fwd(const float *x, const float *gamma, const float *beta, float eps, float momentum,
                         float *running_mean, float *running_var, float *mean, float *invstd, float *y_pooled,
                         int32_t N, int32_t C, int32_t H, int32_t W, int32_t train, void *ws, size_t ws_bytes,
                         void *stream);
int cpg_bn_relu_pool_bwd(const float *x, const float *g_pooled, const float *gamma, const float *beta,
                         const float *mean, const float *invstd, float *gx, float *dgamma, float *dbeta,
                         int32_t N, int32_t C, int32_t H, int32_t W, int32_t train, void *ws, size_t ws_bytes,
                         void *stream);
/* The same pair with E[N][C][H/2][W/2], the window maxima of x from the conv that produced x (cpg_conv2d_fwd_attach_pool_max; the
 * ABI version stays 3, probe for the symbols).  A channel with gamma > 0 reads E instead of x in the forward apply pass and in the
 * backward reduction (1/4 of the bytes); a channel with gamma <= 0 reads x exactly as above.  The backward apply pass is unchanged.
 *   forward: stats != NULL: [C][tiles][2] partial sums of cpg_conv2d_fwd_bnstats, finalised here as cpg_bn_stats_finalize_count does
 *       (num_batches_tracked may be NULL); stats == NULL: mean / invstd are inputs.  y_pooled equals cpg_bn_relu_pool_fwd's as numbers
 *       (the sign of a zero may differ).
 *   backward: dbeta is bit-equal to cpg_bn_relu_pool_bwd's; dgamma and gx are too unless two DIFFERENT values of a window round to the
 *       same BatchNorm output, where the term of sum(g xhat) takes xhat of the larger instead of the first (an ulp of one term).
 *   cpg_bn_relu_pool_attach_max(E, bytes): the same through the entry points above -- arms THE CALLING THREAD, and the next
 *       cpg_bn_relu_pool_fwd or cpg_bn_relu_pool_bwd on it reads E (bytes >= N C (H/2) (W/2) floats, else CPG_E_INVALID) exactly as the
 *       _from_max call would.  One-shot: that call disarms the thread whatever it returns.  E == NULL disarms. */
int cpg_bn_relu_pool_attach_max(const float *E, size_t bytes);
int cpg_bn_relu_pool_fwd_from_max(const float *x, const float *E, const float *stats, int32_t tiles, const float *gamma, const float *beta,
                                  float eps, float momentum, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                                  float *mean, float *invstd, float *y_pooled, int32_t N, int32_t C, int32_t H, int32_t W, void *stream);
int cpg_bn_relu_pool_bwd_from_max(const float *x, const float *E, const float *g_pooled, const float *gamma, const float *beta,
                                  const float *mean, const float *invstd, float *gx, float *dgamma, float *dbeta, int32_t N, int32_t C,
                                  int32_t H, int32_t W, int32_t train, void *ws, size_t ws_bytes, void *stream);

/* BatchNorm2d -> ReLU -> MaxPool2d(3, stride 2, padding 1): the ResNet stem's tail (models/resnet.py:127-129,208-211 -- stock torch:
 * BatchNorm apply, max_pool2d with an int64 index tensor, max_pool2d backward, BatchNorm backward).  mean / invstd are given
 * (cpg_bn_stats_finalize after cpg_conv2d_fwd_bnstats in training, or the running statistics); the un-pooled activation is never
 * written; backward recomputes it plane by plane in LDS, routes the pooled gradient to each window's first maximum (torch's rule)
 * and applies the BatchNorm gradient (train != 0: batch statistics).  cpg_bn_relu_pool3_supported: rows of at most 512 pixels. */
int32_t cpg_bn_relu_pool3_supported(int32_t H, int32_t W);
int cpg_bn_relu_pool3_fwd(const float *x, const float *gamma, const float *beta, const float *mean, const float *invstd,
                          float *y_pooled, int32_t N, int32_t C, int32_t H, int32_t W, void *stream);
int cpg_bn_relu_pool3_bwd(const float *x, const float *g_pooled, const float *gamma, const float *beta, const float *mean,
                          const float *invstd, float *gx, float *dgamma, float *dbeta, int32_t N, int32_t C, int32_t H,
                          int32_t W, int32_t train, void *workspace, size_t workspace_bytes, void *stream);

/* Backward of nn.PReLU on an NCHW tensor (SphereNet-20's activation after every masked conv,
 * models/spherenet.py:126-166 `relu{stage}_{i} = nn.PReLU(channels)`):
 *   gx = x > 0 ? gy : slope[c] * gy,   gslope[c] = sum_{n,hw} (x > 0 ? 0 : gy * x)
 * in ONE pass over x and gy (deterministic two-stage slope reduction).  n_slopes = C (per-channel) or 1. */
size_t cpg_prelu_workspace_bytes(int32_t N, int32_t C, int32_t HW);
int cpg_prelu_bwd(const float *x, const float *gy, const float *slope, float *gx, float *gslope, int32_t N,
                  int32_t C, int32_t HW, int32_t n_slopes, void *ws, size_t ws_bytes, void *stream);
/* ... and, when x is the output of a conv WITH bias that only this PReLU consumes (every SphereNet conv, models/spherenet.py:203-217),
 * also gbias[c] = sum over (n, pixels) of gx -- the conv's bias gradient, so that cpg_conv2d_wgrad is called with gb = NULL and no
 * separate reduction pass over gx runs. */
int cpg_prelu_bwd_bias(const float *x, const float *gy, const float *slope, float *gx, float *gslope, float *gbias, int32_t N,
                       int32_t C, int32_t HW, int32_t n_slopes, void *workspace, size_t workspace_bytes, void *stream);
/* PReLU forward with the residual add of a SphereNet unit folded in (models/spherenet.py:219-247: x + relu(conv(.))):
 * y = residual + (x > 0 ? x : slope[c] x); residual may be NULL.  One pass instead of torch's prelu + add kernels. */
int cpg_prelu_fwd(const float *x, const float *residual, const float *slope, float *y, int32_t N, int32_t C, int32_t HW,
                  int32_t n_slopes, void *stream);

/* ---- image batches: the reference's data transforms on a uint8 image store in device memory (cpg_amd/data.py) ----
 * Images are RGB, HWC, uint8 (3 bytes per pixel), each at its own byte offset of one flat device buffer `src` of src_bytes bytes.
 * `items_host` is a HOST array, as in cpg_sgd_route_step_multi: the library checks every item against the buffer sizes it is
 * given BEFORE it launches anything (a bad item returns CPG_E_INVALID, a short workspace CPG_E_WORKSPACE, cpg_last_error names the
 * item), then passes the items to the kernels by value, so the table may be freed when the call returns.  Compatible additions:
 * the ABI version stays 3.
 *
 * cpg_image_resample: per item, crop rows [crop_y, crop_y + crop_h) x columns [crop_x, crop_x + crop_w) of the image, then resize
 * the crop to out_h x out_w with PIL's 8-bit BILINEAR filter, written HWC at dst + dst_off (dst_bytes bytes in all).  Bit-identical
 * to PIL.Image.crop(box).resize((out_w, out_h), Image.BILINEAR) (Resample.c: fp64 coefficients, 22-bit fixed point, horizontal pass
 * then vertical pass, a pass skipped when its axis keeps its size; the filter never reads outside the crop).  This is what
 * torchvision's RandomSizedCrop / Resize(int) / Scale compute on PIL images (utils/fine_grained_dataset.py:36-70,117-155,
 * utils/face_dataset.py:14-19).  Items that change both sizes need workspace for their horizontal pass:
 * cpg_image_resample_workspace_bytes(items) bytes for the same table.
 *
 * cpg_image_to_tensor: item i writes sample i of dst, fp32 NCHW [n_items][3][out_h][out_w] (dst_bytes bytes at least): output
 * pixel (y, x) is image pixel (y0 + y, x0 + x') with x' = flip ? out_w - 1 - x : x, byte 0 where that lies outside the image
 * (RandomCrop(padding)'s zero fill), then ((float)u / 255 - mean[c]) / std[c] with IEEE divisions (ToTensor + Normalize), times
 * 0.0f inside the Cutout rectangle [cut_y0, cut_y1) x [cut_x0, cut_x1) (empty when cut_y0 >= cut_y1 or cut_x0 >= cut_x1; the
 * multiply keeps -0.0 as `img *= mask` does, utils/fine_grained_dataset.py:33).  mean_host / std_host: 3 host floats each. */
typedef struct cpg_resample_item {
    int64_t src_off;                          /* byte offset of the image in src                 */
    int32_t src_h, src_w;
    int32_t crop_y, crop_x, crop_h, crop_w;   /* crop rectangle inside the image                 */
    int64_t dst_off;                          /* byte offset of the out_h x out_w x 3 result     */
    int32_t out_h, out_w;
} cpg_resample_item;                          /* 48 bytes */
typedef struct cpg_tensor_item {
    int64_t src_off;
    int32_t src_h, src_w;
    int32_t y0, x0;                           /* top-left of the out_h x out_w window; may lie outside the image */
    int32_t flip;                             /* 0 or 1 */
    int32_t cut_y0, cut_y1, cut_x0, cut_x1;   /* Cutout rectangle in output coordinates */
    int32_t reserved;
} cpg_tensor_item;                            /* 48 bytes */
size_t cpg_image_resample_workspace_bytes(const cpg_resample_item *items_host, int32_t n_items);
int cpg_image_resample(const uint8_t *src, int64_t src_bytes, const cpg_resample_item *items_host, int32_t n_items, uint8_t *dst,
                       int64_t dst_bytes, void *workspace, size_t workspace_bytes, void *stream);
int cpg_image_to_tensor(const uint8_t *src, int64_t src_bytes, const cpg_tensor_item *items_host, int32_t n_items, int32_t out_h,
                        int32_t out_w, const float *mean_host, const float *std_host, float *dst, int64_t dst_bytes, void *stream);

/* ---- pair verification: the reference's LFW scoring (utils/metrics.py: distance, then calculate_roc's 10-fold threshold search;
 * utils/manager.py:156-195 evalLFW) on embeddings in device memory (cpg_amd/utils/metrics.py).  Compatible additions: the ABI
 * version stays 3.
 *
 * cpg_pair_distance: dist[i] for the pairs (row i of a, row i of b), i < n; a and b are fp32 row-major [n][d] with leading
 * dimensions lda, ldb >= d; 1 <= d <= 4096.  metric 0: sum((a - b)^2); metric 1: dot / (|a| * |b|), clipped to [0, 1] (NaN stays
 * NaN: a zero row gives NaN), float32(acos) * 4 / float32(pi).  Every row sum is numpy's float32 pairwise summation in numpy's order
 * (np.sum / np.linalg.norm along axis 1 of a C-contiguous float32 matrix), every product and sum rounded to fp32 (no FMA), sqrt and
 * divisions IEEE: metric 0 and the cosine are bit-identical to the reference; metric 1's arccos is fp64's, rounded once to fp32
 * (numpy's float32 arccos is within an ulp or two of it).  sim (may be NULL): metric 1 writes dot / (|a| * |b|) before the clip.
 * n == 0 launches nothing.
 *
 * cpg_pair_sweep: the test-set counts of calculate_accuracy (utils/metrics.py:63-74) for every fold of KFold(nfolds, shuffle=False)
 * over the n pairs (contiguous folds, the first n % nfolds one pair longer) and every threshold of thr_host, a HOST table of n_thr
 * strictly ascending fp64 values (1 <= n_thr <= 480; it travels to the kernel by value).  A pair is predicted "same" at threshold t
 * when (double)dist < thr[t] -- numpy >= 2's comparison of a float32 distance with a float64 threshold; numpy 1.x compared in fp32,
 * which is this call with the table rounded to float32 first.  A NaN distance is never "same".  issame: n bytes, nonzero = same.
 * counts: int64 [nfolds][n_thr][4] = {tp, fp, tn, fn} of the fold's test pairs (the train counts are the totals minus these).
 * best: int64 [nfolds], the first threshold index that maximises the TRAIN set's tp + tn (np.argmax(acc_train)).  Integer work:
 * bit-exact given the distances.  Refused before any launch (CPG_E_INVALID): a table that is not strictly ascending or holds NaN,
 * nfolds < 2, n < nfolds, n_thr outside [1, 480], n > 2^31 - 1. */
int cpg_pair_distance(const float *a, int64_t lda, const float *b, int64_t ldb, int64_t n, int32_t d, int32_t metric, float *dist, float *sim,
                      void *stream);
int cpg_pair_sweep(const float *dist, const uint8_t *issame, int64_t n, const double *thr_host, int32_t n_thr, int32_t nfolds, int64_t *counts,
                   int64_t *best, void *stream);

/* ---- pair verification with subtract_mean, and VAL@FAR (utils/metrics.py: calculate_roc / calculate_val with subtract_mean=True,
 * calculate_val_far).  Compatible additions: the ABI version stays 3.  Folds are KFold(nfolds, shuffle=False)'s, as above.
 *
 * cpg_pair_fold_mean: mean[f][c], fp32 [nfolds][d], = np.mean(np.concatenate([a[train_f], b[train_f]]), axis=0)[c], train_f every pair
 * outside fold f: the sum starts from the add reduction's identity 0 and takes the 2 (n - |fold f|) rows one after another, a's
 * first (numpy's order for axis 0 of a C-contiguous float32 matrix; for d == 1 the rows form one contiguous run, which numpy sums
 * pairwise as cpg_pair_distance's row sums), then one division by float32(row count).  Every (fold, column) walks its own rows: no
 * "total minus the fold".  Bit-identical to numpy.  nfolds >= 2, n >= nfolds.
 *
 * cpg_pair_distance_centred: cpg_pair_distance of (a - mean[f], b - mean[f]) for every fold f < nfolds, each difference rounded to
 * fp32 before use: dist (and sim, may be NULL) are fp32 [nfolds][n], row f for fold f.  Same arithmetic and order as
 * cpg_pair_distance otherwise.
 *
 * cpg_pair_sweep_folds: cpg_pair_sweep where fold f reads row f of a distance matrix [nfolds][ldd], ldd >= n.
 *
 * cpg_pair_val_table: calculate_val's inner loop.  table: int64 [nfolds][n_thr][2] = {true accepts, false accepts} of fold f's
 * TRAIN pairs at threshold t ((double)dist < thr[t], as cpg_pair_sweep); totals: int64 [nfolds][2] = {n_same, n_diff} of those
 * pairs.  ldd == 0: every fold reads the same n distances; ldd >= n: fold f reads row f.  thr_host: a HOST table of n_thr strictly
 * ascending fp64 values, 1 <= n_thr <= cpg_pair_val_max_thresholds (the kernel keeps two histograms of n_thr + 1 counters in
 * one block's LDS; a longer table is refused with CPG_E_INVALID, never truncated).  workspace: cpg_pair_val_workspace_bytes(n_thr)
 * bytes of device memory, 8-byte aligned (the table's device copy; 0 for an n_thr the call refuses).
 *
 * cpg_pair_val_at: calculate_val_far on every fold's TEST pairs at one threshold per fold.  thr_host: nfolds HOST fp64 values (any
 * value; NaN accepts nothing).  out: int64 [nfolds][4] = {true accepts, false accepts, n_same, n_diff}.  nfolds >= 1 (one fold: all
 * n pairs).  ldd as for cpg_pair_val_table. */
int cpg_pair_fold_mean(const float *a, int64_t lda, const float *b, int64_t ldb, int64_t n, int32_t d, int32_t nfolds, float *mean, void *stream);
int cpg_pair_distance_centred(const float *a, int64_t lda, const float *b, int64_t ldb, int64_t n, int32_t d, int32_t metric, const float *mean,
                              int32_t nfolds, float *dist, float *sim, void *stream);
int cpg_pair_sweep_folds(const float *dist, int64_t ldd, const uint8_t *issame, int64_t n, const double *thr_host, int32_t n_thr, int32_t nfolds,
                         int64_t *counts, int64_t *best, void *stream);
int32_t cpg_pair_val_max_thresholds(void);
size_t cpg_pair_val_workspace_bytes(int32_t n_thr);
int cpg_pair_val_table(const float *dist, int64_t ldd, const uint8_t *issame, int64_t n, const double *thr_host, int32_t n_thr, int32_t nfolds,
                       int64_t *table, int64_t *totals, void *workspace, size_t workspace_bytes, void *stream);
int cpg_pair_val_at(const float *dist, int64_t ldd, const uint8_t *issame, int64_t n, const double *thr_host, int32_t nfolds, int64_t *out,
                    void *stream);

/* ---- loss heads: from the network's output to the loss, the accuracy and the gradient that starts the backward pass.  Compatible
 * additions: the ABI version stays 3 (probe with dlsym, as for the rider entries above).  Every reduction has a fixed order (no
 * floating-point atomics): two calls on the same inputs give the same bytes.  loss and correct are ONE float each in device memory;
 * nothing is synchronised.  target: int64 [B].
 *
 * cpg_loss_heads_workspace_bytes: the workspace of the four calls below for B rows, C classes and D embedding features (D == 0: the
 * two cross-entropy calls alone).  16-byte aligned.
 *
 * cpg_softmax_xent_fwd / _fwd_bwd: nn.CrossEntropyLoss(weight=class_weight) with its mean reduction plus classification_accuracy
 * (utils/manager.py:29-36,58-62,120-121; utils/__init__.py:46-49) on logits [B][C], any B >= 1 and C >= 1:
 *   nll_i = logsumexp(z_i) - z_i[t_i] (the row maximum subtracted before the exponentials), W = sum_i class_weight[t_i] (NULL: the
 *   number of counted rows), loss = sum_i class_weight[t_i] nll_i / W, correct = the number of rows whose FIRST maximum index is t_i.
 *   _fwd_bwd also writes dlogits[i][j] = g class_weight[t_i] (softmax_ij - [j == t_i]) / W, g = gscale[0] (a DEVICE scalar: the
 *   upstream gradient of the loss; NULL: 1); there loss and correct may both be NULL (gradient only: the launch that adds the rows'
 *   results up is skipped -- what a backward pass wants after _fwd gave the two numbers).  Rows of up to 8 192 classes are read from
 *   memory once (they live in registers); wider rows are streamed two (forward) or three (with the gradient) times.
 * A row whose target is outside [0, C) -- torch's ignore_index = -100 included -- counts with weight 0, is never correct, gets an
 * exactly zero gradient row and indexes no memory.  A NaN logit in a counted row gives a NaN loss; no counted row gives 0 / 0.
 *
 * cpg_angle_head_fwd / _bwd: AngleLinear followed by AngleLoss (models/spherenet.py:24-61 and :64-98; CPG_face_main.py selects them
 * for face_verification) for m = 4 and gamma = 0 ONLY -- anything else is refused with CPG_E_INVALID before a pointer is looked at.
 * x [B][D] embeddings, w [D][C] (AngleLinear's own layout), lamb = max(LambdaMin, LambdaMax / (1 + 0.1 it)) of THIS call (the caller
 * keeps `it`), s = 1 / (1 + lamb).  With n_j = |w[:, j]|, what = w / n_j, z = x . what, y = t_i, c_i = clamp(z_iy / |x_i|, -1, 1),
 * k_i = floor(4 acos(c_i) / 3.14159265), phi_i = (-1)^k (8 c^4 - 8 c^2 + 1) - 2 k:
 *   f = z except f_iy = (1 - s) z_iy + s |x_i| phi_i;  loss, correct = the cross-entropy above on (f, target), no class weights.
 * That is the reference's result restated: its renorm(2, 1, 1e-5).mul(1e5) cancels against the division by the column norm, and
 * phi(theta) only ever reaches the loss through the target column.  _fwd writes what [D][C], colnorm [C], f [B][C] and
 * saved [B][4] = {|x_i|, c_i, phi_i, phi'_i}, which the caller keeps for _bwd:
 *   phi'_i = (-1)^k (32 c^3 - 16 c) (0 where the clamp bit), dz = df except dz_iy = df_iy ((1 - s) + s phi'_i),
 *   gx_i = dz_i . what^T + df_iy s (phi_i - c_i phi'_i) x_i / |x_i|,  G = x^T . dz,  gw_j = (G_j - what_j (what_j . G_j)) / n_j
 * (the gradient through the renorm included), df being _fwd_bwd's dlogits on f with the same gscale.  The three products run on the
 * fp32-MFMA kernels of the linear layers.  Preconditions, as in the reference, which divides by both: no zero column in w, no zero row
 * in x.  A row whose target is outside [0, C) takes no margin and no part in the loss. */
size_t cpg_loss_heads_workspace_bytes(int32_t B, int32_t D, int32_t C);
int cpg_softmax_xent_fwd(const float *logits, const int64_t *target, const float *class_weight, int32_t B, int32_t C, float *loss,
                         float *correct, void *workspace, size_t workspace_bytes, void *stream);
int cpg_softmax_xent_fwd_bwd(const float *logits, const int64_t *target, const float *class_weight, const float *gscale, int32_t B,
                             int32_t C, float *loss, float *correct, float *dlogits, void *workspace, size_t workspace_bytes,
                             void *stream);
int cpg_angle_head_fwd(const float *x, const float *w, const int64_t *target, int32_t B, int32_t D, int32_t C, int32_t m, float gamma,
                       double lamb, float *what, float *colnorm, float *f, float *saved, float *loss, float *correct, void *workspace,
                       size_t workspace_bytes, void *stream);
int cpg_angle_head_bwd(const float *x, const float *what, const float *colnorm, const float *f, const float *saved,
                       const int64_t *target, const float *gscale, int32_t B, int32_t D, int32_t C, int32_t m, float gamma, double lamb,
                       float *gx, float *gw, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CPG_HIP_H */
