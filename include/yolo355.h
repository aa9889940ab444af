/*
 * yolo355.h — C ABI of libyolo355.so: the MI355X (gfx950) YOLOv3 hot path.
 *
 * This is the drop-in boundary.  The reference
 * (wizyoung/YOLOv3_TensorFlow) has no FFI of its own: its boundary is the Python
 * API of model.py and the utils package, whose arithmetic executes inside TensorFlow.  Each
 * entry point below names the reference interface (file:line under /root/reference)
 * whose TensorFlow-side execution it replaces.  The Python mirror of that API lives
 * in yolov3_tensorflow_amd/ and binds these symbols with ctypes.
 *
 * Conventions
 *   - plain C, no torch/TF types: device pointers + sizes only;
 *   - every call returns 0 on success, a negative Y3_E* code otherwise; the message
 *     is available from y3_last_error() (thread-local);
 *   - the caller owns every device buffer; the library allocates no device memory
 *     and keeps no pointer beyond the call, except the parameter buffer bound to a
 *     y3_net (which the caller must keep alive);
 *   - the other half of that ownership: the library reads no byte that can change a result, and writes no byte, outside the
 *     extents its arguments describe (a tensor's shape and row stride, a count, a *_bytes size).  Where a kernel's loads
 *     run past an extent (ragged tiles, prologues that issue ahead), a range check or a mask discards what they return;
 *     no store ever does.  Every *_bytes function (*_workspace_bytes, *_scratch_bytes, y3_net_params_bytes) is an exact
 *     upper bound on what the call touches in that buffer: a buffer of exactly that many bytes, not rounded up, is enough,
 *     and its contents on entry never matter.  tests/test_guard_bands_gpu.py holds every entry point to this;
 *   - device pointers need 16-byte alignment unless the entry says otherwise (the net's parameter buffer and workspaces:
 *     256; the evaluators' tables: the alignment of their element type; dw_hwio of the weight gradients and the
 *     optimizer's tensors with n %% 4 != 0: 4).  An entry that checks alignment refuses with Y3_EINVAL before any launch;
 *   - activations are NHWC fp32 contiguous; conv kernels in TF layout are HWIO
 *     (utils/misc_utils.py:117-120) and are re-packed once by y3_pack_conv_weights;
 *   - every launch goes to the hipStream_t bound to the context; no call synchronises
 *     the host except y3_nms_counts_to_host-style helpers that say so.
 */
#ifndef YOLO355_H
#define YOLO355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y3_OK 0
#define Y3_EINVAL (-1)   /* bad argument / unsupported shape (maps to ValueError / InvalidArgumentError) */
#define Y3_EHIP (-2)     /* a HIP runtime call failed */
#define Y3_ESTATE (-3)   /* object used before it was fully configured */

/* 5: y3_feed_run takes the blob's size and an arena (the arguments of version 4's second, checked feed entry, which is gone).
 * A caller built against version 4 must not call a version 5 library: the name is the same, the arguments are not. */
#define Y3_ABI_VERSION 5

typedef struct y3_ctx y3_ctx; /* one per (device, stream) */
typedef struct y3_net y3_net; /* the 75-conv YOLOv3 graph bound to caller-owned parameters */
typedef struct y3_train_var y3_train_var; /* one layer's variables (below, with the train step) */

/* Thread-local message of the last failing call on this thread ("" if none). */
const char* y3_last_error(void);
int y3_abi_version(void);

/* stream: a hipStream_t (0 = the null stream).  The library never creates streams.  A context owns one 64-byte block of
 * pinned, device-visible host memory: its error word (below). */
int y3_ctx_create(int device, void* stream, y3_ctx** out);
int y3_ctx_destroy(y3_ctx* ctx);
/* Device-side failures are LOUD.  The stream-K conv schedules (y3_conv2d_fwd*, y3_conv2d_dgrad*, y3_net_forward) finish
 * tiles that were cut between two persistent workgroups inside the kernel: the consumer workgroup polls a flag the
 * producer raises.  The poll is bounded so that a launch can never hang; if it expires the tile's sum
 * is incomplete, and the kernel ORs a code into the context's error word.  From then on every conv / net entry point
 * called on that context returns Y3_EHIP ("a stream-K hand-off timed out ...") WITHOUT launching, until
 * y3_ctx_check — which synchronises the stream, reports the condition once more and clears it — has been called.
 * A caller that wants the guarantee for a specific batch calls y3_ctx_check after it (the Python mirror does so
 * wherever it synchronises anyway: NMS read-back, train.py's loss read-out, bench.py after the timed region).
 * Assumption the protocol rests on, stated here because HIP does not promise it: workgroups of one launch are
 * dispatched in increasing blockIdx order.  A consumer only ever waits for workgroups with SMALLER ids of its own
 * XCD group, so under that order it cannot wait for a workgroup that has not been dispatched; if a future dispatcher
 * broke the order, the bounded poll would expire and the failure would surface here, never as a silent wrong tensor.
 * Test hook: after y3_debug_streamk_fault(1) producers never raise their flag and consumers give up after 2^10 polls,
 * until y3_debug_streamk_fault(0) (process-wide; tests/test_conv_gpu.py::test_streamk_timeout_is_loud).  It is an
 * explicit call on purpose: no environment variable changes what the product library does. */
int y3_ctx_check(y3_ctx* ctx);
void y3_debug_streamk_fault(int on);

/* ---- parameter preparation (one-off, utils/misc_utils.py:114-124 produces HWIO) ---------------
 * w_hwio [k][k][cin][cout]  ->  w_packed [k*k][cout][cin]   (cin contiguous: 16-B loads along K).
 * For the Cin==3 stem conv the kernel consumes HWIO directly and no packing is needed. */
int y3_pack_conv_weights(y3_ctx* ctx, const float* w_hwio, int k, int cin, int cout, float* w_packed);

/* Inference batch-norm folding (model.py:35-41, eps=1e-5):
 *   scale = gamma * rsqrt(var + eps) ; shift = beta - mean * scale                              */
int y3_bn_fold(y3_ctx* ctx, const float* gamma, const float* beta, const float* mean,
               const float* var, float eps, int c, float* scale, float* shift);

/* ---- a1-a4: conv2d + BN + LeakyReLU (+ residual) (+ fused upsample/concat input) ---------------
 * Replaces utils/layer_utils.py:9-22 `conv2d` (slim.conv2d + batch_norm + leaky_relu, model.py:43-49),
 * the residual add of `res_block` (utils/layer_utils.py:25-32), `upsample_layer` (:82-87) and the
 * channel concat of model.py:62,72.
 *
 *   y = act(conv(x, w) * scale + shift) + residual
 *
 * k in {1,3}; stride 1 -> SAME; stride 2 -> explicit zero pad 1 each side then VALID
 * (utils/layer_utils.py:10-21), i.e. input row = oy*stride + ky - (k/2) in both cases.
 * If x_up != NULL (k must be 1): the logical input is concat([nearest_up2x(x_up), x], axis=3),
 * x_up is [N, H/2, W/2, c_up], x is [N, H, W, cin - c_up]; never materialised.
 * act: 0 = linear (detection convs, model.py:55-57), 1 = LeakyReLU(0.1).
 * scale/shift are per-output-channel (folded BN, or scale=1/shift=bias); residual may be NULL. */
typedef struct y3_conv_desc {
    int n, h, w;   /* logical input spatial size (after upsample for the fused-concat case) */
    int cin;       /* logical input channels (c_up + channels of x) */
    int c_up;      /* channels coming from x_up (0 if none) */
    int cout;
    int k;         /* 1 or 3 */
    int stride;    /* 1 or 2 */
    int act;       /* 0 linear, 1 leaky(0.1) */
} y3_conv_desc;

/* Scratch the stream-K schedule of this conv may use (0 if it never does): one accumulator slot per persistent
 * workgroup + one flag word each; uninitialised memory is fine (the library zeroes the words it polls ahead of every
 * launch; y3_net_forward gives each of its layers its own flag words and zeroes them all with one memset per forward)
 * and it must not be shared by launches on different streams.  Passing workspace = NULL to
 * y3_conv2d_fwd is allowed and selects the data-parallel schedule; results of the two schedules differ in
 * the last bits (the K sum of a split tile is associated differently), each is deterministic. */
size_t y3_conv_workspace_bytes(const y3_conv_desc* d);
/* Test hook (host arithmetic only, no device needed): the stream-K work split the kernels evaluate on the device.
 * `units` output tiles (kind 0: direct / split kernels) or Winograd blocks (kind 1) of `ksteps` K-steps each are divided,
 * whole, among 8 workgroup groups (blockIdx %% 8); inside group `group` its workers/8 local workers own equal
 * contiguous ranges of (unit, K-step) items: [*begin, *end) for `local_worker`.  A unit cut by a range boundary is
 * finished inside the kernel by the worker owning its K-step 0, from the partial sums the following local workers
 * publish; tests/test_streamk_partition.py replays that protocol on these ranges.
 * kind 2 = the Winograd kernel's default schedule: of group g's blocks [b0, b1) the first R*G (G = workers/8, R =
 * (b1-b0)/G whole rounds) are computed whole - round r, local worker j: block b0 + r*G + j - and [*begin, *end) is
 * `local_worker`'s range of the remaining (b1 - b0 - R*G) * ksteps items, cut as above. */
int y3_streamk_range(int kind, int units, int ksteps, int workers, int group, int local_worker, long long* begin,
                     long long* end);
/* Image ranges.  The fp32 conv kernels form 32-bit byte offsets, so ONE launch takes tensors below 2^29
 * elements.  Tensors are NHWC with the image index outermost: y3_conv2d_fwd[_stats], y3_conv2d_fwd_split,
 * y3_conv2d_dgrad[_bn], y3_conv2d_dgrad_split and y3_conv_wgrad run a larger call as several launches of the same kernel
 * over consecutive image ranges - nothing changes for the caller, and below the limit the call is the single launch it has
 * always been.  Reductions keep one fixed order: the statistics / BN-backward partial rows of a range lie behind the
 * previous range's (y3_conv_stats_blocks and y3_conv_dgrad_bn_blocks count them so), the weight gradient's split partials
 * of all ranges are added by one sum kernel, range-major (y3_conv_wgrad_scratch_bytes holds them all).  A cut call never
 * takes the stream-K schedule (y3_conv_schedule and y3_conv_workspace_bytes say so).  The Winograd, F(4x4,3x3) and bf16
 * entries keep their own limits (2^29; bf16: 2^30) and refuse larger tensors.
 * y3_conv_image_ranges is the planner all of them use (host arithmetic only): d is the FORWARD conv, its tensors are
 * [n,h,w,cin] and [n,h/stride,w/stride,co] with co = dz_stride where dz_stride > 0 (a gradient's row stride), else cout.
 * It writes begin[i], count[i] of the fewest ranges, of near-equal size, that keep both tensors below `limit` elements and
 * returns their number (1 = not cut), or Y3_EINVAL when one image alone reaches the limit or more than max_ranges ranges
 * would be needed.
 * Test hook: y3_debug_conv_range_limit(elements) lowers the limit of the entries above (process-wide) so that small shapes
 * are cut; 0 restores 2^29; values above 2^29 are ignored - it never raises any limit. */
int y3_conv_image_ranges(const y3_conv_desc* d, int dz_stride, long long limit, int max_ranges, int* begin, int* count);
void y3_debug_conv_range_limit(long long elements);
int y3_conv2d_fwd(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* x_up,
                  const float* w, const float* scale, const float* shift, const float* residual,
                  float* y, void* workspace, size_t workspace_bytes);

/* The first two convs of darknet53_body in one launch (utils/layer_utils.py:34-40: conv2d(inputs, 32, 3) and
 * conv2d(net, 64, 3, strides=2), each with folded batch norm and LeakyReLU), exact fp32 arithmetic: x = the image [n,h,w,3],
 * w0_hwio = the stem's HWIO kernel [3][3][3][32], w1_packed = the second conv's kernel from y3_pack_conv_weights (k = 3,
 * cin = 32, cout = 64), y = [n,h/2,w/2,64].  The stem's output - the largest tensor of the network - exists only in the LDS.
 * h and w even.  y3_net_forward (dtypes 0 and 4) uses it for its layers 0 and 1. */
int y3_conv2d_fwd_stem_s2(y3_ctx* ctx, int n, int h, int w, const float* x, const float* w0_hwio, const float* scale0,
                          const float* shift0, const float* w1_packed, const float* scale1, const float* shift1, float* y);

/* ---- bf16 storage / fp32 accumulate variant (BASELINE configs[4]: 608x608 bf16 inference) -----------------
 * Same contract as y3_conv2d_fwd (utils/layer_utils.py:9-22) with bf16 (round-to-nearest-even) activations, residual
 * and packed weights; scale/shift stay fp32; the accumulator is fp32; ONE rounding to bf16 at the store.
 * out_f32 != 0 writes fp32 (used for the detection convs so that decode/NMS are unchanged).  The Cin==3 stem
 * takes the fp32 image and the fp32 HWIO kernel and writes bf16.
 * w_packed (k*k*cin*cout bf16) is OPAQUE: y3_pack_conv_weights_bf16 chooses the layout from (k, cin) -
 * [tap][cin/64][cout][64] for the 3x3 convs with cin % 64 == 0 and (round 5) for the 1x1 convs with cin >= 512 and
 * cin % 64 == 0, [tap][cin/32][cout][32] otherwise - and y3_conv2d_fwd_bf16 assumes the same rule.  (Kernels behind it:
 * csrc/y3_conv_bf16x.hip - LDS-DMA 3x3 convs, tile shape per launch from a fitted cost model -, csrc/y3_conv_bf16r.hip - the
 * persistent ring kernel of the deep 1x1 convs -, csrc/y3_conv_bf16.hip - the register-staged kernel of the others.) */
int y3_pack_conv_weights_bf16(y3_ctx* ctx, const float* w_hwio, int k, int cin, int cout, void* w_packed);
/* Host-only: which tile shape y3_conv2d_fwd_bf16 runs this launch on - 'A' 256x256, 'B' 256x128, 'C' 128x128, 'D' 192x256, 'E'
 * 192x128 (3x3 convs, csrc/y3_conv_bf16x.hip); 'a'..'g' (the 1x1 ring kernel, csrc/y3_conv_bf16r.hip); 'x' narrow 3x3 forms; 'o'
 * the register-staged kernel; 's' the stem.  Documentation of the dispatch, not needed to call anything. */
int y3_conv_bf16_tile(const y3_conv_desc* d);
int y3_conv2d_fwd_bf16(y3_ctx* ctx, const y3_conv_desc* d, const void* x, const void* x_up, const void* w,
                       const float* scale, const float* shift, const void* residual, void* y, int out_f32);

/* The first two convs of darknet53_body in one launch (utils/layer_utils.py:34-40: conv2d(inputs, 32, 3) and
 * conv2d(net, 64, 3, strides=2), each with folded batch norm and LeakyReLU), bf16 storage: x = the fp32 image [n,h,w,3],
 * w0_hwio = the stem's fp32 HWIO kernel [3][3][3][32], w1_packed = the second conv's kernel from y3_pack_conv_weights_bf16
 * (k = 3, cin = 32, cout = 64), y = bf16 [n,h/2,w/2,64].  The stem's output exists only in the LDS; both convs accumulate
 * in fp32 on the bf16 matrix pipe.  The stem does NOT round the image: the fp32 image and the stem's kernel are each split once
 * into a high and a low bf16 part and the conv runs as three products (hi*hi + hi*lo + lo*hi: fp32-grade; a plainly rounded
 * image cost 0.05 of the mAP-style gate of tests/test_bf16_gpu.py); its output is rounded to bf16 like every other activation
 * of this path.  h and w even.
 * y3_net_forward (dtype 1) uses it for its layers 0 and 1. */
int y3_conv2d_fwd_bf16_stem_s2(y3_ctx* ctx, int n, int h, int w, const float* x, const float* w0_hwio, const float* scale0,
                               const float* shift0, const void* w1_packed, const float* scale1, const float* shift1, void* y);

/* The first residual block of darknet53_body in one launch (utils/layer_utils.py:25-32 res_block(net, 32) on a 64-channel map:
 * y = x + conv3x3(conv1x1(x)), both convs with folded batch norm and LeakyReLU), bf16 storage: x, y = bf16 [n,h,w,64];
 * w2_packed / w3_packed = the kernels of the 1x1 (64 -> 32) and the 3x3 (32 -> 64) conv from y3_pack_conv_weights_bf16.  The
 * 32-channel tensor between the convs exists only in the LDS and x is read once (it is the input AND the shortcut).
 * y3_net_forward (dtype 1) uses it for its layers 2 and 3. */
int y3_resblock64_fwd_bf16(y3_ctx* ctx, int n, int h, int w, const void* x, const void* w2_packed, const float* scale2,
                           const float* shift2, const void* w3_packed, const float* scale3, const float* shift3, void* y);

/* ---- Winograd F(2x2,3x3) form of the stride-1 3x3 conv (exact fp32 arithmetic, 2.25x fewer multiplies) ------------
 * Same tensors and epilogue as y3_conv2d_fwd (utils/layer_utils.py:9-22,25-32) for the convs
 * y3_conv_wino_eligible accepts (k = 3, stride 1, no fused upsample input, Cin %% 32 == 0,
 * Cout %% 32 == 0).  w_wino = G g G^T per (cin, cout), packed [16][cin/8][cout][8] fp32 (16*cin*cout floats) by
 * y3_pack_conv_weights_wino.  Results differ from the direct kernel by a few fp32 roundings per term.  With a
 * workspace the kernel may pick a stream-K schedule (persistent grid; cut blocks are summed inside the kernel in a fixed
 * order, so results are run-to-run bit-exact), as y3_conv2d_fwd does.  The workspace needs no initialisation: the
 * library zeroes the words it polls ahead of every launch. */
int y3_conv_wino_eligible(const y3_conv_desc* d);
int y3_pack_conv_weights_wino(y3_ctx* ctx, const float* w_hwio, int cin, int cout, float* w_wino);
size_t y3_conv_wino_workspace_bytes(const y3_conv_desc* d);   /* stream-K scratch; workspace = NULL is allowed */
int y3_conv2d_fwd_wino(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w_wino, const float* scale,
                       const float* shift, const float* residual, float* y, void* workspace, size_t workspace_bytes);
/* The same conv in its Winograd F(4x4,3x3) form (36 multiplies per 4x4 output tile and channel pair: 1.78x less
 * matrix-pipe work again).  A workgroup owns 16 tiles x 64 channels, two workgroups per CU.  y3_conv_wino44_eligible accepts
 * (k = 3, stride 1, no fused upsample input, Cin %% 32 == 0, Cout %% 64 == 0).  w_wino44 = G g G^T with the 6x3 G of the
 * interpolation points 0, +-1, +-2, inf, packed [18 position pairs][cin/8][cout][4 channel pairs][2 positions][2 channels]
 * fp32 (36*cin*cout floats: an opaque layout, what the kernel's 16-byte fragment loads want) by
 * y3_pack_conv_weights_wino44.  Results differ from the direct kernel by fp32 roundings of the transforms (measured on the
 * whole network: boxes 1.0e-5 of the box scale from the fp64 oracle, 6.3e-6 for the direct sum).
 * WORKSPACE (round 6): y3_conv_wino44_workspace_bytes(d) = the bytes of V = B^T d B for this conv (2.25x the input, rounded up
 * to 16-tile blocks).  With a 16-byte-aligned workspace of at least that size the conv runs as TWO kernels - the input
 * transform written once, then 36 batched GEMMs + the output transform (csrc/y3_conv_wino44.hip, form 1) -; with
 * workspace = NULL (or a smaller one) as ONE kernel that transforms inside its K-loop (form 2: rounds 3-5).  Same arithmetic
 * in the same order either way; the workspace needs no initialisation and carries nothing between calls. */
int y3_conv_wino44_eligible(const y3_conv_desc* d);
int y3_conv_wino44_candidate(const y3_conv_desc* d);   /* by shape: the convs worth an F(4x4,3x3) packing beside the F(2x2) one */
int y3_conv_wino44_preferred(const y3_conv_desc* d);   /* for THIS n, h, w: a candidate with enough blocks to fill the CUs */
int y3_pack_conv_weights_wino44(y3_ctx* ctx, const float* w_hwio, int cin, int cout, float* w_wino44);
size_t y3_conv_wino44_workspace_bytes(const y3_conv_desc* d);   /* bytes of V (two-kernel form); workspace = NULL is allowed */
int y3_conv2d_fwd_wino44(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w_wino44, const float* scale,
                         const float* shift, const float* residual, float* y, void* workspace, size_t workspace_bytes);
/* Training uses of the F(4x4,3x3) kernel (train.py:105-115; round 4; the workspace arguments round 6, same rule as above):
 *   y3_conv2d_fwd_wino44_stats: the conv plus the column sums of y and y^2 per 16-tile block - stats
 *     [y3_conv_stats_blocks(d, 2)][2][cout] floats, for y3_bn_train_stats_partials (same contract as
 *     y3_conv2d_fwd_wino_stats: no residual);
 *   y3_pack_conv_weights_wino44_dgrad + y3_conv2d_dgrad_wino44: the data gradient of a stride-1 3x3 conv as the same kernel
 *     on dz with the flipped, channel-swapped kernel (same arguments as y3_conv2d_dgrad_wino; w_wino44_d = 36 * dz_stride *
 *     cin floats; needs dz_stride %% 32 == 0 and cin %% 64 == 0; its workspace is that of the conv [n,h,w,dz_stride] ->
 *     [n,h,w,cin]: y3_conv_wino44_workspace_bytes of fwd with cin = dz_stride, cout = fwd->cin). */
int y3_conv2d_fwd_wino44_stats(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w_wino44, const float* scale,
                               const float* shift, float* y, float* stats, void* workspace, size_t workspace_bytes);
int y3_pack_conv_weights_wino44_dgrad(y3_ctx* ctx, const float* w_d, int cin, int dz_stride, float* w_wino44_d);
int y3_conv2d_dgrad_wino44(y3_ctx* ctx, const y3_conv_desc* fwd, const float* dz, int dz_stride, const float* w_wino44_d,
                           const float* ones, const float* zeros, int accumulate, float* dx, void* workspace,
                           size_t workspace_bytes);

/* ---- fp32 on the bf16 matrix pipe ----------------------------------------------------------------------------
 * Same contract and tensors as y3_conv2d_fwd (fp32 NHWC in, fp32 out, same epilogue, same workspace rule); every
 * fp32 product a*b is rebuilt from bf16 plane products with fp32 accumulation: planes = 3 splits each operand
 * exactly into three bf16 values and keeps the 6 products a_i*b_j, i+j <= 2 (dropped terms <= 2^-23 |ab|, i.e.
 * fp32-level accuracy at 6/16 of the fp32-MFMA cost); planes = 2 keeps 3 products (<= 2^-15 |ab|).
 * w_split = [k*k][cin/16][planes][cout][16] bf16 (cin % 16 == 0) from y3_pack_conv_weights_split (the Cin==3 stem takes the fp32 HWIO
 * kernel and runs the exact kernel).  Replaces the same reference code as y3_conv2d_fwd
 * (utils/layer_utils.py:9-22). */
int y3_pack_conv_weights_split(y3_ctx* ctx, const float* w_hwio, int k, int cin, int cout, int planes,
                               void* w_split);
int y3_conv2d_fwd_split(y3_ctx* ctx, const y3_conv_desc* d, int planes, const float* x, const float* x_up,
                        const void* w_split, const float* scale, const float* shift, const float* residual,
                        float* y, void* workspace, size_t workspace_bytes);

/* ---- unfused graph ops, for callers composing the network op by op (utils/layer_utils.py) ---------
 * y3_net_forward never launches these (it fuses them into the neighbouring convs).
 * y3_upsample_nearest : tf.image.resize_nearest_neighbor, align_corners=False (utils/layer_utils.py:82-87)
 * y3_concat_channels  : tf.concat([a, b], axis=3) on NHWC with `rows` = N*H*W (model.py:62,72)
 * y3_add              : net + shortcut (utils/layer_utils.py:30)
 * y3_reorg_boxes      : box part of reorg_layer for one scale (model.py:96-131):
 *                       boxes [N,gh,gw,3,4] = (cx,cy,w,h) in input pixels; anchors3 = the 3 (w,h) pairs.
 * The first three move 16 bytes per lane: c, ca, cb and count must be multiples of 4 (every channel count of the network
 * is), anything else is Y3_EINVAL before any launch. */
int y3_upsample_nearest(y3_ctx* ctx, const float* x, int n, int h, int w, int c, int out_h, int out_w,
                        float* y);
int y3_concat_channels(y3_ctx* ctx, const float* a, int ca, const float* b, int cb, long long rows, float* y);
int y3_add(y3_ctx* ctx, const float* a, const float* b, long long count, float* y);
int y3_reorg_boxes(y3_ctx* ctx, const float* fm, int n, int gh, int gw, int class_num, int img_h, int img_w,
                   const float* anchors3_host, float* boxes);

/* ---- a6-a8: reorg_layer + predict (+ conf*prob) ------------------------------------------------
 * Replaces model.py:82-137 / :140-190 and the score product of test_single_image.py:55.
 * fm_s: [N, H/stride_s, W/stride_s, 3*(5+C)] for strides 32,16,8 (in that order).
 * anchors: 9 (w,h) pairs in data/yolo_anchors.txt order; scale s uses anchors[6-3s .. 8-3s].
 * boxes [N,B,4] = (x_min,y_min,x_max,y_max); confs [N,B,1]; probs [N,B,C]; scores [N,B,C] or NULL.
 * B = 3*(g1^2+g2^2+g3^2), box order = scale (13,26,52), then y, x, anchor (model.py:155-180).
 * Alignment: any 4-byte boundary is accepted for every pointer.  With fm1..3, boxes, probs and scores (where given) all
 * 16-byte aligned, class_num %% 4 == 0 and class_num <= 248 the LDS-staged kernel runs (16-byte accesses); otherwise the
 * 4-byte-per-lane kernel does, with the same results and more memory transactions - a slower path, not an error. */
int y3_decode(y3_ctx* ctx, const float* fm1, const float* fm2, const float* fm3, int n, int h, int w,
              int class_num, const float* anchors_host18, float* boxes, float* confs, float* probs,
              float* scores);

/* ---- a9/a10: per-class NMS ---------------------------------------------------------------------
 * mode Y3_NMS_TF : utils/nms_utils.py:8-48 `gpu_nms` = per class {score >= thresh,
 *                  tf.image.non_max_suppression (IoU without +1, suppress if IoU > thresh)}.
 * mode Y3_NMS_PY : utils/nms_utils.py:51-123 `cpu_nms`/`py_nms` (+1 on intersection w/h only,
 *                  keep while ovr <= thresh).
 * Tie-break in both modes: (score descending, box index ascending).
 * Batched over n images (the reference handles one image per call; n=1 reproduces it).
 * Outputs per image i, concatenated by class ascending, selection order within a class:
 *   out_boxes [n][cap][4], out_scores [n][cap], out_labels [n][cap] (int32),
 *   out_index [n][cap] (int32 box index into the B inputs; NULL to skip), out_counts [n] (int32),
 *   with cap = class_num * max_boxes.  All device pointers; counts are read by the caller (nothing in the call waits for
 *   the host: copy them back asynchronously and read them when the batch is consumed).  The scratch may be reused by the next
 *   call on the same stream.  Classes with up to 16,384 candidates are selected from keys sorted in the LDS, in chunks, with an
 *   early exit at max_boxes; beyond that, and for max_boxes above ~1,600 (the selected boxes of a class live in the LDS too), an
 *   arg-max form on global memory takes over - same selections either way. */
#define Y3_NMS_TF 0
#define Y3_NMS_PY 1
size_t y3_nms_workspace_bytes(int n, int num_boxes, int class_num, int max_boxes);
int y3_nms(y3_ctx* ctx, int mode, const float* boxes, const float* scores, int n, int num_boxes,
           int class_num, int max_boxes, float score_thresh, float iou_thresh, void* workspace,
           size_t workspace_bytes, float* out_boxes, float* out_scores, int32_t* out_labels,
           int32_t* out_index, int32_t* out_counts);

/* ---- a5: yolov3.forward (model.py:30-80) as one call -------------------------------------------
 * The graph is fixed by class_num: 52 backbone convs (utils/layer_utils.py:24-68) + 23 head convs
 * (model.py:53-78), indexed 0..74 in variable-creation order (= darknet file order).
 * The net decides per layer and input size which kernel runs (y3_net_layer_fused, y3_net_layer_is_streamk) and packs the
 * layers' weights for those kernels itself: the caller hands over the variables, never a packed kernel. */
int y3_net_create(y3_ctx* ctx, int class_num, y3_net** out);
/* The same with an architecture; y3_net_create is architecture 0.  Y3_ARCH_YOLOV3_SPP (darknet's yolov3-spp.cfg): the first
 * yolo_block of the head (f = 512, the 13-grid) becomes
 *     1x1 512, 3x3 1024, 1x1 512, SPP, 1x1 512 (Cin = 2048), 3x3 1024, 1x1 512 (= route), 3x3 1024
 * instead of 1x1 512, 3x3 1024, 1x1 512, 3x3 1024, 1x1 512 (= route), 3x3 1024; the rest of the graph is unchanged.  76 convs,
 * 73 with BN, 371 variables; layer 55 reads spp(output of layer 54) (y3_net_layer_pool; "SPP" below).  Conv outputs stay
 * the only tensors: the pooled input lives in the workspace for its layer only.  An unknown architecture is Y3_EINVAL. */
#define Y3_ARCH_YOLOV3 0
#define Y3_ARCH_YOLOV3_SPP 1
int y3_net_create_arch(y3_ctx* ctx, int class_num, int arch, y3_net** out);
int y3_net_arch(const y3_net* net);
/* 1: layer i reads spp(src), cin = 4 * channels(src); else 0 */
int y3_net_layer_pool(const y3_net* net, int i);
int y3_net_destroy(y3_net* net);
/* 0 = fp32 (default); 1 = bf16 storage: intermediate activations are bf16, the three feature maps stay fp32; 2 / 3 = fp32
 * tensors with the products on the bf16 matrix pipe (y3_conv2d_fwd_split with planes = 3 / 2); 4 = fp32 with the Winograd
 * kernels for the layers they take: F(4x4,3x3) where y3_conv_wino44_preferred says the launch is large enough (bs=32 at
 * 416x416: yes; bs=4: no), F(2x2,3x3) where y3_conv_wino_eligible holds, the direct kernel elsewhere.  The train step
 * (y3_net_train_*) takes its kernels by the same rules for its own launches.  Unbinds the parameters (y3_net_set_params). */
int y3_net_set_dtype(y3_net* net, int dtype);
int y3_net_num_layers(const y3_net* net);
/* geometry of layer i for input-independent fields: k, stride, cin, cout, has_bn */
int y3_net_layer_info(const y3_net* net, int i, int* k, int* stride, int* cin, int* cout, int* has_bn);
/* The inference parameters.  y3_net_params_bytes (host only) is the size of the buffer they live in; it depends on class_num
 * and the dtype, not on the input size.  y3_net_set_params writes into `params` (256-byte aligned), on the context's stream,
 * every layer's folded batch norm (y3_bn_fold, eps 1e-5; detection convs: scale 1, shift = the bias) and its kernel in every
 * packing the dtype's kernels may read it in at any input size, and binds the net to the buffer.  vars: one y3_train_var per
 * layer (only the variable pointers are read, by the work enqueued here; the g_* fields are ignored); a later change of a
 * variable reaches the net through another call.  vars = NULL: only bind a buffer a net with the same class_num and dtype has filled (nets on several streams
 * share one).  Changing the dtype unbinds; y3_net_forward without bound parameters is Y3_ESTATE. */
size_t y3_net_params_bytes(const y3_net* net);
int y3_net_set_params(y3_net* net, const y3_train_var* vars, void* params, size_t params_bytes);
size_t y3_net_workspace_bytes(const y3_net* net, int n, int h, int w);
/* x [n,h,w,3] -> fm1 [n,h/32,w/32,3*(5+C)], fm2 (/16), fm3 (/8).  h,w multiples of 32. */
int y3_net_forward(y3_net* net, const float* x, int n, int h, int w, void* workspace,
                   size_t workspace_bytes, float* fm1, float* fm2, float* fm3);
/* Optional per-layer timing with hipEvents on the context stream.  While enabled, every forward (up to
 * 256) records one event per layer boundary; y3_net_get_layer_ms synchronises on the last event, writes
 * the per-layer elapsed ms averaged over the forwards recorded since the previous call, and resets. */
int y3_net_set_profiling(y3_net* net, int enabled);
int y3_net_get_layer_ms(y3_net* net, float* ms, int count);
int y3_net_layer_is_streamk(const y3_net* net, int i, int n, int h, int w);
/* which launches y3_net_forward fuses at this size (dtype as set): 0 = layer i has its own launch; 1 = it runs inside the NEXT
 * layer's launch (its output tensor never reaches memory; its profiled time is 0); 2 = its launch also runs the layer before it
 * (stem + stride-2 conv in the fp32 and bf16 paths, the first residual block in the bf16 path: model.py:34-40 of the reference) */
int y3_net_layer_fused(const y3_net* net, int i, int n, int h, int w);

/* graph topology of y3_net (tensor ids: 0 = network input, 1.. = conv outputs in creation order; -1 = none) */
int y3_net_layer_graph(const y3_net* net, int i, int* src, int* up, int* resid, int* dst, int* act);
int y3_net_num_tensors(const y3_net* net);
int y3_net_tensor_info(const y3_net* net, int t, int* channels, int* sdiv, int* ext);

/* ==== training path (train.py:72-115 of the reference) ==========================
 * All reductions are two-stage with a fixed combination order (no float atomics): deterministic. */

/* K8: batch norm in batch-statistics mode (model.py:35-41 with is_training=True, train.py:74).
 * z [rows][c] raw conv output.  Computes the batch mean / biased variance over rows, writes mean, inv_std
 * = rsqrt(var+eps), the folded scale = gamma*inv_std and shift = beta - mean*scale for y3_bn_apply_fwd, and
 * (if non-NULL) updates the moving statistics in place: moving <- moving*decay + batch*(1-decay), the
 * UNBIASED variance going into moving_var (TF fused batch norm).  scratch: y3_reduce_scratch_bytes(c). */
size_t y3_reduce_scratch_bytes(int c);
int y3_bn_train_stats(y3_ctx* ctx, const float* z, long long rows, int c, const float* gamma, const float* beta,
                      float eps, float decay, float* mean, float* inv_std, float* scale, float* shift,
                      float* moving_mean, float* moving_var, float* scratch);
/* The same statistics without the extra pass over z: the conv entry points below also write, per row block of their
 * output, the column sums of y and y^2 — stats [y3_conv_stats_blocks(d, wino)][2][cout] floats — taken in the conv's
 * epilogue where the tile is in registers (the training forward calls them with scale = 1, shift = 0, act = 0, so y = z);
 * y3_bn_train_stats_partials then finishes exactly like y3_bn_train_stats (fixed-order fp64 combination: deterministic).
 * y3_conv_stats_blocks returns 0 for convs without this support (the Cin = 3 stem, Cout %% 4 != 0, fused upsample
 * inputs; wino = 1: convs y3_conv_wino_eligible rejects; wino = 2: the F(4x4,3x3) kernel, convs y3_conv_wino44_eligible
 * rejects).  Same arguments as y3_conv2d_fwd / y3_conv2d_fwd_wino otherwise (no x_up, no residual). */
int y3_conv_stats_blocks(const y3_conv_desc* d, int wino);
int y3_conv2d_fwd_stats(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w, const float* scale,
                        const float* shift, float* y, float* stats, void* workspace, size_t workspace_bytes);
int y3_conv2d_fwd_wino_stats(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w_wino, const float* scale,
                             const float* shift, float* y, float* stats, void* workspace, size_t workspace_bytes);
int y3_bn_train_stats_partials(y3_ctx* ctx, const float* partial, int nblocks, long long rows, int c,
                               const float* gamma, const float* beta, float eps, float decay, float* mean,
                               float* inv_std, float* scale, float* shift, float* moving_mean, float* moving_var);
/* y = act(z*scale + shift) + residual   (act: 1 = LeakyReLU(0.1); residual may be NULL) */
int y3_bn_apply_fwd(y3_ctx* ctx, const float* z, const float* scale, const float* shift, const float* residual,
                    long long rows, int c, int act, float* y);
/* Backward of leaky(BN_train(z)): given dy, writes d gamma, d beta and dz (dz may alias dy).
 * scratch: y3_bn_bwd_scratch_bytes(c). */
size_t y3_bn_bwd_scratch_bytes(int c);
int y3_bn_train_bwd(y3_ctx* ctx, const float* z, const float* dy, const float* gamma, const float* scale,
                    const float* shift, const float* mean, const float* inv_std, long long rows, int c,
                    float* dgamma, float* dbeta, float* dz, float* scratch);
/* d bias = sum over rows of dy [rows][c] (detection convs, model.py:55-57); scratch: 1024*c floats */
int y3_bias_grad(y3_ctx* ctx, const float* dy, long long rows, int c, float* dbias, float* scratch);

/* K9: conv backward (TF autodiff of slim.conv2d, train.py:112).  `fwd` describes the FORWARD layer
 * (n,h,w = its input size; c_up must be 0: training materialises the upsample+concat).
 * dgrad: dx [n,h,w,cin] (+)= data gradient.  dz is [n,h/s,w/s] x dz_stride channels (dz_stride >= cout,
 *        multiple of 32: the 3*(5+C) detection convs pad to the next multiple), w_d = the HWIO kernel with
 *        its last axis padded to dz_stride ([k*k][cin][dz_stride]); `ones`/`zeros` are [cin] device vectors.
 *        workspace (NULL is allowed): that of the conv as launched, [n,h/s,w/s,dz_stride] -> cin at stride 1:
 *        y3_conv_workspace_bytes of that conv (the Winograd forms below: their own size function of it).
 * wgrad: dw_hwio [k][k][cin][cout] = weight gradient; scratch: y3_conv_wgrad_scratch_bytes(fwd), 16-byte aligned
 *        (dw_hwio itself: any 4-byte boundary - also for y3_conv_wgrad_wino and y3_conv_wgrad_bf16 below: the train step
 *        writes every weight gradient at flat_grad + its element offset).  The Cin = 3 stem: dz_stride = cout = 32 only. */
int y3_conv2d_dgrad(y3_ctx* ctx, const y3_conv_desc* fwd, const float* dz, int dz_stride, const float* w_d,
                    const float* ones, const float* zeros, int accumulate, float* dx, void* workspace,
                    size_t workspace_bytes);
/* The data gradient of a stride-1 1x1 conv whose dx IS the dy of the batch-norm layer below it, with that layer's backward
 * reduction taken in the epilogue where the tile is in registers (the backward twin of y3_conv2d_fwd_stats): dx as
 * y3_conv2d_dgrad writes it, and partial [y3_conv_dgrad_bn_blocks(fwd)][2][cin] = per row block of dx, the column sums of
 * g' = dx * leaky'(z*scale + shift) and of g' * (z - mean) * inv_std (dx = the stored sum when accumulate != 0).  bn_z
 * [n*h*w][cin] is that layer's raw conv output, bn_vec [4][cin] its mean / inv_std / folded scale / folded shift as
 * y3_bn_train_stats wrote them.  y3_conv_dgrad_bn_blocks returns 0 where there is no such kernel (3x3 or stride-2 convs,
 * fused upsample inputs, cin %% 4 != 0); y3_conv2d_dgrad_bn then returns Y3_EINVAL and writes nothing.
 * y3_bn_train_bwd_partials is y3_bn_train_bwd with the reduction already done (partial: [nblocks][2][c], combined in a fixed
 * order in fp64): dgamma, dbeta and dz; same scratch. */
int y3_conv_dgrad_bn_blocks(const y3_conv_desc* fwd);
int y3_conv2d_dgrad_bn(y3_ctx* ctx, const y3_conv_desc* fwd, const float* dz, int dz_stride, const float* w_d,
                       const float* ones, const float* zeros, int accumulate, float* dx, const float* bn_z,
                       const float* bn_vec, float* partial);
int y3_bn_train_bwd_partials(y3_ctx* ctx, const float* z, const float* dy, const float* gamma, const float* scale,
                             const float* shift, const float* mean, const float* inv_std, long long rows, int c,
                             const float* partial, int nblocks, float* dgamma, float* dbeta, float* dz, float* scratch);
/* Synchronised batch norm: the two finalizes above cut in two, with a caller-owned device buffer between the halves,
 *   sums = double[2*c + 1]: [0:c) and [c:2c) the two column sums over this rank's rows, [2c] the row count,
 * so that ONE sum of the buffer over ranks (between the halves, on the context's stream) yields the sums and the count of the
 * global batch.  With the buffer left alone, sums-then-finish writes bit for bit what the one-call entries write.
 *   stats_sums    (sum z, sum z^2): of partial [nblocks][2][c] where the conv epilogue took them (y3_bn_train_stats_partials'
 *                 argument; z and scratch unused), else, partial NULL, of z [rows][c] (fp32, or bf16 when z_bf16; c %% 4 == 0)
 *                 through scratch (y3_reduce_scratch_bytes(c)).
 *   stats_finish  y3_bn_train_stats from the sums on: mean, inv_std, scale, shift, and the moving statistics, the unbiased
 *                 factor count / (count - 1) taken of the count in the buffer (the global one after an exchange).
 *   bwd_sums      (sum g', sum g' * zhat) as y3_bn_train_bwd / _partials reduce them (partial NULL / given), written to the buffer,
 *                 and dgamma / dbeta (either may be NULL) from THIS rank's sums: each rank's loss is a mean over its own images
 *                 and the gradient exchange averages over ranks, so the parameter gradients stay local (their average is the
 *                 gradient of the global mean loss); all-reduced sums there would come out world times too large.
 *   bwd_finish    the coefficients from the (exchanged) buffer, then the unchanged apply pass: dz (may alias dy; bf16 when z_bf16).
 *                 scratch: the same y3_bn_bwd_scratch_bytes(c) buffer bwd_sums was given. */
int y3_bn_sync_stats_sums(y3_ctx* ctx, const void* z, int z_bf16, const float* partial, int nblocks, long long rows, int c,
                          double* sums, float* scratch);
int y3_bn_sync_stats_finish(y3_ctx* ctx, const double* sums, int c, const float* gamma, const float* beta, float eps, float decay,
                            float* mean, float* inv_std, float* scale, float* shift, float* moving_mean, float* moving_var);
int y3_bn_sync_bwd_sums(y3_ctx* ctx, const void* z, int z_bf16, const float* dy, const float* scale, const float* shift,
                        const float* mean, const float* inv_std, long long rows, int c, const float* partial, int nblocks,
                        float* dgamma, float* dbeta, double* sums, float* scratch);
int y3_bn_sync_bwd_finish(y3_ctx* ctx, const void* z, int z_bf16, const float* dy, const float* gamma, const float* scale,
                          const float* shift, const float* mean, const float* inv_std, long long rows, int c, const double* sums,
                          void* dz, float* scratch);
/* Which schedule a launch of the exact-fp32 conv family takes (host arithmetic, no device): 0 = one workgroup per tile,
 * 1 = stream-K (3x3 convs on 128x128 tiles, needs the workspace), 2 = the resident walk of the 64x64 tiles (1,024 workgroups
 * walking runs of whole tiles).  `conv` is the conv as launched: for a data gradient [n,h,w,dz_stride] -> fwd cin at stride
 * 1; tmode_taps = 1, 2 or 4 asks for one parity class of a stride-2 3x3 data gradient (h, w = the coarse map), else 0. */
int y3_conv_schedule(const y3_conv_desc* conv, int tmode_taps, int with_workspace);
/* The same data gradient on the bf16 matrix pipe (stride-1 convs; see y3_conv2d_fwd_split): w_split_d comes from
 * y3_pack_conv_weights_split_dgrad(w_d = the [k*k][cin][dz_stride] kernel above). */
int y3_pack_conv_weights_split_dgrad(y3_ctx* ctx, const float* w_d, int k, int cin, int dz_stride, int planes,
                                     void* w_split_d);
int y3_conv2d_dgrad_split(y3_ctx* ctx, const y3_conv_desc* fwd, int planes, const float* dz, int dz_stride,
                          const void* w_split_d, const float* ones, const float* zeros, int accumulate, float* dx,
                          void* workspace, size_t workspace_bytes);
/* The same data gradient in Winograd F(2x2,3x3) form (stride-1 3x3 convs with Cin %% 32 == 0 and dz_stride %% 32 == 0;
 * the gradient of a SAME stride-1 conv is a SAME stride-1 conv with the flipped, channel-swapped kernel, so the forward
 * Winograd kernel runs it): w_wino_d = 16 * dz_stride * cin floats from y3_pack_conv_weights_wino_dgrad(w_d = the
 * [k*k][cin][dz_stride] kernel above); workspace as y3_conv_wino_workspace_bytes of the [n,h,w,dz_stride]->[..,cin] conv. */
int y3_pack_conv_weights_wino_dgrad(y3_ctx* ctx, const float* w_d, int cin, int dz_stride, float* w_wino_d);
int y3_conv2d_dgrad_wino(y3_ctx* ctx, const y3_conv_desc* fwd, const float* dz, int dz_stride, const float* w_wino_d,
                         const float* ones, const float* zeros, int accumulate, float* dx, void* workspace,
                         size_t workspace_bytes);
size_t y3_conv_wgrad_scratch_bytes(const y3_conv_desc* fwd);
int y3_conv_wgrad(y3_ctx* ctx, const y3_conv_desc* fwd, const float* x, const float* dz, int dz_stride,
                  float* dw_hwio, void* scratch, size_t scratch_bytes);
/* The kernels of the bf16 train step (net dtype 1; numerics contract: the train-step block below).  bf16 tensors are
 * 16-bit words (round to nearest even); `fwd` describes the FORWARD layer as for y3_conv2d_dgrad (c_up = 0, act ignored).
 * pack_bf16_train: the kernel as those convs read it: dgrad_stride 0 -> the forward's ([k*k*cin*cout] bf16), else the data
 *        gradient's: flipped, channel axes swapped, its reduction zero-extended to dgrad_stride ([k*k*dgrad_stride*cin]).
 * train_fwd_bf16: z [n,ho,wo,cout] bf16 = conv(x bf16, w) with no scale / shift / activation, and stats
 *        [y3_conv_train_stats_blocks_bf16(fwd)][2][cout] = per row block (sum z, sum z^2) of z AS STORED
 *        (y3_bn_train_stats_partials finalises them).  cin % 32 == 0, cout % 4 == 0.
 * dgrad_bf16: dx [n,h,w,cin] fp32 (+)= data gradient of dz [n,ho,wo,dz_stride] bf16 (stride 1 or the stride-2 3x3).
 * wgrad_bf16: dw_hwio [k][k][cin][cout] fp32 from x [n,h,w,cin] bf16 and dz bf16 (row stride dz_stride >= cout);
 *        scratch: y3_conv_wgrad_bf16_scratch_bytes(fwd) (0: none needed).  Fixed summation order.
 * bn_apply_fwd_bf16: y bf16 = leaky(z*scale + shift) (+ residual bf16); z bf16, or fp32 when z_f32.
 * bn_train_bwd_bf16: y3_bn_train_bwd with z bf16 and dz bf16 (dy, dgamma, dbeta fp32); scratch y3_bn_bwd_scratch_bytes(c).
 * upsample_concat_bf16: out [n,h,w,cu+cx] = concat(upsample2x(up [n,h/2,w/2,cu]), x [n,h,w,cx]), bf16.
 * f32_to_bf16: count (a multiple of 4) values rounded to nearest even; +-Inf stay, every NaN stays a (quiet) NaN. */
int y3_pack_conv_weights_bf16_train(y3_ctx* ctx, const float* w_hwio, int k, int cin, int cout, int dgrad_stride,
                                    void* w_packed);
int y3_conv_train_stats_blocks_bf16(const y3_conv_desc* fwd);
int y3_conv2d_train_fwd_bf16(y3_ctx* ctx, const y3_conv_desc* fwd, const void* x, const void* w_packed, void* z,
                             float* stats);
int y3_conv2d_dgrad_bf16(y3_ctx* ctx, const y3_conv_desc* fwd, const void* dz, int dz_stride, const void* w_packed_d,
                         int accumulate, float* dx);
size_t y3_conv_wgrad_bf16_scratch_bytes(const y3_conv_desc* fwd);
int y3_conv_wgrad_bf16(y3_ctx* ctx, const y3_conv_desc* fwd, const void* x, const void* dz, int dz_stride, float* dw_hwio,
                       void* scratch, size_t scratch_bytes);
int y3_bn_apply_fwd_bf16(y3_ctx* ctx, const void* z, int z_f32, const float* scale, const float* shift, const void* residual,
                         long long rows, int c, void* y);
int y3_bn_train_bwd_bf16(y3_ctx* ctx, const void* z, const float* dy, const float* gamma, const float* scale, const float* shift,
                         const float* mean, const float* inv_std, long long rows, int c, float* dgamma, float* dbeta, void* dz,
                         float* scratch);
int y3_upsample_concat_bf16(y3_ctx* ctx, const void* up, int cu, const void* x, int cx, int n, int h, int w, void* out);
int y3_f32_to_bf16(y3_ctx* ctx, const float* src, long long count, void* dst);
/* The weight gradient of a stride-1 3x3 conv in Winograd F(2x2,3x3) form (Cin %% 64 == 0, Cout %% 64 == 0, at least
 * 8 / ceil(w/2) + 1 rows of 2x2 tiles per image — y3_conv_wgrad_wino_eligible says):
 *   dw = G^T [ sum over 2x2 output tiles of (B^T d B) .* (A dY A^T) ] G,
 * exact fp32 arithmetic with 16/36 of the multiplies of y3_conv_wgrad; results differ from it by a few fp32 roundings
 * per term; deterministic (the tile range is split over workgroups, partial kernels are added in a fixed order).
 * scratch: y3_conv_wgrad_wino_scratch_bytes(fwd), 16-byte aligned. */
int y3_conv_wgrad_wino_eligible(const y3_conv_desc* fwd);
size_t y3_conv_wgrad_wino_scratch_bytes(const y3_conv_desc* fwd);
int y3_conv_wgrad_wino(y3_ctx* ctx, const y3_conv_desc* fwd, const float* x, const float* dz, int dz_stride,
                       float* dw_hwio, void* scratch, size_t scratch_bytes);
/* backward routing: 2x2 sum of the gradient of a nearest-upsampled tensor (g has g_channels per pixel, the
 * first c belong to the upsampled part), channel-slice (accumulate), zero-extension of the channel axis */
int y3_upsample2x_bwd(y3_ctx* ctx, const float* g, int g_channels, int n, int h, int w, int c, int accumulate,
                      float* dx);
int y3_slice_accumulate(y3_ctx* ctx, const float* src, int src_channels, int offset, long long rows, int c,
                        int accumulate, float* dst);
int y3_pad_channels(y3_ctx* ctx, const float* src, int c_src, long long rows, int c_dst, float* dst);

/* K10: loss_layer forward + backward for one scale (model.py:192-304, box_iou :307-345).
 * feature_map [n,gh,gw,3*(5+C)], y_true [n,gh,gw,3,6+C] (utils/data_utils.py:69-113 layout), anchors3 = the
 * 3 (w,h) pairs of this scale.  loss4 (device, 4 floats: xy, wh, conf, class; each already divided by N)
 * is overwritten or accumulated; grad [n,gh,gw] x grad_stride receives d(sum of the four)/d(feature_map): the first
 * 3*(5+C) floats of each row are written, the pad lanes behind them are left as they were.
 * The ignore mask takes the best IoU over every ground-truth box of the image on this scale: there is no limit on their
 * number (up to gh*gw*3, one per record), and the result does not depend on the order in which the boxes were collected,
 * so it is the same bits from run to run.
 *
 * IoU box losses (y3_loss_layer_box; y3_loss_layer is its box_loss = Y3_BOX_MSE call).  Y3_BOX_MSE keeps the reference's
 * box terms: squared error of the cell offset (xy) and of log(w / anchor) (wh), each weighted by 2 - area.  Under an IoU
 * kind ONE box term replaces the two.  For a record with object_mask != 0, with the predicted box (px, py, pw, ph) in
 * pixels as the reference's reorg_layer decodes it (px = (sigmoid(f0) + gx) * ratio_w, pw = exp(f2) * anchor_w, likewise
 * y / h) and the true box (tx, ty, tw, th) = y_true[0:4]:
 *   corners  c -+ s/2:  p1x = px - pw/2, p2x = px + pw/2, ... t2y = ty + th/2
 *   inter = max(min(p2x,t2x) - max(p1x,t1x), 0) * max(min(p2y,t2y) - max(p1y,t1y), 0)
 *   union = pw*ph + tw*th - inter + 1e-10,  iou = inter / union                          (as box_iou, model.py:307-345)
 *   cw = max(p2x,t2x) - min(p1x,t1x),  ch = max(p2y,t2y) - min(p1y,t1y)                  (the enclosing box)
 *   GIoU = iou - (cw*ch - union) / (cw*ch + 1e-10)
 *   DIoU = iou - ((px-tx)^2 + (py-ty)^2) / (cw^2 + ch^2 + 1e-10)
 *   CIoU = DIoU - alpha*v,  v = (4/pi^2) * (atan(tw/th) - atan(pw/ph))^2,  alpha = v / (1 - iou + v + 1e-10)
 *   box term = sum over records of (1 - X) * object_mask * (2 - (tw/img_w)*(th/img_h)) * mixup_weight / N,  X the kind's
 * quantity: the weight is the one the two squared-error terms carry.  alpha is a CONSTANT in the gradient (stop-gradient, as
 * in the CIoU paper's implementation); the gradient w.r.t. f[0..3] runs through the decode (d px / d f0 = s(1-s) * ratio_w,
 * d pw / d f2 = pw); at a tie of a min / max it is that of either side.  A record with object_mask == 0 contributes exactly
 * 0 to the term and gets exactly 0 in its four box lanes whatever its logits hold (exp(f2) = inf included): no NaN or inf
 * reaches loss4 or grad from it.  The box term is reported in the xy slot of loss4 / loss5 and the wh slot is exactly 0.0f;
 * the total stays the sum of the slots.  The conf and class terms and the ignore mask (plain IoU) do not depend on the kind:
 * their slots and gradient lanes are the same bits under every kind.  An unknown kind is Y3_EINVAL before any launch.
 *
 * Conf rule (y3_loss_layer_conf; y3_loss_layer_box is its ignore_thresh = 0.5f, obj_iou_ratio = 0.f call, the reference's
 * rule).  Two numbers decide what the objectness logit x = f[4] of a record is trained towards:
 *   ignore = (best < ignore_thresh), best the record's largest plain IoU with the image's true boxes of this scale, computed
 *            exactly as for the reference's 0.5 (darknet's yolov3.cfg: ignore_thresh = .7);
 *   z      = the target.  object_mask == 0: z = 0 (selected, not multiplied).  object_mask != 0, with r = obj_iou_ratio:
 *            z = (1 - r) + r * q,  q = the plain iou above (box_iou) of the record's decoded prediction with its OWN true box
 *            y_true[0:4]; a q that is NaN, infinite or below 0 counts as 0 (a saturated f[2] gives inf / inf).  q is a
 *            CONSTANT of the gradient (stop-gradient), under every box_loss kind.
 *   conf term = sum over records of cmask * bce(z, x) * mixup_weight / N,  cmask = m + (1 - m) * ignore,  m = object_mask,
 *            bce(z, x) = max(x, 0) - x z + log(1 + exp(-|x|));  d/dx = cmask * (sigmoid(x) - z).  With use_focal_loss the
 *            factor is (z - sigmoid(x))^2 and its derivative follows.
 * The box, class and mix-up arithmetic does not depend on either number.  With r == 0 the kernel is the one without the
 * option (a template parameter), and (0.5f, 0.f) gives the bits of y3_loss_layer_box for every kind.  ignore_thresh or
 * obj_iou_ratio outside [0, 1], NaN included, is Y3_EINVAL before any launch. */
#define Y3_BOX_MSE 0
#define Y3_BOX_GIOU 1
#define Y3_BOX_DIOU 2
#define Y3_BOX_CIOU 3
size_t y3_loss_scratch_bytes(int n, int gh, int gw);
int y3_loss_layer(y3_ctx* ctx, const float* feature_map, const float* y_true, int n, int gh, int gw,
                  int class_num, int img_h, int img_w, const float* anchors3_host, int use_label_smooth,
                  int use_focal_loss, int accumulate, float* loss4, float* grad, int grad_stride, void* scratch,
                  size_t scratch_bytes);
int y3_loss_layer_box(y3_ctx* ctx, const float* feature_map, const float* y_true, int n, int gh, int gw,
                      int class_num, int img_h, int img_w, const float* anchors3_host, int use_label_smooth,
                      int use_focal_loss, int box_loss, int accumulate, float* loss4, float* grad, int grad_stride,
                      void* scratch, size_t scratch_bytes);
int y3_loss_layer_conf(y3_ctx* ctx, const float* feature_map, const float* y_true, int n, int gh, int gw,
                       int class_num, int img_h, int img_w, const float* anchors3_host, int use_label_smooth,
                       int use_focal_loss, int box_loss, float ignore_thresh, float obj_iou_ratio, int accumulate,
                       float* loss4, float* grad, int grad_stride, void* scratch, size_t scratch_bytes);

/* ---- a14 as ONE call: the train step of train.py:72-115 on the y3_net graph ---------------------------------------
 * The per-op entry points above, sequenced by the library over a caller-owned workspace (whole-graph entries;
 * a host in any language trains through these without re-implementing the backward walk):
 *   y3_net_train_forward   yolov3.forward(inputs, is_training=True) (model.py:30-80): batch-statistics BN in all 72 BN
 *                          layers, moving statistics updated in place (decay = opts->bn_decay, unbiased variance), the
 *                          tensors backward needs are kept in the workspace; *fm1..3 = the feature maps (inside it)
 *   y3_net_train_loss      yolov3.compute_loss(y_pred, y_true) (model.py:348-365): loss5 (device, 5 floats) = [total, xy,
 *                          wh, conf, class]; d total / d feature_map_i stays in the workspace
 *   y3_net_train_backward  the gradients of loss[0] w.r.t. every variable whose g_* offset is >= 0, written to
 *                          flat_grad + offset (train.py:112 compute_gradients; the L2 term, the per-tensor clip and the
 *                          update are y3_clip_update_multi's).  Gradients do not flow below the first layer that holds a
 *                          trainable variable (train.py:82 update_vars).  `ready(user, g_end)` is called right after the
 *                          kernels that complete layer i's gradients have been enqueued (layers are visited last to
 *                          first): the hook a data-parallel caller hangs its bucketed all-reduce on; may be NULL.
 *                          Re-runnable from the same forward / loss state.
 *   y3_net_train_step      forward + loss + backward in one call.
 * The net's dtype picks the kernels: 0 direct fp32, 4 Winograd forms of the stride-1 3x3 convs (forward, data AND weight
 * gradient), 2 / 3 products on the bf16 matrix pipe (all four fp32-accurate), 1 mixed precision on the bf16 matrix pipe.
 * dtype 1: rounded once (nearest even) to bf16 where stored: every saved raw conv output z, every activation and the
 * materialised upsample+concat inputs, the packed weights, and dz (the conv-gradient operand the BN backward writes).  fp32:
 * every MFMA accumulation, the BN batch and moving statistics (those of z AS STORED, summed in fp32), the feature maps, the
 * loss and d loss / d fm, every activation gradient dy (accumulated across a tensor's consumers), the weight / gamma / beta /
 * bias gradients, the variables and the optimizer.  No loss scaling (bf16 has fp32's exponent range).  The Cin = 3 stem
 * keeps the fp32 conv, z, statistics, BN backward and weight gradient (only its output is bf16); the detection convs write
 * fp32 feature maps with their bias, and their dz is d loss / d fm rounded once to bf16 (the bias gradient reads it in fp32).
 * y3_net_train_saved_type tells the element type of a layer's saved z.  Variables are plain device pointers
 * in layer order (y3_net_layer_info): HWIO kernel, BN gamma / beta / moving mean / moving variance or the bias.
 * workspace: y3_net_train_workspace_bytes(net, vars, n, h, w) bytes (it depends on which variables are trainable),
 * 256-byte aligned, untouched by the caller between forward and backward.  Deterministic (fixed reduction orders). */
struct y3_train_var {
    float* weights;
    float *gamma, *beta, *moving_mean, *moving_variance;   /* BN layers (NULL otherwise) */
    float* biases;                                         /* detection convs (NULL otherwise) */
    long long g_weights, g_gamma, g_beta, g_biases;        /* element offsets into flat_grad; < 0: not trainable */
    long long g_end;                                       /* passed to `ready` once this layer's gradients are enqueued; < 0: no call */
};
typedef struct y3_train_opts {
    float bn_decay;                    /* model.py:36 batch_norm_decay */
    int use_label_smooth, use_focal_loss;
    const float* anchors;              /* HOST pointer: the 9 (w,h) anchor pairs, smallest first (utils/misc_utils.py:31-37) */
} y3_train_opts;
typedef void (*y3_grad_ready_fn)(void* user, long long g_end);
size_t y3_net_train_workspace_bytes(y3_net* net, const y3_train_var* vars, int n, int h, int w);
int y3_net_train_forward(y3_net* net, const y3_train_var* vars, const float* x, int n, int h, int w,
                         const y3_train_opts* opts, void* workspace, size_t workspace_bytes, float** fm1, float** fm2,
                         float** fm3);
int y3_net_train_loss(y3_net* net, const float* y_true_1, const float* y_true_2, const float* y_true_3,
                      const y3_train_opts* opts, float* loss5);
int y3_net_train_backward(y3_net* net, const y3_train_var* vars, float* flat_grad, y3_grad_ready_fn ready, void* user);
int y3_net_train_step(y3_net* net, const y3_train_var* vars, const float* x, int n, int h, int w, const float* y_true_1,
                      const float* y_true_2, const float* y_true_3, const y3_train_opts* opts, float* flat_grad,
                      void* workspace, size_t workspace_bytes, float* loss5, y3_grad_ready_fn ready, void* user);
/* Optional second stream for backward: a layer's weight gradient is off the critical path of the pass (only the optimizer
 * reads it), its data gradient and the BN backward below it are on it.  With a stream set here (a hipStream_t of the net's
 * device, not the context's; NULL switches it off) the weight gradients run there, ordered against the context's stream by
 * events, and overlap the HBM-bound BN passes of the next layer.  Everything the caller sees keeps its stream order:
 * `ready(g_end)` is called once the context's stream has been made to wait for every weight gradient in flat_grad[0:g_end)
 * (the calls come in increasing g_end order, whichever variables are trainable), and backward
 * returns with the context's stream waiting for all of them.  The workspace is a little larger (one layer's dz lives one
 * layer longer): size it after this call.  Y3_OWN_STREAM: the library creates (once per net, destroyed with it) a stream of
 * the device's LOWEST priority for it - the recommended form: the weight gradient is the work that can wait, and a stream
 * of another priority cannot share the hardware queue of the context's stream (an ordinary stream of the caller's can,
 * once enough streams are alive in the process; the event waits then serialise inside one queue and the step gets slower
 * than on one stream). */
#define Y3_OWN_STREAM ((void*)(size_t)1)
int y3_net_train_set_wgrad_stream(y3_net* net, void* stream);
/* The box term of y3_net_train_loss / _step (a Y3_BOX_* kind, defined at y3_loss_layer_box), for all three scales; a new net
 * has Y3_BOX_MSE.  Valid for every net dtype (the loss of the bf16 step is fp32 too); launches nothing and leaves the
 * workspace size as it was.  An unknown kind is Y3_EINVAL and the net keeps the kind it had. */
int y3_net_train_set_box_loss(y3_net* net, int box_loss);
/* The conf rule of y3_net_train_loss / _step (ignore_thresh and obj_iou_ratio, defined at y3_loss_layer_conf), for all three
 * scales; a new net has (0.5f, 0.f), the reference's.  Valid for every net dtype; launches nothing and leaves the workspace
 * size as it was.  A value outside [0, 1] (NaN included) is Y3_EINVAL and the net keeps both values it had. */
int y3_net_train_set_conf_rule(y3_net* net, float ignore_thresh, float obj_iou_ratio);
/* Optional synchronised batch norm for a data-parallel caller (off by default; a NULL fn switches it off again).  With a hook
 * set, y3_net_train_forward / _backward / _step run every BN layer's finalize as its two halves (y3_bn_sync_*): the sums half
 * is enqueued on the context's stream into exchange_dev, fn(user, layer, phase, doubles) is called on the host thread (phase 0
 * forward, 1 backward; doubles = 2 * cout + 1), then the finish half is enqueued.  On return from fn, work enqueued LATER on
 * the context's stream must see exchange_dev[0:doubles) summed over ranks (the `ready` hook's contract: order the collective
 * behind the stream, and the stream behind the collective).  One buffer serves every layer - all of it is ordered on that
 * stream; it is the caller's, of at least (2 * 1024 + 1) * 8 bytes (else Y3_EINVAL).  fn is not called while the workspace is
 * sized, nor, in backward, for layers below the first trainable one; the calls come in layer order in forward and in reverse
 * in backward - the same sequence on every rank that runs the same variable table and input size.  A nonzero return ends the
 * call with Y3_ESTATE.  The weight gradients (and their second stream) are untouched; parameter gradients stay per rank (to be
 * averaged by the caller), dz and the statistics - the moving ones included - are those of the global batch. */
typedef int (*y3_bn_sync_fn)(void* user, int layer, int phase, int doubles);
int y3_net_train_set_bn_sync(y3_net* net, y3_bn_sync_fn fn, void* user, double* exchange_dev, size_t exchange_bytes);
/* test hook: byte offsets inside the last forward's workspace of layer i's raw conv output z and of its [4][cout]
 * mean / inv_std / folded scale / folded shift (the tensors that fix the LeakyReLU branches); SIZE_MAX for non-BN layers */
int y3_net_train_saved(const y3_net* net, int layer, size_t* z_offset, size_t* stats_offset);
/* the element type of that z: 1 bf16 (net dtype 1, every BN layer but the Cin = 3 stem), 0 fp32 */
int y3_net_train_saved_type(const y3_net* net, int layer);
/* test hook: the byte offset inside the last forward's workspace of a pool layer's materialised spp(x) [n,h,w,4c] (bf16 in net
 * dtype 1, else fp32); SIZE_MAX for every other layer */
int y3_net_train_saved_pool(const y3_net* net, int layer, size_t* offset);

/* ---- SPP: the spatial pyramid pooling block of YOLOv3-SPP ------------------------------------------------------------
 * For an NHWC tensor x [n,h,w,c] (fp32 or bf16):
 *   mp_k(x)[n,y,x',ch] = the maximum of x[n,y+dy,x'+dx,ch] over |dy|,|dx| <= k/2, restricted to positions inside the map
 *                        (max-pool k x k, stride 1, with padding that never wins);
 *   spp(x) = concat_channels([mp_13(x), mp_9(x), mp_5(x), x]), shape [n,h,w,4c]  (yolov3-spp.cfg's route -1,-3,-5,-6).
 * Max is exact: spp is exact in fp32 and in bf16, every output equals one input element bit for bit.  mp_9 = mp_5 o mp_5 and
 * mp_13 = mp_5 o mp_5 o mp_5 hold exactly; the kernel uses that.  Inputs are finite; NaN behaviour is unspecified.
 * Backward, with g [n,h,w,4c] in fp32 and x as stored: the window of (q, ch, k) sends its gradient to the FIRST position, in
 * row-major order of the window (y ascending, then x ascending), whose stored value equals the window's maximum (torch's CPU
 * max_pool2d rule; ties are not rare in bf16).  With slot(13) = 0, slot(9) = 1, slot(5) = 2:
 *   dx[p,ch] = g[p,3c+ch] + sum_{k=5,9,13} sum_{q : argmax_k(q,ch) = p} g[q, slot(k)*c+ch]
 * summed in fp32 in exactly this order: the identity term first, then k = 5, 9, 13, and within a k the q in row-major order.
 * accumulate != 0: the finished sum is added to what dx held; otherwise it overwrites.  No floating-point atomics: the same
 * bits on every run.
 * y3_spp_fwd: out [n,h,w,4c] in x's type, one launch that writes all four slots.  y3_spp_bwd: one launch that recomputes the
 * argmax from x (no index tensor); x_stride is the channel stride of x in elements, so that x may be the last slot of a
 * materialised spp(x) (x + 3c, stride 4c); dx [n,h,w,c] fp32.  c % 8 == 0, x_stride % 8 == 0, n,h,w,c > 0, any h and w;
 * pointers 16-byte aligned; element offsets are 64-bit.  Bad arguments are Y3_EINVAL before any launch. */
int y3_spp_fwd(y3_ctx* ctx, const void* x, int bf16, int n, int h, int w, int c, void* out);
int y3_spp_bwd(y3_ctx* ctx, const void* x, int x_stride, int bf16, const float* g, int n, int h, int w, int c,
               int accumulate, float* dx);

/* ---- next row 8(f)#1: target assignment on the device (utils/data_utils.py:51-115 `process_box`) ------------
 * boxes [n][kmax][5] = (x_min,y_min,x_max,y_max,mix_weight) in resized-image pixels, labels [n][kmax] int32,
 * counts [n] int32 (boxes actually present per image), anchors: 9 (w,h) pairs.  Writes the three y_true
 * tensors [n][g][g][3][6+C] (zero, mix weight 1, then the per-box entries in box order).
 *
 * Multi-anchor positives (y3_process_box_multi; y3_process_box is its assign_iou_thresh = 1 call, the option off; darknet's
 * yolov3.cfg calls the threshold iou_thresh and uses 0.213).  Per image, boxes are taken in order.  For box i, with
 * (bw, bh) = (x_max - x_min, y_max - y_min) and centre (cx, cy), the nine shape IoUs are computed in float32, in numpy's
 * operation order:
 *   w_k = min(bw/2, aw_k/2) - max(-bw/2, -aw_k/2),  h_k likewise,  iou_k = (w_k h_k) / (bw bh + aw_k ah_k - w_k h_k + 1e-10)
 * and best = the first maximum.  Then for anchor k = 0..8 ASCENDING: if k == best, or iou_k > assign_iou_thresh (a float32
 * compare), the record (scale of k: stride 8, 16, 32 for k / 3 = 0, 1, 2;  cell (floor(cx / stride), floor(cy / stride));
 * anchor slot k % 3) is written as the single record is today: the four box fields (cx, cy, bw, bh), mask 1 and the mix
 * weight are written, the class one-hot bit is set and never cleared, a centre outside that scale's grid skips that write,
 * and a later write overwrites an earlier one, whichever box or anchor made it.  That order is the definition: one thread
 * walks an image, no atomics, the same bytes on every run.  assign_iou_thresh >= 1 writes the best anchor only (a shape IoU
 * never exceeds 1): y3_process_box's output bit for bit.  A threshold <= 0 or NaN is Y3_EINVAL before any launch.
 * The executable form of this rule is utils.data_utils.process_box_host (numpy float32). */
int y3_process_box(y3_ctx* ctx, const float* boxes, const int32_t* labels, const int32_t* counts, int n, int kmax,
                   int class_num, int img_w, int img_h, const float* anchors_host18, float* y_true_13,
                   float* y_true_26, float* y_true_52);
int y3_process_box_multi(y3_ctx* ctx, const float* boxes, const int32_t* labels, const int32_t* counts, int n, int kmax,
                         int class_num, int img_w, int img_h, const float* anchors_host18, float assign_iou_thresh,
                         float* y_true_13, float* y_true_26, float* y_true_52);

/* ---- row 8(f)#1, the feeder's pixel work on the device (utils/data_utils.py:118-172 parse_data after its draws:
 * mix_up blend, random_color_distort, the crop window of the expanded canvas, cv2.resize with the drawn interpolation,
 * letterbox padding, random_flip, / 255) for a BATCH of samples.  The host half - the draws, the box arithmetic, Pillow's
 * double-precision filter windows and weights - is liby3feed.so's y3f_plan_batch or y3f_plan_batch_src
 * (include/yolo355_feed.h), which writes one relocatable blob per batch; the caller uploads it and passes its device address
 * and size here, together with the host copy of the n y3f_djob records at its start and the y3f_dtables uploaded once per
 * device.  A source whose record says so (y3f_plan_batch_src) is not in the blob but in the caller's device arena src_dev of
 * src_bytes (whole 8-bit RGB images), and is read where it lies; a packed plan passes NULL, 0.
 * Every record is checked before anything is launched: each blob offset plus extent (records, packed sources, jitter maps,
 * tables by their ksize and counts) against blob_bytes, each arena rectangle (img_off + ((r_y0 + r_h - 1) * stride + r_x0 +
 * r_w) * 3, stride >= r_x0 + r_w) against src_bytes, live inside win, the scratch extents; anything out of range is
 * Y3_EINVAL naming the job.  The kernels read the records from the copy that was checked, uploaded behind the jobs' scratch:
 * scratch_bytes >= the plan's scratch + 16 + n * sizeof(y3f_djob).
 * out: [n][out_h][out_w][3] float32, the bytes y3f_sample writes (tests/test_feed_gpu.py, tests/test_feed_src_gpu.py).
 * Asynchronous on the context's stream; blob, tables, arena and scratch must stay untouched until it has run.
 * (ABI version 5: up to version 4 this name took no blob size and no arena, and checked no record.) */
struct y3f_djob;
int y3_feed_run(y3_ctx* ctx, const void* blob_dev, size_t blob_bytes, const struct y3f_djob* jobs_host, int n,
                const void* tables_dev, void* scratch_dev, size_t scratch_bytes, const void* src_dev, size_t src_bytes,
                float* out, int out_h, int out_w);

/* ---- mosaic: n training images composed on the device from 4n ordinary samples of the same size (the Darknet form:
 * windows are copied, never resampled).  THIS COMMENT IS THE DEFINITION; utils/data_aug.py:mosaic4 is its numpy form.
 * in_images [4n][H][W][3] float32, in_boxes [4n][kmax][5] = (x0,y0,x1,y1,m), in_labels [4n][kmax] int32, in_counts [4n] int32
 * (clamped to [0, kmax]).  Output image i is made of samples 4i+q, q = 0..3, by one record of ten int32 in records_host
 * [n][10]: cx, cy, ox0, oy0, ox1, oy1, ox2, oy2, ox3, oy3.
 *   tiles     q0 = [0,cx) x [0,cy), q1 = [cx,W) x [0,cy), q2 = [0,cx) x [cy,H), q3 = [cx,W) x [cy,H); tile q has origin
 *             (tx,ty) and size (tw,th)
 *   validity  1 <= cx <= W-1, 1 <= cy <= H-1, 0 <= ox_q <= W-tw, 0 <= oy_q <= H-th
 *   pixels    out[i][y][x][c] = in[4i+q][y-ty+oy_q][x-tx+ox_q][c] for (x,y) in tile q
 *   boxes     box k < counts[4i+q] of sample 4i+q is (x0,y0,x1,y1,m); the window is wx0 = ox_q, wy0 = oy_q, wx1 = ox_q+tw,
 *             wy1 = oy_q+th.  Every operation is one float32 operation, rounded, with no fused multiply-add (max / min as
 *             numpy's: a NaN operand is the result, so a box with a NaN corner is dropped):
 *               a0 = max(x0,wx0), b0 = max(y0,wy0), a1 = min(x1,wx1), b1 = min(y1,wy1)
 *               kept iff  a1-a0 >= min_side  and  b1-b0 >= min_side  and  (a1-a0)*(b1-b0) >= min_visible*((x1-x0)*(y1-y0))
 *               a kept box becomes ((a0-wx0)+tx, (b0-wy0)+ty, (a1-wx0)+tx, (b1-wy0)+ty, m), with its label
 *   order     kept boxes are written compacted in the order q = 0..3, k ascending within q; out_counts[i] is their number;
 *             out_boxes [n][4*kmax][5] and out_labels [n][4*kmax] hold kout = 4*kmax rows per image, and every row at or
 *             behind out_counts[i] is written as zero
 * Every record is checked on the host against the validity rule before anything is launched (Y3_EINVAL naming the image);
 * the kernels read the checked copy, uploaded into scratch: y3_mosaic_scratch_bytes(n) bytes (0 for n <= 0).  W is a
 * multiple of 32 (rows of W*12 bytes, written with 16-byte stores: out_images 16-byte aligned, everything else 4); n <=
 * 16383; the outputs do not overlap the inputs.  Asynchronous on the context's stream, no host synchronisation (the records
 * go through the context's pinned staging buffer, like y3_feed_run's: the host waits only while the previous upload out of
 * that buffer is still in flight); n = 0 returns 0 and launches nothing. */
size_t y3_mosaic_scratch_bytes(int n);
int y3_mosaic(y3_ctx* ctx, const float* in_images, const float* in_boxes, const int32_t* in_labels, const int32_t* in_counts,
              int n, int kmax, int H, int W, const int32_t* records_host, float min_side, float min_visible, float* out_images,
              float* out_boxes, int32_t* out_labels, int32_t* out_counts, void* scratch, size_t scratch_bytes);

/* ---- random affine warp: n images resampled on the device through one affine map each (rotation / zoom / shear /
 * translation: the "random perspective" step that follows a mosaic), their boxes mapped, clipped, filtered and compacted.
 * THIS COMMENT IS THE DEFINITION; utils/data_aug.py:affine_warp is its numpy form.
 * in_images / out_images [n][H][W][3] float32; boxes [n][kmax][5] = (x0,y0,x1,y1,m), labels [n][kmax] int32, counts [n] int32
 * (clamped to [0, kmax]) on both sides: a warp never adds boxes.  Image i has one record of twelve int32 in records_host
 * [n][12]: words 0-5 are ia, ib, ic, id, ie, if, the INVERSE map (output pixel -> source pixel) in Q16 fixed point; words
 * 6-11 are the bit patterns of six float32 fa, fb, fc, fd, fe, ff, the FORWARD map (source coordinate -> output coordinate).
 * The host folds the half-pixel centre convention into ic / if (utils/data_aug.py:affine_draw), so the rule below has none.
 * Integer operations are exact; every float operation is one float32 operation, rounded, with no fused multiply-add.
 *   validity  |ia|, |ib|, |id|, |ie| <= 2^20; |ic|, |if| <= 2^30; fa .. ff finite; 1 <= H, W <= 4096 (no multiple is asked of
 *             W: a pixel is written with one 12-byte store at 4-byte alignment); n <= 16383; min_side, min_area and
 *             max_aspect are no NaN
 *   pixels    for output pixel (x, y) of image i, in int64:  SX = ia*x + ib*y + ic,  SY = id*x + ie*y + if;
 *             u0 = SX >> 16, v0 = SY >> 16 (arithmetic shifts: floors);  fx = (SX >> 8) & 255, fy = (SY >> 8) & 255;
 *             wx1 = fx/256, wx0 = (256-fx)/256, wy1 = fy/256, wy0 = (256-fy)/256 (exact in float32);
 *             src(u,v,c) = in[i][v][u][c] if 0 <= u < W and 0 <= v < H, else fill;
 *               top = (wx0*src(u0,v0,c)) + (wx1*src(u0+1,v0,c)),  bot = (wx0*src(u0,v0+1,c)) + (wx1*src(u0+1,v0+1,c))
 *               out[i][y][x][c] = (wy0*top) + (wy1*bot)
 *             All four taps are always taken.  Consequence: with fx = fy = 0 a finite pixel whose three neighbours (or fill)
 *             are finite is reproduced exactly (1*p + 0*q; a -0 comes out as +0)
 *   boxes     box k < counts[i] is (x0,y0,x1,y1,m).  Its corners, in the order (x0,y0), (x1,y0), (x0,y1), (x1,y1), map as
 *             u = ((fa*x) + (fb*y)) + fc,  v = ((fd*x) + (fe*y)) + ff.  a0 / a1 are the min / max of the four u and b0 / b1
 *             of the four v, folded in corner order (max / min as numpy's everywhere: a NaN operand is the result).  Clip:
 *             a0 = max(a0,0), b0 = max(b0,0), a1 = min(a1,(float)W), b1 = min(b1,(float)H).  With w = a1-a0, h = b1-b0,
 *             det = |(fa*fe) - (fb*fd)|, area0 = (x1-x0)*(y1-y0) the box is kept iff
 *               w >= min_side  and  h >= min_side  and  w*h >= min_area*(det*area0)  and  w <= max_aspect*h  and
 *               h <= max_aspect*w
 *             (a NaN anywhere fails a comparison and drops the box); a kept box becomes (a0,b0,a1,b1,m), with its label
 *   order     kept boxes are written compacted in ascending k; out_counts[i] is their number; every row of out_boxes and
 *             out_labels at or behind out_counts[i] is written as zero
 * Every record is checked on the host against the validity rule before anything is launched (Y3_EINVAL naming the image,
 * the word and its range); the kernels read the checked copy, uploaded into scratch: y3_affine_scratch_bytes(n) bytes (0
 * for n <= 0).  Every pointer is 4-byte aligned; the outputs do not overlap the inputs.  Asynchronous on the context's
 * stream, no host synchronisation (the records go through the context's pinned staging buffer, as y3_mosaic's do); n = 0
 * returns 0 and launches nothing. */
size_t y3_affine_scratch_bytes(int n);
int y3_affine(y3_ctx* ctx, const float* in_images, const float* in_boxes, const int32_t* in_labels, const int32_t* in_counts,
              int n, int kmax, int H, int W, const int32_t* records_host, float fill, float min_side, float min_area,
              float max_aspect, float* out_images, float* out_boxes, int32_t* out_labels, int32_t* out_counts, void* scratch,
              size_t scratch_bytes);

/* The device half of the feeder's JPEG decoder (include/yolo355_jpeg.h).  liby3feed.so's y3f_jpeg_plan wrote n files into
 * one blob; the caller uploads it and passes its device address and size, the host copy of the n y3j_rec records at its
 * start, a scratch of >= the plan's scratch bytes and an output of >= its output bytes.  Every record's extents are checked
 * against the three sizes before anything is launched.  Each image is written as packed uint8 RGB HWC at its record's
 * out_off: the bytes Pillow's Image.open(f).convert('RGB') gives.  status_dev: n x 2 int32, per image a status (0: good;
 * else bits: 1 invalid Huffman code, 2 data overrun, 4 wrong block count, 8 no synchronisation) and the number of
 * synchronisation rounds the entropy decoder took.  Asynchronous on the context's stream. */
struct y3j_rec;
int y3_jpeg_decode(y3_ctx* ctx, const void* blob_dev, size_t blob_bytes, const struct y3j_rec* recs_host, int n,
                   void* scratch_dev, size_t scratch_bytes, void* out_dev, size_t out_bytes, int* status_dev);

/* box_iou (model.py:307-345): pred_boxes [num_pred][4], true_boxes [num_true][4], both (cx,cy,w,h);
 * iou [num_pred][num_true] = inter / (area_p + area_t - inter + 1e-10). */
int y3_box_iou(y3_ctx* ctx, const float* pred_boxes, long long num_pred, const float* true_boxes, int num_true,
               float* iou);

/* PASCAL VOC mAP on the device: utils/eval_utils.py:235-261 (`get_preds_gpu`'s rows) and :312-423 (`voc_ap`, `voc_eval`),
 * as restated in yolov3_tensorflow_amd/utils/eval_utils.py:123-146 and :184-244, on the tensors y3_nms leaves in HBM.
 * All three are asynchronous on the context's stream; every index read from device memory is clamped to the extents
 * passed here before it addresses anything.  Arithmetic is float64 in voc_eval's operation order, without contraction.
 *
 * y3_voc_append (eval_utils.py:235-261): rows k < out_counts[i] of batch image i = 0..n-1 of one y3_nms result
 *   (cap = its per-image capacity) are appended, images ascending and rows ascending inside an image, to the caller's
 *   arena: arena_box f64 [capacity_rows][4], arena_score f64 [capacity_rows], arena_label / arena_image int32
 *   [capacity_rows] (image_index[i] is what lands in arena_image).  fp32 widens to fp64 exactly.  state: two int32 device
 *   words the caller zeroes once: [0] rows in the arena, [1] rows that did not fit (not written; saturates at 2^31 - 1).
 *   A row's position is state[0] plus an exclusive scan of the counts inside the kernel: nothing waits for the host.
 *
 * y3_voc_match (eval_utils.py:383-413): order[r] = the arena row of rank r, the rows sorted by (label ascending, score
 *   descending, row ascending); the first *n_rows_dev ranks are detections (NULL: all `rows`).  Ground truth as a CSR over
 *   image indices: gt_start int32 [num_images + 1], gt_box f64 [num_gt][4], gt_label int32 [num_gt].  Per rank: the first
 *   maximum of the pixel-inclusive IoU over the image's objects of the detection's class, in ground-truth order; it is a
 *   candidate when that IoU > iou_thres; the candidate of smallest rank per object (a 32-bit atomicMin on a claim word,
 *   whose result does not depend on arrival order) is the true positive, every other detection a false positive - there
 *   is no second choice of object.  Writes tp uint8 [rows] (0 past the detections) and seg_start int32 [class_num + 1],
 *   the first rank of every class.  scratch: y3_voc_match_scratch_bytes(rows, num_gt).
 *
 * y3_voc_ap (eval_utils.py:312-340 and :415-423): out f64 [class_num][5] = (npos, nd, recall, precision, ap) per class;
 *   (1e-6, 1e-6, 0, 0, 0) for a class without detections; recall and area AP are NaN, precision 0 and the 11-point AP 0
 *   for a class with detections and no object, like numpy's.  One workgroup per class walks its segment in passes of
 *   y3_voc_ap_pass() ranks.  use_07_metric: the 11-point metric with thresholds_host11 (HOST array: the eleven doubles of
 *   np.arange(0., 1.1, 0.1)), added as ap + p / 11.; else the area under the precision envelope, summed in a fixed order
 *   (within nd * 2^-52 of numpy's pairwise sum).  Same bits in every run.  scratch: y3_voc_ap_scratch_bytes(rows). */
int y3_voc_append(y3_ctx* ctx, const float* out_boxes, const float* out_scores, const int32_t* out_labels,
                  const int32_t* out_counts, const int32_t* image_index, int n, int cap, double* arena_box,
                  double* arena_score, int32_t* arena_label, int32_t* arena_image, int capacity_rows, int32_t* state);
size_t y3_voc_match_scratch_bytes(int rows, int num_gt);
int y3_voc_match(y3_ctx* ctx, const double* arena_box, const int32_t* arena_label, const int32_t* arena_image,
                 const int32_t* order, int rows, const int32_t* n_rows_dev, const int32_t* gt_start, const double* gt_box,
                 const int32_t* gt_label, int num_images, int num_gt, int class_num, double iou_thres, void* scratch,
                 size_t scratch_bytes, uint8_t* tp, int32_t* seg_start);
int y3_voc_ap_pass(void);
size_t y3_voc_ap_scratch_bytes(int rows);
int y3_voc_ap(y3_ctx* ctx, const uint8_t* tp, const int32_t* seg_start, int rows, const int32_t* gt_label, int num_gt,
              int class_num, int use_07_metric, const double* thresholds_host11, void* scratch, size_t scratch_bytes,
              double* out);

/* COCO bbox metrics on the device (AP@[.50:.95], AP50, AP75, AP by object size, AR@1/10/100, AR by size): what
 * eval_utils.coco_eval computes on the host, on the arena y3_voc_append fills.  All entries are asynchronous on the
 * context's stream; every index read from device memory is clamped to the extents passed here before it addresses
 * anything.  Arithmetic is float64 in coco_eval's operation order, without contraction (csrc/y3_coco_px.h).
 *
 * The rule (bbox evaluation in the COCOeval style; the annotation format has no crowd objects).  T = 10 IoU thresholds and
 * R = 101 recall thresholds come from the host as numpy makes them (np.linspace(.5, .95, 10), np.linspace(0., 1., 101): the
 * ninth IoU threshold is 0.8999999999999999 and is never recomputed here); A = 4 area ranges (lo, hi): all (0, 1e10), small
 * (0, 32^2), medium (32^2, 96^2), large (96^2, 1e10); M = 3 max-dets values 1, 10, 100.
 *   iou(d, g): w = min(d.x1, g.x1) - max(d.x0, g.x0), h likewise; 0 if w <= 0 or h <= 0; else i = w * h and
 *     i / ((d.x1 - d.x0) * (d.y1 - d.y0) + (g.x1 - g.x0) * (g.y1 - g.y0) - i).  No +1.
 *   area = (x1 - x0) * (y1 - y0) * area_scale[image]; a box is outside a range when area < lo or area > hi.
 *   matching, per (image, class, area range, threshold t): the group's detections by descending score, ties in arena order,
 *     the first 100; the objects of the class in ground-truth order, one ignored when its area is outside the range.  Per
 *     detection in order: best = min(t, 1 - 1e-10), m = none; walk the objects that are not ignored and not yet taken: an
 *     object with iou < best is skipped, else best = iou and m = it (an IoU equal to the threshold matches; among equal IoUs
 *     the later object wins); only if that found nothing, walk the ignored, not yet taken objects by the same rule.  A match
 *     takes its object at this (t, range); the detection is ignored iff its object is.  An unmatched detection is ignored iff
 *     its own area is outside the range.
 *   accumulation, per (class k, range a, max-dets M): the detections of every group's first M, by score descending, image
 *     index ascending, in-group rank ascending.  npig = the class's objects that are not ignored; npig == 0 leaves every entry
 *     -1.  Per threshold, with running counts tp (matched, not ignored) and fp (not matched, not ignored): rc = tp / npig,
 *     pr = tp / (fp + tp + 2.220446049250313e-16); recall[t,k,a,M] = the last rc (0 without detections); pr is replaced by its
 *     running maximum from the right; precision[t,r,k,a,M] = pr at the first position with rc >= rec_thrs[r], 0 if none.
 *   the twelve numbers, each the mean over the entries > -1 of a slice, -1 when there are none: AP, AP50 (t = 0), AP75
 *     (t = 5), APs, APm, APl over precision[:, :, :, a, M=100]; AR@1, AR@10, AR@100 over recall[:, :, all, M]; ARs, ARm,
 *     ARl over recall[:, :, a, M=100].  per_class[k] is the same over class k alone.
 *
 * y3_coco_match: order[r] = the arena row of rank r, the rows sorted by (image ascending, label ascending, score descending,
 *   row ascending); the first *n_rows_dev ranks are detections (NULL: all `rows`).  Ground truth as y3_voc_match takes it;
 *   area_scale f64 [num_images] or NULL (1.0); iou_thrs_host: a HOST array of ten doubles.  Per rank r it writes
 *   matched[r] and ignored[r], uint64 words whose bit t * 4 + a is the detection's verdict at threshold t and area range a,
 *   and group_rank[r], the detection's rank inside its (image, class) group saturating at 255; ranks >= 100 are not matched
 *   (both words 0) and never counted.  npig int32 [class_num][4]: the objects per class inside each area range (integer
 *   atomics).  One wavefront per group; "object taken" words live in the LDS for images of up to y3_coco_lds_objects()
 *   objects, else in the scratch.  scratch: y3_coco_match_scratch_bytes(rows, num_gt).
 * y3_coco_ap: order2[i] = a rank, the ranks sorted by (label ascending, score descending, image ascending, rank ascending);
 *   rec_thrs_host: a HOST array of 101 doubles.  Writes precision f64 [10][101][class_num][4][3] and recall f64
 *   [10][class_num][4][3].  One workgroup per (class, range, max-dets, threshold) visits its class's segment in passes of
 *   y3_coco_ap_pass() ranks; all counts are integers.  scratch: y3_coco_ap_scratch_bytes(rows).
 * y3_coco_summary: per_class f64 [class_num][12] and stats f64 [12] (the mean over the classes where the number is defined:
 *   every such class has the same number of entries), summed in a fixed order: the same bits in every run, within n * 2^-52
 *   of numpy's mean over the n entries.
 * Y3_EINVAL before any launch: a null pointer, a non-positive size, a scratch too small, a misaligned pointer, an index
 * product (num_images * class_num, 12120 * class_num) beyond 2^31 - 1. */
size_t y3_coco_match_scratch_bytes(int rows, int num_gt);
int y3_coco_match(y3_ctx* ctx, const double* arena_box, const int32_t* arena_label, const int32_t* arena_image,
                  const int32_t* order, int rows, const int32_t* n_rows_dev, const int32_t* gt_start, const double* gt_box,
                  const int32_t* gt_label, const double* area_scale, int num_images, int num_gt, int class_num,
                  const double* iou_thrs_host, void* scratch, size_t scratch_bytes, uint64_t* matched, uint64_t* ignored,
                  uint8_t* group_rank, int32_t* npig);
int y3_coco_ap_pass(void);
int y3_coco_lds_objects(void);
size_t y3_coco_ap_scratch_bytes(int rows);
int y3_coco_ap(y3_ctx* ctx, const uint64_t* matched, const uint64_t* ignored, const uint8_t* group_rank,
               const int32_t* arena_label, const int32_t* order, const int32_t* order2, int rows, const int32_t* n_rows_dev,
               const int32_t* npig, int class_num, const double* rec_thrs_host, void* scratch, size_t scratch_bytes,
               double* precision, double* recall);
int y3_coco_summary(y3_ctx* ctx, const double* precision, const double* recall, int class_num, double* per_class,
                    double* stats);

/* Recall / precision counts of one training batch on the device: utils/eval_utils.py:142-232 (`evaluate_on_gpu`), as
 * restated in yolov3_tensorflow_amd/utils/eval_utils.py:53-99, on the tensors y3_nms leaves in HBM (out_boxes f32
 * [n][cap][4], out_labels int32 [n][cap], out_counts int32 [n]) and the three y_true tensors of the batch
 * (f32 [n][g][g'][3][5 + class_num + 1] with g = h/32, h/16, h/8 and g' = w/32, w/16, w/8; h, w = the network input size).
 *   gather: per image, the cells of y_true_1, _2, _3 in that order, row-major (row, column, anchor) inside a scale.  A
 *     cell holds an object when an entry of its class slice (channels 5 .. 5+class_num-1) is > 0 - the precondition is that
 *     the slice is finite and >= 0, where this is eval_utils' `sum > 0`; its label is the slice's first maximum, its box
 *     x0y0 = xy - wh / 2., x1y1 = x0y0 + wh in float64.  Objects are compacted IN THAT ORDER into the scratch; at most gt_cap
 *     per image are kept and state[0] += the number dropped (the caller zeroes state; a non-zero word voids the table).
 *   match: every detection k < out_counts[i] adds 1 to n_pred[label]; its IoU (calc_iou, eval_utils.py:35-50: float64 with
 *     the detection's width, height and area in float32) with every object of the image, of any label; the first maximum
 *     in gather order (a NaN counts as one); a hit when that IoU > iou_thresh and that object's label is the detection's.
 *   tally: every object adds 1 to n_true[label], every object hit at least once adds 1 to n_tp[label].
 * table: int64 [class_num][3] = (n_tp, n_true, n_pred), accumulated with integer atomics into what the caller zeroed, so
 * several batches can be summed in one table; the counts are the same in every run.  Every index read from device memory
 * is clamped to the extents passed here.  scratch: y3_batch_eval_scratch_bytes(n, gt_cap) (0 for non-positive arguments);
 * its contents on entry do not matter.  Asynchronous on the context's stream.  Y3_EINVAL before any launch: a null
 * pointer, a non-positive size, h or w not a multiple of 32, n > 65535, a scratch too small, a product (n * cap,
 * n * gt_cap, n * cells, 1024 * channels) beyond 2^31 - 1. */
size_t y3_batch_eval_scratch_bytes(int n, int gt_cap);
int y3_batch_eval(y3_ctx* ctx, const float* out_boxes, const int32_t* out_labels, const int32_t* out_counts, int n, int cap,
                  const float* y_true_1, const float* y_true_2, const float* y_true_3, int h, int w, int class_num,
                  double iou_thresh, int gt_cap, void* scratch, size_t scratch_bytes, long long* table, int32_t* state);

/* K11: g <- g*grad_scale + weight_decay*w (slim.l2_regularizer, model.py:49) ; g <- tf.clip_by_norm(g, clip)
 * (train.py:113-114) ; TF1 update rule (utils/misc_utils.py:151-161).  kind: 0 sgd, 1 momentum (slot0 =
 * accumulator), 2 adam (slot0 = m, slot1 = v, decay = beta1, lr = lr_t), 3 rmsprop (slot0 = ms, slot1 = mom).
 * scratch: y3_optimizer_scratch_bytes(). */
size_t y3_optimizer_scratch_bytes(void);
int y3_clip_update(y3_ctx* ctx, int kind, float* w, float* g, float* slot0, float* slot1, long long n,
                   float weight_decay, float grad_scale, float clip_norm, float lr, float momentum, float decay,
                   float beta2, float eps, float* scratch);

/* The same K11 for ALL trainable tensors of a step in three launches (train.py:112-115 applies clip_by_norm and the
 * update to every (gradient, variable) pair): per-tensor norms come from a segmented, fixed-order reduction, so the
 * result is deterministic.  `params` is a HOST array (device pointers inside); it is copied to the scratch with an
 * asynchronous copy on the context's stream.  scratch: y3_clip_update_multi_scratch_bytes(params, count), 16-byte
 * aligned.  w and g of a tensor with n %% 4 == 0 must be 16-byte aligned. */
typedef struct y3_param_desc {
    float* w;            /* the variable */
    float* g;            /* its gradient (updated in place to the clipped gradient) */
    float* slot0;        /* optimizer slots as in y3_clip_update (NULL where the rule has none) */
    float* slot1;
    long long n;         /* elements */
    float weight_decay;  /* l2 coefficient (0 for BN parameters and biases) */
    int reserved;        /* flags of y3_layerwise_update_multi (Y3_PARAM_NO_ADAPT); y3_clip_update_multi{,_ema} ignore it */
} y3_param_desc;
size_t y3_clip_update_multi_scratch_bytes(const y3_param_desc* params, int count);
int y3_clip_update_multi(y3_ctx* ctx, int kind, const y3_param_desc* params, int count, float grad_scale,
                         float clip_norm, float lr, float momentum, float decay, float beta2, float eps,
                         void* scratch, size_t scratch_bytes);

/* Weight moving average: TF1's tf.train.ExponentialMovingAverage(decay, num_updates).apply(update_vars) with
 * zero_debias=False, kept by the update kernel.  After the step's update of a variable w:
 *     d_t    = min(decay, (1 + t) / (10 + t))     with warm-up (num_updates = t), else d_t = decay
 *     shadow = shadow - (1 - d_t) * (shadow - w_new)
 *   t       the trainer's global_step BEFORE this step increments it (a resumed run continues the ramp).
 *   shadow  one fp32 tensor per UPDATED variable, of the variable's shape; it starts as a copy of the variable (or with the
 *           value a checkpoint stored).  A variable the step does not update is its own average and has no shadow; BN moving
 *           mean / variance are not trainable and are not averaged (they are averages already).
 *   ema_step = 1 - d_t is what the ABI carries: the host forms it in double and passes ONE float.  Passing `decay` would
 *           make the kernel form 1 - float32(decay), and 1 - float32(0.9998) is 3e-4 (relative) away from 0.0002 - an error
 *           on every step of the average.
 *   arithmetic: s + (-ema_step) * (s - w_new) in fp32, the difference rounded once and the multiply-add fused (two
 *           roundings; error <= 5 * 2^-24 * max(|s|, |w_new|) with room to spare), the same expression in both entries
 *           below, for the fp32 and the bf16 train step alike (variables are fp32 in both).  ema_step = 0 writes no shadow.
 * y3_clip_update_multi_ema: y3_clip_update_multi (same three launches; w, g, slot0, slot1 get the same bits) whose third
 *   launch also updates ema[i], the shadow of params[i], from the w it is about to store.  `ema` is a HOST array of `count`
 *   device pointers (uploaded with the descriptors); a NULL entry = that tensor has no shadow.  A shadow has the alignment
 *   contract of w (16 bytes where n %% 4 == 0, else 4).  scratch: y3_clip_update_multi_ema_scratch_bytes(params, count),
 *   16-byte aligned.  Y3_EINVAL before any launch: what y3_clip_update_multi refuses, a NULL `ema` array, ema_step outside
 *   [0, 1] or not finite, a misaligned shadow, a shadow equal to or overlapping its tensor's w, g or slots.
 * y3_ema_update: the same rule for one tensor of n elements (for a host that updates through y3_clip_update). */
size_t y3_clip_update_multi_ema_scratch_bytes(const y3_param_desc* params, int count);
int y3_clip_update_multi_ema(y3_ctx* ctx, int kind, const y3_param_desc* params, int count, float grad_scale,
                             float clip_norm, float lr, float momentum, float decay, float beta2, float eps,
                             float* const* ema, float ema_step, void* scratch, size_t scratch_bytes);
int y3_ema_update(y3_ctx* ctx, float* shadow, const float* w, long long n, float ema_step);

/* Layer-wise update rules for large global batches: AdamW (decoupled weight decay, Loshchilov & Hutter 2019), LARS (You et
 * al. 2017) and LAMB (You et al. 2020), for ALL tensors of a step like y3_clip_update_multi, on its machinery: chunks of
 * 8192 elements, per-chunk fp32 partial sums, per-tensor sums of the partials in a fixed order in fp64, no atomics - two
 * calls on the same inputs give the same bits.  Kinds 0-3 are not taken here, and kinds 4-6 are not taken by
 * y3_clip_update / y3_clip_update_multi / y3_clip_update_multi_ema (which go on ignoring `reserved`).
 *
 * Per tensor, with lambda = the descriptor's weight_decay, and every hyper-parameter from `hp`:
 *     g     = grad_scale * g_in                 NO L2 term is added to the gradient: lambda is used as each kind says below
 *     G     = ||g||_2,  W = ||w||_2             w BEFORE the step.  Each is float32(sqrt(fp64 sum of the fp32 chunk partials))
 *     c     = clip_norm / max(G, clip_norm)     tf.clip_by_norm, as in y3_clip_update_multi (G = 0: c = 1)
 *     gh    = c * g,   Gh = c * G
 *     adapt = bit 0 of the descriptor's `reserved` (Y3_PARAM_NO_ADAPT) is CLEAR
 *   (1 - beta1) and (1 - beta2) are formed in fp32 in the kernel from the floats passed, as the adam and rmsprop rules do.
 *
 *   Y3_OPT_ADAMW (4)   slot0 = m, slot1 = v
 *     m <- beta1 * m + (1 - beta1) * gh
 *     v <- beta2 * v + (1 - beta2) * gh * gh
 *     w <- w - lr_t * m / (sqrt(v) + eps) - lr * lambda * w_old
 *       lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t): the host forms it in double, as for adam, and passes BOTH lr and lr_t.
 *     g is left holding gh.  The ratio reported is 1.
 *
 *   Y3_OPT_LARS (5)    slot0 = acc
 *     ratio = trust * W / (Gh + lambda * W)     if adapt and W > 0 and Gh > 0, else 1
 *     u     = gh + lambda * w
 *     acc  <- momentum * acc + ratio * u        the ratio sits INSIDE the accumulator, as in the LARS paper
 *     w    <- w - lr * acc
 *     g is left holding gh.  With ratio = 1 this is kind 1 (momentum) with the L2 term added after the clip, not before it.
 *
 *   Y3_OPT_LAMB (6)    slot0 = m, slot1 = v
 *     m, v as for AdamW
 *     r     = (m * bias1) / (sqrt(v * bias2) + eps) + lambda * w
 *       bias1 = 1 / (1 - beta1^t), bias2 = 1 / (1 - beta2^t): the host forms both in double and passes them as floats.
 *     R     = ||r||_2                           by the same reduction as G and W
 *     ratio = W / R                             if adapt and W > 0 and R > 0, else 1
 *     w    <- w - lr * ratio * r
 *     g is left holding r, the direction whose norm was taken: R is the norm of exactly the values that are applied.
 *
 *   Corners: a tensor of zeros (W = 0), a zero gradient (Gh = 0; LAMB: R = 0) and a NO_ADAPT tensor take ratio 1, so they
 *   still move by the plain rule (a new layer can leave zero).  trust = 0 freezes every adapted LARS tensor.  The usual
 *   exclusion is NO_ADAPT on BN gamma / beta and biases, with lambda = 0 there.
 *
 * Launches: AdamW and LARS three - prepare (scales g; two partials per chunk, of g^2 and w^2), norms (one workgroup per
 * tensor: c, Gh, W, ratio), update (the rule, and the shadow where one is given).  LAMB five - prepare, norms, direction
 * (m, v; r into g; partials of r^2), norms of r (the ratio), apply (w, the shadow).  A tensor with n %% 4 == 0 moves four
 * elements per lane in every launch.
 *
 * params: HOST array as in y3_clip_update_multi.  ema: HOST array of `count` shadow pointers as in y3_clip_update_multi_ema
 * ("Weight moving average": the same expression from the w about to be stored, hp->ema_step = 1 - d_t); NULL = no
 * averages, and NULL entries are allowed.  ratio_dev: NULL, or a DEVICE array of `count` floats that receives each tensor's
 * ratio.  scratch: y3_layerwise_update_multi_scratch_bytes(params, count) (0 for no tensors), 16-byte aligned.
 * Asynchronous on the context's stream.
 *
 * Y3_EINVAL before any launch, with w, g, slots and shadows untouched: a kind outside 4..6; a NULL ctx, params, hp or
 * scratch; a tensor with a null w or g, n <= 0 or a missing slot (LARS needs slot0, the others both); a member of hp or a
 * weight_decay that is not finite; a negative trust, lr, eps or weight_decay; ema_step outside [0, 1]; w, g, a slot or a
 * shadow of a tensor with n %% 4 == 0 that is not 16-byte aligned; a shadow that overlaps its tensor's w, g or slots; a
 * scratch too small or misaligned. */
#define Y3_OPT_ADAMW 4
#define Y3_OPT_LARS 5
#define Y3_OPT_LAMB 6
#define Y3_PARAM_NO_ADAPT 1      /* y3_param_desc.reserved, bit 0: this tensor takes ratio 1 */
typedef struct y3_layerwise_hp {
    float grad_scale;    /* 1 / world size, or 1 */
    float clip_norm;
    float lr;
    float lr_t;          /* AdamW's bias-corrected step size */
    float momentum;      /* LARS */
    float beta1, beta2;  /* AdamW, LAMB */
    float eps;           /* AdamW, LAMB */
    float bias1, bias2;  /* LAMB's 1 / (1 - beta^t) */
    float trust;         /* LARS's trust coefficient */
    float ema_step;      /* 1 - d_t of the weight moving average (read only where `ema` is given, checked always) */
} y3_layerwise_hp;
size_t y3_layerwise_update_multi_scratch_bytes(const y3_param_desc* params, int count);
int y3_layerwise_update_multi(y3_ctx* ctx, int kind, const y3_param_desc* params, int count, const y3_layerwise_hp* hp,
                              float* const* ema, float* ratio_dev, void* scratch, size_t scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif /* YOLO355_H */
