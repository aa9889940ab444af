// Host side of the C ABI: error channel, contexts, the conv entry point and the y3_net graph
// (yolov3.forward, model.py:30-80 of the reference, as a fixed launch plan over caller-owned buffers).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
#include <algorithm>
#include "y3_internal.h"
#include "y3_net.h"

static thread_local char g_err[512] = "";

void y3_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* y3_last_error(void) { return g_err; }

int y3_current_device() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= Y3_MAX_DEVICES) return -1;
    return dev;
}

size_t y3_device_max_lds() {
    static size_t cached[Y3_MAX_DEVICES] = {};       // benign race (idempotent)
    const int dev = y3_current_device();
    if (dev >= 0 && cached[dev]) return cached[dev];
    // (the per-block figure is the 64 KB default of static allocations on some runtimes; what a kernel may ask for with
    // hipFuncAttributeMaxDynamicSharedMemorySize is bounded by the CU's LDS: take the largest of the three answers)
    int d = 0, v = 0;
    if (hipGetDevice(&d) != hipSuccess) return 0;
    for (hipDeviceAttribute_t a : {hipDeviceAttributeMaxSharedMemoryPerBlock, hipDeviceAttributeSharedMemPerBlockOptin,
                                   hipDeviceAttributeMaxSharedMemoryPerMultiprocessor}) {
        int q = 0;
        if (hipDeviceGetAttribute(&q, a, d) == hipSuccess && q > v) v = q;
    }
    if (v <= 0) return 0;
    if (dev >= 0) cached[dev] = (size_t)v;
    return (size_t)v;
}
extern "C" int y3_abi_version(void) { return Y3_ABI_VERSION; }

extern "C" int y3_ctx_create(int device, void* stream, y3_ctx** out) {
    Y3_CHECK_ARG(out, "y3_ctx_create: null out pointer");
    int count = 0;
    Y3_CHECK_HIP(hipGetDeviceCount(&count));
    Y3_CHECK_ARG(device >= 0 && device < count, "y3_ctx_create: device %d out of range (have %d)", device,
                 count);
    Y3_CHECK_HIP(hipSetDevice(device));
    void* err = nullptr;
    Y3_CHECK_HIP(hipHostMalloc(&err, 64, hipHostMallocMapped));   // pinned + device-visible: the context's error word
    y3_ctx* c = new y3_ctx;
    c->device = device;
    c->stream = static_cast<hipStream_t>(stream);
    c->err_host = static_cast<unsigned*>(err);
    *c->err_host = 0u;
    *out = c;
    return Y3_OK;
}

extern "C" int y3_ctx_destroy(y3_ctx* ctx) {
    if (ctx) {
        if (ctx->err_host) (void)hipHostFree(ctx->err_host);
        if (ctx->stage_ev) { (void)hipEventSynchronize(ctx->stage_ev); (void)hipEventDestroy(ctx->stage_ev); }
        if (ctx->stage_host) (void)hipHostFree(ctx->stage_host);
        delete ctx;
    }
    return Y3_OK;
}

int y3_ctx_stage_acquire(y3_ctx* ctx, size_t bytes, void** out) {
    if (ctx->stage_busy) {                          // the previous upload may still be reading the buffer
        Y3_CHECK_HIP(hipEventSynchronize(ctx->stage_ev));
        ctx->stage_busy = false;
    }
    if (ctx->stage_bytes < bytes) {
        if (ctx->stage_host) Y3_CHECK_HIP(hipHostFree(ctx->stage_host));
        ctx->stage_host = nullptr;
        ctx->stage_bytes = 0;
        const size_t cap = (bytes + 4095) & ~(size_t)4095;
        Y3_CHECK_HIP(hipHostMalloc(&ctx->stage_host, cap, hipHostMallocDefault));
        ctx->stage_bytes = cap;
    }
    if (!ctx->stage_ev) Y3_CHECK_HIP(hipEventCreateWithFlags(&ctx->stage_ev, hipEventDisableTiming));
    *out = ctx->stage_host;
    return Y3_OK;
}

int y3_ctx_stage_release(y3_ctx* ctx) {
    Y3_CHECK_HIP(hipEventRecord(ctx->stage_ev, ctx->stream));
    ctx->stage_busy = true;
    return Y3_OK;
}

// Fault injection for the loud-time-out test (include/yolo355.h, y3_debug_streamk_fault): an explicit call, not an
// environment variable - nothing outside the process can switch it on.
static int g_sk_fault = 0;
extern "C" void y3_debug_streamk_fault(int on) { __atomic_store_n(&g_sk_fault, on ? 1 : 0, __ATOMIC_RELAXED); }
void y3_sk_debug_env(unsigned* spin_limit, int* fault) {
    *fault = __atomic_load_n(&g_sk_fault, __ATOMIC_RELAXED);
    *spin_limit = *fault ? (1u << 10) : (1u << 22);
}

// ---- image-range launches: the fp32 conv kernels form 32-bit byte offsets, so one launch takes tensors below
// 2^29 elements.  Tensors are NHWC with the image index outermost: a larger launch runs as several launches of the same
// kernel over consecutive image ranges, and this planner is the one place that cuts them - the launchers and the scratch /
// block-count queries all ask it.  d is the FORWARD conv; its tensors are [n,h,w,cin] and [n,h/stride,w/stride,co] with
// co = dz_stride where that is > 0 (a gradient's padded rows), else cout.  As few ranges as possible, of near-equal size
// (the first n % ranges hold one image more).  Returns the number of ranges, or Y3_EINVAL: one image alone reaches the
// limit, or more than max_ranges would be needed.
static long long g_range_limit = 0;
extern "C" void y3_debug_conv_range_limit(long long elements) {
    if (elements < 0 || elements > Y3_CONV_RANGE_LIMIT) return;      // (never raises the limit)
    __atomic_store_n(&g_range_limit, elements, __ATOMIC_RELAXED);
}
long long y3_conv_range_limit() {
    const long long v = __atomic_load_n(&g_range_limit, __ATOMIC_RELAXED);
    return v > 0 ? v : Y3_CONV_RANGE_LIMIT;
}

int y3_conv_image_ranges_impl(const y3_conv_desc* d, int dz_stride, long long limit, int max_ranges, int* begin, int* count) {
    Y3_CHECK_ARG(d && begin && count && max_ranges > 0 && limit > 0 && dz_stride >= 0, "y3_conv_image_ranges: bad argument");
    Y3_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->cin > 0 && d->cout > 0 && d->stride > 0,
                 "y3_conv_image_ranges: non-positive dimension");
    const long long in_img = (long long)d->h * d->w * d->cin;
    const long long out_img = (long long)(d->h / d->stride) * (d->w / d->stride) * (dz_stride > 0 ? dz_stride : d->cout);
    const long long img = in_img > out_img ? in_img : out_img;
    Y3_CHECK_ARG(img < limit, "y3_conv_image_ranges: one image of this conv holds %lld elements, the limit of a launch is %lld "
                 "(tensor exceeds 2^29 elements (32-bit byte offsets) and cannot be cut between images)", img, limit);
    const long long per = (limit - 1) / img;                       // images a launch may take: per * img < limit
    const long long nr = (d->n + per - 1) / per;
    Y3_CHECK_ARG(nr <= max_ranges, "y3_conv_image_ranges: %lld image ranges needed, room for %d", nr, max_ranges);
    const int q = d->n / (int)nr, r = d->n % (int)nr;
    for (int i = 0, b = 0; i < (int)nr; ++i) {
        begin[i] = b;
        count[i] = q + (i < r ? 1 : 0);
        b += count[i];
    }
    return (int)nr;
}
extern "C" int y3_conv_image_ranges(const y3_conv_desc* d, int dz_stride, long long limit, int max_ranges, int* begin, int* count) {
    return y3_conv_image_ranges_impl(d, dz_stride, limit, max_ranges, begin, count);
}

static const char* kStreamKTimeout =
    "a stream-K hand-off timed out in an earlier launch on this context (a consumer workgroup gave up waiting for a "
    "partial sum): the output of that launch is INVALID; y3_ctx_check clears the condition";

// Sticky device-side failure of an earlier launch (no synchronisation: reads the pinned word as it is now).
int ctx_pending_error(const y3_ctx* ctx) {
    if (ctx && ctx->err_host && __atomic_load_n(ctx->err_host, __ATOMIC_RELAXED) != 0u) {
        y3_set_error("%s", kStreamKTimeout);
        return Y3_EHIP;
    }
    return Y3_OK;
}
#define Y3_CHECK_CTX(ctx, who)                                   \
    do {                                                         \
        Y3_CHECK_ARG(ctx, who ": null context");                 \
        if (int rc_ = ctx_pending_error(ctx)) return rc_;        \
    } while (0)

extern "C" int y3_ctx_check(y3_ctx* ctx) {
    Y3_CHECK_ARG(ctx, "y3_ctx_check: null context");
    Y3_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    const unsigned code = __atomic_exchange_n(ctx->err_host, 0u, __ATOMIC_RELAXED);
    if (code != 0u) {
        y3_set_error("%s (code %u)", kStreamKTimeout, code);
        return Y3_EHIP;
    }
    return Y3_OK;
}

extern "C" size_t y3_conv_workspace_bytes(const y3_conv_desc* d) { return y3_conv_workspace_bytes_impl(d); }

extern "C" int y3_streamk_range(int kind, int units, int ksteps, int workers, int group, int local_worker,
                                long long* begin, long long* end) {
    return y3_streamk_range_impl(kind, units, ksteps, workers, group, local_worker, begin, end);
}

extern "C" int y3_conv2d_fwd(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* x_up,
                             const float* w, const float* scale, const float* shift,
                             const float* residual, float* y, void* workspace, size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_fwd");
    y3_sk_opts o;
    o.err = ctx->err_host;
    return y3_launch_conv(ctx->stream, d, x, x_up, w, scale, shift, residual, y, workspace, workspace_bytes, &o);
}

// ---- training forward: the conv + the batch-norm statistics of its output in one pass ---------------------------------
extern "C" int y3_conv_stats_blocks(const y3_conv_desc* d, int wino) { return y3_conv_stats_blocks_impl(d, wino); }

extern "C" int y3_conv2d_fwd_stats(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w,
                                   const float* scale, const float* shift, float* y, float* stats, void* workspace,
                                   size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_fwd_stats");
    Y3_CHECK_ARG(stats && d && y3_conv_stats_blocks_impl(d, 0) > 0,
                 "y3_conv2d_fwd_stats: null stats, or a conv without statistics support (y3_conv_stats_blocks == 0)");
    y3_sk_opts o;
    o.err = ctx->err_host;
    o.stats = stats;
    return y3_launch_conv(ctx->stream, d, x, nullptr, w, scale, shift, nullptr, y, workspace, workspace_bytes, &o);
}

extern "C" int y3_conv2d_fwd_wino_stats(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w_wino,
                                        const float* scale, const float* shift, float* y, float* stats, void* workspace,
                                        size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_fwd_wino_stats");
    Y3_CHECK_ARG(stats && d && y3_conv_stats_blocks_impl(d, 1) > 0,
                 "y3_conv2d_fwd_wino_stats: null stats, or a conv the Winograd kernel does not take");
    y3_sk_opts o;
    o.err = ctx->err_host;
    o.stats = stats;
    return y3_launch_conv_wino(ctx->stream, d, x, w_wino, scale, shift, nullptr, y, workspace, workspace_bytes, &o);
}

extern "C" int y3_pack_conv_weights_split(y3_ctx* ctx, const float* w_hwio, int k, int cin, int cout, int planes,
                                          void* w_split) {
    Y3_CHECK_ARG(ctx && w_hwio && w_split, "y3_pack_conv_weights_split: null argument");
    Y3_CHECK_ARG((k == 1 || k == 3) && cin > 0 && cout > 0 && cin % 16 == 0,
                 "y3_pack_conv_weights_split: k must be 1 or 3 and cin a positive multiple of 16");
    Y3_CHECK_ARG(planes == 2 || planes == 3, "y3_pack_conv_weights_split: planes must be 2 or 3 (got %d)", planes);
    return y3_launch_pack_split(ctx->stream, w_hwio, k, cin, cout, planes, w_split);
}

extern "C" int y3_conv2d_fwd_split(y3_ctx* ctx, const y3_conv_desc* d, int planes, const float* x,
                                   const float* x_up, const void* w_split, const float* scale, const float* shift,
                                   const float* residual, float* y, void* workspace, size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_fwd_split");
    y3_sk_opts o;
    o.err = ctx->err_host;
    return y3_launch_conv_split(ctx->stream, d, planes, x, x_up, w_split, scale, shift, residual, y, workspace,
                                workspace_bytes, &o);
}

extern "C" int y3_conv_wino_eligible(const y3_conv_desc* d) { return y3_conv_wino_eligible_impl(d); }

extern "C" int y3_pack_conv_weights_wino(y3_ctx* ctx, const float* w_hwio, int cin, int cout, float* w_wino) {
    Y3_CHECK_ARG(ctx && w_hwio && w_wino, "y3_pack_conv_weights_wino: null argument");
    Y3_CHECK_ARG(cin > 0 && cout > 0 && cin % 8 == 0, "y3_pack_conv_weights_wino: cin must be a positive multiple of 8");
    return y3_launch_pack_wino(ctx->stream, w_hwio, cin, cout, w_wino);
}

extern "C" size_t y3_conv_wino_workspace_bytes(const y3_conv_desc* d) { return y3_conv_wino_workspace_bytes_impl(d); }

extern "C" int y3_conv2d_fwd_wino(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w_wino,
                                  const float* scale, const float* shift, const float* residual, float* y,
                                  void* workspace, size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_fwd_wino");
    y3_sk_opts o;
    o.err = ctx->err_host;
    return y3_launch_conv_wino(ctx->stream, d, x, w_wino, scale, shift, residual, y, workspace, workspace_bytes, &o);
}

extern "C" int y3_conv_wino44_eligible(const y3_conv_desc* d) { return y3_conv_wino44_eligible_impl(d); }
extern "C" int y3_conv_wino44_candidate(const y3_conv_desc* d) { return y3_conv_wino44_candidate_impl(d); }
extern "C" int y3_conv_wino44_preferred(const y3_conv_desc* d) { return y3_conv_wino44_preferred_impl(d); }

extern "C" int y3_pack_conv_weights_wino44(y3_ctx* ctx, const float* w_hwio, int cin, int cout, float* w_wino44) {
    Y3_CHECK_ARG(ctx && w_hwio && w_wino44, "y3_pack_conv_weights_wino44: null argument");
    Y3_CHECK_ARG(cin > 0 && cout > 0 && cin % 8 == 0, "y3_pack_conv_weights_wino44: cin must be a positive multiple of 8");
    return y3_launch_pack_wino44(ctx->stream, w_hwio, cin, cout, w_wino44);
}

extern "C" size_t y3_conv_wino44_workspace_bytes(const y3_conv_desc* d) { return y3_conv_wino44_workspace_bytes_impl(d); }

extern "C" int y3_conv2d_fwd_wino44(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w_wino44,
                                    const float* scale, const float* shift, const float* residual, float* y,
                                    void* workspace, size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_fwd_wino44");
    y3_sk_opts o;
    o.err = ctx->err_host;
    return y3_launch_conv_wino44(ctx->stream, d, x, w_wino44, scale, shift, residual, y, workspace, workspace_bytes, &o);
}

extern "C" int y3_conv2d_fwd_wino44_stats(y3_ctx* ctx, const y3_conv_desc* d, const float* x, const float* w_wino44,
                                          const float* scale, const float* shift, float* y, float* stats, void* workspace,
                                          size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_fwd_wino44_stats");
    Y3_CHECK_ARG(stats && d && y3_conv_stats_blocks_impl(d, 2) > 0,
                 "y3_conv2d_fwd_wino44_stats: null stats, or a conv the F(4x4,3x3) kernel does not take");
    y3_sk_opts o;
    o.err = ctx->err_host;
    o.stats = stats;
    return y3_launch_conv_wino44(ctx->stream, d, x, w_wino44, scale, shift, nullptr, y, workspace, workspace_bytes, &o);
}

extern "C" int y3_pack_conv_weights_wino44_dgrad(y3_ctx* ctx, const float* w_d, int cin, int dz_stride, float* w_wino44_d) {
    Y3_CHECK_ARG(ctx && w_d && w_wino44_d, "y3_pack_conv_weights_wino44_dgrad: null argument");
    Y3_CHECK_ARG(cin > 0 && dz_stride > 0 && dz_stride % 8 == 0,
                 "y3_pack_conv_weights_wino44_dgrad: dz_stride must be a positive multiple of 8");
    return y3_launch_pack_wino44(ctx->stream, w_d, dz_stride, cin, w_wino44_d, 1);
}

extern "C" int y3_conv2d_dgrad_wino44(y3_ctx* ctx, const y3_conv_desc* fwd, const float* dz, int dz_stride,
                                      const float* w_wino44_d, const float* ones, const float* zeros, int accumulate,
                                      float* dx, void* workspace, size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_dgrad_wino44");
    Y3_CHECK_ARG(fwd && dz && w_wino44_d && ones && zeros && dx, "y3_conv2d_dgrad_wino44: null pointer argument");
    Y3_CHECK_ARG(fwd->k == 3 && fwd->stride == 1 && fwd->c_up == 0 && dz_stride >= fwd->cout,
                 "y3_conv2d_dgrad_wino44: needs a 3x3 stride-1 conv and dz_stride >= Cout");
    const y3_conv_desc g = y3_dgrad_desc(fwd, dz_stride);
    Y3_CHECK_ARG(y3_conv_wino44_eligible_impl(&g), "y3_conv2d_dgrad_wino44: needs dz_stride %% 32 == 0 and Cin %% 64 == 0");
    y3_sk_opts o;
    o.err = ctx->err_host;
    // accumulate: dx is read as the residual and written by the same thread for the same element (no cross-thread hazard)
    return y3_launch_conv_wino44(ctx->stream, &g, dz, w_wino44_d, ones, zeros, accumulate ? dx : nullptr, dx, workspace,
                                 workspace_bytes, &o);
}

// Data gradient of a stride-1 3x3 conv in its Winograd form: dx (+)= conv_same(dz, flipped / channel-swapped kernel) is
// itself a stride-1 3x3 SAME conv [n,h,w,dz_stride] -> [n,h,w,cin], so the forward Winograd kernel runs it unchanged.
static int wino_dgrad_desc(const y3_conv_desc* fwd, int dz_stride, y3_conv_desc* g) {
    Y3_CHECK_ARG(fwd && fwd->k == 3 && fwd->stride == 1 && fwd->c_up == 0, "y3_conv2d_dgrad_wino: needs a 3x3 stride-1 conv");
    Y3_CHECK_ARG(dz_stride >= fwd->cout && dz_stride % 32 == 0 && fwd->cin % 32 == 0,
                 "y3_conv2d_dgrad_wino: dz stride and Cin must be multiples of 32");
    *g = y3_dgrad_desc(fwd, dz_stride);
    Y3_CHECK_ARG(y3_conv_wino_eligible_impl(g), "y3_conv2d_dgrad_wino: shape not eligible for the Winograd kernel");
    return Y3_OK;
}

extern "C" int y3_pack_conv_weights_wino_dgrad(y3_ctx* ctx, const float* w_d, int cin, int dz_stride, float* w_wino_d) {
    Y3_CHECK_ARG(ctx && w_d && w_wino_d, "y3_pack_conv_weights_wino_dgrad: null argument");
    Y3_CHECK_ARG(cin > 0 && dz_stride > 0 && dz_stride % 8 == 0,
                 "y3_pack_conv_weights_wino_dgrad: dz_stride must be a positive multiple of 8");
    return y3_launch_pack_wino(ctx->stream, w_d, dz_stride, cin, w_wino_d, 1);
}

extern "C" int y3_conv2d_dgrad_wino(y3_ctx* ctx, const y3_conv_desc* fwd, const float* dz, int dz_stride,
                                    const float* w_wino_d, const float* ones, const float* zeros, int accumulate,
                                    float* dx, void* workspace, size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_dgrad_wino");
    Y3_CHECK_ARG(dz && w_wino_d && ones && zeros && dx, "y3_conv2d_dgrad_wino: null pointer argument");
    y3_conv_desc g;
    if (int rc = wino_dgrad_desc(fwd, dz_stride, &g)) return rc;
    y3_sk_opts o;
    o.err = ctx->err_host;
    // accumulate: dx is read as the residual and written by the same thread of the same tile (no cross-thread hazard)
    return y3_launch_conv_wino(ctx->stream, &g, dz, w_wino_d, ones, zeros, accumulate ? dx : nullptr, dx, workspace,
                               workspace_bytes, &o);
}

extern "C" int y3_pack_conv_weights_split_dgrad(y3_ctx* ctx, const float* w_d, int k, int cin, int dz_stride,
                                                int planes, void* w_split) {
    Y3_CHECK_ARG(ctx && w_d && w_split, "y3_pack_conv_weights_split_dgrad: null argument");
    Y3_CHECK_ARG((k == 1 || k == 3) && cin > 0 && dz_stride > 0 && dz_stride % 16 == 0,
                 "y3_pack_conv_weights_split_dgrad: k must be 1 or 3 and dz_stride a positive multiple of 16");
    Y3_CHECK_ARG(planes == 2 || planes == 3, "y3_pack_conv_weights_split_dgrad: planes must be 2 or 3 (got %d)", planes);
    // the gradient conv's K axis is dz_stride, its output axis the forward cin: read [k*k][cin][dz_stride] transposed
    return y3_launch_pack_split(ctx->stream, w_d, k, dz_stride, cin, planes, w_split, 1);
}

extern "C" int y3_conv2d_dgrad_split(y3_ctx* ctx, const y3_conv_desc* fwd, int planes, const float* dz, int dz_stride,
                                     const void* w_split_d, const float* ones, const float* zeros, int accumulate,
                                     float* dx, void* workspace, size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_dgrad_split");
    y3_sk_opts o;
    o.err = ctx->err_host;
    return y3_launch_conv_dgrad_split(ctx->stream, fwd, planes, dz, dz_stride, w_split_d, ones, zeros, accumulate, dx,
                                      workspace, workspace_bytes, &o);
}

extern "C" int y3_conv2d_dgrad(y3_ctx* ctx, const y3_conv_desc* fwd, const float* dz, int dz_stride,
                               const float* w_d, const float* ones, const float* zeros, int accumulate,
                               float* dx, void* workspace, size_t workspace_bytes) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_dgrad");
    y3_sk_opts o;
    o.err = ctx->err_host;
    return y3_launch_conv_dgrad(ctx->stream, fwd, dz, dz_stride, w_d, ones, zeros, accumulate, dx, workspace,
                                workspace_bytes, &o);
}

// ---- the 1x1 data gradient with the BN backward reduction of the layer below in its epilogue ----------------------------
extern "C" int y3_conv_dgrad_bn_blocks(const y3_conv_desc* fwd) { return y3_conv_dgrad_stats_blocks_impl(fwd); }

extern "C" int y3_conv2d_dgrad_bn(y3_ctx* ctx, const y3_conv_desc* fwd, const float* dz, int dz_stride, const float* w_d,
                                  const float* ones, const float* zeros, int accumulate, float* dx, const float* bn_z,
                                  const float* bn_vec, float* partial) {
    Y3_CHECK_CTX(ctx, "y3_conv2d_dgrad_bn");
    Y3_CHECK_ARG(fwd && bn_z && bn_vec && partial && y3_conv_dgrad_stats_blocks_impl(fwd) > 0,
                 "y3_conv2d_dgrad_bn: null argument, or a conv without the fused reduction (y3_conv_dgrad_bn_blocks == 0)");
    y3_sk_opts o;
    o.err = ctx->err_host;
    o.stats = partial;
    o.bwd_z = bn_z;
    o.bwd_vec = bn_vec;
    return y3_launch_conv_dgrad(ctx->stream, fwd, dz, dz_stride, w_d, ones, zeros, accumulate, dx, nullptr, 0, &o);
}

extern "C" int y3_conv_schedule(const y3_conv_desc* conv, int tmode_taps, int with_workspace) {
    return y3_conv_schedule_query(conv, tmode_taps, with_workspace);
}

// ------------------------------------------------------------------------------------------------
// y3_net: the 75-conv graph.  Tensor ids: 0 = network input; 1.. = conv outputs in creation order.
// ------------------------------------------------------------------------------------------------
// (struct Tensor / Layer / y3_net: y3_net.h)

extern "C" int y3_net_create_arch(y3_ctx* ctx, int class_num, int arch, y3_net** out) {
    // ctx may be NULL: the graph, layer table and workspace plan are host-only; forward then needs a ctx.
    Y3_CHECK_ARG(out, "y3_net_create: null out pointer");
    Y3_CHECK_ARG(class_num > 0, "y3_net_create: class_num must be positive");
    Y3_CHECK_ARG(arch == Y3_ARCH_YOLOV3 || arch == Y3_ARCH_YOLOV3_SPP, "y3_net_create_arch: unknown architecture %d", arch);
    y3_net* net = new y3_net;
    net->ctx = ctx;
    net->class_num = class_num;
    net->arch = arch;
    net->build();
    *out = net;
    return Y3_OK;
}

extern "C" int y3_net_create(y3_ctx* ctx, int class_num, y3_net** out) { return y3_net_create_arch(ctx, class_num, Y3_ARCH_YOLOV3, out); }

extern "C" int y3_net_arch(const y3_net* net) { return net ? net->arch : Y3_ARCH_YOLOV3; }

extern "C" int y3_net_layer_pool(const y3_net* net, int i) {
    return net && i >= 0 && i < (int)net->layers.size() ? net->layers[i].pool : 0;
}

extern "C" int y3_net_set_dtype(y3_net* net, int dtype) {
    Y3_CHECK_ARG(net, "y3_net_set_dtype: null net");
    Y3_CHECK_ARG(dtype >= 0 && dtype <= 4,
                 "y3_net_set_dtype: dtype must be 0 (fp32), 1 (bf16), 2 (fp32 via bf16x6), 3 (fp32 via bf16x3) or "
                 "4 (fp32, Winograd for the eligible 3x3 convs)");
    net->dtype = static_cast<NetDtype>(dtype);
    net->pn = net->ph = net->pw = 0;   // re-plan
    for (Layer& l : net->layers) {     // the bound parameters are packed for the old dtype
        l.scale = l.shift = nullptr;
        std::fill(std::begin(l.w), std::end(l.w), nullptr);
    }
    return Y3_OK;
}

extern "C" int y3_net_destroy(y3_net* net) {
    if (net) {
        for (auto& set : net->event_sets)
            for (hipEvent_t e : set) (void)hipEventDestroy(e);
        if (net->train) y3_train_state_free(net->train);
        if (net->own_stream) (void)hipStreamDestroy(static_cast<hipStream_t>(net->own_stream));
        delete net;
    }
    return Y3_OK;
}

extern "C" int y3_net_num_layers(const y3_net* net) { return net ? (int)net->layers.size() : 0; }

extern "C" int y3_net_layer_info(const y3_net* net, int i, int* k, int* stride, int* cin, int* cout,
                                 int* has_bn) {
    Y3_CHECK_ARG(net && i >= 0 && i < (int)net->layers.size(), "y3_net_layer_info: bad layer index %d", i);
    const Layer& l = net->layers[i];
    if (k) *k = l.k;
    if (stride) *stride = l.stride;
    if (cin) *cin = l.cin;
    if (cout) *cout = l.cout;
    if (has_bn) *has_bn = l.bn;
    return Y3_OK;
}

extern "C" int y3_net_layer_graph(const y3_net* net, int i, int* src, int* up, int* resid, int* dst, int* act) {
    Y3_CHECK_ARG(net && i >= 0 && i < (int)net->layers.size(), "y3_net_layer_graph: bad layer index %d", i);
    const Layer& l = net->layers[i];
    if (src) *src = l.src;
    if (up) *up = l.up;
    if (resid) *resid = l.resid;
    if (dst) *dst = l.dst;
    if (act) *act = l.act;
    return Y3_OK;
}

extern "C" int y3_net_num_tensors(const y3_net* net) { return net ? (int)net->tensors.size() : 0; }

extern "C" int y3_net_tensor_info(const y3_net* net, int t, int* channels, int* sdiv, int* ext) {
    Y3_CHECK_ARG(net && t >= 0 && t < (int)net->tensors.size(), "y3_net_tensor_info: bad tensor id %d", t);
    if (channels) *channels = net->tensors[t].c;
    if (sdiv) *sdiv = net->tensors[t].sdiv;
    if (ext) *ext = net->tensors[t].ext;
    return Y3_OK;
}

static int check_size(const char* who, int n, int h, int w) {
    Y3_CHECK_ARG(n > 0, "%s: batch must be positive", who);
    Y3_CHECK_ARG(h > 0 && w > 0 && h % 32 == 0 && w % 32 == 0,
                 "%s: input size must be a positive multiple of 32 (got %dx%d)", who, h, w);
    return Y3_OK;
}

extern "C" size_t y3_net_workspace_bytes(const y3_net* net, int n, int h, int w) {
    if (!net || check_size("y3_net_workspace_bytes", n, h, w) != Y3_OK) return 0;
    const_cast<y3_net*>(net)->plan(n, h, w);
    return net->plan_bytes;
}

// ---- routes: the only net-level callers of the kernels' eligibility predicates
// Layers j = 0 / 2 run inside their only reader's launch (round 5): the stem + stride-2 conv (y3_conv_bf16s.hip, fp32 F32 and
// F32_WINO: y3_conv_f32s.hip), and in bf16 the first residual block (y3_conv_bf16b.hip).
static bool fuses_with_next(const y3_net& net, int j, int n, int h, int w) {
    const NetDtype dt = net.dtype;
    const Layer &a = net.layers[j], &b = net.layers[j + 1];
    const Tensor &mid = net.tensors[a.dst], &out = net.tensors[b.dst];
    const y3_conv_desc da = net.desc(j, n, h, w), db = net.desc(j + 1, n, h, w);
    const bool pair = b.src == a.dst && mid.last_use == j + 1 && mid.ext < 0 && out.ext < 0 && a.resid < 0;
    if (j == 0)
        return pair && a.src == 0 && b.resid < 0 &&
               (dt == NetDtype::BF16 ? y3_conv_bf16_stem_s2_takes(&da, &db)
                : (dt == NetDtype::F32 || dt == NetDtype::F32_WINO) && y3_conv_f32_stem_s2_takes(&da, &db)) == 1;
    return j == 2 && dt == NetDtype::BF16 && pair && b.resid == a.src && a.src != 0 && net.tensors[a.src].ext < 0 &&
           y3_conv_bf16_resblock64_takes(&da, &db) == 1;
}

static int split_planes(NetDtype dt) { return dt == NetDtype::F32_BF16X6 ? 3 : dt == NetDtype::F32_BF16X3 ? 2 : 0; }

// conv d on the F(4x4,3x3) kernel, F(2x2,3x3), the split-plane kernel or the direct one, with the scratch that launch needs
static ConvRoute fp32_route(const y3_conv_desc& d, bool wino44, bool wino, int planes) {
    ConvRoute r;
    r.kind = wino44 ? RouteKind::Wino44 : wino ? RouteKind::Wino : planes ? RouteKind::Split : RouteKind::Direct;
    r.planes = planes;
    r.two_pass = wino44 && y3_conv_wino44_two_pass_impl(&d);
    r.streamk = !wino44 && !wino && y3_conv_schedule_impl(&d);      // (a Winograd kernel has no fix-up)
    r.scratch = wino44 ? (r.two_pass ? y3_conv_wino44_workspace_bytes_impl(&d) : 0)
                : wino ? y3_conv_wino_workspace_bytes_impl(&d) : y3_conv_workspace_bytes_impl(&d);
    return r;
}

ConvRoute y3_route_infer(const y3_net& net, int i, int n, int h, int w) {
    ConvRoute r;
    const NetDtype dt = net.dtype;
    const y3_conv_desc d = net.desc(i, n, h, w);
    if ((i == 0 || i == 2) && fuses_with_next(net, i, n, h, w)) r.kind = RouteKind::InNext;
    else if ((i == 1 || i == 3) && fuses_with_next(net, i - 1, n, h, w))
        r.kind = i == 3 ? RouteKind::ResBlock64Bf16 : dt == NetDtype::BF16 ? RouteKind::StemS2Bf16 : RouteKind::StemS2F32;
    else if (dt == NetDtype::BF16) r.kind = RouteKind::Bf16;       // (the bf16 kernels use no stream-K scratch)
    else
        r = fp32_route(d, dt == NetDtype::F32_WINO && y3_conv_wino44_preferred_impl(&d),
                       dt == NetDtype::F32_WINO && y3_conv_wino_eligible_impl(&d), split_planes(dt));
    return r;
}

// The bf16 train step (dtype 1) runs every conv but the Cin = 3 stem (fp32 image in: today's fp32 route) on Bf16Train
static bool bf16_train(const y3_net& net, int i) { return net.dtype == NetDtype::BF16 && net.layers[i].cin != 3; }

ConvRoute y3_route_train_fwd(const y3_net& net, int i, int n, int h, int w) {
    const Layer& l = net.layers[i];
    const y3_conv_desc d = net.desc(i, n, h, w, true);
    if (bf16_train(net, i)) {
        ConvRoute r;
        r.kind = RouteKind::Bf16Train;
        return r;
    }
    const bool wino = net.dtype == NetDtype::F32_WINO && y3_conv_wino_eligible_impl(&d);
    // F(4x4,3x3) where it fills the chip (y3_conv_wino44_preferred); the Cin = 3 stem reads its HWIO kernel as it is
    return fp32_route(d, wino && l.bn && y3_conv_wino44_preferred_impl(&d), wino, l.cin == 3 ? 0 : split_planes(net.dtype));
}

#ifndef Y3_BN_FUSE
#define Y3_BN_FUSE 1
#endif
// The data gradient: a conv over dz [n, ho, wo, dz_stride] (Cout; the detection convs' padded to det_pad), channel axes swapped.
ConvRoute y3_route_dgrad(const y3_net& net, int i, int n, int h, int w) {
    const Layer& l = net.layers[i];
    if (net.dtype == NetDtype::BF16) {      // (the stem's data gradient never runs: nothing is below it)
        ConvRoute r;
        r.kind = RouteKind::Bf16Train;
        return r;
    }
    const y3_conv_desc d = net.desc(i, n, h, w, true);
    y3_conv_desc g = y3_dgrad_desc(&d, net.dz_stride(i));
    // (a stride-2 layer's route, and with it its scratch, has always been asked of the forward's geometry: the image ranges of
    // that view cut no later than the launch's own, y3_launch_conv_dgrad)
    if (l.stride == 2) { g.h = d.h; g.w = d.w; g.stride = 2; }
    const bool wino = net.dtype == NetDtype::F32_WINO && l.up < 0 && l.k == 3 && l.stride == 1 && y3_conv_wino_eligible_impl(&g);
    const int planes = (l.cin != 3 && l.stride == 1 && l.cin % 4 == 0 && g.cin % 32 == 0) ? split_planes(net.dtype) : 0;
    ConvRoute r = fp32_route(g, wino && y3_conv_wino44_preferred_impl(&g), wino, planes);
    // The BN backward reduction of layer pj (column sums of g' and g' * zhat over its dy and z) rides in the epilogue of the data
    // gradient that writes that dy last - its first consumer in forward order - where that is a stride-1 1x1 conv on the direct
    // kernel: the finished dy is in registers there, and the separate pass over z and dy is skipped.
    const int pj = l.src - 1;
    bool fuse = Y3_BN_FUSE && r.kind == RouteKind::Direct && l.up < 0 && !l.pool && pj >= 0 && net.layers[pj].bn;      // (a pool layer's data gradient does not write dy of src)
    for (int j = 0; j < i; ++j)        // (no earlier layer reads l.src)
        fuse = fuse && net.layers[j].src != l.src && net.layers[j].up != l.src && net.layers[j].resid != l.src;
    r.bn_blocks = fuse ? y3_conv_dgrad_stats_blocks_impl(&d) : 0;
    return r;
}

ConvRoute y3_route_wgrad(const y3_net& net, int i, int n, int h, int w) {
    ConvRoute r;
    const y3_conv_desc d = net.desc(i, n, h, w, true);
    if (bf16_train(net, i)) {
        r.kind = RouteKind::Bf16Train;
        r.scratch = y3_conv_wgrad_bf16_scratch_bytes(&d);
        return r;
    }
    if (net.dtype == NetDtype::BF16) {      // the stem: the fp32 kernel over the fp32 image and dz
        r.scratch = y3_conv_wgrad_scratch_bytes(&d);
        return r;
    }
    const bool wino = net.dtype == NetDtype::F32_WINO && y3_conv_wgrad_wino_eligible_impl(&d);
    r.kind = wino ? RouteKind::Wino : RouteKind::Direct;
    // (the Winograd kernel's scratch is reserved in every dtype: the workspace size the train step has always asked for)
    r.scratch = std::max(y3_conv_wgrad_wino_scratch_bytes_impl(&d), wino ? 0 : y3_conv_wgrad_scratch_bytes(&d));
    return r;
}

// ---- packings: what a route reads its kernel in, and how that packing is written
ConvPack y3_conv_pack(const y3_net& net, int i, const ConvRoute& r, bool dgrad) {
    const Layer& l = net.layers[i];
    ConvPack p;
    p.planes = r.planes; p.dgrad = dgrad;
    p.k = l.k; p.cin = l.cin; p.cout = dgrad ? net.dz_stride(i) : l.cout;
    p.wcout = l.cout;
    switch (r.kind) {
    case RouteKind::Wino44: p.kind = Packing::Wino44; break;
    case RouteKind::Wino: p.kind = Packing::Wino; break;
    case RouteKind::Split: p.kind = Packing::Split; break;
    case RouteKind::Bf16: case RouteKind::StemS2Bf16: case RouteKind::ResBlock64Bf16: p.kind = Packing::Bf16; break;
    case RouteKind::InNext: p.kind = net.dtype == NetDtype::BF16 ? Packing::Bf16 : Packing::Direct; break;
    case RouteKind::Direct: case RouteKind::StemS2F32: p.kind = dgrad ? Packing::Hwio : Packing::Direct; break;
    case RouteKind::Bf16Train: p.kind = Packing::Bf16Reg; break;
    }
    if (l.cin == 3 && !dgrad) p.kind = Packing::Hwio;      // the stem reads its HWIO kernel in every dtype
    return p;
}

size_t ConvPack::bytes() const {
    const size_t taps = (size_t)k * k * cin * cout;
    switch (kind) {
    case Packing::Direct: return taps * 4;
    case Packing::Bf16: case Packing::Bf16Reg: return taps * 2;
    case Packing::Split: return taps * 2 * planes;
    case Packing::Wino: return (size_t)16 * cin * cout * 4;
    case Packing::Wino44: return (size_t)36 * cin * cout * 4;
    default: return 0;
    }
}

int ConvPack::launch(y3_ctx* ctx, const float* w, void* out) const {
    float* o = static_cast<float*>(out);
    switch (kind) {
    case Packing::Direct: return y3_pack_conv_weights(ctx, w, k, cin, cout, o);
    case Packing::Bf16: return y3_pack_conv_weights_bf16(ctx, w, k, cin, cout, out);
    case Packing::Bf16Reg:     // (the data gradient's: `cout` is dz_stride, the variable's Cout is the layer's)
        return dgrad ? y3_pack_conv_weights_bf16_reg(ctx, w, k, cin, wcout, cout, out)
                     : y3_pack_conv_weights_bf16_reg(ctx, w, k, cin, cout, 0, out);
    case Packing::Split:
        return dgrad ? y3_pack_conv_weights_split_dgrad(ctx, w, k, cin, cout, planes, out)
                     : y3_pack_conv_weights_split(ctx, w, k, cin, cout, planes, out);
    case Packing::Wino: return dgrad ? y3_pack_conv_weights_wino_dgrad(ctx, w, cin, cout, o) : y3_pack_conv_weights_wino(ctx, w, cin, cout, o);
    case Packing::Wino44:
        return dgrad ? y3_pack_conv_weights_wino44_dgrad(ctx, w, cin, cout, o) : y3_pack_conv_weights_wino44(ctx, w, cin, cout, o);
    default: return Y3_OK;
    }
}

// The parameter buffer of y3_net_set_params: per layer, the folded scale and shift, then the kernel in every packing
// y3_route_infer may read it in at some legal input size (the stem's HWIO kernel copied), each region 256-byte aligned.
// A route depends on the size only through the kernels' predicates, and those refuse a map with a 1-pixel side (the /32 map
// of a 32-pixel input) or take it at every larger size; y3_conv_wino44_preferred is a subset of y3_conv_wino44_candidate,
// whose packing goes in beside the others.  So the routes at 32 x 32 and 64 x 64, plus that one, cover every size.
struct LayerParams {
    size_t scale, shift;
    std::vector<ConvPack> packs;
    std::vector<size_t> at;      // offset of packs[j]
};
static size_t params_layout(const y3_net& net, std::vector<LayerParams>* out) {
    Arena A;
    A.reset(nullptr, 0, true);
    std::vector<LayerParams> lp(net.layers.size());
    for (size_t i = 0; i < net.layers.size(); ++i) {
        const Layer& l = net.layers[i];
        LayerParams& p = lp[i];
        p.scale = A.alloc((size_t)l.cout * 4).off;
        p.shift = A.alloc((size_t)l.cout * 4).off;
        ConvRoute w44;
        w44.kind = RouteKind::Wino44;
        const y3_conv_desc d = net.desc((int)i, 1, 64, 64);
        std::vector<ConvRoute> rs = {y3_route_infer(net, (int)i, 1, 32, 32), y3_route_infer(net, (int)i, 1, 64, 64)};
        if (net.dtype == NetDtype::F32_WINO && y3_conv_wino44_candidate_impl(&d)) rs.push_back(w44);
        for (const ConvRoute& r : rs) {
            const ConvPack k = y3_conv_pack(net, (int)i, r);
            if (std::any_of(p.packs.begin(), p.packs.end(), [&](const ConvPack& q) { return q.kind == k.kind; })) continue;
            p.packs.push_back(k);
            p.at.push_back(A.alloc(k.kind == Packing::Hwio ? (size_t)l.k * l.k * l.cin * l.cout * 4 : k.bytes()).off);
        }
    }
    if (out) out->swap(lp);
    return A.top;
}

extern "C" size_t y3_net_params_bytes(const y3_net* net) { return net ? params_layout(*net, nullptr) : 0; }

extern "C" int y3_net_set_params(y3_net* net, const y3_train_var* vars, void* params, size_t params_bytes) {
    Y3_CHECK_ARG(net && params, "y3_net_set_params: null argument");
    std::vector<LayerParams> lp;
    const size_t need = params_layout(*net, &lp);
    Y3_CHECK_ARG(params_bytes >= need, "y3_net_set_params: buffer too small (%zu < %zu)", params_bytes, need);
    Y3_CHECK_ARG(((uintptr_t)params & 255) == 0, "y3_net_set_params: the buffer must be 256-byte aligned");
    char* base = static_cast<char*>(params);
    if (vars) {
        if (!net->ctx) {
            y3_set_error("y3_net_set_params: the net was created without a context");
            return Y3_ESTATE;
        }
        for (size_t i = 0; i < net->layers.size(); ++i) {
            const y3_train_var& v = vars[i];
            Y3_CHECK_ARG(v.weights && (net->layers[i].bn ? v.gamma && v.beta && v.moving_mean && v.moving_variance : v.biases != nullptr),
                         "y3_net_set_params: layer %zu: a variable is missing", i);
        }
        y3_ctx* ctx = net->ctx;
        for (size_t i = 0; i < net->layers.size(); ++i) {
            const Layer& l = net->layers[i];
            const y3_train_var& v = vars[i];
            float* scale = reinterpret_cast<float*>(base + lp[i].scale);
            float* shift = reinterpret_cast<float*>(base + lp[i].shift);
            if (l.bn) {
                if (int rc = y3_bn_fold(ctx, v.gamma, v.beta, v.moving_mean, v.moving_variance, 1e-5f, l.cout, scale, shift)) return rc;
            } else {      // detection convs: linear, with a bias (model.py:55-57)
                Y3_CHECK_HIP(hipMemsetD32Async(scale, 0x3f800000, l.cout, ctx->stream));      // 1.0f
                Y3_CHECK_HIP(hipMemcpyAsync(shift, v.biases, (size_t)l.cout * 4, hipMemcpyDeviceToDevice, ctx->stream));
            }
            for (size_t j = 0; j < lp[i].packs.size(); ++j) {
                const ConvPack& k = lp[i].packs[j];
                if (k.kind == Packing::Hwio)
                    Y3_CHECK_HIP(hipMemcpyAsync(base + lp[i].at[j], v.weights, (size_t)l.k * l.k * l.cin * l.cout * 4,
                                                hipMemcpyDeviceToDevice, ctx->stream));
                else if (int rc = k.launch(ctx, v.weights, base + lp[i].at[j]))
                    return rc;
            }
        }
    }
    for (size_t i = 0; i < net->layers.size(); ++i) {
        Layer& l = net->layers[i];
        l.scale = reinterpret_cast<const float*>(base + lp[i].scale);
        l.shift = reinterpret_cast<const float*>(base + lp[i].shift);
        std::fill(std::begin(l.w), std::end(l.w), nullptr);
        for (size_t j = 0; j < lp[i].packs.size(); ++j) l.w[(int)lp[i].packs[j].kind] = base + lp[i].at[j];
    }
    return Y3_OK;
}

// 0: layer i has its own launch; 1: it runs inside the NEXT layer's launch (its output tensor never exists; its profiled time
// is 0); 2: its launch also runs the layer before it.
extern "C" int y3_net_layer_fused(const y3_net* net, int i, int n, int h, int w) {
    if (!net || i < 0 || i >= (int)net->layers.size() || n <= 0 || h <= 0 || w <= 0) return 0;
    const RouteKind k = y3_route_infer(*net, i, n, h, w).kind;
    return k == RouteKind::InNext ? 1 : k >= RouteKind::StemS2F32 ? 2 : 0;      // (the fused kinds come last)
}

extern "C" int y3_net_forward(y3_net* net, const float* x, int n, int h, int w, void* workspace,
                              size_t workspace_bytes, float* fm1, float* fm2, float* fm3) {
    Y3_CHECK_ARG(net && x && workspace && fm1 && fm2 && fm3, "y3_net_forward: null argument");
    if (!net->ctx) {
        y3_set_error("y3_net_forward: the net was created without a context");
        return Y3_ESTATE;
    }
    if (int rc = ctx_pending_error(net->ctx)) return rc;
    if (int rc = check_size("y3_net_forward", n, h, w)) return rc;
    net->plan(n, h, w);
    Y3_CHECK_ARG(workspace_bytes >= net->plan_bytes, "y3_net_forward: workspace too small (%zu < %zu)",
                 workspace_bytes, net->plan_bytes);
    Y3_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "y3_net_forward: workspace must be 256-byte aligned");
    const size_t nl = net->layers.size();
    std::vector<const float*> wk(nl);      // each layer's kernel in the packing its route reads
    for (size_t i = 0; i < nl; ++i) {
        wk[i] = static_cast<const float*>(net->layers[i].w[(int)y3_conv_pack(*net, (int)i, net->routes[i]).kind]);
        if (!wk[i] || !net->layers[i].scale) {
            y3_set_error("y3_net_forward: no parameters bound for this dtype (call y3_net_set_params)");
            return Y3_ESTATE;
        }
    }
    float* ext[3] = {fm1, fm2, fm3};
    char* base = static_cast<char*>(workspace);
    auto ptr = [&](int id) -> float* {
        if (id < 0) return nullptr;
        if (id == 0) return const_cast<float*>(x);
        const Tensor& t = net->tensors[id];
        if (t.ext >= 0) return ext[t.ext];
        return reinterpret_cast<float*>(base + net->offsets[id]);
    };
    hipStream_t st = net->ctx->stream;
    hipEvent_t* ev = nullptr;
    if (net->profiling && net->sets_used < 256) {
        if (net->sets_used == net->event_sets.size()) {
            std::vector<hipEvent_t> set(nl + 1, nullptr);   // nl+1 layer boundaries
            for (size_t i = 0; i < set.size(); ++i) Y3_CHECK_HIP(hipEventCreate(&set[i]));
            net->event_sets.push_back(set);
        }
        ev = net->event_sets[net->sets_used++].data();
        Y3_CHECK_HIP(hipEventRecord(ev[0], st));
    }
    // every stream-K layer polls its own pre-zeroed flag region: ONE memset per forward instead of one per launch
    unsigned* flag_base = reinterpret_cast<unsigned*>(base + net->arena_bytes + net->scratch_bytes);
    if (net->flags_bytes) Y3_CHECK_HIP(hipMemsetAsync(flag_base, 0, net->flags_bytes, st));
    void* scratch = base + net->arena_bytes; const size_t sb = net->scratch_bytes;      // (the routes' largest scratch)
    for (size_t i = 0; i < nl; ++i) {
        const Layer& l = net->layers[i];
        const ConvRoute& r = net->routes[i];
        const y3_conv_desc d = net->desc((int)i, n, h, w);
        y3_sk_opts o;
        o.err = net->ctx->err_host;
        o.flags = net->flags_bytes ? flag_base + i * y3_net::FLAG_WORDS : nullptr;
        o.wino44_form = r.two_pass;
        const Layer& p = net->layers[i ? i - 1 : 0];      // the fused kinds: the layer before, whose launch this is too
        const float *pw = wk[i ? i - 1 : 0], *lw = wk[i];
        float *src = ptr(l.src), *up = ptr(l.up), *res = ptr(l.resid), *y = ptr(l.dst);
        int rc = Y3_OK;
        if (l.pool) {      // spp(src) into its buffer of the arena, then the conv as a plain 1x1 over it (timed with the conv)
            float* pooled = reinterpret_cast<float*>(base + net->pool_offsets[i]);
            const bool half = net->dtype == NetDtype::BF16 && l.src != 0 && net->tensors[l.src].ext < 0;
            if (int prc = y3_spp_fwd(net->ctx, src, half, n, d.h, d.w, net->tensors[l.src].c, pooled)) return prc;
            src = pooled;
        }
        switch (r.kind) {
        case RouteKind::InNext: break;
        case RouteKind::StemS2F32:
            rc = y3_launch_conv_f32_stem_s2(st, n, h, w, x, pw, p.scale, p.shift, p.act, lw, l.scale, l.shift, l.act, y); break;
        case RouteKind::StemS2Bf16:
            rc = y3_launch_conv_bf16_stem_s2(st, n, h, w, x, pw, p.scale, p.shift, p.act, lw, l.scale, l.shift, l.act, y); break;
        case RouteKind::ResBlock64Bf16:
            rc = y3_launch_conv_bf16_resblock64(st, n, d.h, d.w, ptr(p.src), pw, p.scale, p.shift, p.act, lw, l.scale, l.shift,
                                                l.act, y);
            break;
        case RouteKind::Bf16:
            rc = y3_launch_conv_bf16(st, &d, src, up, lw, l.scale, l.shift, res, y, net->tensors[l.dst].ext >= 0 ? 1 : 0); break;
        case RouteKind::Wino44: rc = y3_launch_conv_wino44(st, &d, src, lw, l.scale, l.shift, res, y, scratch, sb, &o); break;
        case RouteKind::Wino: rc = y3_launch_conv_wino(st, &d, src, lw, l.scale, l.shift, res, y, scratch, sb, &o); break;
        case RouteKind::Split:
            rc = y3_launch_conv_split(st, &d, r.planes, src, up, lw, l.scale, l.shift, res, y, scratch, sb, &o); break;
        case RouteKind::Direct: rc = y3_launch_conv(st, &d, src, up, lw, l.scale, l.shift, res, y, scratch, sb, &o); break;
        case RouteKind::Bf16Train: y3_set_error("y3_net_forward: layer %d has a train-step route", i); return Y3_EINVAL;
        }
        if (rc != Y3_OK) return rc;
        if (ev) Y3_CHECK_HIP(hipEventRecord(ev[i + 1], st));
    }
    return Y3_OK;
}

extern "C" int y3_net_layer_is_streamk(const y3_net* net, int i, int n, int h, int w) {
    if (!net || i < 0 || i >= (int)net->layers.size() || n <= 0 || h <= 0 || w <= 0) return 0;
    return y3_route_infer(*net, i, n, h, w).streamk;
}

extern "C" int y3_net_set_profiling(y3_net* net, int enabled) {
    Y3_CHECK_ARG(net, "y3_net_set_profiling: null net");
    net->profiling = enabled != 0;     // recorded sets are kept until y3_net_get_layer_ms reads (and clears) them
    return Y3_OK;
}

extern "C" int y3_net_get_layer_ms(y3_net* net, float* ms, int count) {
    Y3_CHECK_ARG(net && ms, "y3_net_get_layer_ms: null argument");
    Y3_CHECK_ARG(count == (int)net->layers.size(), "y3_net_get_layer_ms: count must be %zu",
                 net->layers.size());
    if (net->sets_used == 0) {
        y3_set_error("y3_net_get_layer_ms: no profiled forward has run");
        return Y3_ESTATE;
    }
    for (int i = 0; i < count; ++i) ms[i] = 0.f;
    for (size_t s = 0; s < net->sets_used; ++s) {
        hipEvent_t* ev = net->event_sets[s].data();
        Y3_CHECK_HIP(hipEventSynchronize(ev[count]));
        for (int i = 0; i < count; ++i) {
            float t = 0.f;
            Y3_CHECK_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            ms[i] += t;
        }
    }
    for (int i = 0; i < count; ++i) ms[i] /= (float)net->sets_used;
    net->sets_used = 0;
    return Y3_OK;
}
