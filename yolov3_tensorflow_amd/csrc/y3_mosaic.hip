// Mosaic composition on the device (include/yolo355.h: y3_mosaic): every output image is cut together from windows of
// four samples of the same size, and their boxes are clipped to the windows, filtered and compacted.
//
//   pixels   one thread per 16-byte group of the output (four floats; a row is W * 12 bytes and W a multiple of 32, so a
//            group never crosses a row).  Each of the four floats finds its own tile and source element - a tile border
//            or a source offset may fall anywhere inside the group - and is read where it lies; one 16-byte store
//   boxes    one wavefront per output image walks the 4 * kmax candidates (sample q, box k) in chunks of 64 in the order
//            q, k; a 64-bit ballot and a prefix count compact the kept boxes in that order; rows behind the count are zeroed
//
// Both kernels read the records the host checked, uploaded into the scratch.  The arithmetic is y3_mosaic_px.h's.
#include <string.h>
#include "y3_eval_common.h"
#include "y3_mosaic_px.h"
#include "y3_wave_compact.h"

namespace {

using namespace y3ev;

constexpr int kWave = y3wc::kWave;
constexpr int kThreads = 256;
constexpr int kMaxSide = 16384;

// block (x, i): groups x * kThreads .. of output image i, grid-stride over the image's groups
__global__ __launch_bounds__(kThreads) void mosaic_pixels_kernel(const float* __restrict__ in, const int32_t* __restrict__ recs,
                                                                 int H, int W, float* __restrict__ out) {
    const int i = blockIdx.y;
    const int32_t* rec = recs + (size_t)i * y3mpx::kRecord;       // (uniform over the workgroup)
    const int row_groups = W * 3 / 4;
    const int groups = H * row_groups;          // H, W <= kMaxSide: below 2^31
    float* out_i = out + (size_t)i * H * W * 3;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const int y = g / row_groups, f = (g - y * row_groups) * 4;
        int x = f / 3, c = f - x * 3;
        f32x4 v;
        for (int e = 0; e < 4; ++e) {
            v[e] = in[y3mpx::source_index(rec, i, x, y, c, W, H)];
            if (++c == 3) c = 0, ++x;
        }
        *reinterpret_cast<f32x4*>(out_i + (size_t)g * 4) = v;
    }
}

// block i = one wavefront = output image i
__global__ __launch_bounds__(kWave) void mosaic_boxes_kernel(const float* __restrict__ in_boxes, const int32_t* __restrict__ in_labels,
                                                             const int32_t* __restrict__ in_counts,
                                                             const int32_t* __restrict__ recs, int kmax, int H, int W,
                                                             float min_side, float min_visible, float* __restrict__ out_boxes,
                                                             int32_t* __restrict__ out_labels, int32_t* __restrict__ out_counts) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int32_t* rec = recs + (size_t)i * y3mpx::kRecord;
    const int kout = 4 * kmax;          // checked by the host: below 2^31
    float* ob = out_boxes + (size_t)i * kout * 5;
    int32_t* ol = out_labels + (size_t)i * kout;
    int kept = 0;                       // (uniform over the wavefront)
    for (int j0 = 0; j0 < kout; j0 += kWave) {
        const int j = j0 + lane;
        bool keep = false;
        float row[5];
        int32_t label = 0;
        if (j < kout) {
            const int q = j / kmax, k = j - q * kmax;
            const size_t s = 4 * (size_t)i + q;
            if (k < clampi(in_counts[s], 0, kmax)) {
                keep = y3mpx::box_rule(in_boxes + (s * kmax + k) * 5, y3mpx::tile_of(rec, q, W, H), min_side, min_visible, row);
                label = in_labels[s * kmax + k];
            }
        }
        const int at = y3wc::compact_slot(keep, lane, kept);       // at <= j < kout
        if (keep) {
            for (int e = 0; e < 5; ++e) ob[(size_t)at * 5 + e] = row[e];
            ol[at] = label;
        }
    }
    for (int j = kept + lane; j < kout; j += kWave) {
        for (int e = 0; e < 5; ++e) ob[(size_t)j * 5 + e] = 0.f;
        ol[j] = 0;
    }
    if (lane == 0) out_counts[i] = kept;
}

}  // namespace

// y3_mosaic's scratch: the checked records, int32 [n][10]
extern "C" size_t y3_mosaic_scratch_bytes(int n) { return n > 0 ? align256((size_t)n * y3mpx::kRecord * sizeof(int32_t)) : 0; }

extern "C" int y3_mosaic(y3_ctx* ctx, const float* in_images, const float* in_boxes, const int32_t* in_labels,
                         const int32_t* in_counts, int n, int kmax, int H, int W, const int32_t* records_host, float min_side,
                         float min_visible, float* out_images, float* out_boxes, int32_t* out_labels, int32_t* out_counts,
                         void* scratch, size_t scratch_bytes) {
    Y3_CHECK_ARG(ctx, "y3_mosaic: null context");
    Y3_CHECK_ARG(n >= 0, "y3_mosaic: n=%d is negative", n);
    if (n == 0) return Y3_OK;
    Y3_CHECK_ARG(in_images && in_boxes && in_labels && in_counts && records_host && out_images && out_boxes && out_labels &&
                     out_counts && scratch,
                 "y3_mosaic: null argument");
    Y3_CHECK_ARG(n <= 16383, "y3_mosaic: n=%d exceeds 16383 images", n);
    Y3_CHECK_ARG(kmax > 0 && kmax <= (1 << 24), "y3_mosaic: kmax=%d must lie in [1, 2^24]", kmax);
    Y3_CHECK_ARG(H >= 2 && W >= 32 && W % 32 == 0 && H <= kMaxSide && W <= kMaxSide,
                 "y3_mosaic: H=%d must lie in [2, %d] and W=%d be a multiple of 32 up to %d", H, kMaxSide, W, kMaxSide);
    Y3_CHECK_ARG(min_side == min_side && min_visible == min_visible, "y3_mosaic: min_side or min_visible is NaN");
    const size_t rec_bytes = (size_t)n * y3mpx::kRecord * sizeof(int32_t);
    Y3_CHECK_ARG(scratch_bytes >= y3_mosaic_scratch_bytes(n), "y3_mosaic: scratch too small (%zu < %zu)", scratch_bytes,
                 y3_mosaic_scratch_bytes(n));
    Y3_CHECK_ARG(aligned(out_images, 16), "y3_mosaic: out_images must be 16-byte aligned");
    Y3_CHECK_ARG(aligned(in_images, 4) && aligned(in_boxes, 4) && aligned(in_labels, 4) && aligned(in_counts, 4) &&
                     aligned(out_boxes, 4) && aligned(out_labels, 4) && aligned(out_counts, 4) && aligned(scratch, 4),
                 "y3_mosaic: misaligned pointer");
    void* stage = nullptr;
    if (int rc = y3_ctx_stage_acquire(ctx, rec_bytes, &stage)) return rc;
    memcpy(stage, records_host, rec_bytes);
    const int32_t* recs = static_cast<const int32_t*>(stage);
    for (int i = 0; i < n; ++i) {
        int what[3];
        const char* fault = y3mpx::record_fault(recs + (size_t)i * y3mpx::kRecord, W, H, what);
        Y3_CHECK_ARG(!fault, "y3_mosaic: image %d: %s=%d outside [%d, %d] (W=%d, H=%d)", i, fault, what[0], what[1], what[2], W, H);
    }
    const int32_t* recs_dev = static_cast<const int32_t*>(scratch);
    Y3_CHECK_HIP(hipMemcpyAsync(scratch, stage, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = y3_ctx_stage_release(ctx)) return rc;
    const int groups = H * (W * 3 / 4);
    const int blocks = (groups + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(mosaic_pixels_kernel, dim3(blocks < 1024 ? blocks : 1024, n), dim3(kThreads), 0, ctx->stream, in_images,
                       recs_dev, H, W, out_images);
    Y3_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(mosaic_boxes_kernel, dim3(n), dim3(kWave), 0, ctx->stream, in_boxes, in_labels, in_counts, recs_dev, kmax, H,
                       W, min_side, min_visible, out_boxes, out_labels, out_counts);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}
