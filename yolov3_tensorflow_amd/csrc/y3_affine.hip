// Random affine warp on the device (include/yolo355.h: y3_affine): every output image is a bilinear resampling of its input
// image through one inverse map in Q16 fixed point, and its boxes are mapped through the forward map, clipped, filtered and
// compacted.
//
//   pixels   a gather: under rotation a row of the output reads a slanted line of the input, so a workgroup takes a 2-D tile
//            of the output - 32 x 32 pixels, 256 lanes walking it as four bands of 32 x 8 - and the taps of neighbouring
//            lanes fall into the same cache lines.  One lane makes whole pixels: four taps of 12 contiguous bytes, three
//            channels, one 12-byte store; a wavefront's stores are two runs of 384 contiguous bytes.  blockIdx.z is the image
//   boxes    one wavefront per image walks the kmax candidates in chunks of 64; a 64-bit ballot and a prefix count compact
//            the kept boxes in ascending k (y3_wave_compact.h); rows behind the count are zeroed
//
// Both kernels read the records the host checked, uploaded into the scratch.  The arithmetic is y3_affine_px.h's.
#include <string.h>
#include "y3_eval_common.h"
#include "y3_affine_px.h"
#include "y3_wave_compact.h"

namespace {

using namespace y3ev;

constexpr int kWave = y3wc::kWave;
constexpr int kTileW = 32, kBandH = 8, kBands = 4;
constexpr int kThreads = kTileW * kBandH;

// block (tx, ty, i): the 32 x 32 tile at (32 tx, 32 ty) of output image i
__global__ __launch_bounds__(kThreads) void affine_pixels_kernel(const float* __restrict__ in, const int32_t* __restrict__ recs,
                                                                 int H, int W, float fill, float* __restrict__ out) {
    const int i = blockIdx.z;
    const int32_t* rec = recs + (size_t)i * y3apx::kRecord;       // (uniform over the workgroup)
    const float* in_i = in + (size_t)i * H * W * 3;
    float* out_i = out + (size_t)i * H * W * 3;
    const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int y0 = blockIdx.y * (kBandH * kBands) + (threadIdx.x / kTileW);
    if (x >= W) return;
#pragma unroll
    for (int band = 0; band < kBands; ++band) {
        const int y = y0 + band * kBandH;
        if (y < H) {
            float v[3];
            y3apx::pixel(in_i, rec, x, y, W, H, fill, v);
            float* at = out_i + ((size_t)y * W + x) * 3;
            at[0] = v[0], at[1] = v[1], at[2] = v[2];
        }
    }
}

// block i = one wavefront = image i
__global__ __launch_bounds__(kWave) void affine_boxes_kernel(const float* __restrict__ in_boxes, const int32_t* __restrict__ in_labels,
                                                             const int32_t* __restrict__ in_counts,
                                                             const int32_t* __restrict__ recs, int kmax, int H, int W,
                                                             float min_side, float min_area, float max_aspect,
                                                             float* __restrict__ out_boxes, int32_t* __restrict__ out_labels,
                                                             int32_t* __restrict__ out_counts) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int32_t* rec = recs + (size_t)i * y3apx::kRecord;
    const float* ib = in_boxes + (size_t)i * kmax * 5;
    const int32_t* il = in_labels + (size_t)i * kmax;
    float* ob = out_boxes + (size_t)i * kmax * 5;
    int32_t* ol = out_labels + (size_t)i * kmax;
    const int count = clampi(in_counts[i], 0, kmax);
    int kept = 0;                       // (uniform over the wavefront)
    for (int k0 = 0; k0 < count; k0 += kWave) {
        const int k = k0 + lane;
        bool keep = false;
        float row[5];
        int32_t label = 0;
        if (k < count) {
            keep = y3apx::box_rule(ib + (size_t)k * 5, rec, W, H, min_side, min_area, max_aspect, row);
            label = il[k];
        }
        const int at = y3wc::compact_slot(keep, lane, kept);       // at <= k < kmax
        if (keep) {
            for (int e = 0; e < 5; ++e) ob[(size_t)at * 5 + e] = row[e];
            ol[at] = label;
        }
    }
    for (int j = kept + lane; j < kmax; j += kWave) {
        for (int e = 0; e < 5; ++e) ob[(size_t)j * 5 + e] = 0.f;
        ol[j] = 0;
    }
    if (lane == 0) out_counts[i] = kept;
}

}  // namespace

// y3_affine's scratch: the checked records, int32 [n][12]
extern "C" size_t y3_affine_scratch_bytes(int n) { return n > 0 ? align256((size_t)n * y3apx::kRecord * sizeof(int32_t)) : 0; }

extern "C" int y3_affine(y3_ctx* ctx, const float* in_images, const float* in_boxes, const int32_t* in_labels,
                         const int32_t* in_counts, int n, int kmax, int H, int W, const int32_t* records_host, float fill,
                         float min_side, float min_area, float max_aspect, float* out_images, float* out_boxes,
                         int32_t* out_labels, int32_t* out_counts, void* scratch, size_t scratch_bytes) {
    Y3_CHECK_ARG(ctx, "y3_affine: null context");
    Y3_CHECK_ARG(n >= 0, "y3_affine: n=%d is negative", n);
    if (n == 0) return Y3_OK;
    Y3_CHECK_ARG(in_images && in_boxes && in_labels && in_counts && records_host && out_images && out_boxes && out_labels &&
                     out_counts && scratch,
                 "y3_affine: null argument");
    Y3_CHECK_ARG(n <= 16383, "y3_affine: n=%d exceeds 16383 images", n);
    Y3_CHECK_ARG(kmax > 0 && kmax <= (1 << 24), "y3_affine: kmax=%d must lie in [1, 2^24]", kmax);
    Y3_CHECK_ARG(H >= 1 && W >= 1 && H <= y3apx::kMaxSide && W <= y3apx::kMaxSide, "y3_affine: H=%d and W=%d must lie in [1, %d]",
                 H, W, y3apx::kMaxSide);
    Y3_CHECK_ARG(min_side == min_side && min_area == min_area && max_aspect == max_aspect,
                 "y3_affine: min_side, min_area or max_aspect is NaN");
    const size_t rec_bytes = (size_t)n * y3apx::kRecord * sizeof(int32_t);
    Y3_CHECK_ARG(scratch_bytes >= y3_affine_scratch_bytes(n), "y3_affine: scratch too small (%zu < %zu)", scratch_bytes,
                 y3_affine_scratch_bytes(n));
    Y3_CHECK_ARG(aligned(in_images, 4) && aligned(in_boxes, 4) && aligned(in_labels, 4) && aligned(in_counts, 4) &&
                     aligned(out_images, 4) && aligned(out_boxes, 4) && aligned(out_labels, 4) && aligned(out_counts, 4) &&
                     aligned(scratch, 4),
                 "y3_affine: misaligned pointer");
    void* stage = nullptr;
    if (int rc = y3_ctx_stage_acquire(ctx, rec_bytes, &stage)) return rc;
    memcpy(stage, records_host, rec_bytes);
    const int32_t* recs = static_cast<const int32_t*>(stage);
    for (int i = 0; i < n; ++i) {
        const int32_t* rec = recs + (size_t)i * y3apx::kRecord;
        int bound = 0;
        const int word = y3apx::record_fault(rec, &bound);
        Y3_CHECK_ARG(word < 0 || bound == 0, "y3_affine: image %d: word %d, %s=%d outside [%d, %d]", i, word,
                     y3apx::word_name(word < 0 ? 0 : word), word < 0 ? 0 : rec[word], -bound, bound);
        Y3_CHECK_ARG(word < 0, "y3_affine: image %d: word %d, %s is not finite (bits 0x%08x)", i, word, y3apx::word_name(word),
                     (unsigned)rec[word]);
    }
    const int32_t* recs_dev = static_cast<const int32_t*>(scratch);
    Y3_CHECK_HIP(hipMemcpyAsync(scratch, stage, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = y3_ctx_stage_release(ctx)) return rc;
    const int tile_h = kBandH * kBands;
    hipLaunchKernelGGL(affine_pixels_kernel, dim3((W + kTileW - 1) / kTileW, (H + tile_h - 1) / tile_h, n), dim3(kThreads), 0,
                       ctx->stream, in_images, recs_dev, H, W, fill, out_images);
    Y3_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(affine_boxes_kernel, dim3(n), dim3(kWave), 0, ctx->stream, in_boxes, in_labels, in_counts, recs_dev, kmax, H,
                       W, min_side, min_area, max_aspect, out_boxes, out_labels, out_counts);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}
