// Recall / precision counts of one training batch on the device (include/yolo355.h: y3_batch_eval): what
// eval_utils._evaluate does per image in numpy, on the tensors the NMS kernels leave in HBM and on y_true as the feeder
// uploaded it.
//
//   gather   one workgroup per image walks the cells of y_true_1, _2, _3, laid end to end, in passes of kPass.  A pass streams its
//            cells' floats with coalesced loads; a positive class entry raises the cell's 64-bit key in LDS (atomicMax: the
//            maximum does not depend on arrival order).  A ballot scan over the pass turns "this cell holds an object"
//            into the object's position, so the objects land in the image's scratch in _ground_truth_of_image's order
//   match    one thread per live detection: n_pred, the first-maximum IoU over the image's objects (staged through LDS in
//            tiles), and a plain store of 1 to the object's found word on a hit (idempotent: any number of hits leave 1)
//   tally    one thread per object: n_true, and n_tp where the found word is set
//
// Counts go to the caller's int64 table with integer atomics (through an LDS histogram in match, where a workgroup's
// detections share few labels).  Every index read from device memory (counts, labels) is clamped to the extents the host
// passed before it addresses anything; every loop is bounded by those extents.  The arithmetic is y3_beval_px.h's.
#include "y3_eval_common.h"
#include "y3_beval_px.h"

namespace {

using namespace y3ev;

constexpr int kPass = 1024;         // cells per pass of the gather = its workgroup size
constexpr int kWave = 64;
constexpr int kThreads = 256;       // match and tally
constexpr int kHist = 1024;         // labels below this are counted in LDS first

struct Scales {
    const float* y[3];
    int cells[3];       // grid_h * grid_w * 3 of each scale
};

// ------------------------------------------------------------------------------------------------ gather
__global__ __launch_bounds__(kPass) void beval_gather_kernel(Scales sc, int channels, int class_num, int gt_cap,
                                                             double* __restrict__ gt_box, int32_t* __restrict__ gt_label,
                                                             int32_t* __restrict__ gt_found, int32_t* __restrict__ gt_count,
                                                             int32_t* state) {
    __shared__ unsigned long long s_key[kPass];
    __shared__ int s_wave[kPass / kWave];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    double* box_i = gt_box + 4 * (size_t)i * gt_cap;
    int32_t* label_i = gt_label + (size_t)i * gt_cap;
    const int start1 = sc.cells[0], start2 = sc.cells[0] + sc.cells[1], cells = start2 + sc.cells[2];
    long long carry = 0;        // objects of this image before the pass (uniform over the workgroup)
    for (int c0 = 0; c0 < cells; c0 += kPass) {       // a pass: cells c0 .. c0 + m - 1 of the three scales laid end to end
        const int m = cells - c0 < kPass ? cells - c0 : kPass;
        s_key[tid] = 0;
        __syncthreads();
        for (int s = 0; s < 3; ++s) {
            const int start = s == 0 ? 0 : (s == 1 ? start1 : start2), n_s = s == 0 ? sc.cells[0] : (s == 1 ? sc.cells[1] : sc.cells[2]);
            const int lo = c0 > start ? c0 : start, hi = c0 + m < start + n_s ? c0 + m : start + n_s;
            if (lo >= hi) continue;
            const float* p = (s == 0 ? sc.y[0] : (s == 1 ? sc.y[1] : sc.y[2])) + ((size_t)i * n_s + (lo - start)) * channels;
            const int span = (hi - lo) * channels;      // <= kPass * channels: checked by the host
            for (int e = tid; e < span; e += kPass) {
                const float v = p[e];
                if (v > 0.f) {
                    const int cell = e / channels, c = e - cell * channels - 5;
                    if (c >= 0 && c < class_num) atomicMax(&s_key[lo - c0 + cell], y3bpx::class_key(v, c));
                }
            }
        }
        __syncthreads();
        const unsigned long long key = tid < m ? s_key[tid] : 0;
        const bool has = key != 0;
        const unsigned long long mask = __ballot(has);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < kPass / kWave; ++w) {
            const int t = s_wave[w];
            before += w < wave ? t : 0;
            total += t;
        }
        const long long pos = carry + before;
        if (has && pos < gt_cap) {
            const int g = c0 + tid, s = g >= start2 ? 2 : (g >= start1 ? 1 : 0);
            const int start = s == 0 ? 0 : (s == 1 ? start1 : start2), n_s = s == 0 ? sc.cells[0] : (s == 1 ? sc.cells[1] : sc.cells[2]);
            const float* cell = (s == 0 ? sc.y[0] : (s == 1 ? sc.y[1] : sc.y[2])) + ((size_t)i * n_s + (g - start)) * channels;
            y3bpx::corner_box(cell, box_i + 4 * pos);
            label_i[pos] = y3bpx::key_label(key);
        }
        carry += total;
        __syncthreads();        // s_key and s_wave are rewritten by the next pass
    }
    const int kept = carry < gt_cap ? (int)carry : gt_cap;
    for (int j = tid; j < kept; j += kPass) gt_found[(size_t)i * gt_cap + j] = 0;
    if (tid == 0) {
        gt_count[i] = kept;
        if (carry > kept) atomicAdd(state, (int)(carry - kept));
    }
}

// ------------------------------------------------------------------------------------------------ match
// block (x, i): detections x * kThreads .. of image i
__global__ __launch_bounds__(kThreads) void beval_match_kernel(const float* __restrict__ ob, const int32_t* __restrict__ ol,
                                                               const int32_t* __restrict__ cnt, int cap, int class_num,
                                                               double iou_thresh, int gt_cap, const double* __restrict__ gt_box,
                                                               const int32_t* __restrict__ gt_label, int32_t* gt_found,
                                                               const int32_t* __restrict__ gt_count,
                                                               unsigned long long* table) {
    __shared__ double s_box[kThreads][4];
    __shared__ int s_hist[kHist];
    const int i = blockIdx.y, tid = threadIdx.x;
    const int k_i = clampi(cnt[i], 0, cap);
    const int k = blockIdx.x * kThreads + tid;
    if (blockIdx.x * kThreads >= k_i) return;       // (uniform over the workgroup)
    const bool live = k < k_i;
    const int bins = class_num < kHist ? class_num : kHist;
    for (int c = tid; c < bins; c += kThreads) s_hist[c] = 0;
    __syncthreads();
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    int label = -1;
    if (live) {
        const size_t src = (size_t)i * cap + k;
        const f32x4 b = *reinterpret_cast<const f32x4*>(ob + 4 * src);
        p[0] = b[0], p[1] = b[1], p[2] = b[2], p[3] = b[3];
        label = ol[src];
        if (label >= 0 && label < class_num) {       // np.bincount(...)[:num_classes]
            if (label < kHist) atomicAdd(&s_hist[label], 1);
            else atomicAdd(&table[3 * (size_t)label + 2], 1ull);
        }
    }
    const int g_i = clampi(gt_count[i], 0, gt_cap);
    const double* box_i = gt_box + 4 * (size_t)i * gt_cap;
    y3bpx::Best best = y3bpx::no_best();
    for (int g0 = 0; g0 < g_i; g0 += kThreads) {
        const int m = g_i - g0 < kThreads ? g_i - g0 : kThreads;
        if (tid < m)
            for (int q = 0; q < 4; ++q) s_box[tid][q] = box_i[4 * (size_t)(g0 + tid) + q];
        __syncthreads();
        if (live)
            for (int j = 0; j < m; ++j) y3bpx::consider(&best, g0 + j, y3bpx::iou(p, s_box[j]));
        __syncthreads();
    }
    if (live && best.j >= 0) {
        const size_t at = (size_t)i * gt_cap + best.j;
        if (y3bpx::is_hit(best, iou_thresh, gt_label[at], label)) gt_found[at] = 1;
    }
    __syncthreads();
    for (int c = tid; c < bins; c += kThreads)
        if (s_hist[c]) atomicAdd(&table[3 * (size_t)c + 2], (unsigned long long)s_hist[c]);
}

// ------------------------------------------------------------------------------------------------ tally
__global__ __launch_bounds__(kThreads) void beval_tally_kernel(int class_num, int gt_cap, const int32_t* __restrict__ gt_label,
                                                               const int32_t* __restrict__ gt_found,
                                                               const int32_t* __restrict__ gt_count, unsigned long long* table) {
    const int i = blockIdx.y;
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= clampi(gt_count[i], 0, gt_cap)) return;
    const size_t at = (size_t)i * gt_cap + j;
    const int label = clampi(gt_label[at], 0, class_num - 1);
    atomicAdd(&table[3 * (size_t)label + 1], 1ull);
    if (gt_found[at] != 0) atomicAdd(&table[3 * (size_t)label + 0], 1ull);
}

// y3_batch_eval's scratch: gt_box f64 [n][gt_cap][4] | gt_label i32 [n][gt_cap] | found i32 [n][gt_cap] | gt_count i32 [n]
struct Scratch {
    Carve at;
    int n, gt_cap;
    size_t slots = (size_t)n * gt_cap;
    double* gt_box = at.take<double>(4 * slots);
    int32_t* gt_label = at.take<int32_t>(slots);
    int32_t* gt_found = at.take<int32_t>(slots);
    int32_t* gt_count = at.take<int32_t>(n);
};

}  // namespace

extern "C" size_t y3_batch_eval_scratch_bytes(int n, int gt_cap) {
    return n > 0 && gt_cap > 0 ? Scratch{nullptr, n, gt_cap}.at.bytes() : 0;
}

extern "C" int y3_batch_eval(y3_ctx* ctx, const float* out_boxes, const int32_t* out_labels, const int32_t* out_counts, int n,
                             int cap, const float* y_true_1, const float* y_true_2, const float* y_true_3, int h, int w,
                             int class_num, double iou_thresh, int gt_cap, void* scratch, size_t scratch_bytes, long long* table,
                             int32_t* state) {
    Y3_CHECK_ARG(ctx && out_boxes && out_labels && out_counts && y_true_1 && y_true_2 && y_true_3 && scratch && table && state,
                 "y3_batch_eval: null argument");
    Y3_CHECK_ARG(n > 0 && cap > 0 && h > 0 && w > 0 && class_num > 0 && gt_cap > 0,
                 "y3_batch_eval: non-positive dimension (n=%d, cap=%d, h=%d, w=%d, class_num=%d, gt_cap=%d)", n, cap, h, w,
                 class_num, gt_cap);
    Y3_CHECK_ARG(h % 32 == 0 && w % 32 == 0, "y3_batch_eval: h=%d and w=%d must be multiples of 32", h, w);
    const long long kIntMax = 0x7FFFFFFFLL;
    const long long channels = 5LL + class_num + 1;
    const long long cells3 = 3LL * (h / 8) * (w / 8);      // the finest grid: the largest of the three
    Y3_CHECK_ARG(channels <= kIntMax && 3LL * class_num <= kIntMax && (long long)kPass * channels <= kIntMax,
                 "y3_batch_eval: class_num=%d is too large", class_num);
    const long long cells = 3LL * (h / 32) * (w / 32) + 3LL * (h / 16) * (w / 16) + cells3;
    Y3_CHECK_ARG((long long)n * cells <= kIntMax, "y3_batch_eval: n * cells = %d * %lld exceeds 2^31 - 1", n, cells);
    Y3_CHECK_ARG((long long)n * cap <= kIntMax, "y3_batch_eval: n * cap = %lld exceeds 2^31 - 1", (long long)n * cap);
    Y3_CHECK_ARG((long long)n * gt_cap <= kIntMax, "y3_batch_eval: n * gt_cap = %lld exceeds 2^31 - 1", (long long)n * gt_cap);
    Y3_CHECK_ARG(n <= 65535, "y3_batch_eval: n=%d exceeds 65535 images", n);
    Y3_CHECK_ARG(scratch_bytes >= y3_batch_eval_scratch_bytes(n, gt_cap), "y3_batch_eval: scratch too small (%zu < %zu)",
                 scratch_bytes, y3_batch_eval_scratch_bytes(n, gt_cap));
    Y3_CHECK_ARG(aligned(out_boxes, 16), "y3_batch_eval: out_boxes must be 16-byte aligned");
    Y3_CHECK_ARG(aligned(scratch, 8) && aligned(table, 8) && aligned(out_labels, 4) && aligned(out_counts, 4) &&
                     aligned(y_true_1, 4) && aligned(y_true_2, 4) && aligned(y_true_3, 4) && aligned(state, 4),
                 "y3_batch_eval: misaligned pointer");
    const Scratch ws{scratch, n, gt_cap};
    Scales sc;
    sc.y[0] = y_true_1, sc.y[1] = y_true_2, sc.y[2] = y_true_3;
    sc.cells[0] = 3 * (h / 32) * (w / 32), sc.cells[1] = 3 * (h / 16) * (w / 16), sc.cells[2] = 3 * (h / 8) * (w / 8);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(table);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(beval_gather_kernel, dim3(n), dim3(kPass), 0, st, sc, (int)channels, class_num, gt_cap, ws.gt_box,
                       ws.gt_label, ws.gt_found, ws.gt_count, state);
    Y3_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(beval_match_kernel, dim3((cap + kThreads - 1) / kThreads, n), dim3(kThreads), 0, st, out_boxes, out_labels,
                       out_counts, cap, class_num, iou_thresh, gt_cap, ws.gt_box, ws.gt_label, ws.gt_found, ws.gt_count, counts);
    Y3_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(beval_tally_kernel, dim3((gt_cap + kThreads - 1) / kThreads, n), dim3(kThreads), 0, st, class_num, gt_cap,
                       ws.gt_label, ws.gt_found, ws.gt_count, counts);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}
