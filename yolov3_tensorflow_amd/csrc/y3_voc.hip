// PASCAL VOC evaluation on the device (include/yolo355.h: y3_voc_append / y3_voc_match / y3_voc_ap): what
// eval_utils.get_preds_batch + voc_eval do per detection in Python, on the tensors the NMS kernels leave in HBM.
//
//   append   one batch of y3_nms outputs -> rows of a caller-owned struct-of-arrays arena (fp32 widened to fp64, exactly)
//   match    per ranked detection: best object of its image and class, the flag ov > iou_thres, and a 32-bit atomicMin of
//            the rank on the object's claim word; a second launch turns "my rank is the claim" into tp.  The smallest rank
//            does not depend on the order the atomics arrive in, so tp is the same in every run
//   ap       one workgroup per class over its contiguous ranked segment, in passes of Y3_VOC_AP_PASS ranks: an integer
//            inclusive scan of tp forwards, the precision envelope and the area sum backwards, each in a fixed order
//
// Every index read from device memory (counts, image indices, CSR offsets, order, labels) is clamped to the extents the
// host passed before it addresses anything; every loop is bounded by those extents.  The arithmetic is y3_voc_px.h's.
#include "y3_eval_common.h"
#include "y3_voc_px.h"

namespace {

using namespace y3ev;

constexpr int kThreads = 256;
constexpr int kItems = 4;
constexpr int kPass = kThreads * kItems;      // ranks of a class one pass of voc_ap_kernel covers (y3_voc_ap_pass)

// ------------------------------------------------------------------------------------------------ append
// block (i, y): rows of batch image i.  Its first arena row = the running total + the exclusive scan of the counts at i.
__global__ __launch_bounds__(kThreads) void voc_append_kernel(const float* __restrict__ ob, const float* __restrict__ osc,
                                                              const int32_t* __restrict__ ol, const int32_t* __restrict__ cnt,
                                                              const int32_t* __restrict__ img, int n, int cap,
                                                              double* __restrict__ box, double* __restrict__ score,
                                                              int32_t* __restrict__ label, int32_t* __restrict__ image,
                                                              int capacity, const int32_t* __restrict__ state) {
    __shared__ long long s_part[kThreads];
    const int i = blockIdx.x, tid = threadIdx.x;
    long long part = 0;
    for (int j = tid; j < i; j += kThreads) part += clampi(cnt[j], 0, cap);
    const long long base = (long long)clampi(state[0], 0, capacity) + block_sum<kThreads>(part, s_part);
    const int k_i = clampi(cnt[i], 0, cap);
    const int image_index = img[i];
    for (int k = blockIdx.y * kThreads + tid; k < k_i; k += gridDim.y * kThreads) {
        const long long pos = base + k;
        if (pos >= capacity) break;       // (counted by voc_append_total_kernel)
        const size_t src = (size_t)i * cap + k;
        const f32x4 b = *reinterpret_cast<const f32x4*>(ob + 4 * src);
        double* o = box + 4 * pos;
        o[0] = (double)b[0];
        o[1] = (double)b[1];
        o[2] = (double)b[2];
        o[3] = (double)b[3];
        score[pos] = (double)osc[src];
        label[pos] = ol[src];
        image[pos] = image_index;
    }
}

// one block, after voc_append_kernel on the stream: state[0] += rows written, state[1] += rows that did not fit
__global__ __launch_bounds__(kThreads) void voc_append_total_kernel(const int32_t* __restrict__ cnt, int n, int cap, int capacity,
                                                                    int32_t* __restrict__ state) {
    __shared__ long long s_part[kThreads];
    const int tid = threadIdx.x;
    long long part = 0;
    for (int j = tid; j < n; j += kThreads) part += clampi(cnt[j], 0, cap);
    const long long added = block_sum<kThreads>(part, s_part);
    if (tid == 0) {
        const long long before = clampi(state[0], 0, capacity);
        const long long want = before + added;
        const long long now = want < capacity ? want : capacity;
        const long long lost = (long long)clampi(state[1], 0, 0x7FFFFFFF) + (want - now);
        state[0] = (int32_t)now;
        state[1] = (int32_t)(lost < 0x7FFFFFFF ? lost : 0x7FFFFFFF);
    }
}

// ------------------------------------------------------------------------------------------------ match
__global__ __launch_bounds__(kThreads) void voc_match_kernel(const double* __restrict__ box, const int32_t* __restrict__ label,
                                                             const int32_t* __restrict__ image, const int32_t* __restrict__ order,
                                                             int rows, const int32_t* __restrict__ n_rows_dev,
                                                             const int32_t* __restrict__ gt_start, const double* __restrict__ gt_box,
                                                             const int32_t* __restrict__ gt_label, int num_images, int num_gt,
                                                             double iou_thres, int32_t* __restrict__ jstar, unsigned* claim) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= ranked_total(n_rows_dev, rows)) return;
    int j = -1;
    const int row = order[r];
    if (row >= 0 && row < rows) {
        const int im = image[row];
        if (im >= 0 && im < num_images) {
            const int g0 = clampi(gt_start[im], 0, num_gt), g1 = clampi(gt_start[im + 1], g0, num_gt);
            const double bb[4] = {box[4 * (size_t)row], box[4 * (size_t)row + 1], box[4 * (size_t)row + 2], box[4 * (size_t)row + 3]};
            j = y3vpx::best_object(bb, label[row], gt_box, gt_label, g0, g1, iou_thres);
        }
    }
    jstar[r] = j;
    if (j >= 0) atomicMin(&claim[j], (unsigned)r);      // the most confident detection of this object: eval_utils.py:235-237
}

__device__ __forceinline__ int label_at_rank(const int32_t* label, const int32_t* order, int rows, int class_num, long long r) {
    const int row = order[r];
    return (row >= 0 && row < rows) ? clampi(label[row], 0, class_num - 1) : 0;
}

// tp of every rank (0 past the ranked rows), and seg_start[c] = the first rank of class c (seg_start[class_num] = the end)
__global__ __launch_bounds__(kThreads) void voc_tp_kernel(const int32_t* __restrict__ jstar, const unsigned* __restrict__ claim,
                                                          const int32_t* __restrict__ label, const int32_t* __restrict__ order,
                                                          int rows, const int32_t* __restrict__ n_rows_dev, int num_gt, int class_num,
                                                          uint8_t* __restrict__ tp, int32_t* __restrict__ seg_start) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int total = ranked_total(n_rows_dev, rows);
    if (r == 0 && total == 0)
        for (int c = 0; c <= class_num; ++c) seg_start[c] = 0;
    if (r >= rows) return;
    if (r >= total) {
        tp[r] = 0;
        return;
    }
    const int j = jstar[r];
    tp[r] = (j >= 0 && j < num_gt && claim[j] == (unsigned)r) ? 1 : 0;
    const int l = label_at_rank(label, order, rows, class_num, r);
    const int before = r > 0 ? label_at_rank(label, order, rows, class_num, r - 1) : -1;
    for (int c = before + 1; c <= l; ++c) seg_start[c] = (int32_t)r;
    if (r == total - 1)
        for (int c = l + 1; c <= class_num; ++c) seg_start[c] = total;
}

// ------------------------------------------------------------------------------------------------ ap
struct Thresholds {
    double t[11];
};

// block c: class c's row of out = (npos, nd, recall, precision, ap), eval_utils.py:207-217 and 238-244
__global__ __launch_bounds__(kThreads) void voc_ap_kernel(const uint8_t* __restrict__ tp, const int32_t* __restrict__ seg_start, int rows,
                                                          const int32_t* __restrict__ gt_label, int num_gt, int use_07_metric,
                                                          Thresholds thr, int32_t* ctp, double* __restrict__ out) {
    __shared__ int s_int[kThreads];
    __shared__ double s_dbl[kThreads];
    const int c = blockIdx.x, tid = threadIdx.x;
    int mine = 0, npos = 0;
    for (int g = tid; g < num_gt; g += kThreads) mine += gt_label[g] == c;
    block_excl_sum<kThreads>(mine, s_int, &npos);
    const int s = clampi(seg_start[c], 0, rows), e = clampi(seg_start[c + 1], s, rows), nd = e - s;
    double* o = out + 5 * (size_t)c;
    if (nd == 0) {      // 'no box, ignore'
        if (tid == 0) {
            o[0] = 1e-6;
            o[1] = 1e-6;
            o[2] = 0.;
            o[3] = 0.;
            o[4] = 0.;
        }
        return;
    }
    const uint8_t* tpc = tp + s;
    int32_t* ctpc = ctp + s;
    // forwards: ctp[i] = true positives among ranks 0..i; the 11-point maxima on the way
    double best[11];
    for (int k = 0; k < 11; ++k) best[k] = 0.;
    int carry = 0;
    for (int p0 = 0; p0 < nd; p0 += kPass) {
        const int i0 = p0 + tid * kItems;
        int v[kItems], sum = 0;
        for (int k = 0; k < kItems; ++k) {
            v[k] = i0 + k < nd ? (tpc[i0 + k] != 0) : 0;
            sum += v[k];
        }
        int pass_total;
        int run = carry + block_excl_sum<kThreads>(sum, s_int, &pass_total);
        for (int k = 0; k < kItems; ++k) {
            const int i = i0 + k;
            if (i >= nd) break;
            run += v[k];
            ctpc[i] = run;
            if (use_07_metric) {
                const double rec = y3vpx::recall_at(run, npos), prec = y3vpx::precision_at(run, i);
                for (int t = 0; t < 11; ++t)
                    if (rec >= thr.t[t]) best[t] = y3vpx::dmax(best[t], prec);
            }
        }
        carry += pass_total;
    }
    __syncthreads();      // every ctp of the class is written before the backward passes read a neighbour's
    double ap;
    if (use_07_metric) {
        for (int t = 0; t < 11; ++t) best[t] = block_max<kThreads>(best[t], s_dbl);
        ap = y3vpx::eleven_point(best);
    } else {
        // backwards: the envelope at rank i = max(prec[i..nd-1], 0.); each thread adds the area terms of its ranks in
        // descending order over the passes, and the threads' sums meet in a fixed tree
        double env_right = 0., acc = 0.;
        const int passes = (nd + kPass - 1) / kPass;
        for (int p = passes - 1; p >= 0; --p) {
            const int i0 = p * kPass + tid * kItems;
            double prec[kItems], tmax = 0.;
            int cnt_tp[kItems];
            for (int k = 0; k < kItems; ++k) {
                const int i = i0 + k;
                cnt_tp[k] = i < nd ? ctpc[i] : 0;
                prec[k] = i < nd ? y3vpx::precision_at(cnt_tp[k], i) : 0.;
                tmax = y3vpx::dmax(tmax, prec[k]);
            }
            double pass_max;
            double env = y3vpx::dmax(env_right, block_right_max<kThreads>(tmax, s_dbl, &pass_max));
            for (int k = kItems - 1; k >= 0; --k) {
                const int i = i0 + k;
                if (i >= nd) continue;
                env = y3vpx::dmax(env, prec[k]);
                const int prev = k > 0 ? cnt_tp[k - 1] : (i > 0 ? ctpc[i - 1] : 0);
                const double rec_before = i > 0 ? y3vpx::recall_at(prev, npos) : 0.;
                bool take;
                const double term = y3vpx::area_term(rec_before, y3vpx::recall_at(cnt_tp[k], npos), env, &take);
                if (take) acc = acc + term;
            }
            env_right = y3vpx::dmax(env_right, pass_max);
        }
        ap = block_sum<kThreads>(acc, s_dbl);
        bool take;      // the closing position of the padded arrays: mrec 1., mpre 0.
        const double term = y3vpx::area_term(y3vpx::recall_at(carry, npos), 1., 0., &take);
        if (take) ap = ap + term;
    }
    if (tid == 0) {
        o[0] = (double)npos;
        o[1] = (double)nd;
        o[2] = (double)carry / (double)npos;
        o[3] = (double)carry / (double)nd;
        o[4] = ap;
    }
}

// y3_voc_match's scratch: the best object of every rank | the claim word of every object (one for an empty set)
struct MatchScratch {
    Carve at;
    int rows, num_gt;
    size_t claim_words = num_gt > 0 ? num_gt : 1;
    int32_t* jstar = at.take<int32_t>(rows);
    unsigned* claim = at.take<unsigned>(claim_words);
};

// y3_voc_ap's scratch: the running true-positive count of every rank
struct ApScratch {
    Carve at;
    int rows;
    int32_t* ctp = at.take<int32_t>(rows);
};

}  // namespace

extern "C" int y3_voc_ap_pass(void) { return kPass; }

extern "C" int y3_voc_append(y3_ctx* ctx, const float* out_boxes, const float* out_scores, const int32_t* out_labels,
                             const int32_t* out_counts, const int32_t* image_index, int n, int cap, double* arena_box,
                             double* arena_score, int32_t* arena_label, int32_t* arena_image, int capacity_rows, int32_t* state) {
    Y3_CHECK_ARG(ctx && out_boxes && out_scores && out_labels && out_counts && image_index && arena_box && arena_score &&
                     arena_label && arena_image && state,
                 "y3_voc_append: null argument");
    Y3_CHECK_ARG(n > 0 && cap > 0 && capacity_rows > 0, "y3_voc_append: non-positive dimension (n=%d, cap=%d, capacity_rows=%d)", n,
                 cap, capacity_rows);
    Y3_CHECK_ARG((long long)n * cap <= 0x7FFFFFFFLL, "y3_voc_append: n * cap = %lld rows exceed 2^31 - 1", (long long)n * cap);
    Y3_CHECK_ARG(aligned(out_boxes, 16), "y3_voc_append: out_boxes must be 16-byte aligned");
    Y3_CHECK_ARG(aligned(arena_box, 8) && aligned(arena_score, 8) && aligned(out_scores, 4) && aligned(out_labels, 4) &&
                     aligned(out_counts, 4) && aligned(image_index, 4) && aligned(arena_label, 4) && aligned(arena_image, 4) &&
                     aligned(state, 4),
                 "y3_voc_append: misaligned pointer");
    const int by = (cap + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(voc_append_kernel, dim3(n, by < 32 ? by : 32), dim3(kThreads), 0, ctx->stream, out_boxes, out_scores,
                       out_labels, out_counts, image_index, n, cap, arena_box, arena_score, arena_label, arena_image, capacity_rows,
                       state);
    Y3_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(voc_append_total_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, out_counts, n, cap, capacity_rows, state);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}

extern "C" size_t y3_voc_match_scratch_bytes(int rows, int num_gt) {
    return rows > 0 && num_gt >= 0 ? MatchScratch{nullptr, rows, num_gt}.at.bytes() : 0;
}

extern "C" int y3_voc_match(y3_ctx* ctx, const double* arena_box, const int32_t* arena_label, const int32_t* arena_image,
                            const int32_t* order, int rows, const int32_t* n_rows_dev, const int32_t* gt_start, const double* gt_box,
                            const int32_t* gt_label, int num_images, int num_gt, int class_num, double iou_thres, void* scratch,
                            size_t scratch_bytes, uint8_t* tp, int32_t* seg_start) {
    Y3_CHECK_ARG(ctx && arena_box && arena_label && arena_image && order && gt_start && gt_box && gt_label && scratch && tp &&
                     seg_start,
                 "y3_voc_match: null argument");
    Y3_CHECK_ARG(rows > 0 && num_images > 0 && num_gt >= 0 && class_num > 0,
                 "y3_voc_match: bad dimension (rows=%d, num_images=%d, num_gt=%d, class_num=%d)", rows, num_images, num_gt, class_num);
    Y3_CHECK_ARG(scratch_bytes >= y3_voc_match_scratch_bytes(rows, num_gt), "y3_voc_match: scratch too small (%zu < %zu)",
                 scratch_bytes, y3_voc_match_scratch_bytes(rows, num_gt));
    Y3_CHECK_ARG(aligned(arena_box, 8) && aligned(gt_box, 8) && aligned(scratch, 4) && aligned(arena_label, 4) &&
                     aligned(arena_image, 4) && aligned(order, 4) && aligned(gt_start, 4) && aligned(gt_label, 4) &&
                     aligned(seg_start, 4) && (!n_rows_dev || aligned(n_rows_dev, 4)),
                 "y3_voc_match: misaligned pointer");
    const MatchScratch ws{scratch, rows, num_gt};
    hipStream_t st = ctx->stream;
    Y3_CHECK_HIP(hipMemsetAsync(ws.claim, 0xFF, ws.claim_words * 4, st));      // y3vpx::kUnclaimed
    Y3_CHECK_HIP(hipMemsetAsync(seg_start, 0, (size_t)(class_num + 1) * 4, st));
    const unsigned blocks = (unsigned)(((long long)rows + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(voc_match_kernel, dim3(blocks), dim3(kThreads), 0, st, arena_box, arena_label, arena_image, order, rows,
                       n_rows_dev, gt_start, gt_box, gt_label, num_images, num_gt, iou_thres, ws.jstar, ws.claim);
    Y3_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(voc_tp_kernel, dim3(blocks), dim3(kThreads), 0, st, ws.jstar, ws.claim, arena_label, order, rows, n_rows_dev, num_gt,
                       class_num, tp, seg_start);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}

extern "C" size_t y3_voc_ap_scratch_bytes(int rows) { return rows > 0 ? ApScratch{nullptr, rows}.at.bytes() : 0; }

extern "C" int y3_voc_ap(y3_ctx* ctx, const uint8_t* tp, const int32_t* seg_start, int rows, const int32_t* gt_label, int num_gt,
                         int class_num, int use_07_metric, const double* thresholds_host11, void* scratch, size_t scratch_bytes,
                         double* out) {
    Y3_CHECK_ARG(ctx && tp && seg_start && gt_label && scratch && out, "y3_voc_ap: null argument");
    Y3_CHECK_ARG(rows > 0 && num_gt >= 0 && class_num > 0, "y3_voc_ap: bad dimension (rows=%d, num_gt=%d, class_num=%d)", rows,
                 num_gt, class_num);
    Y3_CHECK_ARG(!use_07_metric || thresholds_host11, "y3_voc_ap: the 11-point metric needs its thresholds");
    Y3_CHECK_ARG(scratch_bytes >= y3_voc_ap_scratch_bytes(rows), "y3_voc_ap: scratch too small (%zu < %zu)", scratch_bytes,
                 y3_voc_ap_scratch_bytes(rows));
    Y3_CHECK_ARG(aligned(out, 8) && aligned(scratch, 4) && aligned(seg_start, 4) && aligned(gt_label, 4),
                 "y3_voc_ap: misaligned pointer");
    Thresholds thr;
    for (int k = 0; k < 11; ++k) thr.t[k] = use_07_metric ? thresholds_host11[k] : 0.;
    hipLaunchKernelGGL(voc_ap_kernel, dim3(class_num), dim3(kThreads), 0, ctx->stream, tp, seg_start, rows, gt_label, num_gt,
                       use_07_metric ? 1 : 0, thr, ApScratch{scratch, rows}.ctp, out);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}
