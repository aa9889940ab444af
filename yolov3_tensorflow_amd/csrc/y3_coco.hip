// COCO bbox evaluation on the device (include/yolo355.h: y3_coco_match / y3_coco_ap / y3_coco_summary): what
// eval_utils.coco_eval does on the host, on the arena y3_voc_append fills (csrc/y3_voc.hip).
//
//   match    the greedy matching is sequential inside an (image, class) group and parallel over groups, thresholds and area
//            ranges.  A workgroup takes 256 consecutive ranks of `order`, finds the groups that BEGIN among them and deals them
//            to its four wavefronts.  Per detection of a group (at most 100) the wave computes one row of IoUs co-operatively
//            (lanes over the image's objects, 64 at a time, into the LDS); then lanes 0..39, one per (threshold, area range),
//            walk that row in ground-truth order.  "Object taken" is one 64-bit word per object, bit = lane: in the LDS for
//            images of up to kLdsObjs objects, else in the scratch (every object belongs to exactly one group, so no two
//            waves share a word).  A wave-wide ballot turns the 40 lanes' verdicts into the two words of the rank.
//   npig     a pass of its own over the objects, integer atomics
//   ap       a gather into class order (order2), then one workgroup per (class, area range, max-dets, threshold): an integer
//            block sum of true / false positives over the class's segment, then passes of kPass ranks from the right - a
//            block scan gives the counts at every position, a block max from the right the precision envelope, and the
//            position where the recall first reaches a threshold writes that threshold's sample.  No thread walks a segment.
//   summary  per class, then over classes, each a strided sum and a fixed tree
//
// No floating-point atomics, no hand-off between workgroups inside a kernel: stages that depend on each other are launches
// on the one stream.  Every index read from device memory is clamped to the extents the host passed before it addresses
// anything; every loop is bounded by those extents.  The arithmetic is y3_coco_px.h's.
#include "y3_eval_common.h"
#include "y3_coco_px.h"

namespace {

using namespace y3ev;
using namespace y3cpx;
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 4;
constexpr int kPass = kThreads * kItems;      // ranks of a class one pass of coco_ap_kernel covers (y3_coco_ap_pass)
constexpr int kLdsObjs = 512;                 // objects of one image whose "taken" words a wave keeps in the LDS (y3_coco_lds_objects)

struct IouThrs {
    double t[kIouThrs];
};
struct RecThrs {
    double r[kRecThrs];
};

// lanes of one wave exchange data through the LDS: order the accesses for the compiler (the hardware runs a wave's LDS
// instructions in order)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------ match
struct Ranked {
    const int32_t *order, *label, *image;
    int rows, num_images, class_num;
};
__device__ __forceinline__ int row_at(const Ranked& q, int r) { return clampi(q.order[r], 0, q.rows - 1); }
// image * class_num + label of rank r (both clamped): ascending along `order`
__device__ __forceinline__ int key_at(const Ranked& q, int r) {
    const int row = row_at(q, r);
    return clampi(q.image[row], 0, q.num_images - 1) * q.class_num + clampi(q.label[row], 0, q.class_num - 1);
}

// One wave, all 64 lanes with the same arguments: the group that begins at rank h.
__device__ void match_group(const Ranked& q, const double* __restrict__ box, int h, int total, const int32_t* __restrict__ gt_start,
                            const double* __restrict__ gt_box, const int32_t* __restrict__ gt_label,
                            const double* __restrict__ area_scale, int num_gt, const double* s_floor, u64* s_taken, double* s_iou,
                            unsigned* s_ig, u64* taken_big, u64* __restrict__ matched, u64* __restrict__ ignored,
                            uint8_t* __restrict__ group_rank) {
    const int lane = threadIdx.x & 63;
    const int key = key_at(q, h);
    int end = total;      // the group's end: the first rank behind h with another key, looked for 64 ranks at a time
    for (int b = h + 1; b < total; b += 64) {
        const int r = b + lane;
        const u64 other = __ballot(r < total && key_at(q, r) != key);
        if (other) {
            end = b + __builtin_ctzll(other);
            break;
        }
    }
    const int nd = end - h, kept = nd < kMaxDets ? nd : kMaxDets;
    for (int i = kept + lane; i < nd; i += 64) {      // behind the cut: never matched, never counted
        matched[h + i] = 0;
        ignored[h + i] = 0;
        group_rank[h + i] = (uint8_t)(i < kRankSaturated ? i : kRankSaturated);
    }
    const int im = key / q.class_num, cls = key - im * q.class_num;
    const int g0 = clampi(gt_start[im], 0, num_gt), g1 = clampi(gt_start[im + 1], g0, num_gt), n_img = g1 - g0;
    const double scale = area_scale ? area_scale[im] : 1.;
    const bool in_lds = n_img <= kLdsObjs;
    if (in_lds)
        for (int j = lane; j < n_img; j += 64) s_taken[j] = 0;
    const bool active = lane < kLanes;
    const int a = lane & 3;
    const double flr = active ? s_floor[lane >> 2] : 2.;
    wave_sync();
    for (int d = 0; d < kept; ++d) {
        const int r = h + d;
        const size_t row = (size_t)row_at(q, r);
        const double bb[4] = {box[4 * row], box[4 * row + 1], box[4 * row + 2], box[4 * row + 3]};
        const bool outside = (outside_mask(area(bb, scale)) >> a) & 1u;
        Greedy s;
        greedy_begin(&s, flr);
        for (int c0 = 0; c0 < n_img; c0 += 64) {
            const int g = g0 + c0 + lane;
            const bool mine = c0 + lane < n_img && gt_label[g] == cls;
            if (mine) {
                const double* gb = gt_box + 4 * (size_t)g;
                s_iou[lane] = iou(bb, gb);
                s_ig[lane] = outside_mask(area(gb, scale));
            }
            u64 todo = __ballot(mine);
            wave_sync();
            while (todo) {      // the class's objects of this chunk, in ground-truth order (the same in every lane)
                const int o = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int idx = c0 + o;
                const u64 tk = in_lds ? s_taken[idx] : __hip_atomic_load(taken_big + g0 + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (active && !((tk >> lane) & 1ull)) greedy_step(&s, s_iou[o], (s_ig[o] >> a) & 1u, idx);
            }
            wave_sync();
        }
        bool ig = false;
        const int m = active ? greedy_end(&s, outside, &ig) : -1;
        if (m >= 0) {
            if (in_lds)
                atomicOr(&s_taken[m], 1ull << lane);
            else
                atomicOr(&taken_big[g0 + m], 1ull << lane);
        }
        if (!in_lds) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the words are at the L2 before the next row reads them there
        const u64 mw = __ballot(m >= 0), iw = __ballot(active && ig);
        wave_sync();
        if (lane == 0) {
            matched[r] = mw;
            ignored[r] = iw;
            group_rank[r] = (uint8_t)d;
        }
    }
}

__global__ __launch_bounds__(kThreads) void coco_match_kernel(const double* __restrict__ box, const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ image, const int32_t* __restrict__ order,
                                                              int rows, const int32_t* __restrict__ n_rows_dev,
                                                              const int32_t* __restrict__ gt_start, const double* __restrict__ gt_box,
                                                              const int32_t* __restrict__ gt_label,
                                                              const double* __restrict__ area_scale, int num_images, int num_gt,
                                                              int class_num, IouThrs thr, u64* taken_big, u64* __restrict__ matched,
                                                              u64* __restrict__ ignored, uint8_t* __restrict__ group_rank) {
    __shared__ u64 s_taken[kWaves][kLdsObjs];
    __shared__ double s_iou[kWaves][64];
    __shared__ unsigned s_ig[kWaves][64];
    __shared__ double s_floor[kIouThrs];
    __shared__ int s_heads[kThreads];
    __shared__ int s_nheads;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int total = ranked_total(n_rows_dev, rows);
    const Ranked q = {order, label, image, rows, num_images, class_num};
    if (tid == 0) s_nheads = 0;
    if (tid < kIouThrs) s_floor[tid] = greedy_floor(thr.t[tid]);
    __syncthreads();
    const long long r = (long long)blockIdx.x * kThreads + tid;
    if (r >= total && r < rows) {      // not a detection
        matched[r] = 0;
        ignored[r] = 0;
        group_rank[r] = (uint8_t)kRankSaturated;
    }
    if (r < total && (r == 0 || key_at(q, (int)r - 1) != key_at(q, (int)r)))
        s_heads[atomicAdd(&s_nheads, 1)] = (int)r;      // (any order: the groups do not depend on one another)
    __syncthreads();
    const int nheads = s_nheads;
    for (int i = wave; i < nheads; i += kWaves)
        match_group(q, box, s_heads[i], total, gt_start, gt_box, gt_label, area_scale, num_gt, s_floor, s_taken[wave], s_iou[wave],
                    s_ig[wave], taken_big, matched, ignored, group_rank);
}

// npig[k][a] += objects of class k whose area is inside range a
__global__ __launch_bounds__(kThreads) void coco_npig_kernel(const int32_t* __restrict__ gt_start, const double* __restrict__ gt_box,
                                                             const int32_t* __restrict__ gt_label,
                                                             const double* __restrict__ area_scale, int num_images, int num_gt,
                                                             int class_num, int32_t* npig) {
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= num_gt) return;
    const int k = gt_label[g];
    if (k < 0 || k >= class_num) return;
    int lo = 0, hi = num_images;      // the image of object g: the last one whose start is <= g
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (gt_start[mid + 1] <= g)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int im = clampi(lo, 0, num_images - 1);
    const unsigned out = outside_mask(area(gt_box + 4 * (size_t)g, area_scale ? area_scale[im] : 1.));
    for (int a = 0; a < kAreas; ++a)
        if (!((out >> a) & 1u)) atomicAdd(&npig[k * kAreas + a], 1);
}

// ------------------------------------------------------------------------------------------------ ap
// position i of order2 -> the words of its rank and its class, so that the AP workgroups read their segment contiguously
__global__ __launch_bounds__(kThreads) void coco_gather_kernel(const u64* __restrict__ matched, const u64* __restrict__ ignored,
                                                               const uint8_t* __restrict__ group_rank,
                                                               const int32_t* __restrict__ label, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ order2, int rows,
                                                               const int32_t* __restrict__ n_rows_dev, int class_num,
                                                               u64* __restrict__ mw2, u64* __restrict__ iw2,
                                                               int32_t* __restrict__ lab2, uint8_t* __restrict__ gr2) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= rows) return;
    const int total = ranked_total(n_rows_dev, rows);
    if (i >= total) {
        mw2[i] = 0;
        iw2[i] = 0;
        lab2[i] = class_num;
        gr2[i] = (uint8_t)kRankSaturated;
        return;
    }
    const int r = clampi(order2[i], 0, total - 1);
    mw2[i] = matched[r];
    iw2[i] = ignored[r];
    gr2[i] = group_rank[r];
    lab2[i] = clampi(label[clampi(order[r], 0, rows - 1)], 0, class_num - 1);
}

// (true positive << 32) | false positive of one position at bit `bit`, among a group's first `max_dets`
__device__ __forceinline__ u64 tp_fp(u64 mw, u64 iw, int grank, int bit, int max_dets) {
    if (grank >= max_dets || ((iw >> bit) & 1ull)) return 0;
    return ((mw >> bit) & 1ull) ? (1ull << 32) : 1ull;
}

// block (k, a * 3 + m, t): precision[t][.][k][a][m] and recall[t][k][a][m]
__global__ __launch_bounds__(kThreads) void coco_ap_kernel(const u64* __restrict__ mw2, const u64* __restrict__ iw2,
                                                           const int32_t* __restrict__ lab2, const uint8_t* __restrict__ gr2, int rows,
                                                           const int32_t* __restrict__ n_rows_dev, const int32_t* __restrict__ npig,
                                                           int class_num, RecThrs thr, double* __restrict__ precision,
                                                           double* __restrict__ recall) {
    __shared__ double s_thr[kRecThrs];
    __shared__ u64 s_u64[kThreads];
    __shared__ double s_dbl[kThreads];
    __shared__ int s_seg[2];
    const int tid = threadIdx.x;
    const int k = blockIdx.x, a = blockIdx.y / kMaxDetKinds, m = blockIdx.y % kMaxDetKinds, t = blockIdx.z;
    const int bit = t * kAreas + a, max_dets = max_dets_of(m);
    const int np = npig[k * kAreas + a];
    if (np <= 0) {      // no object that counts: nothing is defined
        for (int r = tid; r < kRecThrs; r += kThreads) precision[precision_index(t, r, k, a, m, class_num)] = -1.;
        if (tid == 0) recall[recall_index(t, k, a, m, class_num)] = -1.;
        return;
    }
    for (int r = tid; r < kRecThrs; r += kThreads) s_thr[r] = thr.r[r];
    const int total = ranked_total(n_rows_dev, rows);
    if (tid < 2) {      // the class's segment of order2: the first position with a label >= k, >= k + 1
        int lo = 0, hi = total;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (lab2[mid] < k + tid)
                lo = mid + 1;
            else
                hi = mid;
        }
        s_seg[tid] = lo;
    }
    __syncthreads();
    const int s = s_seg[0], e = s_seg[1] < s ? s : s_seg[1], nd = e - s;
    const u64* mw = mw2 + s;
    const u64* iw = iw2 + s;
    const uint8_t* gr = gr2 + s;
    u64 part = 0;
    for (int i = tid; i < nd; i += kThreads) part += tp_fp(mw[i], iw[i], gr[i], bit, max_dets);
    u64 after;      // the counts behind the positions still to visit
    block_excl_sum<kThreads>(part, s_u64, &after);
    const int tp_all = (int)(after >> 32);
    if (tid == 0) recall[recall_index(t, k, a, m, class_num)] = recall_at(tp_all, np);
    // thresholds no position reaches: 0.
    const int reached = nd > 0 ? thresholds_reached(recall_at(tp_all, np), s_thr, kRecThrs) : 0;
    for (int r = reached + tid; r < kRecThrs; r += kThreads) precision[precision_index(t, r, k, a, m, class_num)] = 0.;
    double env_right = 0.;
    const int passes = (nd + kPass - 1) / kPass;
    for (int p = passes - 1; p >= 0; --p) {
        const int i0 = p * kPass + tid * kItems;
        u64 v[kItems], sum = 0;
        for (int j = 0; j < kItems; ++j) {
            const int i = i0 + j;
            v[j] = i < nd ? tp_fp(mw[i], iw[i], gr[i], bit, max_dets) : 0;
            sum += v[j];
        }
        u64 pass_total;
        const u64 excl = block_excl_sum<kThreads>(sum, s_u64, &pass_total);
        const u64 before = after - pass_total;
        u64 run = before + excl;
        int tp_before = (int)(run >> 32), tp[kItems];
        double prec[kItems], tmax = 0.;
        for (int j = 0; j < kItems; ++j) {
            run += v[j];
            tp[j] = (int)(run >> 32);
            prec[j] = i0 + j < nd ? precision_at(tp[j], (int)(run & 0xFFFFFFFFull)) : 0.;
            tmax = dmax(tmax, prec[j]);
        }
        double pass_max;
        double env = dmax(env_right, block_right_max<kThreads>(tmax, s_dbl, &pass_max));
        double envs[kItems];
        for (int j = kItems - 1; j >= 0; --j) {
            env = dmax(env, prec[j]);
            envs[j] = env;
        }
        for (int j = 0; j < kItems; ++j) {
            const int i = i0 + j;
            if (i >= nd) break;
            const int prev = j > 0 ? tp[j - 1] : tp_before;
            if (i > 0 && prev == tp[j]) continue;      // the recall did not move: no threshold is first reached here
            const int r0 = i > 0 ? thresholds_reached(recall_at(prev, np), s_thr, kRecThrs) : 0;
            const int r1 = thresholds_reached(recall_at(tp[j], np), s_thr, kRecThrs);
            for (int r = r0; r < r1; ++r) precision[precision_index(t, r, k, a, m, class_num)] = envs[j];
        }
        env_right = dmax(env_right, pass_max);
        after = before;
    }
}

// ------------------------------------------------------------------------------------------------ summary
// the mean of the entries > -1 among value(0) .. value(n - 1), or -1 without any: every thread adds its strided share in
// ascending order, the threads' sums meet in the fixed tree; the result in every thread
template <class Value>
__device__ double defined_mean(int n, Value value, double* sh) {
    double sum = 0., cnt = 0.;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const double v = value(i);
        if (v > -1.) {
            sum = sum + v;
            cnt = cnt + 1.;
        }
    }
    sum = block_sum<kThreads>(sum, sh);
    cnt = block_sum<kThreads>(cnt, sh);
    return cnt > 0. ? sum / cnt : -1.;
}

// block k: per_class[k][0..12), each the defined_mean of its slice
__global__ __launch_bounds__(kThreads) void coco_class_summary_kernel(const double* __restrict__ precision,
                                                                      const double* __restrict__ recall, int class_num,
                                                                      double* __restrict__ per_class) {
    __shared__ double s_dbl[kThreads];
    const int k = blockIdx.x, tid = threadIdx.x;
    for (int j = 0; j < 12; ++j) {
        int t0, t1, a, m;
        stat_slice(j, &t0, &t1, &a, &m);
        const int per_t = j < 6 ? kRecThrs : 1;
        const double mean = defined_mean((t1 - t0) * per_t, [&](int i) {
            const int t = t0 + i / per_t, r = i % per_t;
            return j < 6 ? precision[precision_index(t, r, k, a, m, class_num)] : recall[recall_index(t, k, a, m, class_num)];
        }, s_dbl);
        if (tid == 0) per_class[12 * (size_t)k + j] = mean;
    }
}

// one block: stats[j] = the defined_mean of per_class[.][j] over the classes
__global__ __launch_bounds__(kThreads) void coco_stats_kernel(const double* __restrict__ per_class, int class_num,
                                                              double* __restrict__ stats) {
    __shared__ double s_dbl[kThreads];
    for (int j = 0; j < 12; ++j) {
        const double mean = defined_mean(class_num, [&](int k) { return per_class[12 * (size_t)k + j]; }, s_dbl);
        if (threadIdx.x == 0) stats[j] = mean;
    }
}

constexpr long long kIntMax = 0x7FFFFFFFLL;
constexpr long long kCurveEntries = (long long)kIouThrs * kRecThrs * kAreas * kMaxDetKinds;      // precision entries per class

// y3_coco_match's scratch: the "taken" word of every object (one for an empty set), for the images the LDS is too small for
struct MatchScratch {
    Carve at;
    int num_gt;
    size_t taken_words = num_gt > 0 ? num_gt : 1;
    u64* taken_big = at.take<u64>(taken_words);
};

// y3_coco_ap's scratch: the gather into class order (order2) of the two words, the label and the in-group rank of a rank
struct ApScratch {
    Carve at;
    int rows;
    u64* mw2 = at.take<u64>(rows);
    u64* iw2 = at.take<u64>(rows);
    int32_t* lab2 = at.take<int32_t>(rows);
    uint8_t* gr2 = at.take<uint8_t>(rows);
};

}  // namespace

extern "C" int y3_coco_ap_pass(void) { return kPass; }
extern "C" int y3_coco_lds_objects(void) { return kLdsObjs; }

extern "C" size_t y3_coco_match_scratch_bytes(int rows, int num_gt) {
    return rows > 0 && num_gt >= 0 ? MatchScratch{nullptr, num_gt}.at.bytes() : 0;
}

extern "C" int y3_coco_match(y3_ctx* ctx, const double* arena_box, const int32_t* arena_label, const int32_t* arena_image,
                             const int32_t* order, int rows, const int32_t* n_rows_dev, const int32_t* gt_start, const double* gt_box,
                             const int32_t* gt_label, const double* area_scale, int num_images, int num_gt, int class_num,
                             const double* iou_thrs_host, void* scratch, size_t scratch_bytes, uint64_t* matched, uint64_t* ignored,
                             uint8_t* group_rank, int32_t* npig) {
    Y3_CHECK_ARG(ctx && arena_box && arena_label && arena_image && order && gt_start && gt_box && gt_label && iou_thrs_host &&
                     scratch && matched && ignored && group_rank && npig,
                 "y3_coco_match: null argument");
    Y3_CHECK_ARG(rows > 0 && num_images > 0 && num_gt >= 0 && class_num > 0,
                 "y3_coco_match: bad dimension (rows=%d, num_images=%d, num_gt=%d, class_num=%d)", rows, num_images, num_gt, class_num);
    Y3_CHECK_ARG((long long)num_images * class_num <= kIntMax && (long long)class_num * kAreas <= kIntMax,
                 "y3_coco_match: num_images * class_num = %lld exceeds 2^31 - 1", (long long)num_images * class_num);
    Y3_CHECK_ARG(scratch_bytes >= y3_coco_match_scratch_bytes(rows, num_gt), "y3_coco_match: scratch too small (%zu < %zu)",
                 scratch_bytes, y3_coco_match_scratch_bytes(rows, num_gt));
    Y3_CHECK_ARG(aligned(arena_box, 8) && aligned(gt_box, 8) && aligned(scratch, 8) && aligned(matched, 8) && aligned(ignored, 8) &&
                     aligned(arena_label, 4) && aligned(arena_image, 4) && aligned(order, 4) && aligned(gt_start, 4) &&
                     aligned(gt_label, 4) && aligned(npig, 4) && (!n_rows_dev || aligned(n_rows_dev, 4)) &&
                     (!area_scale || aligned(area_scale, 8)),
                 "y3_coco_match: misaligned pointer");
    IouThrs thr;
    for (int t = 0; t < kIouThrs; ++t) thr.t[t] = iou_thrs_host[t];
    hipStream_t st = ctx->stream;
    const MatchScratch ws{scratch, num_gt};
    Y3_CHECK_HIP(hipMemsetAsync(ws.taken_big, 0, ws.taken_words * 8, st));
    Y3_CHECK_HIP(hipMemsetAsync(npig, 0, (size_t)class_num * kAreas * 4, st));
    const unsigned blocks = (unsigned)(((long long)rows + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(coco_match_kernel, dim3(blocks), dim3(kThreads), 0, st, arena_box, arena_label, arena_image, order, rows,
                       n_rows_dev, gt_start, gt_box, gt_label, area_scale, num_images, num_gt, class_num, thr, ws.taken_big,
                       reinterpret_cast<u64*>(matched), reinterpret_cast<u64*>(ignored), group_rank);
    Y3_CHECK_HIP(hipGetLastError());
    if (num_gt > 0) {
        hipLaunchKernelGGL(coco_npig_kernel, dim3((unsigned)(((long long)num_gt + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           gt_start, gt_box, gt_label, area_scale, num_images, num_gt, class_num, npig);
        Y3_CHECK_HIP(hipGetLastError());
    }
    return Y3_OK;
}

extern "C" size_t y3_coco_ap_scratch_bytes(int rows) {
    return rows > 0 ? ApScratch{nullptr, rows}.at.bytes() : 0;
}

extern "C" int y3_coco_ap(y3_ctx* ctx, const uint64_t* matched, const uint64_t* ignored, const uint8_t* group_rank,
                          const int32_t* arena_label, const int32_t* order, const int32_t* order2, int rows,
                          const int32_t* n_rows_dev, const int32_t* npig, int class_num, const double* rec_thrs_host, void* scratch,
                          size_t scratch_bytes, double* precision, double* recall) {
    Y3_CHECK_ARG(ctx && matched && ignored && group_rank && arena_label && order && order2 && npig && rec_thrs_host && scratch &&
                     precision && recall,
                 "y3_coco_ap: null argument");
    Y3_CHECK_ARG(rows > 0 && class_num > 0, "y3_coco_ap: bad dimension (rows=%d, class_num=%d)", rows, class_num);
    Y3_CHECK_ARG(kCurveEntries * class_num <= kIntMax, "y3_coco_ap: %lld precision entries exceed 2^31 - 1",
                 kCurveEntries * class_num);
    Y3_CHECK_ARG(scratch_bytes >= y3_coco_ap_scratch_bytes(rows), "y3_coco_ap: scratch too small (%zu < %zu)", scratch_bytes,
                 y3_coco_ap_scratch_bytes(rows));
    Y3_CHECK_ARG(aligned(matched, 8) && aligned(ignored, 8) && aligned(scratch, 8) && aligned(precision, 8) && aligned(recall, 8) &&
                     aligned(arena_label, 4) && aligned(order, 4) && aligned(order2, 4) && aligned(npig, 4) &&
                     (!n_rows_dev || aligned(n_rows_dev, 4)),
                 "y3_coco_ap: misaligned pointer");
    RecThrs thr;
    for (int r = 0; r < kRecThrs; ++r) thr.r[r] = rec_thrs_host[r];
    const ApScratch ws{scratch, rows};
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(coco_gather_kernel, dim3((unsigned)(((long long)rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       reinterpret_cast<const u64*>(matched), reinterpret_cast<const u64*>(ignored), group_rank, arena_label, order,
                       order2, rows, n_rows_dev, class_num, ws.mw2, ws.iw2, ws.lab2, ws.gr2);
    Y3_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(coco_ap_kernel, dim3(class_num, kAreas * kMaxDetKinds, kIouThrs), dim3(kThreads), 0, st, ws.mw2, ws.iw2,
                       ws.lab2, ws.gr2, rows, n_rows_dev, npig, class_num, thr, precision, recall);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}

extern "C" int y3_coco_summary(y3_ctx* ctx, const double* precision, const double* recall, int class_num, double* per_class,
                               double* stats) {
    Y3_CHECK_ARG(ctx && precision && recall && per_class && stats, "y3_coco_summary: null argument");
    Y3_CHECK_ARG(class_num > 0, "y3_coco_summary: bad dimension (class_num=%d)", class_num);
    Y3_CHECK_ARG(kCurveEntries * class_num <= kIntMax, "y3_coco_summary: %lld precision entries exceed 2^31 - 1",
                 kCurveEntries * class_num);
    Y3_CHECK_ARG(aligned(precision, 8) && aligned(recall, 8) && aligned(per_class, 8) && aligned(stats, 8),
                 "y3_coco_summary: misaligned pointer");
    hipLaunchKernelGGL(coco_class_summary_kernel, dim3(class_num), dim3(kThreads), 0, ctx->stream, precision, recall, class_num,
                       per_class);
    Y3_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(coco_stats_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, per_class, class_num, stats);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}
