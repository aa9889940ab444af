// The per-element arithmetic of the device COCO evaluator (y3_coco_match / y3_coco_ap / y3_coco_summary, include/yolo355.h),
// written once for the GPU kernels (y3_coco.hip) and for the host build tests/test_coco_device_cpu.py runs against
// eval_utils.coco_eval (tests/coco_emul.cpp).  float64 throughout, in coco_eval's operation order; both builds compile it
// without FMA contraction.  The rule itself is stated in include/yolo355.h.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define Y3C_HD __host__ __device__ __forceinline__
#else
#define Y3C_HD inline
#endif

namespace y3cpx {

constexpr double kEps = 2.220446049250313e-16;      // np.spacing(1)
constexpr int kIouThrs = 10;                        // T: np.linspace(.5, .95, 10), passed in by the host
constexpr int kRecThrs = 101;                       // R: np.linspace(0., 1., 101), passed in by the host
constexpr int kAreas = 4;                           // A: all, small, medium, large
constexpr int kMaxDetKinds = 3;                     // M: 1, 10, 100
constexpr int kMaxDets = 100;                       // detections of one (image, class) group that are matched at all
constexpr int kLanes = kIouThrs * kAreas;           // (threshold, area range) pairs; pair t * 4 + a is bit t * 4 + a of a word
constexpr int kRankSaturated = 255;                 // the in-group rank is stored in a byte

Y3C_HD double dmax(double a, double b) { return a > b ? a : b; }
Y3C_HD double dmin(double a, double b) { return a < b ? a : b; }
Y3C_HD int max_dets_of(int m) { return m == 0 ? 1 : (m == 1 ? 10 : 100); }

// intersection over union of detection d and object g (x0, y0, x1, y1), no +1; 0. when they do not overlap
Y3C_HD double iou(const double* d, const double* g) {
    const double w = dmin(d[2], g[2]) - dmax(d[0], g[0]);
    const double h = dmin(d[3], g[3]) - dmax(d[1], g[1]);
    if (w <= 0. || h <= 0.) return 0.;
    const double i = w * h;
    return i / ((d[2] - d[0]) * (d[3] - d[1]) + (g[2] - g[0]) * (g[3] - g[1]) - i);
}

Y3C_HD double area(const double* b, double scale) { return (b[2] - b[0]) * (b[3] - b[1]) * scale; }

// bit a set: the area is OUTSIDE range a (area < lo or area > hi); 32^2 is inside small and medium, 96^2 inside medium and large
Y3C_HD unsigned outside_mask(double ar) {
    const double lo[kAreas] = {0., 0., 1024., 9216.};
    const double hi[kAreas] = {1e10, 1024., 9216., 1e10};
    unsigned m = 0;
    for (int a = 0; a < kAreas; ++a)
        if (ar < lo[a] || ar > hi[a]) m |= 1u << a;
    return m;
}

// One detection's greedy choice at one (threshold, area range).  The rule walks the free objects that are not ignored and,
// only if that finds nothing, the free ignored ones, both from best = min(t, 1 - 1e-10); the two walks do not influence each
// other, so one pass in ground-truth order keeps both candidates.  An object is taken when iou >= best (ties: the later one).
struct Greedy {
    double best_in, best_ig;
    int m_in, m_ig;
};
Y3C_HD double greedy_floor(double iou_thr) { return dmin(iou_thr, 1. - 1e-10); }
Y3C_HD void greedy_begin(Greedy* s, double floor) {
    s->best_in = s->best_ig = floor;
    s->m_in = s->m_ig = -1;
}
Y3C_HD void greedy_step(Greedy* s, double ov, bool object_ignored, int g) {
    if (object_ignored) {
        if (ov < s->best_ig) return;
        s->best_ig = ov;
        s->m_ig = g;
    } else {
        if (ov < s->best_in) return;
        s->best_in = ov;
        s->m_in = g;
    }
}
// the matched object (-1: none); *ignored = the detection is ignored (its object is, or, unmatched, its own area is outside)
Y3C_HD int greedy_end(const Greedy* s, bool detection_outside, bool* ignored) {
    if (s->m_in >= 0) {
        *ignored = false;
        return s->m_in;
    }
    *ignored = s->m_ig >= 0 ? true : detection_outside;
    return s->m_ig;
}

// cumulative counts at a position of a (class, area range, max-dets, threshold) list -> recall and precision there
Y3C_HD double recall_at(int tp, int npig) { return (double)tp / (double)npig; }
Y3C_HD double precision_at(int tp, int fp) { return (double)tp / (((double)fp + (double)tp) + kEps); }

// how many of the ascending thresholds thr[0..n) are <= rc: thresholds [count(rc before), count(rc here)) have their first
// position with recall >= threshold here (np.searchsorted(rc, thr, side='left'))
Y3C_HD int thresholds_reached(double rc, const double* thr, int n) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] <= rc)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// flat indices of precision [T][R][K][A][M] and recall [T][K][A][M]
Y3C_HD long long precision_index(int t, int r, int k, int a, int m, int class_num) {
    return ((((long long)t * kRecThrs + r) * class_num + k) * kAreas + a) * kMaxDetKinds + m;
}
Y3C_HD long long recall_index(int t, int k, int a, int m, int class_num) {
    return (((long long)t * class_num + k) * kAreas + a) * kMaxDetKinds + m;
}

// The twelve numbers: which entries of class k go into number j.  j 0..5 average precision[t][r][k][a][M=100] over r and the
// thresholds t0 <= t < t1; j 6..11 average recall[t][k][a][m] over all t.
Y3C_HD void stat_slice(int j, int* t0, int* t1, int* a, int* m) {
    *t0 = 0;
    *t1 = kIouThrs;
    *a = 0;
    *m = 2;
    if (j == 1) { *t0 = 0; *t1 = 1; }
    if (j == 2) { *t0 = 5; *t1 = 6; }
    if (j >= 3 && j <= 5) *a = j - 2;
    if (j >= 6 && j <= 8) *m = j - 6;
    if (j >= 9) *a = j - 8;
}

}  // namespace y3cpx
