// The per-detection and per-rank arithmetic of the device VOC evaluator (y3_voc_match / y3_voc_ap, include/yolo355.h),
// written once for the GPU kernels (y3_voc.hip) and for the host build tests/test_voc_device_cpu.py runs against
// eval_utils.voc_eval (tests/voc_emul.cpp).  float64 throughout, in voc_eval's operation order
// (yolov3_tensorflow_amd/utils/eval_utils.py:201-244); both builds compile it without FMA contraction.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define Y3V_HD __host__ __device__ __forceinline__
#else
#define Y3V_HD inline
#endif

namespace y3vpx {

constexpr double kEps = 2.220446049250313e-16;      // np.finfo(np.float64).eps
constexpr unsigned kUnclaimed = 0xFFFFFFFFu;        // a claim word nobody has written (larger than every rank)

Y3V_HD double dmax(double a, double b) { return a > b ? a : b; }
Y3V_HD double dmin(double a, double b) { return a < b ? a : b; }

// eval_utils.py:228-233: the pixel-inclusive (+1) intersection over union of detection bb and object g
Y3V_HD double overlap(const double* bb, const double* g) {
    const double iw = dmax(dmin(g[2], bb[2]) - dmax(g[0], bb[0]) + 1., 0.);
    const double ih = dmax(dmin(g[3], bb[3]) - dmax(g[1], bb[1]) + 1., 0.);
    const double inters = iw * ih;
    const double uni = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (g[2] - g[0] + 1.) * (g[3] - g[1] + 1.)) - inters;
    return inters / uni;
}

// eval_utils.py:224-235 for one detection: np.argmax of the overlaps with the image's objects [g0, g1) of class `label`,
// in the image's ground-truth order - the first maximum, a NaN counting as one, like numpy's.  Returns the object's index
// into gt_box when overlaps[j] > iou_thres, else -1 (no object of the class, or a best overlap at or under the threshold).
Y3V_HD int best_object(const double* bb, int label, const double* gt_box, const int32_t* gt_label, int g0, int g1,
                       double iou_thres) {
    int best_j = -1;
    double best = 0.;
    for (int g = g0; g < g1; ++g) {
        if (gt_label[g] != label) continue;
        const double ov = overlap(bb, gt_box + 4 * (long long)g);
        if (best_j < 0 || ov > best || (ov != ov && best == best)) {
            best = ov;
            best_j = g;
        }
    }
    return (best_j >= 0 && best > iou_thres) ? best_j : -1;
}

// eval_utils.py:238-242 at 0-based rank i of a class: ctp = true positives among ranks 0..i (tp + fp = i + 1, exactly)
Y3V_HD double recall_at(int ctp, int npos) { return (double)ctp / (double)npos; }
Y3V_HD double precision_at(int ctp, int i) { return (double)ctp / dmax((double)i + 1., kEps); }

// voc_ap's area term (eval_utils.py:194-198) at position i of the padded arrays, 0 <= i <= nd: rec_before = mrec[i]
// (0. at i = 0), rec_here = mrec[i + 1] (1. at i = nd), env = the precision envelope at i + 1 (0. at i = nd).
// `take` says whether voc_ap's `step` holds i.
Y3V_HD double area_term(double rec_before, double rec_here, double env, bool* take) {
    *take = rec_here != rec_before;
    return (rec_here - rec_before) * env;
}

// voc_ap's 11-point sum (eval_utils.py:189-193): best[k] = the largest precision among ranks with recall >= thresholds[k], 0.
// where there is none
Y3V_HD double eleven_point(const double* best) {
    double ap = 0.;
    for (int k = 0; k < 11; ++k) ap = ap + best[k] / 11.;
    return ap;
}

}  // namespace y3vpx
