// The per-cell and per-detection arithmetic of the training-batch evaluator (y3_batch_eval, include/yolo355.h), written
// once for the GPU kernels (y3_beval.hip) and for the host build tests/test_batch_eval_cpu.py runs against
// eval_utils._evaluate (tests/beval_emul.cpp).  It restates yolov3_tensorflow_amd/utils/eval_utils.py:35-50 (calc_iou),
// :53-68 (_ground_truth_of_image) and :90-92 (the matching rule); both builds compile it without FMA contraction.
//
// Precondition on y_true: the entries of a cell's class slice are finite and >= 0 (what process_box and the feeder write,
// mix-up weights and label smoothing included).  _ground_truth_of_image tests `probs.sum(-1) > 0`; for such entries that is
// the test used here, "some entry > 0", and the first maximum of the slice is the first maximum of its positive entries.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define Y3B_HD __host__ __device__ __forceinline__
#else
#define Y3B_HD inline
#endif

namespace y3bpx {

// np.minimum / np.maximum: a NaN operand is the result
Y3B_HD double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
Y3B_HD double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// ---- gather: eval_utils.py:59-61.  A positive class entry v at class c becomes a 64-bit key whose maximum over the cell
// is np.argmax's choice: the larger v first (the bits of a positive float order like the float), the smaller c second.
// 0 is no key: a cell whose maximum stays 0 holds no object.
Y3B_HD unsigned long long class_key(float v, int c) {
    uint32_t bits;
    memcpy(&bits, &v, 4);
    return ((unsigned long long)bits << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)c);
}
Y3B_HD int key_label(unsigned long long key) { return (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)); }

// the key of one cell's class slice cls[0 .. class_num-1]; 0: no object
Y3B_HD unsigned long long cell_key(const float* cls, int class_num) {
    unsigned long long best = 0;
    for (int c = 0; c < class_num; ++c)
        if (cls[c] > 0.f) {
            const unsigned long long k = class_key(cls[c], c);
            if (k > best) best = k;
        }
    return best;
}

// eval_utils.py:64-67: the corner box, in float64 widened from the cell's fp32 (x, y, w, h)
Y3B_HD void corner_box(const float* cell, double* out) {
    const double x = (double)cell[0], y = (double)cell[1], w = (double)cell[2], h = (double)cell[3];
    out[0] = x - w / 2.;
    out[1] = y - h / 2.;
    out[2] = out[0] + w;
    out[3] = out[1] + h;
}

// ---- match: calc_iou (eval_utils.py:42-50) of a float32 detection p against a float64 object t.  numpy promotes the
// mixed min / max to float64 but keeps `p[..., 2:] - p[..., :2]` and the detection's area in float32.
Y3B_HD double iou(const float* p, const double* t) {
    const double w = np_max(np_min((double)p[2], t[2]) - np_max((double)p[0], t[0]), 0.);
    const double h = np_max(np_min((double)p[3], t[3]) - np_max((double)p[1], t[1]), 0.);
    const double inter = w * h;
    const float pw = p[2] - p[0], ph = p[3] - p[1];
    const float p_area = pw * ph;
    const double tw = t[2] - t[0], th = t[3] - t[1];
    const double t_area = tw * th;
    return inter / ((((double)p_area + t_area) - inter) + 1e-10);
}

// np.argmax over the image's objects in gather order, one object at a time: the first maximum, a NaN counting as one
struct Best {
    int j;
    double iou;
};
Y3B_HD Best no_best() { return Best{-1, 0.}; }
Y3B_HD void consider(Best* b, int j, double ov) {
    if (b->j < 0 || ov > b->iou || (ov != ov && b->iou == b->iou)) {
        b->iou = ov;
        b->j = j;
    }
}
Y3B_HD Best best_object(const float* p, const double* gt_box, int count) {
    Best b = no_best();
    for (int j = 0; j < count; ++j) consider(&b, j, iou(p, gt_box + 4 * (long long)j));
    return b;
}

// eval_utils.py:92: the label is checked after the argmax over all objects
Y3B_HD bool is_hit(const Best& b, double iou_thresh, int object_label, int detection_label) {
    return b.j >= 0 && b.iou > iou_thresh && object_label == detection_label;
}

}  // namespace y3bpx
