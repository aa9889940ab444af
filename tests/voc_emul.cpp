// Test infrastructure: the per-detection and per-rank functions of the device VOC evaluator
// (yolov3_tensorflow_amd/csrc/y3_voc_px.h) run on the HOST in the order y3_voc_match's and y3_voc_ap's kernels run them
// (every claim before any tp; the counts forwards, the envelope and the area sum backwards), so that the arithmetic and
// the claim rule can be compared with eval_utils.voc_eval without a GPU (tests/test_voc_device_cpu.py builds this file
// with g++).  Never part of the product: the package has no CPU form of y3_voc_match / y3_voc_ap.
#include <algorithm>
#include <numeric>
#include <vector>
#include "../yolov3_tensorflow_amd/csrc/y3_voc_px.h"

// arena rows (box [rows][4], score, label, image) + the ground-truth CSR -> out [class_num][5], order [rows], tp [rows]
extern "C" int y3v_emulate(const double* box, const double* score, const int32_t* label, const int32_t* image, int rows,
                           const int32_t* gt_start, const double* gt_box, const int32_t* gt_label, int num_images, int num_gt,
                           int class_num, double iou_thres, int use_07_metric, const double* thresholds11, double* out,
                           int32_t* order, uint8_t* tp) {
    // the device order: label ascending, score descending, row ascending (two stable sorts, like DeviceEval.finish)
    std::iota(order, order + rows, 0);
    std::stable_sort(order, order + rows, [&](int a, int b) { return -score[a] < -score[b]; });
    std::stable_sort(order, order + rows, [&](int a, int b) { return label[a] < label[b]; });
    std::vector<int> jstar(rows);
    std::vector<unsigned> claim(num_gt > 0 ? num_gt : 1, y3vpx::kUnclaimed);
    for (int r = rows - 1; r >= 0; --r) {      // (any order: the claim is a minimum)
        const int row = order[r], im = image[row];
        if (im < 0 || im >= num_images) return -1;
        jstar[r] = y3vpx::best_object(box + 4 * (size_t)row, label[row], gt_box, gt_label, gt_start[im], gt_start[im + 1], iou_thres);
        if (jstar[r] >= 0) claim[jstar[r]] = std::min(claim[jstar[r]], (unsigned)r);
    }
    for (int r = 0; r < rows; ++r) tp[r] = jstar[r] >= 0 && claim[jstar[r]] == (unsigned)r;
    for (int c = 0; c < class_num; ++c) {
        int s = 0, e = 0, npos = 0;
        for (int r = 0; r < rows; ++r) {
            s += label[order[r]] < c;
            e += label[order[r]] <= c;
        }
        for (int g = 0; g < num_gt; ++g) npos += gt_label[g] == c;
        double* o = out + 5 * c;
        const int nd = e - s;
        if (nd == 0) {
            o[0] = o[1] = 1e-6;
            o[2] = o[3] = o[4] = 0.;
            continue;
        }
        std::vector<int> ctp(nd);
        double best[11] = {0.};
        int run = 0;
        for (int i = 0; i < nd; ++i) {
            run += tp[s + i];
            ctp[i] = run;
            if (use_07_metric) {
                const double rec = y3vpx::recall_at(run, npos), prec = y3vpx::precision_at(run, i);
                for (int t = 0; t < 11; ++t)
                    if (rec >= thresholds11[t]) best[t] = y3vpx::dmax(best[t], prec);
            }
        }
        double ap;
        if (use_07_metric) {
            ap = y3vpx::eleven_point(best);
        } else {
            bool take;
            double env = 0.;
            ap = 0.;
            for (int i = nd - 1; i >= 0; --i) {
                env = y3vpx::dmax(env, y3vpx::precision_at(ctp[i], i));
                const double before = i > 0 ? y3vpx::recall_at(ctp[i - 1], npos) : 0.;
                const double term = y3vpx::area_term(before, y3vpx::recall_at(ctp[i], npos), env, &take);
                if (take) ap = ap + term;
            }
            const double term = y3vpx::area_term(y3vpx::recall_at(run, npos), 1., 0., &take);
            if (take) ap = ap + term;
        }
        o[0] = (double)npos;
        o[1] = (double)nd;
        o[2] = (double)run / (double)npos;
        o[3] = (double)run / (double)nd;
        o[4] = ap;
    }
    return 0;
}
