// Test infrastructure: the per-cell and per-detection functions of the training-batch evaluator
// (yolov3_tensorflow_amd/csrc/y3_beval_px.h) run on the HOST in the order y3_batch_eval's kernels run them (gather every
// image, then every detection, then the tally), so that the arithmetic and the matching rule can be compared with
// eval_utils._evaluate without a GPU (tests/test_batch_eval_cpu.py builds this file with g++).  Never part of the product:
// the package has no CPU form of y3_batch_eval.
#include <vector>
#include "../yolov3_tensorflow_amd/csrc/y3_beval_px.h"

// the arguments of y3_batch_eval without the context and the scratch; table int64 [class_num][3] is added to
extern "C" int y3be_emulate(const float* out_boxes, const int32_t* out_labels, const int32_t* out_counts, int n, int cap,
                            const float* y_true_1, const float* y_true_2, const float* y_true_3, int h, int w, int class_num,
                            double iou_thresh, int gt_cap, long long* table, int32_t* state) {
    if (n <= 0 || cap <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32 || class_num <= 0 || gt_cap <= 0) return -1;
    const float* y[3] = {y_true_1, y_true_2, y_true_3};
    const int cells[3] = {3 * (h / 32) * (w / 32), 3 * (h / 16) * (w / 16), 3 * (h / 8) * (w / 8)};
    const int channels = 5 + class_num + 1;
    std::vector<double> gt_box((size_t)n * gt_cap * 4, -1e30);
    std::vector<int32_t> gt_label((size_t)n * gt_cap, -77), found((size_t)n * gt_cap, 0), gt_count(n, 0);
    for (int i = 0; i < n; ++i) {
        long long seen = 0;
        for (int s = 0; s < 3; ++s)
            for (int c = 0; c < cells[s]; ++c) {
                const float* cell = y[s] + ((size_t)i * cells[s] + c) * channels;
                const unsigned long long key = y3bpx::cell_key(cell + 5, class_num);
                if (!key) continue;
                if (seen < gt_cap) {
                    y3bpx::corner_box(cell, &gt_box[((size_t)i * gt_cap + seen) * 4]);
                    gt_label[(size_t)i * gt_cap + seen] = y3bpx::key_label(key);
                }
                ++seen;
            }
        gt_count[i] = (int32_t)(seen < gt_cap ? seen : gt_cap);
        state[0] += (int32_t)(seen - gt_count[i]);
    }
    for (int i = 0; i < n; ++i) {
        const int k_i = out_counts[i] < 0 ? 0 : (out_counts[i] > cap ? cap : out_counts[i]);
        for (int k = k_i - 1; k >= 0; --k) {      // (any order: a found word only ever becomes 1)
            const size_t src = (size_t)i * cap + k;
            const int label = out_labels[src];
            if (label >= 0 && label < class_num) table[3 * label + 2] += 1;
            const y3bpx::Best b = y3bpx::best_object(out_boxes + 4 * src, &gt_box[(size_t)i * gt_cap * 4], gt_count[i]);
            if (b.j >= 0 && y3bpx::is_hit(b, iou_thresh, gt_label[(size_t)i * gt_cap + b.j], label))
                found[(size_t)i * gt_cap + b.j] = 1;
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < gt_count[i]; ++j) {
            const int label = gt_label[(size_t)i * gt_cap + j];
            table[3 * label + 1] += 1;
            if (found[(size_t)i * gt_cap + j]) table[3 * label + 0] += 1;
        }
    return 0;
}
