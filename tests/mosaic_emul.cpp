// Test infrastructure: the per-pixel and per-box functions of the mosaic composition
// (yolov3_tensorflow_amd/csrc/y3_mosaic_px.h) run on the HOST in the order y3_mosaic's kernels use them (every output float
// finds its source element; every candidate box in the order q, k), so that the addressing and the box rule can be compared
// with utils.data_aug.mosaic4 without a GPU (tests/test_mosaic_cpu.py builds this file with g++).  Never part of the
// product: the package has no CPU form of y3_mosaic.
#include <stddef.h>
#include "../yolov3_tensorflow_amd/csrc/y3_mosaic_px.h"

// the arguments of y3_mosaic without the context and the scratch; returns 0, -1 for bad sizes, -(2 + i) for a bad record i
extern "C" int y3mo_emulate(const float* in_images, const float* in_boxes, const int32_t* in_labels, const int32_t* in_counts,
                            int n, int kmax, int H, int W, const int32_t* records, float min_side, float min_visible,
                            float* out_images, float* out_boxes, int32_t* out_labels, int32_t* out_counts) {
    if (n < 0 || kmax <= 0 || H < 2 || W < 2) return -1;
    for (int i = 0; i < n; ++i) {
        int what[3];
        if (y3mpx::record_fault(records + (size_t)i * y3mpx::kRecord, W, H, what)) return -(2 + i);
    }
    for (int i = 0; i < n; ++i) {
        const int32_t* rec = records + (size_t)i * y3mpx::kRecord;
        float* out_i = out_images + (size_t)i * H * W * 3;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c)
                    out_i[((size_t)y * W + x) * 3 + c] = in_images[y3mpx::source_index(rec, i, x, y, c, W, H)];
        const int kout = 4 * kmax;
        int kept = 0;
        for (int j = 0; j < kout; ++j) {
            const int q = j / kmax, k = j - q * kmax;
            const size_t s = 4 * (size_t)i + q;
            const int count = in_counts[s] < 0 ? 0 : (in_counts[s] > kmax ? kmax : in_counts[s]);
            if (k >= count) continue;
            float row[5];
            if (!y3mpx::box_rule(in_boxes + (s * kmax + k) * 5, y3mpx::tile_of(rec, q, W, H), min_side, min_visible, row)) continue;
            for (int e = 0; e < 5; ++e) out_boxes[((size_t)i * kout + kept) * 5 + e] = row[e];
            out_labels[(size_t)i * kout + kept] = in_labels[s * kmax + k];
            ++kept;
        }
        for (int j = kept; j < kout; ++j) {
            for (int e = 0; e < 5; ++e) out_boxes[((size_t)i * kout + j) * 5 + e] = 0.f;
            out_labels[(size_t)i * kout + j] = 0;
        }
        out_counts[i] = kept;
    }
    return 0;
}
