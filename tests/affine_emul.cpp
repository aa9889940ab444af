// Test infrastructure: the record check, the per-pixel and the per-box functions of the affine warp
// (yolov3_tensorflow_amd/csrc/y3_affine_px.h) run on the HOST in the order y3_affine's kernels use them (every output pixel
// blends its four taps; every candidate box in ascending k), so that the addressing, the blend and the box rule can be
// compared with utils.data_aug.affine_warp without a GPU (tests/test_affine_cpu.py builds this file with g++).  Never part of
// the product: the package has no CPU form of y3_affine.
#include <stddef.h>
#include "../yolov3_tensorflow_amd/csrc/y3_affine_px.h"

// the arguments of y3_affine without the context and the scratch; returns 0, -1 for bad sizes, -(100 * (1 + i) + word) for a
// bad word of record i
extern "C" int y3af_emulate(const float* in_images, const float* in_boxes, const int32_t* in_labels, const int32_t* in_counts,
                            int n, int kmax, int H, int W, const int32_t* records, float fill, float min_side, float min_area,
                            float max_aspect, float* out_images, float* out_boxes, int32_t* out_labels, int32_t* out_counts) {
    if (n < 0 || kmax <= 0 || H < 1 || W < 1 || H > y3apx::kMaxSide || W > y3apx::kMaxSide) return -1;
    for (int i = 0; i < n; ++i) {
        int bound;
        const int word = y3apx::record_fault(records + (size_t)i * y3apx::kRecord, &bound);
        if (word >= 0) return -(100 * (1 + i) + word);
    }
    for (int i = 0; i < n; ++i) {
        const int32_t* rec = records + (size_t)i * y3apx::kRecord;
        const float* in_i = in_images + (size_t)i * H * W * 3;
        float* out_i = out_images + (size_t)i * H * W * 3;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) y3apx::pixel(in_i, rec, x, y, W, H, fill, out_i + ((size_t)y * W + x) * 3);
        const int count = in_counts[i] < 0 ? 0 : (in_counts[i] > kmax ? kmax : in_counts[i]);
        int kept = 0;
        for (int k = 0; k < count; ++k) {
            float row[5];
            if (!y3apx::box_rule(in_boxes + ((size_t)i * kmax + k) * 5, rec, W, H, min_side, min_area, max_aspect, row)) continue;
            for (int e = 0; e < 5; ++e) out_boxes[((size_t)i * kmax + kept) * 5 + e] = row[e];
            out_labels[(size_t)i * kmax + kept] = in_labels[(size_t)i * kmax + k];
            ++kept;
        }
        for (int j = kept; j < kmax; ++j) {
            for (int e = 0; e < 5; ++e) out_boxes[((size_t)i * kmax + j) * 5 + e] = 0.f;
            out_labels[(size_t)i * kmax + j] = 0;
        }
        out_counts[i] = kept;
    }
    return 0;
}
