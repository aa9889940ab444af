// The per-pixel source address and the per-box rule of the mosaic composition (y3_mosaic, include/yolo355.h - the comment
// there is the definition), written once for the GPU kernels (y3_mosaic.hip) and for the host build that
// tests/test_mosaic_cpu.py runs against utils.data_aug.mosaic4 (tests/mosaic_emul.cpp).  Both builds compile it without FMA
// contraction: every box operation is one rounded float32 operation.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define Y3M_HD __host__ __device__ __forceinline__
#else
#define Y3M_HD inline
#endif

namespace y3mpx {

constexpr int kRecord = 10;         // int32 per output image: cx, cy, ox0, oy0, ox1, oy1, ox2, oy2, ox3, oy3

// tile q of one output image: its origin and size in the output, and where its window begins in sample 4i+q
struct Tile {
    int tx, ty, tw, th, ox, oy;
};

Y3M_HD Tile tile_of(const int32_t* rec, int q, int W, int H) {
    const int cx = rec[0], cy = rec[1];
    Tile t;
    t.tx = (q & 1) ? cx : 0;
    t.ty = (q & 2) ? cy : 0;
    t.tw = (q & 1) ? W - cx : cx;
    t.th = (q & 2) ? H - cy : cy;
    t.ox = rec[2 + 2 * q];
    t.oy = rec[3 + 2 * q];
    return t;
}

// the validity rule; nullptr: the record is good.  what[0 .. 2]: the offending value and the range it has to lie in
inline const char* record_fault(const int32_t* rec, int W, int H, int* what) {
    static const char* const kOx[4] = {"ox0", "ox1", "ox2", "ox3"};
    static const char* const kOy[4] = {"oy0", "oy1", "oy2", "oy3"};
    if (rec[0] < 1 || rec[0] > W - 1) return what[0] = rec[0], what[1] = 1, what[2] = W - 1, "cx";
    if (rec[1] < 1 || rec[1] > H - 1) return what[0] = rec[1], what[1] = 1, what[2] = H - 1, "cy";
    for (int q = 0; q < 4; ++q) {
        const Tile t = tile_of(rec, q, W, H);
        if (t.ox < 0 || t.ox > W - t.tw) return what[0] = t.ox, what[1] = 0, what[2] = W - t.tw, kOx[q];
        if (t.oy < 0 || t.oy > H - t.th) return what[0] = t.oy, what[1] = 0, what[2] = H - t.th, kOy[q];
    }
    return nullptr;
}

// the tile that output pixel (x, y) lies in
Y3M_HD int tile_at(const int32_t* rec, int x, int y) { return (x >= rec[0] ? 1 : 0) + (y >= rec[1] ? 2 : 0); }

// out[i][y][x][c] = in[source_index(...)], an element index into in_images [4n][H][W][3]
Y3M_HD size_t source_index(const int32_t* rec, int i, int x, int y, int c, int W, int H) {
    const int q = tile_at(rec, x, y);
    const Tile t = tile_of(rec, q, W, H);
    const size_t row = ((size_t)(4 * (size_t)i + q) * H + (size_t)(y - t.ty + t.oy)) * W;
    return (row + (size_t)(x - t.tx + t.ox)) * 3 + c;
}

// np.maximum / np.minimum: a NaN operand is the result
Y3M_HD float np_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
Y3M_HD float np_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// the box rule for box (x0, y0, x1, y1, m) of the sample behind tile t: true and out5 written when the box is kept
Y3M_HD bool box_rule(const float* in5, const Tile& t, float min_side, float min_visible, float* out5) {
    const float x0 = in5[0], y0 = in5[1], x1 = in5[2], y1 = in5[3];
    const float wx0 = (float)t.ox, wy0 = (float)t.oy, wx1 = (float)(t.ox + t.tw), wy1 = (float)(t.oy + t.th);
    const float a0 = np_max(x0, wx0), b0 = np_max(y0, wy0), a1 = np_min(x1, wx1), b1 = np_min(y1, wy1);
    const float w = a1 - a0, h = b1 - b0;
    const float bw = x1 - x0, bh = y1 - y0;
    const float visible = w * h;
    const float area = bw * bh;
    const float need = min_visible * area;
    if (!(w >= min_side && h >= min_side && visible >= need)) return false;
    const float tx = (float)t.tx, ty = (float)t.ty;
    const float r0 = a0 - wx0, r1 = b0 - wy0, r2 = a1 - wx0, r3 = b1 - wy0;
    out5[0] = r0 + tx;
    out5[1] = r1 + ty;
    out5[2] = r2 + tx;
    out5[3] = r3 + ty;
    out5[4] = in5[4];
    return true;
}

}  // namespace y3mpx
