// The record check, the per-pixel source / tap / blend and the per-box rule of the affine warp (y3_affine, include/yolo355.h -
// the comment there is the definition), written once for the GPU kernels (y3_affine.hip) and for the host build that
// tests/test_affine_cpu.py runs against utils.data_aug.affine_warp (tests/affine_emul.cpp).  Both builds compile it without
// FMA contraction: every float operation is one rounded float32 operation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define Y3A_HD __host__ __device__ __forceinline__
#else
#define Y3A_HD inline
#endif

namespace y3apx {

constexpr int kRecord = 12;             // int32 per image: ia, ib, ic, id, ie, if (Q16), then the bits of fa, fb, fc, fd, fe, ff
constexpr int kCoefMax = 1 << 20;       // |ia|, |ib|, |id|, |ie|
constexpr int kOffsetMax = 1 << 30;     // |ic|, |if|
constexpr int kMaxSide = 4096;          // H, W: with the two bounds above SX and SY stay below 2^34 in magnitude

// the validity rule; -1: the record is good, else the offending word.  Words 0-5 have to lie in [-*bound, *bound]; words
// 6-11 have to be the bits of a finite float (*bound = 0)
inline int record_fault(const int32_t* rec, int* bound) {
    for (int j = 0; j < 6; ++j) {
        *bound = (j == 2 || j == 5) ? kOffsetMax : kCoefMax;
        if (rec[j] < -*bound || rec[j] > *bound) return j;
    }
    *bound = 0;
    for (int j = 6; j < kRecord; ++j)
        if (((uint32_t)rec[j] & 0x7f800000u) == 0x7f800000u) return j;
    return -1;
}

inline const char* word_name(int j) {
    static const char* const kNames[kRecord] = {"ia", "ib", "ic", "id", "ie", "if", "fa", "fb", "fc", "fd", "fe", "ff"};
    return kNames[j];
}

Y3A_HD float word_float(const int32_t* rec, int j) {
    float f;
    memcpy(&f, rec + j, sizeof f);
    return f;
}

// where output pixel (x, y) reads: the tap (u0, v0) and the four weights, all exact
struct Source {
    long long u0, v0;
    float wx0, wx1, wy0, wy1;
};

Y3A_HD Source source_of(const int32_t* rec, int x, int y) {
    const long long sx = (long long)rec[0] * x + (long long)rec[1] * y + rec[2];
    const long long sy = (long long)rec[3] * x + (long long)rec[4] * y + rec[5];
    const int fx = (int)((sx >> 8) & 255), fy = (int)((sy >> 8) & 255);
    Source s;
    s.u0 = sx >> 16, s.v0 = sy >> 16;       // arithmetic shifts: floors
    s.wx1 = (float)fx / 256.f, s.wx0 = (float)(256 - fx) / 256.f;
    s.wy1 = (float)fy / 256.f, s.wy0 = (float)(256 - fy) / 256.f;
    return s;
}

// src(u, v, 0..2) of one image [H][W][3]: the pixel, or fill outside
Y3A_HD void tap(const float* image, long long u, long long v, int W, int H, float fill, float* p) {
    if (u >= 0 && u < W && v >= 0 && v < H) {
        const float* at = image + ((size_t)v * W + (size_t)u) * 3;
        p[0] = at[0], p[1] = at[1], p[2] = at[2];
    } else {
        p[0] = p[1] = p[2] = fill;
    }
}

// out[y][x][0..2] of one image
Y3A_HD void pixel(const float* image, const int32_t* rec, int x, int y, int W, int H, float fill, float* out) {
    const Source s = source_of(rec, x, y);
    float p00[3], p10[3], p01[3], p11[3];
    tap(image, s.u0, s.v0, W, H, fill, p00);
    tap(image, s.u0 + 1, s.v0, W, H, fill, p10);
    tap(image, s.u0, s.v0 + 1, W, H, fill, p01);
    tap(image, s.u0 + 1, s.v0 + 1, W, H, fill, p11);
    for (int c = 0; c < 3; ++c) {
        const float t0 = s.wx0 * p00[c], t1 = s.wx1 * p10[c], b0 = s.wx0 * p01[c], b1 = s.wx1 * p11[c];
        const float top = t0 + t1, bot = b0 + b1;
        const float a = s.wy0 * top, b = s.wy1 * bot;
        out[c] = a + b;
    }
}

// np.maximum / np.minimum: a NaN operand is the result
Y3A_HD float np_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
Y3A_HD float np_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// the box rule for box (x0, y0, x1, y1, m): true and out5 written when the box is kept
Y3A_HD bool box_rule(const float* in5, const int32_t* rec, int W, int H, float min_side, float min_area, float max_aspect,
                     float* out5) {
    const float fa = word_float(rec, 6), fb = word_float(rec, 7), fc = word_float(rec, 8);
    const float fd = word_float(rec, 9), fe = word_float(rec, 10), ff = word_float(rec, 11);
    const float x0 = in5[0], y0 = in5[1], x1 = in5[2], y1 = in5[3];
    const float cx[4] = {x0, x1, x0, x1}, cy[4] = {y0, y0, y1, y1};
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    for (int j = 0; j < 4; ++j) {
        const float ux = fa * cx[j], uy = fb * cy[j], vx = fd * cx[j], vy = fe * cy[j];
        const float us = ux + uy, vs = vx + vy;
        const float u = us + fc, v = vs + ff;
        a0 = j ? np_min(a0, u) : u, a1 = j ? np_max(a1, u) : u;
        b0 = j ? np_min(b0, v) : v, b1 = j ? np_max(b1, v) : v;
    }
    a0 = np_max(a0, 0.f), b0 = np_max(b0, 0.f), a1 = np_min(a1, (float)W), b1 = np_min(b1, (float)H);
    const float w = a1 - a0, h = b1 - b0;
    const float d0 = fa * fe, d1 = fb * fd;
    const float dd = d0 - d1;
    const float det = dd < 0.f ? -dd : dd;
    const float bw = x1 - x0, bh = y1 - y0;
    const float area0 = bw * bh;
    const float scaled = det * area0;
    const float need = min_area * scaled;
    const float area = w * h;
    const float wmax = max_aspect * h, hmax = max_aspect * w;
    if (!(w >= min_side && h >= min_side && area >= need && w <= wmax && h <= hmax)) return false;
    out5[0] = a0, out5[1] = b0, out5[2] = a1, out5[3] = b1, out5[4] = in5[4];
    return true;
}

}  // namespace y3apx
