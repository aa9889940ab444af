// The per-element rules of the spatial pyramid pooling block (y3_spp_fwd / y3_spp_bwd, include/yolo355.h - the comment under
// "SPP" there is the definition).  Shared by the GPU kernels (y3_spp.hip) and the host build that tests/test_spp_cpu.py runs
// against torch (tests/spp_emul.cpp): the slot order (window_k, window_slot), the window bounds (win_lo, win_hi), the
// forward's comparison (max_of) and one step of backward's first-max scan (first_max_step).  The drivers below them - max5,
// row_first_max, col_first_max, gather_window - state a whole pass for ONE channel in the kernels' order and are what the
// host build runs; the kernels walk the same windows in the same order over 16-byte vectors of channels held in the LDS and
// call the shared steps per channel, so their loops are written out in y3_spp.hip (tests/test_spp_gpu.py holds the kernels
// themselves to the same references, bit for bit).  Nothing here multiplies: every float operation is a comparison or one
// rounded float32 addition.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define Y3S_HD __host__ __device__ __forceinline__
#else
#define Y3S_HD inline
#endif

namespace y3spp {

constexpr int kWindows = 3;                   // the pooled slots; slot 3 is x itself
constexpr int kFwdHalo = 6, kBwdHalo = 12;    // 13 / 2; a window of windows
// the windows in backward's summation order (5, 9, 13) and the output slot of each: spp(x) = [mp_13, mp_9, mp_5, x]
Y3S_HD int window_k(int j) { return 5 + 4 * j; }
Y3S_HD int window_slot(int j) { return 2 - j; }

// the window of centre p along an axis of n positions: [lo, hi], the padding left out
Y3S_HD int win_lo(int p, int k) { return p - k / 2 > 0 ? p - k / 2 : 0; }
Y3S_HD int win_hi(int p, int k, int n) { return p + k / 2 < n - 1 ? p + k / 2 : n - 1; }

// forward: the running maximum (exact; which of two equal values stays is not observable for finite inputs other than +-0)
Y3S_HD float max_of(float m, float v) { return v > m ? v : m; }

// mp_5 along one axis at p: `at(i)` is the value at position i of that axis.  mp_5 over rows of mp_5 over columns is mp_5 of
// the map; mp_9 = mp_5(mp_5), mp_13 = mp_5(mp_9).
template <class At>
Y3S_HD float max5(At&& at, int p, int n) {
    float m = at(win_lo(p, 5));
    for (int i = win_lo(p, 5) + 1; i <= win_hi(p, 5, n); ++i) m = max_of(m, at(i));
    return m;
}

// backward: one step of a first-max scan (ascending positions): a later value takes over only if it is greater
Y3S_HD void first_max_step(float v, int at, float* m, int* arg) {
    if (v > *m) { *m = v; *arg = at; }
}

// the first maximum of row window [win_lo(x), win_hi(x)]: its value and its column
template <class At>
Y3S_HD void row_first_max(At&& at, int x, int k, int w, float* m, int* ax) {
    const int lo = win_lo(x, k), hi = win_hi(x, k, w);
    *m = at(lo);
    *ax = lo;
    for (int i = lo + 1; i <= hi; ++i) first_max_step(at(i), i, m, ax);
}

// the first maximum of the k x k window in row-major order, from the rows' first maxima at this column: the first row whose
// maximum is the window's, and that row's first column.  row_max(y) / row_arg(y): row_first_max of row y at this column.
template <class RowMax, class RowArg>
Y3S_HD void col_first_max(RowMax&& row_max, RowArg&& row_arg, int y, int k, int h, int* ay, int* ax) {
    const int lo = win_lo(y, k), hi = win_hi(y, k, h);
    float m = row_max(lo);
    int a = lo;
    for (int i = lo + 1; i <= hi; ++i) first_max_step(row_max(i), i, &m, &a);
    *ay = a;
    *ax = row_arg(a);
}

// backward's sum for one window size: acc, then + g(q) for every q, row-major, whose window's first maximum is p = (py, px).
// hit(qy, qx): argmax_k(q) == p; g(qy, qx): the gradient of slot k at q.  A q that does not hit adds nothing (not + 0).
template <class Hit, class G>
Y3S_HD float gather_window(float acc, Hit&& hit, G&& g, int py, int px, int k, int h, int w) {
    for (int qy = win_lo(py, k); qy <= win_hi(py, k, h); ++qy)
        for (int qx = win_lo(px, k); qx <= win_hi(px, k, w); ++qx)
            if (hit(qy, qx)) acc = acc + g(qy, qx);
    return acc;
}

// bf16 <-> the float of the same value (exact both ways for a value that came from bf16)
Y3S_HD float bf16_float(uint16_t b) {
    union { uint32_t u; float f; } c;
    c.u = (uint32_t)b << 16;
    return c.f;
}
Y3S_HD uint16_t float_bf16_exact(float f) {
    union { uint32_t u; float f; } c;
    c.f = f;
    return (uint16_t)(c.u >> 16);
}

}  // namespace y3spp
