// The SPP kernels' rules (yolov3_tensorflow_amd/csrc/y3_spp_px.h) run on the host in the kernels' order, for
// tests/test_spp_cpu.py: forward as three rounds of mp_5 (rows, then columns), backward as the first maximum of every window
// (rows, then columns) and the ordered gather per input element.  One map = one tile here; the kernels' tiling only restricts
// which positions a workgroup holds.
#include <vector>
#include "../yolov3_tensorflow_amd/csrc/y3_spp_px.h"

using namespace y3spp;

static float load(const void* x, int bf16, size_t i) {
    return bf16 ? bf16_float(static_cast<const uint16_t*>(x)[i]) : static_cast<const float*>(x)[i];
}
static void store(void* y, int bf16, size_t i, float v) {
    if (bf16) static_cast<uint16_t*>(y)[i] = float_bf16_exact(v);
    else static_cast<float*>(y)[i] = v;
}

extern "C" int y3spp_emul_fwd(const void* x, int bf16, int n, int h, int w, int c, void* out) {
    std::vector<float> A((size_t)h * w), B((size_t)h * w);
    for (int img = 0; img < n; ++img)
        for (int ch = 0; ch < c; ++ch) {
            auto pos = [&](int y, int xx) { return ((size_t)img * h + y) * w + xx; };
            for (int y = 0; y < h; ++y)
                for (int xx = 0; xx < w; ++xx) {
                    A[(size_t)y * w + xx] = load(x, bf16, pos(y, xx) * c + ch);
                    store(out, bf16, pos(y, xx) * 4 * c + 3 * (size_t)c + ch, A[(size_t)y * w + xx]);
                }
            for (int round = 0; round < kWindows; ++round) {
                for (int y = 0; y < h; ++y)
                    for (int xx = 0; xx < w; ++xx)
                        B[(size_t)y * w + xx] = max5([&](int i) { return A[(size_t)y * w + i]; }, xx, w);
                for (int y = 0; y < h; ++y)
                    for (int xx = 0; xx < w; ++xx) {
                        A[(size_t)y * w + xx] = max5([&](int i) { return B[(size_t)i * w + xx]; }, y, h);
                        store(out, bf16, pos(y, xx) * 4 * c + (size_t)window_slot(round) * c + ch, A[(size_t)y * w + xx]);
                    }
            }
        }
    return 0;
}

extern "C" int y3spp_emul_bwd(const void* x, long long x_stride, int bf16, const float* g, int n, int h, int w, int c,
                              int accumulate, float* dx) {
    const size_t hw = (size_t)h * w;
    std::vector<float> X(hw), RM(hw), ACC(hw);
    std::vector<int> RA(hw), AY(hw), AX(hw);
    for (int img = 0; img < n; ++img)
        for (int ch = 0; ch < c; ++ch) {
            auto pos = [&](int y, int xx) { return ((size_t)img * h + y) * w + xx; };
            for (int y = 0; y < h; ++y)
                for (int xx = 0; xx < w; ++xx) {
                    X[(size_t)y * w + xx] = load(x, bf16, pos(y, xx) * (size_t)x_stride + ch);
                    ACC[(size_t)y * w + xx] = g[pos(y, xx) * 4 * c + 3 * (size_t)c + ch];
                }
            for (int j = 0; j < kWindows; ++j) {
                const int k = window_k(j);
                for (int y = 0; y < h; ++y)
                    for (int xx = 0; xx < w; ++xx)
                        row_first_max([&](int i) { return X[(size_t)y * w + i]; }, xx, k, w, &RM[(size_t)y * w + xx], &RA[(size_t)y * w + xx]);
                for (int y = 0; y < h; ++y)
                    for (int xx = 0; xx < w; ++xx)
                        col_first_max([&](int i) { return RM[(size_t)i * w + xx]; }, [&](int i) { return RA[(size_t)i * w + xx]; }, y, k, h,
                                      &AY[(size_t)y * w + xx], &AX[(size_t)y * w + xx]);
                for (int y = 0; y < h; ++y)
                    for (int xx = 0; xx < w; ++xx)
                        ACC[(size_t)y * w + xx] = gather_window(
                            ACC[(size_t)y * w + xx],
                            [&](int qy, int qx) { return AY[(size_t)qy * w + qx] == y && AX[(size_t)qy * w + qx] == xx; },
                            [&](int qy, int qx) { return g[pos(qy, qx) * 4 * c + (size_t)window_slot(j) * c + ch]; }, y, xx, k, h, w);
            }
            for (int y = 0; y < h; ++y)
                for (int xx = 0; xx < w; ++xx) {
                    float* at = dx + pos(y, xx) * c + ch;
                    *at = accumulate ? *at + ACC[(size_t)y * w + xx] : ACC[(size_t)y * w + xx];
                }
        }
    return 0;
}
