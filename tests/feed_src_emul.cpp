// Test infrastructure: the device functions of the feeder's pixel work (yolov3_tensorflow_amd/csrc/y3_feed_px.h) run on
// the HOST in the order y3_feed_run_src's three kernels run them over a by-reference plan (y3f_plan_batch_src): sources the
// records place in the arena are read there, with window_pixel's arena form.  tests/test_feed_src_cpu.py builds this file
// with g++ and compares with y3f_sample without a GPU.  Never part of the product.
#include <cstring>
#include "../yolov3_tensorflow_amd/csrc/y3_feed_px.h"

extern "C" int y3f_emulate_src(const uint8_t* blob, int n, const y3f_dtables* T, const uint8_t* arena, uint8_t* scratch, float* out) {
    const y3f_djob* jobs = reinterpret_cast<const y3f_djob*>(blob);
    for (int j = 0; j < n; ++j) {
        const y3f_djob& d = jobs[j];
        uint8_t* win = scratch + d.win_off;
        uint8_t* tmp = scratch + d.tmp_off;
        const int lw = d.live_x1 - d.live_x0, lh = d.live_y1 - d.live_y0;
        for (long long i = 0; i < (long long)lw * lh; ++i)
            y3fpx::window_pixel<true>(d, blob, arena, *T, d.live_x0 + (int)(i % lw), d.live_y0 + (int)(i / lw), win + 3 * i);
        if (d.mode == Y3F_MODE_RESAMPLE && d.horizontal)
            for (long long i = 0; i < (long long)d.tmp_rows * d.res_w; ++i)
                y3fpx::horizontal_pixel(d, blob, win, (int)(i / d.res_w), (int)(i % d.res_w), tmp + 3 * i);
        float* o = out + (size_t)j * d.out_h * d.out_w * 3;
        for (long long i = 0; i < (long long)d.out_h * d.out_w; ++i)
            y3fpx::output_pixel(d, blob, win, tmp, *T, (int)(i % d.out_w), (int)(i / d.out_w), o + 3 * i);
    }
    return 0;
}

// the check y3_feed_run_src makes of every record before it launches anything: what is wrong with it, or NULL
extern "C" const char* y3f_record_fault(const y3f_djob* d, size_t blob_bytes, size_t arena_bytes, size_t scratch_bytes) {
    return y3fpx::record_fault(*d, blob_bytes, arena_bytes, scratch_bytes);
}
