// Spatial pyramid pooling (YOLOv3-SPP): spp(x) = concat([mp_13(x), mp_9(x), mp_5(x), x]) over NHWC maps, and its backward.
// The definition is the comment under "SPP" in include/yolo355.h; the per-element rules are y3_spp_px.h.
//
// Both kernels: one workgroup per (image, tile of the map, chunk of V 16-byte channel vectors).  The maps are small (13 x 13 to
// 40 x 40), so a tile with its halo - clipped to the map - sits in the LDS as [position][V] vectors; consecutive lanes take
// consecutive vectors of one position, then the next position: 16-byte global accesses over V * 16 contiguous bytes, and
// conflict-free 16-byte LDS accesses.  A map of up to REGION positions a side is one tile.
//   forward   three rounds of mp_5 (a 5-wide row pass, a 5-wide column pass): mp_5, mp_9 = mp_5(mp_5), mp_13 = mp_5(mp_9).
//             A round is exact for positions at least 2 further from a cut edge than the round before: halo 6.
//   backward  per window size k = 5, 9, 13: the first maximum of every window (rows, then columns), then every input element
//             gathers, in row-major order, the gradients of the windows that chose it.  Halo 12: a window's centre is up to
//             k/2 away, its own window reaches k/2 further.  No atomics, one fixed order.
#include <algorithm>
#include "y3_internal.h"
#include "y3_spp_px.h"

namespace {

using namespace y3spp;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int NTH = 256;
constexpr int REGION = 32;                      // most positions a side of a tile with its halo
constexpr int FWD_TILE = REGION - 2 * kFwdHalo, BWD_TILE = REGION - 2 * kBwdHalo;
constexpr size_t LDS_AIM = 64 << 10;            // V is the largest power of two (<= 8) that stays below this ...
constexpr size_t LDS_MAX = 96 << 10;            // ... and one vector a position always fits this
constexpr size_t FWD_BYTES = 2 * 16, BWD_BYTES = 4 * 16 + 8 + 4;      // LDS per (position, vector)

// one axis of the tiling: tile `t` covers [t0, t1), its region [r0, r1) = the tile with its halo, clipped to the map
struct Axis { int t0, t1, r0, r1; };
__device__ __forceinline__ Axis axis_of(int t, int tile, int halo, int n) {
    Axis a;
    a.t0 = t * tile;
    a.t1 = min(a.t0 + tile, n);
    a.r0 = max(a.t0 - halo, 0);
    a.r1 = min(a.t1 + halo, n);
    return a;
}

// the running maximum of a 16-byte vector: 4 floats, or 8 bf16 compared as the floats they are
template <bool BF16>
__device__ __forceinline__ u32x4 vec_max(u32x4 m, u32x4 v) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (BF16) {
            const float lo = max_of(__uint_as_float(m[j] << 16), __uint_as_float(v[j] << 16));
            const float hi = max_of(__uint_as_float(m[j] & 0xffff0000u), __uint_as_float(v[j] & 0xffff0000u));
            r[j] = (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
        } else {
            r[j] = __float_as_uint(max_of(__uint_as_float(m[j]), __uint_as_float(v[j])));
        }
    }
    return r;
}

struct FwdArgs {
    const u32x4* x;      // [n,h,w,vecs] 16-byte vectors
    u32x4* out;          // [n,h,w,4*vecs]
    int h, w, vecs, vshift, tile_h, tile_w, tiles_x;
};

template <bool BF16>
__global__ void __launch_bounds__(NTH) spp_fwd_kernel(const FwdArgs a) {
    extern __shared__ u32x4 smem[];
    const int V = 1 << a.vshift;
    const Axis ay = axis_of((int)blockIdx.y / a.tiles_x, a.tile_h, kFwdHalo, a.h);
    const Axis ax = axis_of((int)blockIdx.y % a.tiles_x, a.tile_w, kFwdHalo, a.w);
    const int rh = ay.r1 - ay.r0, rw = ax.r1 - ax.r0, items = rh * rw * V;
    u32x4 *A = smem, *B = smem + items;
    const long long img = (long long)blockIdx.x * a.h;
    const int v0 = (int)blockIdx.z * V;

    // x into the LDS; the tile's own positions also go to slot 3
    for (int it = threadIdx.x; it < items; it += NTH) {
        const int p = it >> a.vshift, v = v0 + (it & (V - 1));
        const int ry = p / rw, rx = p - ry * rw;
        const int gy = ay.r0 + ry, gx = ax.r0 + rx;
        u32x4 val = {0u, 0u, 0u, 0u};
        if (v < a.vecs) {
            const long long pos = (img + gy) * a.w + gx;
            val = a.x[pos * a.vecs + v];
            if (gy >= ay.t0 && gy < ay.t1 && gx >= ax.t0 && gx < ax.t1) a.out[pos * 4 * a.vecs + 3 * (long long)a.vecs + v] = val;
        }
        A[it] = val;
    }
    for (int round = 0; round < kWindows; ++round) {
        __syncthreads();
        for (int it = threadIdx.x; it < items; it += NTH) {         // rows: A -> B
            const int p = it >> a.vshift, vi = it & (V - 1);
            const int ry = p / rw, rx = p - ry * rw;
            const int lo = win_lo(rx, 5), hi = win_hi(rx, 5, rw);
            u32x4 m = A[((ry * rw + lo) << a.vshift) + vi];
            for (int i = lo + 1; i <= hi; ++i) m = vec_max<BF16>(m, A[((ry * rw + i) << a.vshift) + vi]);
            B[it] = m;
        }
        __syncthreads();
        for (int it = threadIdx.x; it < items; it += NTH) {         // columns: B -> A, and out
            const int p = it >> a.vshift, vi = it & (V - 1), v = v0 + vi;
            const int ry = p / rw, rx = p - ry * rw;
            const int lo = win_lo(ry, 5), hi = win_hi(ry, 5, rh);
            u32x4 m = B[((lo * rw + rx) << a.vshift) + vi];
            for (int i = lo + 1; i <= hi; ++i) m = vec_max<BF16>(m, B[((i * rw + rx) << a.vshift) + vi]);
            A[it] = m;
            const int gy = ay.r0 + ry, gx = ax.r0 + rx;
            if (v < a.vecs && gy >= ay.t0 && gy < ay.t1 && gx >= ax.t0 && gx < ax.t1) {
                const long long pos = (img + gy) * a.w + gx;
                a.out[pos * 4 * a.vecs + (long long)window_slot(round) * a.vecs + v] = m;
            }
        }
    }
}

struct BwdArgs {
    const void* x;       // [n,h,w] rows of x_stride elements, the first c used
    const f32x4* g;      // [n,h,w,4*vecs]
    f32x4* dx;           // [n,h,w,vecs]
    long long x_stride;
    int h, w, vecs, vshift, tile_h, tile_w, tiles_x, accumulate;
};

// 4 channels a vector (g and dx are fp32): x is 16 bytes of fp32 or 8 bytes of bf16
template <bool BF16>
__global__ void __launch_bounds__(NTH) spp_bwd_kernel(const BwdArgs a) {
    extern __shared__ u32x4 smem[];
    const int V = 1 << a.vshift;
    const Axis ay = axis_of((int)blockIdx.y / a.tiles_x, a.tile_h, kBwdHalo, a.h);
    const Axis ax = axis_of((int)blockIdx.y % a.tiles_x, a.tile_w, kBwdHalo, a.w);
    const int rh = ay.r1 - ay.r0, rw = ax.r1 - ax.r0, items = rh * rw * V;
    f32x4* X = reinterpret_cast<f32x4*>(smem);          // x
    f32x4* RM = X + items;                              // a row window's first maximum ...
    f32x4* G = RM + items;                              // the gradient of the window size at hand
    f32x4* ACC = G + items;                             // the sum so far (the tile's own positions)
    u32x2* ARG = reinterpret_cast<u32x2*>(ACC + items); // a window's first maximum: (y << 8 | x) in the region, 16 bits a channel
    unsigned* RA = reinterpret_cast<unsigned*>(ARG + items);   // ... and its column, 8 bits a channel
    const long long img = (long long)blockIdx.x * a.h;
    const int v0 = (int)blockIdx.z * V;

    for (int it = threadIdx.x; it < items; it += NTH) {
        const int p = it >> a.vshift, v = v0 + (it & (V - 1));
        const int ry = p / rw, rx = p - ry * rw;
        const int gy = ay.r0 + ry, gx = ax.r0 + rx;
        f32x4 val = {0.f, 0.f, 0.f, 0.f}, id = val;
        if (v < a.vecs) {
            const long long pos = (img + gy) * a.w + gx;
            if (BF16) {
                const u32x2 raw = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(a.x) + pos * a.x_stride + 4 * v);
                val[0] = __uint_as_float(raw[0] << 16); val[1] = __uint_as_float(raw[0] & 0xffff0000u);
                val[2] = __uint_as_float(raw[1] << 16); val[3] = __uint_as_float(raw[1] & 0xffff0000u);
            } else {
                val = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.x) + pos * a.x_stride + 4 * v);
            }
            if (gy >= ay.t0 && gy < ay.t1 && gx >= ax.t0 && gx < ax.t1) id = a.g[pos * 4 * a.vecs + 3 * (long long)a.vecs + v];
        }
        X[it] = val;
        ACC[it] = id;       // the identity term first
    }
    for (int j = 0; j < kWindows; ++j) {
        const int k = window_k(j);
        __syncthreads();
        for (int it = threadIdx.x; it < items; it += NTH) {         // the gradient of this slot; the rows' first maxima
            const int p = it >> a.vshift, vi = it & (V - 1), v = v0 + vi;
            const int ry = p / rw, rx = p - ry * rw;
            f32x4 gq = {0.f, 0.f, 0.f, 0.f};
            if (v < a.vecs) {
                const long long pos = (img + ay.r0 + ry) * a.w + ax.r0 + rx;
                gq = a.g[pos * 4 * a.vecs + (long long)window_slot(j) * a.vecs + v];
            }
            G[it] = gq;
            const int lo = win_lo(rx, k), hi = win_hi(rx, k, rw);
            f32x4 m = X[((ry * rw + lo) << a.vshift) + vi];
            int arg[4] = {lo, lo, lo, lo};
            for (int i = lo + 1; i <= hi; ++i) {
                const f32x4 val = X[((ry * rw + i) << a.vshift) + vi];
#pragma unroll
                for (int c = 0; c < 4; ++c) { float mc = m[c]; first_max_step(val[c], i, &mc, &arg[c]); m[c] = mc; }
            }
            RM[it] = m;
            RA[it] = (unsigned)arg[0] | (unsigned)arg[1] << 8 | (unsigned)arg[2] << 16 | (unsigned)arg[3] << 24;
        }
        __syncthreads();
        for (int it = threadIdx.x; it < items; it += NTH) {         // columns: the window's first maximum
            const int p = it >> a.vshift, vi = it & (V - 1);
            const int ry = p / rw, rx = p - ry * rw;
            const int lo = win_lo(ry, k), hi = win_hi(ry, k, rh);
            f32x4 m = RM[((lo * rw + rx) << a.vshift) + vi];
            int arg[4] = {lo, lo, lo, lo};
            for (int i = lo + 1; i <= hi; ++i) {
                const f32x4 val = RM[((i * rw + rx) << a.vshift) + vi];
#pragma unroll
                for (int c = 0; c < 4; ++c) { float mc = m[c]; first_max_step(val[c], i, &mc, &arg[c]); m[c] = mc; }
            }
            unsigned code[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned col = (RA[((arg[c] * rw + rx) << a.vshift) + vi] >> (8 * c)) & 255u;
                code[c] = (unsigned)arg[c] << 8 | col;
            }
            u32x2 packed;
            packed[0] = code[0] | code[1] << 16;
            packed[1] = code[2] | code[3] << 16;
            ARG[it] = packed;
        }
        __syncthreads();
        for (int it = threadIdx.x; it < items; it += NTH) {         // gather: the windows that chose this element, row-major
            const int p = it >> a.vshift, vi = it & (V - 1);
            const int ry = p / rw, rx = p - ry * rw;
            const int gy = ay.r0 + ry, gx = ax.r0 + rx;
            if (!(gy >= ay.t0 && gy < ay.t1 && gx >= ax.t0 && gx < ax.t1)) continue;
            const unsigned me = (unsigned)ry << 8 | (unsigned)rx;
            f32x4 acc = ACC[it];
            for (int qy = win_lo(ry, k); qy <= win_hi(ry, k, rh); ++qy)
                for (int qx = win_lo(rx, k); qx <= win_hi(rx, k, rw); ++qx) {
                    const int q = ((qy * rw + qx) << a.vshift) + vi;
                    const u32x2 packed = ARG[q];
                    const f32x4 gq = G[q];
                    if ((packed[0] & 0xffffu) == me) acc[0] = acc[0] + gq[0];
                    if ((packed[0] >> 16) == me) acc[1] = acc[1] + gq[1];
                    if ((packed[1] & 0xffffu) == me) acc[2] = acc[2] + gq[2];
                    if ((packed[1] >> 16) == me) acc[3] = acc[3] + gq[3];
                }
            ACC[it] = acc;
        }
    }
    // (each thread reads back the ACC entries it wrote itself)
    for (int it = threadIdx.x; it < items; it += NTH) {
        const int p = it >> a.vshift, v = v0 + (it & (V - 1));
        const int ry = p / rw, rx = p - ry * rw;
        const int gy = ay.r0 + ry, gx = ax.r0 + rx;
        if (v >= a.vecs || !(gy >= ay.t0 && gy < ay.t1 && gx >= ax.t0 && gx < ax.t1)) continue;
        f32x4* at = a.dx + ((img + gy) * a.w + gx) * a.vecs + v;
        const f32x4 acc = ACC[it];
        *at = a.accumulate ? *at + acc : acc;
    }
}

// The tiling of one axis and the chunk width for a map: a map of up to REGION positions is one tile
struct Shape { int tile_h, tile_w, tiles_y, tiles_x, vshift; size_t lds; };
Shape shape_for(int h, int w, int vecs, int tile, int halo, size_t bytes) {
    Shape s;
    s.tile_h = h <= REGION ? h : tile;
    s.tile_w = w <= REGION ? w : tile;
    s.tiles_y = (h + s.tile_h - 1) / s.tile_h;
    s.tiles_x = (w + s.tile_w - 1) / s.tile_w;
    const size_t region = (size_t)std::min(h, s.tile_h + 2 * halo) * std::min(w, s.tile_w + 2 * halo);
    s.vshift = 0;
    while (s.vshift < 3 && (1 << s.vshift) < vecs && (region * bytes << (s.vshift + 1)) <= LDS_AIM) ++s.vshift;
    s.lds = region * bytes << s.vshift;
    return s;
}

template <auto Kern, class Args>
int launch(hipStream_t stream, const Shape& s, int n, int vecs, const Args& a) {
    static bool attr_set[Y3_MAX_DEVICES] = {};      // (per kernel instantiation and device; a benign race, the call is idempotent)
    const int dev = y3_current_device();
    if (dev < 0 || !attr_set[dev]) {
        Y3_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
        if (dev >= 0) attr_set[dev] = true;
    }
    const int V = 1 << s.vshift;
    hipLaunchKernelGGL(Kern, dim3(n, s.tiles_y * s.tiles_x, (vecs + V - 1) / V), dim3(NTH), s.lds, stream, a);
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}

int check_dims(const char* who, int n, int h, int w, int c) {
    Y3_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "%s: non-positive dimension", who);
    Y3_CHECK_ARG(c % 8 == 0, "%s: channels must be a multiple of 8 (got %d)", who, c);
    Y3_CHECK_ARG(c / 4 <= 65535 && (long long)((h + BWD_TILE - 1) / BWD_TILE) * ((w + BWD_TILE - 1) / BWD_TILE) <= 65535,
                 "%s: the map or the channel count is beyond one launch's grid", who);
    return Y3_OK;
}

}  // namespace

extern "C" int y3_spp_fwd(y3_ctx* ctx, const void* x, int bf16, int n, int h, int w, int c, void* out) {
    Y3_CHECK_ARG(ctx && x && out, "y3_spp_fwd: null argument");
    if (int rc = check_dims("y3_spp_fwd", n, h, w, c)) return rc;
    Y3_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "y3_spp_fwd: x and out must be 16-byte aligned");
    const int vecs = bf16 ? c / 8 : c / 4;
    const Shape s = shape_for(h, w, vecs, FWD_TILE, kFwdHalo, FWD_BYTES);
    FwdArgs a{static_cast<const u32x4*>(x), static_cast<u32x4*>(out), h, w, vecs, s.vshift, s.tile_h, s.tile_w, s.tiles_x};
    return bf16 ? launch<spp_fwd_kernel<true>>(ctx->stream, s, n, vecs, a) : launch<spp_fwd_kernel<false>>(ctx->stream, s, n, vecs, a);
}

extern "C" int y3_spp_bwd(y3_ctx* ctx, const void* x, int x_stride, int bf16, const float* g, int n, int h, int w, int c,
                          int accumulate, float* dx) {
    Y3_CHECK_ARG(ctx && x && g && dx, "y3_spp_bwd: null argument");
    if (int rc = check_dims("y3_spp_bwd", n, h, w, c)) return rc;
    Y3_CHECK_ARG(x_stride >= c && x_stride % 8 == 0, "y3_spp_bwd: x_stride must be a multiple of 8 and at least c (got %d)", x_stride);
    Y3_CHECK_ARG((((uintptr_t)x | (uintptr_t)g | (uintptr_t)dx) & 15) == 0, "y3_spp_bwd: x, g and dx must be 16-byte aligned");
    const int vecs = c / 4;
    const Shape s = shape_for(h, w, vecs, BWD_TILE, kBwdHalo, BWD_BYTES);
    BwdArgs a{x, reinterpret_cast<const f32x4*>(g), reinterpret_cast<f32x4*>(dx), x_stride, h, w, vecs, s.vshift, s.tile_h, s.tile_w,
              s.tiles_x, accumulate};
    return bf16 ? launch<spp_bwd_kernel<true>>(ctx->stream, s, n, vecs, a) : launch<spp_bwd_kernel<false>>(ctx->stream, s, n, vecs, a);
}
