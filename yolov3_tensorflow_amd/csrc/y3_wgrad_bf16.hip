// Convolution weight gradient of the bf16 train step (net dtype 1): bf16 operands, fp32 MFMA accumulation, fp32 result.
//
//   dW[ky][kx][ci][co] = sum over output pixels m of  x[n, oy*s+ky-pad, ox*s+kx-pad, ci] * dz[m, co]
//
// The GEMM of y3_wgrad.hip, D[j][co] = sum_m P[m][j] * dz[m][co] with j = (ky*k+kx)*Cin + ci (D is the HWIO variable), on
// v_mfma_f32_32x32x16_bf16.  Both operands are stored row-major over the reduction index m, while an MFMA lane holds 8
// consecutive k of ONE row of A (column of B): the K-step tiles are staged as they are loaded ([32 pixels][128 columns],
// 16-byte chunks) and both fragments are read with ds_read_b64_tr_b16, the transposed LDS read of gfx950 (per 16-lane group a
// block of 4 pixels x 16 columns, delivered column-major).  LDS rows are 320 bytes: the four pixel rows of one transposed
// read then start 16 banks apart, and a 32-lane half reads 4 x 64 bytes on 64 distinct banks.
// The pixel range is split over `nsplit` workgroups per output tile so that the grid fills the chip; each split writes its
// fp32 partial tile to scratch and wgrad_bf16_sum_kernel adds the splits in a fixed order (bit-reproducible, no atomics).
// Every Cin of the network is a multiple of 32, so a 16-byte chunk of a P row never crosses a tap: each thread stages one
// fixed (tap, ci) column chunk, and the P gather is x's row of that tap (zero outside the image: buffer loads past the end).
#include <algorithm>
#include "y3_bf16.h"
#include "y3_lds.h"

namespace {

typedef short i16x4 __attribute__((ext_vector_type(4)));

struct WgArgs {
    const bf16_t* x;   // [N,H,W,Cin]
    const bf16_t* dz;  // [M][dzs]
    float* out;        // nsplit == 1: dW [J][Cout]; else scratch [nsplit][J][Cout]
    int N, H, W, Cin, Ho, Wo, Cout, dzs;
    int stride, pad;
    int M, J;          // J = k*k*Cin
    int chunk;         // K-steps per split
    int ksteps;        // ceil(M / 32)
};

constexpr int BK = 32;              // pixels per K-step
constexpr int TJ = 128, TC = 128;   // output tile: j x co
constexpr int LDR = 320;            // LDS row stride in bytes (128 bf16 + 64 bytes of pad)

// 8 k (pixels) of operand column `col` for a 32x32x16 MFMA: lane l = 16g + 4q + p supplies row (8(g>>1) + 4rd + q), columns
// col0 + 16(g&1) + 4p .. +3; it receives column col0 + 16(g&1) + (l&15), k = 8(g>>1) + 4rd + 0..3 in its elements 4rd..4rd+3
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* img, int kbase, int col0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const unsigned char* a = img + (kbase + 8 * (g >> 1) + q) * LDR + (col0 + 16 * (g & 1) + 4 * p) * 2;
    typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
    const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(a));
    const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(a + 4 * LDR));
    typedef short i16x8 __attribute__((ext_vector_type(8)));
    const i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int KS>
__global__ void __launch_bounds__(256, 2) wgrad_bf16_kernel(const WgArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* As = smem;                    // [2][32][LDR]  P[m][j]
    unsigned char* Bs = smem + 2 * BK * LDR;     // [2][32][LDR]  dz[m][co]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;     // 2 x 2 waves, each 64 x 64
    const int nct = (p.Cout + TC - 1) / TC;
    const int jt = blockIdx.x / nct, ct = blockIdx.x - jt * nct;
    const int j0 = jt * TJ, co0 = ct * TC;
    const int s0 = blockIdx.y * p.chunk;
    const int T = min(p.chunk, p.ksteps - s0);

    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16_t*>(p.x), 0, (unsigned)((size_t)p.N * p.H * p.W * p.Cin * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_z = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16_t*>(p.dz), 0, (unsigned)((size_t)p.M * p.dzs * 2), 0x00020000);

    // this thread's column chunk (8 elements) and its two pixel rows r + 16 jj of every K-step
    const int c8 = (tid & 15) * 8, r = tid >> 4;
    const int j = j0 + c8;
    const bool jok = j < p.J;
    const int tap = jok ? j / p.Cin : 0, ci = jok ? j - tap * p.Cin : 0;
    const int ky = tap / KS, kx = tap - (tap / KS) * KS;
    const bool cok = co0 + c8 < p.dzs;
    const int HoWo = p.Ho * p.Wo;

    u32x4 ra[2], rb[2];
    auto load = [&](int step) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int m = (s0 + step) * BK + r + 16 * jj;
            const bool mok = m < p.M;
            unsigned xo;
            if (KS == 1) {        // (stride 1): row m of P is pixel m
                xo = (mok && jok) ? (unsigned)((long long)m * p.Cin + ci) * 2u : OOB;
            } else {
                const int n = m / HoWo, rem = m - n * HoWo;
                const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
                const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
                const bool ok = mok && jok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                xo = ok ? (unsigned)(((n * p.H + iy) * p.W + ix) * p.Cin + ci) * 2u : OOB;
            }
            ra[jj] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xo, 0, 0);
            const unsigned zo = (mok && cok) ? (unsigned)((long long)m * p.dzs + co0 + c8) * 2u : OOB;
            rb[jj] = __builtin_amdgcn_raw_buffer_load_b128(rs_z, zo, 0, 0);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            *reinterpret_cast<u32x4*>(As + buf * BK * LDR + (r + 16 * jj) * LDR + c8 * 2) = ra[jj];
            *reinterpret_cast<u32x4*>(Bs + buf * BK * LDR + (r + 16 * jj) * LDR + c8 * 2) = rb[jj];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[mi][ni][q] = 0.f;

    load(0);
    store(0);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const bool more = t + 1 < T;
        if (more) load(t + 1);
        const unsigned char* as = As + (t & 1) * BK * LDR;
        const unsigned char* bs = Bs + (t & 1) * BK * LDR;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[mi] = tr_frag(as, 16 * kk, wm * 64 + mi * 32, lane);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) b[ni] = tr_frag(bs, 16 * kk, wn * 64 + ni * 32, lane);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
        if (more) store((t + 1) & 1);
        __syncthreads();
    }

    // C/D map of 32x32x16: column lane&31, row (q&3) + 8(q>>2) + 4(lane>>5)
    float* out = p.out + (size_t)blockIdx.y * p.J * p.Cout;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int co = co0 + wn * 64 + ni * 32 + (lane & 31);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int jr = j0 + wm * 64 + mi * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                if (jr < p.J && co < p.Cout) out[(size_t)jr * p.Cout + co] = acc[mi][ni][q];
            }
        }
}

// dW[i] = sum over splits s = 0, 1, ... of part[s][i], in that order
__global__ void __launch_bounds__(256) wgrad_bf16_sum_kernel(const float* __restrict__ part, int nsplit, long long total,
                                                             float* __restrict__ dw) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float s = 0.f;
        for (int k = 0; k < nsplit; ++k) s += part[(size_t)k * total + i];
        dw[i] = s;
    }
}

struct Plan {
    int tiles, ksteps, chunk, nsplit;
    size_t scratch;     // bytes of the nsplit fp32 partial tensors (one split writes dW itself: none)
};

Plan plan_of(const y3_conv_desc* d) {
    Plan q;
    const long long m = (long long)d->n * (d->h / d->stride) * (d->w / d->stride);
    const int J = d->k * d->k * d->cin;
    q.tiles = ((J + TJ - 1) / TJ) * ((d->cout + TC - 1) / TC);
    q.ksteps = (int)((m + BK - 1) / BK);
    // about 1024 workgroups (4 per CU), at least 8 K-steps each
    int ns = std::max(1, std::min((1024 + q.tiles - 1) / q.tiles, (q.ksteps + 7) / 8));
    q.chunk = (q.ksteps + ns - 1) / ns;
    q.nsplit = (q.ksteps + q.chunk - 1) / q.chunk;
    q.scratch = q.nsplit > 1 ? (size_t)q.nsplit * J * d->cout * 4 : 0;
    return q;
}

}  // namespace

extern "C" size_t y3_conv_wgrad_bf16_scratch_bytes(const y3_conv_desc* d) { return plan_of(d).scratch; }

int y3_launch_conv_wgrad_bf16(hipStream_t stream, const y3_conv_desc* d, const void* x, const void* dz, int dz_stride, float* dw,
                              void* scratch, size_t scratch_bytes) {
    Y3_CHECK_ARG(d && x && dz && dw, "y3_conv_wgrad_bf16: null argument");
    Y3_CHECK_ARG(d->k == 1 || d->k == 3, "y3_conv_wgrad_bf16: kernel_size must be 1 or 3");
    Y3_CHECK_ARG(d->k == 3 || d->stride == 1, "y3_conv_wgrad_bf16: 1x1 conv must have stride 1");
    Y3_CHECK_ARG(d->stride == 1 || (d->stride == 2 && d->h % 2 == 0 && d->w % 2 == 0), "y3_conv_wgrad_bf16: bad stride");
    Y3_CHECK_ARG(d->c_up == 0 && d->cin % 32 == 0 && d->cout > 0, "y3_conv_wgrad_bf16: Cin must be a multiple of 32");
    Y3_CHECK_ARG(dz_stride >= d->cout && dz_stride % 8 == 0, "y3_conv_wgrad_bf16: dz stride must be >= Cout and a multiple of 8");
    const long long m = (long long)d->n * (d->h / d->stride) * (d->w / d->stride);
    Y3_CHECK_ARG((long long)d->n * d->h * d->w * d->cin < (1LL << 30) && m * dz_stride < (1LL << 30),
                 "y3_conv_wgrad_bf16: tensor exceeds 2^30 elements (32-bit byte offsets)");
    const Plan q = plan_of(d);
    Y3_CHECK_ARG(scratch_bytes >= q.scratch && (q.scratch == 0 || scratch), "y3_conv_wgrad_bf16: scratch too small (%zu < %zu)",
                 scratch_bytes, q.scratch);
    WgArgs a;
    a.x = static_cast<const bf16_t*>(x); a.dz = static_cast<const bf16_t*>(dz);
    a.out = q.nsplit > 1 ? static_cast<float*>(scratch) : dw;
    a.N = d->n; a.H = d->h; a.W = d->w; a.Cin = d->cin; a.Ho = d->h / d->stride; a.Wo = d->w / d->stride;
    a.Cout = d->cout; a.dzs = dz_stride; a.stride = d->stride; a.pad = d->k / 2;
    a.M = (int)m; a.J = d->k * d->k * d->cin; a.chunk = q.chunk; a.ksteps = q.ksteps;
    const size_t lds = (size_t)4 * BK * LDR;
    const dim3 grid(q.tiles, q.nsplit);
    if (d->k == 1) hipLaunchKernelGGL(wgrad_bf16_kernel<1>, grid, dim3(256), lds, stream, a);
    else hipLaunchKernelGGL(wgrad_bf16_kernel<3>, grid, dim3(256), lds, stream, a);
    Y3_CHECK_HIP(hipGetLastError());
    if (q.nsplit > 1) {
        const long long total = (long long)a.J * d->cout;
        const int blocks = y3_blocks_for(total, 2048);
        hipLaunchKernelGGL(wgrad_bf16_sum_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<const float*>(scratch),
                           q.nsplit, total, dw);
        Y3_CHECK_HIP(hipGetLastError());
    }
    return Y3_OK;
}

extern "C" int y3_conv_wgrad_bf16(y3_ctx* ctx, const y3_conv_desc* fwd, const void* x, const void* dz, int dz_stride,
                                  float* dw_hwio, void* scratch, size_t scratch_bytes) {
    Y3_CHECK_ARG(ctx, "y3_conv_wgrad_bf16: null context");
    return y3_launch_conv_wgrad_bf16(ctx->stream, fwd, x, dz, dz_stride, dw_hwio, scratch, scratch_bytes);
}
