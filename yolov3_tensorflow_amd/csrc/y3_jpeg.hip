// y3_jpeg_decode: the device half of the feeder's JPEG decoder (include/yolo355_jpeg.h).  The host planned n files into one
// blob (y3f_jpeg_plan, liby3feed.so): per image a y3j_rec, its Huffman and quantisation tables, the entropy-coded data
// without stuffing or restart markers, and the cut of every restart interval into chunks of a few hundred bits.  Three
// launches:
//   jpeg_entropy_kernel  one workgroup per image: self-synchronising parallel Huffman decoding, then the coefficients
//   jpeg_idct_kernel     one thread per 8x8 block: dequantisation + jpeg_idct_islow into the sample planes
//   jpeg_rgb_kernel      one thread per output pixel: fancy upsampling + YCbCr -> RGB, packed uint8 HWC
//
// The entropy kernel.  A thread decodes each chunk from a guessed start state (its first bit, z = 0, first block of the
// MCU) up to the first codeword that starts at or past the chunk's end, and publishes that exit state.  A chunk whose
// left neighbour exits in another state adopts it and decodes again; rounds repeat until no state changes.  The first
// chunk of every interval starts from the true state, so the true states propagate from the left and the loop ends after
// at most as many rounds as there are chunks.  Grayscale streams settle in 2-3 rounds; colour streams often keep a wrong
// block-of-the-MCU index after the bit position has resynchronised, so there the true state spreads about one chunk per
// round and decoding is close to serial (profiles/jpeg_rate.txt: median 14, max 482 rounds on about 512 chunks; status_dev
// reports the count).  Letting a chunk decode on past its end until it meets a known state is the next step.
// Then a segmented prefix sum of the blocks each chunk completed gives every chunk its first block, a final pass writes the coefficients into zeroed scratch (a block cut by a chunk
// boundary is written by both threads, each its own coefficients), and a segmented prefix sum per component turns the DC
// differences into values, reset at every restart interval.  All arithmetic: y3_jpeg_px.h, shared with the host build of
// the tests.
#include <algorithm>
#include <cstring>
#include "y3_internal.h"
#include "y3_jpeg_px.h"

namespace {

constexpr int kThreads = 512;
constexpr int kMaxTables = 8;

// inclusive segmented scan over the workgroup of (flag, v[N]): a flagged entry starts a new segment
template <int N>
__device__ void segmented_scan(int* flag, int (*val)[kThreads], int tid) {
    for (int d = 1; d < kThreads; d <<= 1) {
        int f = 0, v[N];
        const bool take = tid >= d;
        if (take) {
            f = flag[tid - d];
            for (int i = 0; i < N; ++i) v[i] = val[i][tid - d];
        }
        __syncthreads();
        if (take && !flag[tid]) {
            for (int i = 0; i < N; ++i) val[i][tid] = (int)((unsigned)val[i][tid] + (unsigned)v[i]);
            flag[tid] = f;
        }
        __syncthreads();
    }
}

// Every kernel reads its records from the head of the scratch: the copy y3_jpeg_decode checked and uploaded, never the blob's.
__global__ void __launch_bounds__(kThreads) jpeg_entropy_kernel(const uint8_t* __restrict__ blob, uint8_t* __restrict__ scratch,
                                                                int* __restrict__ status) {
    const y3j_rec r = reinterpret_cast<const y3j_rec*>(scratch)[blockIdx.x];
    const int tid = threadIdx.x;
    __shared__ y3j_huff tabs[kMaxTables];
    __shared__ int flag[kThreads];
    __shared__ int val[3][kThreads];
    __shared__ int changed, bad;

    {   // the tables into LDS, the coefficients zeroed, every chunk at its guess
        const uint32_t* src = reinterpret_cast<const uint32_t*>(blob + r.tables_off);
        uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
        for (int i = tid; i < r.n_tables * (int)(sizeof(y3j_huff) / 4); i += kThreads) dst[i] = src[i];
        uint4* coef = reinterpret_cast<uint4*>(scratch + r.coef_off);
        for (long long i = tid; i < (long long)r.total_blocks * 8; i += kThreads) coef[i] = make_uint4(0, 0, 0, 0);
        for (int c = tid; c < r.n_chunk; c += kThreads) y3jpx::chunk_init(r, blob, scratch, c);
        if (tid == 0) bad = 0;
    }
    __syncthreads();

    int rounds = 0;
    for (;;) {
        for (int c = tid; c < r.n_chunk; c += kThreads) y3jpx::chunk_sync(r, blob, scratch, tabs, c);
        if (tid == 0) changed = 0;
        __syncthreads();
        bool mine = false;
        for (int c = tid; c < r.n_chunk; c += kThreads) mine |= y3jpx::chunk_adopt(r, blob, scratch, c);
        if (mine) changed = 1;
        __syncthreads();
        ++rounds;
        if (!changed) break;
        if (rounds > r.n_chunk + 1) {
            if (tid == 0) bad |= y3jpx::kNoSync;
            break;
        }
        __syncthreads();
    }

    // first block of every chunk: segmented (per interval) exclusive prefix sum of the blocks completed
    int32_t* count = y3jpx::state_row(r, scratch, 4);
    const int per = (r.n_chunk + kThreads - 1) / kThreads;
    const int c0 = std::min(tid * per, r.n_chunk), c1 = std::min(c0 + per, r.n_chunk);
    {
        int sum = 0, f = 0;
        for (int c = c0; c < c1; ++c) {
            const bool first = c == 0 || y3jpx::chunk_of(r, blob, c).seg != y3jpx::chunk_of(r, blob, c - 1).seg;
            if (first) sum = 0, f = 1;
            sum += count[c];
        }
        flag[tid] = f;
        val[0][tid] = sum;
    }
    __syncthreads();
    segmented_scan<1>(flag, val, tid);
    {
        int carry = tid > 0 ? val[0][tid - 1] : 0;
        __syncthreads();
        int st = 0;
        for (int c = c0; c < c1; ++c) {
            const uint32_t seg = y3jpx::chunk_of(r, blob, c).seg;
            if (c == 0 || seg != y3jpx::chunk_of(r, blob, c - 1).seg) carry = 0;
            const int n = count[c];
            count[c] = y3jpx::seg_block0(r, seg) + carry;
            carry += n;
        }
        for (int c = c0; c < c1; ++c) st |= y3jpx::chunk_write(r, blob, scratch, tabs, c, count[c]);
        if (st) atomicOr(&bad, st);
    }
    __syncthreads();

    // DC values: segmented prefix sum per component over the blocks in decode order, reset at every interval
    int16_t* coef = reinterpret_cast<int16_t*>(scratch + r.coef_off);
    const int seg_blocks = r.restart_interval ? r.restart_interval * r.blocks_per_mcu : r.total_blocks;
    const int bper = (r.total_blocks + kThreads - 1) / kThreads;
    const int g0 = std::min(tid * bper, r.total_blocks), g1 = std::min(g0 + bper, r.total_blocks);
    {
        int s[3] = {0, 0, 0}, f = 0;
        for (int g = g0; g < g1; ++g) {
            if (g % seg_blocks == 0) s[0] = s[1] = s[2] = 0, f = 1;
            const int c = r.blk_comp[g % r.blocks_per_mcu];
            s[c] = (int)((unsigned)s[c] + (unsigned)coef[(size_t)y3jpx::block_addr(r, g) * 64]);
        }
        flag[tid] = f;
        for (int i = 0; i < 3; ++i) val[i][tid] = s[i];
    }
    __syncthreads();
    segmented_scan<3>(flag, val, tid);
    {
        int s[3];
        for (int i = 0; i < 3; ++i) s[i] = tid > 0 ? val[i][tid - 1] : 0;
        for (int g = g0; g < g1; ++g) {
            if (g % seg_blocks == 0) s[0] = s[1] = s[2] = 0;
            const int c = r.blk_comp[g % r.blocks_per_mcu];
            int16_t& dc = coef[(size_t)y3jpx::block_addr(r, g) * 64];
            s[c] = (int)((unsigned)s[c] + (unsigned)dc);
            dc = (int16_t)s[c];
        }
    }
    if (tid == 0) {
        status[2 * blockIdx.x] = bad;
        status[2 * blockIdx.x + 1] = rounds;
    }
}

__global__ void __launch_bounds__(256) jpeg_idct_kernel(const uint8_t* __restrict__ blob, uint8_t* __restrict__ scratch) {
    const y3j_rec r = reinterpret_cast<const y3j_rec*>(scratch)[blockIdx.y];
    for (int k = blockIdx.x * 256 + threadIdx.x; k < r.total_blocks; k += gridDim.x * 256) y3jpx::idct_block(r, blob, scratch, k);
}

__global__ void __launch_bounds__(256) jpeg_rgb_kernel(const uint8_t* __restrict__ scratch, uint8_t* __restrict__ out) {
    const y3j_rec r = reinterpret_cast<const y3j_rec*>(scratch)[blockIdx.y];
    const long long total = (long long)r.width * r.height;
    const uint8_t* planes = scratch + r.plane_off;
    uint8_t* o = out + r.out_off;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        uint8_t px[3];
        y3jpx::rgb_pixel(r, planes, (int)(i % r.width), (int)(i / r.width), px);
        o[3 * i] = px[0], o[3 * i + 1] = px[1], o[3 * i + 2] = px[2];
    }
}

inline unsigned blocks_for(long long work) {
    const long long b = (work + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

}  // namespace

extern "C" int y3_jpeg_decode(y3_ctx* ctx, const void* blob_dev, size_t blob_bytes, const y3j_rec* recs_host, int n,
                              void* scratch_dev, size_t scratch_bytes, void* out_dev, size_t out_bytes, int* status_dev) {
    Y3_CHECK_ARG(ctx && blob_dev && recs_host && scratch_dev && out_dev && status_dev, "y3_jpeg_decode: null argument");
    Y3_CHECK_ARG(n > 0 && n <= 65535, "y3_jpeg_decode: bad image count %d", n);
    const size_t head = ((size_t)n * sizeof(y3j_rec) + 255) & ~(size_t)255;
    Y3_CHECK_ARG((size_t)n * sizeof(y3j_rec) <= blob_bytes && head <= scratch_bytes,
                 "y3_jpeg_decode: %d records do not fit a %zu-byte blob or the head of a %zu-byte scratch", n, blob_bytes,
                 scratch_bytes);
    // the records are copied once, into the context's pinned staging buffer; what is checked is that copy, and that copy is
    // what the kernels read (uploaded to the head of the scratch) - a caller rewriting recs_host later changes nothing
    void* stage = nullptr;
    if (int rc = y3_ctx_stage_acquire(ctx, (size_t)n * sizeof(y3j_rec), &stage)) return rc;
    memcpy(stage, recs_host, (size_t)n * sizeof(y3j_rec));
    const y3j_rec* recs = static_cast<const y3j_rec*>(stage);
    long long max_blocks = 0, max_px = 0;
    for (int i = 0; i < n; ++i) {
        const y3j_rec& r = recs[i];
        Y3_CHECK_ARG(y3jpx::rec_check(r, blob_bytes, scratch_bytes, out_bytes, head) && r.n_tables <= kMaxTables,
                     "y3_jpeg_decode: record %d does not fit the blob (%zu bytes), the scratch (%zu) or the output (%zu)", i,
                     blob_bytes, scratch_bytes, out_bytes);
        max_blocks = std::max(max_blocks, (long long)r.total_blocks);
        max_px = std::max(max_px, (long long)r.width * r.height);
    }
    const uint8_t* blob = static_cast<const uint8_t*>(blob_dev);
    uint8_t* scratch = static_cast<uint8_t*>(scratch_dev);
    Y3_CHECK_HIP(hipMemcpyAsync(scratch, stage, (size_t)n * sizeof(y3j_rec), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = y3_ctx_stage_release(ctx)) return rc;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n), dim3(kThreads), 0, ctx->stream, blob, scratch, status_dev);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(blocks_for(max_blocks), n), dim3(256), 0, ctx->stream, blob, scratch);
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3(blocks_for(max_px), n), dim3(256), 0, ctx->stream, scratch,
                       static_cast<uint8_t*>(out_dev));
    Y3_CHECK_HIP(hipGetLastError());
    return Y3_OK;
}
