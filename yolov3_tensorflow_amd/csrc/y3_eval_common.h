// What the evaluator units (y3_voc.hip, y3_coco.hip, y3_beval.hip) share, and y3_nms.hip for the host part: the clamps every
// index read from device memory goes through, the workgroup scans and reductions of the AP kernels, and the one description
// of a scratch layout that its size function and its launcher both evaluate.  The arithmetic that differs between the
// evaluators stays in their *_px.h headers.
#pragma once
#include "y3_internal.h"

namespace y3ev {

// ------------------------------------------------------------------------------------------------ device
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the ranked rows of an arena: the device count word clamped to the arena's rows, or all of them without one
__device__ __forceinline__ int ranked_total(const int32_t* n_rows_dev, int rows) {
    return n_rows_dev ? clampi(*n_rows_dev, 0, rows) : rows;
}

// The block primitives: a workgroup of N threads, every thread calls, `sh` holds N words of the LDS and is free again on
// return.  Each combines in one fixed order, so a result is the same bits in every run.

// exclusive prefix sum of one word per thread in thread order; *total = the block's sum
template <int N, typename T>
__device__ T block_excl_sum(T v, T* sh, T* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const T t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const T incl = sh[tid];
    *total = sh[N - 1];
    __syncthreads();
    return incl - v;
}

// max over the threads to the right of this one (0. for the last), values >= 0; *all = the block's max
template <int N>
__device__ double block_right_max(double v, double* sh, double* all) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const double t = tid + off < N ? sh[tid + off] : 0.;
        __syncthreads();
        sh[tid] = sh[tid] > t ? sh[tid] : t;
        __syncthreads();
    }
    const double right = tid + 1 < N ? sh[tid + 1] : 0.;
    *all = sh[0];
    __syncthreads();
    return right;
}

// the block's sum / the block's max by one fixed tree; the result in every thread
template <int N, typename T, class Op>
__device__ T block_tree(T v, T* sh, Op op) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = op(sh[tid], sh[tid + s]);
        __syncthreads();
    }
    const T out = sh[0];
    __syncthreads();
    return out;
}
template <int N, typename T>
__device__ T block_sum(T v, T* sh) {
    return block_tree<N>(v, sh, [](T a, T b) { return a + b; });
}
template <int N>
__device__ double block_max(double v, double* sh) {
    return block_tree<N>(v, sh, [](double a, double b) { return a > b ? a : b; });
}

// ------------------------------------------------------------------------------------------------ host
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// A scratch layout is written once: a struct whose first member is a Carve and whose regions are members initialised by
// take(), in the order they lie in (or one function, y3_nms.hip).  The launcher builds it on the caller's pointer; the size
// function builds the same struct on null, where every region is null and only bytes() means anything.  Every region begins
// at a 256-byte boundary of a 256-aligned base.
class Carve {
public:
    Carve(void* base) : base_(static_cast<char*>(base)) {}
    template <typename T>
    T* take(size_t count) {
        T* region = base_ ? reinterpret_cast<T*>(base_ + used_) : nullptr;
        used_ += align256(count * sizeof(T));
        return region;
    }
    size_t bytes() const { return used_; }

private:
    char* base_;
    size_t used_ = 0;
};

}  // namespace y3ev
