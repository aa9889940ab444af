// Device primitives the conv and weight-gradient kernels share: the vector types of their loads and MFMA operands, the
// out-of-range buffer offset, the global -> LDS DMA and the F(2x2,3x3) input transform.
// Only what is byte-identical in every user lives here: tile constants (BK is K elements in one file and pixels in another)
// and the LDS swizzles (lds_off has three forms) stay in their files.
#pragma once
#include "y3_internal.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr unsigned OOB = 0x80000000u;  // any offset >= num_records reads as 0 through a buffer load

// 16 bytes per lane, global -> LDS without a register round trip: lane l's bytes land at lds_base + 16*l (lds_base is
// wave-uniform), an out-of-range `voff` writes zeros.  (The builtin exists in the device pass only; hipcc's host pass
// instantiates the kernel templates too and silently drops their launch stubs if it meets it there.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, unsigned char* lds_base, unsigned voff, unsigned soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)lds_base, 16, voff, soff, 0, 0);
#endif
}

// F(2x2,3x3) input transform B^T d B, on floats or float4s (4 channels at once).  d[i][j], i = patch row, j = patch column;
// result v[i*4+j].
template <typename V>
__device__ __forceinline__ void input_transform(const V (&d)[16], V (&v)[16]) {
    V t[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {          // rows: B^T d
        t[0 * 4 + j] = d[0 * 4 + j] - d[2 * 4 + j];
        t[1 * 4 + j] = d[1 * 4 + j] + d[2 * 4 + j];
        t[2 * 4 + j] = d[2 * 4 + j] - d[1 * 4 + j];
        t[3 * 4 + j] = d[1 * 4 + j] - d[3 * 4 + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {          // columns: (B^T d) B
        v[i * 4 + 0] = t[i * 4 + 0] - t[i * 4 + 2];
        v[i * 4 + 1] = t[i * 4 + 1] + t[i * 4 + 2];
        v[i * 4 + 2] = t[i * 4 + 2] - t[i * 4 + 1];
        v[i * 4 + 3] = t[i * 4 + 1] - t[i * 4 + 3];
    }
}
