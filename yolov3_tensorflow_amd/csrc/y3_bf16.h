// bf16 as the kernels store it: the type, the two conversions and the 4-wide accesses of the streaming passes.
#pragma once
#include "y3_internal.h"

typedef unsigned short bf16_t;

__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float((unsigned)v << 16); }

// Round to nearest even in integer arithmetic (finite inputs).
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}

// The same rounding for ANY input: in f32_to_bf16 the rounding increment carries a NaN whose low mantissa bits are set out of
// the mantissa (0x7FFFFFFF -> -0.0, 0xFFFFFFFF -> +0.0, 0x7F800001 -> +Inf).  Here a NaN stays a NaN (quiet, sign and upper
// payload kept).  For values that enter from outside (y3_f32_to_bf16); the conv epilogues keep f32_to_bf16.
__device__ __forceinline__ bf16_t f32_to_bf16_any(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x7FFFFFFFu) > 0x7F800000u ? (bf16_t)((u >> 16) | 0x0040u) : f32_to_bf16(f);
}

// (a, b) -> a packed bf16 pair by the compiler's vector conversion.  Not f32_to_bf16 twice: other instructions (and another
// answer for a NaN), and each kernel was measured with the one it uses.
__device__ __forceinline__ unsigned cvt_pack_bf16(float a, float b) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = __builtin_convertvector(f32x2{a, b}, bf16x2);
    return __builtin_bit_cast(unsigned, v);
}

// four consecutive bf16 (8 bytes, 8-byte aligned) <-> f32x4; the store rounds once with f32_to_bf16
__device__ __forceinline__ f32x4 ld_bf16x4(const bf16_t* p) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return f32x4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16),
                 __uint_as_float(v.y & 0xFFFF0000u)};
}
__device__ __forceinline__ void st_bf16x4(bf16_t* p, f32x4 v) {
    *reinterpret_cast<uint2*>(p) = uint2{(unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16),
                                         (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16)};
}
