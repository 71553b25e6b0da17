// lane primitives of every bf16 MFMA attention kernel (v_mfma_f32_16x16x32_bf16, head_dim = 64): the RVSA family (attn_rvsa_common.h) and the
// full-attention family (attn_full_common.h) include this.  Internal linkage: every translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int HD = 64;

// byte offset of 16-byte chunk `chunk` of row `row` in a row-major [row][64 x bf16] LDS image, chunks xor-swizzled by the row
__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
__device__ __forceinline__ f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ uint4 ld16(const char* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ uint4 ld8x2(const char* p0, const char* p1) {   // two 8-byte LDS reads -> one 8 x bf16 operand
    const uint2 a = *reinterpret_cast<const uint2*>(p0), b = *reinterpret_cast<const uint2*>(p1);
    return make_uint4(a.x, a.y, b.x, b.y);
}

}  // namespace
