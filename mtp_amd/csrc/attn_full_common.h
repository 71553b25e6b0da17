// helpers shared by the full-attention MFMA kernels (attn_full_v3.hip: token grids of at most 16 x 16; attn_full_flash_fwd.hip /
// attn_full_flash_bwd.hip: the flash forward and backward beyond 256 tokens).  Internal linkage: every translation unit gets its own copy.
#pragma once
#include "attn_common.h"

namespace {

__device__ __attribute__((aligned(16))) const uint4 g_zero16f = {0u, 0u, 0u, 0u};

__device__ __forceinline__ uint4 row_frag(const bf16_t* __restrict__ rows, int64_t ld, int tok, bool ok, int e0) {
    return ldg16(ok ? reinterpret_cast<const char*>(rows + (int64_t)tok * ld + e0) : reinterpret_cast<const char*>(&g_zero16f));
}
// the table operands are the BRANCHY forms (the RVSA family has clamped loads under the same names, attn_rvsa_common.h; the two headers never meet in one
// translation unit)
__device__ __forceinline__ uint4 table_frag(const float* __restrict__ tab, int r, int rows, int e0) {
    if (r >= rows) return make_uint4(0, 0, 0, 0);
    const float4 a = *reinterpret_cast<const float4*>(tab + r * HD + e0), b = *reinterpret_cast<const float4*>(tab + r * HD + e0 + 4);
    return pack_bf16x8(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
}
__device__ __forceinline__ uint4 table_frag_t(const float* __restrict__ tab, int d, int rows, int r0) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (r0 + e) < rows ? tab[(r0 + e) * HD + d] : 0.f;
    return pack_bf16x8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
}
// K^T fragment (MFMA A operand: row d = 16 dt + fr, k = keys key0 .. key0+3 and key0+16 .. key0+19) out of the swizzled row-major K image:
// in each 16-lane group, lane i supplies the address of row i >> 2, columns 4 (i & 3) .. +3 of a [4 keys][16 d] block and receives
// column i of its four rows
typedef short tr4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 kt_frag_tr(const char* Ks, int key0, int dt, int fr) {
    const int c = 16 * dt + 4 * (fr & 3);
    const int ra = key0 + (fr >> 2), rb = ra + 16;
    const int oa = ra * 128 + ((((c >> 3) ^ (ra & 7))) << 4) + (c & 7) * 2, ob = rb * 128 + ((((c >> 3) ^ (rb & 7))) << 4) + (c & 7) * 2;
    const tr4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4_t*)(Ks + oa));
    const tr4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4_t*)(Ks + ob));
    const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
    return make_uint4(l.x, l.y, h.x, h.y);
}

// ROWS 64-wide rows of qkv (K, V, ...) -> swizzled row-major LDS image, rows >= N zeroed, in two steps for a software-pipelined block loop: the global loads of the NEXT block are issued into registers right behind the barrier that
// publishes the current one (prefetch_rows) and written to LDS at the top of the next trip (commit_rows) -- their latency runs under the block's MFMAs
template <int ROWS>
__device__ __forceinline__ void prefetch_rows(const bf16_t* __restrict__ src, int64_t ld, int N, int tid, uint4 (&r)[ROWS * 8 / 256]) {
#pragma unroll
    for (int i = 0; i < ROWS * 8 / 256; ++i) {
        const int idx = tid + 256 * i, row = idx >> 3, c = idx & 7;
        r[i] = row_frag(src, ld, row, row < N, 8 * c);
    }
}
template <int ROWS>
__device__ __forceinline__ void commit_rows(char* img, int tid, const uint4 (&r)[ROWS * 8 / 256]) {
#pragma unroll
    for (int i = 0; i < ROWS * 8 / 256; ++i) {
        const int idx = tid + 256 * i, row = idx >> 3, c = idx & 7;
        *reinterpret_cast<uint4*>(img + swz(row, c)) = r[i];
    }
}

}  // namespace
