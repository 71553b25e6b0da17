// Rotated varied-size window attention (RVSA): the sampling geometry and the lane helpers shared by the bf16 MFMA kernels
// (attn_rvsa_fwd4.hip, attn_rvsa_bwd4.hip) and -- the geometry only -- by the f32-math kernels of attn.hip.  ONE definition of the closed-form
// sampling grid: forward, backward and the scatter kernel must place every sample in the same cell.  Internal linkage, like attn_full_common.h.
//
// The MFMA kernels (v_mfma_f32_16x16x32_bf16, head_dim = 64): one workgroup of 4 waves per (image, window, head); the 49 x 49 problem is padded to
// 64 x 64 and wave w owns the 16-query tile w (in the backward's key-major phase: the 16-key tile w).
//   Gather: K_sel / V_sel = bilinear blend of <= 4 token rows per key, split over the 256 threads (key x 16-byte chunk) and written as swizzled
//   row-major bf16 images (swz) into LDS.
//   S^T = K_sel . Q^T -> a lane holds (query = lane & 15 of its wave's tile; 4 consecutive keys per key tile), so a query's softmax needs only
//   in-lane reductions + two cross-lane exchanges (xor 16, 32), and the probabilities are directly the B operand of the next MFMA
//   (O^T = V_sel^T . P^T) -- with the k index permuted identically on the A side (rows_frag_tr: transpose reads of the row-major V_sel image return
//   keys k0 .. k0 + 3 and k0 + 16 .. k0 + 19, the keys the lane's two accumulators hold), so P never goes through LDS in the forward.
//   The backward works in two orientations:
//     phase A, query-major (wave = query tile; lane: query, 4 keys): S^T and dP^T = V_sel . dO^T as above, P and dS in registers,
//                                                                  dQ^T = K_sel^T . dS^T          (contraction over keys)
//     phase B, key-major   (wave = key tile; lane: key, 4 queries):  dK_sel^T = Q^T . dS,  dV_sel^T = dO^T . P   (contraction over queries)
//   P and dS cross from A to B through one pair of LDS images; every other operand that is needed in the other orientation (K_sel^T, Q^T, dO^T)
//   is a transpose read of a row-major image (rvsa_bwd5_mfma_kernel) or a transposed image written in 2-byte units (rvsa_bwd4_mfma_kernel, kept
//   for the grids of the atomic scatter and for A/B runs).  dK_sel / dV_sel go back through the bilinear footprint either as one dense product
//   per (image, head) (rvsa_scatter_gemm_kernel) or with f32 atomics; the sampling-coordinate gradients are reduced to the 5 scalars of the
//   (window, head).
#pragma once
#include "attn_common.h"

namespace {

// =====================================================================================================================
// RVSA geometry shared by forward and backward
// =====================================================================================================================
struct RvsaGeom {
    int Hp, Wp, He, We, pad_t, pad_l, nh, nw, heads;
    float inv_div_x, inv_div_y;
};
inline RvsaGeom make_geom(int64_t Hp, int64_t Wp, int64_t heads) {
    RvsaGeom g;
    const RvsaWindows win(Hp, Wp);
    g.Hp = (int)Hp; g.Wp = (int)Wp;
    g.pad_t = win.pad_t; g.pad_l = win.pad_l;
    g.nh = win.nh; g.nw = win.nw;
    g.He = 7 * g.nh; g.We = 7 * g.nw;
    g.heads = (int)heads;
    g.inv_div_x = 1.0f / (float)(Hp / 7);   // VIT:359: x offset / (h // ws)
    g.inv_div_y = 1.0f / (float)(Wp / 7);   // VIT:360: y offset / (w // ws)
    return g;
}

struct Sample {         // one key position's sampling footprint
    float fx, fy;
    int x0, y0;
    float rx, ry, cs, sn, relx, rely;
};
// kFastTrig: v_cos / v_sin (abs error ~1e-6 on |ang| < pi) in the MFMA kernels -- forward, backward and scatter take the same instantiation;
// the f32-math kernels of attn.hip (parity mode) keep the exact cosf / sinf
template <bool kFastTrig>
__device__ __forceinline__ Sample make_sample(const RvsaGeom& g, const float* __restrict__ sp, int h, int wi, int wj, int a, int bb) {
    Sample s;
    const int H = g.heads;
    const float offx = sp[2 * h] * g.inv_div_x, offy = sp[2 * h + 1] * g.inv_div_y;
    const float sx = sp[2 * H + 2 * h] + 1.0f, sy = sp[2 * H + 2 * h + 1] + 1.0f;
    const float ang = sp[4 * H + h];
    const float stepx = 2.0f / (float)(g.We - 1), stepy = 2.0f / (float)(g.He - 1);
    const float cenx = -1.0f + stepx * (float)(7 * wj + 3), ceny = -1.0f + stepy * (float)(7 * wi + 3);   // mean of 7 linspace points
    s.relx = (float)(bb - 3) * stepx;
    s.rely = (float)(a - 3) * stepy;
    s.rx = s.relx * sx;
    s.ry = s.rely * sy;
    s.cs = kFastTrig ? __cosf(ang) : cosf(ang);
    s.sn = kFastTrig ? __sinf(ang) : sinf(ang);
    const float gx = cenx + (s.rx * s.cs - s.ry * s.sn) + offx;
    const float gy = ceny + (s.ry * s.cs + s.rx * s.sn) + offy;
    float ix = (gx + 1.0f) * 0.5f * (float)(g.We - 1), iy = (gy + 1.0f) * 0.5f * (float)(g.He - 1);
    ix = fminf(fmaxf(ix, -4.0f), (float)g.We + 4.0f);   // far-out samples contribute 0 anyway; keeps floor() in int range
    iy = fminf(fmaxf(iy, -4.0f), (float)g.He + 4.0f);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    s.x0 = (int)fx0; s.y0 = (int)fy0;
    s.fx = ix - fx0; s.fy = iy - fy0;
    return s;
}
// neighbour k in {0:(x0,y0), 1:(x1,y0), 2:(x0,y1), 3:(x1,y1)}: bilinear weight, and token index (or -1 when the neighbour
// is outside the padded map [zeros padding of grid_sample] or inside the zero padding ring of the map itself)
__device__ __forceinline__ int neighbour(const RvsaGeom& g, int x0, int y0, float fx, float fy, int k, float& w) {
    const int dx = k & 1, dy = k >> 1;
    const int xi = x0 + dx, yi = y0 + dy;
    w = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy);
    const int tx = xi - g.pad_l, ty = yi - g.pad_t;
    if (xi < 0 || xi > g.We - 1 || yi < 0 || yi > g.He - 1 || tx < 0 || tx >= g.Wp || ty < 0 || ty >= g.Hp) return -1;
    return ty * g.Wp + tx;
}
__device__ __forceinline__ int query_token(const RvsaGeom& g, int n, int wi, int wj) {   // n < 49
    const int a = n / 7, bb = n - 7 * a;
    const int ty = 7 * wi + a - g.pad_t, tx = 7 * wj + bb - g.pad_l;
    return (ty >= 0 && ty < g.Hp && tx >= 0 && tx < g.Wp) ? ty * g.Wp + tx : -1;
}

// =====================================================================================================================
// lane helpers of the MFMA kernels
// =====================================================================================================================
// The table operands are the CLAMPED forms: unconditional loads on a clamped row, masked afterwards (a branch around the loads makes hipcc wait
// for them inside it).  The full-attention family keeps the branchy forms under the same names (attn_full_common.h); the two headers never meet
// in one translation unit.
// 8 f32 table values (row r, elements e0..e0+7) -> bf16 operand; zero when the row is out of range
__device__ __forceinline__ uint4 table_frag(const float* __restrict__ tab, int r, int rows, int e0) {
    const int rc = r < rows ? r : rows - 1;
    const float m = r < rows ? 1.0f : 0.0f;
    const float4 a = *reinterpret_cast<const float4*>(tab + rc * HD + e0), b = *reinterpret_cast<const float4*>(tab + rc * HD + e0 + 4);
    return pack_bf16x8(m * a.x, m * a.y, m * a.z, m * a.w, m * b.x, m * b.y, m * b.z, m * b.w);
}
// transposed table operand: lane (d, g) -> tab[8g+e][d], e = 0..7
__device__ __forceinline__ uint4 table_frag_t(const float* __restrict__ tab, int d, int rows, int r0) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int r = r0 + e;
        const float t = tab[(r < rows ? r : rows - 1) * HD + d];
        v[e] = r < rows ? t : 0.f;
    }
    return pack_bf16x8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
}

__device__ __attribute__((aligned(16))) const uint4 g_zero16a = {0u, 0u, 0u, 0u};
// 16-byte fragment of row `tok` (or zeros when tok < 0) without a branch around the load
__device__ __forceinline__ uint4 row_frag(const bf16_t* __restrict__ rows, int64_t ld, int tok, int e0) {
    return ldg16(tok >= 0 ? reinterpret_cast<const char*>(rows + (int64_t)tok * ld + e0) : reinterpret_cast<const char*>(&g_zero16a));
}

typedef short tr4s_t __attribute__((ext_vector_type(4)));
// transposed fragment out of a row-major swizzled bf16 image (ds_read_b64_tr_b16): lane (fr, gq) gets column 16 dt + fr of rows row0 .. row0 + 3 and row0 + 16 .. + 19
__device__ __forceinline__ uint4 rows_frag_tr(const char* img, int row0, int dt, int fr) {
    const int c = 16 * dt + 4 * (fr & 3);
    const int ra = row0 + (fr >> 2), rb = ra + 16;
    const int oa = ra * 128 + (((c >> 3) ^ (ra & 7)) << 4) + (c & 7) * 2, ob = rb * 128 + (((c >> 3) ^ (rb & 7)) << 4) + (c & 7) * 2;
    const tr4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4s_t*)(img + oa));
    const tr4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4s_t*)(img + ob));
    const uint2 l = __builtin_bit_cast(uint2, lo), hh = __builtin_bit_cast(uint2, hi);
    return make_uint4(l.x, l.y, hh.x, hh.y);
}

}  // namespace
