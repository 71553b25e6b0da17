// Change detection (open-cd SiamEncoderDecoder + FeatureFusionNeck + UNetHead, RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/
// unet_head.py): the data movement around the decoder's GEMMs.  Two kernel families:
//   fuse_pair   the backbone's 2N-batch NCHW map ("from" images first, "to" images last) -> the fused channels-last rows of the N pairs, the layout
//               change and the fusion in one pass through an LDS tile; the backward recomputes the sign of abs_diff from the saved inputs.
//   up_cat      a decoder block's conv input: x nearest x2 in columns [0, Cx), the skip resized bilinearly (resize_fwd_kernel's index rule and
//               operation order) in columns [Cx, Cx + Cs), written once; the backward is a gather (four children per source pixel, fixed order).
// Maps are channels-last (rows, C) with a row pitch ld as in decode_head.hip; indexing is int64; no float atomics.
#include "common.h"
#include "resize_common.h"

namespace {

constexpr int kTile = 64;       // fuse_pair: positions x channels per workgroup

inline bool policy_ok(int p) { return p == MTP_FUSE_CONCAT || p == MTP_FUSE_SUM || p == MTP_FUSE_DIFF || p == MTP_FUSE_ABS_DIFF; }

// ---------------------------------------------------------------------------------------------------------------- fuse_pair
__device__ __forceinline__ float fuse1(float a, float b, int policy) {
    return policy == MTP_FUSE_SUM ? a + b : policy == MTP_FUSE_DIFF ? b - a : fabsf(a - b);
}

// Workgroup (x: 64 positions, y: 64 channels, z: pair n -- or, for concat, sample b of the 2N, whose columns start at (b / N) * C).  The NCHW side is
// read along the positions (VEC: 4 per lane, when S % 4 == 0 and the base is 16-byte aligned), fused in registers, transposed through LDS
// (tile[channel][position], pitch 65: both sides conflict-free) and written 4 channels per lane.
template <typename TI, typename TO, bool VEC>
__global__ void __launch_bounds__(kThreads) fuse_pair_fwd_kernel(const TI* __restrict__ f, TO* __restrict__ out, int64_t ld, int64_t N, int64_t C, int64_t S,
                                                                 int policy) {
    __shared__ float tile[kTile][kTile + 1];
    const int64_t b = blockIdx.z;
    const bool cat = policy == MTP_FUSE_CONCAT;
    const int64_t n = cat ? b % N : b, col0 = cat ? (b / N) * C : 0;
    const int64_t s0 = (int64_t)blockIdx.x * kTile, c0 = (int64_t)blockIdx.y * kTile;
    const TI* f1 = f + b * C * S;
    const TI* f2 = f + (b + N) * C * S;      // read only when the policy fuses (b < N then)
    const int t = threadIdx.x;
    if (VEC) {
        const int ra = t >> 4, pg = (t & 15) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cl = ra + 16 * k;
            const int64_t c = c0 + cl, s = s0 + pg;
            if (c < C && s < S) {
                float4 a = load4(f1 + c * S + s);
                if (!cat) {
                    const float4 q = load4(f2 + c * S + s);
                    a = make_float4(fuse1(a.x, q.x, policy), fuse1(a.y, q.y, policy), fuse1(a.z, q.z, policy), fuse1(a.w, q.w, policy));
                }
                tile[cl][pg] = a.x; tile[cl][pg + 1] = a.y; tile[cl][pg + 2] = a.z; tile[cl][pg + 3] = a.w;
            }
        }
    } else {
        const int ra = t >> 6, ps = t & 63;
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int cl = ra + 4 * k;
            const int64_t c = c0 + cl, s = s0 + ps;
            if (c < C && s < S) {
                const float a = Elem<TI>::load(f1 + c * S + s);
                tile[cl][ps] = cat ? a : fuse1(a, Elem<TI>::load(f2 + c * S + s), policy);
            }
        }
    }
    __syncthreads();
    const int pr = t >> 4, cg = (t & 15) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pl = pr + 16 * k;
        const int64_t s = s0 + pl, c = c0 + cg;
        if (s < S && c < C) store4(out + (n * S + s) * ld + col0 + c, make_float4(tile[cg][pl], tile[cg + 1][pl], tile[cg + 2][pl], tile[cg + 3][pl]));
    }
}

// The adjoint on the same tiling, the other way round: 4 channels per lane of the row gradient into LDS, then along the positions into both halves of
// the NCHW gradient.  abs_diff: sign(x1 - x2) from the saved inputs, sign(0) = 0 (torch's abs rule); nothing but the inputs is kept for it.
template <typename TI>
__global__ void __launch_bounds__(kThreads) fuse_pair_bwd_kernel(const float* __restrict__ g, int64_t ldg, const TI* __restrict__ f, float* __restrict__ df,
                                                                 int64_t N, int64_t C, int64_t S, int policy) {
    __shared__ float tile[kTile][kTile + 1];
    const int64_t b = blockIdx.z;
    const bool cat = policy == MTP_FUSE_CONCAT;
    const int64_t n = cat ? b % N : b, col0 = cat ? (b / N) * C : 0;
    const int64_t s0 = (int64_t)blockIdx.x * kTile, c0 = (int64_t)blockIdx.y * kTile;
    const int t = threadIdx.x;
    const int pr = t >> 4, cg = (t & 15) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pl = pr + 16 * k;
        const int64_t s = s0 + pl, c = c0 + cg;
        if (s < S && c < C) {
            const float4 v = load4(g + (n * S + s) * ldg + col0 + c);
            tile[cg][pl] = v.x; tile[cg + 1][pl] = v.y; tile[cg + 2][pl] = v.z; tile[cg + 3][pl] = v.w;
        }
    }
    __syncthreads();
    const int ra = t >> 6, ps = t & 63;
    const int64_t o1 = b * C * S, o2 = (b + N) * C * S;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int cl = ra + 4 * k;
        const int64_t c = c0 + cl, s = s0 + ps;
        if (c >= C || s >= S) continue;
        const float gv = tile[cl][ps];
        const int64_t i = c * S + s;
        if (cat) {
            df[o1 + i] = gv;
        } else if (policy == MTP_FUSE_SUM) {
            df[o1 + i] = gv;
            df[o2 + i] = gv;
        } else if (policy == MTP_FUSE_DIFF) {
            df[o1 + i] = -gv;
            df[o2 + i] = gv;
        } else {
            const float d = Elem<TI>::load(f + o1 + i) - Elem<TI>::load(f + o2 + i);
            const float r = gv * (float)((d > 0.0f) - (d < 0.0f));
            df[o1 + i] = r;
            df[o2 + i] = -r;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- up_cat
// One thread per (output pixel, 4 columns of the concatenation).  same: the skip already has the 2h x 2w grid (plain copies).
template <typename TX, typename TY>
__global__ void __launch_bounds__(kThreads) up_cat_fwd_kernel(const void* x, int64_t ldx, int64_t Cx, const void* skip, int64_t lds, int64_t Cs, void* y,
                                                              int64_t ldy, int64_t N, int h, int w, int hs, int ws) {
    const int Ho = 2 * h, Wo = 2 * w;
    const int64_t C4 = (Cx + Cs) / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N * Ho * Wo * C4) return;
    const int64_t pix = i / C4, c = (i - pix * C4) * 4;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
    const int64_t n = pix / ((int64_t)Wo * Ho);
    float4 o;
    if (c < Cx) {
        o = ld4<TX>(x, ((n * h + (oy >> 1)) * w + (ox >> 1)) * ldx + c);
    } else if (hs == Ho && ws == Wo) {
        o = ld4<TX>(skip, pix * lds + (c - Cx));
    } else {
        const int64_t cs = c - Cx, b = n * hs * ws;
        const Lin ly = lin_index(oy, hs, (float)hs / (float)Ho), lx = lin_index(ox, ws, (float)ws / (float)Wo);
        const float4 v00 = ld4<TX>(skip, (b + (int64_t)ly.i0 * ws + lx.i0) * lds + cs), v01 = ld4<TX>(skip, (b + (int64_t)ly.i0 * ws + lx.i1) * lds + cs);
        const float4 v10 = ld4<TX>(skip, (b + (int64_t)ly.i1 * ws + lx.i0) * lds + cs), v11 = ld4<TX>(skip, (b + (int64_t)ly.i1 * ws + lx.i1) * lds + cs);
        const float4 t0 = f4add(f4scale(v00, lx.w0), f4scale(v01, lx.w1)), t1 = f4add(f4scale(v10, lx.w0), f4scale(v11, lx.w1));
        o = f4add(f4scale(t0, ly.w0), f4scale(t1, ly.w1));
    }
    st4<TY>(y, pix * ldy + c, o);
}

// dx[iy][ix] = ((dy[2iy][2ix] + dy[2iy][2ix + 1]) + dy[2iy + 1][2ix]) + dy[2iy + 1][2ix + 1]: always this order
__global__ void __launch_bounds__(kThreads) up_bwd_kernel(const float* dy, int64_t lddy, float* dx, int64_t lddx, int64_t Cx, int64_t N, int h, int w,
                                                          int accumulate) {
    const int64_t C4 = Cx / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N * h * w * C4) return;
    const int64_t pix = i / C4, c = (i - pix * C4) * 4;
    const int ix = (int)(pix % w), iy = (int)((pix / w) % h);
    const int64_t n = pix / ((int64_t)w * h);
    const int64_t Wo = 2 * (int64_t)w;
    const int64_t r0 = ((n * 2 * h + 2 * iy) * Wo + 2 * ix) * lddy + c, r1 = r0 + Wo * lddy;
    float4 acc = f4add(f4add(f4add(load4(dy + r0), load4(dy + r0 + lddy)), load4(dy + r1)), load4(dy + r1 + lddy));
    float* o = dx + pix * lddx + c;
    if (accumulate) acc = f4add(acc, load4(o));
    store4(o, acc);
}

inline bool fits_grid(int64_t threads) { return threads > 0 && (threads + kThreads - 1) / kThreads < (int64_t)INT32_MAX; }

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_fuse_pair_fwd(const void* f, int f_dtype, void* out, int out_dtype, int64_t ld, int64_t N, int64_t C, int64_t H, int64_t W, int policy,
                                 mtp_stream_t stream) {
    MTP_CHECK_ARG(f && out && N > 0 && C > 0 && (C % 4) == 0 && H > 0 && W > 0 && H < INT32_MAX && W < INT32_MAX && dt_ok(f_dtype) && dt_ok(out_dtype));
    MTP_CHECK_ARG(policy_ok(policy) && (ld % 4) == 0 && ld >= (policy == MTP_FUSE_CONCAT ? 2 * C : C) && ((uintptr_t)out & 7) == 0);
    MTP_CHECK_ARG(out_dtype == MTP_BF16 || ((uintptr_t)out & 15) == 0);
    const int64_t S = H * W, nz = policy == MTP_FUSE_CONCAT ? 2 * N : N;
    MTP_CHECK_ARG(nz <= 65535 && (C + kTile - 1) / kTile <= 65535 && (S + kTile - 1) / kTile < (int64_t)INT32_MAX);
    const dim3 grid((unsigned)((S + kTile - 1) / kTile), (unsigned)((C + kTile - 1) / kTile), (unsigned)nz);
    const bool vec = (S % 4) == 0 && ((uintptr_t)f & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    MTP_DISPATCH2(f_dtype, out_dtype,
                  if (vec) fuse_pair_fwd_kernel<TA, TB, true><<<grid, kThreads, 0, s>>>((const TA*)f, (TB*)out, ld, N, C, S, policy);
                  else fuse_pair_fwd_kernel<TA, TB, false><<<grid, kThreads, 0, s>>>((const TA*)f, (TB*)out, ld, N, C, S, policy));
    return mtp_launch_status();
}

extern "C" int mtp_fuse_pair_bwd(const float* g, int64_t ldg, const void* f, int f_dtype, float* df, int64_t N, int64_t C, int64_t H, int64_t W, int policy,
                                 mtp_stream_t stream) {
    MTP_CHECK_ARG(g && df && N > 0 && C > 0 && (C % 4) == 0 && H > 0 && W > 0 && H < INT32_MAX && W < INT32_MAX && policy_ok(policy));
    MTP_CHECK_ARG((ldg % 4) == 0 && ldg >= (policy == MTP_FUSE_CONCAT ? 2 * C : C) && ((uintptr_t)g & 15) == 0);
    MTP_CHECK_ARG(policy != MTP_FUSE_ABS_DIFF || (f && dt_ok(f_dtype)));
    const int64_t S = H * W, nz = policy == MTP_FUSE_CONCAT ? 2 * N : N;
    MTP_CHECK_ARG(nz <= 65535 && (C + kTile - 1) / kTile <= 65535 && (S + kTile - 1) / kTile < (int64_t)INT32_MAX);
    const dim3 grid((unsigned)((S + kTile - 1) / kTile), (unsigned)((C + kTile - 1) / kTile), (unsigned)nz);
    hipStream_t s = (hipStream_t)stream;
    if (policy == MTP_FUSE_ABS_DIFF && f_dtype == MTP_BF16) fuse_pair_bwd_kernel<bf16_t><<<grid, kThreads, 0, s>>>(g, ldg, (const bf16_t*)f, df, N, C, S, policy);
    else fuse_pair_bwd_kernel<float><<<grid, kThreads, 0, s>>>(g, ldg, (const float*)f, df, N, C, S, policy);
    return mtp_launch_status();
}

extern "C" int mtp_unet_up_cat_fwd(const void* x, int64_t ldx, int64_t Cx, const void* skip, int64_t lds, int64_t Cs, int in_dtype, void* y, int y_dtype,
                                   int64_t ldy, int64_t N, int64_t h, int64_t w, int64_t hs, int64_t ws, mtp_stream_t stream) {
    MTP_CHECK_ARG(x && y && N > 0 && h > 0 && w > 0 && h < INT32_MAX / 2 && w < INT32_MAX / 2 && Cx > 0 && (Cx % 4) == 0 && dt_ok(in_dtype) && dt_ok(y_dtype));
    if (!skip) Cs = 0;
    MTP_CHECK_ARG(Cs >= 0 && (Cs % 4) == 0 && ldx >= Cx && (ldx % 4) == 0 && ldy >= Cx + Cs && (ldy % 4) == 0);
    MTP_CHECK_ARG(Cs == 0 || (hs > 0 && ws > 0 && hs < INT32_MAX && ws < INT32_MAX && lds >= Cs && (lds % 4) == 0));
    const int64_t threads = N * 4 * h * w * ((Cx + Cs) / 4);
    MTP_CHECK_ARG(fits_grid(threads));
    hipStream_t s = (hipStream_t)stream;
    MTP_DISPATCH2(in_dtype, y_dtype,
                  up_cat_fwd_kernel<TA, TB><<<blocks_exact(threads), kThreads, 0, s>>>(x, ldx, Cx, skip, lds, Cs, y, ldy, N, (int)h, (int)w, (int)hs, (int)ws));
    return mtp_launch_status();
}

extern "C" int mtp_unet_up_cat_bwd(const float* dy, int64_t lddy, float* dx, int64_t lddx, int64_t Cx, float* dskip, int64_t ldds, int64_t Cs, int64_t N,
                                   int64_t h, int64_t w, int64_t hs, int64_t ws, int accumulate, mtp_stream_t stream) {
    MTP_CHECK_ARG(dy && dx && N > 0 && h > 0 && w > 0 && h < INT32_MAX / 2 && w < INT32_MAX / 2 && Cx > 0 && (Cx % 4) == 0);
    if (!dskip) Cs = 0;
    MTP_CHECK_ARG(Cs >= 0 && (Cs % 4) == 0 && lddx >= Cx && (lddx % 4) == 0 && lddy >= Cx + Cs && (lddy % 4) == 0);
    const int64_t threads = N * h * w * (Cx / 4);
    MTP_CHECK_ARG(fits_grid(threads));
    up_bwd_kernel<<<blocks_exact(threads), kThreads, 0, (hipStream_t)stream>>>(dy, lddy, dx, lddx, Cx, N, (int)h, (int)w, accumulate);
    const int rc = mtp_launch_status();
    if (rc != 0 || Cs == 0) return rc;
    // the skip's bilinear adjoint: the resize backward's gather on the column slice [Cx, Cx + Cs)
    return mtp_resize_bilinear_bwd(dy + Cx, MTP_F32, lddy, dskip, ldds, N, hs, ws, 2 * h, 2 * w, Cs, accumulate, stream);
}
