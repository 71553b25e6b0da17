// The flat-buffer optimizer step (gfx950): clearing of the accumulating gradient runs, the squared gradient norm, AdamW with gradient
// clipping over the flat f32 buffers, the GEMM-side weight images, and the fused form that makes the images from the registers of the update.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ optimizer
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, float* __restrict__ out, int64_t n) {
    __shared__ float red[4];
    float s = 0.f;
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = load4(g + 4 * i);
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float v = g[(n4 << 2) + threadIdx.x];
        s += v * v;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// the factor every gradient element is multiplied by: grad_scale, times the clip_grad_norm_ coefficient min(1, max_norm / (norm + 1e-6)) when the squared
// norm of the unscaled gradients is given
__device__ __forceinline__ float clipped_grad_scale(const float* __restrict__ sqnorm, float max_norm, float grad_scale) {
    float gs = grad_scale;
    if (sqnorm) {
        const float total = sqrtf(*sqnorm) * grad_scale;
        const float coef = max_norm / (total + 1e-6f);
        gs *= coef < 1.0f ? coef : 1.0f;
    }
    return gs;
}

// the AdamW update of one element (torch.optim.AdamW semantics, MAIN:424-457): step = lr / bias_correction1, rbc2 = 1 / sqrt(bias_correction2)
__device__ __forceinline__ void adamw_elem(float& P, float G, float& M, float& V, float gs, float decay, float b1, float b2, float step, float rbc2, float eps) {
    const float ge = G * gs;
    P *= decay;
    M = b1 * M + (1.0f - b1) * ge;
    V = b2 * V + (1.0f - b2) * ge * ge;
    P -= step * M / (sqrtf(V) * rbc2 + eps);
}

// AdamW over a flat buffer; segments start at multiples of 4 elements.
// (round 5: nontemporal loads / stores on all seven streams: 1660 -> 1603 us alone, no difference in the step -- profiles/r05_ab_late_adamw_nontemporal.txt; not kept)
// kLr: layer-wise lr decay -- segment s trains at lr = hyper[0] * seg_lr[s] (torch.optim.AdamW with a per-group lr); without it the
// code is the plain one (no seg_lr load, no multiply).
template <bool kLr>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   const int64_t* __restrict__ seg_start, const float* __restrict__ seg_wd, const float* __restrict__ seg_lr, int nseg,
                                                   const float* __restrict__ hyper, const float* __restrict__ sqnorm, float max_norm, float grad_scale) {
    const float lr0 = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], bc1 = hyper[4], bc2 = hyper[5];
    const float gs = clipped_grad_scale(sqnorm, max_norm, grad_scale);
    const float rbc2 = rsqrtf(bc2), step0 = lr0 / bc1;
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        int lo = 0, hi = nseg - 1;   // last segment with start <= 4*i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (seg_start[mid] <= 4 * i) lo = mid; else hi = mid - 1;
        }
        const float lr = kLr ? lr0 * seg_lr[lo] : lr0, step = kLr ? lr / bc1 : step0;
        const float decay = 1.0f - lr * seg_wd[lo];
        float4 pv = load4(p + 4 * i), gv = load4(g + 4 * i), mv = load4(m + 4 * i), vv = load4(v + 4 * i);
        float P[4] = {pv.x, pv.y, pv.z, pv.w}, G[4] = {gv.x, gv.y, gv.z, gv.w}, M[4] = {mv.x, mv.y, mv.z, mv.w}, V[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) adamw_elem(P[e], G[e], M[e], V[e], gs, decay, b1, b2, step, rbc2, eps);
        store4(p + 4 * i, make_float4(P[0], P[1], P[2], P[3]));
        store4(m + 4 * i, make_float4(M[0], M[1], M[2], M[3]));
        store4(v + 4 * i, make_float4(V[0], V[1], V[2], V[3]));
    }
}

// ---- the weight-image tiles (mtp_wimg_desc): workgroup = one 64 x 64 tile of one matrix, written row-major (d.w) and transposed (d.wt) in the activation
// dtype T, or in f32 where the descriptor says so.  weight_images_kernel and adamw_images_kernel differ in where a tile's values come from, not in how they
// are written: the helpers below are the one writer of both.
struct WimgTile {
    mtp_wimg_desc d;
    int index;            // of the descriptor in the table
    int64_t r0, c0;       // origin of the tile in the matrix
};
__device__ __forceinline__ WimgTile find_wimg_tile(const mtp_wimg_desc* __restrict__ descs, int n) {
    const int64_t tl = blockIdx.x;
    int lo = 0, hi = n - 1;   // last descriptor with tile0 <= tl (uniform over the workgroup: scalar loads)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].tile0 <= tl) lo = mid; else hi = mid - 1;
    }
    WimgTile t;
    t.d = descs[lo];
    t.index = lo;
    const int64_t local = tl - t.d.tile0, tc = (t.d.C + 63) / 64;
    t.r0 = (local / tc) * 64;
    t.c0 = (local % tc) * 64;
    return t;
}
// C (and R, where there is a transposed image) must be a multiple of am + 1 for the 16-byte image stores: 4 floats or 8 bf16 per lane
template <typename T>
__device__ __forceinline__ int wimg_align_mask(const mtp_wimg_desc& d) {
    return (d.f32_out != 0 || sizeof(T) == 4) ? 3 : 7;
}
// odd-sized (tiny) matrices, element-wise: value v of (r, c) into both images
template <typename T>
__device__ __forceinline__ void wimg_store_elem(const mtp_wimg_desc& d, int64_t r, int64_t c, float v) {
    const bool f32o = d.f32_out != 0;
    if (d.w) { if (f32o) reinterpret_cast<float*>(d.w)[r * d.C + c] = v; else Elem<T>::store(reinterpret_cast<T*>(d.w) + r * d.C + c, v); }
    if (d.wt) { if (f32o) reinterpret_cast<float*>(d.wt)[c * d.R + r] = v; else Elem<T>::store(reinterpret_cast<T*>(d.wt) + c * d.R + r, v); }
}
// vector path (round 5): a lane owns 8 consecutive columns of two rows (32 apart), so a row of the tile is ONE 128-byte (bf16) line written by 8 lanes of one
// instruction -- and likewise a row of the transposed tile.  (Rounds 1-4: 16 columns per lane as four 8-byte bf16 stores 32 bytes apart: every line of
// both images was assembled from four partial writes -- 1.26 x the algorithmic bytes at the L2 boundary, 0.51 of the HBM peak.)
// The lane's 8 columns c .. c + 7 of row rr into the row-major image: ok = (rr, c) is inside the matrix, ok2 = columns c + 4 .. c + 7 are too (C % 4 == 0).
template <typename T>
__device__ __forceinline__ void wimg_store_row8(const mtp_wimg_desc& d, int64_t rr, int64_t c, const float (&x)[8], bool ok, bool ok2) {
    const bool f32o = d.f32_out != 0;
    if (ok && d.w) {
        if (ok2) {
            if (f32o) store8(reinterpret_cast<float*>(d.w) + rr * d.C + c, x);
            else store8(reinterpret_cast<T*>(d.w) + rr * d.C + c, x);
        } else {
            if (f32o) store4(reinterpret_cast<float*>(d.w) + rr * d.C + c, make_float4(x[0], x[1], x[2], x[3]));
            else store4(reinterpret_cast<T*>(d.w) + rr * d.C + c, make_float4(x[0], x[1], x[2], x[3]));
        }
    }
}
// The transposed image of the tile, through LDS: x[h] = the lane's 8 columns of row ra + 32 h (zeros outside the matrix); called by the whole workgroup.
template <typename T>
__device__ __forceinline__ void wimg_store_transposed(const WimgTile& tl, float (&tile)[64][65], const float (&x)[2][8]) {
    const mtp_wimg_desc& d = tl.d;
    const bool f32o = d.f32_out != 0;
    const int t = threadIdx.x, ra = t >> 3, cg = (t & 7) * 8;
    if (d.wt) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 8; ++e) tile[cg + e][ra + 32 * h] = x[h][e];      // bank = cg + e + ra (+ 32 h): distinct over the 64 lanes
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int cl = ra + 32 * h;                   // source column = image row
            const int64_t c = tl.c0 + cl, rr = tl.r0 + cg;
            if (c < d.C && rr < d.R) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = tile[cl][cg + e];
                if (rr + 4 < d.R) {
                    if (f32o) store8(reinterpret_cast<float*>(d.wt) + c * d.R + rr, o);
                    else store8(reinterpret_cast<T*>(d.wt) + c * d.R + rr, o);
                } else {                                  // (R % 4 == 0)
                    if (f32o) store4(reinterpret_cast<float*>(d.wt) + c * d.R + rr, make_float4(o[0], o[1], o[2], o[3]));
                    else store4(reinterpret_cast<T*>(d.wt) + c * d.R + rr, make_float4(o[0], o[1], o[2], o[3]));
                }
            }
        }
    }
}

}  // namespace

// ---- every weight image of the model in one launch (descriptor table in HBM)
template <typename T>
__global__ __launch_bounds__(256) void weight_images_kernel(const mtp_wimg_desc* __restrict__ descs, int n) {
    __shared__ float tile[64][65];
    const WimgTile tl = find_wimg_tile(descs, n);
    const mtp_wimg_desc& d = tl.d;
    const int64_t r0 = tl.r0, c0 = tl.c0;
    const int t = threadIdx.x;
    const int am = wimg_align_mask<T>(d);
    if ((d.C & am) || (d.wt && (d.R & am))) {   // odd-sized (tiny) matrices: element-wise
        const int a = t >> 2, g = (t & 3) * 16;
        const int64_t r = r0 + a;
        for (int e = 0; e < 16; ++e) {
            const int64_t c = c0 + g + e;
            if (r < d.R && c < d.C) wimg_store_elem<T>(d, r, c, d.src[r * d.C + c]);
        }
        return;
    }
    const int ra = t >> 3, cg = (t & 7) * 8;
    float x[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t rr = r0 + ra + 32 * h, c = c0 + cg;
        const bool ok = rr < d.R && c < d.C;         // (C % 4 == 0: columns c .. c + 3 are in range; c + 4 .. c + 7 checked separately)
        const bool ok2 = ok && c + 4 < d.C;
        const float4 v0 = ok ? load4(d.src + rr * d.C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 v1 = ok2 ? load4(d.src + rr * d.C + c + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        x[h][0] = v0.x; x[h][1] = v0.y; x[h][2] = v0.z; x[h][3] = v0.w; x[h][4] = v1.x; x[h][5] = v1.y; x[h][6] = v1.z; x[h][7] = v1.w;
        wimg_store_row8<T>(d, rr, c, x[h], ok, ok2);
    }
    wimg_store_transposed<T>(tl, tile, x);
}

// ---- AdamW of the whole flat buffer AND every GEMM-side weight image in one launch (round 6): the update of a 64 x 64 tile of a parameter matrix is followed, from
// the same registers, by the tile's bf16 row-major image and (through LDS) its transpose.  The separate pass (weight_images_kernel) read every f32 master once more:
// 4 of its 8 bytes per GEMM weight, 1.2 GB per ViT-L step.  Descriptors as for mtp_weight_images, one per parameter of the flat buffers (1-D parameters as rows of 64
// with no images), `src` = the parameter inside the flat data buffer, `wd` = its weight decay; g / m / v live at the same offset of their flat buffers.
// kLr: layer-wise lr decay -- descriptor d trains at lr = hyper[0] * desc_lr[d] (one scalar load per workgroup; a table of its own, so mtp_wimg_desc keeps its layout)
template <typename T, bool kLr>
__global__ __launch_bounds__(256) void adamw_images_kernel(const mtp_wimg_desc* __restrict__ descs, const float* __restrict__ desc_lr, int n, const float* __restrict__ p_base,
                                                          const float* __restrict__ g_base, float* __restrict__ m_base, float* __restrict__ v_base, const float* __restrict__ hyper,
                                                          const float* __restrict__ sqnorm, float max_norm, float grad_scale) {
    __shared__ float tile[64][65];
    const WimgTile tl = find_wimg_tile(descs, n);
    const mtp_wimg_desc& d = tl.d;
    const float lr = kLr ? hyper[0] * desc_lr[tl.index] : hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], bc1 = hyper[4], bc2 = hyper[5];
    const float gs = clipped_grad_scale(sqnorm, max_norm, grad_scale);
    const float rbc2 = rsqrtf(bc2), step = lr / bc1, decay = 1.0f - lr * d.wd;
    float* __restrict__ P = const_cast<float*>(d.src);
    const int64_t off = d.src - p_base;
    const float* __restrict__ G = g_base + off;
    float* __restrict__ M = m_base + off;
    float* __restrict__ V = v_base + off;
    const int64_t r0 = tl.r0, c0 = tl.c0;
    const int t = threadIdx.x;
    const int am = wimg_align_mask<T>(d);
    // stricter than weight_images_kernel's condition: the 16-byte loads and stores of P / G / M / V need C % 4 == 0 with or without images
    if ((d.C & 3) || ((d.w || d.wt) && (d.C & am)) || (d.wt && (d.R & am))) {   // odd-sized (tiny) matrices: element-wise
        const int a = t >> 2, g = (t & 3) * 16;
        const int64_t r = r0 + a;
        for (int e = 0; e < 16; ++e) {
            const int64_t c = c0 + g + e;
            if (r < d.R && c < d.C) {
                const int64_t i = r * d.C + c;
                float pv = P[i], mv = M[i], vv = V[i];
                adamw_elem(pv, G[i], mv, vv, gs, decay, b1, b2, step, rbc2, eps);
                P[i] = pv; M[i] = mv; V[i] = vv;
                wimg_store_elem<T>(d, r, c, pv);
            }
        }
        return;
    }
    const int ra = t >> 3, cg = (t & 7) * 8;
    float x[2][8];
    float4 pv[2][2], gv[2][2], mv[2][2], vv[2][2];
    bool okv[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {      // all 16 loads of the lane in flight before the first use
        const int64_t rr = r0 + ra + 32 * h, c = c0 + cg;
        okv[h][0] = rr < d.R && c < d.C;         // (C % 4 == 0: columns c .. c + 3 are in range; c + 4 .. c + 7 checked separately)
        okv[h][1] = okv[h][0] && c + 4 < d.C;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t i = okv[h][q] ? rr * d.C + c + 4 * q : 0;
            pv[h][q] = load4(P + i); gv[h][q] = load4(G + i); mv[h][q] = load4(M + i); vv[h][q] = load4(V + i);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t rr = r0 + ra + 32 * h, c = c0 + cg;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float Pq[4] = {pv[h][q].x, pv[h][q].y, pv[h][q].z, pv[h][q].w}, Mq[4] = {mv[h][q].x, mv[h][q].y, mv[h][q].z, mv[h][q].w};
            float Vq[4] = {vv[h][q].x, vv[h][q].y, vv[h][q].z, vv[h][q].w};
            const float Gq[4] = {gv[h][q].x, gv[h][q].y, gv[h][q].z, gv[h][q].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) adamw_elem(Pq[e], Gq[e], Mq[e], Vq[e], gs, decay, b1, b2, step, rbc2, eps);
            if (okv[h][q]) {
                const int64_t i = rr * d.C + c + 4 * q;
                store4(P + i, make_float4(Pq[0], Pq[1], Pq[2], Pq[3]));
                store4(M + i, make_float4(Mq[0], Mq[1], Mq[2], Mq[3]));
                store4(V + i, make_float4(Vq[0], Vq[1], Vq[2], Vq[3]));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) x[h][4 * q + e] = okv[h][q] ? Pq[e] : 0.f;
        }
        wimg_store_row8<T>(d, rr, c, x[h], okv[h][0], okv[h][1]);
    }
    wimg_store_transposed<T>(tl, tile, x);
}

// One launcher per kernel family: the layer-wise lr decay form (kLr) is selected by the presence of the lr table, so a run without it launches the plain code.
static int launch_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const float* seg_wd, const float* seg_lr, int nseg,
                             const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream) {
    if (!p || !g || !m || !v || n <= 0 || (n % 4) || !seg_start || !seg_wd || nseg <= 0 || !hyper) return MTP_ERR_ARG;
    const dim3 grid(blocks_for(n / 4, kThreads, 8192)), block(kThreads);
    if (seg_lr)
        adamw_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(p, g, m, v, n, seg_start, seg_wd, seg_lr, nseg, hyper, sqnorm, max_norm, grad_scale);
    else
        adamw_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(p, g, m, v, n, seg_start, seg_wd, seg_lr, nseg, hyper, sqnorm, max_norm, grad_scale);
    return mtp_launch_status();
}

static int launch_adamw_images(const mtp_wimg_desc* descs_dev, const float* desc_lr, int n, int64_t total_tiles, int act_dtype, float* p_base, const float* g_base,
                               float* m_base, float* v_base, const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream) {
    if (!descs_dev || n <= 0 || total_tiles <= 0 || total_tiles > INT32_MAX || !p_base || !g_base || !m_base || !v_base || !hyper) return MTP_ERR_ARG;
    return for_act(act_dtype, [&](auto t) {
        using T = decltype(t);
        auto launch = [&](auto kernel) {
            kernel<<<(unsigned)total_tiles, kThreads, 0, (hipStream_t)stream>>>(descs_dev, desc_lr, n, p_base, g_base, m_base, v_base, hyper, sqnorm, max_norm, grad_scale);
        };
        if (desc_lr) launch(adamw_images_kernel<T, true>);
        else launch(adamw_images_kernel<T, false>);
    });
}

extern "C" int mtp_adamw_weight_images(const mtp_wimg_desc* descs_dev, int n, int64_t total_tiles, int act_dtype, float* p_base, const float* g_base, float* m_base,
                                       float* v_base, const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream) {
    return launch_adamw_images(descs_dev, nullptr, n, total_tiles, act_dtype, p_base, g_base, m_base, v_base, hyper, sqnorm, max_norm, grad_scale, stream);
}

extern "C" int mtp_adamw_weight_images_lr(const mtp_wimg_desc* descs_dev, const float* desc_lr, int n, int64_t total_tiles, int act_dtype, float* p_base,
                                          const float* g_base, float* m_base, float* v_base, const float* hyper, const float* sqnorm, float max_norm, float grad_scale,
                                          mtp_stream_t stream) {
    if (!desc_lr) return MTP_ERR_ARG;
    return launch_adamw_images(descs_dev, desc_lr, n, total_tiles, act_dtype, p_base, g_base, m_base, v_base, hyper, sqnorm, max_norm, grad_scale, stream);
}

extern "C" int mtp_weight_images(const mtp_wimg_desc* descs_dev, int n, int64_t total_tiles, int act_dtype, mtp_stream_t stream) {
    if (!descs_dev || n <= 0 || total_tiles <= 0 || total_tiles > INT32_MAX) return MTP_ERR_ARG;
    return for_act(act_dtype, [&](auto t) { weight_images_kernel<decltype(t)><<<(unsigned)total_tiles, kThreads, 0, (hipStream_t)stream>>>(descs_dev, n); });
}

// base[start[i] .. start[i] + count[i]) = 0 for n segments (device tables; the host splits long runs so that one workgroup clears at
// most 64 K floats): the gradients that ACCUMULATE (biases, LayerNorm, rel-pos tables, sampling heads, FPN) inside the flat gradient
// buffer, without touching the 99 % of it that the weight-gradient GEMMs overwrite
__global__ __launch_bounds__(256) void zero_segments_kernel(float* __restrict__ base, const int64_t* __restrict__ start, const int64_t* __restrict__ count, int n) {
    for (int sgm = blockIdx.x; sgm < n; sgm += gridDim.x) {
        float* p = base + start[sgm];
        const int64_t c = count[sgm];
        for (int64_t i = threadIdx.x; i < c; i += 256) p[i] = 0.f;
    }
}
extern "C" int mtp_zero_segments_f32(float* base, const int64_t* start, const int64_t* count, int n, mtp_stream_t stream) {
    if (!base || !start || !count || n <= 0) return MTP_ERR_ARG;
    zero_segments_kernel<<<dim3((unsigned)(n < 4096 ? n : 4096)), kThreads, 0, (hipStream_t)stream>>>(base, start, count, n);
    return mtp_launch_status();
}

// out += sum of squares over n runs base[start[i] .. start[i] + count[i]) (runs of at most 64 K floats, as mtp_zero_segments_f32): the part of the gradient norm that
// is not a by-product of the weight-gradient launches (biases, LayerNorm, tables, sampling heads, split problems) -- ~3 % of the buffer
__global__ __launch_bounds__(256) void sqnorm_segments_kernel(const float* __restrict__ base, const int64_t* __restrict__ start, const int64_t* __restrict__ count, int n,
                                                              float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int sgm = blockIdx.x; sgm < n; sgm += gridDim.x) {
        const float* p = base + start[sgm];
        const int64_t c = count[sgm];
        if (((start[sgm] | c) & 3) == 0) {      // 16-byte loads (the flat buffers pad every parameter to 64 elements: always, for their tables)
            for (int64_t i = 4 * threadIdx.x; i < c; i += 1024) {
                const float4 v = load4(p + i);
                s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
            }
        } else {
            for (int64_t i = threadIdx.x; i < c; i += 256) {
                const float v = p[i];
                s += v * v;
            }
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}
extern "C" int mtp_sqnorm_segments_f32(const float* base, const int64_t* start, const int64_t* count, int n, float* out, mtp_stream_t stream) {
    if (!base || !start || !count || n <= 0 || !out) return MTP_ERR_ARG;
    sqnorm_segments_kernel<<<dim3((unsigned)(n < 4096 ? n : 4096)), kThreads, 0, (hipStream_t)stream>>>(base, start, count, n, out);
    return mtp_launch_status();
}

extern "C" int mtp_sqnorm_f32(const float* g, float* out, int64_t n, mtp_stream_t stream) {
    if (!g || !out || n <= 0) return MTP_ERR_ARG;
    sqnorm_kernel<<<blocks_for(n / 4 + 1, kThreads, 2048), kThreads, 0, (hipStream_t)stream>>>(g, out, n);
    return mtp_launch_status();
}

extern "C" int mtp_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const float* seg_wd, int nseg,
                              const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream) {
    return launch_adamw_flat(p, g, m, v, n, seg_start, seg_wd, nullptr, nseg, hyper, sqnorm, max_norm, grad_scale, stream);
}

extern "C" int mtp_adamw_flat_lr(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const float* seg_wd, const float* seg_lr,
                                 int nseg, const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream) {
    if (!seg_lr) return MTP_ERR_ARG;
    return launch_adamw_flat(p, g, m, v, n, seg_start, seg_wd, seg_lr, nseg, hyper, sqnorm, max_norm, grad_scale, stream);
}
