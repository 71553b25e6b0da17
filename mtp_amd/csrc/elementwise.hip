// HBM-bound layout / elementwise kernels of the backbone path (gfx950): im2col for the patch embedding, dtype
// casts and weight (re)packing, token-major <-> NCHW feature-map transposes (FPN tail), MaxPool2d(2,2), axpy, segment copies
// and the drop-path-scaled operand copy.  All accesses are 8/16-byte vectors on the contiguous dimension; transposes go through a
// padded LDS tile so both sides stay coalesced.  (The optimizer: optimizer.hip; the RVSA sampling heads: rvsa_sampling.hip.)
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ patchify
// cols[t][c*P*P + ky*P + kx] = img[b][c][py*P+ky][px*P+kx], t = (b*Hp + py)*Wp + px   (VIT:529,536-539)
template <typename T, bool INVERSE>
__global__ __launch_bounds__(256) void patchify_kernel(float* __restrict__ img, T* __restrict__ cols, int B, int Cin, int H, int W, int P, int Hp, int Wp) {
    const int K4 = Cin * P * P / 4, P4 = P / 4;
    const int64_t total = (int64_t)B * Hp * Wp * K4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k4 = (int)(i % K4);
        const int64_t t = i / K4;
        const int kx4 = k4 % P4, ky = (k4 / P4) % P, c = k4 / (P4 * P);
        const int px = (int)(t % Wp), py = (int)((t / Wp) % Hp), b = (int)(t / ((int64_t)Wp * Hp));
        float* ip = img + (((int64_t)b * Cin + c) * H + py * P + ky) * W + px * P + kx4 * 4;
        T* cp = cols + t * (K4 * 4) + k4 * 4;
        if (INVERSE)
            *reinterpret_cast<float4*>(ip) = load4(cp);
        else
            store4(cp, *reinterpret_cast<const float4*>(ip));
    }
}

// ------------------------------------------------------------------------------------------------ cast
template <typename Ts, typename Td>
__global__ __launch_bounds__(256) void cast_kernel(const Ts* __restrict__ s, Td* __restrict__ d, int64_t n) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) store4(d + 4 * i, load4(s + 4 * i));
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) Elem<Td>::store(d + (n4 << 2) + threadIdx.x, Elem<Ts>::load(s + (n4 << 2) + threadIdx.x));
}

// ------------------------------------------------------------------------------------------------ tiled transposes
// Generic 64x64 tile through LDS.  "row side": rows (length-C vectors, C contiguous);  "col side": (C, S) with S contiguous.
//   ROWS2COLS: out[bt][c][s] = in[bt][rowmap(s)][c]      (tokens -> NCHW; weight transpose with rowmap = identity)
//   else     : out[bt][rowmap(s)][c] = in[bt][c][s]      (NCHW -> tokens)
// rowmap(s): pixel s = (y, x) of the (Hp<<L, Wp<<L) map -> row ((py*Wp+px)*4 + q1)*4 + q2 ..., q_l = ky_l*2 + kx_l.
__device__ __forceinline__ int64_t pixel_to_row(int64_t s, int Wp, int L) {
    if (L == 0) return s;
    const int Wo = Wp << L;
    const int y = (int)(s / Wo), x = (int)(s % Wo);
    int64_t r = (int64_t)(y >> L) * Wp + (x >> L);
    for (int l = 1; l <= L; ++l) r = r * 4 + (((y >> (L - l)) & 1) << 1) + ((x >> (L - l)) & 1);
    return r;
}

template <typename Tin, typename Tout, bool ROWS2COLS>
__global__ __launch_bounds__(256) void transpose_kernel(const Tin* __restrict__ in, Tout* __restrict__ out, int64_t S, int64_t C, int Wp, int L) {
    __shared__ float tile[64][65];
    const int64_t bt = blockIdx.z;
    const int64_t s0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
    const Tin* ib = in + bt * S * C;
    Tout* ob = out + bt * S * C;
    const int t = threadIdx.x;
    const int a = t >> 2, g = (t & 3) * 16;   // a: index on the "slow" side of this phase, g: 16 contiguous elements
    if (ROWS2COLS) {
        // read rows: row s0+a, channels c0+g..g+15
        const int64_t s = s0 + a;
        if (s < S) {
            const Tin* rp = ib + pixel_to_row(s, Wp, L) * C + c0 + g;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (c0 + g + 4 * v < C) {
                    const float4 x = load4(rp + 4 * v);
                    tile[g + 4 * v + 0][a] = x.x; tile[g + 4 * v + 1][a] = x.y; tile[g + 4 * v + 2][a] = x.z; tile[g + 4 * v + 3][a] = x.w;
                }
            }
        }
        __syncthreads();
        // write cols: channel c0+a, positions s0+g..g+15
        const int64_t c = c0 + a;
        if (c < C) {
            Tout* wp = ob + c * S + s0 + g;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t s2 = s0 + g + 4 * v;
                if (s2 + 3 < S && (S & 3) == 0) {
                    store4(wp + 4 * v, make_float4(tile[a][g + 4 * v], tile[a][g + 4 * v + 1], tile[a][g + 4 * v + 2], tile[a][g + 4 * v + 3]));
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (s2 + e < S) Elem<Tout>::store(wp + 4 * v + e, tile[a][g + 4 * v + e]);
                }
            }
        }
    } else {
        const int64_t c = c0 + a;
        if (c < C) {
            const Tin* rp = ib + c * S + s0 + g;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t s2 = s0 + g + 4 * v;
                if (s2 + 3 < S && (S & 3) == 0) {
                    const float4 x = load4(rp + 4 * v);
                    tile[a][g + 4 * v] = x.x; tile[a][g + 4 * v + 1] = x.y; tile[a][g + 4 * v + 2] = x.z; tile[a][g + 4 * v + 3] = x.w;
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (s2 + e < S) tile[a][g + 4 * v + e] = Elem<Tin>::load(rp + 4 * v + e);
                }
            }
        }
        __syncthreads();
        const int64_t s = s0 + a;
        if (s < S) {
            Tout* wp = ob + pixel_to_row(s, Wp, L) * C + c0 + g;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (c0 + g + 4 * v < C)
                    store4(wp + 4 * v, make_float4(tile[g + 4 * v][a], tile[g + 4 * v + 1][a], tile[g + 4 * v + 2][a], tile[g + 4 * v + 3][a]));
        }
    }
}

// bf16 -> bf16 with S % 8 == 0 and C % 8 == 0 (round 5): a lane owns 8 consecutive elements (16 bytes) of two tile rows 32 apart, so every 128-byte line of the
// tile is read / written by 8 lanes of ONE instruction.  (The generic kernel above gives a lane 16 elements as four 8-byte pieces 32 bytes apart: each line is
// assembled from four partial accesses -- the same pattern cost weight_images_kernel a third of its time.)
template <bool ROWS2COLS>
__global__ __launch_bounds__(256) void transpose8_bf16_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int64_t S, int64_t C, int Wp, int L) {
    __shared__ float tile[64][65];      // [channel][position]
    const int64_t bt = blockIdx.z;
    const int64_t s0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
    const bf16_t* ib = in + bt * S * C;
    bf16_t* ob = out + bt * S * C;
    const int t = threadIdx.x, ra = t >> 3, cg = (t & 7) * 8;
    float x[8];
    if (ROWS2COLS) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t sp = s0 + ra + 32 * h;
            if (sp < S && c0 + cg < C) {
                load8(ib + pixel_to_row(sp, Wp, L) * C + c0 + cg, x);
#pragma unroll
                for (int e = 0; e < 8; ++e) tile[cg + e][ra + 32 * h] = x[e];      // bank = cg + e + ra (+ 32 h): distinct over a wave
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t c = c0 + ra + 32 * h;
            if (c < C && s0 + cg < S) {
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = tile[ra + 32 * h][cg + e];
                store8(ob + c * S + s0 + cg, x);
            }
        }
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t c = c0 + ra + 32 * h;
            if (c < C && s0 + cg < S) {
                load8(ib + c * S + s0 + cg, x);
#pragma unroll
                for (int e = 0; e < 8; ++e) tile[ra + 32 * h][cg + e] = x[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t sp = s0 + ra + 32 * h;
            if (sp < S && c0 + cg < C) {
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = tile[cg + e][ra + 32 * h];
                store8(ob + pixel_to_row(sp, Wp, L) * C + c0 + cg, x);
            }
        }
    }
}

template <bool ROWS2COLS>
int launch_transpose(const void* in, int in_dt, void* out, int out_dt, int64_t batches, int64_t S, int64_t C, int Wp, int L, hipStream_t s) {
    if (C % 4) return MTP_ERR_ARG;
    dim3 grid((unsigned)((S + 63) / 64), (unsigned)((C + 63) / 64), (unsigned)batches), block(256);
    if (in_dt == MTP_BF16 && out_dt == MTP_BF16 && !(S & 7) && !(C & 7) && !(((uintptr_t)in | (uintptr_t)out) & 15)) {
        transpose8_bf16_kernel<ROWS2COLS><<<grid, block, 0, s>>>((const bf16_t*)in, (bf16_t*)out, S, C, Wp, L);
        return mtp_launch_status();
    }
    MTP_DISPATCH2(in_dt, out_dt, transpose_kernel<TA, TB, ROWS2COLS><<<grid, block, 0, s>>>((const TA*)in, (TB*)out, S, C, Wp, L));
    return mtp_launch_status();
}

// ------------------------------------------------------------------------------------------------ ConvTranspose2d weight packing
// w (Cin, Cout, 2, 2) -> wg[(q*Cout + co)][ci], wgT[ci][q*Cout + co], q = ky*2+kx
template <typename T>
__global__ __launch_bounds__(256) void convt_pack_kernel(const float* __restrict__ w, T* __restrict__ wg, T* __restrict__ wgT, int64_t Cin, int64_t Cout) {
    const int64_t total = Cin * Cout * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int q = (int)(i & 3);
        const int64_t co = (i >> 2) % Cout, ci = (i >> 2) / Cout;
        const float v = w[i];
        if (wg) Elem<T>::store(wg + (q * Cout + co) * Cin + ci, v);
        if (wgT) Elem<T>::store(wgT + ci * (4 * Cout) + q * Cout + co, v);
    }
}
__global__ __launch_bounds__(256) void convt_unpack_kernel(const float* __restrict__ dwg, float* __restrict__ dw, int64_t Cin, int64_t Cout) {
    const int64_t total = Cin * Cout * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int q = (int)(i & 3);
        const int64_t co = (i >> 2) % Cout, ci = (i >> 2) / Cout;
        dw[i] = dwg[(q * Cout + co) * Cin + ci];
    }
}

// The same two packings through a (64 ci) x (64 co) tile in LDS, two taps at a time (round 5): every global access is a whole line -- the float4 of the four taps
// of (ci, co) on the parameter side (1 KiB per wave instruction), 8 lanes x 16 bytes per row of the images.  (The element-wise kernels above write 2-byte pieces
// scattered over the images: 31 us for a 1024 x 1024 weight.)  Cin, Cout multiples of 8.
template <typename T>
__global__ __launch_bounds__(256) void convt_pack_tiled_kernel(const float* __restrict__ w, T* __restrict__ wg, T* __restrict__ wgT, int Cin, int Cout) {
    __shared__ float tile[2][64][65];      // [tap of the pair][ci][co]
    const int ci0 = blockIdx.y * 64, co0 = blockIdx.x * 64;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, ra = t >> 3, cg = (t & 7) * 8;
    float4 v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int ci = ci0 + wave + 4 * k, co = co0 + lane;
        v[k] = (ci < Cin && co < Cout) ? load4(w + ((int64_t)ci * Cout + co) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half) __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            tile[0][wave + 4 * k][lane] = half ? v[k].z : v[k].x;
            tile[1][wave + 4 * k][lane] = half ? v[k].w : v[k].y;
        }
        __syncthreads();
        float o[8];
        if (wgT) {         // wgT[ci][q * Cout + co]: a line = (ci, q), 64 co
            for (int l = ra; l < 128; l += 32) {
                const int r = l >> 1, qq = l & 1, ci = ci0 + r;
                if (ci < Cin && co0 + cg < Cout) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = tile[qq][r][cg + e];
                    store8(wgT + (int64_t)ci * 4 * Cout + (int64_t)(2 * half + qq) * Cout + co0 + cg, o);
                }
            }
        }
        if (wg) {          // wg[q * Cout + co][ci]: a line = (q, co), 64 ci
            for (int l = ra; l < 128; l += 32) {
                const int qq = l >> 6, c = l & 63, co = co0 + c;
                if (co < Cout && ci0 + cg < Cin) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = tile[qq][cg + e][c];
                    store8(wg + ((int64_t)(2 * half + qq) * Cout + co) * Cin + ci0 + cg, o);
                }
            }
        }
    }
}
// dw[ci][co][q] = dwg[q * Cout + co][ci]
__global__ __launch_bounds__(256) void convt_unpack_tiled_kernel(const float* __restrict__ dwg, float* __restrict__ dw, int Cin, int Cout) {
    __shared__ float tile[2][64][65];      // [tap of the pair][ci][co]
    const int ci0 = blockIdx.y * 64, co0 = blockIdx.x * 64;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, rb = t >> 4, c4 = (t & 15) * 4;
    float g[16][4];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half) __syncthreads();
        for (int l = rb; l < 128; l += 16) {       // a line = (q, co): 64 ci = 16 lanes x 16 bytes
            const int qq = l >> 6, c = l & 63, co = co0 + c;
            if (co < Cout && ci0 + c4 < Cin) {
                const float4 x = load4(dwg + ((int64_t)(2 * half + qq) * Cout + co) * Cin + ci0 + c4);
                tile[qq][c4 + 0][c] = x.x; tile[qq][c4 + 1][c] = x.y; tile[qq][c4 + 2][c] = x.z; tile[qq][c4 + 3][c] = x.w;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            g[k][2 * half] = tile[0][wave + 4 * k][lane];
            g[k][2 * half + 1] = tile[1][wave + 4 * k][lane];
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int ci = ci0 + wave + 4 * k, co = co0 + lane;
        if (ci < Cin && co < Cout) store4(dw + ((int64_t)ci * Cout + co) * 4, make_float4(g[k][0], g[k][1], g[k][2], g[k][3]));
    }
}

// ------------------------------------------------------------------------------------------------ MaxPool2d(2,2) on tokens
template <typename Tout>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, Tout* __restrict__ y, int B, int Hp, int Wp, int C) {
    const int Ho = Hp / 2, Wo = Wp / 2, C4 = C / 4;
    const int64_t total = (int64_t)B * Ho * Wo * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        const int64_t o = i / C4;
        const int xo = (int)(o % Wo), yo = (int)((o / Wo) % Ho), b = (int)(o / ((int64_t)Wo * Ho));
        const float* p = x + (((int64_t)b * Hp + 2 * yo) * Wp + 2 * xo) * C + 4 * c4;
        const float4 a = load4(p), bb = load4(p + C), c = load4(p + (int64_t)Wp * C), d = load4(p + (int64_t)Wp * C + C);
        store4(y + o * C + 4 * c4, make_float4(fmaxf(fmaxf(a.x, bb.x), fmaxf(c.x, d.x)), fmaxf(fmaxf(a.y, bb.y), fmaxf(c.y, d.y)),
                                              fmaxf(fmaxf(a.z, bb.z), fmaxf(c.z, d.z)), fmaxf(fmaxf(a.w, bb.w), fmaxf(c.w, d.w))));
    }
}
// dx[token] (+)= dy[window] where token is the FIRST maximum of its 2x2 window in scan order (torch's tie rule)
template <typename Tdy>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ x, const Tdy* __restrict__ dy, float* __restrict__ dx, int accumulate,
                                                         int B, int Hp, int Wp, int C) {
    const int Ho = Hp / 2, Wo = Wp / 2, C4 = C / 4;
    const int64_t total = (int64_t)B * Hp * Wp * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        const int64_t t = i / C4;
        const int xx = (int)(t % Wp), yy = (int)((t / Wp) % Hp), b = (int)(t / ((int64_t)Wp * Hp));
        float4 g = make_float4(0, 0, 0, 0);
        if (yy < 2 * Ho && xx < 2 * Wo) {
            const int yo = yy >> 1, xo = xx >> 1, me = ((yy & 1) << 1) | (xx & 1);
            const float* p = x + (((int64_t)b * Hp + 2 * yo) * Wp + 2 * xo) * C + 4 * c4;
            float v[4][4];
            const float4 q0 = load4(p), q1 = load4(p + C), q2 = load4(p + (int64_t)Wp * C), q3 = load4(p + (int64_t)Wp * C + C);
            v[0][0] = q0.x; v[0][1] = q0.y; v[0][2] = q0.z; v[0][3] = q0.w;
            v[1][0] = q1.x; v[1][1] = q1.y; v[1][2] = q1.z; v[1][3] = q1.w;
            v[2][0] = q2.x; v[2][1] = q2.y; v[2][2] = q2.z; v[2][3] = q2.w;
            v[3][0] = q3.x; v[3][1] = q3.y; v[3][2] = q3.z; v[3][3] = q3.w;
            const float4 d = load4(dy + (((int64_t)b * Ho + yo) * Wo + xo) * C + 4 * c4);
            const float dd[4] = {d.x, d.y, d.z, d.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int arg = 0;
                float m = v[0][e];
#pragma unroll
                for (int k = 1; k < 4; ++k)
                    if (v[k][e] > m) { m = v[k][e]; arg = k; }
                o[e] = arg == me ? dd[e] : 0.f;
            }
            g = make_float4(o[0], o[1], o[2], o[3]);
        }
        float* dp = dx + t * C + 4 * c4;
        if (accumulate) {
            const float4 old = load4(dp);
            g.x += old.x; g.y += old.y; g.z += old.z; g.w += old.w;
        }
        store4(dp, g);
    }
}

__global__ __launch_bounds__(256) void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, float alpha, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] += alpha * x[i];
}

}  // namespace

extern "C" int mtp_patchify(const float* img, void* cols, int dtype, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t P, mtp_stream_t stream) {
    if (!img || !cols || B <= 0 || (P % 4) || (W % 4) || H < P || W < P) return MTP_ERR_ARG;
    const int Hp = (int)(H / P), Wp = (int)(W / P);
    const int64_t total = B * Hp * Wp * Cin * P * P / 4;
    return for_act(dtype, [&](auto t) {
        using T = decltype(t);
        patchify_kernel<T, false><<<blocks_for(total, kThreads, 8192), kThreads, 0, (hipStream_t)stream>>>((float*)img, (T*)cols, (int)B, (int)Cin, (int)H, (int)W, (int)P, Hp, Wp);
    });
}

// ---- uint8 HWC image -> normalised patch rows (data preprocessor + im2col in one pass over 1 byte per sample) ------------------
// thread = 4 consecutive pixels of one patch row: 12 input bytes (three aligned dwords when W % 4 == 0), three 4-element
// stores (one per output channel plane of the patch row).  IEEE division, so the f32 result is bit-equal to (x - mean) / std.
struct PreNorm {
    float mean[3], std[3];
};
template <typename T>
__global__ __launch_bounds__(256) void preprocess_patchify_kernel(const uint8_t* __restrict__ img, T* __restrict__ cols, int B, int H, int W, int P, int Hp, int Wp,
                                                                 PreNorm nm, int flip, float pad_value) {
    const int P4 = P / 4, K = 3 * P * P;
    const int64_t total = (int64_t)B * Hp * Wp * P * P4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x4 = (int)(i % P4), ky = (int)((i / P4) % P);
        const int64_t t = i / ((int64_t)P4 * P);
        const int px = (int)(t % Wp), py = (int)((t / Wp) % Hp), b = (int)(t / ((int64_t)Wp * Hp));
        const int y = py * P + ky, x0 = px * P + 4 * x4;
        float v[3][4];
        if (y < H && x0 + 3 < W && (W & 3) == 0) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(img + (((int64_t)b * H + y) * W + x0) * 3);
            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
            const uint32_t byte[12] = {w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, (w1 >> 16) & 255u, w1 >> 24,
                                       w2 & 255u, (w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][j] = ((float)byte[3 * j + (flip ? 2 - c : c)] - nm.mean[c]) / nm.std[c];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = y < H && x0 + j < W;
                const uint8_t* p = img + (((int64_t)b * H + (in ? y : 0)) * W + (in ? x0 + j : 0)) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][j] = in ? ((float)p[flip ? 2 - c : c] - nm.mean[c]) / nm.std[c] : pad_value;
            }
        }
        T* cp = cols + t * K + ky * P + 4 * x4;
#pragma unroll
        for (int c = 0; c < 3; ++c) store4(cp + c * P * P, make_float4(v[c][0], v[c][1], v[c][2], v[c][3]));
    }
}

extern "C" int mtp_preprocess_patchify(const uint8_t* img, void* cols, int dtype, int64_t B, int64_t H, int64_t W, int64_t P, int64_t pad_divisor,
                                       const float* mean, const float* std, int bgr_to_rgb, float pad_value, mtp_stream_t stream) {
    if (!img || !cols || !mean || !std || B <= 0 || H <= 0 || W <= 0 || P <= 0 || (P % 4) || pad_divisor <= 0) return MTP_ERR_ARG;
    const int64_t Hpad = (H + pad_divisor - 1) / pad_divisor * pad_divisor, Wpad = (W + pad_divisor - 1) / pad_divisor * pad_divisor;
    if ((Hpad % P) || (Wpad % P)) return MTP_ERR_ARG;
    PreNorm nm;
    for (int c = 0; c < 3; ++c) {
        if (std[c] == 0.f) return MTP_ERR_ARG;
        nm.mean[c] = mean[c];
        nm.std[c] = std[c];
    }
    const int Hp = (int)(Hpad / P), Wp = (int)(Wpad / P);
    const int64_t total = B * Hp * Wp * P * (P / 4);
    return for_act(dtype, [&](auto t) {
        using T = decltype(t);
        preprocess_patchify_kernel<T><<<blocks_for(total, kThreads, 8192), kThreads, 0, (hipStream_t)stream>>>(img, (T*)cols, (int)B, (int)H, (int)W, (int)P, Hp, Wp, nm, bgr_to_rgb, pad_value);
    });
}

extern "C" int mtp_unpatchify(const void* cols, int dtype, float* dimg, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t P, mtp_stream_t stream) {
    if (!dimg || !cols || B <= 0 || (P % 4) || (W % 4) || H < P || W < P) return MTP_ERR_ARG;
    if (!dt_ok(dtype)) return MTP_ERR_UNSUPPORTED;      // before the memset: a refused call writes nothing
    const int Hp = (int)(H / P), Wp = (int)(W / P);
    hipStream_t s = (hipStream_t)stream;
    if ((H % P) || (W % P)) {
        hipError_t e = hipMemsetAsync(dimg, 0, sizeof(float) * (size_t)(B * Cin * H * W), s);
        if (e != hipSuccess) return (int)e;
    }
    const int64_t total = B * Hp * Wp * Cin * P * P / 4;
    return for_act(dtype, [&](auto t) {
        using T = decltype(t);
        patchify_kernel<T, true><<<blocks_for(total, kThreads, 8192), kThreads, 0, s>>>(dimg, (T*)cols, (int)B, (int)Cin, (int)H, (int)W, (int)P, Hp, Wp);
    });
}

extern "C" int mtp_cast(const void* src, int sd, void* dst, int dd, int64_t n, mtp_stream_t stream) {
    if (!src || !dst || n <= 0) return MTP_ERR_ARG;
    dim3 grid(blocks_for(n / 4 + 1, kThreads, 8192)), block(256);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto ts, auto td) {
        using TS = decltype(ts);
        using TD = decltype(td);
        cast_kernel<TS, TD><<<grid, block, 0, s>>>((const TS*)src, (TD*)dst, n);
    };
    // its own ladder: the two real casts come first in the code object, the two copies after them
    if (sd == MTP_F32 && dd == MTP_BF16) launch(float{}, bf16_t{});
    else if (sd == MTP_BF16 && dd == MTP_F32) launch(bf16_t{}, float{});
    else if (sd == MTP_F32 && dd == MTP_F32) launch(float{}, float{});
    else if (sd == MTP_BF16 && dd == MTP_BF16) launch(bf16_t{}, bf16_t{});
    else return MTP_ERR_UNSUPPORTED;
    return mtp_launch_status();
}

extern "C" int mtp_transpose_cast(const float* src, void* dst, int dst_dtype, int64_t R, int64_t C, mtp_stream_t stream) {
    if (!src || !dst || R <= 0 || C <= 0) return MTP_ERR_ARG;
    // src (R rows of C) is the "row side": out[c][r] = in[r][c]
    return launch_transpose<true>(src, MTP_F32, dst, dst_dtype, 1, R, C, 1, 0, (hipStream_t)stream);
}

extern "C" int mtp_convt_pack(const float* w, void* wg, void* wgT, int dtype, int64_t Cin, int64_t Cout, mtp_stream_t stream) {
    if (!w || Cin <= 0 || Cout <= 0) return MTP_ERR_ARG;
    if (!(Cin & 7) && !(Cout & 7) && Cin < (1 << 20) && Cout < (1 << 20))
        return for_act(dtype, [&](auto t) {
            using T = decltype(t);
            convt_pack_tiled_kernel<T><<<dim3((unsigned)((Cout + 63) / 64), (unsigned)((Cin + 63) / 64)), kThreads, 0, (hipStream_t)stream>>>(w, (T*)wg, (T*)wgT, (int)Cin, (int)Cout);
        });
    return for_act(dtype, [&](auto t) {
        using T = decltype(t);
        convt_pack_kernel<T><<<blocks_for(Cin * Cout * 4, kThreads, 4096), kThreads, 0, (hipStream_t)stream>>>(w, (T*)wg, (T*)wgT, Cin, Cout);
    });
}

extern "C" int mtp_convt_unpack_grad(const float* dwg, float* dw, int64_t Cin, int64_t Cout, mtp_stream_t stream) {
    if (!dwg || !dw || Cin <= 0 || Cout <= 0) return MTP_ERR_ARG;
    if (!(Cin & 7) && !(Cout & 7) && Cin < (1 << 20) && Cout < (1 << 20)) {
        convt_unpack_tiled_kernel<<<dim3((unsigned)((Cout + 63) / 64), (unsigned)((Cin + 63) / 64)), kThreads, 0, (hipStream_t)stream>>>(dwg, dw, (int)Cin, (int)Cout);
        return mtp_launch_status();
    }
    convt_unpack_kernel<<<blocks_for(Cin * Cout * 4, kThreads, 4096), kThreads, 0, (hipStream_t)stream>>>(dwg, dw, Cin, Cout);
    return mtp_launch_status();
}

extern "C" int mtp_tokens_to_nchw(const void* x, int x_dtype, void* out, int out_dtype, int64_t B, int64_t Hp, int64_t Wp, int64_t C, int levels, mtp_stream_t stream) {
    if (!x || !out || B <= 0 || Hp <= 0 || Wp <= 0 || levels < 0 || levels > 4) return MTP_ERR_ARG;
    return launch_transpose<true>(x, x_dtype, out, out_dtype, B, (Hp * Wp) << (2 * levels), C, (int)Wp, levels, (hipStream_t)stream);
}
extern "C" int mtp_nchw_to_tokens(const void* f, int f_dtype, void* out, int out_dtype, int64_t B, int64_t Hp, int64_t Wp, int64_t C, int levels, mtp_stream_t stream) {
    if (!f || !out || B <= 0 || Hp <= 0 || Wp <= 0 || levels < 0 || levels > 4) return MTP_ERR_ARG;
    return launch_transpose<false>(f, f_dtype, out, out_dtype, B, (Hp * Wp) << (2 * levels), C, (int)Wp, levels, (hipStream_t)stream);
}

extern "C" int mtp_maxpool2_tokens_fwd(const float* x, void* y, int y_dtype, int64_t B, int64_t Hp, int64_t Wp, int64_t C, mtp_stream_t stream) {
    if (!x || !y || B <= 0 || Hp < 2 || Wp < 2 || (C % 4)) return MTP_ERR_ARG;
    return for_act(y_dtype, [&](auto t) {
        using T = decltype(t);
        maxpool_fwd_kernel<T><<<blocks_for(B * (Hp / 2) * (Wp / 2) * C / 4, kThreads, 8192), kThreads, 0, (hipStream_t)stream>>>(x, (T*)y, (int)B, (int)Hp, (int)Wp, (int)C);
    });
}
extern "C" int mtp_maxpool2_tokens_bwd(const float* x, const void* dy, int dy_dtype, float* dx, int accumulate, int64_t B, int64_t Hp, int64_t Wp, int64_t C, mtp_stream_t stream) {
    if (!x || !dy || !dx || B <= 0 || Hp < 2 || Wp < 2 || (C % 4)) return MTP_ERR_ARG;
    return for_act(dy_dtype, [&](auto t) {
        using T = decltype(t);
        maxpool_bwd_kernel<T><<<blocks_for(B * Hp * Wp * C / 4, kThreads, 8192), kThreads, 0, (hipStream_t)stream>>>(x, (const T*)dy, dx, accumulate, (int)B, (int)Hp, (int)Wp, (int)C);
    });
}

extern "C" int mtp_axpy_f32(float* y, const float* x, float alpha, int64_t n, mtp_stream_t stream) {
    if (!y || !x || n <= 0) return MTP_ERR_ARG;
    axpy_kernel<<<blocks_for(n, kThreads, 8192), kThreads, 0, (hipStream_t)stream>>>(y, x, alpha, n);
    return mtp_launch_status();
}

// several small independent copies in one launch (blockIdx.y = segment); the table travels in the kernel arguments
struct CopySegs {
    const float* src[MTP_MAX_SEGMENTS];
    float* dst[MTP_MAX_SEGMENTS];
    int64_t count[MTP_MAX_SEGMENTS];
};
__global__ __launch_bounds__(256) void copy_segments_kernel(CopySegs t) {
    const int sgm = blockIdx.y;
    const float* __restrict__ s = t.src[sgm];
    float* __restrict__ d = t.dst[sgm];
    const int64_t n = t.count[sgm];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) d[i] = s[i];
}
extern "C" int mtp_copy_segments_f32(const float* const* src, float* const* dst, const int64_t* count, int n, mtp_stream_t stream) {
    if (!src || !dst || !count || n <= 0 || n > MTP_MAX_SEGMENTS) return MTP_ERR_ARG;
    CopySegs t;
    int64_t mx = 0;
    for (int i = 0; i < n; ++i) {
        if (!src[i] || !dst[i] || count[i] <= 0) return MTP_ERR_ARG;
        t.src[i] = src[i]; t.dst[i] = dst[i]; t.count[i] = count[i];
        mx = count[i] > mx ? count[i] : mx;
    }
    copy_segments_kernel<<<dim3(blocks_for(mx, kThreads, 256), (unsigned)n), kThreads, 0, (hipStream_t)stream>>>(t);
    return mtp_launch_status();
}

namespace {
// dst[r][c] = scale[r / rows_per_sample] * src[r][c]  (f32 -> ACT), the drop-path-scaled operand copy of a residual gradient
template <typename T>
__global__ __launch_bounds__(256) void scale_rows_cast_kernel(const float* __restrict__ src, T* __restrict__ dst, const float* __restrict__ scale,
                                                             int64_t rows_per_sample, int64_t rows, int64_t C) {
    const int64_t C4 = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows * C4; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / C4;
        const float s = scale ? scale[r / rows_per_sample] : 1.0f;
        const float4 v = load4(src + 4 * i);
        store4(dst + 4 * i, make_float4(v.x * s, v.y * s, v.z * s, v.w * s));
    }
}
}  // namespace

extern "C" int mtp_scale_rows_cast(const float* src, void* dst, int dst_dtype, const float* scale, int64_t rows_per_sample, int64_t rows, int64_t C, mtp_stream_t stream) {
    if (!src || !dst || rows <= 0 || (C % 4) || (scale && rows_per_sample <= 0)) return MTP_ERR_ARG;
    return for_act(dst_dtype, [&](auto t) {
        using T = decltype(t);
        scale_rows_cast_kernel<T><<<blocks_for(rows * C / 4, kThreads, 8192), kThreads, 0, (hipStream_t)stream>>>(src, (T*)dst, scale, rows_per_sample, rows, C);
    });
}
