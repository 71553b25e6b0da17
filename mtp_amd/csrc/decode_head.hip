// UperNet decode head (mmseg UPerHead, RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/uper_head.py): the layers around its
// GEMMs.  Every map is channels-last, (rows = N*H*W, C) with a row pitch ld (elements), so a kernel can read or write one channel slice of a
// concatenation in place.  Statistics and reductions are f32 and deterministic: per-workgroup partial rows summed in a fixed order
// (col_sums_kernel, or the single-workgroup tree of the loss), no float atomics anywhere in this file.
#include "common.h"
#include "resize_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- BatchNorm
// rows are split into `nblk` contiguous chunks (a function of `rows` alone, so the summation order never changes); a workgroup of 4 waves
// takes one chunk and 256 channels (4 per lane), the waves stride its rows and are combined in LDS in wave order.
inline int64_t bn_partial_rows(int64_t rows) {
    int64_t nb = (rows + 63) / 64;
    return nb < 512 ? nb : 512;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) bn_stats_kernel(const void* x, int64_t ldx, const float* center, float* part, int64_t rows, int64_t C,
                                                            int64_t chunk) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c = ((int64_t)blockIdx.y * 64 + lane) * 4;
    const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = min(rows, r0 + chunk);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
    if (c < C) {
        const float4 k = center ? load4(center + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t r = r0 + wv; r < r1; r += 4) {
            float4 v = ld4<T>(x, r * ldx + c);
            v = make_float4(v.x - k.x, v.y - k.y, v.z - k.z, v.w - k.w);
            s = f4add(s, v);
            q = make_float4(fmaf(v.x, v.x, q.x), fmaf(v.y, v.y, q.y), fmaf(v.z, v.z, q.z), fmaf(v.w, v.w, q.w));
        }
    }
    __shared__ float4 sh[2][4][64];
    sh[0][wv][lane] = s;
    sh[1][wv][lane] = q;
    __syncthreads();
    if (wv == 0 && c < C) {
        for (int w = 1; w < 4; ++w) {
            s = f4add(s, sh[0][w][lane]);
            q = f4add(q, sh[1][w][lane]);
        }
        float* o = part + (int64_t)blockIdx.x * 2 * C;
        store4(o + c, s);
        store4(o + C + c, q);
    }
}

// out[c] = sum over the nb partial rows of column c, in row order (mtp_reduce_rows_f32 splits rows over workgroups and adds with atomics)
__global__ void __launch_bounds__(kThreads) col_sums_kernel(const float* part, int64_t nb, int64_t n, float* out) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n) return;
    float s = 0.0f;
    for (int64_t r = 0; r < nb; ++r) s += part[r * n + c];
    out[c] = s;
}

// mean / rstd from the global sums of (x - center) (training: and the running statistics, momentum m, unbiased variance) or from the running
// statistics (eval).  With center = a first estimate of the mean (the two-pass form the engine uses), sum (x - center) is small and
// E[(x - c)^2] - E[x - c]^2 does not cancel when |mean| >> std.
__global__ void bn_finalize_kernel(const float* sums, const float* center, double count, float* rmean, float* rvar, float momentum, float eps, float* mean,
                                   float* rstd, int64_t C) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (!sums) {
        mean[c] = rmean[c];
        rstd[c] = 1.0f / sqrtf(rvar[c] + eps);
        return;
    }
    const double d = (double)sums[c] / count;
    double var = (double)sums[C + c] / count - d * d;
    var = var > 0.0 ? var : 0.0;
    const double m = (center ? (double)center[c] : 0.0) + d;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean) {
        rmean[c] = (1.0f - momentum) * rmean[c] + momentum * (float)m;
        const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
        rvar[c] = (1.0f - momentum) * rvar[c] + momentum * (float)unb;
    }
}

template <typename TX, typename TY>
__global__ void __launch_bounds__(kThreads) bn_apply_kernel(const void* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                                                            const float* beta, int relu, void* y, int64_t ldy, int64_t rows, int64_t C) {
    const int64_t C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= rows * C4) return;
    const int64_t r = i / C4, c = (i - r * C4) * 4;
    const float4 v = ld4<TX>(x, r * ldx + c);
    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = (o[k] - mean[c + k]) * rstd[c + k] * gamma[c + k] + beta[c + k];
        o[k] = relu ? fmaxf(t, 0.0f) : t;
    }
    st4<TY>(y, r * ldy + c, make_float4(o[0], o[1], o[2], o[3]));
}

// backward partials: [sum dy' | sum dy' * xhat] with dy' = dy * relu'(gamma * xhat + beta) (the mask recomputed from x exactly as the forward had it)
template <typename TX, typename TD>
__global__ void __launch_bounds__(kThreads) bn_bwd_stats_kernel(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean,
                                                                const float* rstd, const float* gamma, const float* beta, int relu, float* part,
                                                                int64_t rows, int64_t C, int64_t chunk) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c = ((int64_t)blockIdx.y * 64 + lane) * 4;
    const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = min(rows, r0 + chunk);
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        float mu[4], rs[4], g[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { mu[k] = mean[c + k]; rs[k] = rstd[c + k]; g[k] = gamma[c + k]; b[k] = beta[c + k]; }
        for (int64_t r = r0 + wv; r < r1; r += 4) {
            const float4 xv = ld4<TX>(x, r * ldx + c), dv = ld4<TD>(dy, r * lddy + c);
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ds[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xh = (xs[k] - mu[k]) * rs[k];
                const float d = (!relu || xh * g[k] + b[k] > 0.0f) ? ds[k] : 0.0f;
                s[k] += d;
                q[k] = fmaf(d, xh, q[k]);
            }
        }
    }
    __shared__ float4 sh[2][4][64];
    sh[0][wv][lane] = make_float4(s[0], s[1], s[2], s[3]);
    sh[1][wv][lane] = make_float4(q[0], q[1], q[2], q[3]);
    __syncthreads();
    if (wv == 0 && c < C) {
        float4 a = sh[0][0][lane], bq = sh[1][0][lane];
        for (int w = 1; w < 4; ++w) {
            a = f4add(a, sh[0][w][lane]);
            bq = f4add(bq, sh[1][w][lane]);
        }
        float* o = part + (int64_t)blockIdx.x * 2 * C;
        store4(o + c, a);
        store4(o + C + c, bq);
    }
}

// dx = gamma * rstd * (dy' - sum(dy') / n - xhat * sum(dy' xhat) / n)   (training; the sums over the whole -- possibly all-reduced -- batch)
// dx = gamma * rstd * dy'                                                 (eval statistics: sums == NULL)
template <typename TX, typename TD, typename TO>
__global__ void __launch_bounds__(kThreads) bn_bwd_dx_kernel(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean,
                                                             const float* rstd, const float* gamma, const float* beta, int relu, const float* sums,
                                                             float inv_count, void* dx, int64_t lddx, int64_t rows, int64_t C) {
    const int64_t C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= rows * C4) return;
    const int64_t r = i / C4, c = (i - r * C4) * 4;
    const float4 xv = ld4<TX>(x, r * ldx + c), dv = ld4<TD>(dy, r * lddy + c);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ds[4] = {dv.x, dv.y, dv.z, dv.w};
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xh = (xs[k] - mean[c + k]) * rstd[c + k];
        const float d = (!relu || xh * gamma[c + k] + beta[c + k] > 0.0f) ? ds[k] : 0.0f;
        const float t = sums ? d - sums[c + k] * inv_count - xh * sums[C + c + k] * inv_count : d;
        o[k] = gamma[c + k] * rstd[c + k] * t;
    }
    st4<TO>(dx, r * lddx + c, make_float4(o[0], o[1], o[2], o[3]));
}

// ---------------------------------------------------------------------------------------------------------------- bilinear resize
// Lin / lin_index (the F.interpolate align_corners=False index rule): resize_common.h, shared with seg_eval.hip
// weight of source index i in output o's interpolation
__device__ __forceinline__ float lin_weight(int o, int i, int in, float scale) {
    const Lin L = lin_index(o, in, scale);
    return (L.i0 == i ? L.w0 : 0.0f) + (L.i1 == i ? L.w1 : 0.0f);
}
// outputs whose interpolation can touch source i: i0(o) in {i - 1, i}; a margin of one on each side absorbs the float rounding of the bound
__device__ __forceinline__ void lin_range(int i, int in, int out, float scale, int& lo, int& hi) {
    const float inv = (float)out / (float)in;
    lo = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1;
    hi = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > out - 1 ? out - 1 : hi;
    if (i == in - 1) hi = out - 1;
}

template <typename TX, typename TY>
__global__ void __launch_bounds__(kThreads) resize_fwd_kernel(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t N, int Hi, int Wi, int Ho, int Wo,
                                                              int64_t C, int accumulate) {
    const int64_t C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N * Ho * Wo * C4) return;
    const int64_t pix = i / C4, c = (i - pix * C4) * 4;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
    const int64_t n = pix / ((int64_t)Wo * Ho);
    const Lin ly = lin_index(oy, Hi, (float)Hi / (float)Ho), lx = lin_index(ox, Wi, (float)Wi / (float)Wo);
    const int64_t b = n * Hi * Wi;
    const float4 v00 = ld4<TX>(x, (b + (int64_t)ly.i0 * Wi + lx.i0) * ldx + c), v01 = ld4<TX>(x, (b + (int64_t)ly.i0 * Wi + lx.i1) * ldx + c);
    const float4 v10 = ld4<TX>(x, (b + (int64_t)ly.i1 * Wi + lx.i0) * ldx + c), v11 = ld4<TX>(x, (b + (int64_t)ly.i1 * Wi + lx.i1) * ldx + c);
    // ATen's order: h0lambda * (w0lambda * v00 + w1lambda * v01) + h1lambda * (w0lambda * v10 + w1lambda * v11)
    float4 t0 = f4add(f4scale(v00, lx.w0), f4scale(v01, lx.w1)), t1 = f4add(f4scale(v10, lx.w0), f4scale(v11, lx.w1));
    float4 o = f4add(f4scale(t0, ly.w0), f4scale(t1, ly.w1));
    const int64_t yo = pix * ldy + c;
    if (accumulate) o = f4add(o, ld4<TY>(y, yo));
    st4<TY>(y, yo, o);
}

// the adjoint as a gather: every source pixel sums its bounded set of destinations (deterministic, no atomics).  dx f32.
template <typename TD>
__global__ void __launch_bounds__(kThreads) resize_bwd_kernel(const void* dy, int64_t lddy, float* dx, int64_t lddx, int64_t N, int Hi, int Wi, int Ho,
                                                              int Wo, int64_t C, int accumulate) {
    const int64_t C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N * Hi * Wi * C4) return;
    const int64_t pix = i / C4, c = (i - pix * C4) * 4;
    const int ix = (int)(pix % Wi), iy = (int)((pix / Wi) % Hi);
    const int64_t n = pix / ((int64_t)Wi * Hi);
    const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
    int y0, y1, x0, x1;
    lin_range(iy, Hi, Ho, sy, y0, y1);
    lin_range(ix, Wi, Wo, sx, x0, x1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = y0; oy <= y1; ++oy) {
        const float wy = lin_weight(oy, iy, Hi, sy);
        if (wy == 0.0f) continue;
        float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ox = x0; ox <= x1; ++ox) {
            const float wx = lin_weight(ox, ix, Wi, sx);
            if (wx == 0.0f) continue;
            row = f4fma(ld4<TD>(dy, ((n * Ho + oy) * Wo + ox) * lddy + c), wx, row);
        }
        acc = f4fma(row, wy, acc);
    }
    float* o = dx + pix * lddx + c;
    if (accumulate) acc = f4add(acc, load4(o));
    store4(o, acc);
}

// ---------------------------------------------------------------------------------------------------------------- adaptive average pooling
// torch's bins: start = floor(i * H / S), end = ceil((i + 1) * H / S)
__device__ __forceinline__ int bin_start(int i, int H, int S) { return (int)(((int64_t)i * H) / S); }
__device__ __forceinline__ int bin_end(int i, int H, int S) { return (int)(((int64_t)(i + 1) * H + S - 1) / S); }

template <typename TX, typename TY>
__global__ void __launch_bounds__(kThreads) pool_fwd_kernel(const void* x, int64_t ldx, void* y, int64_t N, int H, int W, int64_t C, int S) {
    const int64_t C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N * S * S * C4) return;
    const int64_t pix = i / C4, c = (i - pix * C4) * 4;
    const int ox = (int)(pix % S), oy = (int)((pix / S) % S);
    const int64_t n = pix / ((int64_t)S * S);
    const int ys = bin_start(oy, H, S), ye = bin_end(oy, H, S), xs = bin_start(ox, W, S), xe = bin_end(ox, W, S);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int yy = ys; yy < ye; ++yy)
        for (int xx = xs; xx < xe; ++xx) acc = f4add(acc, ld4<TX>(x, ((n * H + yy) * W + xx) * ldx + c));
    st4<TY>(y, pix * C + c, f4scale(acc, 1.0f / (float)((ye - ys) * (xe - xs))));
}

template <typename TD>
__global__ void __launch_bounds__(kThreads) pool_bwd_kernel(const void* dy, float* dx, int64_t lddx, int64_t N, int H, int W, int64_t C, int S, int accumulate) {
    const int64_t C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N * H * W * C4) return;
    const int64_t pix = i / C4, c = (i - pix * C4) * 4;
    const int xx = (int)(pix % W), yy = (int)((pix / W) % H);
    const int64_t n = pix / ((int64_t)W * H);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = 0; oy < S; ++oy) {
        const int ys = bin_start(oy, H, S), ye = bin_end(oy, H, S);
        if (yy < ys || yy >= ye) continue;
        for (int ox = 0; ox < S; ++ox) {
            const int xs = bin_start(ox, W, S), xe = bin_end(ox, W, S);
            if (xx < xs || xx >= xe) continue;
            acc = f4fma(ld4<TD>(dy, ((n * S + oy) * S + ox) * C + c), 1.0f / (float)((ye - ys) * (xe - xs)), acc);
        }
    }
    float* o = dx + pix * lddx + c;
    if (accumulate) acc = f4add(acc, load4(o));
    store4(o, acc);
}

// ---------------------------------------------------------------------------------------------------------------- Dropout2d
template <typename TX, typename TY>
__global__ void __launch_bounds__(kThreads) channel_scale_kernel(const void* x, int64_t ldx, const float* mask, int64_t rows_per_sample, void* y, int64_t ldy,
                                                                 int64_t rows, int64_t C) {
    const int64_t C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= rows * C4) return;
    const int64_t r = i / C4, c = (i - r * C4) * 4;
    const float* m = mask + (r / rows_per_sample) * C + c;
    const float4 v = ld4<TX>(x, r * ldx + c);
    st4<TY>(y, r * ldy + c, make_float4(v.x * m[0], v.y * m[1], v.z * m[2], v.w * m[3]));
}

// ---------------------------------------------------------------------------------------------------------------- segmentation loss
// One thread per label pixel: the logits interpolated from the low-resolution grid (the resize forward's rule), softmax cross-entropy,
// d(upsampled logits) = scale * (softmax - onehot) into the workspace (zero for ignored pixels), and one loss partial per workgroup.
template <typename TX, typename TL>
__global__ void __launch_bounds__(kThreads) seg_ce_kernel(const void* logits, int64_t ld, const TL* labels, int64_t N, int h, int w, int K, int H, int W,
                                                          int ignore_index, float scale, float* dhr, float* part) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    float loss = 0.0f;
    if (p < N * H * W) {
        const int ox = (int)(p % W), oy = (int)((p / W) % H);
        const int64_t n = p / ((int64_t)W * H);
        const int64_t lab = (int64_t)labels[p];
        float* d = dhr + p * K;
        if (lab == ignore_index) {
            for (int k = 0; k < K; ++k) d[k] = 0.0f;
        } else {
            const Lin ly = lin_index(oy, h, (float)h / (float)H), lx = lin_index(ox, w, (float)w / (float)W);
            const int64_t b = n * h * w;
            const int64_t r00 = (b + (int64_t)ly.i0 * w + lx.i0) * ld, r01 = (b + (int64_t)ly.i0 * w + lx.i1) * ld;
            const int64_t r10 = (b + (int64_t)ly.i1 * w + lx.i0) * ld, r11 = (b + (int64_t)ly.i1 * w + lx.i1) * ld;
            float mx = -INFINITY, zlab = 0.0f;
            for (int k = 0; k < K; ++k) {
                const float z = ly.w0 * (lx.w0 * ld1<TX>(logits, r00 + k) + lx.w1 * ld1<TX>(logits, r01 + k)) +
                                ly.w1 * (lx.w0 * ld1<TX>(logits, r10 + k) + lx.w1 * ld1<TX>(logits, r11 + k));
                d[k] = z;
                zlab = k == lab ? z : zlab;
                mx = fmaxf(mx, z);
            }
            float se = 0.0f;
            for (int k = 0; k < K; ++k) {
                const float e = expf(d[k] - mx);
                d[k] = e;
                se += e;
            }
            const float inv = 1.0f / se;
            for (int k = 0; k < K; ++k) d[k] = scale * (d[k] * inv - (k == lab ? 1.0f : 0.0f));
            loss = logf(se) - (zlab - mx);     // -log softmax[label]
        }
    }
    __shared__ float sh[kThreads];
    sh[threadIdx.x] = loss;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// loss = scale * sum(part): one workgroup, fixed order
__global__ void __launch_bounds__(kThreads) sum_scale_kernel(const float* part, int64_t n, float scale, float* out) {
    float s = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) s += part[i];
    __shared__ float sh[kThreads];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int k = kThreads / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0] * scale;
}

template <typename TD>
__global__ void __launch_bounds__(kThreads) resize_bwd1_kernel(const float* dy, int K, float* dx, int64_t lddx, int64_t N, int Hi, int Wi, int Ho, int Wo) {
    // the scalar-channel form of resize_bwd_kernel for the class dimension (K need not be a multiple of 4)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N * Hi * Wi * K) return;
    const int64_t pix = i / K;
    const int k = (int)(i - pix * K);
    const int ix = (int)(pix % Wi), iy = (int)((pix / Wi) % Hi);
    const int64_t n = pix / ((int64_t)Wi * Hi);
    const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
    int y0, y1, x0, x1;
    lin_range(iy, Hi, Ho, sy, y0, y1);
    lin_range(ix, Wi, Wo, sx, x0, x1);
    float acc = 0.0f;
    for (int oy = y0; oy <= y1; ++oy) {
        const float wy = lin_weight(oy, iy, Hi, sy);
        if (wy == 0.0f) continue;
        float row = 0.0f;
        for (int ox = x0; ox <= x1; ++ox) {
            const float wx = lin_weight(ox, ix, Wi, sx);
            if (wx == 0.0f) continue;
            row = fmaf(dy[((n * Ho + oy) * Wo + ox) * K + k], wx, row);
        }
        acc = fmaf(row, wy, acc);
    }
    dx[pix * lddx + k] = acc;
}

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int64_t mtp_bn_partial_rows(int64_t rows) { return rows > 0 ? bn_partial_rows(rows) : MTP_ERR_ARG; }

extern "C" int mtp_bn_stats(const void* x, int dtype, int64_t ldx, const float* center, float* part, float* sums, int64_t rows, int64_t C,
                            mtp_stream_t stream) {
    MTP_CHECK_ARG(x && part && sums && rows > 0 && C > 0 && (C % 4) == 0 && ldx >= C && (ldx % 4) == 0 && dt_ok(dtype));
    const int64_t nb = bn_partial_rows(rows), chunk = (rows + nb - 1) / nb;
    const dim3 grid((unsigned)nb, (unsigned)((C / 4 + 63) / 64));
    if (dtype == MTP_F32) bn_stats_kernel<float><<<grid, kThreads, 0, (hipStream_t)stream>>>(x, ldx, center, part, rows, C, chunk);
    else bn_stats_kernel<bf16_t><<<grid, kThreads, 0, (hipStream_t)stream>>>(x, ldx, center, part, rows, C, chunk);
    col_sums_kernel<<<blocks_exact(2 * C), kThreads, 0, (hipStream_t)stream>>>(part, nb, 2 * C, sums);
    return mtp_launch_status();
}

extern "C" int mtp_bn_finalize(const float* sums, const float* center, double count, float* running_mean, float* running_var, float momentum, float eps, float* mean, float* rstd,
                               int64_t C, mtp_stream_t stream) {
    MTP_CHECK_ARG(mean && rstd && C > 0);
    MTP_CHECK_ARG(sums ? count > 0.0 && ((running_mean == nullptr) == (running_var == nullptr)) : (running_mean && running_var));
    bn_finalize_kernel<<<blocks_exact(C), kThreads, 0, (hipStream_t)stream>>>(sums, center, count, running_mean, running_var, momentum, eps, mean, rstd, C);
    return mtp_launch_status();
}

extern "C" int mtp_bn_apply(const void* x, int x_dtype, int64_t ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                            void* y, int y_dtype, int64_t ldy, int64_t rows, int64_t C, mtp_stream_t stream) {
    MTP_CHECK_ARG(x && mean && rstd && gamma && beta && y && rows > 0 && C > 0 && (C % 4) == 0 && dt_ok(x_dtype) && dt_ok(y_dtype));
    MTP_CHECK_ARG(ldx >= C && ldy >= C && (ldx % 4) == 0 && (ldy % 4) == 0);
    MTP_DISPATCH2(x_dtype, y_dtype,
                  bn_apply_kernel<TA, TB><<<blocks_exact(rows * (C / 4)), kThreads, 0, (hipStream_t)stream>>>(x, ldx, mean, rstd, gamma, beta, relu, y, ldy, rows, C));
    return mtp_launch_status();
}

extern "C" int mtp_bn_bwd_stats(const void* dy, int dy_dtype, int64_t lddy, const void* x, int x_dtype, int64_t ldx, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, int relu, float* part, float* sums, int64_t rows, int64_t C, mtp_stream_t stream) {
    MTP_CHECK_ARG(dy && x && mean && rstd && gamma && beta && part && sums && rows > 0 && C > 0 && (C % 4) == 0 && dt_ok(dy_dtype) && dt_ok(x_dtype));
    MTP_CHECK_ARG(ldx >= C && lddy >= C && (ldx % 4) == 0 && (lddy % 4) == 0);
    const int64_t nb = bn_partial_rows(rows), chunk = (rows + nb - 1) / nb;
    const dim3 grid((unsigned)nb, (unsigned)((C / 4 + 63) / 64));
    MTP_DISPATCH2(x_dtype, dy_dtype,
                  bn_bwd_stats_kernel<TA, TB><<<grid, kThreads, 0, (hipStream_t)stream>>>(dy, lddy, x, ldx, mean, rstd, gamma, beta, relu, part, rows, C, chunk));
    col_sums_kernel<<<blocks_exact(2 * C), kThreads, 0, (hipStream_t)stream>>>(part, nb, 2 * C, sums);
    return mtp_launch_status();
}

extern "C" int mtp_bn_bwd_dx(const void* dy, int dy_dtype, int64_t lddy, const void* x, int x_dtype, int64_t ldx, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, int relu, const float* sums, double count, void* dx, int dx_dtype, int64_t lddx,
                             int64_t rows, int64_t C, mtp_stream_t stream) {
    MTP_CHECK_ARG(dy && x && mean && rstd && gamma && beta && dx && rows > 0 && C > 0 && (C % 4) == 0);
    MTP_CHECK_ARG(dt_ok(dy_dtype) && dt_ok(x_dtype) && dt_ok(dx_dtype) && (!sums || count > 0.0));
    MTP_CHECK_ARG(ldx >= C && lddy >= C && lddx >= C && (ldx % 4) == 0 && (lddy % 4) == 0 && (lddx % 4) == 0);
    const float inv = sums ? (float)(1.0 / count) : 0.0f;
    const unsigned g = blocks_exact(rows * (C / 4));
    hipStream_t s = (hipStream_t)stream;
    // (x, dy) dtypes x dx dtype
    if (dx_dtype == MTP_F32) {
        MTP_DISPATCH2(x_dtype, dy_dtype, bn_bwd_dx_kernel<TA, TB, float><<<g, kThreads, 0, s>>>(dy, lddy, x, ldx, mean, rstd, gamma, beta, relu, sums, inv, dx, lddx, rows, C));
    } else {
        MTP_DISPATCH2(x_dtype, dy_dtype, bn_bwd_dx_kernel<TA, TB, bf16_t><<<g, kThreads, 0, s>>>(dy, lddy, x, ldx, mean, rstd, gamma, beta, relu, sums, inv, dx, lddx, rows, C));
    }
    return mtp_launch_status();
}

extern "C" int mtp_resize_bilinear_fwd(const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy, int64_t N, int64_t Hi, int64_t Wi,
                                       int64_t Ho, int64_t Wo, int64_t C, int accumulate, mtp_stream_t stream) {
    MTP_CHECK_ARG(x && y && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0 && (C % 4) == 0 && dt_ok(x_dtype) && dt_ok(y_dtype));
    MTP_CHECK_ARG(ldx >= C && ldy >= C && (ldx % 4) == 0 && (ldy % 4) == 0 && Hi < INT32_MAX && Wi < INT32_MAX && Ho < INT32_MAX && Wo < INT32_MAX);
    MTP_DISPATCH2(x_dtype, y_dtype,
                  resize_fwd_kernel<TA, TB><<<blocks_exact(N * Ho * Wo * (C / 4)), kThreads, 0, (hipStream_t)stream>>>(x, ldx, y, ldy, N, (int)Hi, (int)Wi, (int)Ho,
                                                                                                              (int)Wo, C, accumulate));
    return mtp_launch_status();
}

extern "C" int mtp_resize_bilinear_bwd(const void* dy, int dy_dtype, int64_t lddy, float* dx, int64_t lddx, int64_t N, int64_t Hi, int64_t Wi, int64_t Ho,
                                       int64_t Wo, int64_t C, int accumulate, mtp_stream_t stream) {
    MTP_CHECK_ARG(dy && dx && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0 && (C % 4) == 0 && dt_ok(dy_dtype));
    MTP_CHECK_ARG(lddx >= C && lddy >= C && (lddx % 4) == 0 && (lddy % 4) == 0 && Hi < INT32_MAX && Wi < INT32_MAX && Ho < INT32_MAX && Wo < INT32_MAX);
    const unsigned g = blocks_exact(N * Hi * Wi * (C / 4));
    if (dy_dtype == MTP_F32)
        resize_bwd_kernel<float><<<g, kThreads, 0, (hipStream_t)stream>>>(dy, lddy, dx, lddx, N, (int)Hi, (int)Wi, (int)Ho, (int)Wo, C, accumulate);
    else
        resize_bwd_kernel<bf16_t><<<g, kThreads, 0, (hipStream_t)stream>>>(dy, lddy, dx, lddx, N, (int)Hi, (int)Wi, (int)Ho, (int)Wo, C, accumulate);
    return mtp_launch_status();
}

extern "C" int mtp_adaptive_avg_pool_fwd(const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C,
                                         int64_t S, mtp_stream_t stream) {
    MTP_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && (C % 4) == 0 && S > 0 && S <= 64 && ldx >= C && (ldx % 4) == 0);
    MTP_CHECK_ARG(dt_ok(x_dtype) && dt_ok(y_dtype) && H < INT32_MAX && W < INT32_MAX);
    MTP_DISPATCH2(x_dtype, y_dtype,
                  pool_fwd_kernel<TA, TB><<<blocks_exact(N * S * S * (C / 4)), kThreads, 0, (hipStream_t)stream>>>(x, ldx, y, N, (int)H, (int)W, C, (int)S));
    return mtp_launch_status();
}

extern "C" int mtp_adaptive_avg_pool_bwd(const void* dy, int dy_dtype, float* dx, int64_t lddx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t S,
                                         int accumulate, mtp_stream_t stream) {
    MTP_CHECK_ARG(dy && dx && N > 0 && H > 0 && W > 0 && C > 0 && (C % 4) == 0 && S > 0 && S <= 64 && lddx >= C && (lddx % 4) == 0 && dt_ok(dy_dtype));
    MTP_CHECK_ARG(H < INT32_MAX && W < INT32_MAX);
    const unsigned g = blocks_exact(N * H * W * (C / 4));
    if (dy_dtype == MTP_F32) pool_bwd_kernel<float><<<g, kThreads, 0, (hipStream_t)stream>>>(dy, dx, lddx, N, (int)H, (int)W, C, (int)S, accumulate);
    else pool_bwd_kernel<bf16_t><<<g, kThreads, 0, (hipStream_t)stream>>>(dy, dx, lddx, N, (int)H, (int)W, C, (int)S, accumulate);
    return mtp_launch_status();
}

extern "C" int mtp_channel_scale(const void* x, int x_dtype, int64_t ldx, const float* mask, int64_t rows_per_sample, void* y, int y_dtype, int64_t ldy,
                                 int64_t rows, int64_t C, mtp_stream_t stream) {
    MTP_CHECK_ARG(x && mask && y && rows > 0 && C > 0 && (C % 4) == 0 && rows_per_sample > 0 && dt_ok(x_dtype) && dt_ok(y_dtype));
    MTP_CHECK_ARG(ldx >= C && ldy >= C && (ldx % 4) == 0 && (ldy % 4) == 0);
    MTP_DISPATCH2(x_dtype, y_dtype,
                  channel_scale_kernel<TA, TB><<<blocks_exact(rows * (C / 4)), kThreads, 0, (hipStream_t)stream>>>(x, ldx, mask, rows_per_sample, y, ldy, rows, C));
    return mtp_launch_status();
}

extern "C" int64_t mtp_seg_ce_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t K) {
    if (N <= 0 || H <= 0 || W <= 0 || K <= 0) return MTP_ERR_ARG;
    const int64_t pix = N * H * W;
    return (pix * K + (pix + kThreads - 1) / kThreads) * (int64_t)sizeof(float);
}

extern "C" int mtp_seg_ce(const void* logits, int dtype, int64_t ld, int64_t N, int64_t h, int64_t w, int64_t K, const void* labels, int label_bytes, int64_t H,
                          int64_t W, int ignore_index, float loss_weight, float* loss, float* dlogits, int64_t ldd, void* workspace, int64_t workspace_bytes,
                          mtp_stream_t stream) {
    MTP_CHECK_ARG(logits && labels && loss && dlogits && workspace && N > 0 && h > 0 && w > 0 && K > 0 && K <= 4096 && H > 0 && W > 0);
    MTP_CHECK_ARG(dt_ok(dtype) && (label_bytes == 1 || label_bytes == 8) && ld >= K && ldd >= K && h < INT32_MAX && w < INT32_MAX && H < INT32_MAX && W < INT32_MAX);
    MTP_CHECK_ARG(workspace_bytes >= mtp_seg_ce_workspace_bytes(N, H, W, K) && ((uintptr_t)workspace & 15) == 0);
    const int64_t pix = N * H * W, nb = (pix + kThreads - 1) / kThreads;
    float* dhr = reinterpret_cast<float*>(workspace);
    float* part = dhr + pix * K;
    const float scale = loss_weight / (float)pix;       // mmseg CrossEntropyLoss, avg_non_ignore=False: the mean over ALL pixels
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = (unsigned)nb;
    if (dtype == MTP_F32 && label_bytes == 1)
        seg_ce_kernel<float, uint8_t><<<g, kThreads, 0, s>>>(logits, ld, (const uint8_t*)labels, N, (int)h, (int)w, (int)K, (int)H, (int)W, ignore_index, scale, dhr, part);
    else if (dtype == MTP_F32)
        seg_ce_kernel<float, int64_t><<<g, kThreads, 0, s>>>(logits, ld, (const int64_t*)labels, N, (int)h, (int)w, (int)K, (int)H, (int)W, ignore_index, scale, dhr, part);
    else if (label_bytes == 1)
        seg_ce_kernel<bf16_t, uint8_t><<<g, kThreads, 0, s>>>(logits, ld, (const uint8_t*)labels, N, (int)h, (int)w, (int)K, (int)H, (int)W, ignore_index, scale, dhr, part);
    else
        seg_ce_kernel<bf16_t, int64_t><<<g, kThreads, 0, s>>>(logits, ld, (const int64_t*)labels, N, (int)h, (int)w, (int)K, (int)H, (int)W, ignore_index, scale, dhr, part);
    sum_scale_kernel<<<1, kThreads, 0, s>>>(part, nb, scale, loss);
    resize_bwd1_kernel<float><<<blocks_exact(N * h * w * K), kThreads, 0, s>>>(dhr, (int)K, dlogits, ldd, N, (int)h, (int)w, (int)H, (int)W);
    return mtp_launch_status();
}
