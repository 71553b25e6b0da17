// The bodies of the per-window sampling-head kernels (rvsa_sampling.hip) as device functions, so that the same code runs as a stand-alone 256-thread
// workgroup and inside the 512-thread rider workgroups of the NT GEMM launch (gemm_p8.hip).  A group of 256 threads is named by `tid` (0 .. 255), scratch
// by a pointer.  The callers own the barriers between the parts, keep trip counts uniform over the whole workgroup and predicate the tail (a dead group
// computes on a clamped window and stores nothing).
#pragma once
#include "common.h"

namespace {

// zero pad, AvgPool2d(7, 7), LeakyReLU of window `win` by one 256-thread group: the pooled row goes to pl (C floats) and -- store -- to avg / pooled.
// RB: window rows whose loads are in flight together -- 7 (all 49 loads at once) in the stand-alone kernel; the rider, which shares its registers with the
// GEMM's kernel arguments, takes the rows in two batches.  The sums are added in the same order either way.
template <typename T, int RB = 7>
__device__ __forceinline__ void rvsa_pool_window(const T* __restrict__ x, float* __restrict__ avg, float* __restrict__ pooled, int Hp, int Wp, int C,
                                                 int pad_t, int pad_l, int nh, int nw, int win, bool store, int tid, float* __restrict__ pl) {
    const int j = win % nw, i = (win / nw) % nh, b = win / (nw * nh);
    for (int c4 = tid; c4 < C / 4; c4 += 256) {
        float4 s = make_float4(0, 0, 0, 0);
#pragma unroll      // (round 4: all 49 row loads of the window in flight -- with `unroll 1` the seven rows were seven serialised round trips, most of the kernel's 17.6 us)
        for (int a = 0; a < 7; ++a) {
            if (RB < 7 && a == RB) __builtin_amdgcn_sched_barrier(0);
            const int y = i * 7 + a - pad_t;
            const bool yok = y >= 0 && y < Hp;
            // a pad position loads the nearest token row / column, which lies in this window (the padding on either side is less than one window), and
            // masks it: clamped to row / column 0 instead, a non-finite token there turned 0 * Inf into NaN in windows that do not hold it
            const int yc = y < 0 ? 0 : (y < Hp ? y : Hp - 1);
            float4 v[7];
#pragma unroll
            for (int bb = 0; bb < 7; ++bb) {
                const int xx = j * 7 + bb - pad_l;
                const int xc = xx < 0 ? 0 : (xx < Wp ? xx : Wp - 1);
                v[bb] = load4(x + (((int64_t)b * Hp + yc) * Wp + xc) * C + 4 * c4);
            }
#pragma unroll
            for (int bb = 0; bb < 7; ++bb) {
                const int xx = j * 7 + bb - pad_l;
                const float m = (yok && xx >= 0 && xx < Wp) ? 1.f : 0.f;
                s.x += m * v[bb].x; s.y += m * v[bb].y; s.z += m * v[bb].z; s.w += m * v[bb].w;
            }
        }
        const float inv = 1.0f / 49.0f;
        s = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
        const float4 p = make_float4(s.x > 0 ? s.x : 0.01f * s.x, s.y > 0 ? s.y : 0.01f * s.y, s.z > 0 ? s.z : 0.01f * s.z, s.w > 0 ? s.w : 0.01f * s.w);
        if (store) {
            store4(avg + (int64_t)win * C + 4 * c4, s);
            store4(pooled + (int64_t)win * C + 4 * c4, p);
        }
        *reinterpret_cast<float4*>(pl + 4 * c4) = p;
    }
}

// outputs [nlo, nhi) of the stacked heads for W pooled rows pl[0 .. W) (C floats each, in LDS) at once: wave `wave` of `nwaves` takes four output columns
// per pass, and every weight vector it loads serves all W rows.  Row i belongs to window win0 + i * wstep and is stored while that is below `windows`.
// An output's bits depend on the lane -> k mapping and the k order below only, not on which wave or pass produces it, nor on W.
template <int W>
__device__ __forceinline__ void rvsa_heads(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ samp, int C, int N, int nlo, int nhi,
                                           int wave, int nwaves, int lane, const float* __restrict__ pl, int win0, int wstep, int windows) {
#pragma clang fp contract(off)
    for (int n0 = nlo + 4 * wave; n0 < nhi; n0 += 4 * nwaves) {      // 4 output columns per pass
        float acc[W][4];
#pragma unroll
        for (int i = 0; i < W; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
        // 4 k-steps x 4 outputs = 16 weight loads of 16 B in flight per lane before the first use (round 6: written as one k-step per iteration the loop bound is a
        // run-time value, hipcc kept the iterations apart and a pass was C / 256 dependent L2 round trips -- most of the kernel's 21.6 us at C = 1024)
        for (int k0 = lane * 4; k0 < C; k0 += 1024) {
            float4 ww[4][4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int k = k0 + 256 * kk, kc = k < C ? k : 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = n0 + q < N ? n0 + q : N - 1;
                    ww[kk][q] = load4(w + (int64_t)n * C + kc);
                }
            }
#pragma unroll
            for (int i = 0; i < W; ++i) {
                if (W > 1) __builtin_amdgcn_sched_barrier(0);      // one row's LDS reads at a time: hoisted together, the reads of 8 rows do not fit the registers
                float4 a[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int k = k0 + 256 * kk, kc = k < C ? k : 0;
                    a[kk] = k < C ? *reinterpret_cast<const float4*>(pl + (int64_t)i * C + kc) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        // `acc += a.x * w.x + a.y * w.y + a.z * w.z + a.w * w.w` as hipcc compiled it in the one-row kernel, where it packs the columns in
                        // pairs: one rounded product (x in the even columns of a pass, y in the odd ones), FMAs of the other three onto it, one addition.
                        // Spelled out, with contraction off, because the bits otherwise follow the code around the expression: with several rows the
                        // accumulator was fused into the chain.  (Checked on the GPU against the kernel as it was, all 16 x 4 forms: only this one matches.)
                        float t = (q & 1) ? a[kk].y * ww[kk][q].y : a[kk].x * ww[kk][q].x;
                        t = (q & 1) ? fmaf(a[kk].x, ww[kk][q].x, t) : fmaf(a[kk].y, ww[kk][q].y, t);
                        t = fmaf(a[kk].z, ww[kk][q].z, t);
                        t = fmaf(a[kk].w, ww[kk][q].w, t);
                        acc[i][q] += t;
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const int win = win0 + i * wstep;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float t = wave_sum(acc[i][q]);
                if (lane == 0 && win < windows && n0 + q < nhi) samp[(int64_t)win * N + n0 + q] = t + (bias ? bias[n0 + q] : 0.f);
            }
        }
    }
}

// g[win][4 c4 .. 4 c4 + 3] = (dsamp[win] . w) * leaky'(avg) / 49 for the 64 channel quads c4 = c4base + lane: the group's 4 waves split the N head outputs
// of the product, meet in `part` and add in the fixed order (p0 + p1) + (p2 + p3).  ds: N floats (the dsamp row), part: 4 x 64 float4.
__device__ __forceinline__ void rvsa_sampling_bwd_win_body(const float* __restrict__ dsamp, const float* __restrict__ w, const float* __restrict__ avg,
                                                           float* __restrict__ g, int C, int N, int win, int c4base, bool live_win, int tid,
                                                           float* __restrict__ ds, float4* __restrict__ part) {
    const int lane = tid & 63, q = tid >> 6;
    const int c4 = c4base + lane;
    const bool live = c4 < C / 4;
    for (int n = tid; n < N; n += 256) ds[n] = dsamp[(int64_t)win * N + n];
    __syncthreads();
    const int nq = (N + 3) / 4, n0 = q * nq, n1 = (n0 + nq) < N ? (n0 + nq) : N;
    float4 d = make_float4(0, 0, 0, 0);
    if (live) {
#pragma unroll 10
        for (int n = n0; n < n1; ++n) {
            const float4 ww = load4(w + (int64_t)n * C + 4 * c4);
            const float t = ds[n];
            d.x += t * ww.x; d.y += t * ww.y; d.z += t * ww.z; d.w += t * ww.w;
        }
    }
    part[q * 64 + lane] = d;
    __syncthreads();
    if (!live || q || !live_win) return;
    const float4 p0 = part[lane], p1 = part[64 + lane], p2 = part[128 + lane], p3 = part[192 + lane];   // the order of rvsa_sampling_bwd_kernel: same bits
    d = make_float4((p0.x + p1.x) + (p2.x + p3.x), (p0.y + p1.y) + (p2.y + p3.y), (p0.z + p1.z) + (p2.z + p3.z), (p0.w + p1.w) + (p2.w + p3.w));
    const float4 a = load4(avg + (int64_t)win * C + 4 * c4);
    const float k = 1.0f / 49.0f;
    *reinterpret_cast<float4*>(g + (int64_t)win * C + 4 * c4) =
        make_float4(d.x * (a.x > 0 ? k : 0.01f * k), d.y * (a.y > 0 ? k : 0.01f * k), d.z * (a.z > 0 ? k : 0.01f * k), d.w * (a.w > 0 ? k : 0.01f * k));
}

}  // namespace
