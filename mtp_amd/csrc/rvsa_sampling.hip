// The sampling heads of the RVSA blocks (gfx950): zero pad, AvgPool2d(7, 7), LeakyReLU and the three stacked 1x1 convolutions as one
// small f32 linear layer -- separately (rvsa_pool_*, small_linear_*) and as one launch each way per block (rvsa_sampling_*).
// The window geometry is RvsaWindows (common.h), the one the attention kernels and the windowed LayerNorm backward use.
#include "common.h"
#include "rvsa_sampling_body.h"

namespace {

// ------------------------------------------------------------------------------------------------ RVSA sampling heads
// zero-pad to (He,We), AvgPool2d(7,7) (divide by 49 always), LeakyReLU(0.01)    (VIT:229-230, 347)
template <typename T>
__global__ __launch_bounds__(256) void rvsa_pool_fwd_kernel(const T* __restrict__ x, float* __restrict__ avg, float* __restrict__ pooled,
                                                           int Hp, int Wp, int C, int pad_t, int pad_l, int nh, int nw) {
    const int win = blockIdx.x;   // (b, i, j)
    const int j = win % nw, i = (win / nw) % nh, b = win / (nw * nh);
    for (int c4 = blockIdx.y * 256 + threadIdx.x; c4 < C / 4; c4 += gridDim.y * 256) {
        float4 s = make_float4(0, 0, 0, 0);
        for (int a = 0; a < 7; ++a) {
            const int y = i * 7 + a - pad_t;
            if (y < 0 || y >= Hp) continue;
            for (int bb = 0; bb < 7; ++bb) {
                const int xx = j * 7 + bb - pad_l;
                if (xx < 0 || xx >= Wp) continue;
                const float4 v = load4(x + (((int64_t)b * Hp + y) * Wp + xx) * C + 4 * c4);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        }
        const float inv = 1.0f / 49.0f;
        s = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
        store4(avg + (int64_t)win * C + 4 * c4, s);
        store4(pooled + (int64_t)win * C + 4 * c4, make_float4(s.x > 0 ? s.x : 0.01f * s.x, s.y > 0 ? s.y : 0.01f * s.y,
                                                              s.z > 0 ? s.z : 0.01f * s.z, s.w > 0 ? s.w : 0.01f * s.w));
    }
}
template <typename T>
__global__ __launch_bounds__(256) void rvsa_pool_bwd_kernel(const float* __restrict__ dpooled, const float* __restrict__ avg, T* __restrict__ dx, int accumulate,
                                                           int B, int Hp, int Wp, int C, int pad_t, int pad_l, int nh, int nw) {
    const int C4 = C / 4;
    const int64_t total = (int64_t)B * Hp * Wp * C4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(idx % C4);
        const int64_t t = idx / C4;
        const int xx = (int)(t % Wp), yy = (int)((t / Wp) % Hp), b = (int)(t / ((int64_t)Wp * Hp));
        const int win = (b * nh + (yy + pad_t) / 7) * nw + (xx + pad_l) / 7;
        const float4 d = load4(dpooled + (int64_t)win * C + 4 * c4), a = load4(avg + (int64_t)win * C + 4 * c4);
        const float k = 1.0f / 49.0f;
        float4 g = make_float4(d.x * (a.x > 0 ? k : 0.01f * k), d.y * (a.y > 0 ? k : 0.01f * k), d.z * (a.z > 0 ? k : 0.01f * k), d.w * (a.w > 0 ? k : 0.01f * k));
        T* p = dx + t * C + 4 * c4;
        if (accumulate) {
            const float4 o = load4(p);
            g.x += o.x; g.y += o.y; g.z += o.z; g.w += o.w;
        }
        store4(p, g);
    }
}

// ---- the three RVSA 1x1-conv heads as one small f32 linear layer (R = windows ~ 1e3, K = C, N = 5*heads = 80) -----------------
// Far too small for the MFMA GEMMs (8 output tiles); the kernels below are shaped so that the 320 KB weight is not re-read
// from L2 by every thread (the first versions moved ~335 MB of L2 traffic per call and took 35-39 us each).
// y (R,N) = x (R,K) W(N,K)^T + b : generic fallback, one block per row, one wave per output column group
__global__ __launch_bounds__(256) void small_linear_fwd_generic_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                      float* __restrict__ y, int N, int K) {
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* xr = x + (int64_t)r * K;
    for (int n = wave; n < N; n += 4) {
        const float* wr = w + (int64_t)n * K;
        float s = 0.f;
        for (int k = lane * 4; k < K; k += 256) {
            const float4 a = load4(xr + k), b = load4(wr + k);
            s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
        }
        s = wave_sum(s);
        if (lane == 0) y[(int64_t)r * N + n] = s + (bias ? bias[n] : 0.f);
    }
}
// K <= 256*MAXJ: one workgroup per ROWS rows, wave = a quarter of the output columns, the row slices stay in registers and every
// weight vector loaded from L2 is used for ROWS rows (the one-row version re-read the whole 320 KB weight per row: 335 MB of L2
// traffic per call, 39 us); 4 output columns (4*MAXJ weight loads) in flight per pass
template <int ROWS, int MAXJ>
__global__ __launch_bounds__(256) void small_linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                              float* __restrict__ y, int R, int N, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * ROWS;
    const int K4 = K >> 2;
    float4 xs[ROWS][MAXJ];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const float* xr = x + (int64_t)(r0 + i < R ? r0 + i : R - 1) * K;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int k4 = lane + 64 * j;
            xs[i][j] = k4 < K4 ? load4(xr + 4 * k4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const int per = (N + 3) / 4, n_lo = wave * per, n_hi = (n_lo + per) < N ? (n_lo + per) : N;
    for (int n = n_lo; n < n_hi; n += 4) {
        float s[4][ROWS];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int nn = n + q < n_hi ? n + q : n_hi - 1;
            const float* wr = w + (int64_t)nn * K;
#pragma unroll
            for (int i = 0; i < ROWS; ++i) s[q][i] = 0.f;
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) {
                // unconditional load from a clamped index (xs is zero beyond K): a branch around the load makes hipcc wait for
                // each one separately -- 4*MAXJ serialised L2 latencies per pass, measured 10 us per pass
                const int k4 = lane + 64 * j, k4c = k4 < K4 ? k4 : K4 - 1;
                const float4 b = load4(wr + 4 * k4c);
#pragma unroll
                for (int i = 0; i < ROWS; ++i) s[q][i] += xs[i][j].x * b.x + xs[i][j].y * b.y + xs[i][j].z * b.z + xs[i][j].w * b.w;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < ROWS; ++i) s[q][i] = wave_sum(s[q][i]);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < ROWS; ++i)
                    if (n + q < n_hi && r0 + i < R) y[(int64_t)(r0 + i) * N + n + q] = s[q][i] + (bias ? bias[n + q] : 0.f);
        }
    }
}
// dx (R,K) = dy (R,N) W (N,K): thread = 4 k-columns x 4 rows (the dy factors are workgroup-uniform: scalar loads), so each
// weight vector is loaded once per 4 rows
__global__ __launch_bounds__(256) void small_linear_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, int R, int N, int K) {
    const int k = (blockIdx.x * 256 + threadIdx.x) * 4, r0 = blockIdx.y * 4;
    if (k >= K) return;
    const float* d[4];
    float4 s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rr = r0 + i < R ? r0 + i : R - 1;
        d[i] = dy + (int64_t)rr * N;
        s[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll 4
    for (int n = 0; n < N; ++n) {
        const float4 ww = load4(w + (int64_t)n * K + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dv = d[i][n];
            s[i].x += dv * ww.x; s[i].y += dv * ww.y; s[i].z += dv * ww.z; s[i].w += dv * ww.w;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (r0 + i < R) store4(dx + (int64_t)(r0 + i) * K + k, s[i]);
}
// dw (N,K) = dy^T x ; db[n] = sum_r dy[r][n].  Workgroup = 256 k-columns x 8 outputs n x 4*SL_DW_ROWS rows: lane = 4 k-columns,
// wave = a quarter of the rows (dy factors wave-uniform: scalar loads; each x vector feeds 8 outputs), waves combined through
// LDS, then ONE set of f32 atomics per workgroup into the zeroed outputs (the atomics were the cost of the first versions).
constexpr int SL_DW_ROWS = 32;
// SEG: the N output rows are slices of up to 4 separate parameters (the three stacked RVSA heads): row n of segment j goes to
// seg.dw[j] + (n - seg.row0[j]) * K -- accumulated straight into the parameter gradients (no stacked scratch, no clearing pass, no copy)
struct SlSegs {
    float* dw[4];
    float* db[4];
    int row0[5];
    int nseg;
};
// batched form (round 4): the same gradients of up to SL_BATCH independent problems of one shape (the stacked heads of a burst of RVSA
// blocks) in ONE launch -- blockIdx.z = problem * zsplit + row split
constexpr int SL_BATCH = 8;
struct SlBatch {
    const float* dy[SL_BATCH];
    const float* x[SL_BATCH];
    SlSegs seg[SL_BATCH];
    int zsplit;
};
template <bool SEG>
__device__ __forceinline__ void small_linear_dw_body(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dw, float* __restrict__ db, int R, int N, int K,
                                                     const SlSegs& seg, int zrow) {
    __shared__ float4 red[3][8][64];
    __shared__ float redb[3][8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = (blockIdx.x * 64 + lane) * 4, n0 = blockIdx.y * 8;
    const int r0 = (zrow * 4 + wave) * SL_DW_ROWS, r1 = (r0 + SL_DW_ROWS) < R ? (r0 + SL_DW_ROWS) : R;
    const bool kok = k < K;
    const int kc = kok ? k : 0;
    int nn[8];
    float4 s[8];
    float sb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        nn[q] = n0 + q < N ? n0 + q : N - 1;
        s[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        sb[q] = 0.f;
    }
#pragma unroll 8      // (round 4: 8 rows in flight; with 2 the 32 rows of a wave were 16 serialised round trips -- the launch is latency, not bytes)
    for (int r = r0; r < r1; ++r) {
        const float4 xv = load4(x + (int64_t)r * K + kc);
        const float* dr = dy + (int64_t)r * N;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float dv = dr[nn[q]];
            s[q].x += dv * xv.x; s[q].y += dv * xv.y; s[q].z += dv * xv.z; s[q].w += dv * xv.w;
            sb[q] += dv;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            red[wave - 1][q][lane] = s[q];
            if (lane == 0) redb[wave - 1][q] = sb[q];
        }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const float4 o = red[v][q][lane];
                s[q].x += o.x; s[q].y += o.y; s[q].z += o.z; s[q].w += o.w;
                sb[q] += redb[v][q];
            }
            float* dwrow = dw + (int64_t)(n0 + q) * K;
            float* dbp = db ? db + n0 + q : nullptr;
            if constexpr (SEG) {
                int j = 0;
                const int n = n0 + q < N ? n0 + q : N - 1;
#pragma unroll
                for (int t = 1; t < 4; ++t) j += (t < seg.nseg && n >= seg.row0[t]) ? 1 : 0;
                dwrow = seg.dw[j] + (int64_t)(n - seg.row0[j]) * K;
                dbp = seg.db[j] ? seg.db[j] + (n - seg.row0[j]) : nullptr;
            }
            if (kok && n0 + q < N) {
                float* o = dwrow + k;
                atomicAdd(o, s[q].x); atomicAdd(o + 1, s[q].y); atomicAdd(o + 2, s[q].z); atomicAdd(o + 3, s[q].w);
            }
            if (dbp && blockIdx.x == 0 && lane == 0 && n0 + q < N) atomicAdd(dbp, sb[q]);
        }
    }
}
template <bool SEG>
__global__ __launch_bounds__(256) void small_linear_dw_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dw, float* __restrict__ db, int R, int N, int K, SlSegs seg) {
    small_linear_dw_body<SEG>(dy, x, dw, db, R, N, K, seg, (int)blockIdx.z);
}
__global__ __launch_bounds__(256) void small_linear_dw_batched_kernel(SlBatch t, int R, int N, int K) {
    const int pi = __builtin_amdgcn_readfirstlane((int)blockIdx.z / t.zsplit);
    small_linear_dw_body<true>(t.dy[pi], t.x[pi], nullptr, nullptr, R, N, K, t.seg[pi], (int)blockIdx.z - pi * t.zsplit);
}

// ---- what the entry points refuse before any launch: the kernels keep R, N, K, C, Hp, Wp and the window count in an int (element offsets are int64), a grid takes 65535 in y and z
inline bool size_ok(int64_t v) { return v > 0 && v < INT32_MAX; }
// B images of (Hp, Wp) tokens of C channels: the window count is a grid x dimension and an int in the kernels, the element count an int64
inline bool windows_ok(int64_t B, int64_t Hp, int64_t Wp, int64_t C) {
    if (!size_ok(B) || !size_ok(Hp) || !size_ok(Wp) || !size_ok(C)) return false;
    const RvsaWindows win(Hp, Wp);
    return B < INT32_MAX / ((int64_t)win.nh * win.nw) && B * Hp * Wp <= INT64_MAX / C;      // (windows < 2^31: tokens < 49 * 2^31)
}
inline bool small_linear_ok(int64_t R, int64_t N, int64_t K) { return size_ok(R) && size_ok(N) && size_ok(K) && (K % 4) == 0; }
constexpr int64_t kGridYZ = 65535;
// grid of the dw kernels: 8 outputs in y, 4 * SL_DW_ROWS rows (times `count` problems) in z
inline int64_t sl_dw_zsplit(int64_t R) { return (R + 4 * SL_DW_ROWS - 1) / (4 * SL_DW_ROWS); }
inline bool sl_dw_grid_ok(int64_t R, int64_t N, int64_t count) { return (N + 7) / 8 <= kGridYZ && sl_dw_zsplit(R) * count <= kGridYZ; }

}  // namespace

// ---- the sampling heads of one RVSA block in ONE launch each way (VIT:344-358: zero pad, AvgPool2d(7, 7), LeakyReLU, three 1x1
// convolutions stacked as one (N = 5 * heads) x C linear layer).  One workgroup per window: the 49 token rows are averaged with all
// loads of a window row in flight (no branch around a load), the pooled vector stays in LDS, each wave produces a quarter of the N
// outputs.  Backward: dpooled = dsamp . W per window, times leaky'(avg) / 49, added to the 49 token rows of dx.
// (separately: pool 16.5 us + linear 26.8 us, linear-dx 12.6 us + pool-backward 19.4 us per block at ViT-L, B = 64)
template <typename T>
__global__ __launch_bounds__(256) void rvsa_sampling_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ avg, float* __restrict__ pooled, float* __restrict__ samp,
                                                               int Hp, int Wp, int C, int N, int pad_t, int pad_l, int nh, int nw) {
    extern __shared__ __attribute__((aligned(16))) float pl[];     // pooled row of this window
    // gridDim.y workgroups share a window: each pools it (the second reads come out of L2) and produces its share of the N outputs
    const int nper = ((N + (int)gridDim.y - 1) / (int)gridDim.y + 3) / 4 * 4, nlo = (int)blockIdx.y * nper, nhi = (nlo + nper) < N ? (nlo + nper) : N;
    rvsa_pool_window<T>(x, avg, pooled, Hp, Wp, C, pad_t, pad_l, nh, nw, (int)blockIdx.x, blockIdx.y == 0, (int)threadIdx.x, pl);
    __syncthreads();
    rvsa_heads<1>(w, bias, samp, C, N, nlo, nhi, (int)threadIdx.x >> 6, 4, (int)threadIdx.x & 63, pl, (int)blockIdx.x, 0, (int)gridDim.x);
}

// workgroup = (window, 64 channel quads); its 4 waves split the N head outputs of the dsamp . w product (N / 4 dependent-free weight
// loads each instead of N: with one quad per thread and the whole product in it the launch had one latency-bound wave per SIMD),
// meet in LDS, then split the 7 window rows of the dx update
template <typename T>
__global__ __launch_bounds__(256) void rvsa_sampling_bwd_kernel(const float* __restrict__ dsamp, const float* __restrict__ w, const float* __restrict__ avg,
                                                               T* __restrict__ dx, int Hp, int Wp, int C, int N, int pad_t, int pad_l, int nh, int nw) {
    extern __shared__ __attribute__((aligned(16))) float ds[];     // dsamp row of this window
    __shared__ float4 part[4][64];
    const int win = blockIdx.x;
    const int j = win % nw, i = (win / nw) % nh, b = win / (nw * nh);
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c4 = blockIdx.y * 64 + lane;
    const bool live = c4 < C / 4;
    for (int n = threadIdx.x; n < N; n += 256) ds[n] = dsamp[(int64_t)win * N + n];
    __syncthreads();
    const int nq = (N + 3) / 4, n0 = q * nq, n1 = (n0 + nq) < N ? (n0 + nq) : N;
    float4 d = make_float4(0, 0, 0, 0);
    if (live) {
#pragma unroll 4
        for (int n = n0; n < n1; ++n) {
            const float4 ww = load4(w + (int64_t)n * C + 4 * c4);
            const float t = ds[n];
            d.x += t * ww.x; d.y += t * ww.y; d.z += t * ww.z; d.w += t * ww.w;
        }
    }
    part[q][lane] = d;
    __syncthreads();
    if (!live) return;
    const float4 p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];   // fixed order: every wave gets the same bits
    d = make_float4((p0.x + p1.x) + (p2.x + p3.x), (p0.y + p1.y) + (p2.y + p3.y), (p0.z + p1.z) + (p2.z + p3.z), (p0.w + p1.w) + (p2.w + p3.w));
    const float4 a = load4(avg + (int64_t)win * C + 4 * c4);
    const float k = 1.0f / 49.0f;
    const float4 g = make_float4(d.x * (a.x > 0 ? k : 0.01f * k), d.y * (a.y > 0 ? k : 0.01f * k), d.z * (a.z > 0 ? k : 0.01f * k), d.w * (a.w > 0 ? k : 0.01f * k));
#pragma unroll 1
    for (int aa = q; aa < 7; aa += 4) {
        const int y = i * 7 + aa - pad_t;
        if (y < 0 || y >= Hp) continue;       // (uniform over the wave)
        float4 o[7];
#pragma unroll
        for (int bb = 0; bb < 7; ++bb) {
            const int xx = j * 7 + bb - pad_l;
            const int xc = (xx >= 0 && xx < Wp) ? xx : 0;
            o[bb] = load4(dx + (((int64_t)b * Hp + y) * Wp + xc) * C + 4 * c4);
        }
#pragma unroll
        for (int bb = 0; bb < 7; ++bb) {
            const int xx = j * 7 + bb - pad_l;
            if (xx >= 0 && xx < Wp)
                store4(dx + (((int64_t)b * Hp + y) * Wp + xx) * C + 4 * c4, make_float4(o[bb].x + g.x, o[bb].y + g.y, o[bb].z + g.z, o[bb].w + g.w));
        }
    }
}

// The same product, left per window: g (windows, C) f32 = (dsamp . w) * leaky'(avg) / 49 -- the LayerNorm backward that consumes dx adds it to
// every token row of the window while it reads that row anyway (mtp_layernorm_bwd_win), instead of a read-modify-write pass over (T, C).
__global__ __launch_bounds__(256) void rvsa_sampling_bwd_win_kernel(const float* __restrict__ dsamp, const float* __restrict__ w, const float* __restrict__ avg,
                                                                   float* __restrict__ g, int C, int N) {
    extern __shared__ __attribute__((aligned(16))) float ds[];     // dsamp row of this window
    __shared__ float4 part[4 * 64];
    rvsa_sampling_bwd_win_body(dsamp, w, avg, g, C, N, (int)blockIdx.x, (int)blockIdx.y * 64, true, (int)threadIdx.x, ds, part);
}

extern "C" int mtp_rvsa_sampling_bwd_win(const float* dsamp, const float* w, const float* avg, float* g, int64_t windows, int64_t C, int64_t N, mtp_stream_t stream) {
    if (!dsamp || !w || !avg || !g || !size_ok(windows) || !size_ok(C) || (C % 4) || N <= 0 || N > 4096) return MTP_ERR_ARG;
    const dim3 grid((unsigned)windows, (unsigned)((C / 4 + 63) / 64)), block(256);
    rvsa_sampling_bwd_win_kernel<<<grid, block, sizeof(float) * (size_t)N, (hipStream_t)stream>>>(dsamp, w, avg, g, (int)C, (int)N);
    return mtp_launch_status();
}

extern "C" int mtp_rvsa_sampling_fwd(const void* x, int dtype, const float* w, const float* bias, float* avg, float* pooled, float* samp,
                                     int64_t B, int64_t Hp, int64_t Wp, int64_t C, int64_t N, mtp_stream_t stream) {
    if (!x || !w || !avg || !pooled || !samp || !windows_ok(B, Hp, Wp, C) || (C % 4) || C > 8192 || !size_ok(N)) return MTP_ERR_ARG;
    const RvsaWindows win(Hp, Wp);
    // workgroups per window (each pools the window again -- L2 reads -- and makes its share of the N outputs): round 2 measured 24.1 / 18.1 / 19.3 us at 1 / 2 / 4;
    // round 6, with the weight loads of a pass in flight together: 16.8 / 16.3 / 21.1 / 26.2 us at 1 / 2 / 3 / 5 (17.5 before) -- the repeated pooling, not the
    // product, is what more workgroups per window cost
    constexpr int ysplit = 2;
    const dim3 grid((unsigned)(B * win.nh * win.nw), (unsigned)(N >= 16 * ysplit ? ysplit : 1)), block(256);
    const size_t lds = sizeof(float) * (size_t)C;
    return for_act(dtype, [&](auto t) {
        using T = decltype(t);
        rvsa_sampling_fwd_kernel<T><<<grid, block, lds, (hipStream_t)stream>>>((const T*)x, w, bias, avg, pooled, samp, (int)Hp, (int)Wp, (int)C, (int)N, win.pad_t, win.pad_l, win.nh, win.nw);
    });
}
/* dx (T, C) ACT += (dsamp (R, N) . w (N, C)) * leaky'(avg) / 49, broadcast over each window's tokens */
extern "C" int mtp_rvsa_sampling_bwd(const float* dsamp, const float* w, const float* avg, void* dx, int dtype,
                                     int64_t B, int64_t Hp, int64_t Wp, int64_t C, int64_t N, mtp_stream_t stream) {
    if (!dsamp || !w || !avg || !dx || !windows_ok(B, Hp, Wp, C) || (C % 4) || N <= 0 || N > 4096) return MTP_ERR_ARG;
    const RvsaWindows win(Hp, Wp);
    const dim3 grid((unsigned)(B * win.nh * win.nw), (unsigned)((C / 4 + 63) / 64)), block(256);
    const size_t lds = sizeof(float) * (size_t)N;
    return for_act(dtype, [&](auto t) {
        using T = decltype(t);
        rvsa_sampling_bwd_kernel<T><<<grid, block, lds, (hipStream_t)stream>>>(dsamp, w, avg, (T*)dx, (int)Hp, (int)Wp, (int)C, (int)N, win.pad_t, win.pad_l, win.nh, win.nw);
    });
}

extern "C" int mtp_rvsa_pool_fwd(const void* x, int dtype, float* avg, float* pooled, int64_t B, int64_t Hp, int64_t Wp, int64_t C, mtp_stream_t stream) {
    if (!x || !avg || !pooled || !windows_ok(B, Hp, Wp, C) || (C % 4)) return MTP_ERR_ARG;
    const RvsaWindows win(Hp, Wp);
    const dim3 grid((unsigned)(B * win.nh * win.nw), (unsigned)((C / 4 + 255) / 256));
    return for_act(dtype, [&](auto t) {
        using T = decltype(t);
        rvsa_pool_fwd_kernel<T><<<grid, kThreads, 0, (hipStream_t)stream>>>((const T*)x, avg, pooled, (int)Hp, (int)Wp, (int)C, win.pad_t, win.pad_l, win.nh, win.nw);
    });
}
extern "C" int mtp_rvsa_pool_bwd(const float* dpooled, const float* avg, void* dx, int dtype, int accumulate, int64_t B, int64_t Hp, int64_t Wp, int64_t C, mtp_stream_t stream) {
    if (!dpooled || !avg || !dx || !windows_ok(B, Hp, Wp, C) || (C % 4)) return MTP_ERR_ARG;
    const RvsaWindows win(Hp, Wp);
    return for_act(dtype, [&](auto t) {
        using T = decltype(t);
        rvsa_pool_bwd_kernel<T><<<blocks_for(B * Hp * Wp * C / 4, kThreads, 8192), kThreads, 0, (hipStream_t)stream>>>(dpooled, avg, (T*)dx, accumulate, (int)B, (int)Hp, (int)Wp, (int)C,
                                                                                                                      win.pad_t, win.pad_l, win.nh, win.nw);
    });
}

extern "C" int mtp_small_linear_fwd(const float* x, const float* w, const float* b, float* y, int64_t R, int64_t N, int64_t K, mtp_stream_t stream) {
    if (!x || !w || !y || !small_linear_ok(R, N, K)) return MTP_ERR_ARG;      // (K = 0 would pass K % 4 and clamp the weight index to -1)
    if (K <= 1024)
        small_linear_fwd_kernel<4, 4><<<dim3((unsigned)((R + 3) / 4)), kThreads, 0, (hipStream_t)stream>>>(x, w, b, y, (int)R, (int)N, (int)K);
    else if (K <= 2048)
        small_linear_fwd_kernel<2, 8><<<dim3((unsigned)((R + 1) / 2)), kThreads, 0, (hipStream_t)stream>>>(x, w, b, y, (int)R, (int)N, (int)K);
    else
        small_linear_fwd_generic_kernel<<<(unsigned)R, kThreads, 0, (hipStream_t)stream>>>(x, w, b, y, (int)N, (int)K);
    return mtp_launch_status();
}
extern "C" int mtp_small_linear_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int64_t R, int64_t N, int64_t K, mtp_stream_t stream) {
    if (!x || !w || !dy || !small_linear_ok(R, N, K)) return MTP_ERR_ARG;
    if ((dx && (R + 3) / 4 > kGridYZ) || (dw && !sl_dw_grid_ok(R, N, 1))) return MTP_ERR_ARG;      // before the clearing passes: a refusal writes nothing
    hipStream_t s = (hipStream_t)stream;
    if (dx) small_linear_dx_kernel<<<dim3((unsigned)((K + 1023) / 1024), (unsigned)((R + 3) / 4)), kThreads, 0, s>>>(dy, w, dx, (int)R, (int)N, (int)K);
    if (dw) {
        if (db == dw + N * K) {   // one buffer [dw | db]: one clearing pass
            (void)hipMemsetAsync(dw, 0, sizeof(float) * (size_t)(N * K + N), s);
        } else {
            (void)hipMemsetAsync(dw, 0, sizeof(float) * (size_t)(N * K), s);
            if (db) (void)hipMemsetAsync(db, 0, sizeof(float) * (size_t)N, s);
        }
        const dim3 grid((unsigned)((K + 255) / 256), (unsigned)((N + 7) / 8), (unsigned)sl_dw_zsplit(R));
        small_linear_dw_kernel<false><<<grid, kThreads, 0, s>>>(dy, x, dw, db, (int)R, (int)N, (int)K, SlSegs{});
    }
    return mtp_launch_status();
}
/* the weight / bias gradients of nseg <= 4 layers stacked along N, ACCUMULATED into their own (rows_j, K) / (rows_j) f32 buffers:
 * dw[j] += dy[:, r0_j : r0_j + rows_j]^T x.  Host arrays; db[j] may be NULL. */
extern "C" int mtp_small_linear_dw_segments(const float* x, const float* dy, int64_t R, int64_t N, int64_t K, int nseg, const int64_t* seg_rows,
                                            float* const* dw, float* const* db, mtp_stream_t stream) {
    if (!x || !dy || !seg_rows || !dw || !small_linear_ok(R, N, K) || !sl_dw_grid_ok(R, N, 1) || nseg < 1 || nseg > 4) return MTP_ERR_ARG;
    SlSegs seg{};
    int64_t r = 0;
    for (int j = 0; j < nseg; ++j) {
        if (!dw[j] || seg_rows[j] <= 0) return MTP_ERR_ARG;
        seg.dw[j] = dw[j];
        seg.db[j] = db ? db[j] : nullptr;
        seg.row0[j] = (int)r;
        r += seg_rows[j];
    }
    if (r != N) return MTP_ERR_ARG;
    seg.row0[nseg] = (int)N;
    seg.nseg = nseg;
    const dim3 grid((unsigned)((K + 255) / 256), (unsigned)((N + 7) / 8), (unsigned)sl_dw_zsplit(R));
    small_linear_dw_kernel<true><<<grid, kThreads, 0, (hipStream_t)stream>>>(dy, x, (float*)nullptr, (float*)nullptr, (int)R, (int)N, (int)K, seg);
    return mtp_launch_status();
}

/* the same for `count` <= 8 problems of one shape in one launch: xs / dys host arrays of device pointers, dw / db host arrays of
 * count * nseg device pointers (problem-major) */
extern "C" int mtp_small_linear_dw_segments_batched(const float* const* xs, const float* const* dys, int count, int64_t R, int64_t N, int64_t K, int nseg,
                                                    const int64_t* seg_rows, float* const* dw, float* const* db, mtp_stream_t stream) {
    if (!xs || !dys || !seg_rows || !dw || count <= 0 || count > SL_BATCH || !small_linear_ok(R, N, K) || !sl_dw_grid_ok(R, N, count) || nseg < 1 || nseg > 4) return MTP_ERR_ARG;
    SlBatch t{};
    for (int i = 0; i < count; ++i) {
        if (!xs[i] || !dys[i]) return MTP_ERR_ARG;
        t.x[i] = xs[i];
        t.dy[i] = dys[i];
        int64_t r = 0;
        for (int j = 0; j < nseg; ++j) {
            if (!dw[i * nseg + j] || seg_rows[j] <= 0) return MTP_ERR_ARG;
            t.seg[i].dw[j] = dw[i * nseg + j];
            t.seg[i].db[j] = db ? db[i * nseg + j] : nullptr;
            t.seg[i].row0[j] = (int)r;
            r += seg_rows[j];
        }
        if (r != N) return MTP_ERR_ARG;
        t.seg[i].row0[nseg] = (int)N;
        t.seg[i].nseg = nseg;
    }
    t.zsplit = (int)sl_dw_zsplit(R);
    small_linear_dw_batched_kernel<<<dim3((unsigned)((K + 255) / 256), (unsigned)((N + 7) / 8), (unsigned)(t.zsplit * count)), kThreads, 0, (hipStream_t)stream>>>(t, (int)R, (int)N, (int)K);
    return mtp_launch_status();
}
