// GEMM kernels for gfx950: bf16 MFMA (v_mfma_f32_16x16x32_bf16) and exact-f32 MFMA (v_mfma_f32_16x16x4_f32),
// one source for both precisions: everything is expressed in 16-byte "chunks" along the contraction dim
// (8 bf16 or 4 f32).  A K-step = 4 chunks: lane group g = lane>>4 owns chunk g of both operands, which is
// exactly the MFMA operand layout for bf16 (8 consecutive k per lane) and, for f32, a consistent k-permutation
// across 4 chained 16x16x4 MFMAs (k = 16*step + 4*g + e for MFMA e).
//
// Tile: 128 x 128 x 8 chunks (BK = 64 bf16 / 32 f32), 256 threads = 4 waves as 2(M) x 2(N), each wave 64x64 =
// 4x4 MFMA tiles.  LDS image per operand: [128 rows][8 chunk slots] (128 B rows), slot = chunk ^ (row & 7):
// conflict-free for the ds_read_b128 fragment reads (16-lane groups) and for the staging writes.
// MFMA operands are swapped (A-operand = weight rows n, B-operand = activation rows m) so each lane ends up with
// 4 consecutive output columns of one row -> 8/16-byte epilogue accesses.
//
// NT  C[m][n] = sum_k A[m][k] B[n][k]   : both operands K-contiguous -> direct-to-LDS loads (global_load_lds x16B),
//                                         swizzle applied on the per-lane SOURCE address (LDS image is lane-linear).
//                                         Default kernel: ONE 32 KiB stage, 4 workgroups per CU (gemm_nt_sb_kernel).
// TN  C[m][n] = sum_k A[k][m] B[k][n]   : weight gradients, split-K over gridDim.y.  bf16 + complete tiles: both tiles go to
//                                         LDS untransposed (LDS-DMA) and the fragments come out of ds_read_b64_tr_b16
//                                         (gemm_tn_tr_kernel); f32 / ragged shapes: tiles are transposed in registers (ExE
//                                         blocks) between the coalesced global loads and the ds_write_b128.
#include "gemm_common.h"

namespace {

constexpr int BM = 128;
constexpr int BN = 128;
constexpr int NT_THREADS = 256;
constexpr int ROW_BYTES = 128;              // 8 chunks x 16 B
constexpr int OPER_BYTES = BM * ROW_BYTES;  // 16 KiB per operand tile
constexpr int STAGE_BYTES = 2 * OPER_BYTES; // A + B
constexpr int LDS_BYTES = 2 * STAGE_BYTES;  // double buffered: 64 KiB -> 2 blocks / CU

__device__ __forceinline__ int lds_off(int row, int chunk) { return row * ROW_BYTES + ((chunk ^ (row & 7)) << 4); }

// out[i] = sum_s part[s][i]   (float4 granules; deterministic split-K reduction)
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t n4, int split) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 s = *reinterpret_cast<const float4*>(part + 4 * i);
        for (int z = 1; z < split; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(part + 4 * (i + (int64_t)z * n4));
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4*>(out + 4 * i) = s;
    }
}

// ---- one 128x128 tile's worth of MFMAs out of one LDS stage ------------------------------------------------------
template <typename T>
__device__ __forceinline__ void compute_stage(const char* sA, const char* sB, f32x4_t (&acc)[4][4], int wm, int wn, int lane) {
    const int fr = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        uint4 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = *reinterpret_cast<const uint4*>(sA + lds_off(wm * 64 + i * 16 + fr, ks * 4 + g));
            b[i] = *reinterpret_cast<const uint4*>(sB + lds_off(wn * 64 + i * 16 + fr, ks * 4 + g));
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) Mma<T>::run(acc[ni][mi], b[ni], a[mi]);
    }
}

// ---- NT staging, direct to LDS -----------------------------------------------------------------------------------
// wave w fills rows [32w, 32w+32) of both operand tiles with 4 + 4 global_load_lds_dwordx4 (1 KiB each):
// lane l -> LDS slot (row = base + (l>>3), slot = l&7) receives global chunk (slot ^ (row&7)) of that row.
template <typename T>
__device__ __forceinline__ void stage_nt_glds(const KArgs& p, char* sA, char* sB, int m0, int n0, int kt, int wave, int lane) {
    constexpr int E = Elem<T>::kPerChunk;
    const int k0 = kt * 8 * E;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rbase = wave * 32 + i * 8;
        const int row = rbase + (lane >> 3);
        const int chunk = (lane & 7) ^ (row & 7);
        int ra = m0 + row; ra = ra < p.M ? ra : p.M - 1;
        int rb = n0 + row; rb = rb < p.N ? rb : p.N - 1;
        const char* ga = p.A + ((int64_t)ra * p.lda + k0 + chunk * E) * (int64_t)sizeof(T);
        const char* gb = p.B + ((int64_t)rb * p.ldb + k0 + chunk * E) * (int64_t)sizeof(T);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ga,
                                         (__attribute__((address_space(3))) void*)(sA + rbase * ROW_BYTES), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gb,
                                         (__attribute__((address_space(3))) void*)(sB + rbase * ROW_BYTES), 16, 0, 0);
    }
}

// ---- NT staging through registers (MTP_GEMM_NT_REG_STAGED; also handles ragged K) --------------------------------------------------
template <typename T>
struct NtRegs {
    uint4 a[4], b[4];
    uint32_t ok;    // bits 0-3: a[i] in range, bits 4-7: b[i] in range
};
template <typename T>
__device__ __forceinline__ void load_nt_regs(const KArgs& p, NtRegs<T>& r, int m0, int n0, int kt, int tid) {
    constexpr int E = Elem<T>::kPerChunk;
    const int c = tid & 7;
    const int k = kt * 8 * E + c * E;
    const bool kok = k < p.K;
    uint32_t okm = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (tid >> 3) + 32 * i;
        const bool oka = kok && (m0 + row < p.M), okb = kok && (n0 + row < p.N);
        okm |= (oka ? (1u << i) : 0u) | (okb ? (16u << i) : 0u);
        r.a[i] = ldg16(p.A + (oka ? ((int64_t)(m0 + row) * p.lda + k) * (int64_t)sizeof(T) : 0));
        r.b[i] = ldg16(p.B + (okb ? ((int64_t)(n0 + row) * p.ldb + k) * (int64_t)sizeof(T) : 0));
    }
    r.ok = okm;
}
__device__ __forceinline__ uint4 mask4(const uint4& v, uint32_t okm, int e) {
    const uint32_t m = (okm >> e) & 1u ? 0xffffffffu : 0u;
    return make_uint4(v.x & m, v.y & m, v.z & m, v.w & m);
}
template <typename T>
__device__ __forceinline__ void store_nt_regs(const NtRegs<T>& r, char* sA, char* sB, int tid) {
    const int c = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (tid >> 3) + 32 * i;
        *reinterpret_cast<uint4*>(sA + lds_off(row, c)) = mask4(r.a[i], r.ok, i);
        *reinterpret_cast<uint4*>(sB + lds_off(row, c)) = mask4(r.b[i], r.ok, 4 + i);
    }
}

template <typename T, typename Tout, int EPI>
__global__ __launch_bounds__(NT_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_nt_kernel(KArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int tile = (p.order & 1) ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    const int tiles_m_ = (int)gridDim.x / p.tiles_n;
    const int m0 = ((p.order & 2) ? (tile % tiles_m_) : (tile / p.tiles_n)) * BM, n0 = ((p.order & 2) ? (tile / tiles_m_) : (tile % p.tiles_n)) * BN;

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nk = p.k_tiles;
    NtRegs<T> r;
    load_nt_regs<T>(p, r, m0, n0, 0, tid);
    store_nt_regs<T>(r, smem, smem + OPER_BYTES, tid);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        char* cur = smem + (kt & 1) * STAGE_BYTES;
        char* nxt = smem + ((kt + 1) & 1) * STAGE_BYTES;
        load_nt_regs<T>(p, r, m0, n0, kt + 1 < nk ? kt + 1 : kt, tid);   // unconditional prefetch (see gemm_tn_kernel)
        __builtin_amdgcn_sched_barrier(0);
        compute_stage<T>(cur, cur + OPER_BYTES, acc, wm, wn, lane);
        __builtin_amdgcn_sched_barrier(0);
        store_nt_regs<T>(r, nxt, nxt + OPER_BYTES, tid);
    }
    epilogue<Tout, EPI, 4>(p, acc, m0 + wm * 64, n0 + wn * 64, lane);
}

// Single-LDS-stage variant (32 KiB -> 4 workgroups / 16 waves per CU): thread-level parallelism across resident workgroups
// covers each workgroup's load latency instead of a deeper software pipeline.
template <typename T, typename Tout, int EPI>
__global__ __launch_bounds__(NT_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_nt_sb_kernel(KArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int tile = (p.order & 1) ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    int m0, n0;
    if (p.order & 2) {   // grouped order: panels of 8 tile rows, rows fastest inside a panel (an XCD's ~128 resident tiles cover
                         // 8 rows x 16 columns instead of 5 rows x all columns: the B tiles are shared by 8 instead of ~5 tiles)
        const int tiles_m = (int)gridDim.x / p.tiles_n, per = 8 * p.tiles_n;
        const int grp = tile / per, r = tile - grp * per;
        const int gm = (tiles_m - grp * 8) < 8 ? (tiles_m - grp * 8) : 8;
        m0 = (grp * 8 + r % gm) * BM;
        n0 = (r / gm) * BN;
    } else {
        m0 = (tile / p.tiles_n) * BM;
        n0 = (tile % p.tiles_n) * BN;
    }
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < p.k_tiles; ++kt) {
        stage_nt_glds<T>(p, smem, smem + OPER_BYTES, m0, n0, kt, wave, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        compute_stage<T>(smem, smem + OPER_BYTES, acc, wm, wn, lane);
        __syncthreads();
    }
    epilogue<Tout, EPI, 4>(p, acc, m0 + wm * 64, n0 + wn * 64, lane);
}

// 256 x 128 tile, 8 waves (4 x 2, 64 x 64 each), one 48 KiB stage, 2 workgroups per CU: same occupancy and per-wave work as
// the kernel above with 25 % fewer L2->LDS bytes per flop (A tile shared by 2 x more columns).  Selected for wide N only
// (the tile count of N = 1024 problems would leave CUs idle).
constexpr int NT8_THREADS = 512;
constexpr int NT8_BM = 256;
constexpr int NT8_STAGE_BYTES = NT8_BM * ROW_BYTES + OPER_BYTES;
template <typename T, typename Tout, int EPI>
__global__ __launch_bounds__(NT8_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_nt_sb8_kernel(KArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int E = Elem<T>::kPerChunk;
    char* sA = smem;
    char* sB = smem + NT8_BM * ROW_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int tile = (p.order & 1) ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    int m0, n0;
    if (p.order & 2) {
        const int tiles_m = (int)gridDim.x / p.tiles_n, per = 8 * p.tiles_n;
        const int grp = tile / per, r = tile - grp * per;
        const int gm = (tiles_m - grp * 8) < 8 ? (tiles_m - grp * 8) : 8;
        m0 = (grp * 8 + r % gm) * NT8_BM;
        n0 = (r / gm) * BN;
    } else {
        m0 = (tile / p.tiles_n) * NT8_BM;
        n0 = (tile % p.tiles_n) * BN;
    }
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < p.k_tiles; ++kt) {
        const int k0 = kt * 8 * E;
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // A: wave w fills rows [32w, 32w + 32)
            const int rbase = wave * 32 + i * 8, row = rbase + (lane >> 3), chunk = (lane & 7) ^ (row & 7);
            int ra = m0 + row; ra = ra < p.M ? ra : p.M - 1;
            const char* ga = p.A + ((int64_t)ra * p.lda + k0 + chunk * E) * (int64_t)sizeof(T);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ga,
                                             (__attribute__((address_space(3))) void*)(sA + rbase * ROW_BYTES), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {   // B: wave w fills rows [16w, 16w + 16)
            const int rbase = wave * 16 + i * 8, row = rbase + (lane >> 3), chunk = (lane & 7) ^ (row & 7);
            int rb = n0 + row; rb = rb < p.N ? rb : p.N - 1;
            const char* gb = p.B + ((int64_t)rb * p.ldb + k0 + chunk * E) * (int64_t)sizeof(T);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gb,
                                             (__attribute__((address_space(3))) void*)(sB + rbase * ROW_BYTES), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        compute_stage<T>(sA, sB, acc, wm, wn, lane);
        __syncthreads();
    }
    epilogue<Tout, EPI, 4>(p, acc, m0 + wm * 64, n0 + wn * 64, lane);
}

// ---- TN staging: ExE register transposes ------------------------------------------------------------------------------
// Operand source is (Kc, X) row-major, X = M or N contiguous.  Item = one ExE block (E k-rows x E x-columns):
// kb = blk & 7 (LDS chunk column), xb = blk >> 3 (E-wide column group); lanes with consecutive xb read consecutive
// 16-B pieces of a source row, lanes with consecutive kb write the 8 chunk slots of one LDS row (conflict-free).
template <typename T>
struct TnItems;
template <>
struct TnItems<bf16_t> {
    static constexpr int kItems = 1;   // 2 operands x 128 blocks / 256 threads
};
template <>
struct TnItems<float> {
    static constexpr int kItems = 2;   // 2 operands x 256 blocks / 256 threads
};

template <typename T>
struct TnRegs {
    uint4 v[TnItems<T>::kItems][Elem<T>::kPerChunk];
    uint32_t ok[TnItems<T>::kItems];   // bit e: row e of the block is in range (else it is zeroed in the store phase)
};

template <typename T, bool FULL>
__device__ __forceinline__ void load_tn_regs(const KArgs& p, TnRegs<T>& r, int m0, int n0, int kt, int tid) {
    constexpr int E = Elem<T>::kPerChunk;
    constexpr int NB = 8 * (BM / E);   // blocks per operand
#pragma unroll
    for (int it = 0; it < TnItems<T>::kItems; ++it) {
        const int idx = tid + NT_THREADS * it;
        const int oper = idx / NB, blk = idx % NB;
        const int kb = blk & 7, xb = blk >> 3;
        const char* src = oper ? p.B : p.A;
        const int64_t ld = oper ? p.ldb : p.lda;
        const int x = (oper ? n0 : m0) + xb * E;
        const int xlim = oper ? p.N : p.M;
        // Unconditional loads from CLAMPED OFFSETS; out-of-range rows are zeroed later, in the store phase.  (`cond ? load : 0`
        // makes hipcc branch around every load with a vmcnt(0) inside; a select between two POINTERS is lowered to exec-masked
        // blocks as well; a select on the loaded VALUE here would pull the vmcnt wait in front of the MFMAs.)
        // FULL (every tile complete: the training shapes) has no predicates at all -- hipcc keeps re-introducing exec-masked
        // blocks + early vmcnt waits around predicated loads, whichever way the predicate is written.
        uint32_t okm = 0;
        if (FULL) {
            const char* base = src + ((int64_t)(kt * 8 * E + kb * E) * ld + x) * (int64_t)sizeof(T);
#pragma unroll
            for (int e = 0; e < E; ++e) r.v[it][e] = ldg16(base + (int64_t)e * ld * (int64_t)sizeof(T));
            okm = 0xffu;
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = kt * 8 * E + kb * E + e;
                const bool ok = (k < p.K) && (x < xlim);
                okm |= ok ? (1u << e) : 0u;
                const int64_t off = ok ? ((int64_t)k * ld + x) * (int64_t)sizeof(T) : 0;
                r.v[it][e] = ldg16(src + off);
            }
        }
        r.ok[it] = okm;
    }
}


__device__ __forceinline__ uint32_t dw(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

template <typename T>
__device__ __forceinline__ void store_tn_regs(const TnRegs<T>& r, char* smem_stage, int tid);

template <>
__device__ __forceinline__ void store_tn_regs<float>(const TnRegs<float>& r, char* st, int tid) {
    constexpr int E = 4, NB = 8 * (BM / E);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + NT_THREADS * it;
        const int oper = idx / NB, blk = idx % NB;
        const int kb = blk & 7, xb = blk >> 3;
        char* s = st + oper * OPER_BYTES;
#pragma unroll
        for (int f = 0; f < 4; ++f) {   // out row f = column f of the 4x4 block
            const uint32_t okm = r.ok[it];
            uint4 o = make_uint4((okm & 1u) ? dw(r.v[it][0], f) : 0u, (okm & 2u) ? dw(r.v[it][1], f) : 0u,
                                 (okm & 4u) ? dw(r.v[it][2], f) : 0u, (okm & 8u) ? dw(r.v[it][3], f) : 0u);
            *reinterpret_cast<uint4*>(s + lds_off(xb * E + f, kb)) = o;
        }
    }
}

template <>
__device__ __forceinline__ void store_tn_regs<bf16_t>(const TnRegs<bf16_t>& r, char* st, int tid) {
    constexpr int E = 8, NB = 8 * (BM / E);
    const int oper = tid / NB, blk = tid % NB;
    const int kb = blk & 7, xb = blk >> 3;
    char* s = st + oper * OPER_BYTES;
    uint4 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = mask4(r.v[0][e], r.ok[0], e);
#pragma unroll
    for (int d = 0; d < 4; ++d) {       // source dword d holds columns f = 2d (lo half), 2d+1 (hi half)
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // output dword q holds k = 2q (lo), 2q+1 (hi)
            const uint32_t e0 = dw(v[2 * q], d), e1 = dw(v[2 * q + 1], d);
            lo[q] = (e0 & 0xffffu) | (e1 << 16);
            hi[q] = (e0 >> 16) | (e1 & 0xffff0000u);
        }
        *reinterpret_cast<uint4*>(s + lds_off(xb * E + 2 * d, kb)) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        *reinterpret_cast<uint4*>(s + lds_off(xb * E + 2 * d + 1, kb)) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    }
}

template <typename T, bool FULL>
__global__ __launch_bounds__(NT_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_tn_kernel(KArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int tile = (p.order & 1) ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    const int tiles_m_ = (int)gridDim.x / p.tiles_n;
    const int m0 = ((p.order & 2) ? (tile % tiles_m_) : (tile / p.tiles_n)) * BM, n0 = ((p.order & 2) ? (tile / tiles_m_) : (tile % p.tiles_n)) * BN;
    const int kt0 = blockIdx.y * p.k_tiles_per_split;
    int kt1 = kt0 + p.k_tiles_per_split;
    kt1 = kt1 < p.k_tiles ? kt1 : p.k_tiles;
    if (kt0 >= kt1) return;
    p.C += (int64_t)blockIdx.y * p.split_stride * (int64_t)sizeof(float);

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    TnRegs<T> r;
    load_tn_regs<T, FULL>(p, r, m0, n0, kt0, tid);
    store_tn_regs<T>(r, smem, tid);
    for (int kt = kt0; kt < kt1; ++kt) {
        __syncthreads();
        char* cur = smem + ((kt - kt0) & 1) * STAGE_BYTES;
        char* nxt = smem + ((kt - kt0 + 1) & 1) * STAGE_BYTES;
        // The prefetch is UNCONDITIONAL (the last iteration re-loads its own tile into the idle buffer): an `if` around it
        // turns the registers into loop phis and hipcc copies them -- i.e. waits for the loads -- before the MFMAs.
        const int ktn = kt + 1 < kt1 ? kt + 1 : kt;
        load_tn_regs<T, FULL>(p, r, m0, n0, ktn, tid);
        __builtin_amdgcn_sched_barrier(0);   // keep the 8 global loads ahead of the MFMAs (hipcc otherwise sinks them to their use)
        compute_stage<T>(cur, cur + OPER_BYTES, acc, wm, wn, lane);
        __builtin_amdgcn_sched_barrier(0);
        store_tn_regs<T>(r, nxt, tid);
    }
    epilogue<float, MTP_EPI_BIAS, 4>(p, acc, m0 + wm * 64, n0 + wn * 64, lane);
}

// ---- TN, bf16, complete tiles: LDS-DMA staging of the UNtransposed tiles + hardware transpose reads ----------------------
// The register-transposing kernels above spend more LDS-pipe cycles on their 8 ds_write_b128 per thread and k-tile (13 cycles
// each) plus the fragment reads than the SIMDs spend on MFMAs.  Here both operand tiles go HBM -> LDS as they lie in memory
// ([64 t rows][128 x] bf16 = 256-B rows, global_load_lds x16B, no VGPR/ds_write traffic) and the MFMA fragments come out of
// ds_read_b64_tr_b16: a 16-lane group hands in the addresses of a [4 t][16 x] block (lane i: row i>>2, columns 4(i&3)..+3)
// and lane i gets column i, rows 0..3 -- measured on gfx950 with tools/probes/tr_probe.hip.  Two reads = the 8 consecutive k of
// one MFMA operand.  Swizzle: 32-B slot pair ^= f(t), f = (t&3) | (t>>3 & 1)<<2, so that the 8 rows a 32-lane group touches
// ({0..3, 8..11} + const) fall on 8 different bank octets; applied on the per-lane SOURCE address of the DMA.
typedef short tr_v4s __attribute__((ext_vector_type(4)));
constexpr int TR_ROW_BYTES = 256;

__device__ __forceinline__ void stage_tn_glds(const KArgs& p, char* sA, char* sB, int m0, int n0, int kt, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rbase = wave * 16 + i * 4;
        const int row = rbase + (lane >> 4);
        const int f = (row & 3) | ((row >> 1) & 4);
        const int chunk = (lane & 15) ^ (f << 1);
        const int64_t t = (int64_t)kt * 64 + row;
        // edge tiles (M or N not a multiple of 128, e.g. InternImage's 192 channels): columns past the matrix edge re-read the last
        // complete 16-byte chunk of the row; their products land in output columns the epilogue never stores
        int ca = m0 + chunk * 8, cb = n0 + chunk * 8;
        ca = ca < p.M - 8 ? ca : p.M - 8;
        cb = cb < p.N - 8 ? cb : p.N - 8;
        const char* ga = p.A + (t * p.lda + ca) * 2;
        const char* gb = p.B + (t * p.ldb + cb) * 2;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ga,
                                         (__attribute__((address_space(3))) void*)(sA + rbase * TR_ROW_BYTES), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gb,
                                         (__attribute__((address_space(3))) void*)(sB + rbase * TR_ROW_BYTES), 16, 0, 0);
    }
}

__device__ __forceinline__ uint4 tr_frag(const char* s, int off) {
    const tr_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr_v4s*)(s + off));
    const tr_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr_v4s*)(s + off + 4 * TR_ROW_BYTES));
    const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
    return make_uint4(l.x, l.y, h.x, h.y);
}

__device__ __forceinline__ void compute_stage_tr(const char* sA, const char* sB, f32x4_t (&acc)[4][4], int wm, int wn, int lane) {
    const int i = lane & 15, g = lane >> 4;
    const int f = (i >> 2) | ((g & 1) << 2);
    const int rowoff = (8 * g + (i >> 2)) * TR_ROW_BYTES + ((i >> 1) & 1) * 16 + (i & 1) * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        uint4 a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = tr_frag(sA, rowoff + (((q | (wm << 2)) ^ f) << 5) + ks * 32 * TR_ROW_BYTES);
            b[q] = tr_frag(sB, rowoff + (((q | (wn << 2)) ^ f) << 5) + ks * 32 * TR_ROW_BYTES);
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) Mma<bf16_t>::run(acc[ni][mi], b[ni], a[mi]);
    }
}

__global__ __launch_bounds__(NT_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_tn_tr_kernel(KArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int tile = (p.order & 1) ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    // an XCD owns a contiguous tile range and streams, per split, its share of one operand but ALL panels of the other one:
    // walk the tiles so that the replicated operand is the smaller one (order bit 1: M fastest, for N > M, e.g. dW of fc2)
    const int tiles_m = (int)gridDim.x / p.tiles_n;
    const int m0 = ((p.order & 2) ? tile % tiles_m : tile / p.tiles_n) * BM, n0 = ((p.order & 2) ? tile / tiles_m : tile % p.tiles_n) * BN;
    const int kt0 = blockIdx.y * p.k_tiles_per_split;
    int kt1 = kt0 + p.k_tiles_per_split;
    kt1 = kt1 < p.k_tiles ? kt1 : p.k_tiles;
    if (kt0 >= kt1) return;
    p.C += (int64_t)blockIdx.y * p.split_stride * (int64_t)sizeof(float);
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // bias-gradient by-product: the workgroups of tile column 0 also add up the rows of their A (= dY) tiles out of LDS
    // (thread = 16-B slot tid&15 of rows (tid>>4) + 16j; all four rows share one swizzle, i.e. one 8-column chunk)
    const bool do_colsum = p.colsum != nullptr && n0 == 0;
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int kt = kt0; kt < kt1; ++kt) {
        stage_tn_glds(p, smem, smem + OPER_BYTES, m0, n0, kt, wave, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        compute_stage_tr(smem, smem + OPER_BYTES, acc, wm, wn, lane);
        if (do_colsum) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint4 v = *reinterpret_cast<const uint4*>(smem + ((tid >> 4) + 16 * j) * TR_ROW_BYTES + (tid & 15) * 16);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cs[2 * e] += __uint_as_float(w[e] << 16);
                    cs[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u);
                }
            }
        }
        __syncthreads();
    }
    if (do_colsum) {   // (after the loop's last barrier nobody reads the stage any more)
        float* red = reinterpret_cast<float*>(smem);
        const int rg = tid >> 4, f = (rg & 3) | ((rg >> 1) & 4), chunk = (tid & 15) ^ (f << 1);
        *reinterpret_cast<float4*>(red + rg * BM + chunk * 8) = make_float4(cs[0], cs[1], cs[2], cs[3]);
        *reinterpret_cast<float4*>(red + rg * BM + chunk * 8 + 4) = make_float4(cs[4], cs[5], cs[6], cs[7]);
        __syncthreads();
        if (tid < BM) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s += red[r * BM + tid];
            if (m0 + tid < p.M) atomicAdd(p.colsum + m0 + tid, s);
        }
    }
    epilogue<float, MTP_EPI_BIAS, 4>(p, acc, m0 + wm * 64, n0 + wn * 64, lane);
}

template <typename T>
int fill_common(const mtp_gemm_args* a, KArgs& k) {
    constexpr int E = Elem<T>::kPerChunk;
    if (!a->A || !a->B || !a->C || a->M <= 0 || a->N <= 0 || a->K <= 0) return MTP_ERR_ARG;
    if (a->M > INT32_MAX || a->N > INT32_MAX || a->K > INT32_MAX) return MTP_ERR_ARG;
    if ((a->lda % E) || (a->ldb % E) || (a->ldc % 4) || (a->N % 4)) return MTP_ERR_ARG;
    if (((uintptr_t)a->A | (uintptr_t)a->B | (uintptr_t)a->C) & 15) return MTP_ERR_ARG;
    k.A = (const char*)a->A; k.B = (const char*)a->B; k.C = (char*)a->C;
    k.M = (int)a->M; k.N = (int)a->N; k.K = (int)a->K;
    k.lda = a->lda; k.ldb = a->ldb; k.ldc = a->ldc;
    k.bias = a->bias; k.bias_mod = (int)a->bias_mod;
    k.res = a->res; k.res_ld = a->res_ld; k.res_mod = (int)a->res_mod;
    k.rowscale = a->rowscale; k.rows_per_sample = (int)(a->rows_per_sample > 0 ? a->rows_per_sample : 1);
    k.aux = (char*)a->aux; k.aux_ld = a->aux_ld;
    k.tiles_n = (int)((a->N + BN - 1) / BN);
    k.k_tiles = (int)((a->K + 8 * E - 1) / (8 * E));
    k.k_tiles_per_split = k.k_tiles;
    k.atomic_out = 0;
    k.order = 0;            // the launchers set it
    k.split_stride = 0;
    k.colsum = nullptr;
    return 0;
}

// What mtp_gemm_nt runs a problem on, for a stream of `cus` CUs: the launch switches on it and mtp_gemm_nt_plan reports it.  All families are
// bit-identical, so a wrong turn here is a silent slowdown: tests/test_gemm_plan_host.py pins the decisions.
NtPlan nt_plan(const mtp_gemm_args* a, const KArgs& k, int cus) {
    // the one place that reads the NT flags of args.variant (mtp_gemm_variant)
    const int ord = (a->variant & MTP_GEMM_ORDER_MASK) >> MTP_GEMM_ORDER_SHIFT;           // 0 auto, 1 plain blockIdx, 2 grouped, 3 row-major with XCD remap
    const int p8_forced = (a->variant & MTP_GEMM_NT_P8_MASK) / MTP_GEMM_NT_P8;            // 0 no, 1 = tile height picked per problem, 2 = 224 rows, 3 = 256 rows
    const int sp_forced = (a->variant & MTP_GEMM_STORE_MASK) >> MTP_GEMM_STORE_SHIFT;     // 0 = by epilogue, 1 = nt, 2 = sc1 write-through, 3 = plain
    const bool reg_staged = a->variant & MTP_GEMM_NT_REG_STAGED, sb8_force = a->variant & MTP_GEMM_NT_SB8, sb8_forbid = a->variant & MTP_GEMM_NT_NO_SB8;
    const bool p8_forbid = a->variant & MTP_GEMM_NT_NO_P8, persist_force = a->variant & MTP_GEMM_NT_PERSIST, persist_forbid = a->variant & MTP_GEMM_NT_NO_PERSIST;
    const bool s8_force = a->variant & MTP_GEMM_NT_STRIP, s8_forbid = a->variant & MTP_GEMM_NT_NO_STRIP;

    const bool bf16 = a->in_dtype == MTP_BF16;
    // 256 x 256 tiles of the problem, scaled to a round of 256 CUs (cus: the CUs of the stream, 256 unless it is CU-masked -- the thresholds are fractions of a round)
    const int64_t tiles = ((a->M + 255) / 256) * ((a->N + 255) / 256) * 256 / cus;
    NtPlan p = {MTP_GEMM_NT_FAMILY_SB, BM, 0, 0, MTP_GEMM_STORE_PLAIN >> MTP_GEMM_STORE_SHIFT};

    // the strip kernel of gemm_s8.hip (two accumulator sets, the epilogue of a strip under the next strip's K loop), forced when the problem fits, or by
    // default: problems of less than half a round of 256 x 256 tiles on the 256 CUs -- the 768- / 1536-channel levels of InternImage-XL, ViT-B at
    // batch 32 with N = C.  Measured (tools/ab_gemm.py, MTP_AB_SHAPES=mid; profiles/r05_ab_gemm_s8_strip_mid_shapes.txt): 6272 x 768 x 768
    // 17.1 -> 15.6 us, 6272 x 768 x 3072 45.4 -> 38.3, 8192 x 768 x 768 16.8 -> 15.4, 8192 x 768 x 3072 45.5 -> 38.8, 2048 x 1536 x 1536 26.0 -> 22.6,
    // 2048 x 1536 x 6144 83.3 -> 67.9 (twice as many work units, each half as long, the epilogue of all but the last hidden); from 225 tiles on the
    // 8-wave kernel wins (its loop moves 2/3 of the L2 -> LDS bytes per flop): 6272 x 2304 x 768 22.5 vs 29.0, every ViT-L shape 10-38 %.
    // Below 40 tiles (not measured with this kernel) the 128-wide kernels keep the problem: 4 x as many, smaller workgroups.
    if (bf16 && !p8_forbid && !s8_forbid && !p8_forced && mtp_nt_s8_fits(k, a->out_dtype, a->epilogue) && (s8_force || (tiles >= 40 && tiles <= 128))) {
        p.family = MTP_GEMM_NT_FAMILY_STRIP;
        p.order = ord == 1;
        p.persistent = 1;
        p.store_policy = mtp_nt_s8_store_policy(a->out_dtype);
        return p;
    }
    // the 8-wave pipelined kernel of gemm_p8.hip (whole K-tile pairs), forced when the problem fits, or by
    // default: once its 256-wide tiles occupy a good part of the 256 CUs (one workgroup per CU); below that the
    // 128-wide kernels with 4 workgroups per CU spread a small problem better.  Measured on the ViT-L shapes (tools/ab_gemm.py):
    // +15 % (N = 3072 / 4096, K = 1024) ... +25 % (N = 1024, K = 3072 / 4096), +23 % on the FPN GEMM; on the mid-size shapes of
    // InternImage-XL's 768- / 1536-channel levels and of ViT-B at batch 32 (tools/probes/ab_gemm_mid.py, round 3): 96 tiles +6 % (K = 768) /
    // +17 % (K = 3072), 75 tiles +3 % / +16 %, 48 tiles +5 % (K = 1536) / +14 % (K = 6144), but 64 tiles of which half are mostly edge
    // (N = 432, K = 768) -19 %: from 72 tiles on, or from 40 when the contraction is long.
    if (bf16 && !p8_forbid && mtp_nt_p8_fits(k, a->out_dtype, a->epilogue) && (p8_forced || tiles >= 72 || (tiles >= 40 && a->K >= 1536))) {
        p.family = MTP_GEMM_NT_FAMILY_P8;
        p.tile_m = p8_forced == 2 ? 224 : p8_forced == 3 ? 256 : mtp_nt_p8_pick_tile_m(k.M, k.N, cus);
        p.order = ord == 1;
        // persistent tiles: default for problems of more than one round of 224-row tiles (measured, tools/ab_gemm.py: +3...4 % at N = 3072 /
        // 4096, K = 1024 and on the FPN GEMM, nothing to gain on one-round problems; the 256-row instantiations spill 2-17 VGPRs with the
        // second tile loop and stay opt-in)
        p.persistent = persist_force || (!persist_forbid && p.tile_m == 224 && mtp_nt_p8_tiles(k.M, k.N, p.tile_m) > cus);
        // store policy of the epilogue.  Measured with rotating output buffers (tools/ab_gemm.py, MTP_AB_ROTATE=8: in the training step every GEMM
        // writes fresh memory) and in the step itself (profiles/r03_ab_store_policy.txt): nt wins for the bf16 outputs (+2...4 %), sc1 for the f32
        // residual epilogue (+1...5 %: its 103 MB of output per launch do not evict the operand panels from the 4-MiB L2s); whole step +1.0 %.
        // Only the 224-row instantiations have the nt / sc1 stores
        const int sp = sp_forced ? sp_forced : (a->epilogue == MTP_EPI_BIAS_RES ? 2 : 1);
        if (p.tile_m == 224) p.store_policy = sp;
        return p;
    }
    // 128-wide kernels.  Single-stage / 4 workgroups per CU (round 1: +20 % over a double-buffered 2-per-CU LDS-DMA kernel on every ViT-L shape; that
    // kernel is gone since round 4 -- the register-staged form stays for ragged K and as MTP_GEMM_NT_REG_STAGED; it keeps its own meaning of the order bits)
    if (reg_staged || a->K % (8 * (bf16 ? 8 : 4))) {
        p.family = MTP_GEMM_NT_FAMILY_REG;
        p.order = ord;
        return p;
    }
    // tile order of the single-stage kernels.  Grouped (panels of 8 tile rows) measured +2..7 % at N = 3072 and +8..11 % at N = 4096, -2..3 % at N = 1024.
    p.order = ord == 0 ? (k.tiles_n > 8 ? 2 : 0) : ord == 1 ? 1 : ord == 2 ? 2 : 0;
    // 256 x 128 tile / 8 waves when the whole problem is ONE round of such workgroups on the 256 CUs (2 per CU) and every CU
    // gets at least one: measured on M = 12544, N = 1024 (392 workgroups): +7.5 % (K = 1024), +17..18 % (K = 3072, 4096; up to
    // 1095 TF/s); with several rounds (N = 3072: equal, N = 4096: -5 %) the coarser tiles lose to the tail.
    const int tiles8 = ((k.M + NT8_BM - 1) / NT8_BM) * k.tiles_n;
    if (sb8_force || (tiles8 >= 256 && tiles8 <= 512 && !sb8_forbid)) {
        p.family = MTP_GEMM_NT_FAMILY_SB8;
        p.tile_m = NT8_BM;
    }
    return p;
}

template <typename T, typename Tout, int EPI>
int launch_nt(const mtp_gemm_args* a, hipStream_t stream) {
    constexpr int E = Elem<T>::kPerChunk;
    KArgs k;
    int rc = fill_common<T>(a, k);
    if (rc) return rc;
    if (a->K % E) return MTP_ERR_ARG;
    if (EPI == MTP_EPI_BIAS_RES && (!a->res || (a->res_ld % 4))) return MTP_ERR_ARG;
    if ((EPI == MTP_EPI_BIAS_GELU || EPI == MTP_EPI_DGELU || EPI == MTP_EPI_BIAS_GELU_DG || EPI == MTP_EPI_MUL) && (!a->aux || (a->aux_ld % 4))) return MTP_ERR_ARG;
    if (a->bias && a->bias_mod > 0 && (a->bias_mod % 4)) return MTP_ERR_ARG;
    const NtPlan plan = nt_plan(a, k, mtp_stream_cus(stream));
    k.order = plan.order;
    const int tiles = (k.M + plan.tile_m - 1) / plan.tile_m * k.tiles_n;   // (the 128-wide families)
    switch (plan.family) {
        case MTP_GEMM_NT_FAMILY_STRIP: return mtp_nt_s8_launch(k, a->out_dtype, EPI, plan.order, stream);
        case MTP_GEMM_NT_FAMILY_P8: return mtp_nt_p8_launch(k, a->out_dtype, EPI, plan, stream);
        case MTP_GEMM_NT_FAMILY_SB8: hipLaunchKernelGGL((gemm_nt_sb8_kernel<T, Tout, EPI>), dim3(tiles), dim3(NT8_THREADS), NT8_STAGE_BYTES, stream, k); break;
        case MTP_GEMM_NT_FAMILY_REG: hipLaunchKernelGGL((gemm_nt_kernel<T, Tout, EPI>), dim3(tiles), dim3(NT_THREADS), LDS_BYTES, stream, k); break;
        default: hipLaunchKernelGGL((gemm_nt_sb_kernel<T, Tout, EPI>), dim3(tiles), dim3(NT_THREADS), STAGE_BYTES, stream, k);
    }
    return mtp_launch_status();
}

template <typename T>
int launch_tn(const mtp_gemm_args* a, hipStream_t stream) {
    constexpr int E = Elem<T>::kPerChunk;
    KArgs k;
    int rc = fill_common<T>(a, k);
    if (rc) return rc;
    if (a->out_dtype != MTP_F32 || (a->M % E) || (a->N % E)) return MTP_ERR_ARG;
    // the one place that reads the TN flags of args.variant (mtp_gemm_variant)
    const int ord = (a->variant & MTP_GEMM_ORDER_MASK) >> MTP_GEMM_ORDER_SHIFT;   // 0 auto, 1 plain blockIdx, 2 M-fastest, 3 N-fastest
    const bool reg_transpose = a->variant & MTP_GEMM_TN_REG_TRANSPOSE, tr_full_only = a->variant & MTP_GEMM_TN_TR_FULL_ONLY;
    k.bias = nullptr;
    int split = a->split_k > 1 ? a->split_k : 1;
    if (split > k.k_tiles) split = k.k_tiles;
    k.k_tiles_per_split = (k.k_tiles + split - 1) / split;
    split = (k.k_tiles + k.k_tiles_per_split - 1) / k.k_tiles_per_split;
    // split-K: with a caller workspace (args.aux, split*M*N f32) every split stores its partial tile and a second kernel
    // sums them (deterministic; f32 atomics run at only ~80 G lane-ops/s and were slower than the GEMM itself);
    // without a workspace fall back to atomics into the zeroed output.
    const bool use_ws = split > 1 && a->aux != nullptr;
    k.atomic_out = split > 1 && !use_ws;
    k.split_stride = 0;
    if (split > 1) {
        if (a->ldc != a->N) return MTP_ERR_ARG;
        if (use_ws) {
            if ((uintptr_t)a->aux & 15) return MTP_ERR_ARG;
            k.C = (char*)a->aux;
            k.split_stride = (int64_t)a->M * a->N;
        } else {
            hipError_t e = hipMemsetAsync(a->C, 0, sizeof(float) * (size_t)a->M * (size_t)a->N, stream);
            if (e != hipSuccess) return (int)e;
        }
    }
    const int tiles_m = (k.M + BM - 1) / BM;
    dim3 grid(tiles_m * k.tiles_n, split), block(NT_THREADS);
    const bool full = (a->K % (8 * E) == 0) && (a->M % BM == 0) && (a->N % BN == 0);
    // bf16 complete tiles: LDS-DMA + transpose-read kernel, unless the register-transposing kernels are asked for
    // (the transpose-read kernel also takes edge tiles as long as the rows split into whole 16-byte chunks and K into whole 64-row stages)
    const bool tr = sizeof(T) == 2 && !reg_transpose && (full || ((a->K % 64 == 0) && (a->M % 8 == 0) && (a->N % 8 == 0) && a->M >= 8 && a->N >= 8 && !tr_full_only));
    k.order = ord;            // (the register-transposing kernels read the raw field)
    if (a->colsum && !tr) {   // the other kernels do not produce the column sums: separate streaming pass over A
        rc = mtp_colsum_acc(a->A, a->in_dtype, a->lda, a->colsum, a->K, a->M, stream);
        if (rc) return rc;
    }
    if (tr) {
        k.colsum = a->colsum;
        k.order = ord == 0 ? (a->N > a->M ? 2 : 0) : ord == 1 ? 1 : ord == 2 ? 2 : 0;
        hipLaunchKernelGGL(gemm_tn_tr_kernel, grid, block, STAGE_BYTES, stream, k);
    } else if (full)
        hipLaunchKernelGGL((gemm_tn_kernel<T, true>), grid, block, LDS_BYTES, stream, k);
    else
        hipLaunchKernelGGL((gemm_tn_kernel<T, false>), grid, block, LDS_BYTES, stream, k);
    if (use_ws && !a->defer_sum) {   // defer_sum: the caller sums the partial tiles later (mtp_sum_partials_batch, several GEMMs per launch)
        const int64_t n4 = (int64_t)a->M * a->N / 4;
        int64_t nb = (n4 + 255) / 256;
        hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, stream, (const float*)a->aux, (float*)a->C, n4, split);
    }
    return mtp_launch_status();
}

// several split-K reductions in one launch (blockIdx.y = job); the table travels in the kernel arguments
struct SumJobs {
    const float* part[MTP_MAX_SEGMENTS];
    float* out[MTP_MAX_SEGMENTS];
    int64_t n4[MTP_MAX_SEGMENTS];
    int split[MTP_MAX_SEGMENTS];
};
__global__ __launch_bounds__(256) void sum_partials_batch_kernel(SumJobs t) {
    const int j = blockIdx.y;
    const float* __restrict__ part = t.part[j];
    float* __restrict__ out = t.out[j];
    const int64_t n4 = t.n4[j];
    const int split = t.split[j];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 s = *reinterpret_cast<const float4*>(part + 4 * i);
        for (int z = 1; z < split; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(part + 4 * (i + (int64_t)z * n4));
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4*>(out + 4 * i) = s;
    }
}

template <typename T, typename Tout>
int dispatch_epi(const mtp_gemm_args* a, hipStream_t s) {
    switch (a->epilogue) {
        case MTP_EPI_BIAS: return launch_nt<T, Tout, MTP_EPI_BIAS>(a, s);
        case MTP_EPI_BIAS_GELU: return launch_nt<T, Tout, MTP_EPI_BIAS_GELU>(a, s);
        case MTP_EPI_DGELU: return launch_nt<T, Tout, MTP_EPI_DGELU>(a, s);
        case MTP_EPI_BIAS_GELU_DG: return launch_nt<T, Tout, MTP_EPI_BIAS_GELU_DG>(a, s);
        case MTP_EPI_MUL: return launch_nt<T, Tout, MTP_EPI_MUL>(a, s);
        default: return MTP_ERR_UNSUPPORTED;
    }
}

}  // namespace

extern "C" int mtp_gemm_nt(const mtp_gemm_args* a, mtp_stream_t stream) {
    if (!a) return MTP_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (a->epilogue == MTP_EPI_BIAS_RES) {
        if (a->out_dtype != MTP_F32) return MTP_ERR_ARG;
        return a->in_dtype == MTP_BF16 ? launch_nt<bf16_t, float, MTP_EPI_BIAS_RES>(a, s)
                                      : launch_nt<float, float, MTP_EPI_BIAS_RES>(a, s);
    }
    if (a->in_dtype == MTP_BF16 && a->out_dtype == MTP_BF16) return dispatch_epi<bf16_t, bf16_t>(a, s);
    if (a->in_dtype == MTP_F32 && a->out_dtype == MTP_F32) return dispatch_epi<float, float>(a, s);
    if (a->in_dtype == MTP_BF16 && a->out_dtype == MTP_F32 && a->epilogue == MTP_EPI_BIAS) return launch_nt<bf16_t, float, MTP_EPI_BIAS>(a, s);
    return MTP_ERR_UNSUPPORTED;
}

namespace {
// the rider's own argument checks, and its pointers and sizes as the kernel takes them
int rider_args(const struct mtp_nt_rider* r, P8Rider& k8) {
    k8 = P8Rider{};
    if (r->kind == MTP_NT_RIDER_SAMPLING_FWD) {      // the checks of mtp_rvsa_sampling_fwd
        if (!r->x || !r->w || !r->avg || !r->pooled || !r->samp || r->B <= 0 || r->Hp <= 0 || r->Wp <= 0 || r->C <= 0 || (r->C % 4) || r->C > 8192 || r->N <= 0) return MTP_ERR_ARG;
        if (r->act_dtype != MTP_BF16) return MTP_ERR_UNSUPPORTED;
        const RvsaWindows win(r->Hp, r->Wp);
        if (r->B * win.nh * win.nw > INT32_MAX || r->N > INT32_MAX) return MTP_ERR_ARG;
        k8.windows = (int)(r->B * win.nh * win.nw);
        k8.Hp = (int)r->Hp; k8.Wp = (int)r->Wp; k8.pad_t = win.pad_t; k8.pad_l = win.pad_l; k8.nh = win.nh; k8.nw = win.nw;
    } else if (r->kind == MTP_NT_RIDER_SAMPLING_BWD_WIN) {      // the checks of mtp_rvsa_sampling_bwd_win
        if (!r->dsamp || !r->w || !r->avg || !r->g || r->windows <= 0 || r->windows > INT32_MAX || r->C <= 0 || (r->C % 4) || r->C > INT32_MAX || r->N <= 0 || r->N > 4096) return MTP_ERR_ARG;
        k8.windows = (int)r->windows;
    } else if (r->kind != MTP_NT_RIDER_NONE) {
        return MTP_ERR_ARG;
    }
    k8.C = (int)r->C; k8.N = (int)r->N;
    k8.x = r->x; k8.dsamp = r->dsamp; k8.w = r->w; k8.bias = r->bias; k8.avg = r->avg; k8.pooled = r->pooled; k8.samp = r->samp; k8.g = r->g;
    return 0;
}
// a GEMM that can carry a rider at all (bf16 in and out, bias epilogue): its own argument checks, kernel arguments and plan on `cus` CUs.
// 1 = k and plan are filled, 0 = another kind of GEMM (nothing filled), < 0 = a refused argument
int rider_gemm(const mtp_gemm_args* a, int cus, KArgs& k, NtPlan& plan) {
    if (a->in_dtype != MTP_BF16 || a->out_dtype != MTP_BF16 || a->epilogue != MTP_EPI_BIAS) return 0;
    if (const int rc = fill_common<bf16_t>(a, k)) return rc;
    if ((a->K % Elem<bf16_t>::kPerChunk) || (a->bias && a->bias_mod > 0 && (a->bias_mod % 4))) return MTP_ERR_ARG;
    plan = nt_plan(a, k, cus);
    return 1;
}
}  // namespace

// The GEMM with a rider (include/mtp_hip.h).  Every argument check precedes the first launch; a problem that cannot carry the rider falls back to the two
// launches it replaces, in the order GEMM, stand-alone kernel.
extern "C" int mtp_gemm_nt_rider(const mtp_gemm_args* a, const struct mtp_nt_rider* r, mtp_stream_t stream) {
    if (!a || !r) return MTP_ERR_ARG;
    P8Rider k8;
    if (const int rc = rider_args(r, k8)) return rc;
    hipStream_t s = (hipStream_t)stream;
    KArgs k;
    NtPlan plan;
    const int can = rider_gemm(a, mtp_stream_cus(s), k, plan);
    if (can < 0) return can;
    if (can && plan.family == MTP_GEMM_NT_FAMILY_P8) {
        // the decision mtp_gemm_nt_rider_plan reports.  Behind a plan that rides there is no fallback: whatever the launch answers is the answer
        const struct mtp_nt_rider_plan rp = mtp_nt_p8_rider_plan(k, a->out_dtype, a->epilogue, plan, r->kind, k8.windows, k8.C, k8.N, mtp_stream_cus(s));
        if (rp.rides) return mtp_nt_p8_launch_rider(k, plan, r->kind, k8, rp, s);
    }
    if (const int rc = mtp_gemm_nt(a, stream)) return rc;
    if (r->kind == MTP_NT_RIDER_SAMPLING_FWD) return mtp_rvsa_sampling_fwd(r->x, r->act_dtype, r->w, r->bias, r->avg, r->pooled, r->samp, r->B, r->Hp, r->Wp, r->C, r->N, stream);
    if (r->kind == MTP_NT_RIDER_SAMPLING_BWD_WIN) return mtp_rvsa_sampling_bwd_win(r->dsamp, r->w, r->avg, r->g, r->windows, r->C, r->N, stream);
    return 0;
}

// What mtp_gemm_nt_rider does with these arguments on `cus` CUs, without launching: the same checks, the same plan, the same decision function.
extern "C" int mtp_gemm_nt_rider_plan(const mtp_gemm_args* a, const struct mtp_nt_rider* r, int cus, struct mtp_nt_rider_plan* out) {
    if (!a || !r || !out) return MTP_ERR_ARG;
    P8Rider k8;
    if (const int rc = rider_args(r, k8)) return rc;
    if (cus <= 0) cus = mtp_stream_cus(nullptr);
    KArgs k;
    NtPlan plan;
    const int can = rider_gemm(a, cus, k, plan);
    if (can < 0) return can;
    if (!can && mtp_gemm_nt_plan(a, cus, &plan)) return MTP_ERR_ARG;      // (a GEMM of another dtype or epilogue: its plan only names the reason)
    const struct mtp_nt_rider_plan none = {0, 0, 0, 0, 0, plan.family == MTP_GEMM_NT_FAMILY_P8 ? MTP_NT_RIDE_NO_INSTANTIATION : MTP_NT_RIDE_NO_FAMILY};
    *out = can && plan.family == MTP_GEMM_NT_FAMILY_P8 ? mtp_nt_p8_rider_plan(k, a->out_dtype, a->epilogue, plan, r->kind, k8.windows, k8.C, k8.N, cus) : none;
    return 0;
}

// (round 4: the stream-K form that used `workspace` was removed -- measured slower; the query stays in the ABI and answers 0)
extern "C" int64_t mtp_gemm_nt_workspace_bytes(void) { return 0; }

extern "C" int mtp_gemm_nt_plan(const mtp_gemm_args* a, int cus, struct mtp_gemm_nt_plan* out) {
    if (!a || !out) return MTP_ERR_ARG;
    KArgs k;
    if (a->in_dtype == MTP_BF16 ? fill_common<bf16_t>(a, k) : fill_common<float>(a, k)) return MTP_ERR_ARG;
    *out = nt_plan(a, k, cus > 0 ? cus : mtp_stream_cus(nullptr));
    return 0;
}

extern "C" int mtp_gemm_nt_tile(const mtp_gemm_args* a) {
    NtPlan p;
    if (const int rc = mtp_gemm_nt_plan(a, 0, &p)) return rc;
    return p.family == MTP_GEMM_NT_FAMILY_P8 ? 256 : p.family == MTP_GEMM_NT_FAMILY_STRIP ? 64 : 128;
}

extern "C" int mtp_sum_partials_batch(const float* const* parts, float* const* outs, const int64_t* numel, const int* splits, int count, mtp_stream_t stream) {
    if (!parts || !outs || !numel || !splits || count <= 0 || count > MTP_MAX_SEGMENTS) return MTP_ERR_ARG;
    SumJobs t;
    int64_t mx = 0;
    for (int i = 0; i < count; ++i) {
        if (!parts[i] || !outs[i] || numel[i] <= 0 || (numel[i] % 4) || splits[i] < 1) return MTP_ERR_ARG;
        t.part[i] = parts[i]; t.out[i] = outs[i]; t.n4[i] = numel[i] / 4; t.split[i] = splits[i];
        mx = t.n4[i] > mx ? t.n4[i] : mx;
    }
    int64_t nb = (mx + 255) / 256;
    hipLaunchKernelGGL(sum_partials_batch_kernel, dim3((unsigned)(nb > 2048 ? 2048 : nb), (unsigned)count), dim3(256), 0, (hipStream_t)stream, t);
    return mtp_launch_status();
}

extern "C" int mtp_gemm_tn(const mtp_gemm_args* a, mtp_stream_t stream) {
    if (!a) return MTP_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    return a->in_dtype == MTP_BF16 ? launch_tn<bf16_t>(a, s) : launch_tn<float>(a, s);
}
