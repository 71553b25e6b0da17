// bf16 MFMA flash forward for the full (global) attention blocks of the MTP backbone (Attention.forward, VIT:90-111, with the
// decomposed relative-position terms of calc_rel_pos_spatial, VIT:142-193), gfx950, head_dim 64, beyond 256 tokens with sides <= 64
// (448^2 pretraining inputs: 784 tokens; the 1024^2 detection fine-tunes: 4096).  Grids of at most 16 x 16 are attn_full_v3.hip's.
//
// Workgroup = 64 queries of one (image, head) (wave = one 16-query tile), loop over blocks of FKB keys with an online softmax.  Same
// tricks as the RVSA kernels (attn_rvsa_common.h): S^T = K.Q^T so a query's softmax is in-lane + two shuffles and P is directly the
// B operand of O^T = V^T.P^T; the q.Rh / q.Rw terms are one MFMA against the tables, exchanged through a per-wave LDS tile.
// RT = 16-row tiles per table: 4 (Hp, Wp <= 32) or 8 (<= 64).
// dynamic LDS: Ks[FKB*128] | Vs[FKB*128] | QR[4 waves][32 RT][16] f32 | kpos[FKB] u32
#include "attn_launch.h"
#include "attn_full_common.h"

namespace {

template <int RT, int FKB>
__global__ __launch_bounds__(256) void full_fwd_flash_mfma_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ o, float* __restrict__ lse,
                                                                 const float* __restrict__ rel_h, const float* __restrict__ rel_w,
                                                                 int N, int Hp, int Wp, int heads, float scale) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    char* Ks = sm;
    char* Vs = Ks + FKB * 128;      // V rows like the K rows (round 6): the V^T operand of O^T = V^T.P^T comes out of ds_read_b64_tr_b16, not out of a transposed image written
    float* QRall = reinterpret_cast<float*>(Vs + FKB * 128);      // in 2-byte pieces (32 ds_write_b16 per thread and key block)
    uint32_t* kpos = reinterpret_cast<uint32_t*>(QRall + 4 * 32 * RT * 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, gq = lane >> 4;
    const int bh = blockIdx.x, b = bh / heads, h = bh % heads;
    const int C = heads * HD, RH = 2 * Hp - 1, RW = 2 * Wp - 1;
    const int64_t ld = 3 * (int64_t)C;
    const bf16_t* base = qkv + (int64_t)b * N * ld + h * HD;
    float* QR = QRall + wave * 32 * RT * 16;
    const int n = 16 * (blockIdx.y * 4 + wave) + fr;
    const bool nv = n < N;
    const int nc = nv ? n : N - 1;
    uint4 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = row_frag(base, ld, nc, nv, ks * 32 + gq * 8);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {   // q.Rh / q.Rw for every table row: one MFMA tile row each, exchanged through LDS
        f32x4_t ah = {0.f, 0.f, 0.f, 0.f}, aw = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            ah = mma(table_frag(rel_h, 16 * rt + fr, RH, ks * 32 + gq * 8), qf[ks], ah);
            aw = mma(table_frag(rel_w, 16 * rt + fr, RW, ks * 32 + gq * 8), qf[ks], aw);
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            QR[(16 * rt + 4 * gq + rr) * 16 + fr] = ah[rr];
            QR[(16 * RT + 16 * rt + 4 * gq + rr) * 16 + fr] = aw[rr];
        }
    }
    const int hq = nc / Wp + Hp - 1, wq = nc % Wp + Wp - 1;
    float m = -INFINITY, l = 0.f;
    f32x4_t oa[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oa[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int nblk = (N + FKB - 1) / FKB;
    uint4 kpre[FKB * 8 / 256], vpre[FKB * 8 / 256];      // the next key block's rows, in flight while this one is worked on (round 6)
    prefetch_rows<FKB>(base + C, ld, N, tid, kpre);
    prefetch_rows<FKB>(base + 2 * C, ld, N, tid, vpre);
    for (int jb = 0; jb < nblk; ++jb) {
        const int kb0 = jb * FKB, rem = N - kb0;
        __syncthreads();   // the previous block's K / V reads are done (first pass: the QR tiles are visible)
        commit_rows<FKB>(Ks, tid, kpre);
        commit_rows<FKB>(Vs, tid, vpre);
        if (tid < FKB) {
            const int key = kb0 + tid < N ? kb0 + tid : N - 1;
            kpos[tid] = (uint32_t)(key / Wp) | ((uint32_t)(key % Wp) << 8);
        }
        if (jb + 1 < nblk) {
            prefetch_rows<FKB>(base + C + (int64_t)(kb0 + FKB) * ld, ld, rem - FKB, tid, kpre);
            prefetch_rows<FKB>(base + 2 * C + (int64_t)(kb0 + FKB) * ld, ld, rem - FKB, tid, vpre);
        }
        __syncthreads();
        const int keys = rem < FKB ? rem : FKB, tiles = (keys + 15) / 16, kkb = (keys + 31) / 32;
        f32x4_t s[FKB / 16];
#pragma unroll
        for (int kt = 0; kt < FKB / 16; ++kt) {
            s[kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (kt < tiles) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) s[kt] = mma(ld16(Ks + swz(16 * kt + fr, ks * 4 + gq)), qf[ks], s[kt]);
            }
        }
        float bm = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < FKB / 16; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kl = 16 * kt + 4 * gq + r;
                const uint32_t kp = kpos[kl];
                float v = scale * (s[kt][r] + QR[(hq - (int)(kp & 0xffu)) * 16 + fr] + QR[(16 * RT + wq - (int)(kp >> 8)) * 16 + fr]);
                v = kb0 + kl < N ? v : -INFINITY;
                s[kt][r] = v;
                bm = fmaxf(bm, v);
            }
        bm = xor16_max(bm);
        bm = xor32_max(bm);
        const float mnew = fmaxf(m, bm);
        const float alpha = __expf(m - mnew);   // first block: exp(-inf) = 0
        float lb = 0.f;
#pragma unroll
        for (int kt = 0; kt < FKB / 16; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __expf(s[kt][r] - mnew);
                s[kt][r] = p;
                lb += p;
            }
        lb = xor16_sum(lb);
        lb = xor32_sum(lb);
        l = l * alpha + lb;
        m = mnew;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oa[dt] = f32x4_t{oa[dt][0] * alpha, oa[dt][1] * alpha, oa[dt][2] * alpha, oa[dt][3] * alpha};
#pragma unroll
        for (int kk = 0; kk < FKB / 32; ++kk) {
            if (kk < kkb) {
                const uint4 pf = pack_bf16x8(s[2 * kk][0], s[2 * kk][1], s[2 * kk][2], s[2 * kk][3], s[2 * kk + 1][0], s[2 * kk + 1][1], s[2 * kk + 1][2], s[2 * kk + 1][3]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) oa[dt] = mma(kt_frag_tr(Vs, 32 * kk + 4 * gq, dt, fr), pf, oa[dt]);
            }
        }
    }
    if (nv) {
        const float inv = 1.0f / l;
        bf16_t* op = o + ((int64_t)b * N + n) * C + h * HD + 4 * gq;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4(op + 16 * dt, make_float4(oa[dt][0] * inv, oa[dt][1] * inv, oa[dt][2] * inv, oa[dt][3] * inv));
        if (gq == 0) lse[(int64_t)bh * N + n] = m + __logf(l);
    }
}

}  // namespace

int mtp_full_fwd_flash_keys(int64_t Hp, int64_t Wp) {
    if (Hp < 1 || Wp < 1 || Hp * Wp <= 256 || Hp > 64 || Wp > 64) return 0;
    return (Hp > 32 || Wp > 32) ? 256 : 128;          // tables of up to 127 rows: 8 row tiles each
}

int mtp_full_fwd_flash_launch(const void* qkv, void* o, float* lse, const float* rel_h, const float* rel_w,
                              int64_t B, int64_t Hp, int64_t Wp, int64_t heads, float scale, hipStream_t s) {
    const int64_t N = Hp * Wp;
    const int keys = mtp_full_fwd_flash_keys(Hp, Wp);
    if (!keys) return MTP_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(B * heads), (unsigned)((N + 63) / 64));
    if (keys == 256) {
        constexpr int KBLK = 256;
        const size_t lds = 2 * (size_t)KBLK * 128 + (size_t)4 * 32 * 8 * 16 * 4 + KBLK * 4;
        (void)hipFuncSetAttribute((const void*)full_fwd_flash_mfma_kernel<8, KBLK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((full_fwd_flash_mfma_kernel<8, KBLK>), grid, dim3(256), lds, s, (const bf16_t*)qkv, (bf16_t*)o, lse, rel_h, rel_w, (int)N, (int)Hp, (int)Wp, (int)heads, scale);
    } else {
        // 128-key blocks: 65 KiB of LDS, two workgroups (8 waves) per CU instead of one
        constexpr int KBLK = 128;
        const size_t lds = 2 * (size_t)KBLK * 128 + (size_t)4 * 32 * 4 * 16 * 4 + KBLK * 4;
        (void)hipFuncSetAttribute((const void*)full_fwd_flash_mfma_kernel<4, KBLK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((full_fwd_flash_mfma_kernel<4, KBLK>), grid, dim3(256), lds, s, (const bf16_t*)qkv, (bf16_t*)o, lse, rel_h, rel_w, (int)N, (int)Hp, (int)Wp, (int)heads, scale);
    }
    return mtp_launch_status();
}
