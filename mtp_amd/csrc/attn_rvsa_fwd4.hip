// RVSA forward, 4 waves per (image, window, head) (attn_rvsa_common.h has the algorithm and the lane layout).
#include "attn_launch.h"
#include "attn_rvsa_common.h"

namespace {

// ===================================================================================================================
// RVSA forward, 4 waves per (image, window, head): the bilinear gather is split over 256 threads (key x 16-channel quarter)
// and wave w owns query tile w, so 24 waves share a CU (6 workgroups x 4) instead of 4-6 single-wave problems.
// ===================================================================================================================
__global__ __launch_bounds__(256, 4) void rvsa_fwd4_mfma_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ samp, bf16_t* __restrict__ o, float* __restrict__ lse,
                                                            const float* __restrict__ rel_h, const float* __restrict__ rel_w, const float* __restrict__ bias_table,
                                                            RvsaGeom g, float scale) {
    __shared__ __attribute__((aligned(16))) char Ks[64 * 128];
    __shared__ __attribute__((aligned(16))) char Vs[64 * 128];      // V_sel rows like Ks (round 6; it was a [d][key] image written in 2-byte units)
    __shared__ float QR[26 * 64];
    __shared__ float tab[176];
    __shared__ float rec[8 * 64];      // per key: the four neighbour tokens and weights of its bilinear sample
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), fr = lane & 15, gq = lane >> 4;
    const int H = g.heads, nW = g.nh * g.nw;
    const int h = blockIdx.x % H, bw = blockIdx.x / H, b = bw / nW, win = bw % nW, wi = win / g.nw, wj = win % g.nw;
    const int C = H * HD, N = g.Hp * g.Wp;
    const int64_t ld = 3 * (int64_t)C;
    const bf16_t* base = qkv + (int64_t)b * N * ld + h * HD;

    if (tid < 169) tab[tid] = bias_table[tid * H + h];
    // ---- this wave's query tile first: these loads depend on nothing, so they fly under the sample computation and the gather
    const int qt = wave;
    const int n = 16 * qt + fr;
    const int qtok = n < 49 ? query_token(g, n, wi, wj) : -1;
    uint4 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = row_frag(base, ld, qtok, ks * 32 + gq * 8);
    {   // ---- gather: lane = (key of a group of 8, 16-B chunk of the 64-channel row): a wave instruction reads 8 WHOLE 128-B rows
        // (with lane = key it touched 49 cache lines for 16 B each); all 16 loads of the wave's two key groups are issued before
        // the first use.  Every lane computes the sample position of its own key (8 lanes share one: no barrier needed).
        const int kl = lane >> 3, ch = lane & 7;
        uint4 kq[2][4], vq[2][4];
        float wq[2][4];
        {   // ONE sample + four neighbours per key and wave instruction stream (round 5; it was two + eight: every lane its own two keys): lane l < 16 owns
            // key (wave + 4 (l >> 3)) * 8 + (l & 7), writes the neighbour record to `rec`, and the wave reads its own records back -- LDS operations of one
            // wave execute in order, so no barrier is involved (attn_rvsa_bwd4.hip does the same and keeps the records for its coordinate-gradient phase)
            const int l16 = lane & 15;
            const int key = (wave + 4 * (l16 >> 3)) * 8 + (l16 & 7), kc = key < 48 ? key : 48;
            const Sample sm = make_sample<true>(g, samp + (int64_t)bw * 5 * H, h, wi, wj, kc / 7, kc % 7);
            float wv[4];
            int tk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float w;
                const int tok = key < 49 ? neighbour(g, sm.x0, sm.y0, sm.fx, sm.fy, k, w) : -1;      // keys >= 49 are zero rows
                tk[k] = tok;
                wv[k] = tok >= 0 ? w : 0.f;
            }
            if (lane < 16) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    rec[k * 64 + key] = __int_as_float(tk[k]);
                    rec[(4 + k) * 64 + key] = wv[k];
                }
            }
        }
        // (the records cross lanes: a wavefront-scope release + wave barrier keeps the compiler from moving the read-back above the writes; the hardware
        //  executes one wave's LDS operations in order, so this costs no instruction -- ADVICE r05)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int key = (wave + 4 * gi) * 8 + kl;      // 8 groups = 64 key rows
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int tok = __float_as_int(rec[k * 64 + key]);
                const int tc = tok >= 0 ? tok : 0;
                wq[gi][k] = rec[(4 + k) * 64 + key];
                const uint32_t roff = (uint32_t)tc * (uint32_t)(6 * C) + (uint32_t)(16 * ch);      // 32-bit byte offsets off the (image, head) base
                kq[gi][k] = ldg16_at(base + C, roff);
                vq[gi][k] = ldg16_at(base + 2 * C, roff);
            }
        }
        // QR = tables x Q^T of this wave's query tile, while the gather's loads are in flight
    #pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float* tb = t ? rel_w : rel_h;
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            acc = mma(table_frag(tb, fr, 13, gq * 8), qf[0], acc);
            acc = mma(table_frag(tb, fr, 13, 32 + gq * 8), qf[1], acc);
    #pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                if (4 * gq + rr < 13) QR[(t * 13 + 4 * gq + rr) * 64 + n] = acc[rr];
        }
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int key = (wave + 4 * gi) * 8 + kl;
            float ks[8], vs[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { ks[e] = 0.f; vs[e] = 0.f; }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t kw[4] = {kq[gi][k].x, kq[gi][k].y, kq[gi][k].z, kq[gi][k].w}, vw[4] = {vq[gi][k].x, vq[gi][k].y, vq[gi][k].z, vq[gi][k].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ks[2 * e] += wq[gi][k] * bf16_bits_to_f32(kw[e] & 0xffffu); ks[2 * e + 1] += wq[gi][k] * bf16_bits_to_f32(kw[e] >> 16);
                    vs[2 * e] += wq[gi][k] * bf16_bits_to_f32(vw[e] & 0xffffu); vs[2 * e + 1] += wq[gi][k] * bf16_bits_to_f32(vw[e] >> 16);
                }
            }
            *reinterpret_cast<uint4*>(Ks + swz(key, ch)) = pack_bf16x8(ks[0], ks[1], ks[2], ks[3], ks[4], ks[5], ks[6], ks[7]);
            *reinterpret_cast<uint4*>(Vs + swz(key, ch)) = pack_bf16x8(vs[0], vs[1], vs[2], vs[3], vs[4], vs[5], vs[6], vs[7]);
        }
    }
    __syncthreads();
    f32x4_t s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        s[kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) s[kt] = mma(ld16(Ks + swz(16 * kt + fr, ks * 4 + gq)), qf[ks], s[kt]);
    }
    const int nq = n < 48 ? n : 48;
    const int aq = (nq * 37) >> 8, bq = nq - 7 * aq;
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = 16 * kt + 4 * gq + r, kc = key < 48 ? key : 48;
            const int ak = (kc * 37) >> 8, bk = kc - 7 * ak, dh = aq - ak + 6, dw = bq - bk + 6;
            float v = scale * s[kt][r] + QR[dh * 64 + n] + QR[(13 + dw) * 64 + n] + tab[dh * 13 + dw];
            v = key < 49 ? v : -INFINITY;
            s[kt][r] = v;
            m = fmaxf(m, v);
        }
    m = xor16_max(m);
    m = xor32_max(m);
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __expf(s[kt][r] - m);
            s[kt][r] = p;
            l += p;
        }
    l = xor16_sum(l);
    l = xor32_sum(l);
    if (gq == 0 && n < 49) lse[(int64_t)blockIdx.x * 49 + n] = m + __logf(l);
    f32x4_t oa[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oa[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const uint4 pf = pack_bf16x8(s[2 * kk][0], s[2 * kk][1], s[2 * kk][2], s[2 * kk][3], s[2 * kk + 1][0], s[2 * kk + 1][1], s[2 * kk + 1][2], s[2 * kk + 1][3]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            oa[dt] = mma(rows_frag_tr(Vs, 32 * kk + 4 * gq, dt, fr), pf, oa[dt]);      // V^T fragment (d = 16 dt + fr; keys 32 kk + 4 gq .. + 3, + 16 ..) by transpose read
        }
    }
    if (qtok >= 0) {
        const float inv = 1.0f / l;
        bf16_t* op = o + ((int64_t)b * N + qtok) * C + h * HD + 4 * gq;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4(op + 16 * dt, make_float4(oa[dt][0] * inv, oa[dt][1] * inv, oa[dt][2] * inv, oa[dt][3] * inv));
    }
}

}  // namespace

int mtp_rvsa_fwd_mfma_launch(const void* qkv, const float* samp, void* o, float* lse, const float* rel_h, const float* rel_w, const float* bias_table,
                             int64_t B, int64_t Hp, int64_t Wp, int64_t heads, float scale, hipStream_t s) {
    const RvsaGeom g = make_geom(Hp, Wp, heads);
    hipLaunchKernelGGL(rvsa_fwd4_mfma_kernel, dim3((unsigned)(B * g.nh * g.nw * heads)), dim3(256), 0, s, (const bf16_t*)qkv, samp, (bf16_t*)o, lse,
                       rel_h, rel_w, bias_table, g, scale);
    return mtp_launch_status();
}
