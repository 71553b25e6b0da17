// Scene classification head (mmpretrain ImageClassifier = backbone + GlobalAveragePooling + LinearClsHead with CrossEntropyLoss, and the Accuracy
// metric, as every Scene_Classification/configs/mtp/* config of the reference composes them; mmpretrain itself is not vendored there, so the kernels
// follow the published algorithm).  The head is tiny next to the backbone -- N <= 64 samples, K <= 64 classes, C <= 1536 channels -- so a training
// step spends four launches on it, two each way, and every kernel is written for a fixed summation order instead of peak rate: no float atomics,
// two runs give the same bits.
//   gap_fwd        pooled[n, c] = mean over HW of x[n, c, :]       rows of the flat NCHW stream, 16-byte loads wherever the row allows them
//   gap_bwd        dx[n, c, :] = dpooled[n, c] / HW                16-byte stores over the flat stream
//   cls_ce         logits = pooled . w^T + b, softmax, arg-max, per-sample loss, dlogits: one workgroup per sample; the scalar loss is summed in
//                  sample order by the workgroup that finishes last (an integer arrival counter, the only inter-workgroup traffic)
//   cls_head_bwd   dw = dlogits^T . pooled, db = column sums of dlogits, dpooled = dlogits . w: one thread per output element, sums in index order
//   cls_hits       rank of the label among the scores without a sort; integer counters
#include "common.h"

namespace {

constexpr int kWaves = kThreads / MTP_WAVE;
constexpr int kMaxTopk = 8;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
    return v;
}

// ------------------------------------------------------------------------------------------------------------------- pooling
// sum of the `per` elements of one 16-byte chunk, in element order
__device__ __forceinline__ float chunk_sum(const float* p) {
    const float4 v = load4(p);
    return ((v.x + v.y) + v.z) + v.w;
}
__device__ __forceinline__ float chunk_sum(const bf16_t* p) {
    float o[8];
    load8(p, o);
    return ((((((o[0] + o[1]) + o[2]) + o[3]) + o[4]) + o[5]) + o[6]) + o[7];
}

// L lanes per row (16: four rows per wave, for rows of at most two chunks per lane; 64: a wave per row).  A row starts wherever the flat stream puts
// it (2-byte aligned for bf16 with an odd HW): the elements in front of the first 16-byte boundary and behind the last one are read one by one, the
// body in 16-byte chunks.  Every lane sums its share in index order, the lanes are summed by a butterfly: a fixed order.  The trip count is the same
// for every wave and rows past the end are clamped, so all lanes are active at the butterfly (the DPP forms need that).
template <typename T, int L>
__global__ void __launch_bounds__(kThreads) gap_fwd_kernel(const T* __restrict__ x, float* __restrict__ pooled, int64_t rows, int64_t HW) {
    constexpr int kPer = Elem<T>::kPerChunk;
    const int lane = threadIdx.x % L;
    const int64_t groups = (int64_t)gridDim.x * (kThreads / L);
    const int64_t group = (int64_t)blockIdx.x * (kThreads / L) + threadIdx.x / L;
    const int64_t iters = (rows + groups - 1) / groups;
    const float hw = (float)HW;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t row = it * groups + group;
        const bool valid = row < rows;
        const T* p = x + (valid ? row : rows - 1) * HW;
        const int64_t lead = (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(T));
        const int64_t head = lead < HW ? lead : HW;
        const int64_t nv = (HW - head) / kPer;
        float s = 0.0f;
        if (lane < head) s += Elem<T>::load(p + lane);                                        // (head < kPer <= 8 < L)
        for (int64_t v = lane; v < nv; v += L) s += chunk_sum(p + head + v * kPer);
        for (int64_t i = head + nv * kPer + lane; i < HW; i += L) s += Elem<T>::load(p + i);      // (fewer than kPer elements)
        if constexpr (L == 64) {
            s = wave_sum(s);
        } else {
            s += lane_xor<8>(s); s += lane_xor<4>(s); s += lane_xor<2>(s); s += lane_xor<1>(s);
        }
        if (valid && lane == 0) pooled[row] = s / hw;
    }
}

// one 16-byte chunk of the flat dx stream per thread and step; the chunk may span rows (HW is arbitrary); the last chunk of the stream may be partial
template <typename T>
__global__ void __launch_bounds__(kThreads) gap_bwd_kernel(const float* __restrict__ dpooled, T* __restrict__ dx, int64_t total, int64_t HW) {
    constexpr int kPer = Elem<T>::kPerChunk;
    const int64_t chunks = (total + kPer - 1) / kPer;
    const float hw = (float)HW;
    for (int64_t ch = (int64_t)blockIdx.x * kThreads + threadIdx.x; ch < chunks; ch += (int64_t)gridDim.x * kThreads) {
        const int64_t e0 = ch * kPer;
        int64_t row = e0 / HW, rem = e0 - row * HW;
        float v = dpooled[row] / hw;
        float o[8];
        const int n = (int)(total - e0 < kPer ? total - e0 : kPer);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            o[j] = v;
            if (++rem == HW && j + 1 < n) {
                rem = 0;
                v = dpooled[++row] / hw;
            }
        }
        if (n == kPer) {
            if constexpr (kPer == 8) {
                store8(dx + e0, o);
            } else {
                store4(dx + e0, make_float4(o[0], o[1], o[2], o[3]));
            }
        } else {
            for (int j = 0; j < n; ++j) Elem<T>::store(dx + e0 + j, o[j]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- linear + cross-entropy
// One workgroup per sample.  Phase 1: the four waves share the K dot products of length C (lanes over C, 16-byte loads when VEC, a butterfly per
// product) and write the logits row.  Phase 2, wave 0 alone: max, arg-max (lowest index among ties), sum of exp(l - max), then prob, the sample's loss
// and its dlogits row.  Phase 3: the sample's loss is published with an agent-scope atomic store and the arrival counter is bumped (release / acquire
// at agent scope); the workgroup that sees N - 1 reads all N losses with agent-scope atomic loads, sums them in sample order and puts the counter back
// to 0 for the next call.  `counter` must be 0 on entry.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) cls_ce_kernel(const float* __restrict__ pooled, const float* __restrict__ w, const float* __restrict__ b,
                                                          const int64_t* __restrict__ labels, float loss_weight, float* logits, float* __restrict__ prob,
                                                          int64_t* __restrict__ pred, float* loss_rows, float* __restrict__ loss,
                                                          float* __restrict__ dlogits, unsigned* counter, int N, int C, int K) {
    const int n = blockIdx.x, lane = threadIdx.x % MTP_WAVE, wave = threadIdx.x / MTP_WAVE;
    const float* x = pooled + (int64_t)n * C;
    float* lrow = logits + (int64_t)n * K;
    for (int k = wave; k < K; k += kWaves) {
        const float* wr = w + (int64_t)k * C;
        float s = 0.0f;
        if constexpr (VEC) {
            for (int c = lane * 4; c < C; c += MTP_WAVE * 4) {
                const float4 a = load4(x + c), q = load4(wr + c);
                s += ((a.x * q.x + a.y * q.y) + a.z * q.z) + a.w * q.w;
            }
        } else {
            for (int c = lane; c < C; c += MTP_WAVE) s += x[c] * wr[c];
        }
        s = wave_sum(s);
        if (lane == 0) lrow[k] = s + b[k];
    }
    __syncthreads();      // (workgroup-scope release / acquire: wave 0 reads what the other waves stored)
    if (wave != 0) return;
    float m = -INFINITY;
    for (int k = lane; k < K; k += MTP_WAVE) m = fmaxf(m, lrow[k]);
    m = wave_max(m);
    float e = 0.0f;
    int first = INT32_MAX;
    for (int k = lane; k < K; k += MTP_WAVE) {
        const float l = lrow[k];
        e += expf(l - m);
        if (l == m && k < first) first = k;
    }
    e = wave_sum(e);
    first = wave_min_i(first);
    if (first == INT32_MAX) first = 0;      // (a row of NaN)
    const int64_t lab = labels ? labels[n] : -1;
    for (int k = lane; k < K; k += MTP_WAVE) {
        const float pk = expf(lrow[k] - m) / e;
        if (prob) prob[(int64_t)n * K + k] = pk;
        if (dlogits) dlogits[(int64_t)n * K + k] = (loss_weight * (pk - (k == lab ? 1.0f : 0.0f))) / (float)N;
    }
    if (pred && lane == 0) pred[n] = first;
    if (!labels || (!loss_rows && !loss)) return;
    const float lr = lab >= 0 && lab < K ? (m + logf(e)) - lrow[lab] : 0.0f;      // (labels outside [0, K): refused by the host wrapper)
    if (lane == 0 && loss_rows) __hip_atomic_store(loss_rows + n, lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!loss) return;
    unsigned old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    old = __shfl(old, 0);
    if (old != (unsigned)(N - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (lane == 0) {
        float s = 0.0f;
        for (int i = 0; i < N; ++i) s += __hip_atomic_load(loss_rows + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        loss[0] = loss_weight * (s / (float)N);
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one thread per output element: [0, K*C) dw[k, c] = sum_n dl[n, k] pooled[n, c]; [K*C, K*C + N*C) dpooled[n, c] = sum_k dl[n, k] w[k, c]; then K
// threads for db[k] = sum_n dl[n, k].  Consecutive threads read consecutive c; dl is the same address across a wave (nearly always).  Four partial
// sums over the summation index taken round robin, combined in a fixed order.
__global__ void __launch_bounds__(kThreads) cls_head_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ pooled, const float* __restrict__ w,
                                                                float* __restrict__ dw, float* __restrict__ db, float* __restrict__ dpooled, int N, int C,
                                                                int K, int accumulate) {
    const int64_t KC = (int64_t)K * C, NC = dpooled ? (int64_t)N * C : 0, total = KC + NC + K;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < KC) {
            const int k = (int)(i / C), c = (int)(i - (int64_t)k * C);
            for (int n = 0; n < N; ++n) a[n & 3] += dl[(int64_t)n * K + k] * pooled[(int64_t)n * C + c];
            const float s = (a[0] + a[1]) + (a[2] + a[3]);
            dw[i] = accumulate ? dw[i] + s : s;
        } else if (i < KC + NC) {
            const int64_t j = i - KC;
            const int n = (int)(j / C), c = (int)(j - (int64_t)n * C);
            for (int k = 0; k < K; ++k) a[k & 3] += dl[(int64_t)n * K + k] * w[(int64_t)k * C + c];
            dpooled[j] = (a[0] + a[1]) + (a[2] + a[3]);
        } else {
            const int k = (int)(i - KC - NC);
            for (int n = 0; n < N; ++n) a[n & 3] += dl[(int64_t)n * K + k];
            const float s = (a[0] + a[1]) + (a[2] + a[3]);
            db[k] = accumulate ? db[k] + s : s;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- accuracy
struct TopkList {
    int n;
    int k[kMaxTopk];
};

// one wave per sample: rank of the label = #{j : s_j > s_label} + #{j < label : s_j == s_label} (the position a stable descending sort gives it);
// hits per workgroup in LDS, then one 64-bit integer atomic per k and workgroup: exact in any order.  counters[nk] += N by workgroup 0.
__global__ void __launch_bounds__(kThreads) cls_hits_kernel(const float* __restrict__ scores, const int64_t* __restrict__ labels, int64_t N, int K,
                                                            TopkList topk, float thr, int use_thr, unsigned long long* counters) {
    __shared__ int hits[kMaxTopk];
    if (threadIdx.x < kMaxTopk) hits[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x % MTP_WAVE;
    for (int64_t n = (int64_t)blockIdx.x * kWaves + threadIdx.x / MTP_WAVE; n < N; n += (int64_t)gridDim.x * kWaves) {
        const int64_t lab = labels[n];
        if (lab < 0 || lab >= K) continue;      // (refused by the host wrapper; wave-uniform)
        const float* s = scores + n * K;
        const float sl = s[lab];
        int rank = 0;
        for (int j = lane; j < K; j += MTP_WAVE) {
            const float v = s[j];
            rank += (v > sl) || (v == sl && j < lab);
        }
        rank = wave_sum_i(rank);
        if (lane == 0 && (!use_thr || sl > thr))
            for (int t = 0; t < topk.n; ++t)
                if (rank < topk.k[t]) atomicAdd(&hits[t], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < topk.n && hits[threadIdx.x] != 0) atomicAdd(&counters[threadIdx.x], (unsigned long long)hits[threadIdx.x]);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counters[topk.n], (unsigned long long)N);
}

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_gap_fwd(const void* x, int dtype, float* pooled, int64_t N, int64_t C, int64_t HW, mtp_stream_t stream) {
    MTP_CHECK_ARG(x && pooled && N > 0 && C > 0 && HW > 0 && dt_ok(dtype));
    MTP_CHECK_ARG(N < ((int64_t)1 << 40) / C && N * C < ((int64_t)1 << 60) / HW);
    MTP_CHECK_ARG(((uintptr_t)x & (dtype == MTP_F32 ? 3 : 1)) == 0 && ((uintptr_t)pooled & 3) == 0);
    const int64_t rows = N * C;
    hipStream_t s = (hipStream_t)stream;
    const bool narrow = HW * (dtype == MTP_F32 ? 4 : 2) <= 512;      // at most two 16-byte chunks per lane of a 16-lane group
    const unsigned g = blocks_for(rows * (narrow ? 16 : 64), kThreads, kMaxBlocks);
    if (dtype == MTP_F32) {
        if (narrow) gap_fwd_kernel<float, 16><<<g, kThreads, 0, s>>>((const float*)x, pooled, rows, HW);
        else gap_fwd_kernel<float, 64><<<g, kThreads, 0, s>>>((const float*)x, pooled, rows, HW);
    } else {
        if (narrow) gap_fwd_kernel<bf16_t, 16><<<g, kThreads, 0, s>>>((const bf16_t*)x, pooled, rows, HW);
        else gap_fwd_kernel<bf16_t, 64><<<g, kThreads, 0, s>>>((const bf16_t*)x, pooled, rows, HW);
    }
    return mtp_launch_status();
}

extern "C" int mtp_gap_bwd(const float* dpooled, void* dx, int dtype, int64_t N, int64_t C, int64_t HW, mtp_stream_t stream) {
    MTP_CHECK_ARG(dpooled && dx && N > 0 && C > 0 && HW > 0 && dt_ok(dtype));
    MTP_CHECK_ARG(N < ((int64_t)1 << 40) / C && N * C < ((int64_t)1 << 60) / HW);
    MTP_CHECK_ARG(((uintptr_t)dx & 15) == 0 && ((uintptr_t)dpooled & 3) == 0);
    const int64_t total = N * C * HW;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MTP_F32) gap_bwd_kernel<float><<<blocks_for((total + 3) / 4, kThreads, kMaxBlocks), kThreads, 0, s>>>(dpooled, (float*)dx, total, HW);
    else gap_bwd_kernel<bf16_t><<<blocks_for((total + 7) / 8, kThreads, kMaxBlocks), kThreads, 0, s>>>(dpooled, (bf16_t*)dx, total, HW);
    return mtp_launch_status();
}

extern "C" int mtp_cls_ce(const float* pooled, const float* w, const float* b, const int64_t* labels, float loss_weight, float* logits, float* prob,
                          int64_t* pred, float* loss_rows, float* loss, float* dlogits, uint32_t* counter, int64_t N, int64_t C, int64_t K,
                          mtp_stream_t stream) {
    MTP_CHECK_ARG(pooled && w && b && logits && N > 0 && C > 0 && K > 0 && N < INT32_MAX && C < INT32_MAX && K < INT32_MAX);
    MTP_CHECK_ARG(labels || (!loss_rows && !loss && !dlogits));      // evaluation: no loss, no gradient
    MTP_CHECK_ARG(!loss || (loss_rows && counter));                  // the scalar is the sum of the published per-sample losses
    const bool vec = (C % 4) == 0 && (((uintptr_t)pooled | (uintptr_t)w) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        cls_ce_kernel<true><<<(unsigned)N, kThreads, 0, s>>>(pooled, w, b, labels, loss_weight, logits, prob, pred, loss_rows, loss, dlogits, counter, (int)N,
                                                            (int)C, (int)K);
    else
        cls_ce_kernel<false><<<(unsigned)N, kThreads, 0, s>>>(pooled, w, b, labels, loss_weight, logits, prob, pred, loss_rows, loss, dlogits, counter, (int)N,
                                                             (int)C, (int)K);
    return mtp_launch_status();
}

extern "C" int mtp_cls_head_bwd(const float* dlogits, const float* pooled, const float* w, float* dw, float* db, float* dpooled, int64_t N, int64_t C,
                                int64_t K, int accumulate, mtp_stream_t stream) {
    MTP_CHECK_ARG(dlogits && pooled && w && dw && db && N > 0 && C > 0 && K > 0 && N < INT32_MAX && C < INT32_MAX && K < INT32_MAX);
    cls_head_bwd_kernel<<<blocks_for(K * C + (dpooled ? N * C : 0) + K, kThreads, kMaxBlocks), kThreads, 0, (hipStream_t)stream>>>(dlogits, pooled, w, dw, db, dpooled, (int)N,
                                                                                                               (int)C, (int)K, accumulate);
    return mtp_launch_status();
}

extern "C" int mtp_cls_hits(const float* scores, const int64_t* labels, int64_t N, int64_t K, const int32_t* topk, int nk, float thr, int use_thr,
                            int64_t* counters, mtp_stream_t stream) {
    MTP_CHECK_ARG(scores && labels && topk && counters && N > 0 && K > 0 && K < INT32_MAX && nk > 0 && nk <= kMaxTopk);
    TopkList t;
    t.n = nk;
    for (int i = 0; i < kMaxTopk; ++i) t.k[i] = i < nk ? topk[i] : 0;
    for (int i = 0; i < nk; ++i) MTP_CHECK_ARG(t.k[i] >= 1 && t.k[i] <= K && (i == 0 || t.k[i] > t.k[i - 1]));
    cls_hits_kernel<<<blocks_for(N, kWaves, kMaxBlocks), kThreads, 0, (hipStream_t)stream>>>(scores, labels, N, (int)K, t, thr, use_thr,
                                                                                                     reinterpret_cast<unsigned long long*>(counters));
    return mtp_launch_status();
}
