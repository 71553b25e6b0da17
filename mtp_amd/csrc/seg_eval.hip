// Segmentation evaluation (mmseg EncoderDecoder.slide_inference + IoUMetric, Multi-Task_Pretrain/semantic_segmentation/encoder_decoder.py:253-310,
// metric.py:164-200): the passes behind the decode head's low-resolution logits.  The layout is the head's: channels-last rows with a row pitch, f32
// accumulation.  All three kernels are bound by memory traffic: one 16-byte access per lane and class group, consecutive lanes on consecutive addresses.
//   window accumulate   acc[n, y1 + oy, x1 + ox, :] += bilinear(logits[n])[oy, ox, :]   one launch per window position, windows in stream order (no atomics)
//   argmax + areas      one pass over the accumulator: / window count, arg-max over the first K columns, optional NCHW logits, optional histograms
//   areas               the same histograms from an existing prediction map
// Histograms are integers: per-workgroup int32 counters in LDS, flushed with 64-bit integer atomic adds, so the result does not depend on the order.
#include "common.h"
#include "resize_common.h"

namespace {

constexpr int kMaxClasses = 256;      // 3 x 256 int32 counters per workgroup

// one thread per (image, crop pixel, 4 classes): resize_fwd_kernel's arithmetic (decode_head.hip) with the destination a window of a larger map
template <typename TX>
__global__ void __launch_bounds__(kThreads) window_accumulate_kernel(const void* x, int64_t ldx, float* acc, int64_t lda, int64_t N, int h, int w, int Hc,
                                                                     int Wc, int H, int W, int y1, int x1, int64_t C4) {
    const int64_t total = N * Hc * Wc * C4;
    const float sy = (float)h / (float)Hc, sx = (float)w / (float)Wc;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        const int64_t pix = i / C4, c = (i - pix * C4) * 4;
        const int ox = (int)(pix % Wc), oy = (int)((pix / Wc) % Hc);
        const int64_t n = pix / ((int64_t)Wc * Hc);
        const Lin ly = lin_index(oy, h, sy), lx = lin_index(ox, w, sx);
        const int64_t b = n * h * w;
        const float4 v00 = ld4<TX>(x, (b + (int64_t)ly.i0 * w + lx.i0) * ldx + c), v01 = ld4<TX>(x, (b + (int64_t)ly.i0 * w + lx.i1) * ldx + c);
        const float4 v10 = ld4<TX>(x, (b + (int64_t)ly.i1 * w + lx.i0) * ldx + c), v11 = ld4<TX>(x, (b + (int64_t)ly.i1 * w + lx.i1) * ldx + c);
        // ATen's order: h0lambda * (w0lambda * v00 + w1lambda * v01) + h1lambda * (w0lambda * v10 + w1lambda * v11)
        const float4 t0 = f4add(f4scale(v00, lx.w0), f4scale(v01, lx.w1)), t1 = f4add(f4scale(v10, lx.w0), f4scale(v11, lx.w1));
        const float4 o = f4add(f4scale(t0, ly.w0), f4scale(t1, ly.w1));
        float* d = acc + ((n * H + (y1 + oy)) * W + (x1 + ox)) * lda + c;
        store4(d, f4add(load4(d), o));      // preds += pad(crop logits)
    }
}

// ---------------------------------------------------------------------------------------------------------------- histograms
// hist = [intersect | pred | label][K] of this workgroup; a label outside [0, K) that is not ignore_index (the host wrapper refuses it) counts nowhere
__device__ __forceinline__ void hist_count(int* hist, int K, int pred, int64_t lab, int ignore_index) {
    if (lab == (int64_t)ignore_index || lab < 0 || lab >= K || pred < 0 || pred >= K) return;
    atomicAdd(&hist[K + pred], 1);
    atomicAdd(&hist[2 * K + (int)lab], 1);
    if (lab == pred) atomicAdd(&hist[pred], 1);
}
__device__ __forceinline__ void hist_zero(int* hist, int K) {
    for (int t = threadIdx.x; t < 3 * K; t += kThreads) hist[t] = 0;
    __syncthreads();
}
__device__ __forceinline__ void hist_flush(const int* hist, int K, unsigned long long* areas) {
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * K; t += kThreads)
        if (hist[t] != 0) atomicAdd(&areas[t], (unsigned long long)hist[t]);
}

// one thread per pixel, the classes in groups of four.  First strict maximum = the lowest index among ties (torch.argmax); columns >= K never compared.
template <typename TL>
__global__ void __launch_bounds__(kThreads) argmax_areas_kernel(float* acc, int64_t lda, int64_t N, int H, int W, int K, const int32_t* cy, const int32_t* cx,
                                                                int write_back, uint8_t* pred, float* seg, const TL* labels, int ignore_index,
                                                                unsigned long long* areas) {
    __shared__ int hist[3 * kMaxClasses];
    if (areas) hist_zero(hist, K);
    const int64_t HW = (int64_t)H * W, total = N * HW;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < total; p += (int64_t)gridDim.x * kThreads) {
        const int64_t n = p / HW, q = p - n * HW;
        const int y = (int)(q / W), x = (int)(q - (int64_t)y * W);
        const bool div = cy != nullptr;
        const float cnt = div ? (float)(cy[y] * cx[x]) : 1.0f;
        float* row = acc + p * lda;
        float* so = seg ? seg + n * K * HW + q : nullptr;
        float best = 0.0f;
        int bi = 0;
        for (int c = 0; c < K; c += 4) {
            float4 v4 = load4(row + c);
            if (div) v4 = make_float4(v4.x / cnt, v4.y / cnt, v4.z / cnt, v4.w / cnt);      // preds / count_mat: IEEE division, as torch
            if (write_back) store4(row + c, v4);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = c + j;
                if (k < K) {
                    if (so) so[(int64_t)k * HW] = v[j];
                    if (k == 0 || v[j] > best) {
                        best = v[j];
                        bi = k;
                    }
                }
            }
        }
        if (pred) pred[p] = (uint8_t)bi;
        if (areas) hist_count(hist, K, bi, (int64_t)labels[p], ignore_index);
    }
    if (areas) hist_flush(hist, K, areas);
}

template <typename TP, typename TL>
__global__ void __launch_bounds__(kThreads) areas_kernel(const TP* pred, const TL* labels, int64_t total, int K, int ignore_index, unsigned long long* areas) {
    __shared__ int hist[3 * kMaxClasses];
    hist_zero(hist, K);
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < total; p += (int64_t)gridDim.x * kThreads) {
        const int64_t pr = (int64_t)pred[p];
        hist_count(hist, K, pr >= 0 && pr < K ? (int)pr : -1, (int64_t)labels[p], ignore_index);
    }
    hist_flush(hist, K, areas);
}

// every workgroup's int32 counters hold at most its own pixels: total / grid, far below 2^31 for total < 2^40
constexpr int64_t kMaxPixels = (int64_t)1 << 40;

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_seg_window_accumulate(const void* logits, int dtype, int64_t ld, int64_t N, int64_t h, int64_t w, int64_t K, float* acc, int64_t lda,
                                         int64_t H, int64_t W, int64_t y1, int64_t x1, int64_t Hc, int64_t Wc, mtp_stream_t stream) {
    MTP_CHECK_ARG(logits && acc && N > 0 && h > 0 && w > 0 && K > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0 && dt_ok(dtype));
    MTP_CHECK_ARG(h < INT32_MAX && w < INT32_MAX && H < INT32_MAX && W < INT32_MAX && K < INT32_MAX);
    const int64_t K4 = (K + 3) / 4 * 4;
    MTP_CHECK_ARG(ld >= K4 && lda >= K4 && (ld % 4) == 0 && (lda % 4) == 0 && ((uintptr_t)acc & 15) == 0);
    MTP_CHECK_ARG(((uintptr_t)logits & (dtype == MTP_F32 ? 15 : 7)) == 0);
    MTP_CHECK_ARG(y1 >= 0 && x1 >= 0 && Hc <= H && Wc <= W && y1 <= H - Hc && x1 <= W - Wc && N * H * W < kMaxPixels);
    const int64_t total = N * Hc * Wc * (K4 / 4);
    if (dtype == MTP_F32)
        window_accumulate_kernel<float><<<blocks_for(total, kThreads, kMaxBlocks), kThreads, 0, (hipStream_t)stream>>>(logits, ld, acc, lda, N, (int)h, (int)w, (int)Hc, (int)Wc, (int)H,
                                                                                                 (int)W, (int)y1, (int)x1, K4 / 4);
    else
        window_accumulate_kernel<bf16_t><<<blocks_for(total, kThreads, kMaxBlocks), kThreads, 0, (hipStream_t)stream>>>(logits, ld, acc, lda, N, (int)h, (int)w, (int)Hc, (int)Wc, (int)H,
                                                                                                  (int)W, (int)y1, (int)x1, K4 / 4);
    return mtp_launch_status();
}

extern "C" int mtp_seg_argmax_areas(float* acc, int64_t lda, int64_t N, int64_t H, int64_t W, int64_t K, const int32_t* cy, const int32_t* cx, int write_back,
                                    uint8_t* pred, float* seg_logits, const void* labels, int label_bytes, int ignore_index, int64_t* areas,
                                    mtp_stream_t stream) {
    MTP_CHECK_ARG(acc && N > 0 && H > 0 && W > 0 && K > 0 && K <= kMaxClasses && H < INT32_MAX && W < INT32_MAX && N * H * W < kMaxPixels);
    MTP_CHECK_ARG(lda >= (K + 3) / 4 * 4 && (lda % 4) == 0 && ((uintptr_t)acc & 15) == 0);
    MTP_CHECK_ARG((cy == nullptr) == (cx == nullptr) && (labels == nullptr) == (areas == nullptr) && (!labels || label_bytes == 1 || label_bytes == 8));
    MTP_CHECK_ARG(pred || seg_logits || areas || write_back);
    const unsigned g = blocks_for(N * H * W, kThreads, kMaxBlocks);
    unsigned long long* ar = reinterpret_cast<unsigned long long*>(areas);
    hipStream_t s = (hipStream_t)stream;
    if (labels && label_bytes == 8)
        argmax_areas_kernel<int64_t><<<g, kThreads, 0, s>>>(acc, lda, N, (int)H, (int)W, (int)K, cy, cx, write_back, pred, seg_logits, (const int64_t*)labels,
                                                            ignore_index, ar);
    else
        argmax_areas_kernel<uint8_t><<<g, kThreads, 0, s>>>(acc, lda, N, (int)H, (int)W, (int)K, cy, cx, write_back, pred, seg_logits, (const uint8_t*)labels,
                                                            ignore_index, ar);
    return mtp_launch_status();
}

extern "C" int mtp_seg_areas(const void* pred, int pred_bytes, const void* labels, int label_bytes, int64_t pixels, int64_t K, int ignore_index, int64_t* areas,
                             mtp_stream_t stream) {
    MTP_CHECK_ARG(pred && labels && areas && pixels > 0 && pixels < kMaxPixels && K > 0 && K <= kMaxClasses);
    MTP_CHECK_ARG((pred_bytes == 1 || pred_bytes == 8) && (label_bytes == 1 || label_bytes == 8));
    const unsigned g = blocks_for(pixels, kThreads, kMaxBlocks);
    unsigned long long* ar = reinterpret_cast<unsigned long long*>(areas);
    hipStream_t s = (hipStream_t)stream;
    if (pred_bytes == 1 && label_bytes == 1)
        areas_kernel<uint8_t, uint8_t><<<g, kThreads, 0, s>>>((const uint8_t*)pred, (const uint8_t*)labels, pixels, (int)K, ignore_index, ar);
    else if (pred_bytes == 1)
        areas_kernel<uint8_t, int64_t><<<g, kThreads, 0, s>>>((const uint8_t*)pred, (const int64_t*)labels, pixels, (int)K, ignore_index, ar);
    else if (label_bytes == 1)
        areas_kernel<int64_t, uint8_t><<<g, kThreads, 0, s>>>((const int64_t*)pred, (const uint8_t*)labels, pixels, (int)K, ignore_index, ar);
    else
        areas_kernel<int64_t, int64_t><<<g, kThreads, 0, s>>>((const int64_t*)pred, (const int64_t*)labels, pixels, (int)K, ignore_index, ar);
    return mtp_launch_status();
}
