// The DOTA mAP metric of rotated detection (Multi-Task_Pretrain/rotated_detection/metric.py: tpfp_default, get_cls_results, eval_rbbox_map, and
// mmdet's average_precision behind them).  The reference calls box_iou_rotated once per (class, image) and walks the detections in Python; here three
// launches serve any number of images and classes.  f32 boxes, int64 indices, integer atomics only, two calls give the same bits.
//   det_match  one wave per detection; the lanes stride the gts of the detection's image and skip other labels: f32 rotated IoU (the text of
//              rbox_geom.h, detection first, as box_iou_rotated(dets, gts)), the wave maximum and the FIRST gt attaining it (np.argmax over the
//              image's gts in table order: non-ignored first, then ignored).  An image whose first gt is ignored has no non-ignored gt and counts as
//              having none at all (get_cls_results, metric.py:219-232).  Then per threshold t: best_iou >= thr_t (float32 compare) and the gt not
//              ignored -> 64-bit atomicMax of (order-preserving u32 of the score << 32 | ~detection index) into winner[t][gt].
//   det_tpfp   per (t, detection): tp = it owns winner[t][best_gt]; fp = no gt, below thr_t, or a non-ignored gt owned by another; neither when the
//              gt is ignored.  The greedy loop of metric.py:168-180 is VOC-style: a detection's target gt is its arg-max and never depends on what
//              is covered already, so the true positive of a gt is exactly its best-scoring qualifying detection (lower index among equal scores)
//              and no sequential scan is needed.  The same launch counts the non-ignored gts per class (integer atomics).
//   det_ap     one workgroup per (class, threshold) walks the class's score-sorted segment in chunks of 256 with an integer carry: cumulative tp /
//              fp are exact; recall = tp / max(num_gts, eps32) in float64, precision = tp / max(tp + fp, eps32) in float32, correctly rounded (the
//              reference's dtypes, metric.py:342-346).  '11points': eleven running maxima of precision over recall >= point_k (a maximum is
//              order-free), summed in ascending k and divided by 11 in float32: bit-equal to average_precision.  'area': a second, reverse walk
//              with a running suffix maximum, sum over the true positives of (r_i - r_{i-1}) * suffixmax_i in float64 in a fixed order.
#include "block_scan.h"
#include "common.h"
#include "rbox_geom.h"

#pragma clang fp contract(off)

namespace {

constexpr float kEps32 = 1.1920928955078125e-07f;      // np.finfo(np.float32).eps
constexpr unsigned char kTp = 1, kFp = 2;

struct DetThr {
    float v[MTP_DET_MAX_THRS];
};
struct ApPoints {
    double v[MTP_DET_AP_POINTS];
};

// larger float -> larger unsigned
__device__ __forceinline__ unsigned ordered_u32(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long det_key(float score, int64_t d) {      // d < 2^32 - 1: never 0
    return ((unsigned long long)ordered_u32(score) << 32) | (0xffffffffull - (unsigned long long)d);
}

// ------------------------------------------------------------------------------------------------------------------- matching
__global__ void __launch_bounds__(kThreads) det_match_kernel(const float* __restrict__ det_boxes, const float* __restrict__ det_scores,
                                                             const int64_t* __restrict__ det_labels, const int64_t* __restrict__ det_img, int64_t D,
                                                             const float* __restrict__ gt_boxes, const int64_t* __restrict__ gt_labels,
                                                             const unsigned char* __restrict__ gt_ignore, const int64_t* __restrict__ gt_start,
                                                             int64_t I, int64_t G, DetThr thr, int T, float* __restrict__ best_iou,
                                                             int64_t* __restrict__ best_gt, unsigned long long* winner) {
    const int lane = threadIdx.x & (MTP_WAVE - 1);
    const int64_t waves = (int64_t)gridDim.x * (kThreads / MTP_WAVE);
    for (int64_t d = (int64_t)blockIdx.x * (kThreads / MTP_WAVE) + threadIdx.x / MTP_WAVE; d < D; d += waves) {      // wave-uniform
        const int64_t img = det_img[d], label = det_labels[d];
        int64_t s = 0, e = 0;
        if (img >= 0 && img < I) {
            s = gt_start[img];
            e = gt_start[img + 1];
        }
        if (s < 0) s = 0;
        if (e > G) e = G;
        if (s < e && gt_ignore[s]) e = s;      // non-ignored gts come first: none of them -> the image has no gts at all
        const RBox a = load_rbox(det_boxes + d * 5);
        float best = -1.0f;
        int64_t arg = -1;
        for (int64_t g = s + lane; g < e; g += MTP_WAVE) {
            if (gt_labels[g] != label) continue;
            const float ov = box_iou(a, load_rbox(gt_boxes + g * 5), 0, 0.0f);
            if (ov > best) {      // strict: the lowest index of this lane among ties
                best = ov;
                arg = g;
            }
        }
        float m = best;
        for (int off = MTP_WAVE / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        long long cand = (arg >= 0 && best == m) ? (long long)arg : 0x7fffffffffffffffll;
        for (int off = MTP_WAVE / 2; off > 0; off >>= 1) {
            const long long o = __shfl_xor(cand, off);
            cand = o < cand ? o : cand;
        }
        const bool found = m >= 0.0f;
        const int64_t g = found ? (int64_t)cand : -1;
        if (lane == 0) {
            best_iou[d] = found ? m : 0.0f;
            best_gt[d] = g;
        }
        if (found && lane < T && m >= thr.v[lane] && !gt_ignore[g]) atomicMax(&winner[(int64_t)lane * G + g], det_key(det_scores[d], d));
    }
}

// ------------------------------------------------------------------------------------------------------------------- tp / fp flags, gt counts
__global__ void __launch_bounds__(kThreads) det_tpfp_kernel(const float* __restrict__ det_scores, const float* __restrict__ best_iou,
                                                            const int64_t* __restrict__ best_gt, int64_t D, const int64_t* __restrict__ gt_labels,
                                                            const unsigned char* __restrict__ gt_ignore, int64_t G, DetThr thr, int T,
                                                            const unsigned long long* __restrict__ winner, int64_t K,
                                                            unsigned char* __restrict__ flags, unsigned long long* num_gts) {
    const int64_t stride = (int64_t)gridDim.x * kThreads, first = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (int64_t i = first; i < (int64_t)T * D; i += stride) {
        const int64_t t = i / D, d = i - t * D;
        const int64_t g = best_gt[d];
        unsigned char f;
        if (g < 0 || g >= G || !(best_iou[d] >= thr.v[t])) f = kFp;
        else if (gt_ignore[g]) f = 0;
        else f = winner[t * G + g] == det_key(det_scores[d], d) ? kTp : kFp;
        flags[i] = f;
    }
    for (int64_t g = first; g < G; g += stride) {
        const int64_t l = gt_labels[g];
        if (!gt_ignore[g] && l >= 0 && l < K) atomicAdd(&num_gts[l], 1ull);
    }
}

// ------------------------------------------------------------------------------------------------------------------- average precision
// (block_scan_add, the exact inclusive sum in thread order, is block_scan.h)
// max over the threads tid .. 255 (a suffix maximum, order-free); total = the maximum of all
__device__ __forceinline__ float block_suffix_max(float v, float* wmax, int tid, float& total) {
    const int lane = tid & (MTP_WAVE - 1), w = tid / MTP_WAVE;
    for (int off = 1; off < MTP_WAVE; off <<= 1) {
        const float o = __shfl_down(v, off);
        if (lane + off < MTP_WAVE) v = fmaxf(v, o);
    }
    __syncthreads();
    if (lane == 0) wmax[w] = v;
    __syncthreads();
    float all = wmax[0];
    for (int i = 1; i < kThreads / MTP_WAVE; ++i) {
        if (i > w) v = fmaxf(v, wmax[i]);
        all = fmaxf(all, wmax[i]);
    }
    total = all;
    return v;
}

// the sum of 256 doubles in one fixed order: a butterfly inside each wave, then the four waves in order
__device__ __forceinline__ double block_sum_fixed(double v, double* wsum, int tid) {
    const int lane = tid & (MTP_WAVE - 1), w = tid / MTP_WAVE;
    for (int off = MTP_WAVE / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    __syncthreads();
    if (lane == 0) wsum[w] = v;
    __syncthreads();
    double all = wsum[0];
    for (int i = 1; i < kThreads / MTP_WAVE; ++i) all = all + wsum[i];
    return all;
}

__device__ __forceinline__ unsigned long long flag_counts(unsigned char f) {      // tp count << 32 | fp count
    return ((unsigned long long)(f == kTp) << 32) | (unsigned long long)(f == kFp);
}
// the flag of list position i; an index outside the table (a caller's mistake) reads as "neither"
__device__ __forceinline__ unsigned char flag_at(const unsigned char* f, const int64_t* order, int64_t i, int64_t D) {
    const int64_t d = order[i];
    return d >= 0 && d < D ? f[d] : (unsigned char)0;
}
__device__ __forceinline__ float precision_of(unsigned tp, unsigned fp) { return __fdiv_rn((float)tp, fmaxf((float)(tp + fp), kEps32)); }

// grid (K, T).  flags (T, D) in table order, order (D): position in the class-major, score-descending list -> detection; cls_start (K + 1).
__global__ void __launch_bounds__(kThreads) det_ap_kernel(const unsigned char* __restrict__ flags, const int64_t* __restrict__ order,
                                                          const int64_t* __restrict__ cls_start, const int64_t* __restrict__ num_gts, int64_t D, int64_t K,
                                                          int area, ApPoints pts, float* __restrict__ ap, int64_t* __restrict__ num_dets,
                                                          double* __restrict__ last_recall, double* __restrict__ recall, float* __restrict__ precision) {
    __shared__ unsigned long long wsum[kThreads / MTP_WAVE];
    __shared__ float wmax[kThreads / MTP_WAVE];
    __shared__ double dsum[kThreads / MTP_WAVE];
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x, t = blockIdx.y;
    int64_t s = cls_start[k], e = cls_start[k + 1];
    if (s < 0) s = 0;
    if (e > D) e = D;
    if (e < s) e = s;
    const int64_t n = num_gts[k];
    const double den = fmax((double)n, (double)kEps32);
    const unsigned char* f = flags + t * D;
    float pmax[MTP_DET_AP_POINTS];
#pragma unroll
    for (int j = 0; j < MTP_DET_AP_POINTS; ++j) pmax[j] = 0.0f;      // precision >= 0: "no position reaches the point" reads as 0 too
    unsigned long long carry = 0ull, total;
    for (int64_t c0 = s; c0 < e; c0 += kThreads) {
        const int64_t i = c0 + tid;
        const unsigned long long cum = carry + block_scan_add(i < e ? flag_counts(flag_at(f, order, i, D)) : 0ull, wsum, tid, total);
        carry += total;
        if (i < e) {
            const unsigned tp = (unsigned)(cum >> 32), fp = (unsigned)cum;
            const double r = (double)tp / den;
            const float p = precision_of(tp, fp);
            if (recall) recall[t * D + i] = r;
            if (precision) precision[t * D + i] = p;
#pragma unroll
            for (int j = 0; j < MTP_DET_AP_POINTS; ++j)
                if (r >= pts.v[j]) pmax[j] = fmaxf(pmax[j], p);
        }
    }
    float result;
    if (!area) {
        float sum = 0.0f, all;
        for (int j = 0; j < MTP_DET_AP_POINTS; ++j) {      // ascending k, float32, as `ap[i] += prec`
            block_suffix_max(pmax[j], wmax, tid, all);
            sum = sum + all;
        }
        result = __fdiv_rn(sum, 11.0f);
    } else {
        // the reverse walk over the same chunks: the counts before a chunk are the counts after it minus its own
        double acc = 0.0;
        float later = 0.0f;      // the maximum precision of the positions after the chunk (mpre's zero padding at the end)
        unsigned long long after = carry;
        const int64_t chunks = (e - s + kThreads - 1) / kThreads;
        for (int64_t c = chunks - 1; c >= 0; --c) {
            const int64_t i = s + c * kThreads + tid;
            const unsigned char fl = i < e ? flag_at(f, order, i, D) : (unsigned char)0;
            const unsigned long long inc = block_scan_add(i < e ? flag_counts(fl) : 0ull, wsum, tid, total);
            const unsigned long long cum = (after - total) + inc;
            const unsigned tp = (unsigned)(cum >> 32), fp = (unsigned)cum;
            float chunk_max;
            const float smax = fmaxf(block_suffix_max(i < e ? precision_of(tp, fp) : 0.0f, wmax, tid, chunk_max), later);
            double term = 0.0;
            if (i < e && fl == kTp) term = ((double)tp / den - (double)(tp - 1u) / den) * (double)smax;
            acc = acc + block_sum_fixed(term, dsum, tid);
            later = fmaxf(later, chunk_max);
            after -= total;
        }
        result = (float)acc;
    }
    if (tid == 0) {
        ap[t * K + k] = result;
        last_recall[t * K + k] = e > s ? (double)(unsigned)(carry >> 32) / den : 0.0;
        if (t == 0) num_dets[k] = e - s;
    }
}

bool thresholds(const float* iou_thrs, int T, DetThr& thr) {
    if (!iou_thrs || T < 1 || T > MTP_DET_MAX_THRS) return false;
    for (int t = 0; t < MTP_DET_MAX_THRS; ++t) thr.v[t] = t < T ? iou_thrs[t] : 2.0f;
    return true;
}

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_det_match(const float* det_boxes, const float* det_scores, const int64_t* det_labels, const int64_t* det_img, int64_t D,
                             const float* gt_boxes, const int64_t* gt_labels, const uint8_t* gt_ignore, const int64_t* gt_start, int64_t I, int64_t G,
                             const float* iou_thrs, int T, float* best_iou, int64_t* best_gt, void* winner, int64_t winner_bytes, mtp_stream_t stream) {
    DetThr thr;
    MTP_CHECK_ARG(det_boxes && det_scores && det_labels && det_img && best_iou && best_gt && D > 0 && D < (((int64_t)1 << 32) - 1));
    MTP_CHECK_ARG(thresholds(iou_thrs, T, thr) && I >= 0 && G >= 0 && G < ((int64_t)1 << 40) && (I == 0 || gt_start));
    MTP_CHECK_ARG(G == 0 || (gt_boxes && gt_labels && gt_ignore && gt_start && winner && winner_bytes >= (int64_t)T * G * 8 && ((uintptr_t)winner & 7) == 0));
    const unsigned grid = blocks_for(D, kThreads / MTP_WAVE, 4 * kMaxBlocks);
    det_match_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(det_boxes, det_scores, det_labels, det_img, D, gt_boxes, gt_labels, gt_ignore, gt_start, I,
                                                                 G, thr, T, best_iou, best_gt, static_cast<unsigned long long*>(winner));
    return mtp_launch_status();
}

extern "C" int mtp_det_tpfp(const float* det_scores, const float* best_iou, const int64_t* best_gt, int64_t D, const int64_t* gt_labels,
                            const uint8_t* gt_ignore, int64_t G, const float* iou_thrs, int T, const void* winner, int64_t K, uint8_t* flags,
                            int64_t* num_gts, mtp_stream_t stream) {
    DetThr thr;
    MTP_CHECK_ARG(det_scores && best_iou && best_gt && flags && num_gts && D > 0 && D < (((int64_t)1 << 32) - 1));
    MTP_CHECK_ARG(thresholds(iou_thrs, T, thr) && G >= 0 && G < ((int64_t)1 << 40) && K > 0 && K <= MTP_DET_MAX_CLASSES);
    MTP_CHECK_ARG(G == 0 || (gt_labels && gt_ignore && winner && ((uintptr_t)winner & 7) == 0));
    const int64_t work = (int64_t)T * D > G ? (int64_t)T * D : G;
    det_tpfp_kernel<<<blocks_for(work, kThreads, kMaxBlocks), kThreads, 0, (hipStream_t)stream>>>(
        det_scores, best_iou, best_gt, D, gt_labels, gt_ignore, G, thr, T, static_cast<const unsigned long long*>(winner), K, flags,
        reinterpret_cast<unsigned long long*>(num_gts));
    return mtp_launch_status();
}

extern "C" int mtp_det_ap(const uint8_t* flags, const int64_t* order, const int64_t* cls_start, const int64_t* num_gts, int64_t D, int64_t K, int T,
                          int mode, const double* recall_points, float* ap, int64_t* num_dets, double* last_recall, double* recall, float* precision,
                          mtp_stream_t stream) {
    MTP_CHECK_ARG(cls_start && num_gts && ap && num_dets && last_recall && K > 0 && K <= MTP_DET_MAX_CLASSES && T >= 1 && T <= MTP_DET_MAX_THRS);
    MTP_CHECK_ARG(D >= 0 && D < (((int64_t)1 << 32) - 1) && (D == 0 || (flags && order)) && (mode == MTP_DET_AP_11POINTS || mode == MTP_DET_AP_AREA));
    MTP_CHECK_ARG(mode == MTP_DET_AP_AREA || recall_points);
    ApPoints pts;
    for (int j = 0; j < MTP_DET_AP_POINTS; ++j) pts.v[j] = mode == MTP_DET_AP_11POINTS ? recall_points[j] : 2.0;
    det_ap_kernel<<<dim3((unsigned)K, (unsigned)T), kThreads, 0, (hipStream_t)stream>>>(flags, order, cls_start, num_gts, D, K, mode == MTP_DET_AP_AREA, pts,
                                                                                        ap, num_dets, last_recall, recall, precision);
    return mtp_launch_status();
}
