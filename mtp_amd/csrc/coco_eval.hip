// The COCO-style metric of instance segmentation (Multi-Task_Pretrain/instance_segmentation/metric.py, MTP_IS_Metric = mmdet's CocoMetric, which
// hands all arithmetic to pycocotools' COCOeval: computeIoU, evaluateImg, accumulate).  The reference copies every mask to the host, RLE-encodes it,
// writes json files and loops in Python per (image, category, area range); here four kernels work on device tables.  float64 arithmetic with
// contraction off and correctly rounded divisions, integer atomics only, two calls give the same bits.
//   mask_pack        (N, H*W) u8 masks -> (N, ceil(H*W / 64)) 64-bit words, one __ballot per 64 pixels (bit p of word w = pixel 64 w + p, the tail
//                    zero) and the pixel counts by popcount.  One read of the masks.
//   coco_iou         per image of a batch a dense (D_i, G_i) float64 block at host-known offsets.  bbox: one thread per pair, maskApi.c's bbIou on
//                    x, y, w, h doubles (w = x2 - x1 in double on the float32 corners).  segm: one wave per pair, AND + popcount over the words, the
//                    integer intersection reduced over the wave; union = crowd ? a_d : a_d + a_g - i; an empty intersection is 0 without a division.
//                    Pairs of different labels are 0 unless category-agnostic.
//   coco_match       one wave per (cell = image x category, area range) loops over the thresholds and walks the cell's detections SEQUENTIALLY in
//                    score order (evaluateImg's greedy rule depends on what is taken already).  The lanes stride the cell's gts in the order sorted
//                    by gtIg; lane l keeps the taken bits of gts l, l + 64, ... in one 64-bit register (MTP_COCO_MAX_CELL_GTS = 64 x 64).  The pick
//                    is the wave maximum of (non-ignored before ignored, IoU, position): the largest IoU >= min(t, 1 - 1e-10) among the available
//                    non-ignored gts, the highest position among equal IoUs, else the same among the ignored ones.
//   coco_accumulate  one workgroup per (category, area range, maxDet, threshold) over the category's score-sorted list; a detection counts when its
//                    rank in its cell is below maxDet.  Exact integer chunked scans for tp / fp; rc = tp / npig, pr = tp / (fp + tp + 2^-52); a walk
//                    from the right carries the suffix maximum of pr; the position where rc first reaches a recall threshold writes that
//                    threshold's precision and score (rc only grows at a true positive, so only those positions and the first one look).
#include "block_scan.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWaves = kThreads / MTP_WAVE;
constexpr int kIouImgs = 32;      // images per coco_iou launch: their offsets travel as kernel arguments

struct CocoImgs {
    int64_t det_start[kIouImgs + 1], gt_start[kIouImgs + 1], out_start[kIouImgs];
};
struct CocoThr {
    double v[MTP_COCO_MAX_THRS];
};
struct CocoAreas {
    double lo[MTP_COCO_AREAS], hi[MTP_COCO_AREAS];
};
struct CocoRec {
    double v[MTP_COCO_REC_THRS];
};
struct CocoMaxDets {
    int v[MTP_COCO_MAX_DET_LEVELS];
};

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int off = MTP_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ------------------------------------------------------------------------------------------------------------------- pack
// grid (x, y): y strides the masks, the waves of x stride the words of one mask
__global__ void __launch_bounds__(kThreads) mask_pack_kernel(const unsigned char* __restrict__ masks, int64_t N, int64_t HW, int64_t W,
                                                             unsigned long long* __restrict__ words, unsigned long long* areas) {
    const int lane = threadIdx.x & (MTP_WAVE - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWaves + threadIdx.x / MTP_WAVE, waves = (int64_t)gridDim.x * kWaves;
    for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
        const unsigned char* m = masks + n * HW;
        long long count = 0;
        for (int64_t w = wave; w < W; w += waves) {      // wave-uniform
            const int64_t p = w * 64 + lane;
            const unsigned long long bits = __ballot(p < HW && m[p] != 0);
            if (lane == 0) words[n * W + w] = bits;
            count += __popcll(bits);
        }
        if (lane == 0 && count) atomicAdd(&areas[n], (unsigned long long)count);
    }
}

// ------------------------------------------------------------------------------------------------------------------- IoU
// maskApi.c bbIou on (x, y, w, h) doubles
__device__ __forceinline__ double bb_iou(const float* d, const float* g, bool crowd) {
    const double dx = (double)d[0], dy = (double)d[1], dw = (double)d[2] - (double)d[0], dh = (double)d[3] - (double)d[1];
    const double gx = (double)g[0], gy = (double)g[1], gw = (double)g[2] - (double)g[0], gh = (double)g[3] - (double)g[1];
    const double ga = gw * gh, da = dw * dh;
    const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
    if (!(w > 0.0)) return 0.0;
    const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
    if (!(h > 0.0)) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : (da + ga) - i;
    return __ddiv_rn(i, u);
}

// grid (x, images of this launch)
__global__ void __launch_bounds__(kThreads) coco_iou_bbox_kernel(const float* __restrict__ det_boxes, const int64_t* __restrict__ det_labels,
                                                                 const float* __restrict__ gt_boxes, const int64_t* __restrict__ gt_labels,
                                                                 const unsigned char* __restrict__ gt_crowd, int agnostic, CocoImgs im,
                                                                 double* __restrict__ iou) {
    const int s = blockIdx.y;
    const int64_t d0 = im.det_start[s], g0 = im.gt_start[s], ng = im.gt_start[s + 1] - g0, pairs = (im.det_start[s + 1] - d0) * ng;
    double* out = iou + im.out_start[s];
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * kThreads) {
        const int64_t d = d0 + i / ng, g = g0 + i % ng;
        double v = 0.0;
        if (agnostic || det_labels[d] == gt_labels[g]) v = bb_iou(det_boxes + d * 4, gt_boxes + g * 4, gt_crowd[g] != 0);
        out[i] = v;
    }
}

__global__ void __launch_bounds__(kThreads) coco_iou_segm_kernel(const unsigned long long* __restrict__ det_words, const int64_t* __restrict__ det_areas,
                                                                 const int64_t* __restrict__ det_labels, const unsigned long long* __restrict__ gt_words,
                                                                 const int64_t* __restrict__ gt_areas, const int64_t* __restrict__ gt_labels,
                                                                 const unsigned char* __restrict__ gt_crowd, int64_t W, int agnostic, CocoImgs im,
                                                                 double* __restrict__ iou, int64_t* __restrict__ inter) {
    const int s = blockIdx.y, lane = threadIdx.x & (MTP_WAVE - 1);
    const int64_t d0 = im.det_start[s], g0 = im.gt_start[s], ng = im.gt_start[s + 1] - g0, pairs = (im.det_start[s + 1] - d0) * ng;
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    for (int64_t i = (int64_t)blockIdx.x * kWaves + threadIdx.x / MTP_WAVE; i < pairs; i += waves) {      // wave-uniform
        const int64_t d = d0 + i / ng, g = g0 + i % ng;
        long long n = 0;
        if (agnostic || det_labels[d] == gt_labels[g]) {
            const unsigned long long *a = det_words + d * W, *b = gt_words + g * W;
            for (int64_t w = lane; w < W; w += MTP_WAVE) n += __popcll(a[w] & b[w]);
            n = wave_sum_i64(n);
        }
        if (lane == 0) {
            double v = 0.0;
            if (n > 0) {
                const long long u = gt_crowd[g] ? (long long)det_areas[d] : (long long)det_areas[d] + (long long)gt_areas[g] - n;
                v = __ddiv_rn((double)n, (double)u);
            }
            iou[im.out_start[s] + i] = v;
            if (inter) inter[im.out_start[s] + i] = n;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- matching
struct Pick {
    int sec;      // -1 none, 0 an ignored gt, 1 a non-ignored gt
    double iou;
    int pos;
};
__device__ __forceinline__ bool pick_before(const Pick& a, const Pick& b) {      // b beats a
    if (a.sec != b.sec) return b.sec > a.sec;
    if (a.iou != b.iou) return b.iou > a.iou;
    return b.pos > a.pos;
}

__global__ void __launch_bounds__(kThreads) coco_match_kernel(const double* __restrict__ iou, int64_t iou_numel, const int64_t* __restrict__ det_row,
                                                              const double* __restrict__ det_area, const int64_t* __restrict__ det_cell_start, int64_t D,
                                                              const int64_t* __restrict__ gt_order, const int64_t* __restrict__ gt_col,
                                                              const unsigned char* __restrict__ gt_crowd, const unsigned char* __restrict__ gt_ig,
                                                              const int64_t* __restrict__ gt_cell_start, int64_t G, int64_t cells, int64_t K,
                                                              CocoThr thr, int T, CocoAreas rng, int max_det, unsigned char* __restrict__ matched,
                                                              unsigned char* __restrict__ ignored, int* __restrict__ rank, unsigned long long* npig) {
    constexpr int A = MTP_COCO_AREAS;
    const int lane = threadIdx.x & (MTP_WAVE - 1);
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    // list positions past the last cell (labels outside the categories) belong to no wave: they read as unmatched, not ignored, rank 0
    int64_t tail = det_cell_start[cells];
    tail = tail < 0 ? 0 : (tail > D ? D : tail);
    for (int64_t p = tail + (int64_t)blockIdx.x * kThreads + threadIdx.x; p < D; p += (int64_t)gridDim.x * kThreads) {
        rank[p] = 0;
        for (int at = 0; at < A * T; ++at) matched[(int64_t)at * D + p] = 0, ignored[(int64_t)at * D + p] = 0;
    }
    for (int64_t w = (int64_t)blockIdx.x * kWaves + threadIdx.x / MTP_WAVE; w < cells * A; w += waves) {      // wave-uniform
        const int64_t c = w / A;
        const int a = (int)(w % A);
        int64_t ds = det_cell_start[c], de = det_cell_start[c + 1], gs = gt_cell_start[c], ge = gt_cell_start[c + 1];
        ds = ds < 0 ? 0 : ds, de = de > D ? D : de, gs = gs < 0 ? 0 : gs, ge = ge > G ? G : ge;
        if (de < ds) de = ds;
        if (ge < gs) ge = gs;
        if (ge - gs > MTP_COCO_MAX_CELL_GTS) ge = gs + MTP_COCO_MAX_CELL_GTS;      // refused by the caller; never an overrun of the taken bits
        const int ng = (int)(ge - gs);
        const int64_t nd = de - ds < max_det ? de - ds : (int64_t)max_det;
        const int64_t* order = gt_order + (int64_t)a * G + gs;
        const unsigned char* ig = gt_ig + (int64_t)a * G;
        // the gts that count for recall, and the ranks (once per cell)
        long long live = 0;
        for (int j = lane; j < ng; j += MTP_WAVE) live += ig[order[j]] == 0;
        live = wave_sum_i64(live);
        if (lane == 0 && live) atomicAdd(&npig[(c % K) * A + a], (unsigned long long)live);
        if (a == 0)
            for (int64_t p = ds + lane; p < de; p += MTP_WAVE) rank[p] = (int)(p - ds);
        for (int t = 0; t < T; ++t)      // beyond maxDets[-1]: never matched, never counted
            for (int64_t p = ds + nd + lane; p < de; p += MTP_WAVE) {
                matched[((int64_t)a * T + t) * D + p] = 0;
                ignored[((int64_t)a * T + t) * D + p] = 0;
            }
        // this lane's first gt stays in registers: cells of up to 64 gts read only the IoU inside the loops
        const bool has0 = lane < ng;
        const int64_t g0 = has0 ? order[lane] : 0;
        const bool ig0 = has0 && ig[g0] != 0, crowd0 = has0 && gt_crowd[g0] != 0;
        const int64_t col0 = has0 ? gt_col[g0] : 0;
        for (int t = 0; t < T; ++t) {
            const double th = fmin(thr.v[t], 1.0 - 1e-10);
            unsigned long long taken = 0ull;      // bit b: gt lane + 64 b of the sorted cell is matched at this threshold
            for (int64_t d = 0; d < nd; ++d) {
                const int64_t p = ds + d, row = det_row[p];
                Pick best = {-1, 0.0, -1};
                for (int j = lane, b = 0; j < ng; j += MTP_WAVE, ++b) {
                    const int64_t g = b ? order[j] : g0;
                    const bool crowd = b ? gt_crowd[g] != 0 : crowd0;
                    if (((taken >> b) & 1ull) && !crowd) continue;
                    const int64_t at = row + (b ? gt_col[g] : col0);
                    const double v = at >= 0 && at < iou_numel ? iou[at] : 0.0;
                    if (v < th) continue;
                    const Pick cand = {(b ? ig[g] != 0 : ig0) ? 0 : 1, v, j};
                    if (pick_before(best, cand)) best = cand;
                }
                for (int off = MTP_WAVE / 2; off > 0; off >>= 1) {
                    const Pick o = {__shfl_xor(best.sec, off), __shfl_xor(best.iou, off), __shfl_xor(best.pos, off)};
                    if (pick_before(best, o)) best = o;
                }
                const bool hit = best.sec >= 0;
                if (hit && (best.pos & (MTP_WAVE - 1)) == lane) taken |= 1ull << (best.pos / MTP_WAVE);
                if (lane == 0) {
                    const double ar = det_area[p];
                    matched[((int64_t)a * T + t) * D + p] = hit ? 1 : 0;
                    ignored[((int64_t)a * T + t) * D + p] = hit ? (best.sec == 0 ? 1 : 0) : ((ar < rng.lo[a] || ar > rng.hi[a]) ? 1 : 0);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- accumulate
// max over the threads tid .. 255 (order-free); total = the maximum of all
__device__ __forceinline__ double block_suffix_max_f64(double v, double* wmax, int tid, double& total) {
    const int lane = tid & (MTP_WAVE - 1), w = tid / MTP_WAVE;
    for (int off = 1; off < MTP_WAVE; off <<= 1) {
        const double o = __shfl_down(v, off);
        if (lane + off < MTP_WAVE) v = fmax(v, o);
    }
    __syncthreads();
    if (lane == 0) wmax[w] = v;
    __syncthreads();
    double all = wmax[0];
    for (int i = 1; i < kWaves; ++i) {
        if (i > w) v = fmax(v, wmax[i]);
        all = fmax(all, wmax[i]);
    }
    total = all;
    return v;
}

// what list position i adds: (tp << 32 | fp) and whether it is in the list at this maxDet
__device__ __forceinline__ void acc_item(const unsigned char* mt, const unsigned char* ig, const int* rank, const int64_t* order, int64_t i, int64_t D,
                                         int md, unsigned long long& tpfp, unsigned long long& in) {
    const int64_t p = order[i];
    tpfp = 0ull, in = 0ull;
    if (p < 0 || p >= D || rank[p] >= md) return;
    in = 1ull;
    if (!ig[p]) tpfp = mt[p] ? 1ull << 32 : 1ull;
}

// grid (K, A, M * T)
__global__ void __launch_bounds__(kThreads) coco_accumulate_kernel(const unsigned char* __restrict__ matched, const unsigned char* __restrict__ ignored,
                                                                   const int* __restrict__ rank, const float* __restrict__ score,
                                                                   const int64_t* __restrict__ order, const int64_t* __restrict__ cls_start,
                                                                   const int64_t* __restrict__ npig, int64_t D, int64_t K, int T, CocoMaxDets mds, int M,
                                                                   CocoRec rec, double* __restrict__ precision, double* __restrict__ scores,
                                                                   double* __restrict__ recall) {
    constexpr int A = MTP_COCO_AREAS, R = MTP_COCO_REC_THRS;
    __shared__ unsigned long long wsum[kWaves];
    __shared__ double wmax[kWaves];
    __shared__ double q[R], ss[R];
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x;
    const int a = blockIdx.y, m = blockIdx.z / T, t = blockIdx.z % T, md = mds.v[m];
    const int64_t n = npig[k * A + a];
    const int64_t rec_at = (((int64_t)t * K + k) * A + a) * M + m;
    auto out_at = [&](int r) { return ((((int64_t)t * R + r) * K + k) * A + a) * M + m; };
    if (n <= 0) {      // no gt counts here: precision, scores and recall keep COCOeval's -1
        if (tid < R) precision[out_at(tid)] = -1.0, scores[out_at(tid)] = -1.0;
        if (tid == 0) recall[rec_at] = -1.0;
        return;
    }
    int64_t s = cls_start[k], e = cls_start[k + 1];
    s = s < 0 ? 0 : s, e = e > D ? D : e;
    if (e < s) e = s;
    const unsigned char *mt = matched + ((int64_t)a * T + t) * D, *ig = ignored + ((int64_t)a * T + t) * D;
    const double den = (double)n;
    if (tid < R) q[tid] = 0.0, ss[tid] = 0.0;
    // the totals
    unsigned long long all_tpfp = 0ull, all_in = 0ull, total, x, y;
    for (int64_t c0 = s; c0 < e; c0 += kThreads) {
        const int64_t i = c0 + tid;
        x = y = 0ull;
        if (i < e) acc_item(mt, ig, rank, order, i, D, md, x, y);
        block_scan_add(x, wsum, tid, total);
        all_tpfp += total;
        block_scan_add(y, wsum, tid, total);
        all_in += total;
    }
    // from the right: the counts before a chunk are the counts after it minus its own
    double later = 0.0;      // the largest precision right of the chunk (pr >= 0)
    unsigned long long after_tpfp = all_tpfp, after_in = all_in;
    const int64_t chunks = (e - s + kThreads - 1) / kThreads;
    for (int64_t c = chunks - 1; c >= 0; --c) {
        const int64_t i = s + c * kThreads + tid;
        x = y = 0ull;
        if (i < e) acc_item(mt, ig, rank, order, i, D, md, x, y);
        unsigned long long tot_x, tot_y;
        const unsigned long long inc_x = block_scan_add(x, wsum, tid, tot_x), inc_y = block_scan_add(y, wsum, tid, tot_y);
        const unsigned long long cum_tpfp = after_tpfp - tot_x + inc_x, cum_in = after_in - tot_y + inc_y;
        const double tp = (double)(unsigned)(cum_tpfp >> 32), fp = (double)(unsigned)cum_tpfp;
        const double pr = y ? __ddiv_rn(tp, (fp + tp) + 0x1p-52) : 0.0;
        double chunk_max;
        const double smax = fmax(block_suffix_max_f64(pr, wmax, tid, chunk_max), later);
        const bool is_tp = (x >> 32) != 0ull, first = cum_in == 1ull;
        if (y && (is_tp || first)) {
            const double rc = __ddiv_rn(tp, den), before = __ddiv_rn(tp - (is_tp ? 1.0 : 0.0), den);
            const double sc = (double)score[order[i]];
            for (int r = 0; r < R; ++r)
                if (rec.v[r] <= rc && (first || rec.v[r] > before)) q[r] = smax, ss[r] = sc;
        }
        later = fmax(later, chunk_max);
        after_tpfp -= tot_x, after_in -= tot_y;
    }
    __syncthreads();
    if (tid < R) precision[out_at(tid)] = q[tid], scores[out_at(tid)] = ss[tid];
    if (tid == 0) recall[rec_at] = all_in ? __ddiv_rn((double)(unsigned)(all_tpfp >> 32), den) : 0.0;
}

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_mask_pack(const uint8_t* masks, int64_t N, int64_t HW, uint64_t* words, int64_t* areas, mtp_stream_t stream) {
    MTP_CHECK_ARG(N >= 0 && HW >= 1 && HW < ((int64_t)1 << 40));
    if (N == 0) return 0;
    MTP_CHECK_ARG(masks && words && areas && ((uintptr_t)words & 7) == 0 && ((uintptr_t)areas & 7) == 0);
    const int64_t W = (HW + 63) / 64;
    const unsigned gy = (unsigned)(N < 4096 ? N : 4096);
    const unsigned gx = blocks_for(W, kWaves * 8, (kMaxBlocks + gy - 1) / gy);
    mask_pack_kernel<<<dim3(gx, gy), kThreads, 0, (hipStream_t)stream>>>(masks, N, HW, W, reinterpret_cast<unsigned long long*>(words),
                                                                        reinterpret_cast<unsigned long long*>(areas));
    return mtp_launch_status();
}

extern "C" int mtp_coco_iou(int kind, const float* det_boxes, const uint64_t* det_words, const int64_t* det_areas, const int64_t* det_labels, int64_t D,
                            const float* gt_boxes, const uint64_t* gt_words, const int64_t* gt_areas, const int64_t* gt_labels, const uint8_t* gt_crowd,
                            int64_t G, int64_t W, int agnostic, int64_t n_img, const int64_t* det_start, const int64_t* gt_start, const int64_t* out_start,
                            double* iou, int64_t* inter, int64_t out_numel, mtp_stream_t stream) {
    MTP_CHECK_ARG((kind == MTP_COCO_BBOX || kind == MTP_COCO_SEGM) && D >= 0 && G >= 0 && n_img >= 1 && out_numel >= 0);
    MTP_CHECK_ARG(det_start && gt_start && out_start && det_start[0] == 0 && gt_start[0] == 0 && out_start[0] == 0);
    for (int64_t i = 0; i < n_img; ++i) {      // host tables: every block lies inside the buffers before anything is launched
        const int64_t nd = det_start[i + 1] - det_start[i], ng = gt_start[i + 1] - gt_start[i];
        MTP_CHECK_ARG(nd >= 0 && ng >= 0 && det_start[i + 1] <= D && gt_start[i + 1] <= G && nd < ((int64_t)1 << 31) && ng < ((int64_t)1 << 31));
        MTP_CHECK_ARG(out_start[i + 1] - out_start[i] == nd * ng && out_start[i + 1] <= out_numel);
    }
    if (out_start[n_img] == 0) return 0;
    MTP_CHECK_ARG(iou && det_labels && gt_labels && gt_crowd);
    if (kind == MTP_COCO_BBOX) MTP_CHECK_ARG(det_boxes && gt_boxes);
    else MTP_CHECK_ARG(det_words && gt_words && det_areas && gt_areas && W >= 1 && ((uintptr_t)det_words & 7) == 0 && ((uintptr_t)gt_words & 7) == 0);
    for (int64_t i0 = 0; i0 < n_img; i0 += kIouImgs) {
        const int cnt = (int)(n_img - i0 < kIouImgs ? n_img - i0 : kIouImgs);
        CocoImgs im = {};
        int64_t most = 0;
        for (int s = 0; s <= cnt; ++s) im.det_start[s] = det_start[i0 + s], im.gt_start[s] = gt_start[i0 + s];
        for (int s = 0; s < cnt; ++s) {
            im.out_start[s] = out_start[i0 + s];
            const int64_t pairs = out_start[i0 + s + 1] - out_start[i0 + s];
            most = pairs > most ? pairs : most;
        }
        if (most == 0) continue;
        if (kind == MTP_COCO_BBOX)
            coco_iou_bbox_kernel<<<dim3(blocks_for(most, kThreads, 256), (unsigned)cnt), kThreads, 0, (hipStream_t)stream>>>(
                det_boxes, det_labels, gt_boxes, gt_labels, gt_crowd, agnostic, im, iou);
        else
            coco_iou_segm_kernel<<<dim3(blocks_for(most, kWaves, 1024), (unsigned)cnt), kThreads, 0, (hipStream_t)stream>>>(
                reinterpret_cast<const unsigned long long*>(det_words), det_areas, det_labels, reinterpret_cast<const unsigned long long*>(gt_words),
                gt_areas, gt_labels, gt_crowd, W, agnostic, im, iou, inter);
        const int st = mtp_launch_status();
        if (st) return st;
    }
    return 0;
}

extern "C" int mtp_coco_match(const double* iou, int64_t iou_numel, const int64_t* det_row, const double* det_area, const int64_t* det_cell_start, int64_t D,
                              const int64_t* gt_order, const int64_t* gt_col, const uint8_t* gt_crowd, const uint8_t* gt_ig, const int64_t* gt_cell_start,
                              int64_t G, int64_t cells, int64_t K, const double* iou_thrs, int T, const double* area_rng, int max_det, uint8_t* matched,
                              uint8_t* ignored, int32_t* rank, int64_t* npig, mtp_stream_t stream) {
    MTP_CHECK_ARG(iou_thrs && area_rng && T >= 1 && T <= MTP_COCO_MAX_THRS && K >= 1 && K <= MTP_COCO_MAX_CLASSES && cells >= 0 && cells % K == 0);
    MTP_CHECK_ARG(D >= 0 && D < ((int64_t)1 << 31) && G >= 0 && G < ((int64_t)1 << 31) && cells < ((int64_t)1 << 40) && max_det >= 1 && iou_numel >= 0);
    if (cells == 0) return 0;
    MTP_CHECK_ARG(det_cell_start && gt_cell_start && npig && (D == 0 || (det_row && det_area && matched && ignored && rank)) && (iou_numel == 0 || iou));
    MTP_CHECK_ARG(G == 0 || (gt_order && gt_col && gt_crowd && gt_ig));
    CocoThr thr;
    CocoAreas rng;
    for (int t = 0; t < MTP_COCO_MAX_THRS; ++t) thr.v[t] = t < T ? iou_thrs[t] : 2.0;
    for (int a = 0; a < MTP_COCO_AREAS; ++a) rng.lo[a] = area_rng[2 * a], rng.hi[a] = area_rng[2 * a + 1];
    coco_match_kernel<<<blocks_for(cells * MTP_COCO_AREAS, kWaves, 4 * kMaxBlocks), kThreads, 0, (hipStream_t)stream>>>(
        iou, iou_numel, det_row, det_area, det_cell_start, D, gt_order, gt_col, gt_crowd, gt_ig, gt_cell_start, G, cells, K, thr, T, rng, max_det, matched,
        ignored, rank, reinterpret_cast<unsigned long long*>(npig));
    return mtp_launch_status();
}

extern "C" int mtp_coco_accumulate(const uint8_t* matched, const uint8_t* ignored, const int32_t* rank, const float* score, const int64_t* order,
                                   const int64_t* cls_start, const int64_t* npig, int64_t D, int64_t K, int T, const int32_t* max_dets, int M,
                                   const double* rec_thrs, double* precision, double* scores, double* recall, mtp_stream_t stream) {
    MTP_CHECK_ARG(cls_start && npig && max_dets && rec_thrs && precision && scores && recall && K >= 1 && K <= MTP_COCO_MAX_CLASSES);
    MTP_CHECK_ARG(T >= 1 && T <= MTP_COCO_MAX_THRS && M >= 1 && M <= MTP_COCO_MAX_DET_LEVELS && D >= 0 && D < ((int64_t)1 << 31));
    MTP_CHECK_ARG(D == 0 || (matched && ignored && rank && score && order));
    CocoMaxDets mds = {};
    CocoRec rec;
    for (int m = 0; m < M; ++m) mds.v[m] = max_dets[m];
    for (int r = 0; r < MTP_COCO_REC_THRS; ++r) rec.v[r] = rec_thrs[r];
    coco_accumulate_kernel<<<dim3((unsigned)K, MTP_COCO_AREAS, (unsigned)(M * T)), kThreads, 0, (hipStream_t)stream>>>(
        matched, ignored, rank, score, order, cls_start, npig, D, K, T, mds, M, rec, precision, scores, recall);
    return mtp_launch_status();
}
