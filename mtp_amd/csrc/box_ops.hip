// Box operators of the two detection families (Mask R-CNN: Multi-Task_Pretrain/instance_segmentation, Oriented R-CNN: Multi-Task_Pretrain/
// rotated_detection).  The reference owns none of them: it imports bbox_overlaps / box_iou_rotated / nms / nms_rotated / batched_nms from mmdet and
// mmcv and composes MTP_RD_MaxIoUAssigner in torch on a K x N matrix (rotated_detection/max_iou_assigner.py:231-314); the kernels follow the
// published semantics.  f32 boxes, int64 indices and labels, no float atomics, two calls give the same bits.
//   box_iou        pairwise (M, N) or aligned (M) IoU / IoF; axis-aligned x1,y1,x2,y2 (mmdet bbox_overlaps: no +1, union = max(a1 + a2 - inter, eps))
//                  or rotated cx,cy,w,h,theta (mmcv box_iou_rotated: 0 when an area is below 1e-14)
//   nms_mask       one wave per 64 x 64 tile of (row box, column box) pairs of the score-sorted list, both tiles staged in LDS; lane = column, the
//                  ballot of `iou > thr` (col > row, equal group ids) is the row's 64-bit mask word
//   nms_scan       one wave walks the rows in order, the `removed` words in LDS: a block of 64 rows is resolved on its diagonal word with lane reads,
//                  then the kept rows' words are ORed into the later blocks; blocks that are all removed are skipped as a word
//   assign_phase1  per prior: max / arg-max over the gts (tiled through LDS, any K), the assignment of steps 1-3 and the labels; per gt: the key
//                  (overlap bits << 32 | ~prior index) of the positive overlaps maximised with integer atomics (LDS, then one global atomic per gt
//                  and workgroup); a key left at 0 reads as maximum 0 at prior 0
//   assign_phase2  the low-quality rule: per prior the largest gt i with gt_max[i] >= min_pos_iou whose recomputed overlap has the bits of gt_max[i]
//                  (gt_max_assign_all) or whose key names the prior (the first arg-max prior)
// The rotated intersection clips box A, moved into B's frame (both centres first translated to B's centre: no cancellation at large coordinates),
// against B's four axis-parallel half planes (Sutherland-Hodgman, at most 8 vertices) and takes the shoelace area.  Contraction is off in this file:
// every product and sum rounds once, in the written order, so the overlap recomputed by phase 2 has the bits phase 1 saw, whatever is inlined where
// -- and tests/box_ref.py restates the same operations in numpy.
#include "common.h"
#include "rbox_geom.h"      // RBox, load_rbox, clip_plane, rbox_intersection, box_iou(RBox): shared with det_eval.hip

// honoured under hipcc's default -ffp-contract=fast-honor-pragmas; a build that forces -ffp-contract=fast ignores it and breaks phase two's equality test
#pragma clang fp contract(off)

namespace {

constexpr int kTile = 256;          // gts per LDS tile of the assignment
constexpr int kMaxNms = 32768;      // 512 mask words per row

struct HBox {
    float x1, y1, x2, y2, area;
};

__device__ __forceinline__ HBox make_hbox(float x1, float y1, float x2, float y2) {
    HBox b;
    b.x1 = x1; b.y1 = y1; b.x2 = x2; b.y2 = y2;
    b.area = (x2 - x1) * (y2 - y1);
    return b;
}
__device__ __forceinline__ HBox load_hbox(const float* p) { return make_hbox(p[0], p[1], p[2], p[3]); }
// the circumscribed axis-aligned box of a rotated one (mmrotate's rbox2hbox): half extents |w/2 cos| + |h/2 sin| and |w/2 sin| + |h/2 cos|
__device__ __forceinline__ HBox rbox_to_hbox(const RBox& r) {
    const float ex = fabsf(r.hw * r.c) + fabsf(r.hh * r.s), ey = fabsf(r.hw * r.s) + fabsf(r.hh * r.c);
    return make_hbox(r.cx - ex, r.cy - ey, r.cx + ex, r.cy + ey);
}

__device__ __forceinline__ float box_iou(const HBox& a, const HBox& b, int iof, float eps) {
    const float w = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.0f), h = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.0f);
    const float inter = w * h;
    const float base = iof ? a.area : (a.area + b.area) - inter;
    return inter / fmaxf(base, eps);
}

template <int ROT>
struct Kind;
template <>
struct Kind<0> {
    using Box = HBox;
    static constexpr int kStride = 4;
    __device__ static __forceinline__ HBox load(const float* p) { return load_hbox(p); }
};
template <>
struct Kind<1> {
    using Box = RBox;
    static constexpr int kStride = 5;
    __device__ static __forceinline__ RBox load(const float* p) { return load_rbox(p); }
};

// ------------------------------------------------------------------------------------------------------------------- pairwise / aligned
template <int ROT>
__global__ void __launch_bounds__(kThreads) box_iou_kernel(const float* __restrict__ b1, const float* __restrict__ b2, float* __restrict__ out, int64_t M,
                                                           int64_t N, int iof, int aligned, float eps) {
    using K = Kind<ROT>;
    const int64_t total = aligned ? M : M * N;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t i = aligned ? e : e / N, j = aligned ? e : e - i * N;
        out[e] = box_iou(K::load(b1 + i * K::kStride), K::load(b2 + j * K::kStride), iof, eps);
    }
}

// ------------------------------------------------------------------------------------------------------------------- NMS
// grid (column blocks, row blocks), one wave each; only col block >= row block does anything.  mask[row * nb + cb], written for cb >= row / 64.
template <int ROT>
__global__ void __launch_bounds__(MTP_WAVE) nms_mask_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ groups, int64_t n, float thr,
                                                            unsigned long long* __restrict__ mask, int64_t nb) {
    using K = Kind<ROT>;
    const int64_t cb = blockIdx.x, rb = blockIdx.y;
    if (cb < rb) return;
    __shared__ typename K::Box rows[MTP_WAVE], cols[MTP_WAVE];
    __shared__ int64_t rgrp[MTP_WAVE];
    const int lane = threadIdx.x;
    const int64_t r = rb * MTP_WAVE + lane, c = cb * MTP_WAVE + lane;
    const int64_t rc = r < n ? r : n - 1, cc = c < n ? c : n - 1;       // (clamped: every lane stages a real box)
    rows[lane] = K::load(boxes + rc * K::kStride);
    cols[lane] = K::load(boxes + cc * K::kStride);
    rgrp[lane] = groups ? groups[rc] : 0;
    const int64_t cg = groups ? groups[cc] : 0;
    __syncthreads();
    const typename K::Box mine = cols[lane];
    const int nrows = (int)(n - rb * MTP_WAVE < MTP_WAVE ? n - rb * MTP_WAVE : MTP_WAVE);
    for (int i = 0; i < nrows; ++i) {
        const int64_t row = rb * MTP_WAVE + i;
        const float ov = box_iou(rows[i], mine, 0, 1e-6f);
        const bool hit = c < n && c > row && cg == rgrp[i] && ov > thr;
        const unsigned long long w = __ballot(hit);
        if (lane == 0) mask[row * nb + cb] = w;
    }
}

__device__ __forceinline__ unsigned long long read_lane64(unsigned long long v, int src) {      // src wave-uniform
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, src), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// one wave.  keep[0 .. count) = the kept positions of the sorted list, ascending; stops after max_keep.
__global__ void __launch_bounds__(MTP_WAVE) nms_scan_kernel(const unsigned long long* __restrict__ mask, int64_t n, int64_t nb, int64_t max_keep,
                                                            int64_t* __restrict__ keep, int64_t* __restrict__ count) {
    __shared__ unsigned long long removed[kMaxNms / MTP_WAVE];
    const int lane = threadIdx.x;
    for (int64_t w = lane; w < nb; w += MTP_WAVE) removed[w] = 0ull;
    int64_t kept = 0;
    for (int64_t wi = 0; wi < nb && kept < max_keep; ++wi) {
        __syncthreads();                                       // removed[wi] is complete: the ORs of the earlier blocks
        const int64_t left = n - wi * MTP_WAVE;
        const unsigned long long valid = left >= MTP_WAVE ? ~0ull : ((1ull << left) - 1ull);
        unsigned long long cand = ~removed[wi] & valid;        // wave-uniform
        if (cand == 0ull) continue;                            // 64 dead rows skipped as a word
        const int64_t row = wi * MTP_WAVE + lane;
        const unsigned long long diag = row < n ? mask[row * nb + wi] : 0ull;
        unsigned long long keepbits = 0ull;
        while (cand) {
            const int r = __builtin_amdgcn_readfirstlane(__builtin_ctzll(cand));
            keepbits |= 1ull << r;
            cand &= ~read_lane64(diag, r);
            cand &= ~(1ull << r);
        }
        if ((keepbits >> lane) & 1ull) {
            const int64_t pos = kept + __builtin_popcountll(keepbits & ((1ull << lane) - 1ull));
            if (pos < max_keep) keep[pos] = row;
        }
        kept += __builtin_popcountll(keepbits);
        // the kept rows suppress the later blocks: lane = column block, every lane ORs into its own words only
        unsigned long long todo = keepbits;
        while (todo) {
            const int r = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
            todo &= todo - 1ull;
            const unsigned long long* mrow = mask + (wi * MTP_WAVE + r) * nb;
            for (int64_t cb = wi + 1 + lane; cb < nb; cb += MTP_WAVE) removed[cb] |= mrow[cb];
        }
    }
    if (lane == 0) count[0] = kept < max_keep ? kept : max_keep;
}

// ------------------------------------------------------------------------------------------------------------------- MaxIoU assignment
// CALC 0: boxes / boxes; 1: rotated gts -> circumscribed boxes / boxes; 2: rotated / rotated
template <int CALC>
struct Calc {
    using G = HBox;
    using P = HBox;
    static constexpr int kGtStride = CALC == 0 ? 4 : 5, kPriorStride = 4;
    __device__ static __forceinline__ HBox gt(const float* p) {
        if constexpr (CALC == 0) return load_hbox(p);
        else return rbox_to_hbox(load_rbox(p));
    }
    __device__ static __forceinline__ HBox prior(const float* p) { return load_hbox(p); }
};
template <>
struct Calc<2> {
    using G = RBox;
    using P = RBox;
    static constexpr int kGtStride = 5, kPriorStride = 5;
    __device__ static __forceinline__ RBox gt(const float* p) { return load_rbox(p); }
    __device__ static __forceinline__ RBox prior(const float* p) { return load_rbox(p); }
};

struct AssignThr {
    float pos, neg_lo, neg_hi, min_pos;
};

template <int CALC>
__global__ void __launch_bounds__(kThreads) assign_phase1_kernel(const float* __restrict__ gts, const float* __restrict__ priors,
                                                                 const int64_t* __restrict__ gt_labels, int K, int64_t N, AssignThr thr,
                                                                 int64_t* __restrict__ gt_inds, float* __restrict__ max_overlaps,
                                                                 int64_t* __restrict__ labels, unsigned long long* gt_key) {
    using C = Calc<CALC>;
    __shared__ typename C::G tile[kTile];
    __shared__ unsigned long long tmax[kTile];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * kThreads + tid;
    const bool valid = j < N;
    const typename C::P mine = C::prior(priors + (valid ? j : N - 1) * C::kPriorStride);
    const unsigned long long low = 0xffffffffull - (unsigned long long)j;      // the lower prior index wins among equal overlaps
    float best = -1.0f;
    int arg = 0;
    for (int k0 = 0; k0 < K; k0 += kTile) {
        const int kt = K - k0 < kTile ? K - k0 : kTile;
        __syncthreads();
        if (tid < kt) {
            tile[tid] = C::gt(gts + (int64_t)(k0 + tid) * C::kGtStride);
            tmax[tid] = 0ull;
        }
        __syncthreads();
        if (valid) {
            for (int g = 0; g < kt; ++g) {
                const float ov = box_iou(tile[g], mine, 0, 1e-6f);
                if (ov > best) {               // strict: the lowest gt index among ties
                    best = ov;
                    arg = k0 + g;
                }
                if (ov > 0.0f) {               // a key of 0 stands for "maximum 0, at prior 0": the priors that overlap nothing (most) take no atomic
                    const unsigned long long key = ((unsigned long long)__float_as_uint(ov) << 32) | low;
                    if (key > *(volatile unsigned long long*)&tmax[g]) atomicMax(&tmax[g], key);
                }
            }
        }
        __syncthreads();
        if (tid < kt && tmax[tid] != 0ull) atomicMax(&gt_key[k0 + tid], tmax[tid]);
    }
    if (!valid) return;
    int64_t ind = -1;
    if (best >= thr.neg_lo && best < thr.neg_hi) ind = 0;
    if (best >= thr.pos) ind = arg + 1;
    gt_inds[j] = ind;
    max_overlaps[j] = best;
    labels[j] = ind > 0 ? gt_labels[ind - 1] : -1;
}

template <int CALC>
__global__ void __launch_bounds__(kThreads) assign_phase2_kernel(const float* __restrict__ gts, const float* __restrict__ priors,
                                                                 const int64_t* __restrict__ gt_labels, int K, int64_t N, float min_pos, int assign_all,
                                                                 const unsigned long long* __restrict__ gt_key, int64_t* __restrict__ gt_inds,
                                                                 int64_t* __restrict__ labels) {
    using C = Calc<CALC>;
    __shared__ typename C::G tile[kTile];
    __shared__ unsigned long long tkey[kTile];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * kThreads + tid;
    const bool valid = j < N;
    const typename C::P mine = C::prior(priors + (valid ? j : N - 1) * C::kPriorStride);
    int cand = -1;
    for (int k0 = 0; k0 < K; k0 += kTile) {
        const int kt = K - k0 < kTile ? K - k0 : kTile;
        __syncthreads();
        if (tid < kt) {
            tile[tid] = C::gt(gts + (int64_t)(k0 + tid) * C::kGtStride);
            tkey[tid] = gt_key[k0 + tid];
        }
        __syncthreads();
        if (valid) {
            for (int g = 0; g < kt; ++g) {
                const unsigned long long key = tkey[g];
                const unsigned bits = (unsigned)(key >> 32);
                if (!(__uint_as_float(bits) >= min_pos)) continue;
                if (assign_all) {
                    if (box_iou(tile[g], mine, 0, 1e-6f) == __uint_as_float(bits)) cand = k0 + g;      // (the same bits, or both zero)
                } else if ((bits ? 0xffffffffull - (key & 0xffffffffull) : 0ull) == (unsigned long long)j) {
                    cand = k0 + g;
                }
            }
        }
    }
    if (valid && cand >= 0) {
        gt_inds[j] = cand + 1;
        labels[j] = gt_labels[cand];
    }
}

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_box_iou(const float* boxes1, const float* boxes2, float* out, int64_t M, int64_t N, int kind, int iof, int aligned, float eps,
                           mtp_stream_t stream) {
    MTP_CHECK_ARG(boxes1 && boxes2 && out && M > 0 && N > 0 && (kind == MTP_BOX_ALIGNED || kind == MTP_BOX_ROTATED));
    MTP_CHECK_ARG((!aligned || M == N) && M < ((int64_t)1 << 40) / N && eps >= 0.0f);
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = blocks_for(aligned ? M : M * N, kThreads, kMaxBlocks);
    if (kind == MTP_BOX_ALIGNED) box_iou_kernel<0><<<g, kThreads, 0, s>>>(boxes1, boxes2, out, M, N, iof != 0, aligned != 0, eps);
    else box_iou_kernel<1><<<g, kThreads, 0, s>>>(boxes1, boxes2, out, M, N, iof != 0, aligned != 0, eps);
    return mtp_launch_status();
}

extern "C" int mtp_nms_mask(const float* boxes, const int64_t* groups, int64_t n, int kind, float iou_threshold, void* mask, int64_t mask_bytes,
                            mtp_stream_t stream) {
    MTP_CHECK_ARG(boxes && mask && n > 0 && n <= kMaxNms && (kind == MTP_BOX_ALIGNED || kind == MTP_BOX_ROTATED));
    const int64_t nb = (n + MTP_WAVE - 1) / MTP_WAVE;
    MTP_CHECK_ARG(mask_bytes >= n * nb * 8 && ((uintptr_t)mask & 7) == 0);
    const dim3 grid((unsigned)nb, (unsigned)nb);
    unsigned long long* m = static_cast<unsigned long long*>(mask);
    if (kind == MTP_BOX_ALIGNED) nms_mask_kernel<0><<<grid, MTP_WAVE, 0, (hipStream_t)stream>>>(boxes, groups, n, iou_threshold, m, nb);
    else nms_mask_kernel<1><<<grid, MTP_WAVE, 0, (hipStream_t)stream>>>(boxes, groups, n, iou_threshold, m, nb);
    return mtp_launch_status();
}

extern "C" int mtp_nms_scan(const void* mask, int64_t n, int64_t max_keep, int64_t* keep, int64_t* count, mtp_stream_t stream) {
    MTP_CHECK_ARG(mask && keep && count && n > 0 && n <= kMaxNms && max_keep > 0 && ((uintptr_t)mask & 7) == 0);
    nms_scan_kernel<<<1, MTP_WAVE, 0, (hipStream_t)stream>>>(static_cast<const unsigned long long*>(mask), n, (n + MTP_WAVE - 1) / MTP_WAVE, max_keep, keep,
                                                            count);
    return mtp_launch_status();
}

template <int CALC>
static int assign_launch(const float* gts, const float* priors, const int64_t* gt_labels, int K, int64_t N, AssignThr thr, int low_quality, int assign_all,
                         int64_t* gt_inds, float* max_overlaps, int64_t* labels, unsigned long long* key, hipStream_t s) {
    const unsigned g = blocks_exact(N);
    const hipError_t e = hipMemsetAsync(key, 0, (size_t)K * 8, s);
    if (e != hipSuccess) return (int)e;
    assign_phase1_kernel<CALC><<<g, kThreads, 0, s>>>(gts, priors, gt_labels, K, N, thr, gt_inds, max_overlaps, labels, key);
    if (low_quality) assign_phase2_kernel<CALC><<<g, kThreads, 0, s>>>(gts, priors, gt_labels, K, N, thr.min_pos, assign_all, key, gt_inds, labels);
    return mtp_launch_status();
}

extern "C" int mtp_max_iou_assign(const float* gts, const float* priors, const int64_t* gt_labels, int64_t K, int64_t N, int calculator, float pos_iou_thr,
                                  float neg_iou_lo, float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all, int64_t* gt_inds,
                                  float* max_overlaps, int64_t* labels, void* workspace, int64_t workspace_bytes, mtp_stream_t stream) {
    MTP_CHECK_ARG(gts && priors && gt_labels && gt_inds && max_overlaps && labels && workspace && K > 0 && N > 0);
    MTP_CHECK_ARG(K < ((int64_t)1 << 24) && N < ((int64_t)1 << 31) && workspace_bytes >= K * 8 && ((uintptr_t)workspace & 7) == 0);
    MTP_CHECK_ARG(calculator >= MTP_ASSIGN_BOX && calculator <= MTP_ASSIGN_ROTATED);
    const AssignThr thr = {pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou};
    unsigned long long* key = static_cast<unsigned long long*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const int lq = match_low_quality != 0, all = gt_max_assign_all != 0;
    if (calculator == MTP_ASSIGN_BOX) return assign_launch<0>(gts, priors, gt_labels, (int)K, N, thr, lq, all, gt_inds, max_overlaps, labels, key, s);
    if (calculator == MTP_ASSIGN_RBOX2HBOX) return assign_launch<1>(gts, priors, gt_labels, (int)K, N, thr, lq, all, gt_inds, max_overlaps, labels, key, s);
    return assign_launch<2>(gts, priors, gt_labels, (int)K, N, thr, lq, all, gt_inds, max_overlaps, labels, key, s);
}
