// The box half of Mask R-CNN (Multi-Task_Pretrain/instance_segmentation: rpn_head.py, bbox_head.py, base_bbox_head.py, roi_head.py; configured at
// mask_rcnn.py:19-55, 70-119).  DeltaXYWHBBoxCoder is restated from the published mmdet 3.x algorithm (bbox2delta / delta2bbox).
// f32 everywhere, int64 indices, no float atomics, two calls give the same bits.
//   hbox_encode / hbox_decode   one thread per box, one 16-byte access per array; the decode clips to the (h, w) of the row's image when a table is given
//   hrpn_loss        one thread per slot of the per-image sample lists (positives first, then negatives), as rpn_loss has it: sigmoid BCE on the
//                    logit, on positives L1 of the four deltas against the encode of (prior, gt); gradients by plain stores into zeroed maps; the
//                    per-level sums of a workgroup go to a partial row
//   hrpn_loss_sum    one wave adds the partial rows in order and scales by loss_weight / avg_factor, read on the device
//   hrpn_proposals   one thread per kept (image, level, rank): sigmoid score, the decoded box clipped to the image, level id, the size flag
//   hroi_loss        one WAVE per slot of the fixed-size sample lists: the K + 1 logits in trips of 64 (maximum, first arg-max, sum of exponentials by
//                    butterflies), softmax cross-entropy; lane k owns class k's four deltas (one 16-byte load, one 16-byte store), so the dense
//                    (rows, 4 K) gradient is written whole: the label's four columns on a positive, zeros everywhere else
//   hroi_loss_sum    one wave: lane i adds the partial rows i, i + 64, .. in order, then a butterfly; divides by the counts read on the device
//   hroi_predict     one wave per RoI: softmax scores without the background column, lane k decodes and clips class k's box
// L1 has the gradient sign(pred - target), 0 at equality.  Contraction is off: tests/hbox_ref.py restates the same operations.
#include "common.h"
#include "rpn_levels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWaves = kThreads / MTP_WAVE;

struct Codec {
    float mean[4], stdv[4], max_ratio;
};

__device__ __forceinline__ float4 hbox_encode(float4 p, float4 g, const Codec& k) {
    const float px = (p.x + p.z) * 0.5f, py = (p.y + p.w) * 0.5f, pw = p.z - p.x, ph = p.w - p.y;
    const float gx = (g.x + g.z) * 0.5f, gy = (g.y + g.w) * 0.5f, gw = g.z - g.x, gh = g.w - g.y;
    const float dx = (gx - px) / pw, dy = (gy - py) / ph, dw = logf(gw / pw), dh = logf(gh / ph);
    return make_float4((dx - k.mean[0]) / k.stdv[0], (dy - k.mean[1]) / k.stdv[1], (dw - k.mean[2]) / k.stdv[2], (dh - k.mean[3]) / k.stdv[3]);
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// clip: the box is clamped to x in [0, img_w], y in [0, img_h]
__device__ __forceinline__ float4 hbox_decode(float4 p, float4 raw, const Codec& k, bool clip, float img_h, float img_w) {
    const float dx = raw.x * k.stdv[0] + k.mean[0], dy = raw.y * k.stdv[1] + k.mean[1];
    const float dw = clampf(raw.z * k.stdv[2] + k.mean[2], -k.max_ratio, k.max_ratio), dh = clampf(raw.w * k.stdv[3] + k.mean[3], -k.max_ratio, k.max_ratio);
    const float px = (p.x + p.z) * 0.5f, py = (p.y + p.w) * 0.5f, pw = p.z - p.x, ph = p.w - p.y;
    const float gx = px + pw * dx, gy = py + ph * dy, gw = pw * expf(dw), gh = ph * expf(dh);
    float4 o = make_float4(gx - gw * 0.5f, gy - gh * 0.5f, gx + gw * 0.5f, gy + gh * 0.5f);
    if (clip) {
        o.x = clampf(o.x, 0.0f, img_w); o.z = clampf(o.z, 0.0f, img_w);
        o.y = clampf(o.y, 0.0f, img_h); o.w = clampf(o.w, 0.0f, img_h);
    }
    return o;
}

__device__ __forceinline__ float l1_sign(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// ------------------------------------------------------------------------------------------------------------------- the coder on plain arrays
__global__ void __launch_bounds__(kThreads) hbox_encode_kernel(const float* __restrict__ priors, const float* __restrict__ gts, Codec k, int64_t n,
                                                               float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    store4(out + e * 4, hbox_encode(load4(priors + e * 4), load4(gts + e * 4), k));
}

// max_shapes (images, 2) = (h, w) or NULL: no clip; image_ids (n) or NULL: every row belongs to image 0.  A row that names no image is not clipped.
__global__ void __launch_bounds__(kThreads) hbox_decode_kernel(const float* __restrict__ priors, const float* __restrict__ deltas, Codec k, int64_t n,
                                                               const float* __restrict__ max_shapes, const int64_t* __restrict__ image_ids,
                                                               int64_t images, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t b = image_ids ? image_ids[e] : 0;
    const bool clip = max_shapes && b >= 0 && b < images;
    const float h = clip ? max_shapes[b * 2] : 0.0f, w = clip ? max_shapes[b * 2 + 1] : 0.0f;
    store4(out + e * 4, hbox_decode(load4(priors + e * 4), load4(deltas + e * 4), k, clip, h, w));
}

// ------------------------------------------------------------------------------------------------------------------- the sample lists
struct Slots {
    const int64_t* n_pos;
    const int64_t* n_neg;
    int64_t B, S;
};

__device__ __forceinline__ void slot_counts(const Slots& a, int64_t b, int64_t& np, int64_t& nn) {
    np = a.n_pos[b]; nn = a.n_neg[b];
    np = np < 0 ? 0 : (np > a.S ? a.S : np);
    nn = nn < 0 ? 0 : (nn > a.S - np ? a.S - np : nn);
}
__device__ __forceinline__ int64_t slot_total(const Slots& a) {
    int64_t t = 0;
    for (int64_t i = 0; i < a.B; ++i) {
        int64_t p, n;
        slot_counts(a, i, p, n);
        t += p + n;
    }
    return t;
}

// ------------------------------------------------------------------------------------------------------------------- RPN: targets and loss
struct RpnArgs {
    const float* priors;
    const float* gts;            // (K, 4)
    const int64_t* samples;
    const int64_t* sample_gt;
    int64_t total, K;
};

// grid (chunks of the sample list, images); partial[(image * chunks + chunk) * 2 kL + level] = sum of the cls terms, + kL: of the bbox terms
__global__ void __launch_bounds__(kThreads) hrpn_loss_kernel(Levels L, RpnArgs a, Slots sl, Codec k, int A, float w_cls, float w_box,
                                                             float* __restrict__ partial) {
    __shared__ float wsum[kWaves][2 * kL];
    __shared__ int64_t s_avg;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y, j = (int64_t)blockIdx.x * kThreads + tid;
    int64_t np, nn;
    slot_counts(sl, b, np, nn);
    if (tid == 0) s_avg = slot_total(sl);
    __syncthreads();
    const int64_t avg = s_avg;
    const float g_cls = avg > 0 ? w_cls / (float)avg : 0.0f, g_box = avg > 0 ? w_box / (float)avg : 0.0f;
    int64_t idx = j < np + nn ? a.samples[b * sl.S + j] : -1;
    const bool active = idx >= 0 && idx < a.total;
    if (!active) idx = 0;
    const int l = level_of(L, idx);
    const Level& v = L.lv[l];
    const int64_t local = idx - v.first, an = local % A, cell = local / A, x = cell % v.W, y = cell / v.W;
    float lc = 0.0f, lb = 0.0f;
    if (active && y < v.H) {
        const bool pos = j < np;
        const int64_t co = b * v.cs[0] + an * v.cs[1] + y * v.cs[2] + x * v.cs[3];
        const float z = v.cls[co], t = pos ? 1.0f : 0.0f;
        lc = (fmaxf(z, 0.0f) - z * t) + log1pf(expf(-fabsf(z)));
        if (v.dcls) v.dcls[co] = (1.0f / (1.0f + expf(-z)) - t) * g_cls;
        const int64_t g = pos ? a.sample_gt[b * sl.S + j] : -1;
        if (g >= 0 && g < a.K) {
            const float4 t4 = hbox_encode(load4(a.priors + idx * 4), load4(a.gts + g * 4), k);
            const float tgt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t ro = b * v.rs[0] + (an * 4 + c) * v.rs[1] + y * v.rs[2] + x * v.rs[3];
                const float d = v.reg[ro] - tgt[c];
                lb += fabsf(d);
                if (v.dreg) v.dreg[ro] = l1_sign(d) * g_box;
            }
        }
    }
    const int wave = tid / MTP_WAVE, lane = tid % MTP_WAVE;
#pragma unroll
    for (int i = 0; i < kL; ++i) {
        const float sc = wave_sum(active && l == i ? lc : 0.0f), sb = wave_sum(active && l == i ? lb : 0.0f);
        if (lane == 0) {
            wsum[wave][i] = sc;
            wsum[wave][kL + i] = sb;
        }
    }
    __syncthreads();
    if (tid < 2 * kL) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += wsum[w][tid];
        partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (2 * kL) + tid] = s;
    }
}

__global__ void __launch_bounds__(MTP_WAVE) hrpn_loss_sum_kernel(const float* __restrict__ partial, int64_t blocks, Slots sl, int levels, float w_cls,
                                                                 float w_box, float* __restrict__ loss_cls, float* __restrict__ loss_box) {
    const int tid = threadIdx.x;
    if (tid >= 2 * kL) return;
    const int l = tid % kL;
    if (l >= levels) return;
    float s = 0.0f;
    for (int64_t i = 0; i < blocks; ++i) s += partial[i * (2 * kL) + tid];
    const int64_t avg = slot_total(sl);
    s = avg > 0 ? s / (float)avg : 0.0f;
    if (tid < kL) loss_cls[l] = s * w_cls;
    else loss_box[l] = s * w_box;
}

// ------------------------------------------------------------------------------------------------------------------- RPN: proposals
__global__ void __launch_bounds__(kThreads) hrpn_proposals_kernel(Levels L, const float* __restrict__ priors, const int64_t* __restrict__ keep, int64_t B,
                                                                  int64_t T, Codec k, int A, const float* __restrict__ img_shapes, float min_size,
                                                                  float* __restrict__ scores, float* __restrict__ boxes, int64_t* __restrict__ level_ids,
                                                                  uint8_t* __restrict__ valid) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= B * T) return;
    const int64_t b = e / T, t = e - b * T;
    int l = 0;
#pragma unroll
    for (int i = 1; i < kL; ++i)
        if (i < L.n && t >= L.lv[i].keep_first) l = i;
    const Level& v = L.lv[l];
    const int64_t idx = keep[e];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float score = 0.0f;
    bool ok = false;
    if (idx >= 0 && idx < v.count) {
        const int64_t an = idx % A, cell = idx / A, x = cell % v.W, y = cell / v.W;
        score = 1.0f / (1.0f + expf(-v.cls[b * v.cs[0] + an * v.cs[1] + y * v.cs[2] + x * v.cs[3]]));
        float d[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) d[c] = v.reg[b * v.rs[0] + (an * 4 + c) * v.rs[1] + y * v.rs[2] + x * v.rs[3]];
        o = hbox_decode(load4(priors + (v.first + idx) * 4), make_float4(d[0], d[1], d[2], d[3]), k, true, img_shapes[b * 2], img_shapes[b * 2 + 1]);
        ok = o.z - o.x > min_size && o.w - o.y > min_size;
    }
    scores[e] = score;
    store4(boxes + e * 4, o);
    level_ids[e] = l;
    valid[e] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------- RoI head: targets and loss
struct RoiArgs {
    const float* cls;
    const float* reg;
    float* dcls;
    float* dreg;
    int64_t ldc, ldr, K;      // K classes, K + 1 logits and 4 K deltas per row
    const float* rois;        // (images S, 4)
    const float* gts;         // (G, 4)
    const int64_t* gt_labels; // (G)
    const int64_t* sample_gt; // (images, S)
    int64_t G;
    int encoded;              // the regression target: 0 = 1.0 (the reference as written), 1 = encode(roi, gt)
};

// the K + 1 logits of one row by one wave: maximum, the first index that reaches it, the sum of exp(z - maximum).  Every lane of the wave is here.
__device__ __forceinline__ void row_softmax_stats(const float* z, int64_t n, int lane, float& m, int64_t& arg, float& sum) {
    float lm = -INFINITY;
    for (int64_t c = lane; c < n; c += MTP_WAVE) lm = fmaxf(lm, z[c]);
    m = wave_max(lm);
    float first = -INFINITY;      // -(index) of the lane's first column that holds the maximum; indices stay below 2^16: exact
    for (int64_t c = lane; c < n; c += MTP_WAVE)
        if (z[c] == m && first == -INFINITY) first = -(float)c;
    arg = (int64_t)(-wave_max(first));
    float ls = 0.0f;
    for (int64_t c = lane; c < n; c += MTP_WAVE) ls += expf(z[c] - m);
    sum = wave_sum(ls);
}

// one wave per row, kWaves rows per workgroup; partial[workgroup * 3 + (cls, bbox, hits)]
__global__ void __launch_bounds__(kThreads) hroi_loss_kernel(RoiArgs a, Slots sl, Codec k, float w_cls, float w_box, float* __restrict__ partial) {
    __shared__ float wsum[kWaves][3];
    __shared__ int64_t s_total;
    const int tid = threadIdx.x, wave = tid / MTP_WAVE, lane = tid % MTP_WAVE;
    if (tid == 0) s_total = slot_total(sl);
    __syncthreads();
    const int64_t total = s_total;
    const float g_cls = w_cls / (float)(total > 1 ? total : 1), g_box = total > 0 ? w_box / (float)total : 0.0f;
    const int64_t row = (int64_t)blockIdx.x * kWaves + wave;      // the same for the whole wave
    float lc = 0.0f, lb = 0.0f, hit = 0.0f;
    if (row < sl.B * sl.S) {
        const int64_t b = row / sl.S, j = row - b * sl.S;
        int64_t np, nn;
        slot_counts(sl, b, np, nn);
        bool used = j < np + nn;
        const bool pos = j < np;
        int64_t g = -1, label = a.K;
        if (pos) {      // a positive that names no gt or no class is padding
            g = a.sample_gt[row];
            label = g >= 0 && g < a.G ? a.gt_labels[g] : -1;
            if (label < 0 || label >= a.K) used = false;
        }
        const float* z = a.cls + row * a.ldc;
        float* dz = a.dcls ? a.dcls + row * a.ldc : nullptr;
        if (used) {
            float m, sum;
            int64_t arg;
            row_softmax_stats(z, a.K + 1, lane, m, arg, sum);
            lc = lane == 0 ? (logf(sum) + m) - z[label] : 0.0f;
            hit = lane == 0 && arg == label ? 1.0f : 0.0f;
            if (dz)
                for (int64_t c = lane; c <= a.K; c += MTP_WAVE) dz[c] = (expf(z[c] - m) / sum - (c == label ? 1.0f : 0.0f)) * g_cls;
        } else if (dz) {
            for (int64_t c = lane; c <= a.K; c += MTP_WAVE) dz[c] = 0.0f;
        }
        const bool fit = used && pos;
        float4 tgt = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        if (fit && a.encoded) tgt = hbox_encode(load4(a.rois + row * 4), load4(a.gts + g * 4), k);
        for (int64_t c = lane; c < a.K; c += MTP_WAVE) {      // class c: columns 4 c .. 4 c + 3
            float4 dv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (fit && c == label) {
                const float4 p = load4(a.reg + row * a.ldr + c * 4);
                const float dx = p.x - tgt.x, dy = p.y - tgt.y, dw = p.z - tgt.z, dh = p.w - tgt.w;
                lb = ((fabsf(dx) + fabsf(dy)) + fabsf(dw)) + fabsf(dh);
                dv = make_float4(l1_sign(dx) * g_box, l1_sign(dy) * g_box, l1_sign(dw) * g_box, l1_sign(dh) * g_box);
            }
            if (a.dreg) store4(a.dreg + row * a.ldr + c * 4, dv);
        }
    }
    // one lane of the wave holds each term: the butterflies move it to lane 0 and add zeros
    const float sc = wave_sum(lc), sb = wave_sum(lb), sh = wave_sum(hit);
    if (lane == 0) {
        wsum[wave][0] = sc; wsum[wave][1] = sb; wsum[wave][2] = sh;
    }
    __syncthreads();
    if (tid < 3) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += wsum[w][tid];
        partial[(int64_t)blockIdx.x * 3 + tid] = s;
    }
}

// out[0] = loss_cls, out[1] = loss_bbox, out[2] = acc (percent)
__global__ void __launch_bounds__(MTP_WAVE) hroi_loss_sum_kernel(const float* __restrict__ partial, int64_t blocks, Slots sl, float w_cls, float w_box,
                                                                 float* __restrict__ out) {
    const int lane = threadIdx.x;
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int64_t i = lane; i < blocks; i += MTP_WAVE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += partial[i * 3 + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = wave_sum(s[c]);
    if (lane != 0) return;
    const int64_t total = slot_total(sl);
    out[0] = s[0] / (float)(total > 1 ? total : 1) * w_cls;
    out[1] = total > 0 ? s[1] / (float)total * w_box : 0.0f;
    out[2] = total > 0 ? s[2] * 100.0f / (float)total : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------------- RoI head: predict
// rois (R, 5): image, x1, y1, x2, y2.  img_shapes (images, 2) = (h, w); inv_scale (images, 2) = (1 / sx, 1 / sy) or NULL.  A RoI that names no
// image: zero boxes and no flags.
__global__ void __launch_bounds__(kThreads) hroi_predict_kernel(const float* __restrict__ cls, int64_t ldc, const float* __restrict__ reg, int64_t ldr, int64_t K,
                                                                const float* __restrict__ rois, int64_t R, Codec k, const float* __restrict__ img_shapes,
                                                                const float* __restrict__ inv_scale, int64_t images, float score_thr,
                                                                float* __restrict__ scores, float* __restrict__ boxes, uint8_t* __restrict__ flags) {
    const int lane = threadIdx.x % MTP_WAVE;
    const int64_t r = (int64_t)blockIdx.x * kWaves + threadIdx.x / MTP_WAVE;      // the same for the whole wave
    if (r >= R) return;
    const float* z = cls + r * ldc;
    float m, sum;
    int64_t arg;
    row_softmax_stats(z, K + 1, lane, m, arg, sum);
    const float bi = rois[r * 5];
    const int64_t b = bi >= 0.0f && bi < (float)images ? (int64_t)bi : -1;
    const float4 roi = make_float4(rois[r * 5 + 1], rois[r * 5 + 2], rois[r * 5 + 3], rois[r * 5 + 4]);
    const float h = b >= 0 ? img_shapes[b * 2] : 0.0f, w = b >= 0 ? img_shapes[b * 2 + 1] : 0.0f;
    const float fx = b >= 0 && inv_scale ? inv_scale[b * 2] : 1.0f, fy = b >= 0 && inv_scale ? inv_scale[b * 2 + 1] : 1.0f;
    for (int64_t c = lane; c < K; c += MTP_WAVE) {
        const float s = expf(z[c] - m) / sum;
        scores[r * K + c] = s;
        flags[r * K + c] = b >= 0 && s > score_thr ? 1 : 0;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (b >= 0) {
            o = hbox_decode(roi, load4(reg + r * ldr + c * 4), k, true, h, w);
            o = make_float4(o.x * fx, o.y * fy, o.z * fx, o.w * fy);
        }
        store4(boxes + (r * K + c) * 4, o);
    }
}

bool make_codec(const float* means, const float* stds, float wh_ratio_clip, Codec& k) {
    if (!means || !stds || !(wh_ratio_clip > 0.0f)) return false;
    for (int i = 0; i < 4; ++i) {
        k.mean[i] = means[i];
        k.stdv[i] = stds[i];
        if (!(stds[i] > 0.0f)) return false;
    }
    k.max_ratio = fabsf(logf(wh_ratio_clip));
    return true;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_hbox_delta_encode(const float* priors, const float* gts, const float* means, const float* stds, int64_t n, float* deltas,
                                     mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && gts && deltas && n > 0 && n < ((int64_t)1 << 31) && aligned16(priors) && aligned16(gts) && aligned16(deltas));
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, 0.016f, k));
    hbox_encode_kernel<<<blocks_exact(n), kThreads, 0, (hipStream_t)stream>>>(priors, gts, k, n, deltas);
    return mtp_launch_status();
}

extern "C" int mtp_hbox_delta_decode(const float* priors, const float* deltas, const float* means, const float* stds, float wh_ratio_clip, int64_t n,
                                     const float* max_shapes, const int64_t* image_ids, int64_t images, float* boxes, mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && deltas && boxes && n > 0 && n < ((int64_t)1 << 31) && aligned16(priors) && aligned16(deltas) && aligned16(boxes));
    MTP_CHECK_ARG(max_shapes ? images >= 1 : (!image_ids && images == 0));
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, wh_ratio_clip, k));
    hbox_decode_kernel<<<blocks_exact(n), kThreads, 0, (hipStream_t)stream>>>(priors, deltas, k, n, max_shapes, image_ids, images, boxes);
    return mtp_launch_status();
}

extern "C" int64_t mtp_hrpn_loss_workspace_bytes(int64_t images, int64_t samples) {
    if (images < 1 || samples < 1) return MTP_ERR_ARG;
    return images * ((samples + kThreads - 1) / kThreads) * 2 * kL * (int64_t)sizeof(float);
}

extern "C" int mtp_hrpn_loss(const mtp_rpn_level* levels, int num_levels, int64_t A, const float* priors, int64_t num_priors, const float* gts, int64_t K,
                             const int64_t* samples, const int64_t* sample_gt, const int64_t* n_pos, const int64_t* n_neg, int64_t images, int64_t S,
                             const float* means, const float* stds, float cls_weight, float bbox_weight, float* loss_cls, float* loss_bbox,
                             void* workspace, int64_t workspace_bytes, mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && samples && sample_gt && n_pos && n_neg && loss_cls && loss_bbox && workspace && images > 0 && images <= 65535 && S > 0);
    MTP_CHECK_ARG(K >= 0 && (gts || K == 0) && num_priors < ((int64_t)1 << 31) && S < ((int64_t)1 << 31) && aligned16(priors) && aligned16(gts));
    MTP_CHECK_ARG(workspace_bytes >= mtp_hrpn_loss_workspace_bytes(images, S) && ((uintptr_t)workspace & 3) == 0);
    Levels L;
    Codec k;
    int64_t T;
    MTP_CHECK_ARG(make_codec(means, stds, 0.016f, k) && make_levels(levels, num_levels, A, num_priors, false, L, T));
    const RpnArgs a = {priors, gts, samples, sample_gt, num_priors, K};
    const Slots sl = {n_pos, n_neg, images, S};
    const dim3 grid((unsigned)((S + kThreads - 1) / kThreads), (unsigned)images);
    hipStream_t s = (hipStream_t)stream;
    float* partial = static_cast<float*>(workspace);
    hrpn_loss_kernel<<<grid, kThreads, 0, s>>>(L, a, sl, k, (int)A, cls_weight, bbox_weight, partial);
    hrpn_loss_sum_kernel<<<1, MTP_WAVE, 0, s>>>(partial, (int64_t)grid.x * grid.y, sl, num_levels, cls_weight, bbox_weight, loss_cls, loss_bbox);
    return mtp_launch_status();
}

extern "C" int mtp_hrpn_proposals(const mtp_rpn_level* levels, int num_levels, int64_t A, const float* priors, int64_t num_priors, const int64_t* keep,
                                  int64_t images, const float* means, const float* stds, float wh_ratio_clip, const float* img_shapes,
                                  float min_bbox_size, float* scores, float* boxes, int64_t* level_ids, uint8_t* valid, mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && keep && img_shapes && scores && boxes && level_ids && valid && images > 0 && num_priors < ((int64_t)1 << 31));
    MTP_CHECK_ARG(aligned16(priors) && aligned16(boxes));
    Levels L;
    Codec k;
    int64_t T;
    MTP_CHECK_ARG(make_codec(means, stds, wh_ratio_clip, k) && make_levels(levels, num_levels, A, num_priors, true, L, T));
    MTP_CHECK_ARG(T > 0 && images < ((int64_t)1 << 31) / T);
    hrpn_proposals_kernel<<<blocks_exact(images * T), kThreads, 0, (hipStream_t)stream>>>(L, priors, keep, images, T, k, (int)A, img_shapes, min_bbox_size,
                                                                                          scores, boxes, level_ids, valid);
    return mtp_launch_status();
}

extern "C" int64_t mtp_hroi_loss_workspace_bytes(int64_t images, int64_t samples) {
    if (images < 1 || samples < 1 || samples >= ((int64_t)1 << 31) / images) return MTP_ERR_ARG;
    return ((images * samples + kWaves - 1) / kWaves) * 3 * (int64_t)sizeof(float);
}

extern "C" int mtp_hroi_loss(const float* cls_score, int64_t ld_cls, const float* bbox_pred, int64_t ld_reg, int64_t num_classes, const float* rois,
                             const float* gts, const int64_t* gt_labels, int64_t num_gts, const int64_t* sample_gt, const int64_t* n_pos,
                             const int64_t* n_neg, int64_t images, int64_t S, const float* means, const float* stds, int target_mode, float cls_weight,
                             float bbox_weight, float* losses, float* dcls, float* dreg, void* workspace, int64_t workspace_bytes, mtp_stream_t stream) {
    MTP_CHECK_ARG(cls_score && bbox_pred && rois && sample_gt && n_pos && n_neg && losses && workspace && images > 0 && S > 0);
    MTP_CHECK_ARG(S < ((int64_t)1 << 31) / images && num_classes >= 1 && num_classes < (1 << 16) && ld_cls > num_classes && ld_reg >= 4 * num_classes);
    MTP_CHECK_ARG(ld_reg % 4 == 0 && aligned16(bbox_pred) && aligned16(dreg) && aligned16(rois) && aligned16(gts));
    MTP_CHECK_ARG(num_gts >= 0 && ((gts && gt_labels) || num_gts == 0) && (dcls != nullptr) == (dreg != nullptr));
    MTP_CHECK_ARG(target_mode == MTP_HROI_TARGET_ONES || target_mode == MTP_HROI_TARGET_ENCODED);
    MTP_CHECK_ARG(workspace_bytes >= mtp_hroi_loss_workspace_bytes(images, S) && ((uintptr_t)workspace & 3) == 0);
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, 0.016f, k));
    const RoiArgs a = {cls_score, bbox_pred, dcls, dreg, ld_cls, ld_reg, num_classes, rois, gts, gt_labels, sample_gt, num_gts,
                       target_mode == MTP_HROI_TARGET_ENCODED ? 1 : 0};
    const Slots sl = {n_pos, n_neg, images, S};
    const int64_t blocks = (images * S + kWaves - 1) / kWaves;
    hipStream_t s = (hipStream_t)stream;
    float* partial = static_cast<float*>(workspace);
    hroi_loss_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(a, sl, k, cls_weight, bbox_weight, partial);
    hroi_loss_sum_kernel<<<1, MTP_WAVE, 0, s>>>(partial, blocks, sl, cls_weight, bbox_weight, losses);
    return mtp_launch_status();
}

extern "C" int mtp_hroi_predict(const float* cls_score, int64_t ld_cls, const float* bbox_pred, int64_t ld_reg, int64_t num_classes, const float* rois,
                                int64_t R, const float* means, const float* stds, float wh_ratio_clip, const float* img_shapes, const float* inv_scale,
                                int64_t images, float score_thr, float* scores, float* boxes, uint8_t* flags, mtp_stream_t stream) {
    MTP_CHECK_ARG(cls_score && bbox_pred && rois && img_shapes && scores && boxes && flags && R > 0 && R < ((int64_t)1 << 31) && images > 0);
    MTP_CHECK_ARG(num_classes >= 1 && num_classes < (1 << 16) && ld_cls > num_classes && ld_reg >= 4 * num_classes && ld_reg % 4 == 0);
    MTP_CHECK_ARG(aligned16(bbox_pred) && aligned16(boxes));
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, wh_ratio_clip, k));
    hroi_predict_kernel<<<(unsigned)((R + kWaves - 1) / kWaves), kThreads, 0, (hipStream_t)stream>>>(cls_score, ld_cls, bbox_pred, ld_reg, num_classes, rois, R, k,
                                                                                                   img_shapes, inv_scale, images, score_thr, scores, boxes,
                                                                                                   flags);
    return mtp_launch_status();
}
