// The oriented RPN of Oriented R-CNN (Multi-Task_Pretrain/rotated_detection: rpn_head.py, anchor_head.py, random_sampler.py; the coder is mmrotate's
// MidpointOffsetCoder with angle_version 'le90', restated from the published algorithm).  f32 boxes and logits, int64 indices, no float atomics, two
// calls give the same bits.
//   rpn_anchors    per level: the priors (H W A, 4) = base[a] + (x, y, x, y) * stride and the inside flag of every prior, one thread per prior
//   rpn_loss       one thread per slot of the per-image sample lists (positives first, then negatives): the flat anchor index -> (level, y, x, a),
//                  sigmoid BCE on the logit, for positives the midpoint-offset encode of (prior, assigned gt) and SmoothL1 on the six deltas; the dense
//                  gradients are plain stores into zeroed buffers (the indices of one image are distinct); the per-level sums of a workgroup go to a
//                  partial row (wave butterflies, then the four waves in order)
//   rpn_loss_sum   one wave adds the partial rows in order and scales by loss_weight / avg_factor, avg_factor = sum_b (n_pos[b] + n_neg[b]) read on
//                  the device
//   rpn_proposals  one thread per kept (image, level, rank): sigmoid score, decoded rotated box, its circumscribed box, level id and the size flag
//   rpn_encode / rpn_decode   the two __device__ functions on plain (n, .) arrays, for MidpointOffsetCoder
// The maps are addressed by element strides (image, channel, y, x): NCHW (N, A C, H, W) and the engines' rows (N H W, ld) run the same code.
// The decoded quadrilateral c0, c1, -c0, -c1 scaled to a common diagonal is a rectangle centred on (gx, gy) with edges c1 - c0 and c1 + c0, so the
// rotated box is a closed form: no minimum-area-rectangle search.  Contraction is off: tests/rpn_ref.py restates the same operations in the same order.
#include "common.h"
#include "rpn_levels.h"

#pragma clang fp contract(off)

namespace {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kMaxRatio = 4.135166556742356f;      // |log(16 / 1000)|

struct Codec {
    float mean[6], stdv[6];
};
// the circumscribed box of a rotated one as box_ops.hip has it; (ux, uy) and (vx, vy) are the half axes
struct GtGeom {
    float x1, y1, x2, y2, ux, uy, vx, vy;
};
__device__ __forceinline__ GtGeom gt_geom(const float* g) {
    const float hw = g[2] * 0.5f, hh = g[3] * 0.5f;
    float s, c;
    sincosf(g[4], &s, &c);
    const float ex = fabsf(hw * c) + fabsf(hh * s), ey = fabsf(hw * s) + fabsf(hh * c);
    GtGeom o;
    o.x1 = g[0] - ex; o.y1 = g[1] - ey; o.x2 = g[0] + ex; o.y2 = g[1] + ey;
    o.ux = hw * c; o.uy = hw * s; o.vx = -(hh * s); o.vy = hh * c;
    return o;
}

__device__ __forceinline__ void midpoint_encode(const float* p, const float* g, const Codec& k, float* out) {
    const float px = (p[0] + p[2]) * 0.5f, py = (p[1] + p[3]) * 0.5f, pw = p[2] - p[0], ph = p[3] - p[1];
    const GtGeom q = gt_geom(g);
    const float gx = (q.x1 + q.x2) * 0.5f, gy = (q.y1 + q.y2) * 0.5f, gw = q.x2 - q.x1, gh = q.y2 - q.y1;
    float X[4], Y[4];
    X[0] = (g[0] - q.ux) - q.vx; Y[0] = (g[1] - q.uy) - q.vy;
    X[1] = (g[0] + q.ux) - q.vx; Y[1] = (g[1] + q.uy) - q.vy;
    X[2] = (g[0] + q.ux) + q.vx; Y[2] = (g[1] + q.uy) + q.vy;
    X[3] = (g[0] - q.ux) + q.vx; Y[3] = (g[1] - q.uy) + q.vy;
    const float ymin = fminf(fminf(Y[0], Y[1]), fminf(Y[2], Y[3])), xmax = fmaxf(fmaxf(X[0], X[1]), fmaxf(X[2], X[3]));
    float ga = -1000.0f, gb = -1000.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!(fabsf(Y[i] - ymin) > 0.1f)) ga = fmaxf(ga, X[i]);
        if (!(fabsf(X[i] - xmax) > 0.1f)) gb = fmaxf(gb, Y[i]);
    }
    float d[6];
    d[0] = (gx - px) / pw; d[1] = (gy - py) / ph;
    d[2] = logf(gw / pw); d[3] = logf(gh / ph);
    d[4] = (ga - gx) / gw; d[5] = (gb - gy) / gh;
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = (d[i] - k.mean[i]) / k.stdv[i];
}

__device__ __forceinline__ float clampf(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// -> cx, cy, w, h, theta with w >= h and theta in [-pi/2, pi/2)
__device__ __forceinline__ void midpoint_decode(const float* p, const float* raw, const Codec& k, float* r) {
    const float px = (p[0] + p[2]) * 0.5f, py = (p[1] + p[3]) * 0.5f, pw = p[2] - p[0], ph = p[3] - p[1];
    float d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = raw[i] * k.stdv[i] + k.mean[i];
    const float dw = clampf(d[2], kMaxRatio), dh = clampf(d[3], kMaxRatio);
    const float gw = pw * expf(dw), gh = ph * expf(dh), gx = px + pw * d[0], gy = py + ph * d[1];
    const float da = clampf(d[4], 0.5f), db = clampf(d[5], 0.5f);
    const float c0x = da * gw, c0y = -(gh * 0.5f), c1x = gw * 0.5f, c1y = db * gh;
    const float n0 = sqrtf(c0x * c0x + c0y * c0y), n1 = sqrtf(c1x * c1x + c1y * c1y);
    const float diag = fmaxf(n0, n1);
    const float s0 = n0 > 0.0f ? diag / n0 : 0.0f, s1 = n1 > 0.0f ? diag / n1 : 0.0f;
    const float v0x = c0x * s0, v0y = c0y * s0, v1x = c1x * s1, v1y = c1y * s1;
    const float e1x = v1x - v0x, e1y = v1y - v0y, e2x = v1x + v0x, e2y = v1y + v0y;
    const float l1 = sqrtf(e1x * e1x + e1y * e1y), l2 = sqrtf(e2x * e2x + e2y * e2y);
    const bool first = l1 >= l2;
    float t = atan2f(first ? e1y : e2y, first ? e1x : e2x);
    if (t >= kPi * 0.5f) t -= kPi;
    if (t < -(kPi * 0.5f)) t += kPi;
    r[0] = gx; r[1] = gy; r[2] = first ? l1 : l2; r[3] = first ? l2 : l1; r[4] = t;
}

// ------------------------------------------------------------------------------------------------------------------- anchors
__global__ void __launch_bounds__(kThreads) rpn_anchors_kernel(const float* __restrict__ base, int64_t A, int64_t W, int64_t total, float sx, float sy,
                                                               int64_t valid_w, int64_t valid_h, float img_w, float img_h, float border,
                                                               float* __restrict__ priors, uint8_t* __restrict__ flags) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int64_t a = e % A, cell = e / A, x = cell % W, y = cell / W;
    const float4 b = load4(base + a * 4);
    const float fx = (float)x * sx, fy = (float)y * sy;
    const float4 o = make_float4(b.x + fx, b.y + fy, b.z + fx, b.w + fy);
    store4(priors + e * 4, o);
    bool in = x < valid_w && y < valid_h;
    if (border >= 0.0f) in = in && o.x >= -border && o.y >= -border && o.z < img_w + border && o.w < img_h + border;
    flags[e] = in ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------- targets and loss
struct LossArgs {
    const float* priors;
    const float* gts;
    const int64_t* samples;
    const int64_t* sample_gt;
    const int64_t* n_pos;
    const int64_t* n_neg;
    int64_t total, K, B, S;
    float beta;
};

__device__ __forceinline__ void sample_counts(const LossArgs& a, int64_t b, int64_t& np, int64_t& nn) {
    np = a.n_pos[b]; nn = a.n_neg[b];
    np = np < 0 ? 0 : (np > a.S ? a.S : np);
    nn = nn < 0 ? 0 : (nn > a.S - np ? a.S - np : nn);
}
__device__ __forceinline__ int64_t avg_factor(const LossArgs& a) {
    int64_t avg = 0;
    for (int64_t i = 0; i < a.B; ++i) {
        int64_t p, n;
        sample_counts(a, i, p, n);
        avg += p + n;
    }
    return avg;
}

// grid (chunks of the sample list, images); partial[(image * chunks + chunk) * 2 kL + level] = sum of the cls terms, + kL: of the bbox terms
__global__ void __launch_bounds__(kThreads) rpn_loss_kernel(Levels L, LossArgs a, Codec k, int A, float w_cls, float w_box, float* __restrict__ partial) {
    __shared__ float wsum[kThreads / MTP_WAVE][2 * kL];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y, j = (int64_t)blockIdx.x * kThreads + tid;
    int64_t np, nn;
    sample_counts(a, b, np, nn);
    const int64_t avg = avg_factor(a);
    const float g_cls = avg > 0 ? w_cls / (float)avg : 0.0f, g_box = avg > 0 ? w_box / (float)avg : 0.0f;
    int64_t idx = j < np + nn ? a.samples[b * a.S + j] : -1;
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
        const int64_t g = pos ? a.sample_gt[b * a.S + j] : -1;
        if (g >= 0 && g < a.K) {
            float tgt[6];
            midpoint_encode(a.priors + idx * 4, a.gts + g * 5, k, tgt);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const int64_t ro = b * v.rs[0] + (an * 6 + c) * v.rs[1] + y * v.rs[2] + x * v.rs[3];
                const float d = v.reg[ro] - tgt[c], ad = fabsf(d);
                lb += ad < a.beta ? (0.5f * ad) * ad / a.beta : ad - 0.5f * a.beta;
                if (v.dreg) v.dreg[ro] = (ad < a.beta ? d / a.beta : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f))) * g_box;
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
        for (int w = 0; w < kThreads / MTP_WAVE; ++w) s += wsum[w][tid];
        partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (2 * kL) + tid] = s;
    }
}

__global__ void __launch_bounds__(MTP_WAVE) rpn_loss_sum_kernel(const float* __restrict__ partial, int64_t blocks, LossArgs a, int levels, float w_cls,
                                                                float w_box, float* __restrict__ loss_cls, float* __restrict__ loss_box) {
    const int tid = threadIdx.x;
    if (tid >= 2 * kL) return;
    const int l = tid % kL;
    if (l >= levels) return;
    float s = 0.0f;
    for (int64_t i = 0; i < blocks; ++i) s += partial[i * (2 * kL) + tid];
    const int64_t avg = avg_factor(a);
    s = avg > 0 ? s / (float)avg : 0.0f;
    if (tid < kL) loss_cls[l] = s * w_cls;
    else loss_box[l] = s * w_box;
}

// ------------------------------------------------------------------------------------------------------------------- proposals
__global__ void __launch_bounds__(kThreads) rpn_proposals_kernel(Levels L, const float* __restrict__ priors, const int64_t* __restrict__ keep, int64_t B,
                                                                 int64_t T, Codec k, int A, float min_size, float* __restrict__ scores,
                                                                 float* __restrict__ rboxes, float* __restrict__ hboxes, int64_t* __restrict__ level_ids,
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
    float r[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, h[4] = {0.0f, 0.0f, 0.0f, 0.0f}, score = 0.0f;
    bool ok = false;
    if (idx >= 0 && idx < v.count) {
        const int64_t an = idx % A, cell = idx / A, x = cell % v.W, y = cell / v.W;
        score = 1.0f / (1.0f + expf(-v.cls[b * v.cs[0] + an * v.cs[1] + y * v.cs[2] + x * v.cs[3]]));
        float d[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] = v.reg[b * v.rs[0] + (an * 6 + c) * v.rs[1] + y * v.rs[2] + x * v.rs[3]];
        midpoint_decode(priors + (v.first + idx) * 4, d, k, r);
        const GtGeom q = gt_geom(r);
        h[0] = q.x1; h[1] = q.y1; h[2] = q.x2; h[3] = q.y2;
        ok = r[2] > min_size && r[3] > min_size;
    }
    scores[e] = score;
#pragma unroll
    for (int c = 0; c < 5; ++c) rboxes[e * 5 + c] = r[c];
    store4(hboxes + e * 4, make_float4(h[0], h[1], h[2], h[3]));
    level_ids[e] = l;
    valid[e] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------- the coder on its own
__global__ void __launch_bounds__(kThreads) rpn_encode_kernel(const float* __restrict__ priors, const float* __restrict__ gts, Codec k, int64_t n,
                                                              float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    float d[6];
    midpoint_encode(priors + e * 4, gts + e * 5, k, d);
#pragma unroll
    for (int c = 0; c < 6; ++c) out[e * 6 + c] = d[c];
}

__global__ void __launch_bounds__(kThreads) rpn_decode_kernel(const float* __restrict__ priors, const float* __restrict__ deltas, Codec k, int64_t n,
                                                              float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    float d[6], r[5];
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] = deltas[e * 6 + c];
    midpoint_decode(priors + e * 4, d, k, r);
#pragma unroll
    for (int c = 0; c < 5; ++c) out[e * 5 + c] = r[c];
}

bool make_codec(const float* means, const float* stds, Codec& k) {
    if (!means || !stds) return false;
    for (int i = 0; i < 6; ++i) {
        k.mean[i] = means[i];
        k.stdv[i] = stds[i];
        if (!(stds[i] > 0.0f)) return false;
    }
    return true;
}

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_rpn_anchors(const float* base_anchors, int64_t A, int64_t H, int64_t W, int64_t stride_w, int64_t stride_h, int64_t pad_h, int64_t pad_w,
                               int64_t img_h, int64_t img_w, float allowed_border, float* priors, uint8_t* inside_flags, mtp_stream_t stream) {
    MTP_CHECK_ARG(base_anchors && priors && inside_flags && A > 0 && H > 0 && W > 0 && stride_w > 0 && stride_h > 0);
    MTP_CHECK_ARG(pad_h >= 0 && pad_w >= 0 && img_h >= 0 && img_w >= 0 && A <= (1 << 16) && H <= (1 << 20) && W <= (1 << 20) && H * W * A < ((int64_t)1 << 31));
    MTP_CHECK_ARG(((uintptr_t)base_anchors & 15) == 0 && ((uintptr_t)priors & 15) == 0);
    const int64_t vw = (pad_w + stride_w - 1) / stride_w, vh = (pad_h + stride_h - 1) / stride_h, total = H * W * A;
    rpn_anchors_kernel<<<blocks_exact(total), kThreads, 0, (hipStream_t)stream>>>(base_anchors, A, W, total, (float)stride_w, (float)stride_h, vw < W ? vw : W,
                                                                                  vh < H ? vh : H, (float)img_w, (float)img_h, allowed_border, priors,
                                                                                  inside_flags);
    return mtp_launch_status();
}

extern "C" int64_t mtp_rpn_loss_workspace_bytes(int64_t images, int64_t samples) {
    if (images < 1 || samples < 1) return MTP_ERR_ARG;
    return images * ((samples + kThreads - 1) / kThreads) * 2 * kL * (int64_t)sizeof(float);
}

extern "C" int mtp_rpn_loss(const mtp_rpn_level* levels, int num_levels, int64_t A, const float* priors, int64_t num_priors, const float* gts, int64_t K,
                            const int64_t* samples, const int64_t* sample_gt, const int64_t* n_pos, const int64_t* n_neg, int64_t images, int64_t S,
                            const float* means, const float* stds, float beta, float cls_weight, float bbox_weight, float* loss_cls, float* loss_bbox,
                            void* workspace, int64_t workspace_bytes, mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && samples && sample_gt && n_pos && n_neg && loss_cls && loss_bbox && workspace && images > 0 && images <= 65535 && S > 0);
    MTP_CHECK_ARG(K >= 0 && (gts || K == 0) && num_priors < ((int64_t)1 << 31) && S < ((int64_t)1 << 31) && beta > 0.0f);
    MTP_CHECK_ARG(workspace_bytes >= mtp_rpn_loss_workspace_bytes(images, S) && ((uintptr_t)workspace & 3) == 0);
    Levels L;
    Codec k;
    int64_t T;
    MTP_CHECK_ARG(make_codec(means, stds, k) && make_levels(levels, num_levels, A, num_priors, false, L, T));
    const LossArgs a = {priors, gts, samples, sample_gt, n_pos, n_neg, num_priors, K, images, S, beta};
    const dim3 grid((unsigned)((S + kThreads - 1) / kThreads), (unsigned)images);
    hipStream_t s = (hipStream_t)stream;
    float* partial = static_cast<float*>(workspace);
    rpn_loss_kernel<<<grid, kThreads, 0, s>>>(L, a, k, (int)A, cls_weight, bbox_weight, partial);
    rpn_loss_sum_kernel<<<1, MTP_WAVE, 0, s>>>(partial, (int64_t)grid.x * grid.y, a, num_levels, cls_weight, bbox_weight, loss_cls, loss_bbox);
    return mtp_launch_status();
}

extern "C" int mtp_rpn_proposals(const mtp_rpn_level* levels, int num_levels, int64_t A, const float* priors, int64_t num_priors, const int64_t* keep,
                                 int64_t images, const float* means, const float* stds, float min_bbox_size, float* scores, float* rboxes, float* hboxes,
                                 int64_t* level_ids, uint8_t* valid, mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && keep && scores && rboxes && hboxes && level_ids && valid && images > 0 && num_priors < ((int64_t)1 << 31));
    MTP_CHECK_ARG(((uintptr_t)hboxes & 15) == 0);
    Levels L;
    Codec k;
    int64_t T;
    MTP_CHECK_ARG(make_codec(means, stds, k) && make_levels(levels, num_levels, A, num_priors, true, L, T));
    MTP_CHECK_ARG(T > 0 && images < ((int64_t)1 << 31) / T);
    rpn_proposals_kernel<<<blocks_exact(images * T), kThreads, 0, (hipStream_t)stream>>>(L, priors, keep, images, T, k, (int)A, min_bbox_size, scores, rboxes,
                                                                                         hboxes, level_ids, valid);
    return mtp_launch_status();
}

extern "C" int mtp_rpn_encode(const float* priors, const float* gts, const float* means, const float* stds, int64_t n, float* deltas, mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && gts && deltas && n > 0 && n < ((int64_t)1 << 31));
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, k));
    rpn_encode_kernel<<<blocks_exact(n), kThreads, 0, (hipStream_t)stream>>>(priors, gts, k, n, deltas);
    return mtp_launch_status();
}

extern "C" int mtp_rpn_decode(const float* priors, const float* deltas, const float* means, const float* stds, int64_t n, float* rboxes, mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && deltas && rboxes && n > 0 && n < ((int64_t)1 << 31));
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, k));
    rpn_decode_kernel<<<blocks_exact(n), kThreads, 0, (hipStream_t)stream>>>(priors, deltas, k, n, rboxes);
    return mtp_launch_status();
}
