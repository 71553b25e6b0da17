// The RoI head of Oriented R-CNN (Multi-Task_Pretrain/rotated_detection: standard_roi_head.py, bbox_head.py, base_bbox_head.py; configured at
// oriented_rcnn.py:41-75, 100-128).  RoIAlignRotated and DeltaXYWHTRBBoxCoder are restated from the published mmcv / mmrotate algorithms (DESIGN
// section 16).  f32 everywhere, int64 indices, no float atomics, two calls give the same bits.
//   roi_align_fwd       one workgroup per RoI: the first threads work out the out_size^2 x sample_num^2 sample points (four corner offsets and four
//                       bilinear weights each, channel-independent) into LDS, then all threads walk (bin, channel) with the channel fastest, so
//                       the map reads (channels-last rows) and the (R, bins, C) stores coalesce.  A padded slot writes zeros and reads nothing.
//   roi_align_entries   one thread per (RoI, bin, sample): the four (pixel key, weight / count) entries of the backward
//   roi_align_gather    after a stable sort of the keys: one wave per sorted position and 64-channel chunk; the wave whose position starts a run of
//                       equal keys owns that pixel and adds the run in sorted order, then stores (or adds to what is there: accumulate)
//   roi_loss            one thread per slot of the fixed-size sample lists: label, softmax cross-entropy, the delta encode of (RoI, gt) and
//                       SmoothL1 on positives, top-1 hit; dense gradients by plain stores; workgroup sums to a partial row
//   roi_loss_sum        one wave adds the partial rows in order and divides by the counts read on the device
//   roi_predict         one thread per RoI: softmax scores, the decoded box, the score > score_thr flags of the (roi, class) table
//   rbox_delta_encode / rbox_delta_decode   the two __device__ functions on plain (n, 5) arrays, for DeltaXYWHTRBBoxCoder
// The maps are addressed by element strides (image, channel, y, x) as mtp_rpn_level does.  Contraction is off: tests/roi_ref.py restates the same
// operations in the same order.
#include "common.h"
#include "roi_levels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxEntries = 4096;                    // out_size^2 x sample_num^2 x 4 corners per RoI, in LDS
constexpr float kPi = 3.14159265358979323846f;
constexpr float kMaxRatio = 4.135166556742356f;      // |log(16 / 1000)|

struct Geom {
    int P, S, clockwise;      // out_size, sample_num
    float finest;
    int64_t images, C, R, per_group;
};

__device__ __forceinline__ int roi_level(const float* roi, float finest, int n) {
    const float v = floorf(log2f(sqrtf(roi[3] * roi[4]) / finest + 1e-6f));
    return v >= 1.0f ? (int)fminf(v, (float)(n - 1)) : 0;      // NaN -> 0
}

// slot r of the fixed-size lists is in use: r % per_group < valid[r / per_group]; the image index is an index
__device__ __forceinline__ bool roi_in_use(const Geom& g, const float* rois, const int64_t* valid, int64_t r, int64_t& image) {
    const float b = rois[r * 6];
    image = b >= 0.0f && b < (float)g.images ? (int64_t)b : -1;
    if (image < 0) return false;
    return valid ? (r % g.per_group) < valid[r / g.per_group] : true;
}

// sample s of bin `bin`: the four corners (element offsets inside one channel plane of one image; off[0] < 0: the point lies outside) and weights
__device__ __forceinline__ void sample_point(const float* roi, const Level& v, const Geom& g, int bin, int s, int64_t* y4, int64_t* x4, float* w4) {
    const float cx = roi[1] * v.scale - 0.5f, cy = roi[2] * v.scale - 0.5f, rw = roi[3] * v.scale, rh = roi[4] * v.scale;
    const float th = g.clockwise ? -roi[5] : roi[5];
    float sn, cs;
    sincosf(th, &sn, &cs);
    const float bh = rh / (float)g.P, bw = rw / (float)g.P;
    const int ph = bin / g.P, pw = bin % g.P, iy = s / g.S, ix = s % g.S;
    const float yy = (-rh / 2.0f + (float)ph * bh) + ((float)iy + 0.5f) * bh / (float)g.S;
    const float xx = (-rw / 2.0f + (float)pw * bw) + ((float)ix + 0.5f) * bw / (float)g.S;
    float y = (yy * cs - xx * sn) + cy, x = (yy * sn + xx * cs) + cx;
    const float Hf = (float)v.H, Wf = (float)v.W;
    if (!(y >= -1.0f && y <= Hf && x >= -1.0f && x <= Wf)) {      // NaN lands here too
        y4[0] = -1;
        return;
    }
    if (y <= 0.0f) y = 0.0f;
    if (x <= 0.0f) x = 0.0f;
    int64_t yl = (int64_t)y, xl = (int64_t)x, yh, xh;
    if (yl >= v.H - 1) { yh = yl = v.H - 1; y = (float)yl; } else yh = yl + 1;
    if (xl >= v.W - 1) { xh = xl = v.W - 1; x = (float)xl; } else xh = xl + 1;
    const float ly = y - (float)yl, lx = x - (float)xl, hy = 1.0f - ly, hx = 1.0f - lx;
    y4[0] = yl; y4[1] = yl; y4[2] = yh; y4[3] = yh;
    x4[0] = xl; x4[1] = xh; x4[2] = xl; x4[3] = xh;
    w4[0] = hy * hx; w4[1] = hy * lx; w4[2] = ly * hx; w4[3] = ly * lx;
}

// ------------------------------------------------------------------------------------------------------------------- RoIAlignRotated forward
__global__ void __launch_bounds__(kThreads) roi_align_fwd_kernel(Levels L, Geom g, const float* __restrict__ rois, const int32_t* __restrict__ level_in,
                                                                 const int64_t* __restrict__ valid, float* __restrict__ out,
                                                                 int32_t* __restrict__ level_out) {
    __shared__ int64_t s_off[kMaxEntries];
    __shared__ float s_w[kMaxEntries];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int PP = g.P * g.P, S2 = g.S * g.S;
    int64_t image;
    const bool ok = roi_in_use(g, rois, valid, r, image);      // the same for the whole workgroup
    const float* roi = rois + r * 6;
    int l = level_in ? level_in[r] : roi_level(roi, g.finest, L.n);
    l = l < 0 ? 0 : (l >= L.n ? L.n - 1 : l);
    if (tid == 0 && level_out) level_out[r] = ok ? l : -1;
    float* o = out + r * PP * g.C;
    if (!ok) {
        for (int64_t i = tid; i < PP * g.C; i += kThreads) o[i] = 0.0f;
        return;
    }
    const Level& v = L.lv[l];
    for (int i = tid; i < PP * S2; i += kThreads) {
        int64_t y4[4], x4[4];
        float w4[4];
        sample_point(roi, v, g, i / S2, i % S2, y4, x4, w4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s_off[i * 4 + k] = y4[0] < 0 ? -1 : y4[k] * v.st[2] + x4[k] * v.st[3];
            s_w[i * 4 + k] = y4[0] < 0 ? 0.0f : w4[k];
        }
    }
    __syncthreads();
    const float count = (float)(S2 > 1 ? S2 : 1);
    const float* plane = v.map + image * v.st[0];
    for (int64_t i = tid; i < PP * g.C; i += kThreads) {
        const int64_t bin = i / g.C, c = i - bin * g.C;
        const float* base = plane + c * v.st[1];
        float acc = 0.0f;
        for (int s = 0; s < S2; ++s) {
            const int e = ((int)bin * S2 + s) * 4;
            if (s_off[e] < 0) continue;
            const float val = ((s_w[e] * base[s_off[e]] + s_w[e + 1] * base[s_off[e + 1]]) + s_w[e + 2] * base[s_off[e + 2]]) + s_w[e + 3] * base[s_off[e + 3]];
            acc += val;
        }
        o[i] = acc / count;
    }
}

// ------------------------------------------------------------------------------------------------------------------- RoIAlignRotated backward
// entry ((r PP + bin) S2 + s) 4 + corner: key = the pixel in (level, image, y, x) order, or L.pixels; weight = bilinear weight / count
__global__ void __launch_bounds__(kThreads) roi_align_entries_kernel(Levels L, Geom g, const float* __restrict__ rois, const int32_t* __restrict__ level_in,
                                                                     const int64_t* __restrict__ valid, int64_t* __restrict__ keys,
                                                                     float* __restrict__ weights) {
    const int PP = g.P * g.P, S2 = g.S * g.S;
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= g.R * PP * S2) return;
    const int64_t r = t / (PP * S2);
    const int i = (int)(t - r * (PP * S2));
    int64_t image;
    const bool ok = roi_in_use(g, rois, valid, r, image);
    const float* roi = rois + r * 6;
    int l = level_in ? level_in[r] : roi_level(roi, g.finest, L.n);
    l = l < 0 ? 0 : (l >= L.n ? L.n - 1 : l);
    const Level& v = L.lv[l];
    int64_t y4[4] = {-1, 0, 0, 0}, x4[4] = {0, 0, 0, 0};
    float w4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) sample_point(roi, v, g, i / S2, i % S2, y4, x4, w4);
    const float count = (float)(S2 > 1 ? S2 : 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool in = ok && y4[0] >= 0;
        keys[t * 4 + k] = in ? v.first + (image * v.H + y4[k]) * v.W + x4[k] : L.pixels;
        weights[t * 4 + k] = in ? w4[k] / count : 0.0f;
    }
}

// grid (ceil(n / 4), ceil(C / 64)): wave w of a workgroup looks at sorted position blockIdx.x * 4 + w, lane c at channel blockIdx.y * 64 + c
__global__ void __launch_bounds__(kThreads) roi_align_gather_kernel(Levels L, Geom g, const float* __restrict__ dout, const int64_t* __restrict__ keys,
                                                                    const int64_t* __restrict__ order, const float* __restrict__ weights, int64_t n,
                                                                    int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * (kThreads / MTP_WAVE) + threadIdx.x / MTP_WAVE;
    const int64_t c = (int64_t)blockIdx.y * MTP_WAVE + threadIdx.x % MTP_WAVE;
    if (i >= n || c >= g.C) return;
    const int64_t key = keys[i];
    if (key < 0 || key >= L.pixels || (i > 0 && keys[i - 1] == key)) return;      // nothing touched, or not the owner
    int l = 0;
#pragma unroll
    for (int k = 1; k < kL; ++k)
        if (k < L.n && key >= L.lv[k].first) l = k;
    const Level& v = L.lv[l];
    const int64_t local = key - v.first, x = local % v.W, y = (local / v.W) % v.H, image = local / (v.W * v.H);
    if (image >= g.images) return;
    const int per = g.S * g.S * 4;
    float acc = 0.0f;
    for (int64_t j = i; j < n && keys[j] == key; ++j) {
        const int64_t e = order[j];
        if (e < 0 || e >= n) continue;
        acc += weights[e] * dout[(e / per) * g.C + c];
    }
    float* dst = v.dmap + image * v.st[0] + c * v.st[1] + y * v.st[2] + x * v.st[3];
    *dst = accumulate ? *dst + acc : acc;
}

// ------------------------------------------------------------------------------------------------------------------- DeltaXYWHTRBBoxCoder, 'le90'
struct Codec {
    float mean[5], stdv[5];
};

__device__ __forceinline__ float norm_angle(float a) {      // (a + pi/2) mod pi - pi/2, the modulus with the sign of pi
    const float t = a + kPi * 0.5f;
    return (t - floorf(t / kPi) * kPi) - kPi * 0.5f;
}

// p, g: cx, cy, w, h, theta
__device__ __forceinline__ void delta_encode(const float* p, const float* g, const Codec& k, float* out) {
    float sn, cs;
    sincosf(p[4], &sn, &cs);
    const float ex = g[0] - p[0], ey = g[1] - p[1];
    float d[5];
    d[0] = (cs * ex + sn * ey) / p[2];
    d[1] = (-sn * ex + cs * ey) / p[3];
    const float d1 = norm_angle(g[4] - p[4]), d2 = norm_angle((g[4] - p[4]) + kPi * 0.5f);
    const bool first = fabsf(d1) < fabsf(d2);
    d[2] = logf((first ? g[2] : g[3]) / p[2]);
    d[3] = logf((first ? g[3] : g[2]) / p[3]);
    d[4] = first ? d1 : d2;
#pragma unroll
    for (int i = 0; i < 5; ++i) out[i] = (d[i] - k.mean[i]) / k.stdv[i];
}

__device__ __forceinline__ float clampf(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// -> cx, cy, w, h, theta with w >= h and theta in [-pi/2, pi/2)
__device__ __forceinline__ void delta_decode(const float* p, const float* raw, const Codec& k, float* r) {
    float d[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) d[i] = raw[i] * k.stdv[i] + k.mean[i];
    const float dw = clampf(d[2], kMaxRatio), dh = clampf(d[3], kMaxRatio);
    float sn, cs;
    sincosf(p[4], &sn, &cs);
    const float gx = ((d[0] * p[2]) * cs - (d[1] * p[3]) * sn) + p[0], gy = ((d[0] * p[2]) * sn + (d[1] * p[3]) * cs) + p[1];
    const float gw = p[2] * expf(dw), gh = p[3] * expf(dh), ga = norm_angle(p[4] + d[4]);
    const bool keep = gw > gh;
    r[0] = gx; r[1] = gy; r[2] = keep ? gw : gh; r[3] = keep ? gh : gw;
    r[4] = norm_angle(keep ? ga : ga + kPi * 0.5f);
}

__global__ void __launch_bounds__(kThreads) rbox_encode_kernel(const float* __restrict__ priors, const float* __restrict__ gts, Codec k, int64_t n,
                                                               float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    float d[5];
    delta_encode(priors + e * 5, gts + e * 5, k, d);
#pragma unroll
    for (int c = 0; c < 5; ++c) out[e * 5 + c] = d[c];
}

__global__ void __launch_bounds__(kThreads) rbox_decode_kernel(const float* __restrict__ priors, const float* __restrict__ deltas, Codec k, int64_t n,
                                                               float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    float d[5], r[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) d[c] = deltas[e * 5 + c];
    delta_decode(priors + e * 5, d, k, r);
#pragma unroll
    for (int c = 0; c < 5; ++c) out[e * 5 + c] = r[c];
}

// ------------------------------------------------------------------------------------------------------------------- targets and loss
struct LossArgs {
    const float* cls;
    const float* reg;
    float* dcls;
    float* dreg;
    int64_t ldc, ldr, K;      // K classes, K + 1 logits per row
    const float* rois;        // (images S, 5)
    const float* gts;         // (G, 5)
    const int64_t* gt_labels; // (G)
    const int64_t* sample_gt; // (images, S)
    const int64_t* n_pos;
    const int64_t* n_neg;
    int64_t G, B, S;
    float beta;
};

__device__ __forceinline__ void sample_counts(const LossArgs& a, int64_t b, int64_t& np, int64_t& nn) {
    np = a.n_pos[b]; nn = a.n_neg[b];
    np = np < 0 ? 0 : (np > a.S ? a.S : np);
    nn = nn < 0 ? 0 : (nn > a.S - np ? a.S - np : nn);
}
__device__ __forceinline__ int64_t total_samples(const LossArgs& a) {
    int64_t t = 0;
    for (int64_t i = 0; i < a.B; ++i) {
        int64_t p, n;
        sample_counts(a, i, p, n);
        t += p + n;
    }
    return t;
}

// grid (chunks of the sample list, images); partial[(image * chunks + chunk) * 3 + (cls, bbox, hits)]
__global__ void __launch_bounds__(kThreads) roi_loss_kernel(LossArgs a, Codec k, float w_cls, float w_box, float* __restrict__ partial) {
    __shared__ float wsum[kThreads / MTP_WAVE][3];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y, j = (int64_t)blockIdx.x * kThreads + tid;
    int64_t np, nn;
    sample_counts(a, b, np, nn);
    __shared__ int64_t s_total;      // the sum over the images, once per workgroup
    if (tid == 0) s_total = total_samples(a);
    __syncthreads();
    const int64_t total = s_total;
    const float g_cls = w_cls / (float)(total > 1 ? total : 1), g_box = total > 0 ? w_box / (float)total : 0.0f;
    float lc = 0.0f, lb = 0.0f, hit = 0.0f;
    if (j < a.S) {
        const int64_t row = b * a.S + j;
        const bool used = j < np + nn;
        const int64_t g = used && j < np ? a.sample_gt[row] : -1;
        const bool pos = g >= 0 && g < a.G;
        int64_t label = pos ? a.gt_labels[g] : a.K;
        if (label < 0 || label > a.K) label = a.K;
        const float* z = a.cls + row * a.ldc;
        float* dz = a.dcls ? a.dcls + row * a.ldc : nullptr;
        if (used) {
            float m = z[0];
            int64_t arg = 0;
            for (int64_t c = 1; c <= a.K; ++c)
                if (z[c] > m) { m = z[c]; arg = c; }
            float sum = 0.0f;
            for (int64_t c = 0; c <= a.K; ++c) sum += expf(z[c] - m);
            lc = (logf(sum) + m) - z[label];
            hit = arg == label ? 1.0f : 0.0f;
            if (dz)
                for (int64_t c = 0; c <= a.K; ++c) dz[c] = (expf(z[c] - m) / sum - (c == label ? 1.0f : 0.0f)) * g_cls;
        } else if (dz) {
            for (int64_t c = 0; c <= a.K; ++c) dz[c] = 0.0f;
        }
        float* dr = a.dreg ? a.dreg + row * a.ldr : nullptr;
        if (pos) {
            float tgt[5];
            delta_encode(a.rois + row * 5, a.gts + g * 5, k, tgt);
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                const float d = a.reg[row * a.ldr + c] - tgt[c], ad = fabsf(d);
                lb += ad < a.beta ? (0.5f * ad) * ad / a.beta : ad - 0.5f * a.beta;
                if (dr) dr[c] = (ad < a.beta ? d / a.beta : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f))) * g_box;
            }
        } else if (dr) {
#pragma unroll
            for (int c = 0; c < 5; ++c) dr[c] = 0.0f;
        }
    }
    const int wave = tid / MTP_WAVE, lane = tid % MTP_WAVE;
    const float sc = wave_sum(lc), sb = wave_sum(lb), sh = wave_sum(hit);
    if (lane == 0) {
        wsum[wave][0] = sc; wsum[wave][1] = sb; wsum[wave][2] = sh;
    }
    __syncthreads();
    if (tid < 3) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < kThreads / MTP_WAVE; ++w) s += wsum[w][tid];
        partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + tid] = s;
    }
}

// out[0] = loss_cls, out[1] = loss_bbox, out[2] = acc (percent)
__global__ void __launch_bounds__(MTP_WAVE) roi_loss_sum_kernel(const float* __restrict__ partial, int64_t blocks, LossArgs a, float w_cls, float w_box,
                                                                float* __restrict__ out) {
    const int tid = threadIdx.x;
    if (tid >= 3) return;
    float s = 0.0f;
    for (int64_t i = 0; i < blocks; ++i) s += partial[i * 3 + tid];
    const int64_t total = total_samples(a);
    if (tid == 0) out[0] = s / (float)(total > 1 ? total : 1) * w_cls;
    else if (tid == 1) out[1] = total > 0 ? s / (float)total * w_box : 0.0f;
    else out[2] = total > 0 ? s * 100.0f / (float)total : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------------- predict
__global__ void __launch_bounds__(kThreads) roi_predict_kernel(const float* __restrict__ cls, int64_t ldc, const float* __restrict__ reg, int64_t ldr, int64_t K,
                                                               const float* __restrict__ rois, int64_t R, Codec k, float score_thr,
                                                               float* __restrict__ scores, float* __restrict__ boxes, uint8_t* __restrict__ flags) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const float* z = cls + r * ldc;
    float m = z[0];
    for (int64_t c = 1; c <= K; ++c) m = fmaxf(m, z[c]);
    float sum = 0.0f;
    for (int64_t c = 0; c <= K; ++c) sum += expf(z[c] - m);
    for (int64_t c = 0; c < K; ++c) {
        const float s = expf(z[c] - m) / sum;
        scores[r * K + c] = s;
        flags[r * K + c] = s > score_thr ? 1 : 0;
    }
    float d[5], o[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) d[c] = reg[r * ldr + c];
    delta_decode(rois + r * 5, d, k, o);
#pragma unroll
    for (int c = 0; c < 5; ++c) boxes[r * 5 + c] = o[c];
}

bool make_codec(const float* means, const float* stds, Codec& k) {
    if (!means || !stds) return false;
    for (int i = 0; i < 5; ++i) {
        k.mean[i] = means[i];
        k.stdv[i] = stds[i];
        if (!(stds[i] > 0.0f)) return false;
    }
    return true;
}

bool make_geom(int64_t images, int64_t C, int64_t R, int64_t per_group, const int64_t* valid, int out_size, int sample_num, int clockwise,
               float finest_scale, Geom& g) {
    if (C < 1 || C > (1 << 20) || R < 1 || R > (1 << 24) || out_size < 1 || sample_num < 1 || !(finest_scale > 0.0f)) return false;
    if ((int64_t)out_size * out_size * sample_num * sample_num * 4 > kMaxEntries) return false;
    if (valid && (per_group < 1 || R % per_group)) return false;
    g.P = out_size; g.S = sample_num; g.clockwise = clockwise ? 1 : 0; g.finest = finest_scale;
    g.images = images; g.C = C; g.R = R; g.per_group = valid ? per_group : R;
    return true;
}

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_roi_align_rotated_fwd(const mtp_roi_level* levels, int num_levels, int64_t images, int64_t C, const float* rois,
                                         const int32_t* roi_levels, const int64_t* valid, int64_t R, int64_t per_group, int out_size, int sample_num,
                                         int clockwise, float finest_scale, float* out, int32_t* levels_out, mtp_stream_t stream) {
    MTP_CHECK_ARG(rois && out);
    Levels L;
    Geom g;
    MTP_CHECK_ARG(make_levels(levels, num_levels, images, 1, L) && make_geom(images, C, R, per_group, valid, out_size, sample_num, clockwise, finest_scale, g));
    roi_align_fwd_kernel<<<(unsigned)R, kThreads, 0, (hipStream_t)stream>>>(L, g, rois, roi_levels, valid, out, levels_out);
    return mtp_launch_status();
}

extern "C" int64_t mtp_roi_align_rotated_entries(int64_t R, int out_size, int sample_num) {
    if (R < 1 || out_size < 1 || sample_num < 1) return MTP_ERR_ARG;
    return R * out_size * out_size * sample_num * sample_num * 4;
}

extern "C" int mtp_roi_align_rotated_bwd_entries(const mtp_roi_level* levels, int num_levels, int64_t images, const float* rois, const int32_t* roi_levels,
                                                 const int64_t* valid, int64_t R, int64_t per_group, int out_size, int sample_num, int clockwise,
                                                 float finest_scale, int64_t* keys, float* weights, mtp_stream_t stream) {
    MTP_CHECK_ARG(rois && keys && weights);
    Levels L;
    Geom g;
    MTP_CHECK_ARG(make_levels(levels, num_levels, images, 0, L) && make_geom(images, 1, R, per_group, valid, out_size, sample_num, clockwise, finest_scale, g));
    const int64_t points = R * out_size * out_size * sample_num * sample_num;
    roi_align_entries_kernel<<<blocks_exact(points), kThreads, 0, (hipStream_t)stream>>>(L, g, rois, roi_levels, valid, keys, weights);
    return mtp_launch_status();
}

extern "C" int mtp_roi_align_rotated_bwd_gather(const mtp_roi_level* levels, int num_levels, int64_t images, int64_t C, const float* dout,
                                                const int64_t* sorted_keys, const int64_t* order, const float* weights, int64_t R, int out_size,
                                                int sample_num, int accumulate, mtp_stream_t stream) {
    MTP_CHECK_ARG(dout && sorted_keys && order && weights);
    Levels L;
    Geom g;
    MTP_CHECK_ARG(make_levels(levels, num_levels, images, 2, L) && make_geom(images, C, R, 0, nullptr, out_size, sample_num, 0, 1.0f, g));
    const int64_t n = mtp_roi_align_rotated_entries(R, out_size, sample_num);
    const int64_t bx = (n + kThreads / MTP_WAVE - 1) / (kThreads / MTP_WAVE), by = (C + MTP_WAVE - 1) / MTP_WAVE;
    MTP_CHECK_ARG(bx < ((int64_t)1 << 31) && by <= 65535);
    roi_align_gather_kernel<<<dim3((unsigned)bx, (unsigned)by), kThreads, 0, (hipStream_t)stream>>>(L, g, dout, sorted_keys, order, weights, n, accumulate);
    return mtp_launch_status();
}

extern "C" int mtp_rbox_delta_encode(const float* priors, const float* gts, const float* means, const float* stds, int64_t n, float* deltas,
                                     mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && gts && deltas && n > 0 && n < ((int64_t)1 << 31));
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, k));
    rbox_encode_kernel<<<blocks_exact(n), kThreads, 0, (hipStream_t)stream>>>(priors, gts, k, n, deltas);
    return mtp_launch_status();
}

extern "C" int mtp_rbox_delta_decode(const float* priors, const float* deltas, const float* means, const float* stds, int64_t n, float* rboxes,
                                     mtp_stream_t stream) {
    MTP_CHECK_ARG(priors && deltas && rboxes && n > 0 && n < ((int64_t)1 << 31));
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, k));
    rbox_decode_kernel<<<blocks_exact(n), kThreads, 0, (hipStream_t)stream>>>(priors, deltas, k, n, rboxes);
    return mtp_launch_status();
}

extern "C" int64_t mtp_roi_loss_workspace_bytes(int64_t images, int64_t samples) {
    if (images < 1 || samples < 1) return MTP_ERR_ARG;
    return images * ((samples + kThreads - 1) / kThreads) * 3 * (int64_t)sizeof(float);
}

extern "C" int mtp_roi_loss(const float* cls_score, int64_t ld_cls, const float* bbox_pred, int64_t ld_reg, int64_t num_classes, const float* rois,
                            const float* gts, const int64_t* gt_labels, int64_t num_gts, const int64_t* sample_gt, const int64_t* n_pos,
                            const int64_t* n_neg, int64_t images, int64_t S, const float* means, const float* stds, float beta, float cls_weight,
                            float bbox_weight, float* losses, float* dcls, float* dreg, void* workspace, int64_t workspace_bytes, mtp_stream_t stream) {
    MTP_CHECK_ARG(cls_score && bbox_pred && rois && sample_gt && n_pos && n_neg && losses && workspace && images > 0 && images <= 65535 && S > 0);
    MTP_CHECK_ARG(num_classes >= 1 && num_classes < (1 << 16) && ld_cls > num_classes && ld_reg >= 5 && S < ((int64_t)1 << 31) && beta > 0.0f);
    MTP_CHECK_ARG(num_gts >= 0 && ((gts && gt_labels) || num_gts == 0) && (dcls != nullptr) == (dreg != nullptr));
    MTP_CHECK_ARG(workspace_bytes >= mtp_roi_loss_workspace_bytes(images, S) && ((uintptr_t)workspace & 3) == 0);
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, k));
    const LossArgs a = {cls_score, bbox_pred, dcls, dreg, ld_cls, ld_reg, num_classes, rois, gts, gt_labels, sample_gt, n_pos, n_neg, num_gts, images, S, beta};
    const dim3 grid((unsigned)((S + kThreads - 1) / kThreads), (unsigned)images);
    hipStream_t s = (hipStream_t)stream;
    float* partial = static_cast<float*>(workspace);
    roi_loss_kernel<<<grid, kThreads, 0, s>>>(a, k, cls_weight, bbox_weight, partial);
    roi_loss_sum_kernel<<<1, MTP_WAVE, 0, s>>>(partial, (int64_t)grid.x * grid.y, a, cls_weight, bbox_weight, losses);
    return mtp_launch_status();
}

extern "C" int mtp_roi_predict(const float* cls_score, int64_t ld_cls, const float* bbox_pred, int64_t ld_reg, int64_t num_classes, const float* rois,
                               int64_t R, const float* means, const float* stds, float score_thr, float* scores, float* boxes, uint8_t* flags,
                               mtp_stream_t stream) {
    MTP_CHECK_ARG(cls_score && bbox_pred && rois && scores && boxes && flags && R > 0 && R < ((int64_t)1 << 31));
    MTP_CHECK_ARG(num_classes >= 1 && num_classes < (1 << 16) && ld_cls > num_classes && ld_reg >= 5);
    Codec k;
    MTP_CHECK_ARG(make_codec(means, stds, k));
    roi_predict_kernel<<<blocks_exact(R), kThreads, 0, (hipStream_t)stream>>>(cls_score, ld_cls, bbox_pred, ld_reg, num_classes, rois, R, k, score_thr, scores,
                                                                             boxes, flags);
    return mtp_launch_status();
}
