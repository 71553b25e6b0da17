// The mask branch of Mask R-CNN (Multi-Task_Pretrain/instance_segmentation: mask_head.py, roi_head.py; configured at mask_rcnn.py:56-68, 92-119).
// RoIAlign, mask_target / crop_and_resize, mask_cross_entropy and grid_sample are restated from the published mmcv / mmdet / PyTorch algorithms
// (DESIGN section 18).  f32 everywhere, int64 indices, no float atomics, two calls give the same bits.
//   roialign_fwd      one workgroup per RoI; threads walk (bin, channel) with the channel fastest, so the four corner loads of a sample (channels-last
//                     rows) and the (R, bins, C) stores coalesce.  The sample grid is sampling_ratio^2 or the adaptive ceil(roi / out)^2, which has no
//                     bound: nothing is kept per sample, every thread walks its bin's grid.  A padded slot writes zeros and reads nothing.
//   roialign_bwd      a gather: one wave per map pixel and 256-channel chunk walks the RoIs in index order, 64 at a time (one lane tests one RoI,
//                     a ballot names the ones that touch the pixel).  The bilinear weights of an axis-aligned RoI are separable,
//                     d pixel = sum_ij dOut[i, j] / count * Wy[i, py] * Wx[j, px]: lanes 0 .. P - 1 add up Wy, lanes 32 .. 32 + P - 1 Wx, and the
//                     wave reads them by shuffles.  No entries, no sort, no workspace; every pixel of every level is stored.
//   mask_loss         one workgroup per sample slot: the box clipped to the gt's image, the slot's gt bitmap sampled at M x M by the RoIAlign rule
//                     (aligned, adaptive grid, scale 1), >= 0.5, binary cross-entropy with the logits of the slot's class channel; the targets, the
//                     slot's loss sum and the dense gradient (all K channels, padding slots too) by plain stores
//   mask_loss_sum     one wave adds the slot sums in a fixed order and divides by n_pos_total M M, read on the device
//   mask_paste        one thread per (instance, image pixel): sigmoid of the class channel sampled bilinearly with zero padding (grid_sample,
//                     align_corners=False) at the pixel centre mapped through the box, then the threshold (bool) or x 255 (uint8)
// Work is bounded by the maps, not by the boxes: of a bin's sample grid only the stretch that can fall inside [-1, size] is walked (the rest adds 0
// by mmcv's border rule), so a box of 1e9 pixels costs what a box of the map's size costs.  Contraction is off: tests/mask_ref.py restates the same
// operations in the same order.
#include "common.h"
#include "roi_levels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxOut = 32;           // out_size of the RoIAlign pair: the backward keeps Wy / Wx in the two halves of a wave
constexpr int kMaxSampling = 64;      // a fixed sampling_ratio
constexpr int kLaneChannels = 4;      // channels a lane of the backward owns, 64 apart
constexpr int kDenseGrid = 8;         // grids up to this are walked whole
constexpr float kMaxGrid = 16777216.0f;      // 2^24: an adaptive grid beyond it is cut (its sample index would not be exact in f32)

struct Geom {
    int P, sampling, aligned;      // out_size; sampling_ratio (0: adaptive)
    float finest;
    int64_t images, C, R, per_group;
};

// mmdet's map_roi_levels; NaN (a box with x2 < x1 and y2 > y1) -> 0
__device__ __forceinline__ int roi_level(const float* roi, float finest, int n) {
    const float v = floorf(log2f(sqrtf((roi[3] - roi[1]) * (roi[4] - roi[2])) / finest + 1e-6f));
    return v >= 1.0f ? (int)fminf(v, (float)(n - 1)) : 0;
}

// slot r of the fixed-size lists is in use: r % per_group < valid[r / per_group]; the image index is an index
__device__ __forceinline__ bool roi_in_use(const Geom& g, const float* rois, const int64_t* valid, int64_t r, int64_t& image) {
    const float b = rois[r * 5];
    image = b >= 0.0f && b < (float)g.images ? (int64_t)b : -1;
    if (image < 0) return false;
    return valid ? (r % g.per_group) < valid[r / g.per_group] : true;
}

// one axis of a RoI on a map: start, bin size, grid
struct Axis {
    float start, bin;
    int grid;
};
__device__ __forceinline__ Axis make_axis(float a, float b, float scale, int P, int sampling, int aligned) {
    const float off = aligned ? 0.5f : 0.0f;
    const float lo = a * scale - off, hi = b * scale - off;
    float len = hi - lo;
    if (!aligned) len = fmaxf(len, 1.0f);
    Axis x;
    x.start = lo;
    x.bin = len / (float)P;
    x.grid = sampling > 0 ? sampling : (int)fminf(fmaxf(ceilf(len / (float)P), 0.0f), kMaxGrid);      // NaN -> 0
    return x;
}
__device__ __forceinline__ float grid_count(const Axis& y, const Axis& x) { return fmaxf((float)y.grid * (float)x.grid, 1.0f); }

// the stretch [lo, hi) of bin p's grid that can fall inside [-1, size]: wide by 2 and 1e-5 of itself, every sample in it is still tested
__device__ __forceinline__ void grid_range(const Axis& a, int p, float size, int& lo, int& hi) {
    lo = 0; hi = a.grid;
    const float step = a.bin / (float)a.grid;
    if (a.grid <= kDenseGrid || !(step > 0.0f)) return;
    const float base = a.start + (float)p * a.bin;
    float u = floorf((-1.0f - base) / step - 0.5f), v = ceilf((size - base) / step - 0.5f);
    u -= 2.0f + fabsf(u) * 1e-5f;
    v += 2.0f + fabsf(v) * 1e-5f;
    lo = (int)fminf(fmaxf(u, 0.0f), (float)a.grid);
    hi = (int)fminf(fmaxf(v, 0.0f), (float)a.grid);
}

// sample i of bin p: false when it lies further than 1 px outside, else the two pixels and their weights (mmcv's bilinear_interpolate, one axis)
__device__ __forceinline__ bool axis_sample(const Axis& a, int p, int i, int64_t size, int64_t& lo, int64_t& hi, float& wl, float& wh) {
    float v = (a.start + (float)p * a.bin) + ((float)i + 0.5f) * a.bin / (float)a.grid;
    if (!(v >= -1.0f && v <= (float)size)) return false;      // NaN lands here too
    if (v <= 0.0f) v = 0.0f;
    lo = (int64_t)v;
    if (lo >= size - 1) { hi = lo = size - 1; v = (float)lo; } else hi = lo + 1;
    wh = v - (float)lo;       // the weight of hi
    wl = 1.0f - wh;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------- RoIAlign forward
__global__ void __launch_bounds__(kThreads) roialign_fwd_kernel(Levels L, Geom g, const float* __restrict__ rois, const int32_t* __restrict__ level_in,
                                                                const int64_t* __restrict__ valid, float* __restrict__ out,
                                                                int32_t* __restrict__ level_out) {
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int PP = g.P * g.P;
    int64_t image;
    const bool ok = roi_in_use(g, rois, valid, r, image);      // the same for the whole workgroup
    const float* roi = rois + r * 5;
    int l = level_in ? level_in[r] : roi_level(roi, g.finest, L.n);
    l = l < 0 ? 0 : (l >= L.n ? L.n - 1 : l);
    if (tid == 0 && level_out) level_out[r] = ok ? l : -1;
    float* o = out + r * PP * g.C;
    if (!ok) {
        for (int64_t i = tid; i < PP * g.C; i += kThreads) o[i] = 0.0f;
        return;
    }
    const Level& v = L.lv[l];
    const Axis ay = make_axis(roi[2], roi[4], v.scale, g.P, g.sampling, g.aligned), ax = make_axis(roi[1], roi[3], v.scale, g.P, g.sampling, g.aligned);
    const float count = grid_count(ay, ax);
    const float* plane = v.map + image * v.st[0];
    for (int64_t i = tid; i < PP * g.C; i += kThreads) {
        const int64_t bin = i / g.C, c = i - bin * g.C;
        const int ph = (int)(bin / g.P), pw = (int)(bin % g.P);
        const float* base = plane + c * v.st[1];
        int y0, y1, x0, x1;
        grid_range(ay, ph, (float)v.H, y0, y1);
        grid_range(ax, pw, (float)v.W, x0, x1);
        float acc = 0.0f;
        for (int iy = y0; iy < y1; ++iy) {
            int64_t yl, yh;
            float ly, hy;      // hy: the weight of the low row
            if (!axis_sample(ay, ph, iy, v.H, yl, yh, hy, ly)) continue;
            for (int ix = x0; ix < x1; ++ix) {
                int64_t xl, xh;
                float lx, hx;
                if (!axis_sample(ax, pw, ix, v.W, xl, xh, hx, lx)) continue;
                const float v1 = base[yl * v.st[2] + xl * v.st[3]], v2 = base[yl * v.st[2] + xh * v.st[3]];
                const float v3 = base[yh * v.st[2] + xl * v.st[3]], v4 = base[yh * v.st[2] + xh * v.st[3]];
                acc += (((hy * hx) * v1 + (hy * lx) * v2) + (ly * hx) * v3) + (ly * lx) * v4;
            }
        }
        o[i] = acc / count;
    }
}

// ------------------------------------------------------------------------------------------------------------------- RoIAlign backward
// sum over the samples of bin p of the weight they put on pixel `at` of this axis
__device__ __forceinline__ float axis_weight(const Axis& a, int p, int64_t size, int64_t at) {
    int i0, i1;
    grid_range(a, p, (float)size, i0, i1);
    float w = 0.0f;
    for (int i = i0; i < i1; ++i) {
        int64_t lo, hi;
        float wl, wh;
        if (!axis_sample(a, p, i, size, lo, hi, wl, wh)) continue;
        if (lo == at) w += wl;
        if (hi == at) w += wh;
    }
    return w;
}

// grid (ceil(pixels / 4), ceil(C / 256)): wave w of a workgroup owns pixel blockIdx.x * 4 + w in (level, image, y, x) order, lane c the channels
// blockIdx.y * 256 + c + 64 k, k < 4 (the walk over the RoIs and the weights are paid once per 256 channels).  Every lane stays in the loop (the
// shuffles need the whole wave); channels past C only skip the loads and the store.
__global__ void __launch_bounds__(kThreads) roialign_bwd_kernel(Levels L, Geom g, const float* __restrict__ dout, const float* __restrict__ rois,
                                                                const int32_t* __restrict__ level_in, const int64_t* __restrict__ valid, int accumulate) {
    const int lane = threadIdx.x % MTP_WAVE;
    const int64_t key = (int64_t)blockIdx.x * (kThreads / MTP_WAVE) + threadIdx.x / MTP_WAVE;      // the same for the whole wave
    const int64_t c = (int64_t)blockIdx.y * (kLaneChannels * MTP_WAVE) + lane;
    if (key >= L.pixels) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < kL; ++k)
        if (k < L.n && key >= L.lv[k].first) l = k;
    const Level& v = L.lv[l];
    const int64_t local = key - v.first, px = local % v.W, py = (local / v.W) % v.H, image = local / (v.W * v.H);
    const float fy = (float)py, fx = (float)px;
    const int P = g.P;
    float acc[kLaneChannels] = {};
    // 64 RoIs at a time: lane i tests RoI r0 + i (in use, this image, this level, within a pixel of (py, px)); the wave then takes the hits in
    // index order, so the sum has the order of a plain walk over r
    for (int64_t r0 = 0; r0 < g.R; r0 += MTP_WAVE) {
        const int64_t rl = r0 + lane;
        bool hit = false;
        if (rl < g.R) {
            int64_t im;
            if (roi_in_use(g, rois, valid, rl, im) && im == image) {
                const float* roi = rois + rl * 5;
                int lr = level_in ? level_in[rl] : roi_level(roi, g.finest, L.n);
                lr = lr < 0 ? 0 : (lr >= L.n ? L.n - 1 : lr);
                if (lr == l) {
                    const Axis ay = make_axis(roi[2], roi[4], v.scale, P, g.sampling, g.aligned), ax = make_axis(roi[1], roi[3], v.scale, P, g.sampling, g.aligned);
                    // false: no sample of this RoI comes within a pixel of (py, px); NaN geometry is not rejected here and adds nothing below
                    const float ya = ay.start, yb = ay.start + ay.bin * (float)P, xa = ax.start, xb = ax.start + ax.bin * (float)P;
                    hit = !(fy < fminf(ya, yb) - 1.0f || fy > fmaxf(ya, yb) + 1.0f || fx < fminf(xa, xb) - 1.0f || fx > fmaxf(xa, xb) + 1.0f);
                }
            }
        }
        unsigned long long hits = __ballot(hit);      // the same for the whole wave
        while (hits) {
            const int64_t r = r0 + (__ffsll((long long)hits) - 1);
            hits &= hits - 1;
            const float* roi = rois + r * 5;
            const Axis ay = make_axis(roi[2], roi[4], v.scale, P, g.sampling, g.aligned), ax = make_axis(roi[1], roi[3], v.scale, P, g.sampling, g.aligned);
            float w = 0.0f;
            if (lane < P) w = axis_weight(ay, lane, v.H, py);
            else if (lane >= 32 && lane < 32 + P) w = axis_weight(ax, lane - 32, v.W, px);
            const float count = grid_count(ay, ax);
            const float* d = dout + r * P * P * g.C;
            for (int i = 0; i < P; ++i) {
                const float wy = __shfl(w, i, MTP_WAVE);
                if (wy == 0.0f) continue;
                for (int j = 0; j < P; ++j) {
                    const float wx = __shfl(w, 32 + j, MTP_WAVE);
                    if (wx == 0.0f) continue;
                    const float* dj = d + (int64_t)(i * P + j) * g.C;
#pragma unroll
                    for (int k = 0; k < kLaneChannels; ++k)
                        if (c + k * MTP_WAVE < g.C) acc[k] += (wy * wx) * (dj[c + k * MTP_WAVE] / count);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kLaneChannels; ++k) {
        const int64_t ck = c + k * MTP_WAVE;
        if (ck >= g.C) break;
        float* dst = v.dmap + image * v.st[0] + ck * v.st[1] + py * v.st[2] + px * v.st[3];
        *dst = accumulate ? *dst + acc[k] : acc[k];
    }
}

// ------------------------------------------------------------------------------------------------------------------- mask targets and loss
struct MaskLoss {
    const float* logits;        // (B S, Kc, M, M): Kc >= K channels, of which the labels name the first K
    const float* boxes;         // (B S, 4)
    const int64_t* labels;      // (B S) or null: channel 0
    const int64_t* sample_gt;   // (B, S) rows of bitmaps
    const int64_t* n_pos;       // (B)
    const uint8_t* bitmaps;     // (G, H, W)
    const int64_t* img_hw;      // (B, 2) or null: H, W
    int64_t B, S, K, Kc, G, H, W;
    int M;
};

__device__ __forceinline__ int64_t positives(const MaskLoss& a, int64_t b) {
    const int64_t n = a.n_pos[b];
    return n < 0 ? 0 : (n > a.S ? a.S : n);
}
__device__ __forceinline__ int64_t total_positives(const MaskLoss& a) {
    int64_t t = 0;
    for (int64_t b = 0; b < a.B; ++b) t += positives(a, b);
    return t;
}

// grid (B S); slot_loss[slot] = the sum of the slot's M M cross-entropies (0 on a slot that is not positive)
__global__ void __launch_bounds__(kThreads) mask_loss_kernel(MaskLoss a, float weight, uint8_t* __restrict__ targets, float* __restrict__ target_avg,
                                                             float* __restrict__ slot_loss, float* __restrict__ dlogits) {
    __shared__ float wsum[kThreads / MTP_WAVE];
    __shared__ int64_t s_total;
    const int tid = threadIdx.x;
    const int64_t slot = blockIdx.x, b = slot / a.S, j = slot - b * a.S;
    if (tid == 0) s_total = total_positives(a);
    __syncthreads();
    const int64_t total = s_total;
    const int MM = a.M * a.M;
    int64_t gt = j < positives(a, b) ? a.sample_gt[slot] : -1;
    int64_t ch = a.labels ? a.labels[slot] : 0;
    const bool pos = gt >= 0 && gt < a.G && ch >= 0 && ch < a.K;      // the same for the whole workgroup
    if (!pos) ch = -1;
    int64_t h = a.H, w = a.W;
    if (a.img_hw) {
        h = a.img_hw[b * 2]; w = a.img_hw[b * 2 + 1];
        h = h < 1 ? 1 : (h > a.H ? a.H : h);
        w = w < 1 ? 1 : (w > a.W ? a.W : w);
    }
    Axis ay = {}, ax = {};
    float count = 1.0f;
    if (pos) {
        const float* box = a.boxes + slot * 4;      // mask_target_single: np.clip to the gt's image (a NaN stays a NaN, and samples nothing)
        const float x1 = fminf(fmaxf(box[0], 0.0f), (float)w), x2 = fminf(fmaxf(box[2], 0.0f), (float)w);
        const float y1 = fminf(fmaxf(box[1], 0.0f), (float)h), y2 = fminf(fmaxf(box[3], 0.0f), (float)h);
        ay = make_axis(box[1] != box[1] ? box[1] : y1, box[3] != box[3] ? box[3] : y2, 1.0f, a.M, 0, 1);
        ax = make_axis(box[0] != box[0] ? box[0] : x1, box[2] != box[2] ? box[2] : x2, 1.0f, a.M, 0, 1);
        count = grid_count(ay, ax);
    }
    const float gscale = total > 0 ? weight / ((float)total * (float)MM) : 0.0f;
    const uint8_t* bm = a.bitmaps + (pos ? gt : 0) * a.H * a.W;
    float loss = 0.0f;
    for (int i = tid; i < MM; i += kThreads) {
        float avg = 0.0f;
        if (pos) {
            const int ph = i / a.M, pw = i % a.M;
            int y0, y1, x0, x1;
            grid_range(ay, ph, (float)h, y0, y1);
            grid_range(ax, pw, (float)w, x0, x1);
            float acc = 0.0f;
            for (int iy = y0; iy < y1; ++iy) {
                int64_t yl, yh;
                float ly, hy;
                if (!axis_sample(ay, ph, iy, h, yl, yh, hy, ly)) continue;
                for (int ix = x0; ix < x1; ++ix) {
                    int64_t xl, xh;
                    float lx, hx;
                    if (!axis_sample(ax, pw, ix, w, xl, xh, hx, lx)) continue;
                    const float v1 = (float)bm[yl * a.W + xl], v2 = (float)bm[yl * a.W + xh], v3 = (float)bm[yh * a.W + xl], v4 = (float)bm[yh * a.W + xh];
                    acc += (((hy * hx) * v1 + (hy * lx) * v2) + (ly * hx) * v3) + (ly * lx) * v4;
                }
            }
            avg = acc / count;
        }
        const float t = avg >= 0.5f ? 1.0f : 0.0f;
        targets[slot * MM + i] = (uint8_t)t;
        if (target_avg) target_avg[slot * MM + i] = avg;
        for (int64_t k = 0; k < a.Kc; ++k) {
            const int64_t e = (slot * a.Kc + k) * MM + i;
            float d = 0.0f;
            if (k == ch) {
                const float z = a.logits[e], en = expf(-fabsf(z));
                loss += (fmaxf(z, 0.0f) - z * t) + log1pf(en);
                const float sg = z >= 0.0f ? 1.0f / (1.0f + en) : en / (1.0f + en);
                d = (sg - t) * gscale;
            }
            if (dlogits) dlogits[e] = d;
        }
    }
    const float s = wave_sum(loss);
    if (tid % MTP_WAVE == 0) wsum[tid / MTP_WAVE] = s;
    __syncthreads();
    if (tid == 0) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < kThreads / MTP_WAVE; ++k) t += wsum[k];
        slot_loss[slot] = t;
    }
}

// lane i adds slots i, i + 64, ... in order, then the butterfly: a fixed order
__global__ void __launch_bounds__(MTP_WAVE) mask_loss_sum_kernel(MaskLoss a, float weight, const float* __restrict__ slot_loss, float* __restrict__ out) {
    float s = 0.0f;
    for (int64_t i = threadIdx.x; i < a.B * a.S; i += MTP_WAVE) s += slot_loss[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        const int64_t total = total_positives(a);
        out[0] = total > 0 ? s / ((float)total * (float)(a.M * a.M)) * weight : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------------- mask paste
// one axis of _do_paste_mask + grid_sample(align_corners=False): pixel centre -> normalised -> source coordinate; inf -> 0 as the reference
__device__ __forceinline__ float paste_coord(int64_t p, float a, float b, int M) {
    float n = (((float)p + 0.5f) - a) / (b - a) * 2.0f - 1.0f;
    if (isinf(n)) n = 0.0f;
    return ((n + 1.0f) * (float)M - 1.0f) / 2.0f;
}

__global__ void __launch_bounds__(kThreads) mask_paste_kernel(const float* __restrict__ logits, int64_t K, int M, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ boxes, int64_t N, int64_t img_h, int64_t img_w, float threshold,
                                                              int activate, uint8_t* __restrict__ out, float* __restrict__ values) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= N * img_h * img_w) return;
    const int64_t n = e / (img_h * img_w), rem = e - n * img_h * img_w, y = rem / img_w, x = rem - y * img_w;
    int64_t ch = labels ? labels[n] : 0;
    const float* box = boxes + n * 4;
    const float sx = paste_coord(x, box[0], box[2], M), sy = paste_coord(y, box[1], box[3], M);
    float val;
    if (ch < 0 || ch >= K) {              // no such channel: an empty mask whatever the threshold
        out[e] = 0;
        if (values) values[e] = 0.0f;
        return;
    } else if (sx != sx || sy != sy) {
        val = sx + sy;                    // 0 / 0 in the box mapping: the reference's value is a NaN, which is below every threshold
    } else {
        const float* m = logits + (n * K + ch) * M * M;
        const float fx0 = floorf(sx), fy0 = floorf(sy);
        const float wx1 = sx - fx0, wx0 = (fx0 + 1.0f) - sx, wy1 = sy - fy0, wy0 = (fy0 + 1.0f) - sy;
        // far outside: every corner is padding (and the casts below stay in range)
        const bool far = !(fx0 >= -2.0f && fx0 <= (float)M + 1.0f && fy0 >= -2.0f && fy0 <= (float)M + 1.0f);
        const int x0 = far ? -2 : (int)fx0, y0 = far ? -2 : (int)fy0;
        float corner[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
            float p = 0.0f;
            if (cx >= 0 && cx < M && cy >= 0 && cy < M) {
                const float z = m[cy * M + cx];
                if (activate) {
                    const float en = expf(-fabsf(z));
                    p = z >= 0.0f ? 1.0f / (1.0f + en) : en / (1.0f + en);
                } else {
                    p = z;
                }
            }
            corner[k] = p;
        }
        val = ((corner[0] * (wx0 * wy0) + corner[1] * (wx1 * wy0)) + corner[2] * (wx0 * wy1)) + corner[3] * (wx1 * wy1);
    }
    if (values) values[e] = val;
    if (threshold >= 0.0f) {
        out[e] = val >= threshold ? 1 : 0;
    } else {
        const float s = val * 255.0f;
        out[e] = s >= 0.0f ? (uint8_t)fminf(s, 255.0f) : 0;      // NaN -> 0
    }
}

bool make_geom(int64_t images, int64_t C, int64_t R, int64_t per_group, const int64_t* valid, int out_size, int sampling_ratio, int aligned,
               float finest_scale, Geom& g) {
    if (C < 1 || C > (1 << 20) || R < 1 || R > (1 << 24) || out_size < 1 || out_size > kMaxOut || sampling_ratio < 0 || sampling_ratio > kMaxSampling) return false;
    if (!(finest_scale > 0.0f)) return false;
    if (valid && (per_group < 1 || R % per_group)) return false;
    g.P = out_size; g.sampling = sampling_ratio; g.aligned = aligned ? 1 : 0; g.finest = finest_scale;
    g.images = images; g.C = C; g.R = R; g.per_group = valid ? per_group : R;
    return true;
}

}  // namespace

// ======================================================================================================================== C ABI
extern "C" int mtp_roi_align_fwd(const mtp_roi_level* levels, int num_levels, int64_t images, int64_t C, const float* rois, const int32_t* roi_levels,
                                 const int64_t* valid, int64_t R, int64_t per_group, int out_size, int sampling_ratio, int aligned, float finest_scale,
                                 float* out, int32_t* levels_out, mtp_stream_t stream) {
    MTP_CHECK_ARG(rois && out);
    Levels L;
    Geom g;
    MTP_CHECK_ARG(make_levels(levels, num_levels, images, 1, L) && make_geom(images, C, R, per_group, valid, out_size, sampling_ratio, aligned, finest_scale, g));
    roialign_fwd_kernel<<<(unsigned)R, kThreads, 0, (hipStream_t)stream>>>(L, g, rois, roi_levels, valid, out, levels_out);
    return mtp_launch_status();
}

extern "C" int mtp_roi_align_bwd(const mtp_roi_level* levels, int num_levels, int64_t images, int64_t C, const float* dout, const float* rois,
                                 const int32_t* roi_levels, const int64_t* valid, int64_t R, int64_t per_group, int out_size, int sampling_ratio,
                                 int aligned, float finest_scale, int accumulate, mtp_stream_t stream) {
    MTP_CHECK_ARG(rois && dout);
    Levels L;
    Geom g;
    MTP_CHECK_ARG(make_levels(levels, num_levels, images, 2, L) && make_geom(images, C, R, per_group, valid, out_size, sampling_ratio, aligned, finest_scale, g));
    const int64_t bx = (L.pixels + kThreads / MTP_WAVE - 1) / (kThreads / MTP_WAVE), by = (C + kLaneChannels * MTP_WAVE - 1) / (kLaneChannels * MTP_WAVE);
    MTP_CHECK_ARG(bx < ((int64_t)1 << 31) && by <= 65535);
    roialign_bwd_kernel<<<dim3((unsigned)bx, (unsigned)by), kThreads, 0, (hipStream_t)stream>>>(L, g, dout, rois, roi_levels, valid, accumulate);
    return mtp_launch_status();
}

extern "C" int mtp_mask_loss(const float* mask_preds, int64_t num_classes, int64_t channels, int mask_size, const float* boxes, const int64_t* labels,
                             const int64_t* sample_gt, const int64_t* n_pos, int64_t images, int64_t S, const uint8_t* bitmaps, int64_t num_gts,
                             int64_t H, int64_t W, const int64_t* img_hw, float loss_weight, uint8_t* targets, float* target_avg, float* slot_loss,
                             float* loss, float* dlogits, mtp_stream_t stream) {
    MTP_CHECK_ARG(mask_preds && boxes && sample_gt && n_pos && targets && slot_loss && loss && images > 0 && S > 0 && images * S < ((int64_t)1 << 24));
    MTP_CHECK_ARG(num_classes >= 1 && channels >= num_classes && channels < (1 << 16) && mask_size >= 1 && mask_size <= 1024 && num_gts >= 0 && (bitmaps || num_gts == 0));
    MTP_CHECK_ARG(H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20));
    const MaskLoss a = {mask_preds, boxes, labels, sample_gt, n_pos, bitmaps, img_hw, images, S, num_classes, channels, num_gts, H, W, mask_size};
    hipStream_t s = (hipStream_t)stream;
    mask_loss_kernel<<<(unsigned)(images * S), kThreads, 0, s>>>(a, loss_weight, targets, target_avg, slot_loss, dlogits);
    mask_loss_sum_kernel<<<1, MTP_WAVE, 0, s>>>(a, loss_weight, slot_loss, loss);
    return mtp_launch_status();
}

extern "C" int mtp_mask_paste(const float* mask_preds, int64_t num_classes, int mask_size, const int64_t* labels, const float* boxes, int64_t N,
                              int64_t img_h, int64_t img_w, float threshold, int activate, uint8_t* out, float* values, mtp_stream_t stream) {
    MTP_CHECK_ARG(mask_preds && boxes && out && N > 0 && img_h > 0 && img_w > 0 && img_h <= (1 << 20) && img_w <= (1 << 20));
    MTP_CHECK_ARG(num_classes >= 1 && num_classes < (1 << 16) && mask_size >= 1 && mask_size <= 1024 && threshold == threshold);
    MTP_CHECK_ARG(N < ((int64_t)1 << 24) && N * img_h * img_w < ((int64_t)1 << 38));
    mask_paste_kernel<<<blocks_exact(N * img_h * img_w), kThreads, 0, (hipStream_t)stream>>>(mask_preds, num_classes, mask_size, labels, boxes, N, img_h,
                                                                                            img_w, threshold, activate, out, values);
    return mtp_launch_status();
}
