// The rotated-box intersection shared by box_ops.hip (IoU, NMS, assignment) and det_eval.hip (the DOTA metric's matching): one text, so that both
// files give the same IoU bits for a pair.  Box A is moved into B's frame (both centres first translated to B's centre: no cancellation at large
// coordinates), clipped against B's four axis-parallel half planes (Sutherland-Hodgman, at most 8 vertices), shoelace area.  Every including file
// compiles this with contraction off: each product and sum rounds once, in the written order, and tests/box_ref.py restates the same operations.
#pragma once
#include "common.h"

// honoured under hipcc's default -ffp-contract=fast-honor-pragmas; a build that forces -ffp-contract=fast ignores it
#pragma clang fp contract(off)

namespace {

struct RBox {
    float cx, cy, hw, hh, c, s, area;
};

__device__ __forceinline__ RBox load_rbox(const float* p) {
    RBox b;
    b.cx = p[0]; b.cy = p[1];
    b.hw = p[2] * 0.5f; b.hh = p[3] * 0.5f;
    sincosf(p[4], &b.s, &b.c);
    b.area = p[2] * p[3];
    return b;
}

// one Sutherland-Hodgman pass: keep SIGN * coordinate[AXIS] <= bound.  The crossing point is put exactly on the plane.  At most 8 vertices.
template <int AXIS, int SIGN>
__device__ __forceinline__ int clip_plane(const float* ix, const float* iy, int n, float* ox, float* oy, float bound) {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < n) {
            const int j = i + 1 < n ? i + 1 : 0;
            const float px = ix[i], py = iy[i], qx = ix[j], qy = iy[j];
            const float dp = (float)SIGN * (AXIS ? py : px) - bound, dq = (float)SIGN * (AXIS ? qy : qx) - bound;
            const bool pin = dp <= 0.0f, qin = dq <= 0.0f;
            if (pin && m < 8) {
                ox[m] = px; oy[m] = py;
                ++m;
            }
            if (pin != qin && m < 8) {
                const float t = dp / (dp - dq);
                float x = px + t * (qx - px), y = py + t * (qy - py);
                if (AXIS) y = (float)SIGN * bound;
                else x = (float)SIGN * bound;
                ox[m] = x; oy[m] = y;
                ++m;
            }
        }
    }
    return m;
}

__device__ __forceinline__ float rbox_intersection(const RBox& a, const RBox& b) {
    const float dx = a.cx - b.cx, dy = a.cy - b.cy;
    const float ox = dx * b.c + dy * b.s, oy = dy * b.c - dx * b.s;              // a's centre in b's frame
    const float cp = a.c * b.c + a.s * b.s, sp = a.s * b.c - a.c * b.s;          // cos / sin of (theta_a - theta_b)
    const float ux = a.hw * cp, uy = a.hw * sp, vx = -(a.hh * sp), vy = a.hh * cp;
    float px[8], py[8], qx[8], qy[8];
    px[0] = (ox - ux) - vx; py[0] = (oy - uy) - vy;
    px[1] = (ox + ux) - vx; py[1] = (oy + uy) - vy;
    px[2] = (ox + ux) + vx; py[2] = (oy + uy) + vy;
    px[3] = (ox - ux) + vx; py[3] = (oy - uy) + vy;
    int n = clip_plane<0, 1>(px, py, 4, qx, qy, b.hw);
    n = clip_plane<0, -1>(qx, qy, n, px, py, b.hw);
    n = clip_plane<1, 1>(px, py, n, qx, qy, b.hh);
    n = clip_plane<1, -1>(qx, qy, n, px, py, b.hh);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < n) {
            const int j = i + 1 < n ? i + 1 : 0;
            acc += px[i] * py[j] - px[j] * py[i];
        }
    }
    return 0.5f * fabsf(acc);
}

__device__ __forceinline__ float box_iou(const RBox& a, const RBox& b, int iof, float /*eps*/) {
    if (a.area < 1e-14f || b.area < 1e-14f) return 0.0f;
    const float inter = rbox_intersection(a, b);
    const float base = iof ? a.area : (a.area + b.area) - inter;
    return inter / base;
}

}  // namespace
