// The bilinear index rule shared by every kernel that interpolates (decode_head.hip: resize, segmentation loss; seg_eval.hip: window accumulate).
#pragma once
#include "common.h"

// F.interpolate(mode='bilinear', align_corners=False) index rule (ATen area_pixel_compute_source_index): src = max(scale * (o + 0.5) - 0.5, 0),
// scale = in / out, i0 = (int)src, i1 = i0 + (i0 < in - 1), weights (1 - l, l) with l = src - i0.
struct Lin {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Lin lin_index(int o, int in, float scale) {
    float src = scale * ((float)o + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    Lin L;
    L.i0 = (int)src;
    if (L.i0 > in - 1) L.i0 = in - 1;
    L.i1 = L.i0 + (L.i0 < in - 1 ? 1 : 0);
    L.w1 = src - (float)L.i0;
    L.w0 = 1.0f - L.w1;
    return L;
}
