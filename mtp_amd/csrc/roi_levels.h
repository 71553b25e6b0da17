// The pyramid levels of the RoI operators (csrc/roi_head.hip, csrc/mask_head.hip): mtp_roi_level as the kernels take it.  A level's map is addressed by
// element strides (image, channel, y, x); `first` is the level's first pixel in the key order (level, image, y, x) and `pixels` the number of pixels of
// all levels and images.  One definition, so that both files agree on the order of the pixels and on what a valid level is.
#pragma once
#include "common.h"

namespace {

constexpr int kL = MTP_ROI_MAX_LEVELS;

struct Level {
    const float* map;
    float* dmap;
    int64_t H, W, first;
    int64_t st[4];
    float scale;
};
struct Levels {
    Level lv[kL];
    int n;
    int64_t pixels;
};

// need: 0 the geometry alone, 1 the maps, 2 the gradient maps
inline bool make_levels(const mtp_roi_level* levels, int n, int64_t images, int need, Levels& L) {
    if (!levels || n < 1 || n > kL || images < 1 || images > (1 << 20)) return false;
    int64_t first = 0;
    for (int i = 0; i < n; ++i) {
        const mtp_roi_level& s = levels[i];
        if ((need == 1 && !s.map) || (need == 2 && !s.dmap) || s.H < 1 || s.W < 1 || s.H > (1 << 20) || s.W > (1 << 20) || !(s.spatial_scale > 0.0f)) return false;
        Level& d = L.lv[i];
        d.map = s.map; d.dmap = s.dmap; d.H = s.H; d.W = s.W; d.first = first; d.scale = s.spatial_scale;
        for (int c = 0; c < 4; ++c) {
            if (s.stride[c] < 0) return false;
            d.st[c] = s.stride[c];
        }
        first += images * s.H * s.W;
    }
    for (int i = n; i < kL; ++i) L.lv[i] = L.lv[n - 1];
    L.n = n;
    L.pixels = first;
    return true;
}

}  // namespace
