// The pyramid levels of the RPN kernels (csrc/rpn.hip, csrc/hbox_head.hip): mtp_rpn_level as the kernels take it.  The maps are addressed by element
// strides (image, channel, y, x); `first` is the level's first anchor in the flat multi-level order (level, y, x, a), `count` its H W A anchors and
// `keep_first` its first column of the kept list.  One definition, so that both heads agree on the anchor order and on what a valid level is.
#pragma once
#include "common.h"

namespace {

constexpr int kL = MTP_RPN_MAX_LEVELS;

struct Level {
    const float* cls;
    const float* reg;
    float* dcls;
    float* dreg;
    int64_t H, W, first, count, keep_first;
    int64_t cs[4], rs[4];
};
struct Levels {
    Level lv[kL];
    int n;
};

__device__ __forceinline__ int level_of(const Levels& L, int64_t idx) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < kL; ++i)
        if (i < L.n && idx >= L.lv[i].first) l = i;
    return l;
}

// the levels tile the flat anchor order without gaps; every map pointer is there, the gradient maps both or neither on every level
inline bool make_levels(const mtp_rpn_level* levels, int n, int64_t A, int64_t total, bool keeps, Levels& L, int64_t& T) {
    if (!levels || n < 1 || n > kL || A < 1 || A > (1 << 16) || total < 1) return false;
    int64_t first = 0;
    T = 0;
    const bool grads = levels[0].dcls != nullptr;
    for (int i = 0; i < n; ++i) {
        const mtp_rpn_level& s = levels[i];
        if (!s.cls || !s.reg || s.H < 1 || s.W < 1 || s.H > (1 << 20) || s.W > (1 << 20)) return false;
        if ((s.dcls != nullptr) != grads || (s.dreg != nullptr) != grads) return false;
        Level& d = L.lv[i];
        d.cls = s.cls; d.reg = s.reg; d.dcls = s.dcls; d.dreg = s.dreg;
        d.H = s.H; d.W = s.W; d.first = first; d.count = s.H * s.W * A;
        d.keep_first = T;
        if (keeps && (s.keep_count < 0 || s.keep_count > d.count)) return false;
        for (int c = 0; c < 4; ++c) {
            if (s.cls_stride[c] < 0 || s.reg_stride[c] < 0) return false;
            d.cs[c] = s.cls_stride[c];
            d.rs[c] = s.reg_stride[c];
        }
        first += d.count;
        T += keeps ? s.keep_count : 0;
    }
    for (int i = n; i < kL; ++i) L.lv[i] = L.lv[n - 1];
    L.n = n;
    return first == total;
}

}  // namespace
