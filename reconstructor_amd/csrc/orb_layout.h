// orb_layout.h -- the host side of the ORB stage's geometry (csrc/orb.hip): option defaults and ranges, the pattern check, level
// sizes, offsets and cv::ORB's keypoint quotas.  Pure C++ over include/rcn.h, no device code, so that tests/cpp/orb_host_test.cpp
// can run it alone under the address and undefined-behaviour sanitizers.  The float arithmetic of the quotas and the float64
// division of the level sizes are part of the contract (tests/orb_ref.py::layout): build without contraction.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rcn.h"

namespace {

constexpr int ORB_HALF = 15;
// half widths of the rows of the circular patch of radius 15, as OpenCV builds them (tests/orb_ref.py::umax_table)
#define ORB_UMAX_INIT {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3}
[[maybe_unused]] constexpr int ORB_UMAX_HOST[16] = ORB_UMAX_INIT;
// the 7 taps of the blur: rint(256 g / sum g) of the fp64 Gaussian of sigma 2, half to even, the centre taking the remainder
[[maybe_unused]] constexpr int ORB_BLUR_W[7] = {18, 34, 49, 54, 49, 34, 18};

inline void orb_defaults(rcn_orb_options *opt)
{
    opt->nfeatures = 500;
    opt->nlevels = 8;
    opt->edge_threshold = 31;
    opt->fast_threshold = 20;
    opt->scale_factor = 1.2;
    opt->pattern = nullptr;
}

inline const char *orb_pattern_check(const int8_t *p)
{
    if (!p) return nullptr;
    for (int i = 0; i < 1024; ++i) if (p[i] > ORB_HALF || p[i] < -ORB_HALF) return "pattern coordinate beyond +-15";
    return nullptr;
}

inline const char *orb_layout_fill(int32_t H, int32_t W, const rcn_orb_options *opt, rcn_orb_pyramid_layout *L, rcn_orb_options *use)
{
    rcn_orb_options d;
    orb_defaults(&d);
    if (opt) d = *opt;
    if (use) *use = d;
    if (d.nfeatures < 1) return "nfeatures < 1";
    if (d.nlevels < 1 || d.nlevels > RCN_ORB_MAX_LEVELS) return "nlevels outside 1..16";
    if (d.edge_threshold < 22 || d.edge_threshold > 4096) return "edge_threshold outside 22..4096";
    if (d.fast_threshold < 1 || d.fast_threshold > 254) return "fast_threshold outside 1..254";
    if (!(d.scale_factor > 1.0) || !(d.scale_factor <= 4.0)) return "scale_factor outside (1, 4]";
    if (const char *why = orb_pattern_check(d.pattern)) return why;
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (int64_t)H * W > 0x7FFFFFFFll) return "image size out of range (1..65535 a side, H W <= 2^31 - 1)";
    std::memset(L, 0, sizeof *L);
    L->n_levels = d.nlevels;
    int64_t off = 0;
    for (int l = 0; l < d.nlevels; ++l) {
        const float s = (float)std::pow(d.scale_factor, (double)l);
        L->scale[l] = s;
        L->level_h[l] = (int32_t)std::nearbyint((double)H / (double)s);
        L->level_w[l] = (int32_t)std::nearbyint((double)W / (double)s);
        if (L->level_h[l] < 1 || L->level_w[l] < 1) return "a level is empty";
        if (l && L->level_h[l - 1] == 2 * L->level_h[l] && L->level_w[l - 1] == 2 * L->level_w[l]) return "a level halves the one before it on both axes";
        L->active[l] = std::min(L->level_h[l], L->level_w[l]) > 2 * d.edge_threshold;
        L->level_offset[l] = off;
        off += ((int64_t)L->level_h[l] * L->level_w[l] + 15) & ~(int64_t)15;
    }
    L->bytes_per_image = off;
    // cv::ORB's split, in float as there
    const float f = (float)(1.0 / d.scale_factor);
    float nd = (float)d.nfeatures * (1.f - f) / (1.f - (float)std::pow((double)f, (double)d.nlevels));
    int total = 0;
    for (int l = 0; l < d.nlevels - 1; ++l) {
        L->quota[l] = (int32_t)std::nearbyint((double)nd);
        total += L->quota[l];
        nd *= f;
    }
    L->quota[d.nlevels - 1] = std::max(d.nfeatures - total, 0);
    return nullptr;
}

}  // namespace
