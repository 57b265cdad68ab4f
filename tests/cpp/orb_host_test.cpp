// Host-only check of the ORB stage's geometry (reconstructor_amd/csrc/orb_layout.h, orb_pattern.h) for tests/test_orb_host.py:
// built as an executable of its own with the address and undefined-behaviour sanitizers.  Every expectation is derived here from
// the inputs: level sizes from the division, offsets from the sizes, the quota sum, the tables from their formulas.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../reconstructor_amd/csrc/orb_layout.h"
#include "../../reconstructor_amd/csrc/orb_pattern.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static void layout_case(int H, int W, int nfeatures, int nlevels, double sf, int edge)
{
    rcn_orb_options o;
    orb_defaults(&o);
    o.nfeatures = nfeatures; o.nlevels = nlevels; o.scale_factor = sf; o.edge_threshold = edge;
    rcn_orb_pyramid_layout L;
    rcn_orb_options use;
    const char *why = orb_layout_fill(H, W, &o, &L, &use);
    if (why) { std::printf("FAIL %d x %d: %s\n", H, W, why); ++failures; return; }
    CHECK(L.n_levels == nlevels && use.nfeatures == nfeatures);
    CHECK(L.level_h[0] == H && L.level_w[0] == W && L.scale[0] == 1.f && L.level_offset[0] == 0);
    long long off = 0, sum = 0;
    for (int l = 0; l < nlevels; ++l) {
        const double s = (double)L.scale[l];
        CHECK(std::fabs((double)H / s - L.level_h[l]) <= 0.5 && std::fabs((double)W / s - L.level_w[l]) <= 0.5);
        CHECK(L.level_offset[l] == off && off % 16 == 0);
        off += ((long long)L.level_h[l] * L.level_w[l] + 15) / 16 * 16;
        CHECK(L.active[l] == (L.level_h[l] > 2 * edge && L.level_w[l] > 2 * edge));
        CHECK(L.quota[l] >= 0);
        if (l) CHECK(L.scale[l] > L.scale[l - 1] && L.quota[l] <= L.quota[l - 1] + 1);
        sum += L.quota[l];
    }
    CHECK(L.bytes_per_image == off);
    CHECK(sum == nfeatures);
    for (int l = nlevels; l < RCN_ORB_MAX_LEVELS; ++l) CHECK(L.level_h[l] == 0 && L.quota[l] == 0 && L.level_offset[l] == 0);
}

int main()
{
    layout_case(96, 128, 500, 8, 1.2, 31);
    layout_case(97, 131, 500, 8, 1.2, 31);
    layout_case(480, 640, 500, 8, 1.2, 31);
    layout_case(200, 264, 24, 8, 1.2, 31);
    layout_case(300, 413, 1000, 16, 1.1, 22);
    layout_case(300, 413, 7, 3, 1.5, 40);
    layout_case(65535, 32767, 500, 1, 1.2, 31);
    layout_case(6, 6, 500, 8, 1.2, 31);

    rcn_orb_pyramid_layout L;
    rcn_orb_options o;
    auto refused = [&](int H, int W) { return orb_layout_fill(H, W, &o, &L, nullptr) != nullptr; };
    orb_defaults(&o);
    CHECK(!refused(96, 128) && refused(0, 128) && refused(96, 0) && refused(1, 1) && refused(2, 2) && refused(65536, 8) && refused(65535, 65535));
    orb_defaults(&o); o.nlevels = 0; CHECK(refused(96, 128));
    orb_defaults(&o); o.nlevels = RCN_ORB_MAX_LEVELS + 1; CHECK(refused(96, 128));
    orb_defaults(&o); o.nfeatures = 0; CHECK(refused(96, 128));
    orb_defaults(&o); o.edge_threshold = 21; CHECK(refused(96, 128));
    orb_defaults(&o); o.fast_threshold = 0; CHECK(refused(96, 128));
    orb_defaults(&o); o.fast_threshold = 255; CHECK(refused(96, 128));
    orb_defaults(&o); o.scale_factor = 1.0; CHECK(refused(96, 128));
    orb_defaults(&o); o.scale_factor = 2.0; CHECK(refused(96, 128));           // level 1 halves level 0
    orb_defaults(&o); o.scale_factor = std::nan(""); CHECK(refused(96, 128));

    // the built-in pattern and the pattern check
    CHECK(orb_pattern_check(nullptr) == nullptr && orb_pattern_check(orb_default_pattern_table) == nullptr);
    for (int t = 0; t < 256; ++t) {
        const int8_t *q = orb_default_pattern_table + 4 * t;
        for (int k = 0; k < 4; ++k) CHECK(q[k] >= -13 && q[k] <= 13);
        CHECK(q[0] != q[2] || q[1] != q[3]);
    }
    std::vector<int8_t> pat(orb_default_pattern_table, orb_default_pattern_table + 1024);
    for (int at : {0, 517, 1023}) for (int v : {16, -16, 127, -128}) {
        const int8_t keep = pat[(size_t)at];
        pat[(size_t)at] = (int8_t)v;
        CHECK(orb_pattern_check(pat.data()) != nullptr);
        orb_defaults(&o); o.pattern = pat.data(); CHECK(refused(96, 128));
        pat[(size_t)at] = keep;
    }
    pat[5] = 15; pat[6] = -15;
    CHECK(orb_pattern_check(pat.data()) == nullptr);

    // the tables against their formulas
    int umax[ORB_HALF + 2] = {0};
    const int vmax = (int)std::floor(ORB_HALF * std::sqrt(2.0) / 2 + 1), vmin = (int)std::ceil(ORB_HALF * std::sqrt(2.0) / 2);
    for (int v = 0; v <= vmax; ++v) umax[v] = (int)std::nearbyint(std::sqrt((double)(ORB_HALF * ORB_HALF - v * v)));
    for (int v = ORB_HALF, v0 = 0; v >= vmin; --v) { while (umax[v0] == umax[v0 + 1]) ++v0; umax[v] = v0; ++v0; }
    for (int v = 0; v <= ORB_HALF; ++v) CHECK(umax[v] == ORB_UMAX_HOST[v]);
    double g[7], gs = 0.0;
    for (int i = 0; i < 7; ++i) { g[i] = std::exp(-((i - 3) * (i - 3)) / 8.0); gs += g[i]; }
    int wsum = 0;
    for (int i = 0; i < 7; ++i) { if (i != 3) CHECK(ORB_BLUR_W[i] == (int)std::nearbyint(256.0 * g[i] / gs)); wsum += ORB_BLUR_W[i]; }
    CHECK(wsum == 256);

    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("all cases pass\n");
    return 0;
}
