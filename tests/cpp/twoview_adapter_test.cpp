// twoview_adapter_test -- drives NextViewSearch::chooseInitialPair (reconstructor_amd/host/HipNextView.h) and
// GeometricFilter::estimateEssential (HipGeometricFilter.h) over the reference's containers and compares them with
// rcn_twoview_init called directly on the same data (tests/test_twoview_cpp.py runs it).
//
//   usage: twoview_adapter_test <in.txt>
//   in:   images N; per image: id, 6 intrinsics, K; K x (x y); pairs P; per pair: i j n; n x (f g)
//   out:  "pair <i> <j> <n> <count> <in front>", "pose" + 12 doubles as hex words, "E" + 9 doubles as hex words, "end";
//         exit 1 on any difference.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <unordered_map>
#include <vector>

#include "../../reconstructor_amd/host/HipGeometricFilter.h"
#include "../../reconstructor_amd/host/HipNextView.h"

using namespace reconstructor::Core;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::fprintf(stderr, "MISMATCH: %s\n", msg); ++fails; } } while (0)

static void hex(const char *tag, const double *v, int n)
{
    std::printf("%s", tag);
    for (int i = 0; i < n; ++i) { unsigned long long w; std::memcpy(&w, v + i, 8); std::printf(" %016llx", w); }
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s in\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string tag;
    int n_img = 0, n_pairs = 0;
    in >> tag >> n_img;
    std::unordered_map<int, std::vector<FeaturePtr<>>> features;
    std::unordered_map<int, PinholeCamera> intr;
    for (int k = 0; k < n_img; ++k) {
        int id, K;
        PinholeCamera cam;
        in >> id >> cam.fX >> cam.fY >> cam.cX >> cam.cY >> cam.k1 >> cam.k2 >> K;
        intr[id] = cam;
        features[id];
        for (int f = 0; f < K; ++f) {
            int x, y;
            in >> x >> y;
            features[id].push_back(std::make_shared<Feature<>>(FeatCoord<>(x, y), FeatDesc()));
        }
    }
    in >> tag >> n_pairs;
    std::map<std::pair<int, int>, std::unordered_map<int, int>> featureMatches;
    for (int p = 0; p < n_pairs; ++p) {
        int i, j, n;
        in >> i >> j >> n;
        auto &m = featureMatches[{i, j}];
        for (int e = 0; e < n; ++e) { int f, g; in >> f >> g; m[f] = g; }
    }
    if (!in) { std::fprintf(stderr, "short input\n"); return 2; }
    rcn_ctx *ctx = nullptr;
    if (rcn_create(0, &ctx) != RCN_OK) { std::fprintf(stderr, "no device\n"); return 2; }
    {
        NextViewSearch next(ctx);
        GeometricFilter filter(ctx);
        int i1 = -1, i2 = -1;
        std::vector<bool> inl;
        const Mat4d T = next.chooseInitialPair(i1, i2, features, featureMatches, intr, &inl);
        // the ABI, directly, on the chosen pair's matches in ascending order of the first image's feature
        const auto &m = featureMatches.at({i1, i2});
        std::vector<std::pair<int, int>> qt(m.begin(), m.end());
        std::sort(qt.begin(), qt.end());
        const int n = (int)qt.size();
        std::vector<int32_t> xy1, xy2;
        std::vector<FeaturePtr<>> f1, f2;
        for (const auto &[f, g] : qt) {
            f1.push_back(features[i1][f]); f2.push_back(features[i2][g]);
            xy1.push_back(f1.back()->featCoord.x); xy1.push_back(f1.back()->featCoord.y);
            xy2.push_back(f2.back()->featCoord.x); xy2.push_back(f2.back()->featCoord.y);
        }
        const PinholeCamera &a = intr[i1], &b = intr[i2];
        const double K1[6] = {a.fX, a.fY, a.cX, a.cY, a.k1, a.k2}, K2[6] = {b.fX, b.fY, b.cX, b.cY, b.k1, b.k2};
        const int64_t off[2] = {0, n};
        double E[9], P[12];
        std::vector<uint8_t> mask(n + 1), cmask(n + 1);
        int32_t count[2] = {0, 0};
        if (rcn_twoview_init(ctx, 1, off, xy1.data(), xy2.data(), K1, K2, nullptr, E, P, mask.data(), cmask.data(), count, nullptr) != RCN_OK) {
            std::fprintf(stderr, "rcn_twoview_init: %s\n", rcn_last_error(ctx));
            return 1;
        }
        bool same = true;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) same &= std::memcmp(&T.m[4 * r + c], &P[4 * r + c], 8) == 0;
        EXPECT(same, "pose bits");
        EXPECT(T(3, 0) == 0 && T(3, 1) == 0 && T(3, 2) == 0 && T(3, 3) == 1, "last row");
        EXPECT((int)inl.size() == n, "one flag per match");
        for (int e = 0; e < n && e < (int)inl.size(); ++e) EXPECT(inl[e] == (mask[e] != 0), "inlier flags = mask bytes");
        std::vector<bool> inl2;
        const Mat3d E2 = filter.estimateEssential(f1, f2, a, b, inl2);
        EXPECT(std::memcmp(E2.m, E, 72) == 0, "E bits");
        EXPECT(inl2 == inl, "estimateEssential fills the mask");
        EXPECT(std::memcmp(filter.lastPose34(), P, 96) == 0 && filter.lastInliers() == count[0] && filter.lastInFront() == count[1], "pose of the last call");
        std::vector<bool> none;                                   // fewer than 5 matches: a zero matrix, no flags
        f1.resize(std::min(n, 4)); f2.resize(std::min(n, 4));
        const Mat3d Z = filter.estimateEssential(f1, f2, a, b, none);
        bool zero = true;
        for (double v : Z.m) zero &= v == 0.0;
        EXPECT(zero && none.empty() && filter.lastInliers() == -2, "no model below 5 matches");
        std::printf("pair %d %d %d %d %d\n", i1, i2, n, count[0], count[1]);
        hex("pose", P, 12);
        hex("E", E, 9);
    }
    rcn_destroy(ctx);
    if (fails) return 1;
    std::printf("end\n");
    return 0;
}
