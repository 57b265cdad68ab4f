// twoview_geometry_adapter_test -- drives NextViewSearch::chooseInitialPairByGeometry (reconstructor_amd/host/HipNextView.h)
// and GeometricFilter::estimateHomography (HipGeometricFilter.h) over the reference's containers, compares them with the C
// calls (rcn_twoview_init, rcn_homography_ransac) on the same matches bit for bit, and prints what
// tests/test_twoview_geometry_cpp.py compares with the Python entries.  chooseInitialPair must give what it gave before.
//   twoview_geometry_adapter_test in top_m
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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
    if (argc != 3) { std::fprintf(stderr, "usage: %s in top_m\n", argv[0]); return 2; }
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
        int c1 = -1, c2 = -1;
        const Mat4d Tc = next.chooseInitialPair(c1, c2, features, featureMatches, intr);
        std::printf("canonical %d %d\n", c1, c2);
        hex("canonical_pose", Tc.m, 12);
        rcn_twoview_geometry_options o;
        rcn_twoview_geometry_default_options(&o);
        o.top_m = std::atoi(argv[2]);
        int i1 = -1, i2 = -1;
        std::vector<bool> inl;
        NextViewSearch::PairChoiceReport rep;
        const Mat4d T = next.chooseInitialPairByGeometry(i1, i2, features, featureMatches, intr, &o, &inl, &rep);
        std::printf("chosen %d %d %d %d\n", i1, i2, rep.chosen, rep.fallback ? 1 : 0);
        for (const auto &g : rep.candidates) {
            std::printf("cand %d %d %d %d %d %d %d", g.imgIdx1, g.imgIdx2, g.matches, g.inliersE, g.inFront, g.inliersH, g.label);
            hex("", &g.ratio, 1);
        }
        for (const auto &g : rep.candidates) hex("angle", &g.medianAngle, 1);
        EXPECT(rep.chosen >= 0 && rep.chosen < (int)rep.candidates.size() && rep.candidates[rep.chosen].imgIdx1 == i1 && rep.candidates[rep.chosen].imgIdx2 == i2, "the report names the chosen pair");
        // the C calls, directly, on the chosen pair's matches in ascending order of the first image's feature
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
        double P[12], H[9];
        std::vector<uint8_t> mask(n + 1), hmask(n + 1);
        int32_t count[2] = {0, 0}, hcount = 0;
        if (rcn_twoview_init(ctx, 1, off, xy1.data(), xy2.data(), K1, K2, nullptr, nullptr, P, mask.data(), nullptr, count, nullptr) != RCN_OK ||
            rcn_homography_ransac(ctx, 1, off, xy1.data(), xy2.data(), nullptr, H, hmask.data(), &hcount, nullptr) != RCN_OK) {
            std::fprintf(stderr, "C calls: %s\n", rcn_last_error(ctx));
            return 1;
        }
        bool same = true;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) same &= std::memcmp(&T.m[4 * r + c], &P[4 * r + c], 8) == 0;
        EXPECT(same, "pose bits");
        EXPECT(T(3, 0) == 0 && T(3, 1) == 0 && T(3, 2) == 0 && T(3, 3) == 1, "last row");
        EXPECT((int)inl.size() == n, "one flag per match");
        for (int e = 0; e < n && e < (int)inl.size(); ++e) EXPECT(inl[e] == (mask[e] != 0), "inlier flags = mask bytes");
        EXPECT(rep.candidates[rep.chosen].inliersE == count[0] && rep.candidates[rep.chosen].inFront == count[1] && rep.candidates[rep.chosen].inliersH == hcount, "the report's counts");
        std::vector<bool> hin;
        const Mat3d H2 = filter.estimateHomography(f1, f2, hin);
        EXPECT(std::memcmp(H2.m, H, 72) == 0, "H bits");
        EXPECT((int)hin.size() == n && filter.lastInliers() == hcount, "estimateHomography fills the mask");
        for (int e = 0; e < n && e < (int)hin.size(); ++e) EXPECT(hin[e] == (hmask[e] != 0), "H inlier flags = mask bytes");
        std::vector<bool> none;                                   // fewer than 4 matches: a zero matrix, no flags
        f1.resize(std::min(n, 3)); f2.resize(std::min(n, 3));
        const Mat3d Z = filter.estimateHomography(f1, f2, none);
        bool zero = true;
        for (double v : Z.m) zero &= v == 0.0;
        EXPECT(zero && none.empty() && filter.lastInliers() == -2, "no model below 4 matches");
        hex("pose", P, 12);
        hex("H", H, 9);
        std::printf("hcount %d\n", hcount);
    }
    rcn_destroy(ctx);
    if (fails) return 1;
    std::printf("end\n");
    return 0;
}
