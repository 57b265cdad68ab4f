// pnp_adapter_test -- drives NextViewSearch::registerImagePnP (reconstructor_amd/host/HipNextView.h) over the reference's
// containers and compares it with rcn_pnp_ransac called directly on the same data (tests/test_pnp_cpp.py runs it).
//
//   usage: pnp_adapter_test <in.txt>
//   in:   points N; N x (x y z); views V; per view: image id, 6 intrinsics, n; n x (landmark x y)
//   out:  one line per view: "view <id> <count> <kept>" or "view <id> <count> threw", then "end"; exit 1 on any difference.
// Entry e of a view is feature e of its image.  A view with count < 0 must throw and leave both lists as they were.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <unordered_map>
#include <vector>

#include "../../reconstructor_amd/host/HipNextView.h"

using namespace reconstructor::Core;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::fprintf(stderr, "MISMATCH: %s\n", msg); ++fails; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s in\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string tag;
    int n_pts = 0, n_views = 0;
    in >> tag >> n_pts;
    std::vector<Landmark> landmarks;
    std::vector<double> pts;
    for (int j = 0; j < n_pts; ++j) {
        double x, y, z;
        in >> x >> y >> z;
        landmarks.emplace_back(x, y, z);
        pts.push_back(x); pts.push_back(y); pts.push_back(z);
    }
    in >> tag >> n_views;
    rcn_ctx *ctx = nullptr;
    if (rcn_create(0, &ctx) != RCN_OK) { std::fprintf(stderr, "no device\n"); return 2; }
    {
        NextViewSearch next(ctx);
        for (int v = 0; v < n_views; ++v) {
            int id, n;
            PinholeCamera cam;
            in >> id >> cam.fX >> cam.fY >> cam.cX >> cam.cY >> cam.k1 >> cam.k2 >> n;
            std::unordered_map<int, std::vector<FeaturePtr<>>> features;
            std::unordered_map<int, PinholeCamera> intr;
            intr[id] = cam;
            std::vector<int> featureIdxs, landmarkIdxs;
            std::vector<int32_t> lid, xy;
            for (int e = 0; e < n; ++e) {
                int l, x, y;
                in >> l >> x >> y;
                features[id].push_back(std::make_shared<Feature<>>(FeatCoord<>(x, y), FeatDesc()));
                featureIdxs.push_back(e);
                landmarkIdxs.push_back(l);
                lid.push_back(l); xy.push_back(x); xy.push_back(y);
            }
            if (!in) { std::fprintf(stderr, "short input\n"); return 2; }
            // the ABI, directly
            const double K[6] = {cam.fX, cam.fY, cam.cX, cam.cY, cam.k1, cam.k2};
            const int64_t off[2] = {0, n};
            double P[12];
            std::vector<uint8_t> mask(n + 1);
            int32_t count = 0;
            if (rcn_pnp_ransac(ctx, 1, off, lid.data(), xy.data(), n_pts, pts.data(), K, nullptr, P, nullptr, mask.data(), &count, nullptr) != RCN_OK) {
                std::fprintf(stderr, "rcn_pnp_ransac: %s\n", rcn_last_error(ctx));
                return 1;
            }
            const std::vector<int> f0 = featureIdxs, l0 = landmarkIdxs;
            bool threw = false;
            Mat4d T;
            try {
                T = next.registerImagePnP(id, featureIdxs, landmarkIdxs, features, landmarks, intr);
            } catch (const std::runtime_error &) {
                threw = true;
            }
            EXPECT(threw == (count < 0), "throws exactly when there is no model");
            if (threw) {
                EXPECT(featureIdxs == f0 && landmarkIdxs == l0, "lists untouched after a throw");
                std::printf("view %d %d threw\n", id, count);
                continue;
            }
            std::vector<int> wantF, wantL;
            for (int e = 0; e < n; ++e)
                if (mask[e]) { wantF.push_back(e); wantL.push_back(lid[e]); }
            EXPECT((int)wantF.size() == count, "count = mask bytes");
            EXPECT(featureIdxs == wantF && landmarkIdxs == wantL, "trimmed lists = masked entries in order");
            bool same = true;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) same &= std::memcmp(&T.m[4 * r + c], &P[4 * r + c], 8) == 0;
            EXPECT(same, "pose bits");
            EXPECT(T(3, 0) == 0 && T(3, 1) == 0 && T(3, 2) == 0 && T(3, 3) == 1, "last row");
            std::printf("view %d %d %zu\n", id, count, featureIdxs.size());
        }
    }
    rcn_destroy(ctx);
    if (fails) return 1;
    std::printf("end\n");
    return 0;
}
