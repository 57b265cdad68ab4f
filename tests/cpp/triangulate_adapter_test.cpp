// triangulate_adapter_test -- drives reconstructor_amd/host/HipTriangulator.h over the reference's containers
// (tests/test_triangulate_cpp.py writes them, then restates the loop sequentially in Python and compares).
//
//   usage: triangulate_adapter_test <in.txt> <out.txt>
//   in:   images N; per image: id, n_feat, 12 pose numbers (rows of [R | t]), 6 intrinsics, n_feat x (x y);
//         pairs M; per pair: i j n, n x (q t); per image: n, the images it was matched with; init i1 i2; views V, V ids
//   out:  the iteration order of featureMatches[(i1, i2)] and, per view, of registeredImages (std::unordered_map: the
//         test restates the loop in exactly these orders); every landmark (x y z as hex floats, its track); every
//         feature's landmarkId.
// The driver registers the initial pair, triangulates it, then per view computes the 2D-3D matches the way
// calc2d3dMatches does (:654-679), runs triangulateMatchedLandmarks and registers the view (:805-809).  No PnP, no BA.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <unordered_map>
#include <vector>

#include "../../reconstructor_amd/host/HipTriangulator.h"

using namespace reconstructor::Core;

struct pair_hash {
    std::size_t operator()(const std::pair<int, int> &p) const { return std::hash<long long>()(((long long)p.first << 32) ^ (unsigned)p.second); }
};
using FeatureMatches = std::unordered_map<std::pair<int, int>, std::unordered_map<int, int>, pair_hash>;

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string tag;
    int n_img = 0;
    in >> tag >> n_img;
    std::unordered_map<int, std::vector<FeaturePtr<>>> features;
    std::unordered_map<int, Mat4d> imgIdx2camPose;
    std::unordered_map<int, PinholeCamera> imgIdx2camIntrinsics;
    std::vector<int> imgIds;
    for (int k = 0; k < n_img; ++k) {
        int id, nf;
        in >> id >> nf;
        imgIds.push_back(id);
        Mat4d T;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) in >> T(r, c);
        imgIdx2camPose[id] = T;
        PinholeCamera cam;
        in >> cam.fX >> cam.fY >> cam.cX >> cam.cY >> cam.k1 >> cam.k2;
        imgIdx2camIntrinsics[id] = cam;
        auto &fs = features[id];
        for (int f = 0; f < nf; ++f) {
            int x, y;
            in >> x >> y;
            auto p = std::make_shared<Feature<>>();
            p->featCoord = FeatCoord<>(x, y);
            fs.push_back(p);
        }
    }
    int n_pairs = 0;
    in >> tag >> n_pairs;
    FeatureMatches featureMatches;
    for (int k = 0; k < n_pairs; ++k) {
        int i, j, n;
        in >> i >> j >> n;
        auto &m = featureMatches[{i, j}];
        for (int e = 0; e < n; ++e) { int q, t; in >> q >> t; m[q] = t; }
    }
    std::unordered_map<int, std::vector<int>> imgMatches;
    for (int id : imgIds) {
        int n;
        in >> n;
        auto &v = imgMatches[id];
        for (int e = 0; e < n; ++e) { int j; in >> j; v.push_back(j); }
    }
    int i1, i2, n_views;
    in >> tag >> i1 >> i2 >> tag >> n_views;
    std::vector<int> views(n_views);
    for (int &v : views) in >> v;
    if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }

    std::ofstream out(argv[2]);
    std::vector<Landmark> landmarks;
    std::unordered_map<int, bool> registeredImages;
    Triangulator tri;
    registeredImages[i1] = true;                                   // :1018-1021
    registeredImages[i2] = true;
    out << "pairorder";
    for (const auto &kv : featureMatches[{i1, i2}]) out << ' ' << kv.first;
    out << '\n';
    tri.triangulateInitialPair(i1, i2, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics, featureMatches);
    for (int v : views) {
        std::vector<int> featureIds, landmarkIds;                  // calc2d3dMatches, :654-679
        const auto &cand = imgMatches[v];
        for (size_t lid = 0; lid < landmarks.size(); ++lid)
            for (const auto &tf : landmarks[lid].triangulatedFeatures) {
                if (std::find(cand.begin(), cand.end(), tf.imgIdx) == cand.end()) continue;
                auto &fm = featureMatches[std::make_pair(tf.imgIdx, v)];
                auto it = fm.find(tf.featIdx);
                if (it != fm.end() && features[v][it->second]->landmarkId == -1) {
                    featureIds.push_back(it->second);
                    landmarkIds.push_back((int)lid);
                }
            }
        out << "regorder " << v;
        for (const auto &kv : registeredImages) out << ' ' << kv.first << ' ' << (kv.second ? 1 : 0);
        out << '\n';
        tri.triangulateMatchedLandmarks(v, featureIds, landmarkIds, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics,
                                        registeredImages, imgMatches, featureMatches);
        registeredImages[v] = true;                                // :809
    }
    char buf[128];
    for (const auto &lm : landmarks) {
        std::snprintf(buf, sizeof buf, "lm %a %a %a %zu", lm.x, lm.y, lm.z, lm.triangulatedFeatures.size());
        out << buf;
        for (const auto &tf : lm.triangulatedFeatures) out << ' ' << tf.imgIdx << ' ' << tf.featIdx;
        out << '\n';
    }
    for (int id : imgIds) {
        out << "ids " << id;
        for (const auto &f : features[id]) out << ' ' << f->landmarkId;
        out << '\n';
    }
    out << "end\n";
    return out ? 0 : 1;
}
