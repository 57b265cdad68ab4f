// new_view_tracks_adapter_test -- drives Triangulator::triangulateMatchedLandmarksDevice (reconstructor_amd/host/
// HipTriangulator.h) next to the host method on equal containers (tests/test_new_view_tracks_cpp.py compares the two).
//
//   usage: new_view_tracks_adapter_test <in.txt> <out.txt>
//   in:   triangulate_adapter_test's format
//   out:  per run ("host": triangulateMatchedLandmarks, "dev": uploadContainers once, then triangulateMatchedLandmarksDevice)
//         every landmark (x y z as hex floats, its track) and every feature's landmarkId, each line behind the run's name;
//         for the dev run also the landmark-id table of every image as the device holds it at the end ("table").
//   Both runs register the initial pair, triangulate it on the host path, then per view compute the 2D-3D matches the way
//   calc2d3dMatches does (:654-679), run step 1 + step 3 and register the view (:805-809).  No PnP, no BA.
//
//   usage: new_view_tracks_adapter_test --time-host-loop <in.txt> <reps>
//   Times step 3's walk alone (Triangulator::newViewTracks) on the reference's containers; needs no GPU.
//   in:   view v K_v R; K_v landmark ids of v; per registered image: id K n, K landmark ids, n x (f g) = featureMatches[(v, id)]
//   out:  one line "host_loop tracks <n> ms_median <t> ms_min <t>" on stdout
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
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
using Features = std::unordered_map<int, std::vector<FeaturePtr<>>>;

static Features clone(const Features &src)
{
    Features out;
    for (const auto &[id, fs] : src) {
        auto &v = out[id];
        for (const auto &f : fs) v.push_back(std::make_shared<Feature<>>(*f));
    }
    return out;
}

static int time_host_loop(const char *path, int reps)
{
    std::ifstream in(path);
    std::string tag;
    int v, Kv, R;
    in >> tag >> v >> Kv >> R;
    Features features;
    auto fill = [&](int id, int K) {
        auto &fs = features[id];
        for (int f = 0; f < K; ++f) {
            auto p = std::make_shared<Feature<>>();
            in >> p->landmarkId;
            fs.push_back(p);
        }
    };
    fill(v, Kv);
    FeatureMatches featureMatches;
    std::unordered_map<int, bool> registeredImages;
    std::unordered_map<int, std::vector<int>> imgMatches;
    for (int k = 0; k < R; ++k) {
        int id, K, n;
        in >> id >> K >> n;
        fill(id, K);
        auto &m = featureMatches[{v, id}];
        for (int e = 0; e < n; ++e) { int f, g; in >> f >> g; m[f] = g; }
        registeredImages[id] = true;
        imgMatches[v].push_back(id);
    }
    if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }
    std::vector<double> ms;
    size_t n_tracks = 0;
    for (int r = 0; r < reps + 2; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        const auto batch = Triangulator::newViewTracks(v, features, registeredImages, imgMatches, featureMatches);
        const auto t1 = std::chrono::steady_clock::now();
        n_tracks = batch.size();
        if (r >= 2) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());       // two warm-up rounds
    }
    std::sort(ms.begin(), ms.end());
    std::printf("host_loop tracks %zu ms_median %.6f ms_min %.6f\n", n_tracks, ms[ms.size() / 2], ms[0]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "--time-host-loop")) return time_host_loop(argv[2], std::max(1, std::atoi(argv[3])));
    if (argc != 3) { std::fprintf(stderr, "usage: %s in out | --time-host-loop in reps\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string tag;
    int n_img = 0;
    in >> tag >> n_img;
    Features features0;
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
        auto &fs = features0[id];
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
    Triangulator tri;
    char buf[128];
    for (int run = 0; run < 2; ++run) {
        const char *name = run ? "dev" : "host";
        Features features = clone(features0);
        std::vector<Landmark> landmarks;
        std::unordered_map<int, bool> registeredImages;
        registeredImages[i1] = true;                                   // :1018-1021
        registeredImages[i2] = true;
        tri.triangulateInitialPair(i1, i2, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics, featureMatches);
        if (run) tri.uploadContainers(features, featureMatches);
        for (int v : views) {
            std::vector<int> featureIds, landmarkIds;                  // calc2d3dMatches, :654-679
            const auto &cand = imgMatches[v];
            for (size_t lid = 0; lid < landmarks.size(); ++lid)
                for (const auto &tf : landmarks[lid].triangulatedFeatures) {
                    if (std::find(cand.begin(), cand.end(), tf.imgIdx) == cand.end()) continue;
                    const auto fm = featureMatches.find(std::make_pair(tf.imgIdx, v));
                    if (fm == featureMatches.end()) continue;
                    const auto it = fm->second.find(tf.featIdx);
                    if (it != fm->second.end() && features[v][it->second]->landmarkId == -1) {
                        featureIds.push_back(it->second);
                        landmarkIds.push_back((int)lid);
                    }
                }
            if (run)
                tri.triangulateMatchedLandmarksDevice(v, featureIds, landmarkIds, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics,
                                                      registeredImages, imgMatches, featureMatches);
            else
                tri.triangulateMatchedLandmarks(v, featureIds, landmarkIds, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics,
                                                registeredImages, imgMatches, featureMatches);
            registeredImages[v] = true;                                // :809
        }
        for (const auto &lm : landmarks) {
            std::snprintf(buf, sizeof buf, "%s lm %a %a %a %zu", name, lm.x, lm.y, lm.z, lm.triangulatedFeatures.size());
            out << buf;
            for (const auto &tf : lm.triangulatedFeatures) out << ' ' << tf.imgIdx << ' ' << tf.featIdx;
            out << '\n';
        }
        for (int id : imgIds) {
            out << name << " ids " << id;
            for (const auto &f : features[id]) out << ' ' << f->landmarkId;
            out << '\n';
            if (!run) continue;
            std::vector<int32_t> row(features[id].size() + 1);
            if (rcn_landmark_ids_read(tri.ctx(), id, row.data(), (int32_t)features[id].size()) != RCN_OK) {
                std::fprintf(stderr, "rcn_landmark_ids_read: %s\n", rcn_last_error(tri.ctx()));
                return 1;
            }
            out << "dev table " << id;
            for (size_t f = 0; f < features[id].size(); ++f) out << ' ' << row[f];
            out << '\n';
        }
    }
    out << "end\n";
    return out ? 0 : 1;
}
