// next_view_adapter_test -- drives reconstructor_amd/host/HipNextView.h over the reference's containers and compares it, one
// call at a time, with a plain restatement of the reference's loops written here (tests/test_nextview_cpp.py runs it).
//
//   usage: next_view_adapter_test <in.txt>
//   in:   images N; per image: id, n_feat, 12 pose numbers (rows of [R | t]), 6 intrinsics, n_feat x (x y);
//         pairs M; per pair: i j n, n x (q t); per image: n, the images it was matched with; init i1 i2; shape rows cols
//   out:  one line per step: "step <mode-0 order size> <chosen view> <entries> <score ties>", then "end"; exit 1 on any
//         difference.
// Every step: calc2d3dMatches + rankNextImages in both modes (adapter and restatement, on the same maps), the view the
// density ranking puts first is registered with its scene pose (no PnP), step 1 by the adapter against the restatement,
// step 3 by HipTriangulator.h.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <set>
#include <unordered_map>
#include <vector>

#include "../../reconstructor_amd/host/HipNextView.h"
#include "../../reconstructor_amd/host/HipTriangulator.h"

using namespace reconstructor::Core;

struct pair_hash {
    std::size_t operator()(const std::pair<int, int> &p) const { return std::hash<long long>()(((long long)p.first << 32) ^ (unsigned)p.second); }
};
using FeatureMatches = std::unordered_map<std::pair<int, int>, std::unordered_map<int, int>, pair_hash>;
using Features = std::unordered_map<int, std::vector<FeaturePtr<>>>;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::fprintf(stderr, "MISMATCH: %s\n", msg); ++fails; } } while (0)

// calc2d3dMatches (:654-679), restated
static void plain_calc(const std::set<int> &cands, std::unordered_map<int, std::vector<int>> &imgMatches, FeatureMatches &fm,
                       Features &features, const std::vector<Landmark> &landmarks, std::unordered_map<int, std::vector<int>> &L,
                       std::unordered_map<int, std::vector<int>> &F)
{
    for (int c : cands) {
        std::vector<int> lids, fids;
        const auto &cm = imgMatches[c];
        for (size_t l = 0; l < landmarks.size(); ++l)
            for (const auto &tf : landmarks[l].triangulatedFeatures) {
                if (std::find(cm.begin(), cm.end(), tf.imgIdx) == cm.end()) continue;
                auto it = fm.find({tf.imgIdx, c});
                if (it == fm.end()) continue;
                auto m = it->second.find(tf.featIdx);
                if (m != it->second.end() && features[c][m->second]->landmarkId == -1) { lids.push_back((int)l); fids.push_back(m->second); }
            }
        L[c] = lids;
        F[c] = fids;
    }
}

static int density(const std::vector<int> &fids, const std::vector<FeaturePtr<>> &feats, std::pair<int, int> shape)
{
    bool cell[32][32] = {};
    for (int g : fids) {
        const int cx = 32 * feats[g]->featCoord.x / static_cast<double>(shape.second);
        const int cy = 32 * feats[g]->featCoord.y / static_cast<double>(shape.first);
        if (cx >= 0 && cx < 32 && cy >= 0 && cy < 32) cell[cy][cx] = true;      // the reference writes out of bounds here
    }
    int s = 0;
    for (auto &r : cell) for (bool b : r) s += b;
    return s;
}

// rankNextImages (:697-759), restated
static std::vector<int> plain_rank(int mode, const std::unordered_map<int, std::vector<int>> &L, const std::unordered_map<int, std::vector<int>> &F,
                                   Features &features, std::unordered_map<int, std::pair<int, int>> &shapes, int minNum, int *ties)
{
    std::vector<int> out;
    if (mode == MatchTotal) {
        std::map<int, int, std::greater<int>> m;
        for (const auto &[id, l] : L) m[id] = (int)l.size();
        for (const auto &kv : m) out.push_back(kv.first);
        return out;
    }
    std::map<int, int, std::greater<int>> s2i;
    std::map<int, int> seen;
    for (const auto &[id, f] : F) {
        const int s = density(f, features[id], shapes[id]);
        s2i[s] = id;
        if (s > minNum && ++seen[s] == 2) ++*ties;
    }
    for (const auto &[s, id] : s2i) if (s > minNum) out.push_back(id);
    return out;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s in\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string tag;
    int n_img = 0;
    in >> tag >> n_img;
    Features features;
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
    int i1, i2, rows, cols;
    in >> tag >> i1 >> i2 >> tag >> rows >> cols;
    if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }
    std::unordered_map<int, std::pair<int, int>> shapes;
    for (int id : imgIds) shapes[id] = {rows, cols};

    rcn_ctx *ctx = nullptr;
    if (rcn_create(0, &ctx) != RCN_OK) { std::fprintf(stderr, "no device\n"); return 2; }
    {
        Triangulator tri(ctx);
        NextViewSearch nv(ctx);
        std::vector<Landmark> landmarks;
        std::unordered_map<int, bool> registeredImages{{i1, true}, {i2, true}};
        tri.triangulateInitialPair(i1, i2, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics, featureMatches);
        nv.uploadMatches(features, imgMatches, featureMatches);
        for (;;) {
            std::set<int> cands;
            for (int id : imgIds) if (!registeredImages.count(id)) cands.insert(id);
            if (cands.empty()) break;
            std::vector<int> sorted[2];
            std::unordered_map<int, std::vector<int>> L, F;
            int ties = 0;
            for (int mode : {MatchTotal, MatchDensity}) {
                std::unordered_map<int, std::vector<int>> aL, aF, pL, pF;
                nv.nextImageRankingMode = (NextImageRankingMode)mode;
                nv.calc2d3dMatches(cands, aL, aF, features, landmarks, shapes);
                nv.rankNextImages(aL, aF, sorted[mode]);
                plain_calc(cands, imgMatches, featureMatches, features, landmarks, pL, pF);
                EXPECT(aL == pL && aF == pF, "calc2d3dMatches");
                EXPECT(sorted[mode] == plain_rank(mode, aL, aF, features, shapes, nv.min2d3dMatchNum, &ties), "rankNextImages");
                L = aL; F = aF;
            }
            if (sorted[MatchDensity].empty()) { std::cout << "stop " << cands.size() << "\n"; break; }
            const int v = sorted[MatchDensity][0];
            // step 1, restated on the side (no mutation), then by the adapter
            std::vector<int> want;
            std::set<int> taken;
            for (size_t e = 0; e < F[v].size(); ++e) {
                const Landmark &lm = landmarks[L[v][e]];
                double depth;
                const double r = Triangulator::projectionError(imgIdx2camPose[v], imgIdx2camIntrinsics[v], lm.x, lm.y, lm.z,
                                                               features[v][F[v][e]]->featCoord, &depth);
                want.push_back(!(depth > 0) ? 1 : !(r < 4.0) ? 2 : taken.count(F[v][e]) ? 3 : 0);
                if (want.back() == 0) taken.insert(F[v][e]);
            }
            std::vector<size_t> before;
            for (const auto &lm : landmarks) before.push_back(lm.triangulatedFeatures.size());
            const std::vector<uint8_t> st = nv.attachMatchedLandmarks(v, F[v], L[v], features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics);
            EXPECT(std::vector<int>(st.begin(), st.end()) == want, "attach status");
            size_t added = 0;
            for (size_t l = 0; l < landmarks.size(); ++l) added += landmarks[l].triangulatedFeatures.size() - before[l];
            EXPECT(added == taken.size(), "attach appended");
            tri.triangulateMatchedLandmarks(v, {}, {}, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics, registeredImages,
                                            imgMatches, featureMatches);
            registeredImages[v] = true;
            std::cout << "step " << sorted[MatchTotal].size() << ' ' << v << ' ' << F[v].size() << ' ' << ties << ' ' << taken.size() << "\n";
        }
        std::cout << "end " << landmarks.size() << "\n";
    }
    rcn_destroy(ctx);
    return fails ? 1 : 0;
}
