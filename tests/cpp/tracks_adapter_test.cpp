// tracks_adapter_test -- TrackBuilder (reconstructor_amd/host/HipTrackBuilder.h) on the reference's containers against a sequential
// union-find written here: 9 images of up to 300 keypoints, random injective matches on most pairs, most of them between keypoints
// of one planted landmark and some wrong.  Compared: build() under both conflict policies, with a selection and min_length 3, and
// buildDevice()'s CSR copied back.  Prints "tracks A B C observations D" (the four builds' track counts, the first one's
// observations) and returns 0 when everything is equal.
#include <algorithm>
#include <cstdio>
#include <map>
#include <numeric>
#include <set>

#include "../../reconstructor_amd/host/HipTrackBuilder.h"

using namespace reconstructor::Core;
using FeatureMatches = std::map<std::pair<int, int>, std::map<int, int>>;
using Track = TrackBuilder::Track;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

// the loop a user runs today: union-find over (image, feature), components, the conflict rule, the selection, the length filter
static std::vector<Track> hostTracks(const std::unordered_map<int, std::vector<FeaturePtr<>>> &features, const FeatureMatches &fm, int conflict,
                                     const std::vector<int> *selected, int minLength)
{
    std::set<int> imgs;
    for (const auto &[key, m] : fm) { imgs.insert(key.first); imgs.insert(key.second); }
    std::map<int, int> first;
    std::vector<std::pair<int, int>> node;
    for (int i : imgs) {
        first[i] = (int)node.size();
        for (size_t f = 0; f < features.at(i).size(); ++f) node.emplace_back(i, (int)f);
    }
    std::vector<int> parent(node.size());
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (const auto &[key, m] : fm)
        for (const auto &[f, g] : m) {
            const int a = find(first[key.first] + f), b = find(first[key.second] + g);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);
        }
    std::map<int, std::vector<int>> comp;
    for (int x = 0; x < (int)node.size(); ++x) comp[find(x)].push_back(x);
    std::vector<Track> out;
    for (const auto &[root, xs] : comp) {
        if (xs.size() < 2) continue;
        std::map<int, int> perImg;
        for (int x : xs) ++perImg[node[x].first];
        bool any = false;
        for (const auto &[i, c] : perImg) any = any || c >= 2;
        if (any && conflict == RCN_TRACKS_CONFLICT_DROP_TRACK) continue;
        Track t;
        for (int x : xs) {
            if (perImg[node[x].first] >= 2) continue;
            if (selected && std::find(selected->begin(), selected->end(), node[x].first) == selected->end()) continue;
            t.push_back(node[x]);
        }
        if ((int)t.size() >= minLength) out.push_back(t);
    }
    std::sort(out.begin(), out.end());
    return out;
}

int main()
{
    const int nImg = 9, nLandmarks = 400;
    std::unordered_map<int, std::vector<FeaturePtr<>>> features;
    std::map<int, std::vector<int>> landmarkOf;
    for (int i = 0; i < nImg; ++i) {
        const int id = 3 * i + 1;
        const int K = 200 + (int)rnd(101);
        for (int f = 0; f < K; ++f) {
            features[id].push_back(std::make_shared<Feature<>>(FeatCoord<>(1000 * i + f, 7 * f + i), FeatDesc()));
            landmarkOf[id].push_back((int)rnd(nLandmarks));
        }
    }
    FeatureMatches fm;
    for (const auto &[a, fa] : features)
        for (const auto &[b, fb] : features) {
            if (a >= b || rnd(10) < 3) continue;
            std::set<int> used;
            for (size_t f = 0; f < fa.size(); ++f) {
                int g = -1;
                if (rnd(100) < 4) g = (int)rnd((uint32_t)fb.size());                       // a wrong match
                else
                    for (size_t c = 0; c < fb.size() && g < 0; ++c)
                        if (landmarkOf[b][c] == landmarkOf[a][f]) g = (int)c;             // the first keypoint of the same landmark
                if (g >= 0 && used.insert(g).second && rnd(4) != 0) fm[{a, b}][(int)f] = g;
            }
        }
    fm[{4, 1}] = {};                                                                      // a reverse pair with an empty list

    TrackBuilder tb;
    int counts[4] = {0, 0, 0, 0};
    size_t obs = 0;
    const std::vector<int> selected = {25, 4, 13, 7, 19};
    for (int run = 0; run < 3; ++run) {
        tb.options.conflict = run == 1 ? RCN_TRACKS_CONFLICT_DROP_IMAGE : RCN_TRACKS_CONFLICT_DROP_TRACK;
        tb.options.min_length = run == 2 ? 3 : 2;
        const std::vector<int> *sel = run == 2 ? &selected : nullptr;
        const std::vector<Track> got = tb.build(features, fm, sel), want = hostTracks(features, fm, tb.options.conflict, sel, tb.options.min_length);
        if (got != want) { std::fprintf(stderr, "run %d: %zu tracks, the host loop has %zu\n", run, got.size(), want.size()); return 1; }
        counts[run] = (int)got.size();
        if (run == 0) for (const Track &t : got) obs += t.size();
    }
    // the CSR left on the device, for the selection above (camera row = position in the selection)
    std::vector<std::pair<int, int>> imgCam;
    for (size_t k = 0; k < selected.size(); ++k) imgCam.emplace_back(selected[k], (int)k);
    const TrackBuilder::DeviceTracks d = tb.buildDevice(imgCam);
    const std::vector<Track> want = hostTracks(features, fm, tb.options.conflict, &selected, tb.options.min_length);
    if (d.nTracks != (int)want.size() || d.nTracks > d.capTracks || d.nObs > d.capObs) { std::fprintf(stderr, "buildDevice: %d tracks, the host loop has %zu\n", d.nTracks, want.size()); return 1; }
    std::vector<int32_t> off((size_t)d.nTracks + 1), img((size_t)d.nObs), feat((size_t)d.nObs), cam((size_t)d.nObs), xy(2 * (size_t)d.nObs);
    if (hipMemcpy(off.data(), d.trkOff, 4 * off.size(), 2) || hipMemcpy(img.data(), d.obsImg, 4 * img.size(), 2) || hipMemcpy(feat.data(), d.obsFeat, 4 * feat.size(), 2) ||
        hipMemcpy(cam.data(), d.obsCam, 4 * cam.size(), 2) || hipMemcpy(xy.data(), d.obsXy, 4 * xy.size(), 2)) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
    for (int j = 0; j < d.nTracks; ++j) {
        if (off[(size_t)j + 1] - off[(size_t)j] != (int)want[(size_t)j].size()) { std::fprintf(stderr, "buildDevice: length of track %d\n", j); return 1; }
        for (int o = off[(size_t)j]; o < off[(size_t)j + 1]; ++o) {
            const auto [i, f] = want[(size_t)j][(size_t)(o - off[(size_t)j])];
            const int row = (int)(std::find(selected.begin(), selected.end(), i) - selected.begin());
            const auto &c = features[i][(size_t)f]->featCoord;
            if (img[(size_t)o] != i || feat[(size_t)o] != f || cam[(size_t)o] != row || xy[2 * (size_t)o] != c.x || xy[2 * (size_t)o + 1] != c.y) {
                std::fprintf(stderr, "buildDevice: observation %d of track %d\n", o - off[(size_t)j], j);
                return 1;
            }
        }
    }
    counts[3] = d.nTracks;
    std::printf("tracks %d %d %d %d observations %zu\n", counts[0], counts[1], counts[2], counts[3], obs);
    return 0;
}
