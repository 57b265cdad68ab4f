// HipTrackBuilder.h -- the tracks that the pairwise matches tie together across all images, over the reference's own containers,
// backed by librcn.so (include/rcn.h, rcn_tracks_*).
//
// The reference has no such stage: it creates two-view tracks at a new view and lengthens them one observation at a time
// (SequentialReconstructor.cpp:492-556).  A global pipeline, an N-view triangulation of everything seen so far or a retriangulation
// after a global adjustment needs the tracks as a whole: the connected components of the graph whose nodes are the (image, feature)
// pairs and whose edges are the entries of every featureMatches[(a, b)], without the components in which an image occurs twice
// (options.conflict), cut to the selected images and filtered by length.
//   uploadContainers   every image's pixel coordinates and every directed list of featureMatches, resident in the ctx (the same
//                      residency HipTriangulator.h's uploadContainers sets up; either call serves both)
//   build              uploadContainers + the tracks as std::vector<matchedImgIdFeatId>: observations ascending by (image, feature),
//                      tracks by their first observation
//   buildDevice        the CSR (trk_off, obs_cam, obs_xy) left in HBM for rcn_triangulate_device, over the resident containers;
//                      the buffers belong to the builder and live until the next buildDevice
#pragma once
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/rcn.h"
#include "rcn_types.h"

// The HIP runtime calls this adapter needs for its own buffers, declared here so that the header builds with a plain host
// compiler and no ROCm include path (hipError_t and hipMemcpyKind are int-sized enums; 0 is hipSuccess).
extern "C" {
int hipMalloc(void **ptr, size_t bytes);
int hipFree(void *ptr);
int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);
}

namespace reconstructor::Core {

class TrackBuilder {
public:
    using Track = std::vector<std::pair<int, int>>;     // (imgIdx, featIdx), the reference's matchedImgIdFeatId

    // the result of buildDevice: device pointers into the builder's block
    struct DeviceTracks {
        int32_t nTracks = 0, nObs = 0;                  // of the full result; capTracks / capObs rows were available
        int32_t capTracks = 0, capObs = 0;
        int32_t *trkOff = nullptr, *obsImg = nullptr, *obsFeat = nullptr, *obsCam = nullptr, *obsXy = nullptr;
    };

    explicit TrackBuilder(rcn_ctx *ctx = nullptr) : ctx_(ctx), owned_(false)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("TrackBuilder: no usable gfx950 device");
            owned_ = true;
        }
        rcn_tracks_default_options(&options);
    }
    ~TrackBuilder()
    {
        if (dev_) (void)hipFree(dev_);
        if (owned_) rcn_destroy(ctx_);
    }
    TrackBuilder(const TrackBuilder &) = delete;
    TrackBuilder &operator=(const TrackBuilder &) = delete;

    rcn_ctx *ctx() const { return ctx_; }

    rcn_tracks_options options;     // min_length 2, no max_length, RCN_TRACKS_CONFLICT_DROP_TRACK

    template <class FeatureMatches>
    void uploadContainers(const std::unordered_map<int, std::vector<FeaturePtr<>>> &features, const FeatureMatches &featureMatches)
    {
        std::vector<int32_t> xy;
        for (const auto &[imgIdx, feats] : features) {
            xy.clear();
            for (const auto &f : feats) { xy.push_back(f->featCoord.x); xy.push_back(f->featCoord.y); }
            check(rcn_coords_upload(ctx_, imgIdx, xy.empty() ? nullptr : xy.data(), (int32_t)feats.size()), "uploadContainers");
        }
        std::vector<int32_t> pairs, qt;
        std::vector<int64_t> offsets(1, 0);
        for (const auto &[key, m] : featureMatches) {
            pairs.push_back(key.first); pairs.push_back(key.second);
            for (const auto &[q, t] : m) { qt.push_back(q); qt.push_back(t); }
            offsets.push_back((int64_t)(qt.size() / 2));
        }
        check(rcn_match_lists_upload(ctx_, (int32_t)(pairs.size() / 2), pairs.data(), offsets.data(), qt.empty() ? nullptr : qt.data(), 0), "uploadContainers");
    }

    // selected == nullptr: every image
    template <class FeatureMatches>
    std::vector<Track> build(const std::unordered_map<int, std::vector<FeaturePtr<>>> &features, const FeatureMatches &featureMatches,
                             const std::vector<int> *selected = nullptr)
    {
        uploadContainers(features, featureMatches);
        const int64_t nodes = nodeCount("build");
        const int32_t capT = (int32_t)(nodes / 2), capO = (int32_t)nodes;
        std::vector<int32_t> off((size_t)capT + 1), img((size_t)capO + 1), feat((size_t)capO + 1), selImg, selCam;
        if (selected)
            for (size_t k = 0; k < selected->size(); ++k) { selImg.push_back((*selected)[k]); selCam.push_back((int32_t)k); }
        int32_t counts[2] = {0, 0};
        check(rcn_tracks_build(ctx_, &options, (int32_t)selImg.size(), selImg.empty() ? nullptr : selImg.data(), selCam.empty() ? nullptr : selCam.data(),
                               capT, capO, counts, off.data(), img.data(), feat.data(), nullptr, nullptr, nullptr, nullptr), "build");
        std::vector<Track> tracks((size_t)counts[0]);
        for (int32_t j = 0; j < counts[0]; ++j)
            for (int32_t o = off[(size_t)j]; o < off[(size_t)j + 1]; ++o) tracks[(size_t)j].emplace_back(img[(size_t)o], feat[(size_t)o]);
        return tracks;
    }

    // imgCam: (image, camera row) of the images whose observations are wanted (rcn_triangulate_device's rows of poses / intrinsics).
    // The containers must be resident (uploadContainers, or a build).  Waits for the counts only.
    DeviceTracks buildDevice(const std::vector<std::pair<int, int>> &imgCam)
    {
        if (imgCam.empty()) throw std::invalid_argument("TrackBuilder::buildDevice: no images selected");
        const int64_t nodes = nodeCount("buildDevice");
        DeviceTracks d;
        d.capTracks = (int32_t)(nodes / 2);
        d.capObs = (int32_t)nodes;
        const size_t wOff = pad((size_t)d.capTracks + 1), wObs = pad((size_t)d.capObs + 1), words = 64 + wOff + 5 * wObs;
        if (words > devWords_) {
            if (dev_) (void)hipFree(dev_);
            dev_ = nullptr; devWords_ = 0;
            if (hipMalloc(reinterpret_cast<void **>(&dev_), 4 * words) != 0) throw std::runtime_error("TrackBuilder::buildDevice: hipMalloc failed");
            devWords_ = words;
        }
        int32_t *counts = dev_;
        d.trkOff = dev_ + 64; d.obsImg = d.trkOff + wOff; d.obsFeat = d.obsImg + wObs; d.obsCam = d.obsFeat + wObs; d.obsXy = d.obsCam + wObs;
        std::vector<int32_t> selImg, selCam;
        for (const auto &[i, c] : imgCam) { selImg.push_back(i); selCam.push_back(c); }
        check(rcn_tracks_build_device(ctx_, &options, (int32_t)selImg.size(), selImg.data(), selCam.data(), d.capTracks, d.capObs, counts, d.trkOff,
                                      d.obsImg, d.obsFeat, d.obsCam, d.obsXy, nullptr, nullptr), "buildDevice");
        check(rcn_synchronize(ctx_), "buildDevice");
        int32_t h[2] = {0, 0};
        if (hipMemcpy(h, counts, sizeof(h), kMemcpyDeviceToHost) != 0) throw std::runtime_error("TrackBuilder::buildDevice: hipMemcpy failed");
        d.nTracks = h[0]; d.nObs = h[1];
        return d;
    }

private:
    static constexpr int kMemcpyDeviceToHost = 2;   // hipMemcpyKind
    static size_t pad(size_t words) { return (words + 63) / 64 * 64; }
    void check(int rc, const char *who) const
    {
        if (rc != RCN_OK) throw std::runtime_error(std::string("TrackBuilder::") + who + ": " + rcn_last_error(ctx_));
    }
    int64_t nodeCount(const char *who)
    {
        int32_t n = 0;
        check(rcn_tracks_layout(ctx_, nullptr, nullptr, &n), who);
        std::vector<int64_t> off((size_t)n + 1);
        std::vector<int32_t> ids((size_t)n + 1);
        check(rcn_tracks_layout(ctx_, ids.data(), off.data(), &n), who);
        return off[(size_t)n];
    }

    rcn_ctx *ctx_ = nullptr;
    bool owned_ = true;
    int32_t *dev_ = nullptr;       // buildDevice's block, grown when a build needs more
    size_t devWords_ = 0;
};

}  // namespace reconstructor::Core
