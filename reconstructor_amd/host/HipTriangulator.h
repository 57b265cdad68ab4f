// HipTriangulator.h -- SequentialReconstructor::triangulateMultiView, ::triangulateInitialPair and
// ::triangulateMatchedLandmarks (SequentialReconstructor.cpp:396-489, :377-394, :492-556) over the reference's own
// containers, with the triangulation itself handed to rcn_triangulate (include/rcn.h) as ONE batch per call.
// In the reference these are private members working on `features`, `landmarks`, `imgIdx2camPose`,
// `imgIdx2camIntrinsics`, `registeredImages`, `imgMatches`, `featureMatches`; here the same containers are passed in.
// Pose matrices: anything indexable as M(r,c).  An accepted landmark takes the colour of the first entry of its track
// (:429-433), read from the caller's features: zero when they carry none (HipImagePrep.h's extractFeatureColors fills
// them).  initialLandmark is not carried (rcn_types.h does not have it).
//
// Why one batch gives the reference's result:
//   - triangulateInitialPair triangulates every match of the pair: nothing depends on an earlier call.
//   - step 3 of triangulateMatchedLandmarks: a call changes only the landmarkId of its own two features; the new image's
//     feature is not looked at again, and the partner cannot be another candidate's partner (every pair's match map is
//     injective).  The break of :548 follows the call whether or not the track is accepted.  So the candidates are the
//     same whatever the earlier calls decided, and are collected first, in the containers' own iteration order.
//   - step 1 (:497-512) is sequential when a feature is listed twice, and it is a few flops per 2D-3D match: it stays
//     on the host, in the reference's order.
//
// triangulateMatchedLandmarksDevice runs step 3 without the host walk: the candidates come from the
// match lists, the pixel coordinates and the landmark-id table resident in the ctx (uploadContainers puts them there once),
// are triangulated where they are, and only the accepted tracks come back into the caller's containers.
#pragma once
#include <algorithm>
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

class Triangulator {
public:
    using Track = std::vector<std::pair<int, int>>;     // (imgIdx, featIdx), the reference's matchedImgIdFeatId

    explicit Triangulator(rcn_ctx *ctx = nullptr) : ctx_(ctx), owned_(false)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("Triangulator: no usable gfx950 device");
            owned_ = true;
        }
    }
    ~Triangulator()
    {
        if (dev_) (void)hipFree(dev_);
        if (owned_) rcn_destroy(ctx_);
    }
    Triangulator(const Triangulator &) = delete;
    Triangulator &operator=(const Triangulator &) = delete;

    rcn_ctx *ctx() const { return ctx_; }

    double maxProjectionError = 4.0;      // SequentialReconstructor.h:256
    double minTriangulationAngle = 1.0;   // SequentialReconstructor.h:257

    // triangulateMultiView for every track of the batch: accepted tracks are appended to `landmarks` in batch order and
    // their features get the new landmark's index.  Returns the status per track (0 accepted, 1 singular value 0 or
    // world z not > 0, 2 reprojection, 3 angle).
    template <class Pose4>
    std::vector<uint8_t> triangulateMultiView(const std::vector<Track> &batch,
                                              std::unordered_map<int, std::vector<FeaturePtr<>>> &features,
                                              std::vector<Landmark> &landmarks,
                                              std::unordered_map<int, Pose4> &imgIdx2camPose,
                                              std::unordered_map<int, PinholeCamera> &imgIdx2camIntrinsics)
    {
        std::unordered_map<int, int> local;              // image index -> row in the flat camera arrays
        std::vector<double> poses, intr;
        std::vector<int32_t> off(batch.size() + 1, 0), cam, xy;
        for (size_t j = 0; j < batch.size(); ++j) {
            for (const auto &[imgIdx, featIdx] : batch[j]) {
                auto it = local.find(imgIdx);
                if (it == local.end()) {
                    it = local.emplace(imgIdx, (int)local.size()).first;
                    const Pose4 &T = imgIdx2camPose.at(imgIdx);
                    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) poses.push_back(T(r, c));
                    const PinholeCamera &k = imgIdx2camIntrinsics.at(imgIdx);
                    const double kk[6] = {k.fX, k.fY, k.cX, k.cY, k.k1, k.k2};
                    intr.insert(intr.end(), kk, kk + 6);
                }
                const auto &feat = features.at(imgIdx).at(featIdx);
                cam.push_back(it->second);
                xy.push_back(feat->featCoord.x); xy.push_back(feat->featCoord.y);
            }
            off[j + 1] = (int32_t)cam.size();
        }
        std::vector<double> X(3 * batch.size() + 3);
        std::vector<uint8_t> status(batch.size() + 1);
        rcn_triangulation_problem pb = {(int32_t)local.size(), (int32_t)batch.size(), (int32_t)cam.size(), 0,
                                        poses.data(), intr.data(), off.data(), cam.data(), xy.data()};
        if (rcn_triangulate(ctx_, &pb, maxProjectionError, minTriangulationAngle, X.data(), status.data(), nullptr) != RCN_OK)
            throw std::runtime_error(std::string("triangulateMultiView: ") + rcn_last_error(ctx_));
        for (size_t j = 0; j < batch.size(); ++j) {
            if (status[j] != 0) continue;
            Landmark lm(X[3 * j], X[3 * j + 1], X[3 * j + 2]);
            if (!batch[j].empty()) colourOf(lm, *features.at(batch[j].front().first).at(batch[j].front().second));
            for (const auto &[imgIdx, featIdx] : batch[j]) {
                lm.triangulatedFeatures.emplace_back(imgIdx, featIdx);
                features.at(imgIdx).at(featIdx)->landmarkId = (int)landmarks.size();      // :481-487
            }
            landmarks.push_back(std::move(lm));
        }
        status.resize(batch.size());
        return status;
    }

    // :377-394: every match of featureMatches[(imgIdx1, imgIdx2)], in the map's own iteration order
    template <class Pose4, class FeatureMatches>
    void triangulateInitialPair(int imgIdx1, int imgIdx2,
                                std::unordered_map<int, std::vector<FeaturePtr<>>> &features, std::vector<Landmark> &landmarks,
                                std::unordered_map<int, Pose4> &imgIdx2camPose,
                                std::unordered_map<int, PinholeCamera> &imgIdx2camIntrinsics, FeatureMatches &featureMatches)
    {
        std::vector<Track> batch;
        for (const auto &[featIdx1, featIdx2] : featureMatches[std::make_pair(imgIdx1, imgIdx2)])
            batch.push_back({{imgIdx1, featIdx1}, {imgIdx2, featIdx2}});
        triangulateMultiView(batch, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics);
    }

    // :492-556: step 1 on the host in the reference's order, step 3 as one batch (candidates in feature order, each with
    // the first registered image -- registeredImages' own iteration order -- that qualifies)
    template <class Pose4, class FeatureMatches>
    void triangulateMatchedLandmarks(int imgIdx, const std::vector<int> &featureIds, const std::vector<int> &landmarkIds,
                                     std::unordered_map<int, std::vector<FeaturePtr<>>> &features, std::vector<Landmark> &landmarks,
                                     std::unordered_map<int, Pose4> &imgIdx2camPose,
                                     std::unordered_map<int, PinholeCamera> &imgIdx2camIntrinsics,
                                     std::unordered_map<int, bool> &registeredImages,
                                     std::unordered_map<int, std::vector<int>> &imgMatches, FeatureMatches &featureMatches)
    {
        const Pose4 &T = imgIdx2camPose.at(imgIdx);
        const PinholeCamera &K = imgIdx2camIntrinsics.at(imgIdx);
        for (size_t pairIdx = 0; pairIdx < featureIds.size(); ++pairIdx) {                 // step 1, :497-512
            const int featIdx = featureIds[pairIdx], landmarkId = landmarkIds[pairIdx];
            const Landmark &lm = landmarks[landmarkId];
            double depth;
            const double residualTotal = projectionError(T, K, lm.x, lm.y, lm.z, features.at(imgIdx).at(featIdx)->featCoord, &depth);
            if (depth > 0 && residualTotal < maxProjectionError && features[imgIdx][featIdx]->landmarkId == -1) {
                landmarks[landmarkId].triangulatedFeatures.emplace_back(imgIdx, featIdx);
                features[imgIdx][featIdx]->landmarkId = landmarkId;
            }
        }
        const std::vector<Track> batch = newViewTracks(imgIdx, features, registeredImages, imgMatches, featureMatches);   // step 3, :518-553
        triangulateMultiView(batch, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics);
    }

    // step 3's walk (:518-553): for every feature of imgIdx that is not a landmark, the first registered image matched with
    // imgIdx whose pair map holds the feature and whose partner is not a landmark either
    template <class FeatureMatches>
    static std::vector<Track> newViewTracks(int imgIdx, std::unordered_map<int, std::vector<FeaturePtr<>>> &features,
                                            std::unordered_map<int, bool> &registeredImages,
                                            std::unordered_map<int, std::vector<int>> &imgMatches, FeatureMatches &featureMatches)
    {
        std::vector<Track> batch;
        const auto &imgFeats = features[imgIdx];
        const auto &curImgMatches = imgMatches[imgIdx];
        for (size_t featIdx = 0; featIdx < imgFeats.size(); ++featIdx) {
            if (imgFeats[featIdx]->landmarkId != -1) continue;
            for (const auto &[regImgIdx, regStatus] : registeredImages) {
                if (!regStatus || std::find(curImgMatches.begin(), curImgMatches.end(), regImgIdx) == curImgMatches.end()) continue;
                const auto pm = featureMatches.find(std::make_pair(imgIdx, regImgIdx));
                if (pm == featureMatches.end()) continue;
                const auto m = pm->second.find((int)featIdx);
                if (m == pm->second.end()) continue;
                if (features[regImgIdx][m->second]->landmarkId == -1) {
                    batch.push_back({{regImgIdx, m->second}, {imgIdx, (int)featIdx}});
                    break;
                }
            }
        }
        return batch;
    }

    // What step 3 on the device reads, made resident in the ctx: every image's pixel coordinates, every directed list of
    // featureMatches as given (no mirroring) and the landmark-id table filled from features[*][*]->landmarkId.  Call it once
    // the matches are final; triangulateMatchedLandmarksDevice keeps the table current from then on, and whoever else
    // changes a landmarkId (removeOutlierLandmarks) tells the table with rcn_landmark_ids_set.
    template <class FeatureMatches>
    void uploadContainers(std::unordered_map<int, std::vector<FeaturePtr<>>> &features, FeatureMatches &featureMatches)
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
        check(rcn_landmark_ids_reset(ctx_), "uploadContainers");
        std::vector<int32_t> img, feat, id;
        for (const auto &[imgIdx, feats] : features)
            for (size_t f = 0; f < feats.size(); ++f)
                if (feats[f]->landmarkId != -1) { img.push_back(imgIdx); feat.push_back((int32_t)f); id.push_back(feats[f]->landmarkId); }
        check(rcn_landmark_ids_set(ctx_, (int32_t)img.size(), img.data(), feat.data(), id.data()), "uploadContainers");
    }

    // :492-556 with step 3 on the device: step 1 as triangulateMatchedLandmarks runs it (its attachments go into the table),
    // then the candidates, their triangulation and the new landmarks' ids in one asynchronous call
    // (rcn_new_view_triangulate_device); `landmarks`, triangulatedFeatures and every landmarkId end up exactly as the host
    // method leaves them.  Needs uploadContainers.  Returns the status per candidate, in feature order.
    template <class Pose4, class FeatureMatches>
    std::vector<uint8_t> triangulateMatchedLandmarksDevice(int imgIdx, const std::vector<int> &featureIds, const std::vector<int> &landmarkIds,
                                                           std::unordered_map<int, std::vector<FeaturePtr<>>> &features, std::vector<Landmark> &landmarks,
                                                           std::unordered_map<int, Pose4> &imgIdx2camPose,
                                                           std::unordered_map<int, PinholeCamera> &imgIdx2camIntrinsics,
                                                           std::unordered_map<int, bool> &registeredImages,
                                                           std::unordered_map<int, std::vector<int>> &imgMatches, FeatureMatches &featureMatches)
    {
        const char *who = "triangulateMatchedLandmarksDevice";
        const Pose4 &T = imgIdx2camPose.at(imgIdx);
        const PinholeCamera &K = imgIdx2camIntrinsics.at(imgIdx);
        std::vector<int32_t> setImg, setFeat, setId;
        for (size_t pairIdx = 0; pairIdx < featureIds.size(); ++pairIdx) {                 // step 1, :497-512
            const int featIdx = featureIds[pairIdx], landmarkId = landmarkIds[pairIdx];
            const Landmark &lm = landmarks[landmarkId];
            double depth;
            const double residualTotal = projectionError(T, K, lm.x, lm.y, lm.z, features.at(imgIdx).at(featIdx)->featCoord, &depth);
            if (depth > 0 && residualTotal < maxProjectionError && features[imgIdx][featIdx]->landmarkId == -1) {
                landmarks[landmarkId].triangulatedFeatures.emplace_back(imgIdx, featIdx);
                features[imgIdx][featIdx]->landmarkId = landmarkId;
                setImg.push_back(imgIdx); setFeat.push_back(featIdx); setId.push_back(landmarkId);
            }
        }
        check(rcn_landmark_ids_set(ctx_, (int32_t)setImg.size(), setImg.data(), setFeat.data(), setId.data()), who);
        // the registered images the walk would look at, in registeredImages' own iteration order; camera row 0 is imgIdx
        std::vector<int32_t> reg, regCam;
        std::vector<double> poses, intr;
        auto addCamera = [&](int img) {
            const Pose4 &P = imgIdx2camPose.at(img);
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) poses.push_back(P(r, c));
            const PinholeCamera &k = imgIdx2camIntrinsics.at(img);
            const double kk[6] = {k.fX, k.fY, k.cX, k.cY, k.k1, k.k2};
            intr.insert(intr.end(), kk, kk + 6);
        };
        addCamera(imgIdx);
        const auto &curImgMatches = imgMatches[imgIdx];
        for (const auto &[regImgIdx, regStatus] : registeredImages) {
            if (!regStatus || std::find(curImgMatches.begin(), curImgMatches.end(), regImgIdx) == curImgMatches.end()) continue;
            if (featureMatches.find(std::make_pair(imgIdx, regImgIdx)) == featureMatches.end()) continue;
            regCam.push_back((int32_t)reg.size() + 1);
            reg.push_back(regImgIdx);
            addCamera(regImgIdx);
        }
        if (reg.empty()) return {};
        const int32_t cap = (int32_t)features[imgIdx].size(), nc = (int32_t)reg.size() + 1;
        if (cap == 0) return {};
        // one device block: poses | intrinsics | xyz || n_tracks, n_accepted, 2 words | trk_src | status || trk_off | obs_cam | obs_xy
        auto al = [](size_t b) { return (b + 255) / 256 * 256; };
        const size_t n = (size_t)cap;
        const size_t oPose = 0, oIntr = oPose + al(96 * (size_t)nc), oXyz = oIntr + al(48 * (size_t)nc), oBack = oXyz + al(24 * n);
        const size_t oSrc = oBack + 16, oSt = oSrc + 12 * n, backBytes = 16 + 13 * n;
        const size_t oOff = oBack + al(backBytes), oCam = oOff + al(4 * (n + 1)), oXy = oCam + al(8 * n), total = oXy + al(16 * n);
        if (total > devBytes_) {
            if (dev_) (void)hipFree(dev_);
            dev_ = nullptr; devBytes_ = 0;
            if (hipMalloc((void **)&dev_, total + total / 2)) throw std::runtime_error(std::string(who) + ": out of device memory");
            devBytes_ = total + total / 2;
        }
        char *d = dev_;
        if (hipMemcpy(d + oPose, poses.data(), poses.size() * sizeof(double), kMemcpyHostToDevice) ||
            hipMemcpy(d + oIntr, intr.data(), intr.size() * sizeof(double), kMemcpyHostToDevice))
            throw std::runtime_error(std::string(who) + ": copy to the device failed");
        int32_t *hdr = reinterpret_cast<int32_t *>(d + oBack);
        check(rcn_new_view_triangulate_device(ctx_, imgIdx, (int32_t)reg.size(), reg.data(), 0, regCam.data(), nc,
                                              reinterpret_cast<const double *>(d + oPose), reinterpret_cast<const double *>(d + oIntr),
                                              maxProjectionError, minTriangulationAngle, (int32_t)landmarks.size(), cap, hdr,
                                              reinterpret_cast<int32_t *>(d + oOff), reinterpret_cast<int32_t *>(d + oCam),
                                              reinterpret_cast<int32_t *>(d + oXy), reinterpret_cast<int32_t *>(d + oSrc),
                                              reinterpret_cast<double *>(d + oXyz), reinterpret_cast<uint8_t *>(d + oSt), nullptr, 0, hdr + 1), who);
        check(rcn_synchronize(ctx_), who);
        std::vector<char> back(backBytes);
        std::vector<double> X(3 * n);
        if (hipMemcpy(back.data(), d + oBack, backBytes, kMemcpyDeviceToHost) || hipMemcpy(X.data(), d + oXyz, 24 * n, kMemcpyDeviceToHost))
            throw std::runtime_error(std::string(who) + ": copy from the device failed");
        const int32_t *h = reinterpret_cast<const int32_t *>(back.data()), *src = h + 4;
        const uint8_t *st = reinterpret_cast<const uint8_t *>(back.data() + 16 + 12 * n);
        const int32_t nTracks = h[0];
        if (nTracks < 0 || nTracks > cap) throw std::runtime_error(std::string(who) + ": candidate count out of range");
        for (int32_t j = 0; j < nTracks; ++j) {
            if (st[j] != 0) continue;
            Landmark lm(X[3 * (size_t)j], X[3 * (size_t)j + 1], X[3 * (size_t)j + 2]);
            const int regImgIdx = src[3 * (size_t)j], regFeat = src[3 * (size_t)j + 1], featIdx = src[3 * (size_t)j + 2];
            colourOf(lm, *features.at(regImgIdx).at(regFeat));
            lm.triangulatedFeatures.emplace_back(regImgIdx, regFeat);                       // matchedImgIdFeatId order, :543-544
            lm.triangulatedFeatures.emplace_back(imgIdx, featIdx);
            features.at(regImgIdx).at(regFeat)->landmarkId = (int)landmarks.size();          // :481-487; the table holds the same
            features.at(imgIdx).at(featIdx)->landmarkId = (int)landmarks.size();
            landmarks.push_back(std::move(lm));
        }
        return std::vector<uint8_t>(st, st + nTracks);
    }

    // :429-433: a landmark is coloured by the first feature of its track
    static void colourOf(Landmark &lm, const Feature<> &first)
    {
        lm.red = first.featColor.red; lm.green = first.featColor.green; lm.blue = first.featColor.blue;
    }

    // getLandmarkLocalCoords + calcProjectionError (:842-867) in the operation order of the device kernels (camgeom.h)
    template <class Pose4>
    static double projectionError(const Pose4 &T, const PinholeCamera &K, double X, double Y, double Z, const FeatCoord<> &c, double *depth)
    {
        double l[3];
        for (int i = 0; i < 3; ++i) l[i] = ((T(i, 0) * X + T(i, 1) * Y) + T(i, 2) * Z) + T(i, 3);
        double x = l[0] / l[2], y = l[1] / l[2];
        const double radius = x * x + y * y;
        const double distortion = K.k1 * radius + (K.k2 * radius) * radius;
        x += distortion;
        y += distortion;
        const double u = K.fX * x + K.cX, v = K.fY * y + K.cY;
        *depth = l[2];
        return std::abs(u - (double)c.x) + std::abs(v - (double)c.y);
    }

    static constexpr int kMemcpyHostToDevice = 1, kMemcpyDeviceToHost = 2;   // hipMemcpyKind

private:
    void check(int rc, const char *who) const
    {
        if (rc != RCN_OK) throw std::runtime_error(std::string(who) + ": " + rcn_last_error(ctx_));
    }

    rcn_ctx *ctx_;
    bool owned_;
    char *dev_ = nullptr;          // triangulateMatchedLandmarksDevice's device block, grown when a view needs more
    size_t devBytes_ = 0;
};

}  // namespace reconstructor::Core
