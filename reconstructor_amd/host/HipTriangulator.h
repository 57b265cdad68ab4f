// HipTriangulator.h -- SequentialReconstructor::triangulateMultiView, ::triangulateInitialPair and
// ::triangulateMatchedLandmarks (SequentialReconstructor.cpp:396-489, :377-394, :492-556) over the reference's own
// containers, with the triangulation itself handed to rcn_triangulate (include/rcn.h) as ONE batch per call.
// In the reference these are private members working on `features`, `landmarks`, `imgIdx2camPose`,
// `imgIdx2camIntrinsics`, `registeredImages`, `imgMatches`, `featureMatches`; here the same containers are passed in.
// Pose matrices: anything indexable as M(r,c).  Landmark colour and initialLandmark are not carried (rcn_types.h has
// neither).
//
// Why one batch gives the reference's result:
//   - triangulateInitialPair triangulates every match of the pair: nothing depends on an earlier call.
//   - step 3 of triangulateMatchedLandmarks: a call changes only the landmarkId of its own two features; the new image's
//     feature is not looked at again, and the partner cannot be another candidate's partner (every pair's match map is
//     injective).  The break of :548 follows the call whether or not the track is accepted.  So the candidates are the
//     same whatever the earlier calls decided, and are collected first, in the containers' own iteration order.
//   - step 1 (:497-512) is sequential when a feature is listed twice, and it is a few flops per 2D-3D match: it stays
//     on the host, in the reference's order.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/rcn.h"
#include "rcn_types.h"

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
    ~Triangulator() { if (owned_) rcn_destroy(ctx_); }
    Triangulator(const Triangulator &) = delete;
    Triangulator &operator=(const Triangulator &) = delete;

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
        std::vector<Track> batch;                                                         // step 3, :518-553
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
        triangulateMultiView(batch, features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics);
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

private:
    rcn_ctx *ctx_;
    bool owned_;
};

}  // namespace reconstructor::Core
