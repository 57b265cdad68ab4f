// HipGeometricFilter.h -- GeometricFilter::estimateFundamental with the reference's signature
// (GeometricFilter.h:33-35, GeometricFilter.cpp:39-61), the RANSAC / LMedS search handed to
// rcn_fmat_filter (include/rcn.h) instead of cv::findFundamentalMat.
// estimateEssential (GeometricFilter.h, GeometricFilter.cpp:10-37) goes to rcn_twoview_init instead of cv::findEssentialMat: it
// returns E (unit Frobenius norm, normalised coordinates) and -- unlike the reference, which reads an empty inliersCV there
// (:25-33) -- fills the mask.  The call also recovers the pose (the canonical flow is one search followed by the recovery on
// its own mask): lastPose34() holds the rows of [R | t] for essentialMatToPose's caller.
// Return value: Eigen::Matrix3d in the reference; Mat3d here (M(r,c)).  Zero when no model was found
// (GeometricFilter.cpp:50-53), else the winning 7-point hypothesis -- OpenCV returns an 8-point refit
// on the inliers, which no caller of the reference reads (SequentialReconstructor.cpp:250).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rcn.h"
#include "rcn_types.h"

namespace reconstructor::Core {

struct Mat3d {
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double &operator()(int r, int c) { return m[3 * r + c]; }
    double operator()(int r, int c) const { return m[3 * r + c]; }
};

class GeometricFilter {
public:
    explicit GeometricFilter(rcn_ctx *ctx = nullptr) : ctx_(ctx), owned_(false)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("GeometricFilter: no usable gfx950 device");
            owned_ = true;
        }
    }
    ~GeometricFilter() { if (owned_) rcn_destroy(ctx_); }
    GeometricFilter(const GeometricFilter &) = delete;
    GeometricFilter &operator=(const GeometricFilter &) = delete;

    // inlierMatchIds is appended to, one flag per match, exactly when a model was found
    // (writeInliersToVector, utils.cpp:328-343); it stays empty otherwise and the caller drops the pair.
    Mat3d estimateFundamental(const std::vector<FeaturePtr<>> &features1, const std::vector<FeaturePtr<>> &features2,
                              std::vector<bool> &inlierMatchIds)
    {
        const size_t n = features1.size();
        if (features2.size() != n) throw std::invalid_argument("estimateFundamental: one feature of image 2 per feature of image 1");
        std::vector<int32_t> xy1(2 * n + 2), xy2(2 * n + 2);
        for (size_t i = 0; i < n; ++i) {      // featuresToCvPoints, utils.cpp:165-177
            xy1[2 * i] = features1[i]->featCoord.x; xy1[2 * i + 1] = features1[i]->featCoord.y;
            xy2[2 * i] = features2[i]->featCoord.x; xy2[2 * i + 1] = features2[i]->featCoord.y;
        }
        std::vector<uint8_t> mask(n + 1);
        int32_t count = 0;
        Mat3d F;
        if (rcn_fmat_filter(ctx_, xy1.data(), xy2.data(), (int32_t)n, mask.data(), &count, F.m) != RCN_OK)
            throw std::runtime_error(std::string("estimateFundamental: ") + rcn_last_error(ctx_));
        if (count == -1 || count == -2) return Mat3d();       // cv::findFundamentalMat returns an empty matrix below 7 points too
        for (size_t i = 0; i < n; ++i) inlierMatchIds.push_back(mask[i] != 0);
        return F;
    }

    // inlierMatchIds is appended to, one flag per match, exactly when a model was found; a zero matrix otherwise.
    Mat3d estimateEssential(const std::vector<FeaturePtr<>> &features1, const std::vector<FeaturePtr<>> &features2,
                            const PinholeCamera &intrinsics1, const PinholeCamera &intrinsics2, std::vector<bool> &inlierMatchIds)
    {
        const size_t n = features1.size();
        if (features2.size() != n) throw std::invalid_argument("estimateEssential: one feature of image 2 per feature of image 1");
        std::vector<int32_t> xy1(2 * n + 2), xy2(2 * n + 2);
        for (size_t i = 0; i < n; ++i) {      // featuresToCvPoints, utils.cpp:165-177
            xy1[2 * i] = features1[i]->featCoord.x; xy1[2 * i + 1] = features1[i]->featCoord.y;
            xy2[2 * i] = features2[i]->featCoord.x; xy2[2 * i + 1] = features2[i]->featCoord.y;
        }
        const double K1[6] = {intrinsics1.fX, intrinsics1.fY, intrinsics1.cX, intrinsics1.cY, intrinsics1.k1, intrinsics1.k2};
        const double K2[6] = {intrinsics2.fX, intrinsics2.fY, intrinsics2.cX, intrinsics2.cY, intrinsics2.k1, intrinsics2.k2};
        const int64_t off[2] = {0, (int64_t)n};
        std::vector<uint8_t> mask(n + 1), cmask(n + 1);
        Mat3d E;
        lastCount_[0] = lastCount_[1] = 0;
        if (rcn_twoview_init(ctx_, 1, off, xy1.data(), xy2.data(), K1, K2, nullptr, E.m, lastPose_, mask.data(), cmask.data(), lastCount_,
                             nullptr) != RCN_OK)
            throw std::runtime_error(std::string("estimateEssential: ") + rcn_last_error(ctx_));
        if (lastCount_[0] < 0) return Mat3d();
        for (size_t i = 0; i < n; ++i) inlierMatchIds.push_back(mask[i] != 0);
        return E;
    }
    // cv::findHomography(pts1, pts2, cv::RANSAC, 3.0, mask, 2000, 0.995) through rcn_homography_ransac, beside the two above:
    // inlierMatchIds is appended to, one flag per match, exactly when a model was found; a zero matrix otherwise.
    // lastInliers() is the number of inliers of the returned H (-1 / -2: none).
    Mat3d estimateHomography(const std::vector<FeaturePtr<>> &features1, const std::vector<FeaturePtr<>> &features2,
                             std::vector<bool> &inlierMatchIds)
    {
        const size_t n = features1.size();
        if (features2.size() != n) throw std::invalid_argument("estimateHomography: one feature of image 2 per feature of image 1");
        std::vector<int32_t> xy1(2 * n + 2), xy2(2 * n + 2);
        for (size_t i = 0; i < n; ++i) {      // featuresToCvPoints, utils.cpp:165-177
            xy1[2 * i] = features1[i]->featCoord.x; xy1[2 * i + 1] = features1[i]->featCoord.y;
            xy2[2 * i] = features2[i]->featCoord.x; xy2[2 * i + 1] = features2[i]->featCoord.y;
        }
        const int64_t off[2] = {0, (int64_t)n};
        std::vector<uint8_t> mask(n + 1);
        Mat3d H;
        lastCount_[0] = lastCount_[1] = 0;
        for (double &p : lastPose_) p = 0.0;
        if (rcn_homography_ransac(ctx_, 1, off, xy1.data(), xy2.data(), nullptr, H.m, mask.data(), lastCount_, nullptr) != RCN_OK)
            throw std::runtime_error(std::string("estimateHomography: ") + rcn_last_error(ctx_));
        if (lastCount_[0] < 0) return Mat3d();
        for (size_t i = 0; i < n; ++i) inlierMatchIds.push_back(mask[i] != 0);
        return H;
    }
    // of the last estimateEssential: rows of [R | t] of the second camera (zeros when there was no model), the number of
    // inliers (-1 / -2: none) and of inliers in front of both cameras
    const double *lastPose34() const { return lastPose_; }
    int lastInliers() const { return lastCount_[0]; }
    int lastInFront() const { return lastCount_[1]; }

private:
    rcn_ctx *ctx_;
    bool owned_;
    double lastPose_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int32_t lastCount_[2] = {-2, 0};
};

}  // namespace reconstructor::Core
