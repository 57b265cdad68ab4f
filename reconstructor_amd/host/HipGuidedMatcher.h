// HipGuidedMatcher.h -- guided matching of one image pair behind the reference's boundary types, backed by librcn.so (include/rcn.h,
// rcn_match_pair_guided).
//
// The reference has no such stage: its pair loop matches every pair without a constraint and filters afterwards
// (SequentialReconstructor.cpp:232-275).  Once GeometricFilter has a pair's fundamental matrix, `GuidedMatcher::matchFeatures` matches
// the pair again inside the epipolar band of that matrix and fills the same std::map<int, int> the loop stores; a maintainer calls it
// between the filter and the store of the pair's matches -- see INTEGRATION.md.
//   F        9 doubles, row-major, the filter's convention: x2^T F x1 = 0 with x1 a keypoint of features1 (featCoord), x2 one of features2
//   options  ratio, max_error_px, max_distance, cross_check as rcn_guided_options
// Re-entrant like the other plugins: callers are serialised.
#pragma once
#include <mutex>
#include <stdexcept>
#include <string>

#include "../../include/rcn.h"
#include "HipFeatureMatcher.h"
#include "rcn_types.h"

namespace reconstructor::Core {

class GuidedMatcher {
public:
    explicit GuidedMatcher(int device = 0) : owned_(true)
    {
        if (rcn_create(device, &ctx_) != RCN_OK) throw std::runtime_error("GuidedMatcher: no usable gfx950 device");
        rcn_guided_default_options(&options);
    }
    explicit GuidedMatcher(rcn_ctx *shared) : ctx_(shared), owned_(false)
    {
        if (!ctx_) throw std::runtime_error("GuidedMatcher: null ctx");
        rcn_guided_default_options(&options);
    }
    ~GuidedMatcher() { if (owned_) rcn_destroy(ctx_); }
    GuidedMatcher(const GuidedMatcher &) = delete;
    GuidedMatcher &operator=(const GuidedMatcher &) = delete;

    void matchFeatures(const std::vector<FeaturePtr<>> &features1, const std::vector<FeaturePtr<>> &features2, const double F[9],
                       std::map<int, int> &matches)
    {
        if (features1.empty() || features2.empty()) return;
        if (!F) throw std::invalid_argument("GuidedMatcher::matchFeatures: null F");
        int D1 = 0, D2 = 0;
        const std::vector<float> q = featDescToDense(features1, D1), t = featDescToDense(features2, D2);
        if (D1 != D2) throw std::runtime_error("descriptor lengths differ");
        const std::vector<int32_t> xy1 = coords(features1), xy2 = coords(features2);
        std::vector<int32_t> out(features1.size(), -1);
        int32_t count = 0;
        std::lock_guard<std::mutex> lk(mu_);
        const int rc = rcn_match_pair_guided(ctx_, q.data(), (int32_t)features1.size(), xy1.data(), t.data(), (int32_t)features2.size(), xy2.data(), D1, F,
                                             &options, out.data(), &count);
        if (rc != RCN_OK) throw std::runtime_error(std::string("GuidedMatcher::matchFeatures: ") + rcn_last_error(ctx_));
        for (size_t i = 0; i < out.size(); ++i)
            if (out[i] >= 0) matches[(int)i] = out[i];
    }
    rcn_ctx *context() { return ctx_; }

    rcn_guided_options options;     // 0.7, 3 px, no distance limit, one-way

private:
    static std::vector<int32_t> coords(const std::vector<FeaturePtr<>> &f)
    {
        std::vector<int32_t> xy(2 * f.size());
        for (size_t i = 0; i < f.size(); ++i) { xy[2 * i] = f[i]->featCoord.x; xy[2 * i + 1] = f[i]->featCoord.y; }
        return xy;
    }
    rcn_ctx *ctx_ = nullptr;
    bool owned_ = true;
    std::mutex mu_;
};

}  // namespace reconstructor::Core
