// HipImageMatcher.h -- an ImageMatcher (ImageMatcher.h:14-22) that retrieves, over the C ABI (rcn_retr_*, include/rcn.h).
//
// The reference ships FakeImgMatcher (ImageMatcher.cpp:6-23: every image with every other) and leaves the real one open.  This
// one ranks the images by a VLAD global descriptor built from their local descriptors and keeps the topK neighbours of each:
//   match        the reference's signature.  Slots are the keys of `features` in ascending order; the descriptors are packed
//                [n][K][D] (K the largest image, rows past an image's own count unused) and uploaded once; the codebook is
//                trained on them unless one was given to the constructor; imgMatches[id] receives the ascending ids of the
//                partners of id.  The relation is symmetric, and with topK >= n - 1 it is what FakeImgMatcher fills.
//   matchDevice  the same for a block that is in HBM already (the slot of rcn_shard_reserve, a detector's output): returns the
//                pair list (first id, second id, ...) in the order rcn_match_grid and HipPairGridDriver take
#pragma once
#include <algorithm>
#include <cstdint>
#include <filesystem>
#include <stdexcept>
#include <string>
#include <unordered_map>
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

class HipImageMatcher : public ImageMatcher {
public:
    static constexpr int kMemcpyHostToDevice = 1;   // hipMemcpyKind

    // trains a codebook of nCentroids on the descriptors of every call
    explicit HipImageMatcher(rcn_ctx *ctx = nullptr, int topK = 20, int nCentroids = 64, int iterations = 10) : ctx_(ctx), topK_(topK)
    {
        acquire();
        rcn_retr_default_options(&opt_);
        opt_.n_centroids = nCentroids; opt_.iterations = iterations; opt_.top_k = topK;
    }
    // the caller's own codebook: centroids [C][D], row-major
    HipImageMatcher(rcn_ctx *ctx, int topK, const std::vector<float> &centroids, int C, int D) : ctx_(ctx), topK_(topK)
    {
        acquire();
        rcn_retr_default_options(&opt_);
        if ((size_t)C * D != centroids.size() || rcn_retr_codebook_create(ctx_, centroids.data(), C, D, &cb_) != RCN_OK) {
            const std::string why = centroids.size() == (size_t)C * D ? rcn_last_error(ctx_) : "centroids are not C x D";
            if (owned_) rcn_destroy(ctx_);
            throw std::runtime_error("HipImageMatcher: " + why);
        }
    }
    ~HipImageMatcher() override
    {
        if (cb_) rcn_retr_codebook_destroy(cb_);
        if (owned_) rcn_destroy(ctx_);
    }
    HipImageMatcher(const HipImageMatcher &) = delete;
    HipImageMatcher &operator=(const HipImageMatcher &) = delete;

    void match(const std::unordered_map<int, std::filesystem::path> &imgIds2Paths,
               const std::unordered_map<int, std::vector<FeaturePtr<>>> &features,
               std::unordered_map<int, std::vector<int>> &imgMatches) override
    {
        (void)imgIds2Paths;
        std::vector<int> ids;
        for (const auto &kv : features) ids.push_back(kv.first);
        std::sort(ids.begin(), ids.end());
        const int n = (int)ids.size();
        size_t K = 0, D = 0;
        for (int id : ids) {
            const auto &f = features.at(id);
            K = std::max(K, f.size());
            if (!f.empty() && !D) D = f[0]->featDesc.desc.size();
        }
        for (int id : ids) imgMatches[id] = {};
        if (n < 2) return;
        if (!K || !D) throw std::runtime_error("HipImageMatcher::match: no image has a descriptor");
        std::vector<float> rows((size_t)n * K * D, 0.f);
        std::vector<int32_t> counts((size_t)n);
        for (int s = 0; s < n; ++s) {
            const auto &f = features.at(ids[(size_t)s]);
            counts[(size_t)s] = (int32_t)f.size();
            for (size_t r = 0; r < f.size(); ++r) {
                if (f[r]->featDesc.desc.size() != D) throw std::runtime_error("HipImageMatcher::match: descriptor lengths differ");
                std::copy(f[r]->featDesc.desc.begin(), f[r]->featDesc.desc.end(), rows.begin() + ((size_t)s * K + r) * D);
            }
        }
        float *descDev = nullptr;
        int32_t *countsDev = nullptr;
        if (hipMalloc((void **)&descDev, rows.size() * sizeof(float)) || hipMalloc((void **)&countsDev, counts.size() * sizeof(int32_t))) {
            if (descDev) (void)hipFree(descDev);
            throw std::runtime_error("HipImageMatcher: out of device memory");
        }
        std::vector<int32_t> pairs;
        std::string err;
        if (hipMemcpy(descDev, rows.data(), rows.size() * sizeof(float), kMemcpyHostToDevice) ||
            hipMemcpy(countsDev, counts.data(), counts.size() * sizeof(int32_t), kMemcpyHostToDevice))
            err = "host to device copy failed";
        else
            try { pairs = matchDevice(descDev, countsDev, n, (int)K, (int)D, 0); } catch (const std::exception &e) { err = e.what(); }
        (void)hipFree(descDev);
        (void)hipFree(countsDev);
        if (!err.empty()) throw std::runtime_error("HipImageMatcher::match: " + err);
        for (size_t p = 0; p + 1 < pairs.size(); p += 2) {                  // ascending pairs: every partner list comes out ascending
            imgMatches[ids[(size_t)pairs[p]]].push_back(ids[(size_t)pairs[p + 1]]);
            imgMatches[ids[(size_t)pairs[p + 1]]].push_back(ids[(size_t)pairs[p]]);
        }
        for (int id : ids) std::sort(imgMatches[id].begin(), imgMatches[id].end());
    }

    // descDev: [n][K][D] floats in HBM; countsDev: rows in use per image, or NULL for K each.  Image slot s has id firstImgId + s.
    std::vector<int32_t> matchDevice(const float *descDev, const int32_t *countsDev, int n, int K, int D, int firstImgId)
    {
        rcn_retr_codebook *cb = cb_;
        if (!cb && rcn_retr_codebook_train_device(ctx_, descDev, countsDev, n, K, D, &opt_, &cb) != RCN_OK)
            throw std::runtime_error(std::string("HipImageMatcher: ") + rcn_last_error(ctx_));
        const int kk = std::max(0, std::min(topK_, n - 1));
        const size_t cap = std::min((size_t)n * kk, (size_t)n * (size_t)std::max(n - 1, 0) / 2);
        std::vector<int32_t> pairs(2 * cap + 2);
        int32_t count = 0;
        const int rc = rcn_retr_image_pairs(ctx_, cb, descDev, countsDev, n, K, D, firstImgId, topK_, pairs.data(), (int64_t)cap, &count);
        const std::string err = rc == RCN_OK ? "" : rcn_last_error(ctx_);
        if (!cb_) rcn_retr_codebook_destroy(cb);
        if (rc != RCN_OK) throw std::runtime_error("HipImageMatcher: " + err);
        pairs.resize(2 * (size_t)count);
        return pairs;
    }

private:
    void acquire()
    {
        owned_ = false;
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("HipImageMatcher: no usable gfx950 device");
            owned_ = true;
        }
    }

    rcn_ctx *ctx_;
    bool owned_ = false;
    int topK_;
    rcn_retr_options opt_;
    rcn_retr_codebook *cb_ = nullptr;
};

}  // namespace reconstructor::Core
