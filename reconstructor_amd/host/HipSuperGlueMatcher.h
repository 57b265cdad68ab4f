// HipSuperGlueMatcher.h -- the algorithmic half of FeatureMatcherSuperglue::matchFeatures (FeatureMatcherSuperglue.cpp:51-101)
// behind the graph network: the score matrix of the two sets of matching descriptors, the dustbin-augmented Sinkhorn
// iteration, the mutual-argmax selection and the two thresholds, through rcn_sg_match_device.  A device
// pointer plus element strides stands where the reference holds a torch::Tensor.
//   matchFeatures      one pair: the network's two [descSize][featuresNum] outputs in HBM (the featDescs layout of
//                      featsToTensors, :17: stride descriptor = featuresNum, stride feature = 1) -> the std::map<int, int>
//                      the reference fills at :76-87 with its matchScoreThreshold (:82)
//   matchFeaturesBatch B pairs in one call; the table (out[i] = feature of image 2 or -1) and the counts stay in HBM in the
//                      layout of rcn_match_grid_device: rcn_match_compact_begin, rcn_match_table_filter_device and
//                      everything behind them take them as they are
#pragma once
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rcn.h"
#include "rcn_types.h"

// The three HIP runtime calls this adapter needs for its own buffers, declared here so that the header builds with a plain
// host compiler and no ROCm include path (hipError_t and hipMemcpyKind are int-sized enums; 0 is hipSuccess).
extern "C" {
int hipMalloc(void **ptr, size_t bytes);
int hipFree(void *ptr);
int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);
}

namespace reconstructor::Core {

class FeatureMatcherSuperglueAssign {
public:
    static constexpr int kMemcpyHostToDevice = 1, kMemcpyDeviceToHost = 2;   // hipMemcpyKind

    // binScore: the network's learned bin_score; matchThreshold: the network's own threshold (0.2 in the published
    // configuration); matchScoreThreshold: the reference's second threshold (FeatureMatcherSuperglue.h, 0.5)
    explicit FeatureMatcherSuperglueAssign(rcn_ctx *ctx = nullptr, double binScore = 1.0, double matchThreshold = 0.2,
                                           double matchScoreThreshold = 0.5, int sinkhornIterations = 100)
        : ctx_(ctx), owned_(false)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("FeatureMatcherSuperglueAssign: no usable gfx950 device");
            owned_ = true;
        }
        rcn_sg_default_options(&opt_);
        opt_.alpha = binScore;
        opt_.match_threshold = matchThreshold;
        opt_.score_threshold = matchScoreThreshold;
        opt_.iterations = sinkhornIterations;
    }
    ~FeatureMatcherSuperglueAssign()
    {
        release();
        if (owned_) rcn_destroy(ctx_);
    }
    FeatureMatcherSuperglueAssign(const FeatureMatcherSuperglueAssign &) = delete;
    FeatureMatcherSuperglueAssign &operator=(const FeatureMatcherSuperglueAssign &) = delete;

    rcn_sg_options &options() { return opt_; }

    // descs1Dev / descs2Dev: the matching descriptors of the two images as the network leaves them, [descSize][featuresNum]
    // in HBM; strideD / strideF: element strides of the descriptor and the feature index (featuresNum and 1 for that layout).
    // matches[feature of image 1] = feature of image 2, for the pairs the reference keeps (:82).
    void matchFeatures(const float *descs1Dev, int64_t strideD1, int64_t strideF1, int featuresNum1, const float *descs2Dev, int64_t strideD2,
                       int64_t strideF2, int featuresNum2, int descSize, std::map<int, int> &matches)
    {
        if (featuresNum1 < 1 || featuresNum2 < 1) return;
        reserve(featuresNum1);
        if (rcn_sg_match_device(ctx_, descs1Dev, 0, strideF1, strideD1, descs2Dev, 0, strideF2, strideD2, nullptr, nullptr, 1, featuresNum1,
                                featuresNum2, descSize, &opt_, matches0_, nullptr, scores0_, nullptr, table_, featuresNum1, count_, nullptr,
                                count_ + 1) != RCN_OK || rcn_synchronize(ctx_) != RCN_OK)
            throw std::runtime_error(std::string("matchFeatures: ") + rcn_last_error(ctx_));
        std::vector<int32_t> table((size_t)featuresNum1);
        int32_t host[2] = {0, 0};
        copyOut(table.data(), table_, table.size() * sizeof(int32_t));
        copyOut(host, count_, sizeof(host));
        lastStatus_ = host[1];
        int kept = 0;
        for (int featIdx = 0; featIdx < featuresNum1; ++featIdx)
            if (table[featIdx] != -1) { matches[featIdx] = table[featIdx]; ++kept; }
        if (kept != host[0]) throw std::runtime_error("matchFeatures: the table and its count disagree");
    }

    // The batched form: B pairs, descriptors addressed by (pair, feature, descriptor) strides, per-pair feature counts in HBM
    // (or nullptr: maxFeatures1 / maxFeatures2 everywhere).  tableDev [B][tableStride] and countsDev [B] stay in HBM.
    void matchFeaturesBatch(const float *descs1Dev, int64_t strideP1, int64_t strideF1, int64_t strideD1, const float *descs2Dev, int64_t strideP2,
                            int64_t strideF2, int64_t strideD2, const int32_t *featuresNum1Dev, const int32_t *featuresNum2Dev, int pairs,
                            int maxFeatures1, int maxFeatures2, int descSize, int32_t *tableDev, int64_t tableStride, int32_t *countsDev,
                            int32_t *statusDev = nullptr)
    {
        if (pairs < 1) return;
        if ((size_t)pairs * maxFeatures1 > cap_) reserve((size_t)pairs * maxFeatures1);
        if (rcn_sg_match_device(ctx_, descs1Dev, strideP1, strideF1, strideD1, descs2Dev, strideP2, strideF2, strideD2, featuresNum1Dev,
                                featuresNum2Dev, pairs, maxFeatures1, maxFeatures2, descSize, &opt_, matches0_, nullptr, nullptr, nullptr, tableDev,
                                tableStride, countsDev, nullptr, statusDev) != RCN_OK)
            throw std::runtime_error(std::string("matchFeaturesBatch: ") + rcn_last_error(ctx_));
    }
    int lastStatus() const { return lastStatus_; }      // 1: the last pair of matchFeatures held a non-finite score (no matches)
    rcn_ctx *ctx() const { return ctx_; }

private:
    void release()
    {
        for (void *p : {(void *)matches0_, (void *)table_, (void *)scores0_, (void *)count_}) if (p) (void)hipFree(p);
        matches0_ = nullptr; table_ = nullptr; scores0_ = nullptr; count_ = nullptr;
        cap_ = 0;
    }
    void reserve(size_t rows)
    {
        if (rows <= cap_) return;
        release();
        if (hipMalloc((void **)&matches0_, rows * sizeof(int32_t)) || hipMalloc((void **)&table_, rows * sizeof(int32_t)) ||
            hipMalloc((void **)&scores0_, rows * sizeof(float)) || hipMalloc((void **)&count_, 2 * sizeof(int32_t)))
            throw std::runtime_error("FeatureMatcherSuperglueAssign: out of device memory");
        cap_ = rows;
    }
    void copyOut(void *dst, const void *src, size_t bytes)
    {
        if (bytes && hipMemcpy(dst, src, bytes, kMemcpyDeviceToHost)) throw std::runtime_error("FeatureMatcherSuperglueAssign: device to host copy failed");
    }

    rcn_ctx *ctx_;
    bool owned_;
    rcn_sg_options opt_;
    size_t cap_ = 0;
    int lastStatus_ = 0;
    int32_t *matches0_ = nullptr, *table_ = nullptr, *count_ = nullptr;
    float *scores0_ = nullptr;
};

}  // namespace reconstructor::Core
