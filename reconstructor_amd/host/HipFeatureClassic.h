// HipFeatureClassic.h -- FeatureClassic (FeatureDetector.h:40-52, FeatureDetector.cpp:7-50) over the C ABI, with the
// reference's parameter lists: GreyImage (rcn_types.h) stands where the reference passes a cv::Mat.
//   prepImg  (:37-50)  the image in the detector's input type (bytes): a float image is converted as cv::Mat::convertTo does,
//                      saturate_cast<uchar> = round-half-even, clamped to 0..255; a byte image is copied
//   detect   (:13-35)  cv::SIFT::create()->detectAndCompute = rcn_sift_detect_and_compute_device; per keypoint a Feature whose
//                      featCoord is pt truncated toward zero (the float -> int assignment of :28-29) and whose featDesc.desc
//                      holds the 128 floats of the row converted to CV_32F (:24, :30-32)
//   detectBatch        n images that are in HBM already; the rows stay there, [n][K][128] in a buffer of the caller's (the slot
//                      of rcn_shard_reserve, for one); only the integer coordinates and the counts come to the host
//   detectBatchPacked  the ORB branch's batch with the descriptor's 32 BYTES per keypoint and the counts left in HBM, as
//                      rcn_bits_upload_batch_device takes them (the Hamming matcher, HipFeatureMatcher.h); only the coordinates come back
//   Detector           the reference's one-line switch (FeatureDetector.cpp:9, :19): Sift (the default, cv::SIFT::create()) or Orb
//                      (cv::ORB::create() = rcn_orb_detect_and_compute_device): rows of 32 floats, the descriptor's bytes converted
//                      to CV_32F (:24); setOrbPattern supplies the 256 tests (NULL: the built-in pattern)
// The reference has no cap on the number of keypoints: when detect finds more than its buffers hold, the buffers grow and
// the call runs again, as FeatureSuperPointPost::run does.
#pragma once
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
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

class FeatureClassic {
public:
    static constexpr int kMemcpyHostToDevice = 1, kMemcpyDeviceToHost = 2;   // hipMemcpyKind

    enum class Detector { Sift, Orb };

    explicit FeatureClassic(Detector detector, rcn_ctx *ctx = nullptr, int capacity = 4096) : FeatureClassic(ctx, capacity, detector) {}
    explicit FeatureClassic(rcn_ctx *ctx = nullptr, int capacity = 4096, Detector detector = Detector::Sift)
        : ctx_(ctx), owned_(false), orb_(detector == Detector::Orb), dim_(detector == Detector::Orb ? 32 : 128)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("FeatureClassic: no usable gfx950 device");
            owned_ = true;
        }
        rcn_sift_default_options(&opt_);
        rcn_orb_default_options(&orbOpt_);
        reserve(capacity < 1 ? 1 : capacity);
    }
    ~FeatureClassic()
    {
        release();
        if (img_) (void)hipFree(img_);
        if (owned_) rcn_destroy(ctx_);
    }
    FeatureClassic(const FeatureClassic &) = delete;
    FeatureClassic &operator=(const FeatureClassic &) = delete;

    int descriptorSize() const { return dim_; }
    // 256 tests (x0, y0, x1, y1) as 1024 signed bytes, every |coordinate| <= 15, copied; nullptr: the built-in pattern again
    void setOrbPattern(const int8_t *pattern)
    {
        if (pattern) { orbPattern_.assign(pattern, pattern + 1024); orbOpt_.pattern = orbPattern_.data(); }
        else { orbPattern_.clear(); orbOpt_.pattern = nullptr; }
    }

    GreyImage prepImg(const GreyImage &img) const
    {
        GreyImage out;
        out.rows = img.rows; out.cols = img.cols;
        if (!img.isFloat) { out.u8 = img.u8; return out; }
        out.u8.resize(img.f32.size());
        for (size_t i = 0; i < img.f32.size(); ++i) {
            const float r = std::nearbyint(img.f32[i]);              // round-half-even in the default rounding mode
            out.u8[i] = (uint8_t)(r < 0.f ? 0.f : r > 255.f ? 255.f : r);
        }
        return out;
    }

    void detect(const GreyImage &img, std::vector<FeaturePtr<>> &features)
    {
        const size_t pixels = (size_t)img.rows * img.cols, bytes = pixels * (img.isFloat ? sizeof(float) : 1);
        if (bytes > imgCap_) {
            if (img_) (void)hipFree(img_);
            img_ = nullptr; imgCap_ = 0;
            if (hipMalloc(&img_, bytes)) throw std::runtime_error("FeatureClassic: out of device memory");
            imgCap_ = bytes;
        }
        const void *src = img.isFloat ? (const void *)img.f32.data() : (const void *)img.u8.data();
        if (bytes && hipMemcpy(img_, src, bytes, kMemcpyHostToDevice)) throw std::runtime_error("FeatureClassic: host to device copy failed");
        int m = 0;
        for (;;) {
            const int rc = orb_ ? rcn_orb_detect_and_compute_device(ctx_, img_, img.isFloat ? RCN_ORB_INPUT_F32 : RCN_ORB_INPUT_U8, (int64_t)pixels, img.cols, 1, 1,
                                                                    img.rows, img.cols, &orbOpt_, cap_, xy_, xyInt_, size_, angle_, resp_, oct_, count_, rows_, nullptr)
                                : rcn_sift_detect_and_compute_device(ctx_, img_, img.isFloat ? RCN_SIFT_INPUT_F32 : RCN_SIFT_INPUT_U8, (int64_t)pixels, img.cols, 1, 1,
                                                                     img.rows, img.cols, &opt_, cap_, xy_, xyInt_, size_, angle_, resp_, oct_, count_, rows_);
            if (rc != RCN_OK || rcn_synchronize(ctx_) != RCN_OK)
                throw std::runtime_error(std::string("FeatureClassic::detect: ") + rcn_last_error(ctx_));
            int32_t host = 0;
            copyOut(&host, count_, sizeof(host));
            ++runs_;
            if (host < 0) throw std::runtime_error(orb_ ? "FeatureClassic::detect: more tied FAST corners than the workspace holds"
                                                        : "FeatureClassic::detect: more scale-space extrema than the workspace holds");
            m = host;
            if (m <= cap_) break;
            reserve(m);
        }
        std::vector<int32_t> xy(2 * (size_t)m + 2);
        const size_t D = (size_t)dim_;
        std::vector<float> rows((size_t)m * D + 1);
        copyOut(xy.data(), xyInt_, 2 * (size_t)m * sizeof(int32_t));
        copyOut(rows.data(), rows_, (size_t)m * D * sizeof(float));
        for (int i = 0; i < m; ++i) {
            FeaturePtr<> feat = std::make_shared<Feature<>>();
            feat->featCoord.x = xy[2 * i];
            feat->featCoord.y = xy[2 * i + 1];
            feat->featDesc.desc.assign(rows.begin() + (size_t)i * D, rows.begin() + (size_t)(i + 1) * D);
            features.push_back(feat);
        }
    }

    // imagesDev: n byte images [rows][cols], dense, in HBM; rowsOutDev: [n][K][descriptorSize()] floats in HBM, rows past min(count, K) zero.
    // coords[i]: the integer coordinates of the min(counts[i], K) keypoints emitted for image i; counts[i]: the uncapped number.
    void detectBatch(const uint8_t *imagesDev, int n, int rows, int cols, int K, float *rowsOutDev, std::vector<std::vector<FeatCoord<>>> &coords,
                     std::vector<int> &counts)
    {
        coords.assign((size_t)(n > 0 ? n : 0), {});
        counts.assign((size_t)(n > 0 ? n : 0), 0);
        if (n <= 0) return;
        const size_t nk = (size_t)n * K;
        float *f = nullptr;
        int32_t *i32 = nullptr;
        if (hipMalloc((void **)&f, nk * 5 * sizeof(float)) || hipMalloc((void **)&i32, (nk * 3 + (size_t)n) * sizeof(int32_t))) {
            if (f) (void)hipFree(f);
            throw std::runtime_error("FeatureClassic: out of device memory");
        }
        const int rc = orb_ ? rcn_orb_detect_and_compute_device(ctx_, imagesDev, RCN_ORB_INPUT_U8, (int64_t)rows * cols, cols, 1, n, rows, cols, &orbOpt_, K, f, i32,
                                                                f + 2 * nk, f + 3 * nk, f + 4 * nk, i32 + 2 * nk, i32 + 3 * nk, rowsOutDev, nullptr)
                            : rcn_sift_detect_and_compute_device(ctx_, imagesDev, RCN_SIFT_INPUT_U8, (int64_t)rows * cols, cols, 1, n, rows, cols, &opt_, K, f, i32,
                                                                 f + 2 * nk, f + 3 * nk, f + 4 * nk, i32 + 2 * nk, i32 + 3 * nk, rowsOutDev);
        std::vector<int32_t> host(nk * 2 + (size_t)n);
        const bool ok = rc == RCN_OK && rcn_synchronize(ctx_) == RCN_OK && !hipMemcpy(host.data(), i32, nk * 2 * sizeof(int32_t), kMemcpyDeviceToHost) &&
                        !hipMemcpy(host.data() + nk * 2, i32 + 3 * nk, (size_t)n * sizeof(int32_t), kMemcpyDeviceToHost);
        (void)hipFree(f);
        (void)hipFree(i32);
        if (!ok) throw std::runtime_error(std::string("FeatureClassic::detectBatch: ") + rcn_last_error(ctx_));
        for (int i = 0; i < n; ++i) {
            counts[(size_t)i] = host[nk * 2 + (size_t)i];
            const int m = counts[(size_t)i] < K ? (counts[(size_t)i] < 0 ? 0 : counts[(size_t)i]) : K;
            for (int k = 0; k < m; ++k) coords[(size_t)i].emplace_back(host[((size_t)i * K + k) * 2], host[((size_t)i * K + k) * 2 + 1]);
        }
    }
    // Detector::Orb only.  bytesOutDev: [n][K][32] bytes in HBM; countsOutDev: [n] int32 in HBM, ORB's own counts (uncapped; -1: a level
    // overflowed) -- both as rcn_bits_upload_batch_device(ctx, firstId, n, bytesOutDev, countsOutDev, K, 32) takes them, no host round trip
    // for either.  coords / counts as detectBatch.
    void detectBatchPacked(const uint8_t *imagesDev, int n, int rows, int cols, int K, uint8_t *bytesOutDev, int32_t *countsOutDev,
                           std::vector<std::vector<FeatCoord<>>> &coords, std::vector<int> &counts)
    {
        if (!orb_) throw std::runtime_error("FeatureClassic::detectBatchPacked: packed rows are the ORB detector's");
        coords.assign((size_t)(n > 0 ? n : 0), {});
        counts.assign((size_t)(n > 0 ? n : 0), 0);
        if (n <= 0) return;
        if (!bytesOutDev || !countsOutDev) throw std::runtime_error("FeatureClassic::detectBatchPacked: null output");
        const size_t nk = (size_t)n * K;
        float *f = nullptr;
        int32_t *i32 = nullptr;
        if (hipMalloc((void **)&f, nk * (5 + 32) * sizeof(float)) || hipMalloc((void **)&i32, nk * 3 * sizeof(int32_t))) {
            if (f) (void)hipFree(f);
            throw std::runtime_error("FeatureClassic: out of device memory");
        }
        const int rc = rcn_orb_detect_and_compute_device(ctx_, imagesDev, RCN_ORB_INPUT_U8, (int64_t)rows * cols, cols, 1, n, rows, cols, &orbOpt_, K, f, i32,
                                                         f + 2 * nk, f + 3 * nk, f + 4 * nk, i32 + 2 * nk, countsOutDev, f + 5 * nk, bytesOutDev);
        std::vector<int32_t> host(nk * 2 + (size_t)n);
        const bool ok = rc == RCN_OK && rcn_synchronize(ctx_) == RCN_OK && !hipMemcpy(host.data(), i32, nk * 2 * sizeof(int32_t), kMemcpyDeviceToHost) &&
                        !hipMemcpy(host.data() + nk * 2, countsOutDev, (size_t)n * sizeof(int32_t), kMemcpyDeviceToHost);
        (void)hipFree(f);
        (void)hipFree(i32);
        if (!ok) throw std::runtime_error(std::string("FeatureClassic::detectBatchPacked: ") + rcn_last_error(ctx_));
        for (int i = 0; i < n; ++i) {
            counts[(size_t)i] = host[nk * 2 + (size_t)i];
            const int m = counts[(size_t)i] < K ? (counts[(size_t)i] < 0 ? 0 : counts[(size_t)i]) : K;
            for (int k = 0; k < m; ++k) coords[(size_t)i].emplace_back(host[((size_t)i * K + k) * 2], host[((size_t)i * K + k) * 2 + 1]);
        }
    }
    int runs() const { return runs_; }      // device calls of detect so far (a call that had to grow its buffers counts twice)

private:
    void release()
    {
        for (void *p : {(void *)xy_, (void *)xyInt_, (void *)size_, (void *)angle_, (void *)resp_, (void *)oct_, (void *)count_, (void *)rows_})
            if (p) (void)hipFree(p);
        xy_ = size_ = angle_ = resp_ = rows_ = nullptr;
        xyInt_ = oct_ = count_ = nullptr;
    }
    void reserve(int cap)
    {
        release();
        cap_ = cap;
        const size_t c = (size_t)cap;
        if (hipMalloc((void **)&xy_, c * 2 * sizeof(float)) || hipMalloc((void **)&xyInt_, c * 2 * sizeof(int32_t)) || hipMalloc((void **)&size_, c * sizeof(float)) ||
            hipMalloc((void **)&angle_, c * sizeof(float)) || hipMalloc((void **)&resp_, c * sizeof(float)) || hipMalloc((void **)&oct_, c * sizeof(int32_t)) ||
            hipMalloc((void **)&count_, sizeof(int32_t)) || hipMalloc((void **)&rows_, c * (size_t)dim_ * sizeof(float)))
            throw std::runtime_error("FeatureClassic: out of device memory");
    }
    void copyOut(void *dst, const void *src, size_t bytes)
    {
        if (bytes && hipMemcpy(dst, src, bytes, kMemcpyDeviceToHost)) throw std::runtime_error("FeatureClassic: device to host copy failed");
    }

    rcn_ctx *ctx_;
    bool owned_;
    bool orb_;
    int dim_;
    rcn_sift_options opt_;
    rcn_orb_options orbOpt_;
    std::vector<int8_t> orbPattern_;
    int cap_ = 0, runs_ = 0;
    float *xy_ = nullptr, *size_ = nullptr, *angle_ = nullptr, *resp_ = nullptr, *rows_ = nullptr;
    int32_t *xyInt_ = nullptr, *oct_ = nullptr, *count_ = nullptr;
    void *img_ = nullptr;
    size_t imgCap_ = 0;
};

}  // namespace reconstructor::Core
