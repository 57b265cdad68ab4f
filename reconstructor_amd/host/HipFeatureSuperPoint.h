// HipFeatureSuperPoint.h -- the post-processing half of FeatureSuperPoint::detect (FeatureSuperPoint.cpp:228-263) behind the
// network's forward pass, with the reference's parameter lists: a device pointer plus element strides stands where the
// reference passes a torch::Tensor.
//   processKeypoints (:145-179)  -> rcn_kp_detect_device: heat map, threshold, nmsFast, removeBorderKeypoints
//   detectPost                   -> the same, then processDescriptors (:183-211) through rcn_desc_sample_batch_device, and the
//                                   features pushed as detect() pushes them (:257-262)
// The network's two outputs stay where the network left them (HBM); what crosses to the host is what the reference's
// containers hold: the keypoints, and in detectPost their 256 floats each.  Order: raster (y, then x), the order of nmsFast's
// final grid scan.  The reference has no cap on the number of keypoints: when more survive than the buffers hold, the buffers
// grow and the call runs again.  FeatureSuperPointNet below puts the network itself in front: the whole of detect().
#pragma once
#include <cstring>
#include <memory>
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

class FeatureSuperPointPost {
public:
    static constexpr int kMemcpyHostToDevice = 1, kMemcpyDeviceToHost = 2;   // hipMemcpyKind

    // heatMode: RCN_KP_HEAT_REFERENCE is extractHeatMap as written; nmsRadius: nmsFast's distThresh (4 in the reference)
    explicit FeatureSuperPointPost(rcn_ctx *ctx = nullptr, int heatMode = RCN_KP_HEAT_REFERENCE, int nmsRadius = 4, int capacity = 2048)
        : ctx_(ctx), owned_(false), mode_(heatMode), radius_(nmsRadius)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("FeatureSuperPointPost: no usable gfx950 device");
            owned_ = true;
        }
        reserve(capacity < 1 ? 1 : capacity);
    }
    ~FeatureSuperPointPost()
    {
        release();
        if (owned_) rcn_destroy(ctx_);
    }
    FeatureSuperPointPost(const FeatureSuperPointPost &) = delete;
    FeatureSuperPointPost &operator=(const FeatureSuperPointPost &) = delete;

    // keypointTensor: the [65][imgHeight / 8][imgWidth / 8] logits of ONE image in HBM, addressed by element strides
    // (the network's own output: strideC = Hc * Wc, strideY = Wc, strideX = 1)
    std::vector<FeatCoordConf<>> processKeypoints(const float *keypointTensorDev, int64_t strideC, int64_t strideY, int64_t strideX,
                                                  const int imgHeight, const int imgWidth, const double confThresh, const int borderSize)
    {
        const int m = run(keypointTensorDev, strideC, strideY, strideX, imgHeight, imgWidth, confThresh, borderSize);
        std::vector<int32_t> xy(2 * (size_t)m + 2);
        std::vector<float> conf((size_t)m + 1);
        copyOut(xy.data(), xy_, 2 * (size_t)m * sizeof(int32_t));
        copyOut(conf.data(), conf_, (size_t)m * sizeof(float));
        std::vector<FeatCoordConf<>> out;
        out.reserve(m);
        for (int i = 0; i < m; ++i) out.emplace_back(xy[2 * i], xy[2 * i + 1], conf[i]);
        return out;
    }

    // detect() behind superNet.forward: keypoints from keypointTensorDev, descriptors from the [256][Hc][Wc] map at
    // descriptorsDev (strides in elements; the reference's permuted view is the same memory), features appended
    void detectPost(const float *keypointTensorDev, int64_t strideC, int64_t strideY, int64_t strideX, const float *descriptorsDev,
                    int64_t descStrideC, int64_t descStrideY, int64_t descStrideX, const int imgHeight, const int imgWidth,
                    const double confThresh, const int borderSize, std::vector<FeaturePtr<>> &features)
    {
        const int D = 256;
        const int m = run(keypointTensorDev, strideC, strideY, strideX, imgHeight, imgWidth, confThresh, borderSize);
        if (rcn_desc_sample_batch_device(ctx_, descriptorsDev, 0, descStrideC, descStrideY, descStrideX, imgHeight / 8, imgWidth / 8, xy_,
                                         count_, 1, cap_, D, rows_) != RCN_OK || rcn_synchronize(ctx_) != RCN_OK)
            throw std::runtime_error(std::string("detectPost: ") + rcn_last_error(ctx_));
        std::vector<int32_t> xy(2 * (size_t)m + 2);
        std::vector<float> conf((size_t)m + 1), rows((size_t)m * D + 1);
        copyOut(xy.data(), xy_, 2 * (size_t)m * sizeof(int32_t));
        copyOut(conf.data(), conf_, (size_t)m * sizeof(float));
        copyOut(rows.data(), rows_, (size_t)m * D * sizeof(float));
        for (int i = 0; i < m; ++i) {
            FeatDesc desc(rows.begin() + (size_t)i * D, rows.begin() + (size_t)(i + 1) * D);
            features.push_back(std::make_shared<FeatureConf<>>(FeatCoordConf<>(xy[2 * i], xy[2 * i + 1], conf[i]), std::move(desc)));
        }
    }
    int lastRounds() const { return lastRounds_; }      // rounds of the NMS iteration of the last call

private:
    void release()
    {
        for (void *p : {(void *)xy_, (void *)conf_, (void *)count_, (void *)rows_}) if (p) (void)hipFree(p);
        xy_ = nullptr; conf_ = nullptr; count_ = nullptr; rows_ = nullptr;
    }
    void reserve(int cap)
    {
        release();
        cap_ = cap;
        if (hipMalloc((void **)&xy_, (size_t)cap * 2 * sizeof(int32_t)) || hipMalloc((void **)&conf_, (size_t)cap * sizeof(float)) ||
            hipMalloc((void **)&count_, 2 * sizeof(int32_t)) || hipMalloc((void **)&rows_, (size_t)cap * 256 * sizeof(float)))
            throw std::runtime_error("FeatureSuperPointPost: out of device memory");
    }
    void copyOut(void *dst, const void *src, size_t bytes)
    {
        if (bytes && hipMemcpy(dst, src, bytes, kMemcpyDeviceToHost)) throw std::runtime_error("FeatureSuperPointPost: device to host copy failed");
    }
    // keypoints of one image into xy_ / conf_; returns how many (all of them: the buffers grow until they fit)
    int run(const float *logits, int64_t sc, int64_t sy, int64_t sx, int H, int W, double confThresh, int borderSize)
    {
        for (;;) {
            if (rcn_kp_detect_device(ctx_, logits, 0, sc, sy, sx, 1, H, W, mode_, confThresh, radius_, borderSize, cap_, xy_, conf_, count_,
                                     nullptr, count_ + 1) != RCN_OK || rcn_synchronize(ctx_) != RCN_OK)
                throw std::runtime_error(std::string("processKeypoints: ") + rcn_last_error(ctx_));
            int32_t host[2] = {0, 0};
            copyOut(host, count_, sizeof(host));
            lastRounds_ = host[1];
            if (host[0] <= cap_) return host[0];
            reserve(host[0]);
        }
    }

    rcn_ctx *ctx_;
    bool owned_;
    int mode_, radius_, cap_ = 0, lastRounds_ = 0;
    int32_t *xy_ = nullptr, *count_ = nullptr;
    float *conf_ = nullptr, *rows_ = nullptr;
};

// FeatureSuperPoint::detect (:228-263) with the network itself behind the C ABI (rcn_sp_net_*): image in,
// features out, no libtorch and no TorchScript blob.  The caller supplies the weights as the packed block of rcn_sp_net_create
// (reconstructor_amd/superpoint_net.py packs a state dict); the library ships none.
//   prepImg  (:265-288)  bytes -> float, v / 255.0 with the reference's float /= double; host code
//   detect               the image (what prepImg returns: rows x cols floats, row-major) goes to HBM, rcn_sp_net_detect_device
//                        runs the forward, processKeypoints and processDescriptors, and the features are pushed as :257-262
// rows and cols must be multiples of 8.  When more keypoints survive than the buffers hold, the buffers grow and the call
// runs again, as FeatureSuperPointPost::run does.
class FeatureSuperPointNet {
public:
    static constexpr int kMemcpyHostToDevice = 1, kMemcpyDeviceToHost = 2;   // hipMemcpyKind

    FeatureSuperPointNet(const float *params, int64_t nParams, rcn_ctx *ctx = nullptr, int heatMode = RCN_KP_HEAT_REFERENCE, int nmsRadius = 4,
                         int capacity = 2048, double confThresh = 0.015, int borderSize = 4)
        : ctx_(ctx), owned_(false), mode_(heatMode), radius_(nmsRadius), border_(borderSize), thresh_(confThresh)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("FeatureSuperPointNet: no usable gfx950 device");
            owned_ = true;
        }
        if (rcn_sp_net_create(ctx_, params, nParams, &net_) != RCN_OK) {
            const std::string why = rcn_last_error(ctx_);
            if (owned_) rcn_destroy(ctx_);
            throw std::runtime_error("FeatureSuperPointNet: " + why);
        }
        reserve(capacity < 1 ? 1 : capacity);
    }
    ~FeatureSuperPointNet()
    {
        release();
        if (img_) (void)hipFree(img_);
        rcn_sp_net_destroy(net_);
        if (owned_) rcn_destroy(ctx_);
    }
    FeatureSuperPointNet(const FeatureSuperPointNet &) = delete;
    FeatureSuperPointNet &operator=(const FeatureSuperPointNet &) = delete;

    // a byte image as floats in [0, 1]: every pixel converted to float, then divided by the double 255.0 and rounded back
    static std::vector<float> prepImg(const uint8_t *img, int rows, int cols)
    {
        std::vector<float> out((size_t)rows * cols);
        for (size_t i = 0; i < out.size(); ++i) {
            float v = (float)img[i];
            v /= 255.0;
            out[i] = v;
        }
        return out;
    }

    void detect(const float *img, int rows, int cols, std::vector<FeaturePtr<>> &features)
    {
        const int D = 256;
        const size_t pixels = (size_t)rows * cols;
        if (pixels > imgCap_) {
            if (img_) (void)hipFree(img_);
            img_ = nullptr; imgCap_ = 0;
            if (hipMalloc((void **)&img_, pixels * sizeof(float))) throw std::runtime_error("FeatureSuperPointNet: out of device memory");
            imgCap_ = pixels;
        }
        if (pixels && hipMemcpy(img_, img, pixels * sizeof(float), kMemcpyHostToDevice)) throw std::runtime_error("FeatureSuperPointNet: host to device copy failed");
        int m = 0;
        for (;;) {
            if (rcn_sp_net_detect_device(ctx_, net_, img_, RCN_SP_INPUT_F32, (int64_t)pixels, cols, 1, 1, rows, cols, RCN_SP_NORMALIZE_DESC, mode_, thresh_,
                                         radius_, border_, cap_, D, xy_, conf_, count_, rows_, nullptr, count_ + 1) != RCN_OK ||
                rcn_synchronize(ctx_) != RCN_OK)
                throw std::runtime_error(std::string("FeatureSuperPointNet::detect: ") + rcn_last_error(ctx_));
            int32_t host[2] = {0, 0};
            copyOut(host, count_, sizeof(host));
            lastRounds_ = host[1];
            ++lastRuns_;
            m = host[0];
            if (m <= cap_) break;
            reserve(m);
        }
        std::vector<int32_t> xy(2 * (size_t)m + 2);
        std::vector<float> conf((size_t)m + 1), rows_host((size_t)m * D + 1);
        copyOut(xy.data(), xy_, 2 * (size_t)m * sizeof(int32_t));
        copyOut(conf.data(), conf_, (size_t)m * sizeof(float));
        copyOut(rows_host.data(), rows_, (size_t)m * D * sizeof(float));
        for (int i = 0; i < m; ++i) {
            FeatDesc desc(rows_host.begin() + (size_t)i * D, rows_host.begin() + (size_t)(i + 1) * D);
            features.push_back(std::make_shared<FeatureConf<>>(FeatCoordConf<>(xy[2 * i], xy[2 * i + 1], conf[i]), std::move(desc)));
        }
    }
    int lastRounds() const { return lastRounds_; }      // rounds of the NMS iteration of the last call
    int runs() const { return lastRuns_; }              // device calls so far (a call that had to grow its buffers counts twice)

private:
    void release()
    {
        for (void *p : {(void *)xy_, (void *)conf_, (void *)count_, (void *)rows_}) if (p) (void)hipFree(p);
        xy_ = nullptr; conf_ = nullptr; count_ = nullptr; rows_ = nullptr;
    }
    void reserve(int cap)
    {
        release();
        cap_ = cap;
        if (hipMalloc((void **)&xy_, (size_t)cap * 2 * sizeof(int32_t)) || hipMalloc((void **)&conf_, (size_t)cap * sizeof(float)) ||
            hipMalloc((void **)&count_, 2 * sizeof(int32_t)) || hipMalloc((void **)&rows_, (size_t)cap * 256 * sizeof(float)))
            throw std::runtime_error("FeatureSuperPointNet: out of device memory");
    }
    void copyOut(void *dst, const void *src, size_t bytes)
    {
        if (bytes && hipMemcpy(dst, src, bytes, kMemcpyDeviceToHost)) throw std::runtime_error("FeatureSuperPointNet: device to host copy failed");
    }

    rcn_ctx *ctx_;
    rcn_sp_net *net_ = nullptr;
    bool owned_;
    int mode_, radius_, border_, cap_ = 0, lastRounds_ = 0, lastRuns_ = 0;
    double thresh_;
    int32_t *xy_ = nullptr, *count_ = nullptr;
    float *conf_ = nullptr, *rows_ = nullptr, *img_ = nullptr;
    size_t imgCap_ = 0;
};

}  // namespace reconstructor::Core
