// HipImagePrep.h -- what Utils does around the detectors (utils.cpp:61-109, :205-275, :345-368) and detectFeatures' colour loop
// (SequentialReconstructor.cpp:98-106) over the C ABI, with the reference's names and parameter orders; ColourImage
// (rcn_types.h) stands where the reference passes a cv::Mat, anything indexable as M(r,c) where it passes an Eigen::Matrix4d.
//   reshapeImg (:61-98)       cv::resize to at most imgMaxSize on the longer side, in place; returns the factor
//   readImg (:100-109)        its half behind cv::imread: BGR -> RGB, then reshapeImg; the grey image of the RESIZED colours
//                             (cvtColor(RGB2GRAY), SequentialReconstructor.cpp:89-90) comes out of the same kernel on request
//   prepareBatch              n decoded images of one size that are in HBM already: colours and grey stay there
//   extractFeatureColors      featColor = the pixel under featCoord for every feature of one image (:98-106)
//   saveCloud (:345-368)      landmarks (with outliers painted when flags are given) and camera centres as a PLY file, ASCII as
//                             pcl::io::savePLYFile writes by default; cameras in imgIdx2camPose's own iteration order
// JPEG decoding stays with the caller.  Defined by tests/img_ref.py.
#pragma once
#include <algorithm>
#include <cstdint>
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

namespace reconstructor::Utils {

using reconstructor::Core::ColourImage;
using reconstructor::Core::FeaturePtr;
using reconstructor::Core::GreyImage;
using reconstructor::Core::Landmark;

class ImagePrep {
public:
    static constexpr int kMemcpyHostToDevice = 1, kMemcpyDeviceToHost = 2;   // hipMemcpyKind

    explicit ImagePrep(rcn_ctx *ctx = nullptr) : ctx_(ctx), owned_(false)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("ImagePrep: no usable gfx950 device");
            owned_ = true;
        }
    }
    ~ImagePrep()
    {
        if (owned_) rcn_destroy(ctx_);
    }
    ImagePrep(const ImagePrep &) = delete;
    ImagePrep &operator=(const ImagePrep &) = delete;

    int grayBits = 14;       // 14: cvtColor's table in OpenCV 4.2, the reference's version; 15: later releases

    double reshapeImg(ColourImage &img, const int imgMaxSize) { return prepareHost(img, imgMaxSize, RCN_IMG_RGB, nullptr); }

    // img: what cv::imread delivered (BGR); afterwards RGB at the prepared size, dense.  gray (may be NULL): cvtColor(RGB2GRAY) of it.
    double readImg(ColourImage &img, const int imgMaxSize, GreyImage *gray = nullptr) { return prepareHost(img, imgMaxSize, RCN_IMG_BGR, gray); }

    // srcDev: n images of srcRows x srcCols x channels in HBM, rows strideRowBytes and images strideImgBytes apart; order: RCN_IMG_BGR
    // for what imread delivers.  rgbOutDev [n][rows][cols][3] and grayOutDev [n][rows][cols] (either may be NULL) stay in HBM and
    // feed rcn_sift_*_device / rcn_sp_net_*_device (input dtype U8) unchanged.  Returns the factor; rows / cols: the prepared size.
    double prepareBatch(const uint8_t *srcDev, int n, int srcRows, int srcCols, int channels, int64_t strideImgBytes, int64_t strideRowBytes,
                        int imgMaxSize, int order, uint8_t *rgbOutDev, uint8_t *grayOutDev, int &rows, int &cols)
    {
        int32_t r = 0, c = 0;
        double factor = 1.0;
        if (rcn_img_reshape_size(srcRows, srcCols, imgMaxSize, &r, &c, &factor) != RCN_OK) throw std::runtime_error("ImagePrep: no image is left at this size");
        const rcn_img_options opt = {order, grayBits};
        if (rcn_img_prepare_device(ctx_, srcDev, strideImgBytes, strideRowBytes, channels, n, srcRows, srcCols, r, c, &opt, rgbOutDev, grayOutDev) != RCN_OK ||
            rcn_synchronize(ctx_) != RCN_OK)
            throw std::runtime_error(std::string("ImagePrep::prepareBatch: ") + rcn_last_error(ctx_));
        rows = r; cols = c;
        return factor;
    }

    // rgb: the prepared colour image the features were detected on (readImg's result).  It keeps the reference's shape, one image
    // per call, and so uploads that whole image and launches a kernel for a gather whose data is on the host already: fine for the
    // reference's loop, wasteful over many images.  A pipeline whose prepared images stay in HBM (prepareBatch) calls
    // rcn_feat_colors_device on them for all images at once instead.
    void extractFeatureColors(std::vector<FeaturePtr<>> &features, const ColourImage &rgb)
    {
        const size_t K = features.size();
        if (!K) return;
        if (rgb.channels != 3) throw std::runtime_error("ImagePrep::extractFeatureColors: a colour image has three channels");
        const std::vector<uint8_t> dense = densePixels(rgb);
        std::vector<int32_t> xy(2 * K);
        for (size_t k = 0; k < K; ++k) { xy[2 * k] = features[k]->featCoord.x; xy[2 * k + 1] = features[k]->featCoord.y; }
        const int32_t count = (int32_t)K;
        Block d(dense.size() + 256 + 8 * K + 256 + 4 * K + 256);
        uint8_t *dRgb = d.p, *dXy = align(dRgb + dense.size()), *dCnt = align(dXy + 8 * K), *dOut = dCnt + 16;
        up(dRgb, dense.data(), dense.size()); up(dXy, xy.data(), 8 * K); up(dCnt, &count, 4);
        if (rcn_feat_colors_device(ctx_, dRgb, 1, rgb.rows, rgb.cols, reinterpret_cast<int32_t *>(dXy), reinterpret_cast<int32_t *>(dCnt), (int32_t)K, dOut) != RCN_OK ||
            rcn_synchronize(ctx_) != RCN_OK)
            throw std::runtime_error(std::string("ImagePrep::extractFeatureColors: ") + rcn_last_error(ctx_));
        std::vector<uint8_t> rgba(4 * K);
        down(rgba.data(), dOut, 4 * K);
        for (size_t k = 0; k < K; ++k) {
            features[k]->featColor.red = rgba[4 * k];
            features[k]->featColor.green = rgba[4 * k + 1];
            features[k]->featColor.blue = rgba[4 * k + 2];
        }
    }

    template <class Pose4>
    void saveCloud(std::vector<Landmark> &landmarks, std::unordered_map<int, Pose4> &imgIdx2camPose, const std::string &cloudPath)
    {
        writeCloud(landmarks, imgIdx2camPose, cloudPath, nullptr);
    }

    // the same, every landmark once more in front with the outliers painted red
    template <class Pose4>
    void saveCloud(std::vector<Landmark> &landmarks, std::unordered_map<int, Pose4> &imgIdx2camPose, const std::string &cloudPath,
                   const std::vector<bool> &inliers)
    {
        if (inliers.size() != landmarks.size()) throw std::runtime_error("ImagePrep::saveCloud: one flag per landmark");
        writeCloud(landmarks, imgIdx2camPose, cloudPath, &inliers);
    }

    bool binaryPly = false;

private:
    struct Block {       // one device allocation, freed on every path
        explicit Block(size_t bytes) { if (hipMalloc((void **)&p, bytes ? bytes : 1)) throw std::runtime_error("ImagePrep: out of device memory"); }
        ~Block() { (void)hipFree(p); }
        Block(const Block &) = delete;
        Block &operator=(const Block &) = delete;
        uint8_t *p = nullptr;
    };
    static uint8_t *align(uint8_t *p) { return reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255); }
    static void up(void *dst, const void *src, size_t bytes)
    {
        if (bytes && hipMemcpy(dst, src, bytes, kMemcpyHostToDevice)) throw std::runtime_error("ImagePrep: host to device copy failed");
    }
    static void down(void *dst, const void *src, size_t bytes)
    {
        if (bytes && hipMemcpy(dst, src, bytes, kMemcpyDeviceToHost)) throw std::runtime_error("ImagePrep: device to host copy failed");
    }
    static std::vector<uint8_t> densePixels(const ColourImage &img)
    {
        const size_t row = (size_t)img.cols * img.channels;
        if (img.rows < 1 || img.cols < 1 || img.rowBytes() < row || img.data.size() < (size_t)(img.rows - 1) * img.rowBytes() + row)
            throw std::runtime_error("ImagePrep: the image's buffer is smaller than its shape");
        std::vector<uint8_t> out((size_t)img.rows * row);
        for (int y = 0; y < img.rows; ++y) std::copy(img.at(y, 0), img.at(y, 0) + row, out.begin() + (size_t)y * row);
        return out;
    }

    double prepareHost(ColourImage &img, int imgMaxSize, int order, GreyImage *gray)
    {
        const size_t row = (size_t)img.cols * img.channels;
        if (img.rows < 1 || img.cols < 1 || img.rowBytes() < row || img.data.size() < (size_t)(img.rows - 1) * img.rowBytes() + row)
            throw std::runtime_error("ImagePrep: the image's buffer is smaller than its shape");
        int32_t r = 0, c = 0;
        double factor = 1.0;
        if (rcn_img_reshape_size(img.rows, img.cols, imgMaxSize, &r, &c, &factor) != RCN_OK) throw std::runtime_error("ImagePrep: no image is left at this size");
        const bool colour = img.channels == 3;
        const size_t px = (size_t)r * c, srcBytes = (size_t)(img.rows - 1) * img.rowBytes() + row;
        Block d(srcBytes + 256 + 3 * px + 256 + px);
        uint8_t *dSrc = d.p, *dRgb = align(dSrc + srcBytes), *dGray = align(dRgb + 3 * px);
        up(dSrc, img.data.data(), srcBytes);                                   // the row stride travels as it is: the kernel reads padded rows
        int rows = 0, cols = 0;
        const bool wantGray = gray || !colour;
        prepareBatch(dSrc, 1, img.rows, img.cols, img.channels, (int64_t)srcBytes, (int64_t)img.rowBytes(), imgMaxSize, order, colour ? dRgb : nullptr,
                     wantGray ? dGray : nullptr, rows, cols);
        ColourImage out;
        out.rows = r; out.cols = c; out.channels = img.channels; out.step = 0;
        out.data.resize(px * (size_t)img.channels);
        down(out.data.data(), colour ? dRgb : dGray, out.data.size());
        if (gray) {
            gray->rows = r; gray->cols = c; gray->isFloat = false; gray->f32.clear();
            gray->u8.resize(px);
            down(gray->u8.data(), dGray, px);
        }
        img = std::move(out);
        return factor;
    }

    template <class Pose4>
    void writeCloud(std::vector<Landmark> &landmarks, std::unordered_map<int, Pose4> &imgIdx2camPose, const std::string &cloudPath, const std::vector<bool> *inliers)
    {
        const size_t L = landmarks.size(), C = imgIdx2camPose.size();
        std::vector<double> xyz(3 * L), poses;
        std::vector<uint8_t> rgba(4 * L), flags(L);
        for (size_t l = 0; l < L; ++l) {
            xyz[3 * l] = landmarks[l].x; xyz[3 * l + 1] = landmarks[l].y; xyz[3 * l + 2] = landmarks[l].z;
            rgba[4 * l] = (uint8_t)landmarks[l].red; rgba[4 * l + 1] = (uint8_t)landmarks[l].green; rgba[4 * l + 2] = (uint8_t)landmarks[l].blue;
            if (inliers) flags[l] = (*inliers)[l] ? 1 : 0;
        }
        for (const auto &[imgIdx, camPose] : imgIdx2camPose) {
            (void)imgIdx;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) poses.push_back(camPose(r, c));
        }
        const size_t total = (inliers ? 2 : 1) * L + C;
        Block d(24 * L + 256 + 4 * L + 256 + L + 256 + 96 * C + 256 + 16 * total);
        uint8_t *dXyz = d.p, *dCol = align(dXyz + 24 * L), *dInl = align(dCol + 4 * L), *dPose = align(dInl + L + 1), *dOut = align(dPose + 96 * C);
        up(dXyz, xyz.data(), 24 * L); up(dCol, rgba.data(), 4 * L); up(dInl, flags.data(), L); up(dPose, poses.data(), 96 * C);
        int64_t n = 0;
        if (rcn_cloud_vertices_device(ctx_, reinterpret_cast<double *>(dXyz), dCol, inliers ? dInl : nullptr, (int32_t)L, reinterpret_cast<double *>(dPose), (int32_t)C,
                                      dOut, &n) != RCN_OK || rcn_synchronize(ctx_) != RCN_OK)
            throw std::runtime_error(std::string("ImagePrep::saveCloud: ") + rcn_last_error(ctx_));
        std::vector<uint8_t> host(16 * (size_t)n);
        down(host.data(), dOut, host.size());
        if (rcn_cloud_write_ply(cloudPath.c_str(), host.data(), n, binaryPly ? 1 : 0) != RCN_OK)
            throw std::runtime_error("ImagePrep::saveCloud: cannot write " + cloudPath);
    }

    rcn_ctx *ctx_;
    bool owned_;
};

}  // namespace reconstructor::Utils
