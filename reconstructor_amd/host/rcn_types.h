// rcn_types.h -- boundary types of the hot path, re-declared without OpenCV / Eigen / PCL.
//
// Same names and member names as the reference (namespace reconstructor::Core) so that the
// adapters below read like the reference's own call sites:
//   FeatCoord / FeatDesc / FeatColor / Feature / FeaturePtr   datatypes.h:10-107
//   FeatCoordConf / FeatureConf                   datatypes.h:30-44, 112-136 (SuperPoint: a confidence per keypoint)
//   TriangulatedFeature / Landmark                datatypes.h:125-183
//   PinholeCamera                                 Camera.h:12-120 (fX,fY,cX,cY,k1,k2 + project)
//   GreyImage                                     the cv::Mat a FeatureDetector takes (FeatureDetector.h:28-31): one grey image
//   ColourImage                                   the cv::Mat Utils::readImg fills (utils.cpp:100-109): interleaved 8-bit pixels
//   ImageMatcher                                  ImageMatcher.h:14-22: the plugin that decides which image pairs are matched
// Only the members the matcher / bundle-adjuster boundary touches are declared.
#pragma once
#include <cmath>
#include <cstdint>
#include <filesystem>
#include <map>
#include <memory>
#include <unordered_map>
#include <utility>
#include <vector>

namespace reconstructor::Core {

template <typename coordType = int> struct FeatCoord {
    FeatCoord() = default;
    FeatCoord(coordType x_, coordType y_) : x(x_), y(y_) {}
    coordType x{}, y{};
};

template <typename coordType = int> struct FeatCoordConf : FeatCoord<coordType> {
    FeatCoordConf() = default;
    FeatCoordConf(coordType x_, coordType y_, double conf_) : FeatCoord<coordType>(x_, y_), conf(conf_) {}
    double conf = 0.01;
};

struct FeatDesc {
    FeatDesc() = default;
    template <typename It> FeatDesc(It first, It last) : desc(first, last) {}
    std::vector<float> desc;   // 128 (SIFT) / 32 (ORB as float) / 256 (SuperPoint) floats
};

struct FeatColor {
    FeatColor() = default;
    FeatColor(int red_, int green_, int blue_) : red(red_), green(green_), blue(blue_) {}
    int red = 0, green = 0, blue = 0;
};

template <typename coordType = int> struct Feature {
    Feature() = default;
    Feature(FeatCoord<coordType> c, FeatDesc d) : featCoord(c), featDesc(std::move(d)) {}
    FeatCoord<coordType> featCoord;
    FeatDesc featDesc;
    FeatColor featColor;       // the pixel under the feature (SequentialReconstructor.cpp:98-106); zero until extractFeatureColors fills it
    int landmarkId = -1;
};
template <typename coordType = int> using FeaturePtr = std::shared_ptr<Feature<coordType>>;

template <typename coordType = int> struct FeatureConf : Feature<coordType> {
    FeatureConf() = default;
    FeatureConf(FeatCoordConf<coordType> c, FeatDesc d) : Feature<coordType>(static_cast<FeatCoord<coordType>>(c), std::move(d)), conf(c.conf) {}
    double conf = 0.0;
};

struct TriangulatedFeature {
    TriangulatedFeature() = default;
    TriangulatedFeature(int img, int feat) : imgIdx(img), featIdx(feat) {}
    int imgIdx = 0, featIdx = 0;
};

struct Landmark {
    Landmark() = default;
    Landmark(double x_, double y_, double z_) : x(x_), y(y_), z(z_) {}
    Landmark(double x_, double y_, double z_, int red_, int green_, int blue_) : x(x_), y(y_), z(z_), red(red_), green(green_), blue(blue_) {}
    std::vector<TriangulatedFeature> triangulatedFeatures;
    double x = 0, y = 0, z = 0;
    int red = 0, green = 0, blue = 0;      // the colour of the first feature of the track (:429-433)
};

// A grey image, row-major, standing in for cv::Mat where a detector takes one: bytes (the detector's input type) or floats on the 0..255 scale
struct GreyImage {
    int rows = 0, cols = 0;
    bool isFloat = false;
    std::vector<uint8_t> u8;
    std::vector<float> f32;
};

// A decoded photograph standing in for the cv::Mat of Utils::readImg: `channels` interleaved bytes per pixel, rows `step` bytes
// apart (cv::Mat::step: padding allowed; 0 = dense)
struct ColourImage {
    int rows = 0, cols = 0, channels = 3;
    size_t step = 0;
    std::vector<uint8_t> data;
    size_t rowBytes() const { return step ? step : (size_t)cols * channels; }
    const uint8_t *at(int y, int x) const { return data.data() + (size_t)y * rowBytes() + (size_t)x * channels; }
};

// Which images are matched against which: imgMatches[id] lists the partners of image id (the reference ships FakeImgMatcher, every
// other image; HipImageMatcher.h retrieves them).
class ImageMatcher {
public:
    virtual void match(const std::unordered_map<int, std::filesystem::path> &imgIds2Paths,
                       const std::unordered_map<int, std::vector<FeaturePtr<>>> &features,
                       std::unordered_map<int, std::vector<int>> &imgMatches) = 0;
    virtual ~ImageMatcher() {}
};

// 4x4 row-major double matrix standing in for Eigen::Matrix4d at the boundary: M(r,c).
struct Mat4d {
    double m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double &operator()(int r, int c) { return m[4 * r + c]; }
    double operator()(int r, int c) const { return m[4 * r + c]; }
};

}  // namespace reconstructor::Core

// global namespace in the reference too (Camera.h:12)
class PinholeCamera {
public:
    PinholeCamera() = default;
    PinholeCamera(int height, int width, double fx, double fy) : fX(fx), fY(fy), cX(width / 2), cY(height / 2) {}
    // u = fX (x + d) + cX, v = fY (y + d) + cY with d = k1 r + k2 r^2, r = x^2 + y^2: the
    // reference's additive model (Camera.h:59-76), identical to the BA residual.
    std::pair<double, double> project(double X, double Y, double Z) const
    {
        const double x = X / Z, y = Y / Z, r = x * x + y * y, d = k1 * r + k2 * r * r;
        return {fX * (x + d) + cX, fY * (y + d) + cY};
    }
    double fX = 0, fY = 0, cX = 0, cY = 0, k1 = 0, k2 = 0;
};
