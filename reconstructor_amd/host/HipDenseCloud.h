// HipDenseCloud.h -- the dense stage behind the reference's pipeline, over the C ABI (rcn_mvs_*): the adjusted
// cameras and the prepared photographs -> per-view depth maps -> a dense coloured cloud.  The reference stops at the sparse cloud
// (Utils::saveCloud); this adapter takes the containers its caller holds at that point -- imgIdx2camPose (anything indexable as
// M(r,c), world -> camera), the intrinsics per image (fx fy cx cy k1 k2, PinholeCamera's order), the prepared images of
// Utils::readImg -- and gives the cloud reconstructor_amd.mvs.dense_cloud gives for the same views and plane lists.
//   computeDepthMaps    undistort, sweep: plane / depth / cost per reference view (kept on the host for the caller)
//   denseCloud          ... consistency, fusion: the vertices (16-byte records, rcn_cloud_write_ply's)
//   saveDenseCloud      ... as a PLY file
// Images are identified by the caller's ids; cameras are numbered in ascending id order.  A view: a reference id, its source ids,
// the depth range [near, far] its planes cover uniformly in inverse depth (rcn_ba_session_mvs_views supplies both from a session).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rcn.h"
#include "rcn_types.h"

extern "C" {
int hipMalloc(void **ptr, size_t bytes);
int hipFree(void *ptr);
int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);
}

namespace reconstructor::Utils {

using reconstructor::Core::ColourImage;
using reconstructor::Core::GreyImage;

struct DenseVertex { float x, y, z; uint8_t red, green, blue, alpha; };
static_assert(sizeof(DenseVertex) == 16, "rcn_cloud_write_ply's record");

struct DenseView {
    int refId = 0;
    std::vector<int> sourceIds;
    double nearDepth = 0.0, farDepth = 0.0;
};

struct DepthMaps {
    int rows = 0, cols = 0;
    std::vector<int> refIds;
    std::vector<int16_t> plane;      // [views][rows][cols], -1: invalid
    std::vector<float> depth, cost;
};

class DenseCloud {
public:
    explicit DenseCloud(rcn_ctx *ctx = nullptr) : ctx_(ctx), owned_(false)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("DenseCloud: no usable gfx950 device");
            owned_ = true;
        }
        rcn_mvs_default_options(&options);
    }
    ~DenseCloud()
    {
        release();
        if (owned_) rcn_destroy(ctx_);
    }
    DenseCloud(const DenseCloud &) = delete;
    DenseCloud &operator=(const DenseCloud &) = delete;

    rcn_mvs_options options;
    int numPlanes = 128;

    template <class Pose4>
    DepthMaps computeDepthMaps(const std::map<int, Pose4> &imgIdx2camPose, const std::map<int, std::array<double, 6>> &intrinsics,
                               const std::map<int, GreyImage> &grays, const std::vector<DenseView> &views)
    {
        prepare(imgIdx2camPose, intrinsics, views);
        uploadImages(grays, nullptr);
        sweep();
        DepthMaps m;
        m.rows = rows_; m.cols = cols_;
        for (const DenseView &v : views) m.refIds.push_back(v.refId);
        const size_t px = (size_t)V_ * rows_ * cols_;
        m.plane.resize(px); m.depth.resize(px); m.cost.resize(px);
        down(m.plane.data(), dPlane_, 2 * px); down(m.depth.data(), dDepth_, 4 * px); down(m.cost.data(), dCost_, 4 * px);
        release();
        return m;
    }

    // colours: the prepared RGB images (may be empty: black vertices).  capacity < 0: room for every sampled pixel.
    template <class Pose4>
    std::vector<DenseVertex> denseCloud(const std::map<int, Pose4> &imgIdx2camPose, const std::map<int, std::array<double, 6>> &intrinsics,
                                        const std::map<int, GreyImage> &grays, const std::map<int, ColourImage> &colours, const std::vector<DenseView> &views,
                                        int64_t capacity = -1)
    {
        prepare(imgIdx2camPose, intrinsics, views);
        uploadImages(grays, colours.empty() ? nullptr : &colours);
        sweep();
        const size_t px = (size_t)V_ * rows_ * cols_;
        dMask_ = alloc(px); dCounts_ = alloc(4 * (size_t)V_ + 16);
        check(rcn_mvs_consistency_device(ctx_, table_.data(), V_, S_, (double *)dPoses_, (double *)dIntr_, n_, rows_, cols_, (int16_t *)dPlane_, (float *)dDepth_, &options,
                                         dMask_, (int32_t *)dCounts_), "consistency");
        const int st = std::max(options.stride, 1);
        if (capacity < 0) capacity = (int64_t)V_ * ((rows_ + st - 1) / st) * ((cols_ + st - 1) / st);
        dVert_ = alloc(16 * (size_t)capacity); dFused_ = alloc(16);
        check(rcn_mvs_fuse_device(ctx_, table_.data(), V_, S_, (double *)dPoses_, (double *)dIntr_, n_, dRgb_, rows_, cols_, (float *)dDepth_, dMask_, &options, capacity,
                                  dVert_, (int64_t *)dFused_), "fusion");
        check(rcn_synchronize(ctx_), "synchronize");
        int64_t fused[2] = {0, 0};
        down(fused, dFused_, 16);
        lastTotal = fused[1];
        std::vector<DenseVertex> out((size_t)fused[0]);
        down(out.data(), dVert_, 16 * out.size());
        release();
        return out;
    }

    template <class Pose4>
    size_t saveDenseCloud(const std::map<int, Pose4> &imgIdx2camPose, const std::map<int, std::array<double, 6>> &intrinsics, const std::map<int, GreyImage> &grays,
                          const std::map<int, ColourImage> &colours, const std::vector<DenseView> &views, const std::string &cloudPath, bool binary = true)
    {
        const std::vector<DenseVertex> v = denseCloud(imgIdx2camPose, intrinsics, grays, colours, views);
        if (rcn_cloud_write_ply(cloudPath.c_str(), v.empty() ? nullptr : v.data(), (int64_t)v.size(), binary ? 1 : 0) != RCN_OK)
            throw std::runtime_error("DenseCloud::saveDenseCloud: cannot write " + cloudPath);
        return v.size();
    }

    int64_t lastTotal = 0;           // vertices of the full result of the last denseCloud, also beyond its capacity

private:
    static constexpr int kMemcpyHostToDevice = 1, kMemcpyDeviceToHost = 2;   // hipMemcpyKind

    void check(int rc, const char *what)
    {
        if (rc == RCN_OK) return;
        const std::string msg = std::string("DenseCloud (") + what + "): " + rcn_last_error(ctx_);
        release();
        throw std::runtime_error(msg);
    }
    uint8_t *alloc(size_t bytes)
    {
        void *p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 1)) { release(); throw std::runtime_error("DenseCloud: out of device memory"); }
        blocks_.push_back(p);
        return static_cast<uint8_t *>(p);
    }
    void release()
    {
        for (void *p : blocks_) (void)hipFree(p);
        blocks_.clear();
        dRgb_ = nullptr;
    }
    void up(void *dst, const void *src, size_t bytes)
    {
        if (bytes && hipMemcpy(dst, src, bytes, kMemcpyHostToDevice)) { release(); throw std::runtime_error("DenseCloud: host to device copy failed"); }
    }
    void down(void *dst, const void *src, size_t bytes)
    {
        if (bytes && hipMemcpy(dst, src, bytes, kMemcpyDeviceToHost)) { release(); throw std::runtime_error("DenseCloud: device to host copy failed"); }
    }

    // cameras in ascending id order, the view table in camera indices, the plane lists and homographies (host code of the library)
    template <class Pose4>
    void prepare(const std::map<int, Pose4> &poses, const std::map<int, std::array<double, 6>> &intrinsics, const std::vector<DenseView> &views)
    {
        release();
        n_ = (int)poses.size(); V_ = (int)views.size();
        if (n_ < 2 || V_ < 1) throw std::runtime_error("DenseCloud: at least two cameras and one view");
        index_.clear(); poses34_.clear(); intr_.clear();
        for (const auto &kv : poses) {
            const auto it = intrinsics.find(kv.first);
            if (it == intrinsics.end()) throw std::runtime_error("DenseCloud: a camera without intrinsics");
            index_[kv.first] = (int)index_.size();
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) poses34_.push_back(kv.second(r, c));
            intr_.insert(intr_.end(), it->second.begin(), it->second.end());
        }
        S_ = 1;
        for (const DenseView &v : views) S_ = std::max(S_, (int)v.sourceIds.size());
        table_.assign((size_t)V_ * (1 + S_), -1);
        inv_.assign((size_t)V_ * numPlanes, 0.0);
        H_.assign((size_t)V_ * S_ * numPlanes * 9, 0.0);
        for (int v = 0; v < V_; ++v) {
            int32_t *row = table_.data() + (size_t)v * (1 + S_);
            row[0] = cam(views[v].refId);
            for (size_t s = 0; s < views[v].sourceIds.size(); ++s) row[1 + s] = cam(views[v].sourceIds[s]);
            if (rcn_mvs_inv_depths(views[v].nearDepth, views[v].farDepth, numPlanes, inv_.data() + (size_t)v * numPlanes) != RCN_OK)
                throw std::runtime_error("DenseCloud: a view's depth range or the number of planes is out of range");
            if (rcn_mvs_homographies(poses34_.data(), intr_.data(), row[0], row + 1, S_, inv_.data() + (size_t)v * numPlanes, numPlanes,
                                     H_.data() + (size_t)v * S_ * numPlanes * 9) != RCN_OK)
                throw std::runtime_error("DenseCloud: a view lists its reference among its sources, or has more than 16 sources");
        }
    }
    int cam(int id) const
    {
        const auto it = index_.find(id);
        if (it == index_.end()) throw std::runtime_error("DenseCloud: a view names an image without a camera");
        return it->second;
    }

    void uploadImages(const std::map<int, GreyImage> &grays, const std::map<int, ColourImage> *colours)
    {
        rows_ = cols_ = 0;
        for (const auto &kv : index_) {
            const auto it = grays.find(kv.first);
            if (it == grays.end() || it->second.isFloat || it->second.rows < 1 || it->second.u8.size() != (size_t)it->second.rows * it->second.cols)
                throw std::runtime_error("DenseCloud: every camera needs its prepared 8-bit grey image");
            if (!rows_) { rows_ = it->second.rows; cols_ = it->second.cols; }
            if (it->second.rows != rows_ || it->second.cols != cols_) throw std::runtime_error("DenseCloud: the prepared images must share one size");
        }
        const size_t px = (size_t)rows_ * cols_;
        uint8_t *raw = alloc(px * n_);
        dGray_ = alloc(px * n_);
        for (const auto &kv : index_) up(raw + px * kv.second, grays.at(kv.first).u8.data(), px);
        dPoses_ = alloc(96 * (size_t)n_); dIntr_ = alloc(48 * (size_t)n_);
        up(dPoses_, poses34_.data(), 96 * (size_t)n_); up(dIntr_, intr_.data(), 48 * (size_t)n_);
        check(rcn_img_undistort_device(ctx_, raw, (int64_t)px, cols_, 1, n_, rows_, cols_, (double *)dIntr_, dGray_), "undistort");
        if (colours) {
            uint8_t *rawc = alloc(3 * px * n_);
            dRgb_ = alloc(3 * px * n_);
            std::vector<uint8_t> dense(3 * px);
            for (const auto &kv : index_) {
                const auto it = colours->find(kv.first);
                if (it == colours->end() || it->second.channels != 3 || it->second.rows != rows_ || it->second.cols != cols_ ||
                    it->second.data.size() < (size_t)(rows_ - 1) * it->second.rowBytes() + 3 * (size_t)cols_)
                    throw std::runtime_error("DenseCloud: every camera needs its prepared colour image at the grey image's size");
                for (int y = 0; y < rows_; ++y) std::copy(it->second.at(y, 0), it->second.at(y, 0) + 3 * (size_t)cols_, dense.begin() + 3 * (size_t)y * cols_);
                up(rawc + 3 * px * kv.second, dense.data(), 3 * px);
            }
            check(rcn_img_undistort_device(ctx_, rawc, (int64_t)(3 * px), 3 * (int64_t)cols_, 3, n_, rows_, cols_, (double *)dIntr_, dRgb_), "undistort");
        }
    }

    void sweep()
    {
        const size_t px = (size_t)V_ * rows_ * cols_;
        uint8_t *dH = alloc(8 * H_.size()), *dInv = alloc(8 * inv_.size());
        up(dH, H_.data(), 8 * H_.size()); up(dInv, inv_.data(), 8 * inv_.size());
        dPlane_ = alloc(2 * px); dDepth_ = alloc(4 * px); dCost_ = alloc(4 * px);
        check(rcn_mvs_sweep_device(ctx_, dGray_, (int64_t)rows_ * cols_, cols_, n_, rows_, cols_, table_.data(), V_, S_, (double *)dH, (double *)dInv, numPlanes, &options,
                                   (int16_t *)dPlane_, (float *)dDepth_, (float *)dCost_), "sweep");
        check(rcn_synchronize(ctx_), "synchronize");
    }

    rcn_ctx *ctx_;
    bool owned_;
    int n_ = 0, V_ = 0, S_ = 1, rows_ = 0, cols_ = 0;
    std::map<int, int> index_;
    std::vector<double> poses34_, intr_, inv_, H_;
    std::vector<int32_t> table_;
    std::vector<void *> blocks_;
    uint8_t *dGray_ = nullptr, *dRgb_ = nullptr, *dPoses_ = nullptr, *dIntr_ = nullptr, *dPlane_ = nullptr, *dDepth_ = nullptr, *dCost_ = nullptr,
            *dMask_ = nullptr, *dCounts_ = nullptr, *dVert_ = nullptr, *dFused_ = nullptr;
};

}  // namespace reconstructor::Utils
