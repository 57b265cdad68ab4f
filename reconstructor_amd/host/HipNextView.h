// HipNextView.h -- SequentialReconstructor::chooseInitialPair, ::calc2d3dMatches, ::rankNextImages, ::registerImagePnP and step 1 of
// ::triangulateMatchedLandmarks (SequentialReconstructor.cpp:643-695, :697-759, :559-638, :497-512) over the reference's own
// containers, with the search handed to rcn_corr_2d3d, the pose to rcn_pnp_ransac and the attach rules to rcn_landmark_attach
// (include/rcn.h).
//   uploadMatches     once per reconstruction: every image's keypoint coordinates and the lists featureMatches[(i, c)] for
//                     which i is in imgMatches[c] (calc2d3dMatches' own condition), as given (no mirror)
//   calc2d3dMatches   the reference's signature plus the containers it reads; fills imgIdToLandmarkIds /
//                     imgIdToFeatureIds per candidate in the reference's order.  Throws if a candidate feature already has
//                     a landmark (the reference skips it; in its flow an unregistered image has none, and the device search
//                     does not model the test).
//   rankNextImages    the reference's own ranking code and containers (std::map keyed by score / image id) over the scores
//                     the last calc2d3dMatches computed on the GPU: both modes and their ties exactly as the reference.
//   registerImagePnP  SequentialReconstructor::registerImagePnP (:559-638) through rcn_pnp_ransac: returns the 4 x 4 pose and
//                     trims both lists to the inliers, in list order.  (The reference reads the inlier INDEX list that
//                     cv::solvePnPRansac returns as if it were a byte mask, utils.cpp:328-343; the adapter keeps the entries
//                     whose mask is 1, which is what the code evidently means: DESIGN.md section 17.)  Throws where the
//                     reference would go on with an empty rvec: no model, or fewer than 4 entries.
//   attachMatchedLandmarks  step 1: rcn_landmark_attach, then push_back / landmarkId in list order.
#pragma once
#include <algorithm>
#include <functional>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/rcn.h"
#include "rcn_types.h"

namespace reconstructor::Core {

enum NextImageRankingMode { MatchTotal = 0, MatchDensity = 1 };      // SequentialReconstructor.h:45

class NextViewSearch {
public:
    explicit NextViewSearch(rcn_ctx *ctx = nullptr) : ctx_(ctx), owned_(false)
    {
        if (!ctx_) {
            if (rcn_create(0, &ctx_) != RCN_OK) throw std::runtime_error("NextViewSearch: no usable gfx950 device");
            owned_ = true;
        }
    }
    ~NextViewSearch() { if (owned_) rcn_destroy(ctx_); }
    NextViewSearch(const NextViewSearch &) = delete;
    NextViewSearch &operator=(const NextViewSearch &) = delete;

    NextImageRankingMode nextImageRankingMode = MatchDensity;   // SequentialReconstructor.h:237
    int min2d3dMatchNum = 30;                                   // SequentialReconstructor.h:240
    double maxProjectionError = 4.0;                            // SequentialReconstructor.h:256

    template <class FeatureMatches>
    void uploadMatches(std::unordered_map<int, std::vector<FeaturePtr<>>> &features,
                       std::unordered_map<int, std::vector<int>> &imgMatches, FeatureMatches &featureMatches)
    {
        for (const auto &[imgIdx, feats] : features) {
            std::vector<int32_t> xy;
            for (const auto &f : feats) { xy.push_back(f->featCoord.x); xy.push_back(f->featCoord.y); }
            check(rcn_coords_upload(ctx_, imgIdx, xy.empty() ? nullptr : xy.data(), (int32_t)feats.size()), "rcn_coords_upload");
        }
        std::vector<int32_t> pairs, qt;
        std::vector<int64_t> offsets{0};
        for (const auto &[key, m] : featureMatches) {
            const auto &cm = imgMatches[key.second];
            if (m.empty() || std::find(cm.begin(), cm.end(), key.first) == cm.end()) continue;
            pairs.push_back(key.first); pairs.push_back(key.second);
            for (const auto &[f, g] : m) { qt.push_back(f); qt.push_back(g); }
            offsets.push_back((int64_t)qt.size() / 2);
        }
        check(rcn_match_lists_upload(ctx_, (int32_t)(pairs.size() / 2), pairs.data(), offsets.data(), qt.empty() ? nullptr : qt.data(), 0),
              "rcn_match_lists_upload");
    }

    void calc2d3dMatches(const std::set<int> &candidateImgIds, std::unordered_map<int, std::vector<int>> &imgIdToLandmarkIds,
                         std::unordered_map<int, std::vector<int>> &imgIdToFeatureIds,
                         std::unordered_map<int, std::vector<FeaturePtr<>>> &features, const std::vector<Landmark> &landmarks,
                         std::unordered_map<int, std::pair<int, int>> &imgIdx2imgShape)
    {
        std::vector<int32_t> off{0}, img, feat, cand, shape;
        for (const auto &lm : landmarks) {
            for (const auto &tf : lm.triangulatedFeatures) { img.push_back(tf.imgIdx); feat.push_back(tf.featIdx); }
            off.push_back((int32_t)img.size());
        }
        for (int c : candidateImgIds) {
            cand.push_back(c);
            const auto &s = imgIdx2imgShape.at(c);
            shape.push_back(s.first); shape.push_back(s.second);
        }
        const size_t n = cand.size();
        std::vector<int64_t> coff(n + 1);
        std::vector<int32_t> cells(n + 1), lid, fid;
        int64_t total = 0, cap = (int64_t)std::min<size_t>(img.size() * std::max<size_t>(n, 1), 1u << 20) + 1;
        for (int attempt = 0;; ++attempt) {
            lid.resize(cap); fid.resize(cap);
            const int rc = rcn_corr_2d3d(ctx_, (int32_t)landmarks.size(), off.data(), img.data(), feat.data(), (int32_t)n, cand.data(),
                                         shape.data(), coff.data(), lid.data(), fid.data(), cap, &total, cells.data(), nullptr);
            if (rc == RCN_OK) break;
            if (attempt || total <= cap) check(rc, "rcn_corr_2d3d");
            cap = total;
        }
        lastScore_.clear();
        for (size_t k = 0; k < n; ++k) {
            const int c = cand[k];
            std::vector<int> L(lid.begin() + coff[k], lid.begin() + coff[k + 1]), F(fid.begin() + coff[k], fid.begin() + coff[k + 1]);
            for (int g : F)
                if (features.at(c).at(g)->landmarkId != -1)
                    throw std::runtime_error("calc2d3dMatches: feature " + std::to_string(g) + " of candidate " + std::to_string(c) +
                                             " already has a landmark");
            imgIdToLandmarkIds[c] = std::move(L);
            imgIdToFeatureIds[c] = std::move(F);
            lastScore_[c] = cells[k];
        }
    }

    // :697-759 with projDensity.sum() replaced by the GPU's count of occupied cells
    void rankNextImages(const std::unordered_map<int, std::vector<int>> &imgIdToLandmarkIds,
                        const std::unordered_map<int, std::vector<int>> &imgIdToFeatureIds, std::vector<int> &candidateImgIdsSorted)
    {
        if (nextImageRankingMode == MatchTotal) {
            std::map<int, int, std::greater<int>> imgId2NumMatches;
            for (const auto &[imgId, landmarkIds] : imgIdToLandmarkIds) imgId2NumMatches[imgId] = (int)landmarkIds.size();
            for (const auto &[imgId, numMatches] : imgId2NumMatches) candidateImgIdsSorted.push_back(imgId);
        } else if (nextImageRankingMode == MatchDensity) {
            std::map<int, int, std::greater<int>> score2imgId;
            for (const auto &[imgId, featIds] : imgIdToFeatureIds) score2imgId[lastScore_.at(imgId)] = imgId;
            for (const auto &[score, imgId] : score2imgId)
                if (score > min2d3dMatchNum) candidateImgIdsSorted.push_back(imgId);
        } else {
            throw std::runtime_error("Wrong next image ranking mode!");
        }
    }

    // SequentialReconstructor::chooseInitialPair (:325-375) through rcn_twoview_init: the pair with the most matches (the
    // lexicographically first (i, j) among equals -- the reference's choice among equals is an accident of an unordered_map
    // and an unstable sort), its matches in ascending order of the first image's feature, cv::findEssentialMat's and
    // cv::recoverPose's defaults.  Returns the 4 x 4 pose of the second image relative to the first (|t| = 1); throws when
    // there are no matches or no model.  inlierMatchIds (may be NULL): one flag per match in that order.
    template <class Pose4 = Mat4d, class FeatureMatches>
    Pose4 chooseInitialPair(int &imgIdx1, int &imgIdx2, std::unordered_map<int, std::vector<FeaturePtr<>>> &features,
                            const FeatureMatches &featureMatches, std::unordered_map<int, PinholeCamera> &imgIdx2camIntrinsics,
                            std::vector<bool> *inlierMatchIds = nullptr)
    {
        bool have = false;
        size_t bestN = 0;
        std::pair<int, int> best{0, 0};
        for (const auto &[key, m] : featureMatches) {
            const std::pair<int, int> k(key.first, key.second);
            if (!have || m.size() > bestN || (m.size() == bestN && k < best)) { have = true; bestN = m.size(); best = k; }
        }
        if (!have) throw std::runtime_error("chooseInitialPair: no matches");
        imgIdx1 = best.first; imgIdx2 = best.second;
        std::vector<std::pair<int, int>> qt;
        for (const auto &[key, m] : featureMatches)
            if (key.first == best.first && key.second == best.second) qt.assign(m.begin(), m.end());
        std::sort(qt.begin(), qt.end());
        const size_t n = qt.size();
        std::vector<int32_t> xy1(2 * n + 2), xy2(2 * n + 2);
        for (size_t e = 0; e < n; ++e) {
            const auto &a = features.at(imgIdx1).at(qt[e].first)->featCoord, &b = features.at(imgIdx2).at(qt[e].second)->featCoord;
            xy1[2 * e] = a.x; xy1[2 * e + 1] = a.y; xy2[2 * e] = b.x; xy2[2 * e + 1] = b.y;
        }
        const PinholeCamera &k1 = imgIdx2camIntrinsics.at(imgIdx1), &k2 = imgIdx2camIntrinsics.at(imgIdx2);
        const double K1[6] = {k1.fX, k1.fY, k1.cX, k1.cY, k1.k1, k1.k2}, K2[6] = {k2.fX, k2.fY, k2.cX, k2.cY, k2.k1, k2.k2};
        const int64_t off[2] = {0, (int64_t)n};
        double P[12];
        std::vector<uint8_t> mask(n + 1);
        int32_t count[2] = {0, 0};
        check(rcn_twoview_init(ctx_, 1, off, xy1.data(), xy2.data(), K1, K2, nullptr, nullptr, P, mask.data(), nullptr, count, nullptr),
              "rcn_twoview_init");
        if (count[0] < 0)
            throw std::runtime_error("chooseInitialPair: no pose for the pair (" + std::to_string(imgIdx1) + ", " + std::to_string(imgIdx2) +
                                     (count[0] == -2 ? ") (fewer than 5 matches)" : ") (no model)"));
        if (inlierMatchIds) { inlierMatchIds->clear(); for (size_t e = 0; e < n; ++e) inlierMatchIds->push_back(mask[e] != 0); }
        Pose4 T;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = r == c ? 1.0 : 0.0;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) T(r, c) = P[4 * r + c];
        return T;
    }

    // One candidate of chooseInitialPairByGeometry: the pair, its number of matches and what rcn_twoview_geometry says of it.
    struct PairGeometry {
        int imgIdx1 = 0, imgIdx2 = 0, matches = 0;
        int inliersE = 0, inFront = 0, inliersH = 0, label = RCN_TV_NO_MODEL;
        double ratio = 0.0, medianAngle = 0.0;
    };
    struct PairChoiceReport {
        std::vector<PairGeometry> candidates;   // in candidate order
        int chosen = 0;                         // index into candidates
        bool fallback = false;                  // no candidate passed: candidate 0, the reference's choice
    };

    // chooseInitialPair with a degeneracy check.  The candidates are the options.top_m pairs with the
    // most matches, in chooseInitialPair's order (size descending, then (i, j)); one rcn_twoview_geometry call runs the E
    // search, the H search and the classification on all of them; the choice is the first RCN_TV_GENERAL candidate, else the
    // first RCN_TV_PLANAR one, else candidate 0 with report->fallback set -- exactly chooseInitialPair's pair.  Returns the pose
    // of the chosen pair as chooseInitialPair does (the same bits for the same pair); throws when there are no matches or
    // the chosen pair has no model.  options == NULL: the defaults.
    template <class Pose4 = Mat4d, class FeatureMatches>
    Pose4 chooseInitialPairByGeometry(int &imgIdx1, int &imgIdx2, std::unordered_map<int, std::vector<FeaturePtr<>>> &features,
                                      const FeatureMatches &featureMatches, std::unordered_map<int, PinholeCamera> &imgIdx2camIntrinsics,
                                      const rcn_twoview_geometry_options *options = nullptr, std::vector<bool> *inlierMatchIds = nullptr,
                                      PairChoiceReport *report = nullptr)
    {
        rcn_twoview_geometry_options o;
        if (options) o = *options; else rcn_twoview_geometry_default_options(&o);
        if (o.top_m < 1) throw std::runtime_error("chooseInitialPairByGeometry: top_m >= 1");
        std::vector<std::pair<std::pair<long, std::pair<int, int>>, const typename FeatureMatches::mapped_type *>> order;
        for (const auto &[key, m] : featureMatches)
            order.push_back({{-(long)m.size(), {key.first, key.second}}, &m});
        if (order.empty()) throw std::runtime_error("chooseInitialPairByGeometry: no matches");
        std::sort(order.begin(), order.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        if (order.size() > (size_t)o.top_m) order.resize((size_t)o.top_m);
        const size_t nc = order.size();
        std::vector<int64_t> off(nc + 1, 0);
        std::vector<int32_t> xy1, xy2;
        std::vector<double> K1, K2;
        for (size_t c = 0; c < nc; ++c) {
            const int a = order[c].first.second.first, b = order[c].first.second.second;
            std::vector<std::pair<int, int>> qt(order[c].second->begin(), order[c].second->end());
            std::sort(qt.begin(), qt.end());
            for (const auto &e : qt) {
                const auto &pa = features.at(a).at(e.first)->featCoord, &pb = features.at(b).at(e.second)->featCoord;
                xy1.push_back(pa.x); xy1.push_back(pa.y); xy2.push_back(pb.x); xy2.push_back(pb.y);
            }
            off[c + 1] = off[c] + (int64_t)qt.size();
            const PinholeCamera &k1 = imgIdx2camIntrinsics.at(a), &k2 = imgIdx2camIntrinsics.at(b);
            for (double v : {k1.fX, k1.fY, k1.cX, k1.cY, k1.k1, k1.k2}) K1.push_back(v);
            for (double v : {k2.fX, k2.fY, k2.cX, k2.cY, k2.k1, k2.k2}) K2.push_back(v);
        }
        const size_t ne = (size_t)off[nc];
        xy1.resize(2 * ne + 2); xy2.resize(2 * ne + 2);
        std::vector<double> P(12 * nc), H(9 * nc), ratio(nc), angle(nc);
        std::vector<uint8_t> mask(ne + 1), hmask(ne + 1);
        std::vector<int32_t> count(2 * nc), hcount(nc), label(nc);
        check(rcn_twoview_geometry(ctx_, (int32_t)nc, off.data(), xy1.data(), xy2.data(), K1.data(), K2.data(), nullptr, nullptr, &o, nullptr,
                                   P.data(), mask.data(), nullptr, count.data(), nullptr, H.data(), hmask.data(), hcount.data(), nullptr,
                                   ratio.data(), angle.data(), label.data()),
              "rcn_twoview_geometry");
        size_t pick = 0;
        bool fallback = true;
        for (int want : {(int)RCN_TV_GENERAL, (int)RCN_TV_PLANAR}) {
            for (size_t c = 0; c < nc && fallback; ++c)
                if (label[c] == want) { pick = c; fallback = false; }
            if (!fallback) break;
        }
        if (report) {
            report->candidates.clear();
            for (size_t c = 0; c < nc; ++c) {
                PairGeometry g;
                g.imgIdx1 = order[c].first.second.first; g.imgIdx2 = order[c].first.second.second; g.matches = (int)(off[c + 1] - off[c]);
                g.inliersE = count[2 * c]; g.inFront = count[2 * c + 1]; g.inliersH = hcount[c]; g.label = label[c];
                g.ratio = ratio[c]; g.medianAngle = angle[c];
                report->candidates.push_back(g);
            }
            report->chosen = (int)pick; report->fallback = fallback;
        }
        imgIdx1 = order[pick].first.second.first; imgIdx2 = order[pick].first.second.second;
        if (count[2 * pick] < 0)
            throw std::runtime_error("chooseInitialPairByGeometry: no pose for the pair (" + std::to_string(imgIdx1) + ", " + std::to_string(imgIdx2) +
                                     (count[2 * pick] == -2 ? ") (fewer than 5 matches)" : ") (no model)"));
        if (inlierMatchIds) {
            inlierMatchIds->clear();
            for (int64_t e = off[pick]; e < off[pick + 1]; ++e) inlierMatchIds->push_back(mask[(size_t)e] != 0);
        }
        Pose4 T;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = r == c ? 1.0 : 0.0;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) T(r, c) = P[12 * pick + 4 * r + c];
        return T;
    }

    // :559-638.  maxProjectionError is the threshold (:596), confidence 0.99 and 10000 iterations as the reference passes them.
    template <class Pose4 = Mat4d>
    Pose4 registerImagePnP(int imgIdx, std::vector<int> &featureIdxs, std::vector<int> &landmarkIdxs,
                           std::unordered_map<int, std::vector<FeaturePtr<>>> &features, const std::vector<Landmark> &landmarks,
                           std::unordered_map<int, PinholeCamera> &imgIdx2camIntrinsics)
    {
        if (featureIdxs.size() != landmarkIdxs.size()) throw std::runtime_error("registerImagePnP: lists of different length");
        const size_t n = featureIdxs.size();
        const PinholeCamera &k = imgIdx2camIntrinsics.at(imgIdx);
        const double K[6] = {k.fX, k.fY, k.cX, k.cY, k.k1, k.k2};
        std::vector<double> pts;
        pts.reserve(3 * landmarks.size() + 3);
        for (const auto &lm : landmarks) { pts.push_back(lm.x); pts.push_back(lm.y); pts.push_back(lm.z); }
        std::vector<int32_t> xy, lid(landmarkIdxs.begin(), landmarkIdxs.end());
        for (int f : featureIdxs) { xy.push_back(features.at(imgIdx).at(f)->featCoord.x); xy.push_back(features.at(imgIdx).at(f)->featCoord.y); }
        rcn_pnp_options opt;
        rcn_pnp_default_options(&opt);
        opt.max_projection_error = maxProjectionError;
        const int64_t off[2] = {0, (int64_t)n};
        double P[12];
        std::vector<uint8_t> mask(n + 1);
        int32_t count = 0;
        check(rcn_pnp_ransac(ctx_, 1, off, lid.data(), xy.data(), (int32_t)landmarks.size(), pts.data(), K, &opt, P, nullptr, mask.data(),
                             &count, nullptr), "rcn_pnp_ransac");
        if (count < 0)
            throw std::runtime_error("registerImagePnP: no pose for image " + std::to_string(imgIdx) +
                                     (count == -2 ? " (fewer than 4 matches)" : " (no model)"));
        std::vector<int> keptF, keptL;
        for (size_t e = 0; e < n; ++e)
            if (mask[e]) { keptF.push_back(featureIdxs[e]); keptL.push_back(landmarkIdxs[e]); }
        featureIdxs = std::move(keptF);
        landmarkIdxs = std::move(keptL);
        Pose4 T;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = r == c ? 1.0 : 0.0;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) T(r, c) = P[4 * r + c];
        return T;
    }

    // step 1 of triangulateMatchedLandmarks (:497-512).  Returns the status per entry (0 attached, 1 depth,
    // 2 reprojection, 3 feature already taken).
    template <class Pose4>
    std::vector<uint8_t> attachMatchedLandmarks(int imgIdx, const std::vector<int> &featureIds, const std::vector<int> &landmarkIds,
                                                std::unordered_map<int, std::vector<FeaturePtr<>>> &features,
                                                std::vector<Landmark> &landmarks, std::unordered_map<int, Pose4> &imgIdx2camPose,
                                                std::unordered_map<int, PinholeCamera> &imgIdx2camIntrinsics)
    {
        const size_t n = featureIds.size();
        std::vector<uint8_t> status(n + 1);
        if (n == 0) { status.resize(0); return status; }
        double P[12], K[6];
        const Pose4 &T = imgIdx2camPose.at(imgIdx);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) P[4 * r + c] = T(r, c);
        const PinholeCamera &k = imgIdx2camIntrinsics.at(imgIdx);
        K[0] = k.fX; K[1] = k.fY; K[2] = k.cX; K[3] = k.cY; K[4] = k.k1; K[5] = k.k2;
        std::vector<double> pts;
        pts.reserve(3 * landmarks.size() + 3);
        for (const auto &lm : landmarks) { pts.push_back(lm.x); pts.push_back(lm.y); pts.push_back(lm.z); }
        std::vector<int32_t> xy;
        for (int f : featureIds) { xy.push_back(features.at(imgIdx).at(f)->featCoord.x); xy.push_back(features.at(imgIdx).at(f)->featCoord.y); }
        std::vector<int32_t> lid(landmarkIds.begin(), landmarkIds.end()), fid(featureIds.begin(), featureIds.end());
        check(rcn_landmark_attach(ctx_, P, K, (int32_t)landmarks.size(), pts.data(), (int32_t)n, lid.data(), fid.data(), xy.data(),
                                  maxProjectionError, status.data(), nullptr), "rcn_landmark_attach");
        status.resize(n);
        for (size_t e = 0; e < n; ++e) {
            if (status[e] != 0) continue;
            if (features[imgIdx][featureIds[e]]->landmarkId != -1)
                throw std::runtime_error("attachMatchedLandmarks: feature already has a landmark");
            landmarks[landmarkIds[e]].triangulatedFeatures.emplace_back(imgIdx, featureIds[e]);
            features[imgIdx][featureIds[e]]->landmarkId = landmarkIds[e];
        }
        return status;
    }

private:
    void check(int rc, const char *what)
    {
        if (rc != RCN_OK) throw std::runtime_error(std::string(what) + ": " + rcn_last_error(ctx_));
    }
    rcn_ctx *ctx_;
    bool owned_;
    std::unordered_map<int, int> lastScore_;
};

}  // namespace reconstructor::Core
