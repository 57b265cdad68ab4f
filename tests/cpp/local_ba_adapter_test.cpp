// local_ba_adapter_test -- the reference's incremental loop with a LOCAL adjustment after every registered view
// (IncrementalBundleAdjuster::adjustLocal, HipBundleSession.h: rcn_ba_session_covisible + rcn_ba_session_solve_local) and one global
// adjust at the end.  Checked after every view, against the containers themselves:
//   the window     the new view, then the `window` views that share the most landmarks with it (count descending, ties to the view
//                  registered earlier), counted here from the landmarks' triangulatedFeatures; the first two registered views are
//                  dropped from it (they hold the frame of every global adjust), unless it covers all views: then the adjust is global
//   what moved     only the window's pose matrices and intrinsics, and only landmarks the window sees: everything else keeps its bits
//   localInfo      views of the sub-problem = those that see a landmark of the window; constant = those outside the window
//   the cost       does not rise
// and at the end: the global adjust brings the RMS below a pixel, without a rebuild of the session anywhere.
// Input (tests/test_cpp_adapter.py's scene file): nc, np, order[nc], 4x4 poses, intrinsics, then per scene point its xyz, an
// observation count and (local camera, x, y) records in ascending camera order.  argv[2]: the window (default 3).
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../../reconstructor_amd/host/HipBundleSession.h"

using namespace reconstructor::Core;

static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

struct Obs { int cam, x, y; };
struct Containers {
    std::unordered_map<int, std::vector<FeaturePtr<>>> feats;
    std::vector<Landmark> landmarks;
    std::unordered_map<int, Mat4d> poses;
    std::unordered_map<int, PinholeCamera> intr;
};

static bool same_view(const Containers &a, const Containers &b, int g)
{
    if (memcmp(a.poses.at(g).m, b.poses.at(g).m, 128)) return false;
    const PinholeCamera &x = a.intr.at(g), &y = b.intr.at(g);
    const double u[6] = {x.fX, x.fY, x.cX, x.cY, x.k1, x.k2}, v[6] = {y.fX, y.fY, y.cX, y.cY, y.k1, y.k2};
    return memcmp(u, v, 48) == 0;
}
static bool same_landmark(const Landmark &a, const Landmark &b) { return !memcmp(&a.x, &b.x, 8) && !memcmp(&a.y, &b.y, 8) && !memcmp(&a.z, &b.z, 8); }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: local_ba_adapter_test <scene.bin> [window]\n"); return 2; }
    const int window = argc > 2 ? atoi(argv[2]) : 3;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    int32_t nc, np;
    rd(f, &nc, 4); rd(f, &np, 4);
    std::vector<int> order(nc);
    rd(f, order.data(), 4 * (size_t)nc);
    std::vector<Mat4d> T0(nc);
    std::vector<PinholeCamera> K0(nc);
    for (int l = 0; l < nc; ++l) rd(f, T0[l].m, 128);
    for (int l = 0; l < nc; ++l) { double k[6]; rd(f, k, 48); K0[l].fX = k[0]; K0[l].fY = k[1]; K0[l].cX = k[2]; K0[l].cY = k[3]; K0[l].k1 = k[4]; K0[l].k2 = k[5]; }
    std::vector<std::array<double, 3>> X0(np);
    std::vector<std::vector<Obs>> obs(np);
    for (int j = 0; j < np; ++j) {
        int32_t cnt;
        rd(f, X0[j].data(), 24); rd(f, &cnt, 4);
        for (int k = 0; k < cnt; ++k) { int32_t r[3]; rd(f, r, 12); obs[j].push_back({r[0], r[1], r[2]}); }
    }
    fclose(f);

    rcn_ctx *ctx = nullptr;
    if (rcn_create(0, &ctx) != RCN_OK) { fprintf(stderr, "no device\n"); return 3; }
    IncrementalBundleAdjuster ba(ctx);
    Containers B;
    std::vector<int> lm_of(np, -1);
    std::vector<size_t> used(np, 0);
    std::vector<int> registered;
    int locals = 0, globals = 0;
    for (int r = 0; r < nc; ++r) {
        const int g = order[r];
        registered.push_back(g);
        B.poses[g] = T0[r]; B.intr[g] = K0[r]; B.feats[g] = {};
        if (r < 2) continue;
        for (int j = 0; j < np; ++j) {
            size_t visible = 0;
            while (visible < obs[j].size() && obs[j][visible].cam <= r) ++visible;
            if (visible < 2) continue;
            if (lm_of[j] < 0) { lm_of[j] = (int)B.landmarks.size(); B.landmarks.emplace_back(X0[j][0], X0[j][1], X0[j][2]); }
            for (size_t k = used[j]; k < visible; ++k) {
                const int gi = order[obs[j][k].cam];
                B.feats[gi].push_back(std::make_shared<Feature<>>(FeatCoord<>(obs[j][k].x, obs[j][k].y), FeatDesc()));
                B.feats[gi].back()->landmarkId = lm_of[j];
                B.landmarks[lm_of[j]].triangulatedFeatures.emplace_back(gi, (int)B.feats[gi].size() - 1);
            }
            used[j] = visible;
        }
        // the window, from the containers: landmarks shared with the new view per registered view
        std::unordered_map<int, int> shared;
        for (const Landmark &lm : B.landmarks) {
            std::set<int> views;
            for (const auto &tf : lm.triangulatedFeatures) views.insert(tf.imgIdx);
            if (views.count(g)) for (int v : views) shared[v]++;
        }
        std::vector<int> near;
        for (int k = 0; k < r; ++k) if (shared[order[k]] > 0) near.push_back(k);           // positions in the registration order
        std::stable_sort(near.begin(), near.end(), [&](int a, int b) { return shared[order[a]] > shared[order[b]]; });
        if ((int)near.size() > window) near.resize(window);
        const bool global = (int)near.size() + 1 >= r + 1;                                 // the window covers every view: a global adjust
        if (!global) near.erase(std::remove_if(near.begin(), near.end(), [](int k) { return k < 2; }), near.end());      // the first two views hold the frame
        std::vector<int> want{g};
        for (int k : near) want.push_back(order[k]);
        std::set<int> win(want.begin(), want.end());

        const Containers before = B;
        ba.adjustLocal(B.feats, B.landmarks, B.poses, B.intr, registered, g, window);
        if (ba.lastWindow() != want) { fprintf(stderr, "view %d: the window differs from the containers' covisibility\n", r); return 1; }
        (global ? globals : locals)++;
        if (!(ba.summary.final_cost <= ba.summary.initial_cost)) { fprintf(stderr, "view %d: the cost rose\n", r); return 1; }
        if (global) continue;
        std::set<int> takes_part;
        int n_sel = 0, n_moved = 0;
        for (size_t j = 0; j < B.landmarks.size(); ++j) {
            bool sel = false;
            for (const auto &tf : B.landmarks[j].triangulatedFeatures) sel = sel || win.count(tf.imgIdx);
            if (sel) { ++n_sel; for (const auto &tf : B.landmarks[j].triangulatedFeatures) takes_part.insert(tf.imgIdx); }
            const bool moved = !same_landmark(B.landmarks[j], before.landmarks[j]);
            n_moved += moved;
            if (moved && !sel) { fprintf(stderr, "view %d: landmark %zu moved without an observation in the window\n", r, j); return 1; }
        }
        for (int v : registered)
            if (!win.count(v) && !same_view(B, before, v)) { fprintf(stderr, "view %d: view %d outside the window moved\n", r, v); return 1; }
        int moved_views = 0;
        for (int v : want) moved_views += !same_view(B, before, v);
        if (ba.localInfo[0] != (int)takes_part.size() || ba.localInfo[1] != (int)takes_part.size() - (int)want.size() || ba.localInfo[2] != n_sel ||
            moved_views == 0 || n_moved == 0) {
            fprintf(stderr, "view %d: sub-problem of %d views (%d constant), %d landmarks; expected %zu views, %d landmarks; %d views and %d landmarks moved\n",
                    r, ba.localInfo[0], ba.localInfo[1], ba.localInfo[2], takes_part.size(), n_sel, moved_views, n_moved);
            return 1;
        }
    }
    ba.adjust(B.feats, B.landmarks, B.poses, B.intr, registered);
    if (!(ba.summary.final_rms_px < 1.0) || ba.rebuilds() != 0 || locals == 0) {
        fprintf(stderr, "final rms %.6f, %d rebuild(s), %d local adjustments\n", ba.summary.final_rms_px, ba.rebuilds(), locals);
        return 1;
    }
    printf("local_ba_adapter_test ok: %d local and %d global adjusts, %zu landmarks, final rms %.6f\n", locals, globals + 1, B.landmarks.size(),
           ba.summary.final_rms_px);
    rcn_destroy(ctx);
    return 0;
}
