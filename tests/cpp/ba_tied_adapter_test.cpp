// ba_tied_adapter_test -- shared intrinsics through both bundle-adjuster adapters (tests/test_ba_tied_cpp.py):
//   BundleAdjuster::setSharedIntrinsics + adjust              (HipBundleAdjuster.h) against rcn_ba_solve_tied on the problem packed by hand
//   IncrementalBundleAdjuster::setSharedIntrinsics + adjust   (HipBundleSession.h) against the same, view by view
// Landmarks, poses, intrinsics and the summary must be equal bit for bit, and every member's PinholeCamera must hold the same six numbers
// after every adjust.  Odd views form one group, views 0 and 2 (in registration order) another, the rest keep intrinsics of their own; a view
// enters with the pipeline's initial intrinsics and takes its group's refined ones in the pack.  With an empty map the adapters give
// rcn_ba_solve's bits again.  Input: the scene file of session_adapter_test (tests/test_cpp_adapter.py writes it).
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

static bool same(const Containers &a, const Containers &b, const std::vector<int> &order)
{
    if (a.landmarks.size() != b.landmarks.size()) return false;
    for (size_t j = 0; j < a.landmarks.size(); ++j)
        if (memcmp(&a.landmarks[j].x, &b.landmarks[j].x, 8) || memcmp(&a.landmarks[j].y, &b.landmarks[j].y, 8) || memcmp(&a.landmarks[j].z, &b.landmarks[j].z, 8)) return false;
    for (int g : order) {
        if (memcmp(a.poses.at(g).m, b.poses.at(g).m, 128)) return false;
        const PinholeCamera &x = a.intr.at(g), &y = b.intr.at(g);
        const double u[6] = {x.fX, x.fY, x.cX, x.cY, x.k1, x.k2}, v[6] = {y.fX, y.fY, y.cX, y.cY, y.k1, y.k2};
        if (memcmp(u, v, 48)) return false;
    }
    return true;
}

// the solve of BundleAdjuster::adjust by hand: packed as BundleAdjuster.cpp:17-97 -- every member on its group's first view's intrinsics --,
// handed to the C entry, unpacked as :149-187
static int by_hand(rcn_ctx *ctx, Containers &c, const std::vector<int> &order, const std::unordered_map<int, int> *groups, rcn_ba_summary *sum)
{
    const int nc = (int)order.size();
    std::vector<double> extr(6 * (size_t)nc), intr(6 * (size_t)nc), pts(3 * c.landmarks.size()), uv;
    std::vector<int32_t> cam, pt, grp((size_t)nc, -1);
    std::unordered_map<int, int> g2l, first;
    for (int l = 0; l < nc; ++l) {
        const PinholeCamera &K = c.intr[order[l]];
        const double k6[6] = {K.fX, K.fY, K.cX, K.cY, K.k1, K.k2};
        std::copy(k6, k6 + 6, intr.begin() + 6 * l);
        if (groups && groups->count(order[l]) && groups->at(order[l]) >= 0) {
            grp[l] = groups->at(order[l]);
            if (!first.count(grp[l])) first[grp[l]] = l;
            else std::copy(intr.begin() + 6 * first[grp[l]], intr.begin() + 6 * first[grp[l]] + 6, intr.begin() + 6 * l);
        }
        detail::rotationToAngleAxis(c.poses[order[l]], &extr[6 * l]);
        for (int i = 0; i < 3; ++i) extr[6 * l + 3 + i] = c.poses[order[l]](i, 3);
        g2l[order[l]] = l;
    }
    for (size_t j = 0; j < c.landmarks.size(); ++j) {
        pts[3 * j] = c.landmarks[j].x; pts[3 * j + 1] = c.landmarks[j].y; pts[3 * j + 2] = c.landmarks[j].z;
        for (const TriangulatedFeature &tf : c.landmarks[j].triangulatedFeatures) {
            const FeaturePtr<> &f = c.feats[tf.imgIdx][tf.featIdx];
            uv.push_back((double)f->featCoord.x); uv.push_back((double)f->featCoord.y);
            cam.push_back(g2l[tf.imgIdx]); pt.push_back((int32_t)j);
        }
    }
    rcn_ba_problem pb{nc, (int32_t)c.landmarks.size(), (int32_t)cam.size(), 0, extr.data(), intr.data(), pts.data(), uv.data(), cam.data(), pt.data()};
    rcn_ba_options opt;
    rcn_ba_default_options(nc, &opt);
    const int rc = groups ? rcn_ba_solve_tied(ctx, &pb, &opt, nullptr, nullptr, grp.data(), sum, nullptr, nullptr) : rcn_ba_solve(ctx, &pb, &opt, sum);
    if (rc != RCN_OK && rc != RCN_ERR_NUMERIC) return rc;
    for (size_t j = 0; j < c.landmarks.size(); ++j) { c.landmarks[j].x = pts[3 * j]; c.landmarks[j].y = pts[3 * j + 1]; c.landmarks[j].z = pts[3 * j + 2]; }
    for (int l = 0; l < nc; ++l) {
        Mat4d T = c.poses[order[l]];
        detail::angleAxisToPose(&extr[6 * l], T);
        c.poses[order[l]] = T;
        PinholeCamera &K = c.intr[order[l]];
        K.fX = intr[6 * l]; K.fY = intr[6 * l + 1]; K.cX = intr[6 * l + 2]; K.cY = intr[6 * l + 3]; K.k1 = intr[6 * l + 4]; K.k2 = intr[6 * l + 5];
    }
    return RCN_OK;
}

static bool members_equal(const Containers &c, const std::vector<int> &order, const std::unordered_map<int, int> &groups)
{
    std::unordered_map<int, int> first;
    for (int g : order) {
        if (!groups.count(g) || groups.at(g) < 0) continue;
        if (!first.count(groups.at(g))) { first[groups.at(g)] = g; continue; }
        const PinholeCamera &x = c.intr.at(g), &y = c.intr.at(first[groups.at(g)]);
        const double u[6] = {x.fX, x.fY, x.cX, x.cY, x.k1, x.k2}, v[6] = {y.fX, y.fY, y.cX, y.cY, y.k1, y.k2};
        if (memcmp(u, v, 48)) return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: ba_tied_adapter_test <scene.bin>\n"); return 2; }
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
    std::unordered_map<int, int> groups;
    for (int r = 0; r < nc; ++r) groups[order[r]] = (r % 2) ? 5 : (r == 0 || r == 2) ? 9 : -1;
    BundleAdjuster whole(ctx);
    IncrementalBundleAdjuster incremental(ctx);
    whole.setSharedIntrinsics(groups);
    incremental.setSharedIntrinsics(groups);      // before the session exists: kept for it
    Containers A, B, H;                     // A: the re-packing adapter, B: the session adapter, H: the C entry by hand
    std::vector<int> lm_of(np, -1);
    std::vector<size_t> used(np, 0);
    std::vector<int> registered;
    int rounds = 0, tied_rounds = 0;
    for (int r = 0; r < nc; ++r) {
        const int g = order[r];
        registered.push_back(g);
        for (Containers *c : {&A, &B, &H}) { c->poses[g] = T0[r]; c->intr[g] = K0[r]; c->feats[g] = {}; }
        if (r < 2) continue;
        for (int j = 0; j < np; ++j) {
            size_t visible = 0;
            while (visible < obs[j].size() && obs[j][visible].cam <= r) ++visible;
            if (visible < 2) continue;
            if (lm_of[j] < 0) {
                lm_of[j] = (int)A.landmarks.size();
                for (Containers *c : {&A, &B, &H}) c->landmarks.emplace_back(X0[j][0], X0[j][1], X0[j][2]);
            }
            for (size_t k = used[j]; k < visible; ++k) {
                const int gi = order[obs[j][k].cam];
                for (Containers *c : {&A, &B, &H}) {
                    c->feats[gi].push_back(std::make_shared<Feature<>>(FeatCoord<>(obs[j][k].x, obs[j][k].y), FeatDesc()));
                    c->feats[gi].back()->landmarkId = lm_of[j];
                    c->landmarks[lm_of[j]].triangulatedFeatures.emplace_back(gi, (int)c->feats[gi].size() - 1);
                }
            }
            used[j] = visible;
        }
        rcn_ba_summary hs;
        if (by_hand(ctx, H, registered, &groups, &hs) != RCN_OK) { fprintf(stderr, "view %d: rcn_ba_solve_tied: %s\n", r, rcn_last_error(ctx)); return 1; }
        whole.adjust(A.feats, A.landmarks, A.poses, A.intr, registered);
        incremental.adjust(B.feats, B.landmarks, B.poses, B.intr, registered);
        ++rounds;
        // (from the tenth view on the reference frees the intrinsics: views 1, 3, 5, ... share four columns, views 0 and 2 four more)
        const int nv = r + 1, members = nv / 2 + 2;
        const int want_dim = 6 * (nv - 1) - 3 + (nv >= 10 ? 4 * (nv - members) + 8 : 0);
        if (hs.reduced_dim != want_dim) { fprintf(stderr, "view %d: the tied system has %d columns, expected %d\n", r, hs.reduced_dim, want_dim); return 1; }
        tied_rounds += nv >= 10;
        if (!same(A, H, registered) || memcmp(&whole.summary.final_cost, &hs.final_cost, 8) || whole.summary.iterations != hs.iterations || whole.summary.reduced_dim != hs.reduced_dim) {
            fprintf(stderr, "view %d: BundleAdjuster with groups is not rcn_ba_solve_tied (iterations %d / %d, cost %.17g / %.17g)\n", r, whole.summary.iterations, hs.iterations,
                    whole.summary.final_cost, hs.final_cost);
            return 1;
        }
        if (!same(B, H, registered) || memcmp(&incremental.summary.final_cost, &hs.final_cost, 8) || incremental.summary.iterations != hs.iterations ||
            incremental.summary.reduced_dim != hs.reduced_dim) {
            fprintf(stderr, "view %d: IncrementalBundleAdjuster with groups is not rcn_ba_solve_tied (iterations %d / %d, cost %.17g / %.17g)\n", r,
                    incremental.summary.iterations, hs.iterations, incremental.summary.final_cost, hs.final_cost);
            return 1;
        }
        if (!members_equal(A, registered, groups) || !members_equal(B, registered, groups)) { fprintf(stderr, "view %d: the members of a group hold different intrinsics\n", r); return 1; }
    }
    if (incremental.rebuilds() != 0) { fprintf(stderr, "the session was rebuilt %d times\n", incremental.rebuilds()); return 1; }
    if (tied_rounds == 0) { fprintf(stderr, "no adjust with free intrinsics: the scene does not exercise the groups\n"); return 1; }
    // the groups switched off again: both adapters give rcn_ba_solve's bits on the same containers
    whole.setSharedIntrinsics({});
    incremental.setSharedIntrinsics({});
    rcn_ba_summary hs;
    if (by_hand(ctx, H, registered, nullptr, &hs) != RCN_OK) { fprintf(stderr, "rcn_ba_solve: %s\n", rcn_last_error(ctx)); return 1; }
    whole.adjust(A.feats, A.landmarks, A.poses, A.intr, registered);
    incremental.adjust(B.feats, B.landmarks, B.poses, B.intr, registered);
    if (!same(A, H, registered) || !same(B, H, registered) || memcmp(&whole.summary.final_cost, &hs.final_cost, 8) || memcmp(&incremental.summary.final_cost, &hs.final_cost, 8) ||
        whole.summary.reduced_dim != hs.reduced_dim || incremental.rebuilds() != 0) {
        fprintf(stderr, "without groups the adapters are not rcn_ba_solve (cost %.17g / %.17g / %.17g)\n", whole.summary.final_cost, incremental.summary.final_cost, hs.final_cost);
        return 1;
    }
    printf("ba_tied_adapter_test ok: %d adjusts, %d of them with tied intrinsics, %zu landmarks; without groups again: %d columns, %d iterations to cost %.6f\n", rounds, tied_rounds,
           B.landmarks.size(), hs.reduced_dim, hs.iterations, incremental.summary.final_cost);
    rcn_destroy(ctx);
    return 0;
}
