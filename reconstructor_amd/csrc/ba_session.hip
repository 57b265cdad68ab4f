// ba_session.hip -- device-resident bundle adjustment across the reference's incremental loop.  C ABI: include/rcn.h.
//
// SequentialReconstructor::reconstruct (SequentialReconstructor.cpp:1040-1094) registers one view at a time and, after
// every view, runs   checkLandmarkValidity -> BundleAdjuster().adjust(everything so far) -> checkLandmarkValidity ->
// removeOutlierLandmarks   on a problem that differs from the previous one by one camera, its new landmarks and a few
// hundred observations: N - 2 global solves, each of which the reference re-packs from its containers.  A session
// keeps that problem where the solver works:
//   in HBM, across solves   the landmark coordinates (in and out of every solve, of the validity sweep, compacted on
//                           the device when outliers are removed), the observation arrays in landmark-major order,
//                           the observation-pair lists of the Schur build (rebuilt on the device only when the graph
//                           has changed), the solver workspace of the ctx
//   host mirror             the graph itself (tracks in triangulatedFeatures order: additions append, exactly like
//                           push_back in the reference) and the 12 numbers per camera, which the solver's accept /
//                           reject logic reads anyway
// Appending a view costs the bytes of what is new; nothing is re-packed.  The arithmetic of a session solve is the
// arithmetic of rcn_ba_solve on the same problem (same kernels, same order): results are identical bit for bit.
#include "rcn_internal.h"
#include "ba_tied.h"

#include <algorithm>
#include <climits>
#include <atomic>
#include <chrono>
#include <cmath>
#include <set>
#include <unordered_map>

namespace {

struct TrackObs { int32_t cam, x, y; };

std::atomic<uint32_t> g_session_ids{1};

// out[k] = in[idx[k]]  (3 doubles per landmark): compaction of the landmark array on the device
__global__ void k_gather_points(const double *__restrict__ in, const int32_t *__restrict__ idx, int n, double *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t s = 3 * (size_t)idx[k];
    out[3 * (size_t)k] = in[s]; out[3 * (size_t)k + 1] = in[s + 1]; out[3 * (size_t)k + 2] = in[s + 2];
}

// a device array that keeps its contents when it grows
struct KeepBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t grow(size_t bytes, size_t used, hipStream_t st)
    {
        if (bytes <= cap) return hipSuccess;
        void *q = nullptr;
        const size_t want = bytes + bytes / 2 + 4096;
        hipError_t e = hipMalloc(&q, want);
        if (e != hipSuccess) return e;
        if (p && used) {
            e = hipMemcpyAsync(q, p, used, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { (void)hipFree(q); return e; }
        }
        if (p) (void)hipFree(p);
        p = q; cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

struct rcn_ba_session {
    rcn_ctx *ctx = nullptr;
    uint32_t id = 0, version = 1;
    std::vector<double> poses, intr;                 // 6 + 6 per camera, rcn_ba_problem layout
    std::vector<std::vector<TrackObs>> tracks;       // per landmark, triangulatedFeatures order
    int64_t n_obs = 0;
    KeepBuf pts;                                     // n_points x 3 doubles, HBM
    DevBuf uv, ocam, opt, xy, pt_off, poses34, intr_dev, inl, keep, cnt, idx, tmp_pts;
    DevBuf t_in, t_xyz, t_ws;                        // rcn_ba_session_triangulate: tracks staged in HBM, every track's X, workspace
    DevBuf g_in;                                     // rcn_ba_session_grow_view: the candidates' CSR arrays and what comes back to the host
    std::vector<char> g_host;                        // ... and its host side
    std::vector<int32_t> h_cam, h_pt;                // flattened graph (host), rebuilt with the device arrays
    std::vector<double> h_uv;
    bool obs_dirty = true;                           // device observation arrays do not reflect `tracks`
    std::vector<uint8_t> last_inlier;                // result of the last validity sweep (for remove_outliers)
    bool have_inlier = false;
    rcn_ba_loss loss{RCN_BA_LOSS_TRIVIAL, 0, 0.0};   // rcn_ba_session_set_loss: the loss of every later solve (trivial: none)
    std::vector<int32_t> groups;                     // rcn_ba_session_set_groups: per camera, -1 = its own intrinsics (shorter than the camera count: the rest are -1; empty: none)
    std::vector<int32_t> loc_groups;                 // ... mapped through a local solve's camera map
    DevBuf cams_dev;                                 // rcn_ba_session_loss_report: the cameras' 6 + 6 numbers, uploaded per call
    BaLocalWs loc;                                   // rcn_ba_session_solve_local / _covisible: the sub-problem's arrays (ba_local.hip)
    std::vector<double> loc_poses, loc_intr;         // ... its cameras' 6 + 6 numbers
    std::vector<uint8_t> loc_free, loc_const;        // ... free per session camera, constant per local camera
    double loc_seconds[3] = {0.0, 0.0, 0.0};         // the last local solve: extraction, rcn_int_ba_solve, scatter (host clock; each ends synchronised)
};

#define SES_HIP(call)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            ctx->set_error(std::string(#call) + ": " + hipGetErrorString(e_));           \
            return RCN_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

// flatten the tracks (landmark-major, track order) and refresh the device copies
static int sync_observations(rcn_ba_session *s)
{
    rcn_ctx *ctx = s->ctx;
    if (!s->obs_dirty) return RCN_OK;
    const size_t no = (size_t)s->n_obs, np = s->tracks.size();
    s->h_cam.resize(no); s->h_pt.resize(no); s->h_uv.resize(2 * no);
    std::vector<int32_t> xy(2 * no), off(np + 1, 0);
    size_t o = 0;
    for (size_t j = 0; j < np; ++j) {
        for (const TrackObs &t : s->tracks[j]) {
            s->h_cam[o] = t.cam; s->h_pt[o] = (int32_t)j;
            s->h_uv[2 * o] = (double)t.x; s->h_uv[2 * o + 1] = (double)t.y;      // integer pixel coordinates cast to double (BundleAdjuster.cpp:83-84)
            xy[2 * o] = t.x; xy[2 * o + 1] = t.y;
            ++o;
        }
        off[j + 1] = (int32_t)o;
    }
    hipStream_t st = ctx->stream;
    SES_HIP(s->uv.reserve(std::max<size_t>(1, 2 * no) * sizeof(double)));
    SES_HIP(s->ocam.reserve(std::max<size_t>(1, no) * sizeof(int32_t)));
    SES_HIP(s->opt.reserve(std::max<size_t>(1, no) * sizeof(int32_t)));
    SES_HIP(s->xy.reserve(std::max<size_t>(1, 2 * no) * sizeof(int32_t)));
    SES_HIP(s->pt_off.reserve((np + 1) * sizeof(int32_t)));
    if (no) {
        SES_HIP(hipMemcpyAsync(s->uv.p, s->h_uv.data(), 2 * no * sizeof(double), hipMemcpyHostToDevice, st));
        SES_HIP(hipMemcpyAsync(s->ocam.p, s->h_cam.data(), no * sizeof(int32_t), hipMemcpyHostToDevice, st));
        SES_HIP(hipMemcpyAsync(s->opt.p, s->h_pt.data(), no * sizeof(int32_t), hipMemcpyHostToDevice, st));
        SES_HIP(hipMemcpyAsync(s->xy.p, xy.data(), 2 * no * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    SES_HIP(hipMemcpyAsync(s->pt_off.p, off.data(), (np + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SES_HIP(hipStreamSynchronize(st));       // xy / off are locals
    s->obs_dirty = false;
    return RCN_OK;
}

extern "C" {

int rcn_ba_session_create(rcn_ctx *ctx, rcn_ba_session **out)
{
    if (!ctx || !out) return RCN_ERR_ARG;
    rcn_ba_session *s = new rcn_ba_session();
    s->ctx = ctx;
    s->id = g_session_ids.fetch_add(1);
    *out = s;
    return RCN_OK;
}

void rcn_ba_session_destroy(rcn_ba_session *s)
{
    if (!s) return;
    rcn_ctx *ctx = s->ctx;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        if ((ctx->ba_pair_token >> 32) == s->id) ctx->ba_pair_token = 0;
        s->pts.release();
        DevBuf *bufs[] = {&s->uv, &s->ocam, &s->opt, &s->xy, &s->pt_off, &s->poses34, &s->intr_dev, &s->inl, &s->keep, &s->cnt, &s->idx, &s->tmp_pts,
                          &s->t_in, &s->t_xyz, &s->t_ws, &s->g_in, &s->cams_dev};
        for (DevBuf *b : bufs) b->release();
        s->loc.release();
    }
    delete s;
}

int rcn_ba_session_add_camera(rcn_ba_session *s, const double *pose6, const double *intr6, int32_t *index_out)
{
    if (!s || !pose6 || !intr6) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->ctx->mu);
    if (index_out) *index_out = (int32_t)(s->poses.size() / 6);
    s->poses.insert(s->poses.end(), pose6, pose6 + 6);
    s->intr.insert(s->intr.end(), intr6, intr6 + 6);
    ++s->version;                 // the tangent columns / the reduced system change with the camera count
    return RCN_OK;
}

int rcn_ba_session_cameras(rcn_ba_session *s, double *poses_out, double *intr_out, const double *poses_in, const double *intr_in)
{
    if (!s) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->ctx->mu);
    if (poses_in) std::copy(poses_in, poses_in + s->poses.size(), s->poses.begin());
    if (intr_in) std::copy(intr_in, intr_in + s->intr.size(), s->intr.begin());
    if (poses_out) std::copy(s->poses.begin(), s->poses.end(), poses_out);
    if (intr_out) std::copy(s->intr.begin(), s->intr.end(), intr_out);
    return RCN_OK;
}

int rcn_ba_session_add_points(rcn_ba_session *s, int32_t n, const double *xyz_host, int32_t *first_index_out)
{
    if (!s || n < 0 || (n > 0 && !xyz_host)) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t np = s->tracks.size();
    if (first_index_out) *first_index_out = (int32_t)np;
    if (n == 0) return RCN_OK;
    SES_HIP(hipSetDevice(ctx->device));
    SES_HIP(s->pts.grow((np + n) * 24, np * 24, ctx->stream));
    SES_HIP(hipMemcpyAsync(static_cast<char *>(s->pts.p) + np * 24, xyz_host, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
    SES_HIP(hipStreamSynchronize(ctx->stream));      // the host rows are borrowed
    s->tracks.resize(np + n);
    s->obs_dirty = true; s->have_inlier = false;
    ++s->version;
    return RCN_OK;
}

int rcn_ba_session_add_observations(rcn_ba_session *s, int32_t n, const int32_t *pt, const int32_t *cam, const int32_t *xy)
{
    if (!s || n < 0 || (n > 0 && (!pt || !cam || !xy))) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t np = (int32_t)s->tracks.size(), nc = (int32_t)(s->poses.size() / 6);
    for (int i = 0; i < n; ++i)
        if (pt[i] < 0 || pt[i] >= np || cam[i] < 0 || cam[i] >= nc) { ctx->set_error("rcn_ba_session_add_observations: landmark or camera index out of range"); return RCN_ERR_ARG; }
    for (int i = 0; i < n; ++i) s->tracks[pt[i]].push_back(TrackObs{cam[i], xy[2 * i], xy[2 * i + 1]});     // triangulatedFeatures.push_back
    s->n_obs += n;
    if (n) { s->obs_dirty = true; s->have_inlier = false; ++s->version; }
    return RCN_OK;
}

int rcn_ba_session_counts(const rcn_ba_session *s, int32_t *n_cams, int32_t *n_points, int64_t *n_obs)
{
    if (!s) return RCN_ERR_ARG;
    if (n_cams) *n_cams = (int32_t)(s->poses.size() / 6);
    if (n_points) *n_points = (int32_t)s->tracks.size();
    if (n_obs) *n_obs = s->n_obs;
    return RCN_OK;
}

int rcn_ba_session_graph(rcn_ba_session *s, int32_t *pt_out, int32_t *cam_out, int32_t *xy_out)
{
    if (!s) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->ctx->mu);
    size_t o = 0;
    for (size_t j = 0; j < s->tracks.size(); ++j)
        for (const TrackObs &t : s->tracks[j]) {
            if (pt_out) pt_out[o] = (int32_t)j;
            if (cam_out) cam_out[o] = t.cam;
            if (xy_out) { xy_out[2 * o] = t.x; xy_out[2 * o + 1] = t.y; }
            ++o;
        }
    return RCN_OK;
}

int rcn_ba_session_solve(rcn_ba_session *s, const rcn_ba_options *options, rcn_ba_summary *summary)
{
    if (!s || !summary) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t nc = (int32_t)(s->poses.size() / 6), np = (int32_t)s->tracks.size();
    if (nc < 1) { ctx->set_error("rcn_ba_session_solve: no camera"); return RCN_ERR_ARG; }
    SES_HIP(hipSetDevice(ctx->device));
    int rc = sync_observations(s);
    if (rc) return rc;
    rcn_ba_options o;
    if (options) o = *options;
    else rcn_ba_default_options(nc, &o);                      // BundleAdjuster.cpp:99-142 for the current camera count
    rcn_ba_problem pb{nc, np, (int32_t)s->n_obs, 0, s->poses.data(), s->intr.data(), nullptr,
                      s->h_uv.data(), s->h_cam.data(), s->h_pt.data()};
    BaResident res{static_cast<double *>(s->pts.p), s->uv.as<double>(), s->ocam.as<int>(), s->opt.as<int>(),
                   ((uint64_t)s->id << 32) | s->version};
    s->have_inlier = false;
    if (!s->groups.empty()) s->groups.resize((size_t)nc, -1);      // (cameras added since the groups were set)
    return rcn_int_ba_solve(ctx, &pb, &o, summary, &res,     // poses / intrinsics come back into the host mirror, points stay in HBM
                            s->loss.kind != RCN_BA_LOSS_TRIVIAL ? &s->loss : nullptr, nullptr, nullptr, nullptr, s->groups.empty() ? nullptr : s->groups.data());
}

int rcn_ba_session_set_groups(rcn_ba_session *s, const int32_t *cam_group, int32_t n)
{
    if (!s) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!cam_group && n == 0) { s->groups.clear(); return RCN_OK; }
    const int32_t nc = (int32_t)(s->poses.size() / 6);
    if (!cam_group || n != nc) { ctx->set_error("rcn_ba_session_set_groups: " + std::to_string(n) + " entries for " + std::to_string(nc) + " cameras"); return RCN_ERR_ARG; }
    for (int32_t c = 0; c < n; ++c)
        if (cam_group[c] < -1) { ctx->set_error("rcn_ba_session_set_groups: camera " + std::to_string(c) + ": group id " + std::to_string(cam_group[c]) + " is below -1"); return RCN_ERR_ARG; }
    s->groups.assign(cam_group, cam_group + n);
    return RCN_OK;
}

// A local adjustment: the cameras free_cams[] move, with the landmarks they see; every other camera that sees one of those landmarks
// takes part as a constant, every other landmark stays where it is (ba_local.hip).  The sub-problem goes through rcn_int_ba_solve
// like a session's global problem -- resident arrays, the session's loss -- with the constant mask and no pair-list token: lists of a
// sub-problem are never taken for cached, and the ctx's token ends up 0, so the next global solve rebuilds its own.
int rcn_ba_session_solve_local(rcn_ba_session *s, const int32_t *free_cams, int32_t n_free, const rcn_ba_options *options,
                               rcn_ba_summary *summary, int32_t info_out[4])
{
    if (!s || !summary) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    const char *who = "rcn_ba_session_solve_local";
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t nc = (int32_t)(s->poses.size() / 6), np = (int32_t)s->tracks.size();
    if (info_out) std::fill(info_out, info_out + 4, 0);
    if (!free_cams || n_free <= 0) { ctx->set_error(std::string(who) + ": no free camera"); return RCN_ERR_ARG; }
    s->loc_free.assign((size_t)nc, 0);
    for (int32_t k = 0; k < n_free; ++k) {
        const int32_t c = free_cams[k];
        if (c < 0 || c >= nc) { ctx->set_error(std::string(who) + ": camera index out of range"); return RCN_ERR_ARG; }
        if (s->loc_free[c]) { ctx->set_error(std::string(who) + ": camera " + std::to_string(c) + " is listed twice"); return RCN_ERR_ARG; }
        s->loc_free[c] = 1;
    }
    SES_HIP(hipSetDevice(ctx->device));
    int rc = sync_observations(s);
    if (rc) return rc;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    BaLocalWs &w = s->loc;
    rc = rcn_int_ba_local_extract(ctx, w, nc, np, (int32_t)s->n_obs, static_cast<const double *>(s->pts.p), s->uv.as<double>(), s->ocam.as<int32_t>(),
                                  s->pt_off.as<int32_t>(), s->loc_free.data());
    if (rc) return rc;
    const double t1 = now();
    if (w.n_points == 0) { ctx->set_error(std::string(who) + ": the free cameras have no observation: the reduced system has no free parameter"); return RCN_ERR_ARG; }
    const int32_t ncl = w.n_cams;
    s->loc_poses.resize(6 * (size_t)ncl); s->loc_intr.resize(6 * (size_t)ncl); s->loc_const.resize((size_t)ncl);
    // a group moves only when the window frees ALL its members: one that has a member outside -- a constant camera of the sub-problem or
    // a camera that is not part of it at all -- is held, or its members would leave with different intrinsics
    std::set<int32_t> held_ids;
    if (!s->groups.empty()) {
        s->loc_groups.assign((size_t)ncl, -1);
        for (size_t c = 0; c < s->groups.size() && c < (size_t)nc; ++c)
            if (s->groups[c] >= 0 && !s->loc_free[c]) held_ids.insert(s->groups[c]);
    }
    int32_t n_const = 0;
    for (int32_t l = 0; l < ncl; ++l) {
        const int32_t c = w.h_cam_map[l];
        if (c < 0 || c >= nc || (l && c <= w.h_cam_map[l - 1])) { ctx->set_error(std::string(who) + ": camera map out of order"); return RCN_ERR_HIP; }
        std::copy(s->poses.begin() + 6 * (size_t)c, s->poses.begin() + 6 * (size_t)c + 6, s->loc_poses.begin() + 6 * (size_t)l);
        std::copy(s->intr.begin() + 6 * (size_t)c, s->intr.begin() + 6 * (size_t)c + 6, s->loc_intr.begin() + 6 * (size_t)l);
        s->loc_const[l] = s->loc_free[c] ? 0 : 1;
        if (!s->groups.empty() && (size_t)c < s->groups.size() && s->groups[c] >= 0)
            s->loc_groups[l] = held_ids.count(s->groups[c]) ? ba_tied::HELD : s->groups[c];
        n_const += s->loc_const[l];
    }
    if (info_out) { info_out[0] = ncl; info_out[1] = n_const; info_out[2] = w.n_points; info_out[3] = w.n_obs; }
    rcn_ba_options o;
    if (options) o = *options;
    else rcn_ba_default_options(n_free, &o);                  // a local bundle of < 10 views keeps all intrinsics constant
    rcn_ba_problem pb{ncl, w.n_points, w.n_obs, 0, s->loc_poses.data(), s->loc_intr.data(), nullptr,
                      s->h_uv.data(), w.h_ocam.data(), w.h_opt.data()};      // (obs_uv: the solver reads the resident copy; the pointer only has to be there)
    BaResident res{w.pts.as<double>(), w.uv.as<double>(), w.ocam.as<int>(), w.opt.as<int>(), 0};
    s->have_inlier = false;
    rc = rcn_int_ba_solve(ctx, &pb, &o, summary, &res, s->loss.kind != RCN_BA_LOSS_TRIVIAL ? &s->loss : nullptr, nullptr, nullptr, s->loc_const.data(),
                          s->groups.empty() ? nullptr : s->loc_groups.data());
    if (rc != RCN_OK && rc != RCN_ERR_NUMERIC) return rc;     // (a failed solve has still written its last accepted point, as rcn_ba_session_solve leaves it)
    const double t2 = now();
    const int rcs = rcn_int_ba_local_scatter(ctx, w, static_cast<double *>(s->pts.p));
    if (rcs) return rcs;
    for (int32_t l = 0; l < ncl; ++l) {
        if (s->loc_const[l]) continue;
        const int32_t c = w.h_cam_map[l];
        std::copy(s->loc_poses.begin() + 6 * (size_t)l, s->loc_poses.begin() + 6 * (size_t)l + 6, s->poses.begin() + 6 * (size_t)c);
        std::copy(s->loc_intr.begin() + 6 * (size_t)l, s->loc_intr.begin() + 6 * (size_t)l + 6, s->intr.begin() + 6 * (size_t)c);
    }
    s->loc_seconds[0] = t1 - t0; s->loc_seconds[1] = t2 - t1; s->loc_seconds[2] = now() - t2;
    return rc;
}

int rcn_ba_session_local_seconds(const rcn_ba_session *s, double seconds_out[3])
{
    if (!s || !seconds_out) return RCN_ERR_ARG;
    std::copy(s->loc_seconds, s->loc_seconds + 3, seconds_out);
    return RCN_OK;
}

int rcn_ba_session_covisible(rcn_ba_session *s, int32_t cam, int32_t k, int32_t *cams_out, int32_t *n_out, int32_t *counts_out)
{
    if (!s) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    const char *who = "rcn_ba_session_covisible";
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t nc = (int32_t)(s->poses.size() / 6), np = (int32_t)s->tracks.size();
    if (n_out) *n_out = 0;
    if (cam < 0 || cam >= nc) { ctx->set_error(std::string(who) + ": camera index out of range"); return RCN_ERR_ARG; }
    if (k < 0) { ctx->set_error(std::string(who) + ": k is negative"); return RCN_ERR_ARG; }
    if (k > 0 && (!cams_out || !n_out)) { ctx->set_error(std::string(who) + ": no room for the cameras"); return RCN_ERR_ARG; }
    SES_HIP(hipSetDevice(ctx->device));
    int rc = sync_observations(s);
    if (rc) return rc;
    std::vector<int32_t> counts((size_t)nc);
    rc = rcn_int_ba_local_covisible(ctx, s->loc, nc, np, s->ocam.as<int32_t>(), s->pt_off.as<int32_t>(), cam, counts.data());
    if (rc) return rc;
    if (counts_out) std::copy(counts.begin(), counts.end(), counts_out);
    // the selection among n_cams numbers: count descending, ties to the lower index
    std::vector<int32_t> order;
    for (int32_t c = 0; c < nc; ++c) if (c != cam && counts[c] > 0) order.push_back(c);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return counts[a] > counts[b]; });
    const int32_t n = std::min<int32_t>(k, (int32_t)order.size());
    for (int32_t i = 0; i < n; ++i) cams_out[i] = order[i];
    if (n_out) *n_out = n;
    return RCN_OK;
}

int rcn_ba_session_mvs_views(rcn_ba_session *s, const double *poses34_host, int32_t S, int32_t *sources_out, double *range_out, int32_t *covisible_out)
{
    if (!s) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    const char *who = "rcn_ba_session_mvs_views";
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t nc = (int32_t)(s->poses.size() / 6), np = (int32_t)s->tracks.size();
    if (S < 1 || S > RCN_MVS_MAX_SOURCES) { ctx->set_error(std::string(who) + ": S outside 1 .. 16"); return RCN_ERR_ARG; }
    if (nc > 0 && (!poses34_host || !sources_out || !range_out)) { ctx->set_error(std::string(who) + ": null pointer"); return RCN_ERR_ARG; }
    if (nc > 16384) { ctx->set_error(std::string(who) + ": more than 16384 cameras"); return RCN_ERR_ARG; }
    if (nc == 0) return RCN_OK;
    SES_HIP(hipSetDevice(ctx->device));
    int rc = sync_observations(s);
    if (rc) return rc;
    return rcn_int_mvs_views(ctx, nc, np, s->ocam.as<int32_t>(), s->pt_off.as<int32_t>(), static_cast<const double *>(s->pts.p), poses34_host, S, sources_out, range_out,
                             covisible_out);
}

int rcn_ba_session_set_loss(rcn_ba_session *s, const rcn_ba_loss *loss)
{
    if (!s) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    int kind;
    double a, b;
    const int rc = rcn_int_ba_loss_check(ctx, loss, "rcn_ba_session_set_loss", &kind, &a, &b);
    if (rc) return rc;
    s->loss = loss ? *loss : rcn_ba_loss{RCN_BA_LOSS_TRIVIAL, 0, 0.0};
    s->loss.reserved = 0;
    return RCN_OK;
}

int rcn_ba_session_loss_report(rcn_ba_session *s, rcn_ba_loss_report *report, double *weights_host)
{
    if (!s) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t nc = s->poses.size() / 6;
    SES_HIP(hipSetDevice(ctx->device));
    int rc = sync_observations(s);
    if (rc) return rc;
    SES_HIP(s->cams_dev.reserve(std::max<size_t>(1, 12 * nc) * sizeof(double)));
    double *cd = s->cams_dev.as<double>();
    if (nc) {
        SES_HIP(hipMemcpyAsync(cd, s->poses.data(), 6 * nc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        SES_HIP(hipMemcpyAsync(cd + 6 * nc, s->intr.data(), 6 * nc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    // (a session whose loss is trivial reports like rcn_ba_solve_robust without one: nothing beyond the scale, weights 1)
    return rcn_int_ba_loss_report(ctx, (int)s->n_obs, cd, cd + 6 * nc, static_cast<const double *>(s->pts.p), s->uv.as<double>(), s->ocam.as<int>(),
                                  s->opt.as<int>(), s->loss.kind != RCN_BA_LOSS_TRIVIAL ? &s->loss : nullptr, report, weights_host);
}

int rcn_ba_session_read_points(rcn_ba_session *s, double *xyz_host)
{
    if (!s || !xyz_host) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t np = s->tracks.size();
    if (!np) return RCN_OK;
    SES_HIP(hipSetDevice(ctx->device));
    SES_HIP(hipMemcpyAsync(xyz_host, s->pts.p, np * 24, hipMemcpyDeviceToHost, ctx->stream));
    SES_HIP(hipStreamSynchronize(ctx->stream));
    return RCN_OK;
}

const double *rcn_ba_session_points_device(rcn_ba_session *s) { return s ? static_cast<const double *>(s->pts.p) : nullptr; }

// checkLandmarkValidity on the session's own arrays: the sweep runs on the device; observations it erases are erased
// from the tracks (the reference erases them from triangulatedFeatures in place, SequentialReconstructor.cpp:877-898)
int rcn_ba_session_validity(rcn_ba_session *s, const double *poses34_host, double max_projection_error, double min_triangulation_angle,
                            uint8_t *inlier_out, int32_t *n_inliers_out, int32_t *n_erased_out)
{
    if (!s || !poses34_host) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    const int32_t nc = (int32_t)(s->poses.size() / 6), np = (int32_t)s->tracks.size();
    const size_t no = (size_t)s->n_obs;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        SES_HIP(hipSetDevice(ctx->device));
        int rc = sync_observations(s);
        if (rc) return rc;
        hipStream_t st = ctx->stream;
        SES_HIP(s->poses34.reserve(std::max(nc, 1) * 12 * sizeof(double)));
        SES_HIP(s->intr_dev.reserve(std::max(nc, 1) * 6 * sizeof(double)));
        SES_HIP(s->inl.reserve(std::max(np, 1)));
        SES_HIP(s->keep.reserve(std::max<size_t>(no, 1)));
        SES_HIP(s->cnt.reserve(16));
        SES_HIP(hipMemcpyAsync(s->poses34.p, poses34_host, (size_t)nc * 12 * sizeof(double), hipMemcpyHostToDevice, st));
        SES_HIP(hipMemcpyAsync(s->intr_dev.p, s->intr.data(), (size_t)nc * 6 * sizeof(double), hipMemcpyHostToDevice, st));
        SES_HIP(hipStreamSynchronize(st));
    }
    if (np == 0) { if (n_inliers_out) *n_inliers_out = 0; if (n_erased_out) *n_erased_out = 0; return RCN_OK; }
    rcn_landmark_problem lp{nc, np, (int32_t)no, 0, s->poses34.as<double>(), s->intr_dev.as<double>(), static_cast<const double *>(s->pts.p),
                            s->pt_off.as<int32_t>(), s->ocam.as<int32_t>(), s->xy.as<int32_t>()};
    int rc = rcn_landmark_validity_device(ctx, &lp, max_projection_error, min_triangulation_angle, s->inl.as<uint8_t>(), s->keep.as<uint8_t>(), s->cnt.as<int32_t>());
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::vector<uint8_t> keep(no);
    s->last_inlier.assign(np, 0);
    int32_t n_in = 0;
    SES_HIP(hipMemcpyAsync(s->last_inlier.data(), s->inl.p, np, hipMemcpyDeviceToHost, ctx->stream));
    if (no) SES_HIP(hipMemcpyAsync(keep.data(), s->keep.p, no, hipMemcpyDeviceToHost, ctx->stream));
    SES_HIP(hipMemcpyAsync(&n_in, s->cnt.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SES_HIP(hipStreamSynchronize(ctx->stream));
    int32_t erased = 0;
    size_t o = 0;
    for (int32_t j = 0; j < np; ++j) {
        std::vector<TrackObs> &t = s->tracks[j];
        size_t w = 0;
        for (size_t k = 0; k < t.size(); ++k, ++o) {
            if (keep[o]) t[w++] = t[k];
            else ++erased;
        }
        t.resize(w);
    }
    if (erased) { s->n_obs -= erased; s->obs_dirty = true; ++s->version; }
    s->have_inlier = true;
    if (inlier_out) std::copy(s->last_inlier.begin(), s->last_inlier.end(), inlier_out);
    if (n_inliers_out) *n_inliers_out = n_in;
    if (n_erased_out) *n_erased_out = erased;
    return RCN_OK;
}

// removeOutlierLandmarks (SequentialReconstructor.cpp:956-976) for the flags of the last sweep: the landmark array is
// compacted on the device, the tracks on the host.  new_index_out (may be NULL): n_points entries, -1 = removed.
int rcn_ba_session_remove_outliers(rcn_ba_session *s, int32_t *new_index_out, int32_t *n_removed_out)
{
    if (!s) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!s->have_inlier) { ctx->set_error("rcn_ba_session_remove_outliers: no validity sweep since the last change"); return RCN_ERR_ARG; }
    const int32_t np = (int32_t)s->tracks.size();
    std::vector<int32_t> keep_idx;
    keep_idx.reserve(np);
    for (int32_t j = 0; j < np; ++j) {
        if (s->last_inlier[j]) { if (new_index_out) new_index_out[j] = (int32_t)keep_idx.size(); keep_idx.push_back(j); }
        else if (new_index_out) new_index_out[j] = -1;
    }
    const int32_t left = (int32_t)keep_idx.size();
    if (n_removed_out) *n_removed_out = np - left;
    s->have_inlier = false;
    if (left == np) return RCN_OK;
    SES_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SES_HIP(s->idx.reserve(std::max(left, 1) * sizeof(int32_t)));
    SES_HIP(s->tmp_pts.reserve(std::max(left, 1) * 24));
    if (left) {
        SES_HIP(hipMemcpyAsync(s->idx.p, keep_idx.data(), (size_t)left * sizeof(int32_t), hipMemcpyHostToDevice, st));
        k_gather_points<<<(left + 255) / 256, 256, 0, st>>>(static_cast<const double *>(s->pts.p), s->idx.as<int32_t>(), left, s->tmp_pts.as<double>());
        SES_HIP(hipGetLastError());
        SES_HIP(hipMemcpyAsync(s->pts.p, s->tmp_pts.p, (size_t)left * 24, hipMemcpyDeviceToDevice, st));
        SES_HIP(hipStreamSynchronize(st));
    }
    int64_t no = 0;
    for (int32_t k = 0; k < left; ++k) {
        if (keep_idx[k] != k) s->tracks[k] = std::move(s->tracks[keep_idx[k]]);
        no += (int64_t)s->tracks[k].size();
    }
    s->tracks.resize(left);
    s->n_obs = no;
    s->obs_dirty = true;
    ++s->version;
    return RCN_OK;
}

// triangulateMultiView for a batch of tracks straight into the session (triangulate.hip): the accepted tracks' X are
// compacted by the kernels into the session's point array behind the landmarks already there; the host learns only the
// status bytes and appends the accepted tracks to its mirror of the graph (landmarks.push_back, triangulatedFeatures in
// track order).
int rcn_ba_session_triangulate(rcn_ba_session *s, const double *poses34_host, int32_t n_tracks, const int32_t *trk_off,
                               const int32_t *obs_cam, const int32_t *obs_xy, double max_projection_error, double min_triangulation_angle,
                               uint8_t *status_out, int32_t *first_index_out, int32_t *n_added_out)
{
    if (!s || !poses34_host || n_tracks < 0 || (n_tracks > 0 && (!trk_off || !obs_cam || !obs_xy))) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t nc = (int32_t)(s->poses.size() / 6), np = (int32_t)s->tracks.size();
    if (first_index_out) *first_index_out = np;
    if (n_added_out) *n_added_out = 0;
    if (n_tracks == 0) return RCN_OK;
    const int32_t n_obs = trk_off[n_tracks];
    int rc = rcn_int_triangulate_check(ctx, nc, n_tracks, n_obs, trk_off, obs_cam);
    if (rc) return rc;
    if ((int64_t)np + n_tracks > INT32_MAX) { ctx->set_error("rcn_ba_session_triangulate: too many landmarks"); return RCN_ERR_ARG; }
    SES_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nt = n_tracks, no = n_obs;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_off = 4 * (nt + 1), b_cam = 4 * no, b_xy = 8 * no;
    SES_HIP(s->poses34.reserve(std::max(nc, 1) * 12 * sizeof(double)));
    SES_HIP(s->intr_dev.reserve(std::max(nc, 1) * 6 * sizeof(double)));
    SES_HIP(s->t_in.reserve(al(b_off) + al(b_cam) + al(b_xy) + al(nt) + 256));
    SES_HIP(s->t_xyz.reserve(24 * nt));
    SES_HIP(s->t_ws.reserve(rcn_int_triangulate_ws_bytes(nc, n_tracks)));
    SES_HIP(s->cnt.reserve(16));
    SES_HIP(s->pts.grow(((size_t)np + nt) * 24, (size_t)np * 24, st));          // room for every track behind the landmarks
    char *in = s->t_in.as<char>();
    int32_t *d_off = reinterpret_cast<int32_t *>(in), *d_cam = reinterpret_cast<int32_t *>(in + al(b_off)),
            *d_xy = reinterpret_cast<int32_t *>(in + al(b_off) + al(b_cam));
    uint8_t *d_st = reinterpret_cast<uint8_t *>(in + al(b_off) + al(b_cam) + al(b_xy));
    SES_HIP(hipMemcpyAsync(s->poses34.p, poses34_host, (size_t)nc * 12 * sizeof(double), hipMemcpyHostToDevice, st));
    SES_HIP(hipMemcpyAsync(s->intr_dev.p, s->intr.data(), (size_t)nc * 6 * sizeof(double), hipMemcpyHostToDevice, st));
    SES_HIP(hipMemcpyAsync(d_off, trk_off, b_off, hipMemcpyHostToDevice, st));
    if (no) {
        SES_HIP(hipMemcpyAsync(d_cam, obs_cam, b_cam, hipMemcpyHostToDevice, st));
        SES_HIP(hipMemcpyAsync(d_xy, obs_xy, b_xy, hipMemcpyHostToDevice, st));
    }
    rcn_triangulation_problem dp{nc, n_tracks, n_obs, 0, s->poses34.as<double>(), s->intr_dev.as<double>(), d_off, d_cam, d_xy};
    rc = rcn_int_triangulate_launch(ctx, &dp, max_projection_error, min_triangulation_angle, s->t_ws.p, s->t_xyz.as<double>(), d_st,
                                    static_cast<double *>(s->pts.p), np, s->cnt.as<int32_t>());
    if (rc) return rc;
    std::vector<uint8_t> status(nt);
    int32_t added = 0;
    SES_HIP(hipMemcpyAsync(status.data(), d_st, nt, hipMemcpyDeviceToHost, st));
    SES_HIP(hipMemcpyAsync(&added, s->cnt.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SES_HIP(hipStreamSynchronize(st));
    int32_t n_acc = 0;
    for (size_t j = 0; j < nt; ++j) {
        if (status[j] != 0) continue;
        std::vector<TrackObs> t;
        for (int32_t o = trk_off[j]; o < trk_off[j + 1]; ++o) t.push_back(TrackObs{obs_cam[o], obs_xy[2 * (size_t)o], obs_xy[2 * (size_t)o + 1]});
        s->n_obs += (int64_t)t.size();
        s->tracks.push_back(std::move(t));
        ++n_acc;
    }
    if (n_acc != added) { ctx->set_error("rcn_ba_session_triangulate: accepted count differs from the status bytes"); return RCN_ERR_HIP; }
    if (n_acc) { s->obs_dirty = true; s->have_inlier = false; ++s->version; }
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    if (n_added_out) *n_added_out = n_acc;
    return RCN_OK;
}

// step 1 of triangulateMatchedLandmarks (:497-512) against the session's landmarks (corr2d3d.hip): the points never leave
// HBM, the status bytes come back, and the attached entries are appended to their tracks in list order -- exactly what
// rcn_ba_session_add_observations of those entries does.
int rcn_ba_session_attach(rcn_ba_session *s, const double *poses34_host, int32_t cam, int32_t n, const int32_t *landmark,
                          const int32_t *feat, const int32_t *xy, double max_projection_error, uint8_t *status_out, int32_t *n_added_out)
{
    if (!s || !poses34_host || n < 0 || (n > 0 && (!landmark || !feat || !xy))) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t nc = (int32_t)(s->poses.size() / 6), np = (int32_t)s->tracks.size();
    if (n_added_out) *n_added_out = 0;
    if (cam < 0 || cam >= nc) { ctx->set_error("rcn_ba_session_attach: camera index out of range"); return RCN_ERR_ARG; }
    int32_t n_feat = 0;
    int rc = rcn_int_attach_check(ctx, "rcn_ba_session_attach", np, n, landmark, feat, &n_feat);
    if (rc) return rc;
    if (n == 0) return RCN_OK;
    SES_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_e = al(4 * (size_t)n);
    SES_HIP(ctx->att_ws.reserve(256 + 4 * b_e + al((size_t)n) + rcn_int_attach_ws_bytes(n_feat)));
    char *w = ctx->att_ws.as<char>();
    double *d_P = reinterpret_cast<double *>(w), *d_K = reinterpret_cast<double *>(w + 128);
    int32_t *d_lm = reinterpret_cast<int32_t *>(w + 256), *d_ft = reinterpret_cast<int32_t *>(w + 256 + b_e),
            *d_xy = reinterpret_cast<int32_t *>(w + 256 + 2 * b_e);
    uint8_t *d_st = reinterpret_cast<uint8_t *>(w + 256 + 4 * b_e);
    void *d_ws = w + 256 + 4 * b_e + al((size_t)n);
    SES_HIP(hipMemcpyAsync(d_P, poses34_host + 12 * (size_t)cam, 96, hipMemcpyHostToDevice, st));
    SES_HIP(hipMemcpyAsync(d_K, s->intr.data() + 6 * (size_t)cam, 48, hipMemcpyHostToDevice, st));
    SES_HIP(hipMemcpyAsync(d_lm, landmark, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    SES_HIP(hipMemcpyAsync(d_ft, feat, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    SES_HIP(hipMemcpyAsync(d_xy, xy, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    rc = rcn_int_attach_launch(ctx, d_P, d_K, static_cast<const double *>(s->pts.p), np, n, d_lm, d_ft, d_xy, n_feat,
                               max_projection_error, d_st, d_ws);
    if (rc) return rc;
    std::vector<uint8_t> status((size_t)n);
    SES_HIP(hipMemcpyAsync(status.data(), d_st, (size_t)n, hipMemcpyDeviceToHost, st));
    SES_HIP(hipStreamSynchronize(st));
    int32_t added = 0;
    for (int32_t e = 0; e < n; ++e) {
        if (status[e] != 0) continue;
        s->tracks[landmark[e]].push_back(TrackObs{cam, xy[2 * (size_t)e], xy[2 * (size_t)e + 1]});     // triangulatedFeatures.push_back
        ++added;
    }
    s->n_obs += added;
    if (added) { s->obs_dirty = true; s->have_inlier = false; ++s->version; }
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    if (n_added_out) *n_added_out = added;
    return RCN_OK;
}

// step 3 of triangulateMatchedLandmarks (:514-553) for the new view v, end to end on the device (corr2d3d.hip, triangulate.hip): the
// candidates from the resident lists and the landmark-id table, the triangulation over one row per keypoint of v (rows past the
// candidates are empty tracks), the accepted X compacted behind the session's landmarks, their indices committed to the table.  No
// host synchronisation between the stages; one copy back (count, (reg image, g, f), both pixels and the status per candidate), from
// which the host mirror of the graph is appended exactly as rcn_ba_session_triangulate appends it.
int rcn_ba_session_grow_view(rcn_ba_session *s, const double *poses34_host, int32_t v, int32_t cam_v, int32_t n_reg, const int32_t *reg_img,
                             const int32_t *reg_cam, double max_projection_error, double min_triangulation_angle, int32_t *n_tracks_out,
                             int32_t *trk_src_out, uint8_t *status_out, int32_t *first_index_out, int32_t *n_added_out)
{
    if (!s || !poses34_host || n_reg < 0 || (n_reg > 0 && (!reg_img || !reg_cam))) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    const char *who = "rcn_ba_session_grow_view";
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t nc = (int32_t)(s->poses.size() / 6), np = (int32_t)s->tracks.size();
    if (first_index_out) *first_index_out = np;
    if (n_added_out) *n_added_out = 0;
    if (n_tracks_out) *n_tracks_out = 0;
    if (cam_v < 0 || cam_v >= nc) { ctx->set_error(std::string(who) + ": camera index out of range"); return RCN_ERR_ARG; }
    std::unordered_map<int32_t, int32_t> cam_of;
    for (int32_t k = 0; k < n_reg; ++k) {
        if (reg_cam[k] < 0 || reg_cam[k] >= nc) { ctx->set_error(std::string(who) + ": camera index out of range"); return RCN_ERR_ARG; }
        cam_of[reg_img[k]] = reg_cam[k];
    }
    const int32_t cap = rcn_int_coords_rows(ctx, v);        // one row per keypoint of v: every candidate fits
    if (cap < 0) { ctx->set_error(std::string(who) + ": image " + std::to_string(v) + " has no coordinates (rcn_coords_upload)"); return RCN_ERR_NOT_FOUND; }
    if ((int64_t)np + cap > INT32_MAX) { ctx->set_error(std::string(who) + ": too many landmarks"); return RCN_ERR_ARG; }
    SES_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nt = (size_t)cap;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    // what comes back, contiguous: n_tracks, n_added, 2 words of padding | trk_src 3 nt | obs_xy 4 nt | status nt bytes
    const size_t o_src = 16, o_xy = o_src + 12 * nt, o_st = o_xy + 16 * nt, b_back = o_st + nt;
    const size_t o_off = al(b_back), o_cam = o_off + al(4 * (nt + 1));
    SES_HIP(s->poses34.reserve(std::max(nc, 1) * 12 * sizeof(double)));
    SES_HIP(s->intr_dev.reserve(std::max(nc, 1) * 6 * sizeof(double)));
    SES_HIP(s->g_in.reserve(o_cam + al(8 * std::max<size_t>(nt, 1))));
    SES_HIP(s->t_xyz.reserve(24 * std::max<size_t>(nt, 1)));
    SES_HIP(s->t_ws.reserve(rcn_int_triangulate_ws_bytes(nc, cap)));
    SES_HIP(s->pts.grow(((size_t)np + nt) * 24, (size_t)np * 24, st));          // room for every row behind the landmarks
    char *g = s->g_in.as<char>();
    int32_t *d_hdr = reinterpret_cast<int32_t *>(g), *d_src = reinterpret_cast<int32_t *>(g + o_src), *d_xy = reinterpret_cast<int32_t *>(g + o_xy);
    uint8_t *d_st = reinterpret_cast<uint8_t *>(g + o_st);
    int32_t *d_off = reinterpret_cast<int32_t *>(g + o_off), *d_cam = reinterpret_cast<int32_t *>(g + o_cam);
    SES_HIP(hipMemsetAsync(d_hdr, 0, 16, st));
    SES_HIP(hipMemcpyAsync(s->poses34.p, poses34_host, (size_t)nc * 12 * sizeof(double), hipMemcpyHostToDevice, st));
    SES_HIP(hipMemcpyAsync(s->intr_dev.p, s->intr.data(), (size_t)nc * 6 * sizeof(double), hipMemcpyHostToDevice, st));
    int rc = rcn_int_new_view_tracks(ctx, who, v, n_reg, reg_img, cam_v, reg_cam, cap, d_hdr, d_off, d_cam, d_xy, d_src);
    if (rc) return rc;
    rcn_triangulation_problem dp{nc, cap, 2 * cap, 0, s->poses34.as<double>(), s->intr_dev.as<double>(), d_off, d_cam, d_xy};
    rc = rcn_int_triangulate_launch(ctx, &dp, max_projection_error, min_triangulation_angle, s->t_ws.p, s->t_xyz.as<double>(), d_st,
                                    static_cast<double *>(s->pts.p), np, d_hdr + 1);
    if (rc) return rc;
    rc = rcn_int_new_view_commit(ctx, v, cap, d_hdr, d_src, d_st, np);
    if (rc) return rc;
    s->g_host.resize(b_back);
    SES_HIP(hipMemcpyAsync(s->g_host.data(), g, b_back, hipMemcpyDeviceToHost, st));
    SES_HIP(hipStreamSynchronize(st));
    const int32_t *h_hdr = reinterpret_cast<const int32_t *>(s->g_host.data()), *h_src = reinterpret_cast<const int32_t *>(s->g_host.data() + o_src),
                  *h_xy = reinterpret_cast<const int32_t *>(s->g_host.data() + o_xy);
    const uint8_t *h_st = reinterpret_cast<const uint8_t *>(s->g_host.data() + o_st);
    const int32_t n_tracks = h_hdr[0], added = h_hdr[1];
    if (n_tracks < 0 || n_tracks > cap) { ctx->set_error(std::string(who) + ": candidate count out of range"); return RCN_ERR_HIP; }
    int32_t n_acc = 0;
    for (int32_t j = 0; j < n_tracks; ++j) {
        if (h_st[j] != 0) continue;
        std::vector<TrackObs> t;                     // the registered observation first, as the candidates list it
        t.push_back(TrackObs{cam_of[h_src[3 * (size_t)j]], h_xy[4 * (size_t)j], h_xy[4 * (size_t)j + 1]});
        t.push_back(TrackObs{cam_v, h_xy[4 * (size_t)j + 2], h_xy[4 * (size_t)j + 3]});
        s->n_obs += 2;
        s->tracks.push_back(std::move(t));
        ++n_acc;
    }
    if (n_acc != added) { ctx->set_error(std::string(who) + ": accepted count differs from the status bytes"); return RCN_ERR_HIP; }
    if (n_acc) { s->obs_dirty = true; s->have_inlier = false; ++s->version; }
    if (n_tracks_out) *n_tracks_out = n_tracks;
    if (trk_src_out) std::copy(h_src, h_src + 3 * (size_t)n_tracks, trk_src_out);
    if (status_out) std::copy(h_st, h_st + n_tracks, status_out);
    if (n_added_out) *n_added_out = n_acc;
    return RCN_OK;
}

// registerImagePnP (:559-638) of one view against the session's landmarks (pnp.hip): the points never leave HBM
int rcn_ba_session_pnp(rcn_ba_session *s, int32_t n, const int32_t *landmark, const int32_t *xy, const double *intr6,
                       const rcn_pnp_options *opt, double *pose34_out, uint8_t *mask_out, int32_t *count_out)
{
    if (!s || n < 0) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int64_t off[2] = {0, n};
    return rcn_int_pnp_host(ctx, "rcn_ba_session_pnp", 1, off, landmark, xy, (int32_t)s->tracks.size(), nullptr,
                            static_cast<const double *>(s->pts.p), intr6, opt, pose34_out, nullptr, mask_out, count_out, nullptr);
}

// chooseInitialPair + triangulateInitialPair (:325-394) into an empty session: the search and the pose recovery of
// twoview.hip, the two cameras (the identity, the recovered pose), then every match of the pair -- not the inliers only --
// as a two-observation track through rcn_ba_session_triangulate.
int rcn_ba_session_init_pair(rcn_ba_session *s, int32_t n, const int32_t *xy1, const int32_t *xy2, const double *intr6_1,
                             const double *intr6_2, const rcn_twoview_options *opt, double max_projection_error,
                             double min_triangulation_angle, double *E_out, double *pose34_out, uint8_t *mask_out,
                             uint8_t *cheir_mask_out, int32_t *count_out, int32_t *iterations_out, uint8_t *status_out,
                             int32_t *n_added_out)
{
    if (!s || n < 0 || !intr6_1 || !intr6_2 || !count_out || (n > 0 && (!xy1 || !xy2))) return RCN_ERR_ARG;
    rcn_ctx *ctx = s->ctx;
    double pose34[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<uint8_t> mask((size_t)std::max(n, 1));
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!s->poses.empty() || !s->tracks.empty()) { ctx->set_error("rcn_ba_session_init_pair: the session is not empty"); return RCN_ERR_ARG; }
        const int64_t off[2] = {0, n};
        int rc = rcn_int_twoview_host(ctx, "rcn_ba_session_init_pair", 1, off, xy1, xy2, intr6_1, intr6_2, opt, E_out, pose34 + 12,
                                      mask_out ? mask_out : mask.data(), cheir_mask_out, count_out, iterations_out);
        if (rc) return rc;
        if (pose34_out) std::copy(pose34 + 12, pose34 + 24, pose34_out);
        if (n_added_out) *n_added_out = 0;
        if (count_out[0] < 0) return RCN_OK;                // no pose: the session stays empty
        double pose6[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        rcn_pose34_to_pose6(pose34 + 12, pose6 + 6);
        // the two cameras under the same lock as the emptiness check (rcn_ba_session_add_camera's body, twice)
        s->poses.insert(s->poses.end(), pose6, pose6 + 12);
        s->intr.insert(s->intr.end(), intr6_1, intr6_1 + 6);
        s->intr.insert(s->intr.end(), intr6_2, intr6_2 + 6);
        s->version += 2;
    }
    std::vector<int32_t> off((size_t)n + 1), cam(2 * (size_t)n), xy(4 * (size_t)n);
    for (int32_t e = 0; e < n; ++e) {
        off[e] = 2 * e;
        cam[2 * (size_t)e] = 0; cam[2 * (size_t)e + 1] = 1;
        xy[4 * (size_t)e] = xy1[2 * (size_t)e]; xy[4 * (size_t)e + 1] = xy1[2 * (size_t)e + 1];
        xy[4 * (size_t)e + 2] = xy2[2 * (size_t)e]; xy[4 * (size_t)e + 3] = xy2[2 * (size_t)e + 1];
    }
    off[n] = 2 * n;
    return rcn_ba_session_triangulate(s, pose34, n, off.data(), cam.data(), xy.data(), max_projection_error, min_triangulation_angle,
                                      status_out, nullptr, n_added_out);
}

}  // extern "C"
