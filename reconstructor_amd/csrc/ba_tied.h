// ba_tied.h -- shared intrinsics of the bundle adjuster: cameras tied in groups.
//
// Tying parameters is a linear map.  The per-camera reduced system  S delta = b  has n columns (rcn_int_ba_solve's cam_off / cam_dim /
// cols); P (n x n') has one 1 per row: a pose column, or an intrinsics column of a camera of its own, goes to its own column of the tied
// system, the four intrinsics columns of every member of a group go to the group's four.  The tied system is  S' = P' S P,  b' = P' b,  and
// the per-camera step is  delta = P delta'.  This file is the host side of that: validation of cam_group, its normalisation, the
// per-camera tables and the column map.  The kernels are ba_tied.hip.
//
// Normalisation (what `grp` holds per camera afterwards):
//   OWN  (-1)  the camera's intrinsics are its own: cam_group < 0, intrinsics mode 0, a constant camera, or a group of one camera
//   HELD (-2)  a free camera of a group that has a constant member: the group's intrinsics are held, the camera keeps its pose columns only
//   g >= 0     a member of live group g: no constant member, two cameras or more.  Live groups are numbered in ascending order of their
//              smallest member.
// Column order of the tied system: cameras in index order, each with its pose columns and -- OWN, mode 1 -- its four intrinsics columns
// (n_own columns in all), then four columns (fx, fy, k1, k2: cols 6, 7, 10, 11) per live group.
// Plain C++: no HIP dependency, a host compiler takes this file alone (tests/cpp/ba_tied_test.cpp).
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace ba_tied {

constexpr int OWN = -1, HELD = -2;

struct Plan {
    bool tied = false;                 // false: no live group and no held camera -- the solve is the one without groups, nothing below is used
    int n = 0, n_tied = 0, n_own = 0, n_groups = 0;      // per-camera columns, tied columns, of which the cameras' own, live groups
    std::vector<int> grp;              // [nc] normalised group (above)
    std::vector<uint8_t> intr_free;    // [nc] the camera's intrinsics move (its own columns or its group's)
    std::vector<int> cam_off, cam_dim, cols;      // per-camera tables as the kernels read them: [nc + 1], [nc], [10 nc]
    std::vector<int> map;              // [n] per-camera column -> tied column: a function onto 0 .. n_tied - 1
    std::vector<int> src_off, src;     // CSR [n_tied + 1], [n]: the per-camera columns of a tied column, ascending
    std::vector<int> grp_off, grp_cam; // CSR [n_groups + 1], members of the live groups, ascending
    std::string error;
};

// 0: plan filled.  1: bad argument, plan.error says which.  intr: 6 numbers per camera (members of a group must agree bit for bit).
// cam_constant / cam_group may be null (no constant camera / no groups); n_group is cam_group's length and must equal nc.
// allow_held (the library's own callers: a local window whose group has members outside it): an entry HELD marks a camera whose
// intrinsics are held although no constant member of its group is part of the problem.
inline int build(int nc, int mode, bool fix_cam0_pose, bool fix_cam1_translation, const uint8_t *cam_constant, const int32_t *cam_group,
                 int n_group, const double *intr, Plan &p, bool allow_held = false)
{
    p = Plan();
    if (nc <= 0) { p.error = "no camera"; return 1; }
    if (cam_group && n_group != nc) { p.error = "cam_group has " + std::to_string(n_group) + " entries for " + std::to_string(nc) + " cameras"; return 1; }
    p.grp.assign((size_t)nc, OWN);
    std::map<int, std::vector<int>> members;      // by id; the vectors ascend
    if (cam_group)
        for (int c = 0; c < nc; ++c) {
            if (allow_held && cam_group[c] == HELD) continue;      // (below)
            if (cam_group[c] < -1) { p.error = "camera " + std::to_string(c) + ": group id " + std::to_string(cam_group[c]) + " is below -1"; return 1; }
            if (cam_group[c] >= 0) members[cam_group[c]].push_back(c);
        }
    for (const auto &kv : members)
        for (size_t k = 1; k < kv.second.size() && intr; ++k)
            if (memcmp(intr + 6 * (size_t)kv.second[k], intr + 6 * (size_t)kv.second[0], 6 * sizeof(double)) != 0) {
                p.error = "camera " + std::to_string(kv.second[k]) + " does not enter with the intrinsics of camera " + std::to_string(kv.second[0]) +
                          ", the first member of its group " + std::to_string(kv.first);
                return 1;
            }
    // live groups in ascending order of their smallest member (the map is ordered by id: order the first members)
    std::map<int, const std::vector<int> *> live;
    if (mode == 1)
        for (const auto &kv : members) {
            if (kv.second.size() < 2) continue;      // a singleton is a camera of its own
            bool held = false;
            for (int c : kv.second) held = held || (cam_constant && cam_constant[c]);
            if (!held) { live[kv.second[0]] = &kv.second; continue; }
            for (int c : kv.second)
                if (!(cam_constant && cam_constant[c])) { p.grp[c] = HELD; p.tied = true; }
        }
    if (cam_group && allow_held && mode == 1)
        for (int c = 0; c < nc; ++c)
            if (cam_group[c] == HELD && !(cam_constant && cam_constant[c])) { p.grp[c] = HELD; p.tied = true; }
    p.grp_off.push_back(0);
    for (const auto &kv : live) {
        for (int c : *kv.second) { p.grp[c] = p.n_groups; p.grp_cam.push_back(c); }
        p.grp_off.push_back((int)p.grp_cam.size());
        p.n_groups++;
        p.tied = true;
    }
    // per-camera tables (BundleAdjuster.cpp:99-129 constraints -> tangent columns) and the cameras' own tied columns
    p.cam_off.assign((size_t)nc + 1, 0); p.cam_dim.assign((size_t)nc, 0); p.cols.assign(10 * (size_t)nc, 0); p.intr_free.assign((size_t)nc, 0);
    int n = 0, a = 0;
    for (int c = 0; c < nc; ++c) {
        int dcm = 0;
        const bool constant = cam_constant && cam_constant[c];
        if (!constant && !(c == 0 && fix_cam0_pose)) {
            const int npose = (c == 1 && fix_cam1_translation) ? 3 : 6;
            for (int k = 0; k < npose; ++k) { p.cols[10 * (size_t)c + dcm++] = k; p.map.push_back(a++); }
        }
        if (!constant && mode == 1 && p.grp[c] != HELD) {
            static const int icol[4] = {6, 7, 10, 11};
            for (int k = 0; k < 4; ++k) { p.cols[10 * (size_t)c + dcm++] = icol[k]; p.map.push_back(p.grp[c] == OWN ? a++ : -1 - k); }      // (a member's: filled in below)
            p.intr_free[c] = 1;
        }
        p.cam_off[c] = n; p.cam_dim[c] = dcm; n += dcm;
    }
    p.cam_off[nc] = n;
    p.n = n; p.n_own = a; p.n_tied = a + 4 * p.n_groups;
    for (int c = 0; c < nc; ++c)
        if (p.grp[c] >= 0)
            for (int k = 0; k < 4; ++k) p.map[(size_t)p.cam_off[c] + p.cam_dim[c] - 4 + k] = p.n_own + 4 * p.grp[c] + k;
    p.src_off.assign((size_t)p.n_tied + 1, 0); p.src.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) p.src_off[(size_t)p.map[i] + 1]++;
    for (int t = 0; t < p.n_tied; ++t) p.src_off[t + 1] += p.src_off[t];
    {
        std::vector<int> fill(p.src_off.begin(), p.src_off.end() - 1);
        for (int i = 0; i < n; ++i) p.src[fill[p.map[i]]++] = i;      // (i ascends: so does every list)
    }
    return 0;
}

// What the tied solve keeps in HBM beside the solver's own tables (ba_tied.hip reads it, rcn_int_ba_solve fills it).
struct Dev {
    int nc, n, npad, n_tied, npad_tied, n_own, n_groups, mode;
    double ub;
    const int *cam_off, *cam_dim, *cols, *cam_obs_off;      // the solver's tables
    const int *grp, *map, *src_off, *src, *grp_off, *grp_cam;
    double *C;       // [n][n_groups][4]: a per-camera row folded over the members' columns (the fold's first stage)
    double *dgt;     // [4 n_groups]: the clamped LM diagonal of the groups' columns
    double *S2, *rhs2;      // the tied system (npad_tied^2) and its right-hand side
};

}  // namespace ba_tied

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// ba_tied.hip, all on `st`.  scale: rule 1, behind k_ba_diag(what = 0).  diag: rule 2, behind every launch that writes dgc.  fold: S', b'
// out of S (row stride npad) and rhs.  expand: rule 4.  gradmax, norms: rule 5.
hipError_t rcn_tied_scale(const ba_tied::Dev &t, const double *Uraw, double *sc, int jacobi, hipStream_t st);
hipError_t rcn_tied_diag(const ba_tied::Dev &t, const double *Uraw, const double *sc, double *dgc, double lo, double hi, hipStream_t st);
hipError_t rcn_tied_fold(const ba_tied::Dev &t, const double *S, const double *rhs, double inv_radius, hipStream_t st);
hipError_t rcn_tied_expand(const ba_tied::Dev &t, const double *x, double *out, hipStream_t st);
hipError_t rcn_tied_gradmax(const ba_tied::Dev &t, const double *gcraw, const double *gpraw, int np, const double *intr, double *out, hipStream_t st);
hipError_t rcn_tied_norms(const ba_tied::Dev &t, const double *intr, const double *intr2, double *scal, hipStream_t st);
#endif
