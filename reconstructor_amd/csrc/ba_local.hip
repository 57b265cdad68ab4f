// ba_local.hip -- the sub-problem of a local bundle adjustment, cut out of a session's resident arrays on the device.
//
// A local adjustment (COLMAP's FindLocalBundle / AdjustLocalBundle) frees a window of cameras -- the new view and the views that share
// the most landmarks with it -- and holds every other camera that sees one of the window's landmarks constant.  From a byte per
// session camera ("free") and the session's landmark-major arrays this unit builds, on the ctx stream:
//   selected landmarks   those with at least one observation in a free camera; every other landmark (an empty track, or one seen
//                        by non-free cameras only) is left out AND LEFT ALONE: it has no residual in the sub-problem, so nothing
//                        would hold it, and the cameras it constrains outside the window must find it where it was
//   participating cams   those that observe a selected landmark; local index = rank in ascending session index; the ones that are
//                        not free are the constant cameras of the solve (rcn_int_ba_solve's cam_constant)
//   compacted arrays     the selected points, their observations in the original landmark-major, track order (uv, local camera, local
//                        landmark), the local -> session maps
// and, after the solve, scatters the points back.  The covisibility counts that choose the window are the fourth kernel.
// Integer work only: flags (plain stores of one value), integer scans (wgprim.h: exact in any order) and, for the covisibility counts,
// integer atomics -- the extracted arrays do not depend on the launch shape, and neither do the bits of the solve behind them.
#include "rcn_internal.h"
#include "wgprim.h"

#include <algorithm>

namespace {

// One thread per landmark: is it selected, how many observations does it bring (0 when it is not), and -- selected landmarks only --
// which cameras take part.  cam_flag is zero on entry; every store to it writes 1.
__global__ __launch_bounds__(256) void k_loc_select(int np, const int *__restrict__ pt_off, const int *__restrict__ ocam, const uint8_t *__restrict__ free_cam,
                                                     uint8_t *__restrict__ sel, int *__restrict__ cnt, int *__restrict__ cam_flag)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= np) return;
    const int a = pt_off[j], b = pt_off[j + 1];
    bool s = false;
    for (int o = a; o < b; ++o) s = s || free_cam[ocam[o]] != 0;
    sel[j] = s ? 1 : 0;
    cnt[j] = s ? b - a : 0;
    if (s) for (int o = a; o < b; ++o) cam_flag[ocam[o]] = 1;
}

// One workgroup: local landmark index, first local observation and local camera index by exclusive scan; hdr = (local cameras, landmarks,
// observations).  p_loc / o_loc have np + 1 entries, c_loc nc + 1 (the last one is the total).
__global__ __launch_bounds__(1024) void k_loc_scan(int np, int nc, const uint8_t *sel, const int *cnt, const int *cam_flag, int *p_loc, int *o_loc, int *c_loc, int *hdr)
{
    const int n_pts = wg_scan_array<uint8_t, int>(sel, np, p_loc, 0);
    const int n_obs = wg_scan_array<int, int>(cnt, np, o_loc, 0);
    const int n_cam = wg_scan_array<int, int>(cam_flag, nc, c_loc, 0);
    if (threadIdx.x == 0) { p_loc[np] = n_pts; o_loc[np] = n_obs; c_loc[nc] = n_cam; hdr[0] = n_cam; hdr[1] = n_pts; hdr[2] = n_obs; hdr[3] = 0; }
}

// One thread per landmark (its point, its track) and per camera (its entry of the camera map)
__global__ __launch_bounds__(256) void k_loc_compact(int np, int nc, const int *__restrict__ pt_off, const int *__restrict__ ocam, const double *__restrict__ pts,
                                                      const double *__restrict__ uv, const uint8_t *__restrict__ sel, const int *__restrict__ cam_flag,
                                                      const int *__restrict__ p_loc, const int *__restrict__ o_loc, const int *__restrict__ c_loc,
                                                      double *__restrict__ l_pts, double *__restrict__ l_uv, int *__restrict__ l_ocam, int *__restrict__ l_opt,
                                                      int *__restrict__ pt_map, int *__restrict__ cam_map)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nc && cam_flag[j]) cam_map[c_loc[j]] = j;
    if (j >= np || !sel[j]) return;
    const int jl = p_loc[j], a = pt_off[j], b = pt_off[j + 1];
    pt_map[jl] = j;
    for (int k = 0; k < 3; ++k) l_pts[3 * (size_t)jl + k] = pts[3 * (size_t)j + k];
    int ol = o_loc[j];
    for (int o = a; o < b; ++o, ++ol) {
        l_uv[2 * (size_t)ol] = uv[2 * (size_t)o]; l_uv[2 * (size_t)ol + 1] = uv[2 * (size_t)o + 1];
        l_ocam[ol] = c_loc[ocam[o]];
        l_opt[ol] = jl;
    }
}

// pts[pt_map[k]] = l_pts[k]: the solved points back into the session's array (the map is injective)
__global__ __launch_bounds__(256) void k_loc_scatter(int n, const int *__restrict__ pt_map, const double *__restrict__ l_pts, double *__restrict__ pts)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t d = 3 * (size_t)pt_map[k];
    pts[d] = l_pts[3 * (size_t)k]; pts[d + 1] = l_pts[3 * (size_t)k + 1]; pts[d + 2] = l_pts[3 * (size_t)k + 2];
}

// Landmarks shared with camera `cam`, per camera: one thread per landmark; a landmark that sees `cam` counts once for every DISTINCT
// camera of its track (the first occurrence of a camera in the track counts, found by looking back over the track), so counts[cam] is
// the number of landmarks `cam` sees.  counts is zero on entry; integer atomics.
__global__ __launch_bounds__(256) void k_loc_covisible(int np, const int *__restrict__ pt_off, const int *__restrict__ ocam, int cam, int *__restrict__ counts)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= np) return;
    const int a = pt_off[j], b = pt_off[j + 1];
    bool sees = false;
    for (int o = a; o < b; ++o) sees = sees || ocam[o] == cam;
    if (!sees) return;
    for (int o = a; o < b; ++o) {
        const int c = ocam[o];
        bool first = true;
        for (int q = a; q < o; ++q) first = first && ocam[q] != c;
        if (first) atomicAdd(counts + c, 1);
    }
}

}  // namespace

void BaLocalWs::release()
{
    DevBuf *bufs[] = {&flags, &ints, &pts, &uv, &ocam, &opt, &pt_map, &cam_map, &counts};
    for (DevBuf *b : bufs) b->release();
}

// Extraction (ctx->mu held, the session's observation arrays current).  free_host: nc bytes.  On return w.n_cams / n_points / n_obs are the
// sub-problem's sizes, w.h_ocam / h_opt / h_cam_map its structure on the host, everything else stays in HBM.  Sizes of 0 launch nothing.
int rcn_int_ba_local_extract(rcn_ctx *ctx, BaLocalWs &w, int32_t nc, int32_t np, int32_t no, const double *pts, const double *uv,
                             const int32_t *ocam, const int32_t *pt_off, const uint8_t *free_host)
{
    w.n_cams = w.n_points = w.n_obs = 0;
    w.h_ocam.clear(); w.h_opt.clear(); w.h_cam_map.clear();
    if (nc <= 0 || np <= 0 || no <= 0) return RCN_OK;
    hipStream_t st = ctx->stream;
    // flags: free[nc] | sel[np];  ints: cnt[np] | cam_flag[nc] | p_loc[np + 1] | o_loc[np + 1] | c_loc[nc + 1] | hdr[4]
    const size_t n_flags = (size_t)nc + np, n_ints = 3 * (size_t)np + 2 * (size_t)nc + 7;
    RCN_HIP(w.flags.reserve(n_flags));
    RCN_HIP(w.ints.reserve(n_ints * sizeof(int)));
    RCN_HIP(w.pts.reserve(24 * (size_t)np));
    RCN_HIP(w.uv.reserve(16 * (size_t)no));
    RCN_HIP(w.ocam.reserve(4 * (size_t)no));
    RCN_HIP(w.opt.reserve(4 * (size_t)no));
    RCN_HIP(w.pt_map.reserve(4 * (size_t)np));
    RCN_HIP(w.cam_map.reserve(4 * (size_t)nc));
    uint8_t *d_free = w.flags.as<uint8_t>(), *d_sel = d_free + nc;
    int *d_cnt = w.ints.as<int>(), *d_camflag = d_cnt + np, *d_ploc = d_camflag + nc, *d_oloc = d_ploc + np + 1, *d_cloc = d_oloc + np + 1,
        *d_hdr = d_cloc + nc + 1;
    RCN_HIP(hipMemcpyAsync(d_free, free_host, (size_t)nc, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemsetAsync(d_camflag, 0, sizeof(int) * (size_t)nc, st));
    const int grid = (std::max(np, nc) + 255) / 256;
    k_loc_select<<<(np + 255) / 256, 256, 0, st>>>(np, pt_off, ocam, d_free, d_sel, d_cnt, d_camflag);
    k_loc_scan<<<1, 1024, 0, st>>>(np, nc, d_sel, d_cnt, d_camflag, d_ploc, d_oloc, d_cloc, d_hdr);
    k_loc_compact<<<grid, 256, 0, st>>>(np, nc, pt_off, ocam, pts, uv, d_sel, d_camflag, d_ploc, d_oloc, d_cloc, w.pts.as<double>(), w.uv.as<double>(),
                                        w.ocam.as<int>(), w.opt.as<int>(), w.pt_map.as<int>(), w.cam_map.as<int>());
    RCN_HIP(hipGetLastError());
    // What comes back: the three sizes, the camera map and the structure of the sub-problem (local camera and landmark per observation).
    // The sizes are not known before the copy is queued: the copy takes as many observations as the last extraction had, and some more
    // (one synchronisation when the window has not grown much, which is the incremental loop's case), the rest in a second copy.
    int hdr[4] = {0, 0, 0, 0};
    const size_t guess = std::min<size_t>((size_t)no, w.last_obs + w.last_obs / 4 + 4096);
    w.h_ocam.resize((size_t)no); w.h_opt.resize((size_t)no); w.h_cam_map.resize((size_t)nc);
    RCN_HIP(hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(w.h_cam_map.data(), w.cam_map.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, st));      // (entries past the count: whatever was there)
    RCN_HIP(hipMemcpyAsync(w.h_ocam.data(), w.ocam.p, 4 * guess, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(w.h_opt.data(), w.opt.p, 4 * guess, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipStreamSynchronize(st));
    if (hdr[0] < 0 || hdr[0] > nc || hdr[1] < 0 || hdr[1] > np || hdr[2] < 0 || hdr[2] > no) { ctx->set_error("rcn_ba_session_solve_local: sub-problem sizes out of range"); return RCN_ERR_HIP; }
    if ((size_t)hdr[2] > guess) {
        const size_t rest = (size_t)hdr[2] - guess;
        RCN_HIP(hipMemcpyAsync(w.h_ocam.data() + guess, w.ocam.as<int>() + guess, 4 * rest, hipMemcpyDeviceToHost, st));
        RCN_HIP(hipMemcpyAsync(w.h_opt.data() + guess, w.opt.as<int>() + guess, 4 * rest, hipMemcpyDeviceToHost, st));
        RCN_HIP(hipStreamSynchronize(st));
    }
    w.n_cams = hdr[0]; w.n_points = hdr[1]; w.n_obs = hdr[2];
    w.last_obs = (size_t)hdr[2];
    w.h_ocam.resize((size_t)hdr[2]); w.h_opt.resize((size_t)hdr[2]); w.h_cam_map.resize((size_t)hdr[0]);
    return RCN_OK;
}

// The solved points of the last extraction (w.pts) back into the session's landmark array
int rcn_int_ba_local_scatter(rcn_ctx *ctx, BaLocalWs &w, double *pts)
{
    if (w.n_points <= 0) return RCN_OK;
    k_loc_scatter<<<(w.n_points + 255) / 256, 256, 0, ctx->stream>>>(w.n_points, w.pt_map.as<int>(), w.pts.as<double>(), pts);
    RCN_HIP(hipGetLastError());
    RCN_HIP(hipStreamSynchronize(ctx->stream));
    return RCN_OK;
}

// counts_host[nc]: landmarks shared with `cam` per camera (counts_host[cam]: its own landmarks)
int rcn_int_ba_local_covisible(rcn_ctx *ctx, BaLocalWs &w, int32_t nc, int32_t np, const int32_t *ocam, const int32_t *pt_off, int32_t cam, int32_t *counts_host)
{
    std::fill(counts_host, counts_host + nc, 0);
    if (np <= 0) return RCN_OK;
    hipStream_t st = ctx->stream;
    RCN_HIP(w.counts.reserve(4 * (size_t)nc));
    RCN_HIP(hipMemsetAsync(w.counts.p, 0, 4 * (size_t)nc, st));
    k_loc_covisible<<<(np + 255) / 256, 256, 0, st>>>(np, pt_off, ocam, cam, w.counts.as<int>());
    RCN_HIP(hipGetLastError());
    RCN_HIP(hipMemcpyAsync(counts_host, w.counts.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipStreamSynchronize(st));
    return RCN_OK;
}
