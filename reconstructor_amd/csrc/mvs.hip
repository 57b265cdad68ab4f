// mvs.hip -- plane-sweep depth maps, the cross-view check and the dense cloud (the arithmetic: mvs_geom.h,
// restated in tests/mvs_ref.py, which every output equals bit for bit).
//
//   k_mvs_sweep        one workgroup of 256 lanes per 16 x 16 tile of a reference view, blockIdx.y the view of the batch.  The reference
//                      bytes of tile + halo go to LDS once; each lane keeps Sa and Va of its own window.  Per (plane, source): the lanes
//                      write the ONE sample of every pixel of tile + halo (fronto-parallel planes: a pixel's sample is the same through
//                      every window) to LDS, a horizontal pass forms the row sums of b, b^2, a b and the count of valid samples over
//                      2R + 1 columns for 16 columns x (16 + 2R) rows, and each lane adds 2R + 1 of those rows.  Integer sums: any order
//                      gives the contract's bits.  The sources' costs are folded in source order; the lane keeps the best plane and the
//                      costs on either side of it for the parabola.
//   k_img_undistort    the 5-bit bilinear resample through the additive distortion model, one lane per output pixel
//   k_mvs_consistency  one lane per pixel: lift, project into each source, compare with the source's own depth map
//   k_mvs_fuse_count / _scan / _emit   kept pixels of every stride-th row and column as 16-byte vertices in (view, y, x) order: counts
//                      per row, one exclusive scan (wgprim.h), then each row's workgroup ranks and writes its own vertices
#include "rcn_internal.h"
#include "mvs_geom.h"
#include "wgprim.h"

#include <algorithm>
#include <cmath>

namespace {

#define MV_T 16                            // tile edge
#define MV_W (MV_T + 2 * MG_RMAX)          // tile + halo at the largest radius: 26
#define MV_LD 48                           // words per LDS row of tile + halo: 16 mod 32, so the two rows a half-wave reads in the horizontal
                                           // pass (16 columns each, ds_read_b32: 32 banks) fall on disjoint banks
#define MV_CNT_SHIFT 25                    // row sums of b stay below 11 * 255 * 1024 < 2^22, a window's below 2^25: the valid count rides above
#define MV_MAX_BLOCKS 0x00FFFFFFll

struct MvVertex { float x, y, z; uchar4 c; };
static_assert(sizeof(MvVertex) == 16, "rcn_cloud_write_ply's record");

struct MvSweepArgs {
    const uint8_t *gray;
    int64_t si, sr;                        // bytes between images / rows
    const int32_t *views;                  // [V][1 + 2 S]: reference image, source images (-1: none), the sources' views (consistency)
    const double *H;                       // [V][S][D][9]
    const double *inv;                     // [V][D]
    int16_t *plane;
    float *depth, *cost;
    double max_cost;
    int32_t rows, cols, S, D, R, min_sources, tiles_x;
};

__global__ __launch_bounds__(256) void k_mvs_sweep(MvSweepArgs a)
{
#pragma clang fp contract(off)
    __shared__ int s_a[MV_W * MV_LD], s_b[MV_W * MV_LD];          // reference bytes; samples, -1: not valid
    __shared__ unsigned s_hb[MV_W * MV_T], s_hab[MV_W * MV_T];    // row sums: b | valid count << 25; a b (below 11 * 255 * 255 * 1024 < 2^30)
    __shared__ long long s_hbb[MV_W * MV_T];                      // b^2
    const int tid = threadIdx.x, tx = tid & (MV_T - 1), ty = tid >> 4;
    const int view = blockIdx.y, S = a.S, D = a.D, R = a.R, rows = a.rows, cols = a.cols;
    const int W = MV_T + 2 * R, win = 2 * R + 1, n = win * win;
    const int x0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * MV_T - R, y0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * MV_T - R;      // corner of tile + halo
    const int32_t *vw = a.views + (size_t)view * (1 + 2 * S);
    const uint8_t *ref = a.gray + (int64_t)vw[0] * a.si;

    for (int i = tid; i < W * W; i += 256) {
        const int ly = i / W, lx = i - ly * W, gx = x0 + lx, gy = y0 + ly;
        const bool in = gx >= 0 && gx < cols && gy >= 0 && gy < rows;
        s_a[ly * MV_LD + lx] = in ? (int)ref[(int64_t)gy * a.sr + gx] : 0;
    }
    __syncthreads();
    const int px = x0 + R + tx, py = y0 + R + ty;
    const bool inside = px < cols && py < rows;
    long long Sa = 0, Saa = 0;
    for (int dy = 0; dy < win; ++dy)
        for (int dx = 0; dx < win; ++dx) { const int v = s_a[(ty + dy) * MV_LD + tx + dx]; Sa += v; Saa += v * v; }
    const long long Va = (long long)n * Saa - Sa * Sa;
    const bool pix_ok = inside && px - R >= 0 && px + R < cols && py - R >= 0 && py + R < rows && Va > 0;

    double best = INFINITY, bm = INFINITY, bp = INFINITY, prev = INFINITY;
    int bk = -1;
    for (int k = 0; k < D; ++k) {
        double sum = 0.0;
        int cnt = 0;
        for (int s = 0; s < S; ++s) {
            const int src = vw[1 + s];                         // uniform over the workgroup, and so is the branch around the barriers
            if (src < 0) continue;
            const double *Hp = a.H + (((size_t)view * S + s) * D + k) * 9;
            double H[9];
            for (int i = 0; i < 9; ++i) H[i] = Hp[i];
            const uint8_t *img = a.gray + (int64_t)src * a.si;
            __syncthreads();                                   // the previous round's reads of s_b and the row sums are done
            for (int i = tid; i < W * W; i += 256) {
                const int ly = i / W, lx = i - ly * W, gx = x0 + lx, gy = y0 + ly;
                int b = -1, qu, qv;
                if (gx >= 0 && gx < cols && gy >= 0 && gy < rows && mg_warp(H, gx, gy, rows, cols, &qu, &qv)) b = mg_sample(img, a.sr, 1, rows, cols, qu, qv);
                s_b[ly * MV_LD + lx] = b;
            }
            __syncthreads();
            for (int e = tid; e < W * MV_T; e += 256) {
                const int ly = e >> 4, lx = e & (MV_T - 1);
                unsigned hb = 0, hab = 0;
                long long hbb = 0;
                for (int dx = 0; dx < win; ++dx) {
                    const int b = s_b[ly * MV_LD + lx + dx], av = s_a[ly * MV_LD + lx + dx];
                    if (b >= 0) { hb += (unsigned)b + (1u << MV_CNT_SHIFT); hab += (unsigned)(av * b); hbb += (long long)b * b; }
                }
                s_hb[e] = hb; s_hab[e] = hab; s_hbb[e] = hbb;
            }
            __syncthreads();
            unsigned pb = 0;
            long long Sab = 0, Sbb = 0;
            for (int dy = 0; dy < win; ++dy) {
                const int e = (ty + dy) * MV_T + tx;
                pb += s_hb[e]; Sab += s_hab[e]; Sbb += s_hbb[e];
            }
            double c;
            if (pix_ok && (int)(pb >> MV_CNT_SHIFT) == n && mg_cost(n, Sa, Va, (long long)(pb & ((1u << MV_CNT_SHIFT) - 1u)), Sbb, Sab, &c)) { sum += c; ++cnt; }
        }
        const double c = (cnt >= a.min_sources && cnt > 0) ? sum / (double)cnt : INFINITY;
        if (c < best) { best = c; bk = k; bm = prev; bp = INFINITY; }
        else if (k == bk + 1) bp = c;
        prev = c;
    }
    if (!inside) return;
    const size_t o = ((size_t)view * rows + py) * cols + px;
    if (bk < 0 || best > a.max_cost) { a.plane[o] = -1; a.depth[o] = 0.f; a.cost[o] = INFINITY; return; }
    const double *inv = a.inv + (size_t)view * D;
    const bool have_m = bk > 0 && bm < INFINITY, have_p = bk + 1 < D && bp < INFINITY;
    const double r = mg_refine(bm, best, bp, have_m, have_p, have_m ? inv[bk - 1] : 0.0, inv[bk], have_p ? inv[bk + 1] : 0.0);
    a.plane[o] = (int16_t)bk;
    a.depth[o] = (float)(1.0 / r);
    a.cost[o] = (float)best;
}

__global__ __launch_bounds__(256) void k_img_undistort(const uint8_t *__restrict__ src, int64_t si, int64_t sr, int ch, int rows, int cols, const double *__restrict__ intr,
                                                       uint8_t *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)rows * cols) return;
    const int img = blockIdx.y, y = (int)(i / cols), x = (int)(i - (long long)y * cols);
    double K[6], u, v;
    for (int k = 0; k < 6; ++k) K[k] = intr[6 * (size_t)img + k];
    mg_distort(K, x, y, &u, &v);
    int qu, qv;
    const bool ok = mg_quantise(u, v, rows, cols, &qu, &qv);
    uint8_t *o = out + (((size_t)img * rows + y) * cols + x) * ch;
    for (int c = 0; c < ch; ++c) o[c] = ok ? (uint8_t)((mg_sample(src + (int64_t)img * si + c, sr, ch, rows, cols, qu, qv) + 512) >> 10) : (uint8_t)0;
}

struct MvCheckArgs {
    const int32_t *views;
    const double *poses, *intr;            // [n][12], [n][6]
    const int16_t *plane;
    const float *depth;
    uint8_t *mask;
    int32_t *counts;
    double rel_tol;
    int32_t rows, cols, S, min_consistent;
};

__global__ __launch_bounds__(256) void k_mvs_consistency(MvCheckArgs a)
{
#pragma clang fp contract(off)
    __shared__ int sh[4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, np = (long long)a.rows * a.cols;
    const int view = blockIdx.y, S = a.S;
    const int32_t *vw = a.views + (size_t)view * (1 + 2 * S);
    bool keep = false;
    if (i < np && a.plane[(size_t)view * np + i] >= 0) {
        const int y = (int)(i / a.cols), x = (int)(i - (long long)y * a.cols);
        double Xw[3];
        mg_lift(a.poses + 12 * (size_t)vw[0], a.intr + 6 * (size_t)vw[0], x, y, (double)a.depth[(size_t)view * np + i], Xw);
        int agree = 0;
        for (int s = 0; s < S; ++s) {
            const int src = vw[1 + s], sv = vw[1 + S + s];
            if (src < 0 || sv < 0) continue;
            double u, v, z;
            mg_project(a.poses + 12 * (size_t)src, a.intr + 6 * (size_t)src, Xw, &u, &v, &z);
            if (!(z > 0.0)) continue;
            const double fu = floor(u + 0.5), fv = floor(v + 0.5);
            if (!(fu >= 0.0 && fu <= (double)(a.cols - 1) && fv >= 0.0 && fv <= (double)(a.rows - 1))) continue;
            const size_t o = (size_t)sv * np + (size_t)((int)fv) * a.cols + (int)fu;
            if (a.plane[o] < 0) continue;
            if (fabs(z - (double)a.depth[o]) <= a.rel_tol * z) ++agree;
        }
        keep = agree >= a.min_consistent;
    }
    if (i < np) a.mask[(size_t)view * np + i] = keep ? 1 : 0;
    int total;
    wg_rank<256>(keep, sh, total);
    if (threadIdx.x == 0 && total) atomicAdd(a.counts + view, total);      // integer: exact in any order
}

// kept pixels of sampled row j of a view (row j * stride, columns 0, stride, ...)
__global__ __launch_bounds__(256) void k_mvs_fuse_count(const uint8_t *__restrict__ mask, int rows, int cols, int stride, int srows, int scols, int32_t *__restrict__ rowcnt)
{
    __shared__ int sh[4];
    const int view = blockIdx.x / srows, j = blockIdx.x - view * srows;
    const uint8_t *m = mask + ((size_t)view * rows + (size_t)j * stride) * cols;
    int mine = 0;
    for (int c = threadIdx.x; c < scols; c += 256) mine += m[(size_t)c * stride] ? 1 : 0;
    int total;
    wg_scan_incl<int, 256>(mine, sh, total);
    if (threadIdx.x == 0) rowcnt[blockIdx.x] = total;
}

// off[i]: vertices in front of sampled row i; count_out[1]: all of them
__global__ __launch_bounds__(1024) void k_mvs_fuse_scan(const int32_t *__restrict__ rowcnt, long nrows, long long *__restrict__ off, long long *__restrict__ count_out)
{
    const long long total = wg_scan_array<int32_t, long long>(rowcnt, nrows, off, 0ll);
    if (threadIdx.x == 0) { off[nrows] = total; count_out[1] = total; }
}

struct MvFuseArgs {
    const int32_t *views;
    const double *poses, *intr;
    const uint8_t *rgb;                    // [n][rows][cols][3], may be NULL: black
    const float *depth;
    const uint8_t *mask;
    const long long *off;
    MvVertex *out;
    long long *count_out, capacity;
    int32_t rows, cols, S, stride, srows, scols;
};

__global__ __launch_bounds__(256) void k_mvs_fuse_emit(MvFuseArgs a)
{
    __shared__ int sh[4];
    const long nrows = gridDim.x;
    const long long lo = a.off[blockIdx.x], hi = a.off[blockIdx.x + 1];
    if (hi > a.capacity) return;                                   // whole rows only; the offsets ascend, so every later row is refused too
    if (threadIdx.x == 0 && ((long)blockIdx.x + 1 == nrows || a.off[blockIdx.x + 2] > a.capacity)) a.count_out[0] = hi;      // the last row that fits
    if (hi == lo) return;
    const int view = blockIdx.x / a.srows, j = blockIdx.x - view * a.srows, y = j * a.stride;
    const int ref = a.views[(size_t)view * (1 + 2 * a.S)];
    const size_t row = ((size_t)view * a.rows + y) * a.cols;
    double P[12], K[4];
    for (int k = 0; k < 12; ++k) P[k] = a.poses[12 * (size_t)ref + k];
    for (int k = 0; k < 4; ++k) K[k] = a.intr[6 * (size_t)ref + k];
    long long base = lo;
    for (int c0 = 0; c0 < a.scols; c0 += 256) {
        const int c = c0 + threadIdx.x, x = c * a.stride;
        const bool keep = c < a.scols && a.mask[row + x] != 0;
        int total;
        const int r = wg_rank<256>(keep, sh, total);
        if (keep) {
            double Xw[3];
            mg_lift(P, K, x, y, (double)a.depth[row + x], Xw);
            MvVertex v;
            v.x = (float)Xw[0]; v.y = (float)Xw[1]; v.z = (float)Xw[2];
            v.c = make_uchar4(0, 0, 0, 255);
            if (a.rgb) { const uint8_t *p = a.rgb + (((size_t)ref * a.rows + y) * a.cols + x) * 3; v.c = make_uchar4(p[0], p[1], p[2], 255); }
            a.out[base + r] = v;
        }
        base += total;
    }
}

// Views and ranges from a session's graph.  One lane per landmark: every DISTINCT camera of its track (the first occurrence counts,
// k_loc_covisible's rule) counts once against every other distinct camera of the track and once against itself, and folds the
// landmark's camera-frame depth (reproj_l1's l[2]) into its range when positive.  Integer atomics and min / max of the bits of positive
// doubles (which order as the numbers do): exact in any order.  cov is zero, lo +inf's bits and hi zero on entry.
__global__ __launch_bounds__(256) void k_mvs_views_count(int np, int nc, const int *__restrict__ pt_off, const int *__restrict__ ocam, const double *__restrict__ pts,
                                                         const double *__restrict__ poses, int *__restrict__ cov, unsigned long long *__restrict__ lo,
                                                         unsigned long long *__restrict__ hi)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= np) return;
    const int a = pt_off[j], b = pt_off[j + 1];
    const double X[3] = {pts[3 * (size_t)j], pts[3 * (size_t)j + 1], pts[3 * (size_t)j + 2]};
    for (int o = a; o < b; ++o) {
        const int c = ocam[o];
        if (c < 0 || c >= nc) continue;
        bool first = true;
        for (int q = a; q < o; ++q) first = first && ocam[q] != c;
        if (!first) continue;
        const double *P = poses + 12 * (size_t)c;
        const double z = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
        if (z > 0.0 && z < INFINITY) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(z);
            atomicMin(lo + c, bits);
            atomicMax(hi + c, bits);
        }
        for (int q = a; q < b; ++q) {
            const int d = ocam[q];
            if (d < 0 || d >= nc) continue;
            bool firstd = true;
            for (int r = a; r < q; ++r) firstd = firstd && ocam[r] != d;
            if (firstd) atomicAdd(cov + (size_t)c * nc + d, 1);
        }
    }
}

// One lane per camera: its S most covisible cameras (count descending, ties to the lower index, -1 where fewer share a landmark) and
// its range as doubles ((0, 0): it sees no landmark in front of it).
__global__ __launch_bounds__(256) void k_mvs_views_pick(int nc, int S, const int *__restrict__ cov, const unsigned long long *__restrict__ lo,
                                                        const unsigned long long *__restrict__ hi, int32_t *__restrict__ sources, double *__restrict__ range)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const int *row = cov + (size_t)c * nc;
    int last_cnt = INT32_MAX, last_idx = -1;
    for (int s = 0; s < S; ++s) {
        int best = -1, best_cnt = 0;
        for (int d = 0; d < nc; ++d) {
            const int n = row[d];
            if (d == c || n <= 0) continue;
            if (!(n < last_cnt || (n == last_cnt && d > last_idx))) continue;      // taken in an earlier round
            if (n > best_cnt) { best = d; best_cnt = n; }                          // the first of equal counts: the lower index
        }
        sources[(size_t)c * S + s] = best;
        if (best < 0) { for (int r = s + 1; r < S; ++r) sources[(size_t)c * S + r] = -1; break; }
        last_cnt = best_cnt; last_idx = best;
    }
    const bool any = hi[c] != 0ull;
    range[2 * (size_t)c] = any ? __longlong_as_double((long long)lo[c]) : 0.0;
    range[2 * (size_t)c + 1] = any ? __longlong_as_double((long long)hi[c]) : 0.0;
}

int mv_fail(rcn_ctx *ctx, const char *who, const char *what)
{
    ctx->set_error(std::string(who) + ": " + what);
    return RCN_ERR_ARG;
}

int mv_check_opt(rcn_ctx *ctx, const char *who, const rcn_mvs_options &o)
{
    if (o.radius < 1 || o.radius > MG_RMAX) return mv_fail(ctx, who, "radius outside 1 .. 5");
    if (o.min_sources < 1 || o.min_consistent < 0 || o.stride < 1) return mv_fail(ctx, who, "min_sources < 1, min_consistent < 0 or stride < 1");
    if (std::isnan(o.max_cost) || !(o.rel_tol >= 0.0)) return mv_fail(ctx, who, "max_cost is not a number or rel_tol is negative");
    return RCN_OK;
}

// Checks the view table and stages it as [V][1 + 2 S] (reference, sources, the sources' views) behind one asynchronous copy.
int mv_stage_views(rcn_ctx *ctx, const char *who, const int32_t *views_host, int32_t V, int32_t S, int32_t n_images)
{
    if (ctx->mvs_stage_pending) { RCN_HIP(hipEventSynchronize(ctx->mvs_ev)); ctx->mvs_stage_pending = false; }      // the staging buffer is free again
    const size_t w = 1 + 2 * (size_t)S;
    ctx->mvs_stage_host.resize((size_t)V * w);
    std::vector<int32_t> view_of((size_t)n_images, -1);
    for (int32_t v = 0; v < V; ++v) {
        const int32_t ref = views_host[(size_t)v * (1 + S)];
        if (ref < 0 || ref >= n_images) return mv_fail(ctx, who, "a reference image outside 0 .. n_images - 1");
        if (view_of[ref] < 0) view_of[ref] = v;                   // an image swept twice: its first map answers for it
    }
    for (int32_t v = 0; v < V; ++v) {
        int32_t *t = ctx->mvs_stage_host.data() + (size_t)v * w;
        const int32_t *in = views_host + (size_t)v * (1 + S);
        t[0] = in[0];
        for (int32_t s = 0; s < S; ++s) {
            const int32_t src = in[1 + s];
            if (src >= n_images) return mv_fail(ctx, who, "a source image outside the batch");
            if (src == in[0]) return mv_fail(ctx, who, "a reference listed as its own source");
            t[1 + s] = src < 0 ? -1 : src;
            t[1 + S + s] = src < 0 ? -1 : view_of[src];
        }
    }
    if (!ctx->mvs_ev && hipEventCreateWithFlags(&ctx->mvs_ev, hipEventDisableTiming) != hipSuccess) { ctx->mvs_ev = nullptr; RCN_HIP(hipGetLastError()); }
    const size_t bytes = ctx->mvs_stage_host.size() * 4;
    RCN_HIP(ctx->mvs_tab.reserve(bytes));
    RCN_HIP(hipMemcpyAsync(ctx->mvs_tab.p, ctx->mvs_stage_host.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    RCN_HIP(hipEventRecord(ctx->mvs_ev, ctx->stream));
    ctx->mvs_stage_pending = true;
    return RCN_OK;
}

int mv_check_shape(rcn_ctx *ctx, const char *who, int32_t n_images, int32_t rows, int32_t cols, int32_t V, int32_t S)
{
    if (V < 0) return mv_fail(ctx, who, "a negative number of views");
    if (n_images < 1 || rows < 1 || cols < 1) return mv_fail(ctx, who, "a size is not positive");
    if (S < 1 || S > RCN_MVS_MAX_SOURCES) return mv_fail(ctx, who, "S outside 1 .. 16");
    if ((int64_t)rows * cols > INT32_MAX / 4) return mv_fail(ctx, who, "rows * cols > 2^29 - 1");
    if (V > 65535) return mv_fail(ctx, who, "more than 65535 views in one launch");
    return RCN_OK;
}

}  // namespace

void rcn_int_mvs_release(rcn_ctx *ctx)
{
    ctx->mvs_tab.release(); ctx->mvs_ws.release();
    if (ctx->mvs_ev) (void)hipEventDestroy(ctx->mvs_ev);
    ctx->mvs_ev = nullptr;
}

// rcn_ba_session_mvs_views (ba_session.hip holds the session): ctx->mu held, the session's observation arrays current.
int rcn_int_mvs_views(rcn_ctx *ctx, int32_t nc, int32_t np, const int32_t *ocam, const int32_t *pt_off, const double *pts, const double *poses34_host, int32_t S,
                      int32_t *sources_out, double *range_out, int32_t *cov_out)
{
    hipStream_t st = ctx->stream;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_pose = al(96 * (size_t)nc), b_cov = al(4 * (size_t)nc * nc), b_lo = al(8 * (size_t)nc), b_src = al(4 * (size_t)nc * S), b_rng = al(16 * (size_t)nc);
    RCN_HIP(ctx->mvs_ws.reserve(b_pose + b_cov + 2 * b_lo + b_src + b_rng));
    char *base = ctx->mvs_ws.as<char>();
    double *d_pose = (double *)base;
    int *d_cov = (int *)(base + b_pose);
    unsigned long long *d_lo = (unsigned long long *)(base + b_pose + b_cov), *d_hi = (unsigned long long *)(base + b_pose + b_cov + b_lo);
    int32_t *d_src = (int32_t *)(base + b_pose + b_cov + 2 * b_lo);
    double *d_rng = (double *)(base + b_pose + b_cov + 2 * b_lo + b_src);
    RCN_HIP(hipMemcpyAsync(d_pose, poses34_host, 96 * (size_t)nc, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemsetAsync(d_cov, 0, b_cov + 2 * b_lo, st));                                   // counts and hi: zero; lo: the next line
    RCN_HIP(hipMemsetD32Async((hipDeviceptr_t)d_lo, 0x7FF00000u, 2 * (size_t)nc, st));       // every word 0x7FF00000: a NaN's bits above every finite depth's
    if (np > 0) k_mvs_views_count<<<(np + 255) / 256, 256, 0, st>>>(np, nc, pt_off, ocam, pts, d_pose, d_cov, d_lo, d_hi);
    k_mvs_views_pick<<<(nc + 255) / 256, 256, 0, st>>>(nc, S, d_cov, d_lo, d_hi, d_src, d_rng);
    RCN_HIP(hipGetLastError());
    RCN_HIP(hipMemcpyAsync(sources_out, d_src, 4 * (size_t)nc * S, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(range_out, d_rng, 16 * (size_t)nc, hipMemcpyDeviceToHost, st));
    if (cov_out) RCN_HIP(hipMemcpyAsync(cov_out, d_cov, 4 * (size_t)nc * nc, hipMemcpyDeviceToHost, st));
    RCN_HIP(rcn_int_stream_wait(ctx));       // the host arrays are the caller's
    return RCN_OK;
}

extern "C" {

void rcn_mvs_default_options(rcn_mvs_options *o)
{
    if (!o) return;
    o->radius = 3; o->min_sources = 2; o->min_consistent = 2; o->stride = 1;
    o->max_cost = 0.5; o->rel_tol = 0.01;
}

int rcn_mvs_layout(int32_t rows, int32_t cols, int32_t V, int32_t D, int32_t S, int32_t radius, rcn_mvs_sizes *out)
{
    if (!out || rows < 1 || cols < 1 || V < 0 || D < 1 || D > RCN_MVS_MAX_PLANES || S < 1 || S > RCN_MVS_MAX_SOURCES || radius < 1 || radius > MG_RMAX) return RCN_ERR_ARG;
    out->tile = MV_T;
    out->tiles_x = (cols + MV_T - 1) / MV_T;
    out->tiles_y = (rows + MV_T - 1) / MV_T;
    out->lds_bytes = (int32_t)(2 * MV_W * MV_LD * 4 + MV_W * MV_T * (4 + 4 + 8));
    out->pixels = (int64_t)V * rows * cols;
    out->h_doubles = (int64_t)V * S * D * 9;
    out->samples = out->pixels * D * S;
    return RCN_OK;
}

int rcn_mvs_inv_depths(double near_z, double far_z, int32_t D, double *inv_out)
{
    return mg_inv_depths(near_z, far_z, D, RCN_MVS_MAX_PLANES, inv_out) ? RCN_OK : RCN_ERR_ARG;
}

int rcn_mvs_homographies(const double *poses34, const double *intrinsics, int32_t ref, const int32_t *srcs, int32_t S, const double *inv, int32_t D, double *H_out)
{
    return mg_homographies(poses34, intrinsics, ref, srcs, S, inv, D, RCN_MVS_MAX_SOURCES, RCN_MVS_MAX_PLANES, H_out) ? RCN_OK : RCN_ERR_ARG;
}

int rcn_img_undistort_device(rcn_ctx *ctx, const uint8_t *src_dev, int64_t stride_img_bytes, int64_t stride_row_bytes, int32_t channels, int32_t n, int32_t rows,
                             int32_t cols, const double *intrinsics_dev, uint8_t *out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_img_undistort_device";
    if (n < 0) return mv_fail(ctx, who, "n < 0");
    if (channels != 1 && channels != 3) return mv_fail(ctx, who, "channels is neither 1 nor 3");
    if (rows < 1 || cols < 1) return mv_fail(ctx, who, "a size is not positive");
    if ((int64_t)rows * cols * 3 > INT32_MAX) return mv_fail(ctx, who, "rows * cols * 3 > 2^31 - 1");
    if (stride_row_bytes < (int64_t)cols * channels) return mv_fail(ctx, who, "a row stride below cols * channels");
    if (n > 65535) return mv_fail(ctx, who, "more than 65535 images in one launch");
    if (n > 0 && (!src_dev || !intrinsics_dev || !out_dev)) return mv_fail(ctx, who, "null pointer");
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    k_img_undistort<<<dim3((unsigned)(((int64_t)rows * cols + 255) / 256), (unsigned)n), 256, 0, ctx->stream>>>(src_dev, stride_img_bytes, stride_row_bytes, channels, rows, cols,
                                                                                                                 intrinsics_dev, out_dev);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int rcn_mvs_sweep_device(rcn_ctx *ctx, const uint8_t *gray_dev, int64_t stride_img_bytes, int64_t stride_row_bytes, int32_t n_images, int32_t rows, int32_t cols,
                         const int32_t *views_host, int32_t V, int32_t S, const double *H_dev, const double *inv_dev, int32_t D, const rcn_mvs_options *opt,
                         int16_t *plane_out_dev, float *depth_out_dev, float *cost_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_mvs_sweep_device";
    rcn_mvs_options use;
    rcn_mvs_default_options(&use);
    if (opt) use = *opt;
    if (int rc = mv_check_opt(ctx, who, use)) return rc;
    if (int rc = mv_check_shape(ctx, who, n_images, rows, cols, V, S)) return rc;
    if (D < 1 || D > RCN_MVS_MAX_PLANES) return mv_fail(ctx, who, "D outside 1 .. 1024");
    if (stride_row_bytes < cols) return mv_fail(ctx, who, "a row stride below cols");
    const int64_t tiles = (int64_t)((cols + MV_T - 1) / MV_T) * ((rows + MV_T - 1) / MV_T);
    if (tiles > MV_MAX_BLOCKS) return mv_fail(ctx, who, "more than 2^24 - 1 tiles per view");
    if (V > 0 && (!gray_dev || !views_host || !H_dev || !inv_dev || !plane_out_dev || !depth_out_dev || !cost_out_dev)) return mv_fail(ctx, who, "null pointer");
    if (V == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = mv_stage_views(ctx, who, views_host, V, S, n_images)) return rc;
    MvSweepArgs a;
    a.gray = gray_dev; a.si = stride_img_bytes; a.sr = stride_row_bytes;
    a.views = ctx->mvs_tab.as<int32_t>(); a.H = H_dev; a.inv = inv_dev;
    a.plane = plane_out_dev; a.depth = depth_out_dev; a.cost = cost_out_dev;
    a.max_cost = use.max_cost;
    a.rows = rows; a.cols = cols; a.S = S; a.D = D; a.R = use.radius; a.min_sources = use.min_sources; a.tiles_x = (cols + MV_T - 1) / MV_T;
    k_mvs_sweep<<<dim3((unsigned)tiles, (unsigned)V), 256, 0, ctx->stream>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int rcn_mvs_consistency_device(rcn_ctx *ctx, const int32_t *views_host, int32_t V, int32_t S, const double *poses34_dev, const double *intrinsics_dev, int32_t n_images,
                               int32_t rows, int32_t cols, const int16_t *plane_dev, const float *depth_dev, const rcn_mvs_options *opt, uint8_t *mask_out_dev,
                               int32_t *counts_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_mvs_consistency_device";
    rcn_mvs_options use;
    rcn_mvs_default_options(&use);
    if (opt) use = *opt;
    if (int rc = mv_check_opt(ctx, who, use)) return rc;
    if (int rc = mv_check_shape(ctx, who, n_images, rows, cols, V, S)) return rc;
    if (V > 0 && (!views_host || !poses34_dev || !intrinsics_dev || !plane_dev || !depth_dev || !mask_out_dev || !counts_out_dev)) return mv_fail(ctx, who, "null pointer");
    if (V == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = mv_stage_views(ctx, who, views_host, V, S, n_images)) return rc;
    RCN_HIP(hipMemsetAsync(counts_out_dev, 0, 4 * (size_t)V, ctx->stream));
    MvCheckArgs a;
    a.views = ctx->mvs_tab.as<int32_t>(); a.poses = poses34_dev; a.intr = intrinsics_dev; a.plane = plane_dev; a.depth = depth_dev;
    a.mask = mask_out_dev; a.counts = counts_out_dev; a.rel_tol = use.rel_tol; a.rows = rows; a.cols = cols; a.S = S; a.min_consistent = use.min_consistent;
    k_mvs_consistency<<<dim3((unsigned)(((int64_t)rows * cols + 255) / 256), (unsigned)V), 256, 0, ctx->stream>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int rcn_mvs_fuse_device(rcn_ctx *ctx, const int32_t *views_host, int32_t V, int32_t S, const double *poses34_dev, const double *intrinsics_dev, int32_t n_images,
                        const uint8_t *rgb_dev, int32_t rows, int32_t cols, const float *depth_dev, const uint8_t *mask_dev, const rcn_mvs_options *opt, int64_t capacity,
                        void *vertices_out_dev, int64_t *counts_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_mvs_fuse_device";
    rcn_mvs_options use;
    rcn_mvs_default_options(&use);
    if (opt) use = *opt;
    if (int rc = mv_check_opt(ctx, who, use)) return rc;
    if (int rc = mv_check_shape(ctx, who, n_images, rows, cols, V, S)) return rc;
    if (capacity < 0) return mv_fail(ctx, who, "a negative capacity");
    if (!counts_out_dev) return mv_fail(ctx, who, "null pointer");
    if (V > 0 && (!views_host || !poses34_dev || !intrinsics_dev || !depth_dev || !mask_dev || (capacity > 0 && !vertices_out_dev))) return mv_fail(ctx, who, "null pointer");
    const int srows = (rows + use.stride - 1) / use.stride, scols = (cols + use.stride - 1) / use.stride;
    const int64_t nrows = (int64_t)V * srows;
    if (nrows > MV_MAX_BLOCKS) return mv_fail(ctx, who, "more than 2^24 - 1 sampled rows");
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(hipMemsetAsync(counts_out_dev, 0, 16, ctx->stream));
    if (V == 0) return RCN_OK;
    if (int rc = mv_stage_views(ctx, who, views_host, V, S, n_images)) return rc;
    const size_t b_cnt = ((size_t)nrows * 4 + 255) / 256 * 256;
    RCN_HIP(ctx->mvs_ws.reserve(b_cnt + ((size_t)nrows + 2) * 8));
    int32_t *rowcnt = ctx->mvs_ws.as<int32_t>();
    long long *off = reinterpret_cast<long long *>(ctx->mvs_ws.as<char>() + b_cnt);
    long long *cnt = reinterpret_cast<long long *>(counts_out_dev);
    hipStream_t st = ctx->stream;
    k_mvs_fuse_count<<<(unsigned)nrows, 256, 0, st>>>(mask_dev, rows, cols, use.stride, srows, scols, rowcnt);
    k_mvs_fuse_scan<<<1, 1024, 0, st>>>(rowcnt, (long)nrows, off, cnt);
    RCN_HIP(hipGetLastError());
    MvFuseArgs a;
    a.views = ctx->mvs_tab.as<int32_t>(); a.poses = poses34_dev; a.intr = intrinsics_dev; a.rgb = rgb_dev; a.depth = depth_dev; a.mask = mask_dev;
    a.off = off; a.out = reinterpret_cast<MvVertex *>(vertices_out_dev); a.count_out = cnt; a.capacity = capacity;
    a.rows = rows; a.cols = cols; a.S = S; a.stride = use.stride; a.srows = srows; a.scols = scols;
    k_mvs_fuse_emit<<<(unsigned)nrows, 256, 0, st>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

}  // extern "C"
