// triangulate.hip -- batched multi-view triangulation behind rcn_triangulate (include/rcn.h).  gfx950, fp64.
//
// SequentialReconstructor::triangulateMultiView (SequentialReconstructor.cpp:396-489) for a whole batch of tracks in
// one launch: per track (n >= 2 observations, in the caller's order)
//   unproject every observation (Camera.h:79-93), two rows per observation of the DLT system A (2n x 4) against the
//   extrinsics [R | t], X = the right singular vector of A's smallest singular value, hnormalized; accepted only if that
//   singular value is not 0 and the WORLD z of X is > 0 (:432), every observation reprojects within the L1 threshold
//   (:447-451) and EVERY pair of rays subtends at least the minimum angle (:458-478).
//
//   T1 k_cam_centres   -R't of every camera (camgeom.h, shared with validity.hip)                      [trivial]
//   T2 k_triangulate   one thread per track: A streamed row by row into a 4x4 upper-triangular R by Givens
//                      rotations (A = QR: same right singular vectors, A^T A is never formed), cyclic one-sided
//                      Jacobi on R; status, X, accepted tracks per block                               [fp64 latency]
//   T3 k_tri_scan      one workgroup: exclusive scan of the per-block counts (integer sums: exact in any order)
//   T4 k_tri_compact   rank of every accepted track = block offset + wave prefix + lane prefix; X copied to
//                      out_compact[first + rank]                                                      [trivial]
// No atomic decides a position: the compacted order is the track order.
//
// Every operation is a separately rounded IEEE double (contraction off) in the fixed order below; tests/tri_ref.py
// restates that order operation by operation, and X agrees with it bit for bit.  The angle rule goes through acos, whose
// last ulp the device library and a host libm may round differently: a decision can differ only for a track at exactly
// the threshold.
#include "camgeom.h"
#include "wgprim.h"

namespace {

constexpr int TRI_BLOCK = 256;                  // 4 waves
constexpr int TRI_SWEEPS = 20;                  // one-sided Jacobi: at most this many cyclic sweeps
constexpr double TRI_JACOBI_TOL = 1e-15;        // rotate (p, q) while |gamma| > tol * sqrt(alpha * beta)

struct TriArgs {
    const double *poses, *intr, *centres;
    const int32_t *trk_off, *obs_cam, *obs_xy;
    int32_t n_tracks;
    double max_err, min_angle;
    double *xyz;
    uint8_t *status;
    int32_t *blk_cnt;
};

// Camera.h:79-93 and :411-412: the two rows of A of one observation
__device__ __forceinline__ void dlt_rows(const double *P, const double *K, int32_t ox, int32_t oy, double *a, double *b)
{
#pragma clang fp contract(off)
    double x = ((double)ox - K[2]) / K[0];
    double y = ((double)oy - K[3]) / K[1];
    const double radius = x * x + y * y;
    const double distortion = K[4] * radius + (K[5] * radius) * radius;
    x -= distortion;
    y -= distortion;
    for (int c = 0; c < 4; ++c) {
        a[c] = x * P[8 + c] - P[c];
        b[c] = y * P[8 + c] - P[4 + c];
    }
}

// rotate the row a into the upper-triangular R (Givens, column by column; a zero entry needs no rotation)
__device__ __forceinline__ void givens_row(double (&R)[4][4], double *a)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (a[k] != 0.0) {
            const double rho = sqrt(R[k][k] * R[k][k] + a[k] * a[k]);
            const double c = R[k][k] / rho, s = a[k] / rho;
            R[k][k] = rho;
#pragma unroll
            for (int j = k + 1; j < 4; ++j) {
                const double rk = R[k][j];
                R[k][j] = c * rk + s * a[j];
                a[j] = c * a[j] - s * rk;
            }
            a[k] = 0.0;
        }
    }
}

__device__ __forceinline__ double col_dot(const double (&W)[4][4], int p, int q)
{
#pragma clang fp contract(off)
    return ((W[0][p] * W[0][q] + W[1][p] * W[1][q]) + W[2][p] * W[2][q]) + W[3][p] * W[3][q];
}

// cyclic one-sided Jacobi on the columns of W (= R on entry), pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), V
// accumulating the rotations; stops after the first sweep without a rotation.  Returns the smallest column norm and,
// in v, the column of V that belongs to it (the first one on a tie).  Every index is a constant after unrolling: W and
// V stay in registers.
__device__ __forceinline__ double jacobi_min(double (&W)[4][4], double (&V)[4][4], double *v)
{
#pragma clang fp contract(off)
    for (int sweep = 0; sweep < TRI_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double alpha = col_dot(W, p, p), beta = col_dot(W, q, q), gamma = col_dot(W, p, q);
                if (!(fabs(gamma) > TRI_JACOBI_TOL * sqrt(alpha * beta))) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double wp = W[i][p], wq = W[i][q];
                    W[i][p] = c * wp - s * wq;
                    W[i][q] = s * wp + c * wq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
                rotated = true;
            }
        }
        if (!rotated) break;
    }
    double smin = sqrt(col_dot(W, 0, 0));
    v[0] = V[0][0]; v[1] = V[1][0]; v[2] = V[2][0]; v[3] = V[3][0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const double sj = sqrt(col_dot(W, j, j));
        if (sj < smin) { smin = sj; v[0] = V[0][j]; v[1] = V[1][j]; v[2] = V[2][j]; v[3] = V[3][j]; }
    }
    return smin;
}

__global__ __launch_bounds__(TRI_BLOCK) void k_triangulate(TriArgs a)
{
#pragma clang fp contract(off)
    __shared__ int32_t wave_cnt[TRI_BLOCK / 64];
    const int j = blockIdx.x * TRI_BLOCK + threadIdx.x;
    bool acc = false;
    if (j < a.n_tracks) {
        const int o0 = a.trk_off[j], k = a.trk_off[j + 1] - o0;
        double R[4][4] = {};
        for (int o = o0; o < o0 + k; ++o) {               // :405-419, streamed: only R is kept
            const int c = a.obs_cam[o];
            double ra[4], rb[4];
            dlt_rows(a.poses + 12 * (size_t)c, a.intr + 6 * (size_t)c, a.obs_xy[2 * (size_t)o], a.obs_xy[2 * (size_t)o + 1], ra, rb);
            givens_row(R, ra);
            givens_row(R, rb);
        }
        double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
        double v[4];
        const double sigma = jacobi_min(R, V, v);         // :421-422
        const double X[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
        uint8_t st = 0;
        if (k < 2 || !(sigma != 0.0 && X[2] > 0.0)) st = 1;     // :425 (a track of < 2 observations: only through the device entry)
        for (int o = o0; st == 0 && o < o0 + k; ++o) {          // :440-455, track order, no depth test
            const int c = a.obs_cam[o];
            double depth;
            const double resid = reproj_l1(a.poses + 12 * (size_t)c, a.intr + 6 * (size_t)c, X, a.obs_xy[2 * (size_t)o], a.obs_xy[2 * (size_t)o + 1], &depth);
            if (resid > a.max_err) st = 2;
        }
        for (int p = 0; st == 0 && p < k; ++p) {                // :458-478: every pair (the angle is symmetric)
            const double *c1 = a.centres + 3 * (size_t)a.obs_cam[o0 + p];
            for (int q = p + 1; q < k; ++q)
                if (tri_angle(X, c1, a.centres + 3 * (size_t)a.obs_cam[o0 + q]) < a.min_angle) { st = 3; break; }
        }
        a.xyz[3 * (size_t)j] = X[0]; a.xyz[3 * (size_t)j + 1] = X[1]; a.xyz[3 * (size_t)j + 2] = X[2];
        a.status[j] = st;
        acc = st == 0;
    }
    const unsigned long long m = __ballot(acc);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = (int32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t s = 0;
        for (int w = 0; w < TRI_BLOCK / 64; ++w) s += wave_cnt[w];
        a.blk_cnt[blockIdx.x] = s;
    }
}

// exclusive scan of n block counts in one workgroup of 1024 threads: thread t owns a contiguous run of ceil(n / 1024)
__global__ __launch_bounds__(1024) void k_tri_scan(const int32_t *__restrict__ cnt, int n, int32_t *__restrict__ off, int32_t *__restrict__ total)
{
    const int32_t sum = wg_scan_array(cnt, n, off, (int32_t)0);
    if (threadIdx.x == 1023) *total = sum;
}

__global__ __launch_bounds__(TRI_BLOCK) void k_tri_compact(const uint8_t *__restrict__ status, const double *__restrict__ xyz, int n,
                                                        const int32_t *__restrict__ blk_off, double *__restrict__ out, int32_t first)
{
    __shared__ int32_t wave_cnt[TRI_BLOCK / 64];
    const int j = blockIdx.x * TRI_BLOCK + threadIdx.x;
    const bool acc = j < n && status[j] == 0;
    int in_block;
    const int32_t r = blk_off[blockIdx.x] + wg_rank<TRI_BLOCK>(acc, wave_cnt, in_block);
    if (!acc) return;
    const size_t d = 3 * ((size_t)first + (size_t)r);
    out[d] = xyz[3 * (size_t)j]; out[d + 1] = xyz[3 * (size_t)j + 1]; out[d + 2] = xyz[3 * (size_t)j + 2];
}

int validate(rcn_ctx *ctx, const rcn_triangulation_problem *p, const void *xyz, const void *status)
{
    if (!ctx) return RCN_ERR_ARG;
    if (!p || p->n_cams < 0 || p->n_tracks < 0 || p->n_obs < 0 || (p->n_tracks > 0 && (!xyz || !status || !p->trk_off)) ||
        (p->n_obs > 0 && (!p->obs_cam || !p->obs_xy)) || (p->n_cams > 0 && (!p->poses34 || !p->intrinsics))) {
        ctx->set_error("rcn_triangulate: bad argument");
        return RCN_ERR_ARG;
    }
    return RCN_OK;
}

size_t blocks_of(int32_t n_tracks) { return ((size_t)n_tracks + TRI_BLOCK - 1) / TRI_BLOCK; }

}  // namespace

// bytes of device workspace rcn_int_triangulate_launch needs (camera centres, block counts, block offsets)
size_t rcn_int_triangulate_ws_bytes(int32_t n_cams, int32_t n_tracks)
{
    return (24 * (size_t)n_cams + 255) / 256 * 256 + 2 * ((4 * blocks_of(n_tracks) + 255) / 256 * 256) + 256;
}

int rcn_int_triangulate_launch(rcn_ctx *ctx, const rcn_triangulation_problem *dp, double max_err, double min_angle, void *ws,
                               double *xyz, uint8_t *status, double *compact, int32_t compact_first, int32_t *n_accepted)
{
    hipStream_t st = ctx->stream;
    const size_t nb = blocks_of(dp->n_tracks);
    char *w = static_cast<char *>(ws);
    double *centres = reinterpret_cast<double *>(w);
    int32_t *blk_cnt = reinterpret_cast<int32_t *>(w + (24 * (size_t)dp->n_cams + 255) / 256 * 256);
    int32_t *blk_off = blk_cnt + (4 * nb + 255) / 256 * 64;
    if (dp->n_tracks == 0) {
        if (n_accepted) RCN_HIP(hipMemsetAsync(n_accepted, 0, sizeof(int32_t), st));
        return RCN_OK;
    }
    if (dp->n_cams > 0) k_cam_centres<<<(dp->n_cams + 127) / 128, 128, 0, st>>>(dp->poses34, dp->n_cams, centres);
    TriArgs a;
    a.poses = dp->poses34; a.intr = dp->intrinsics; a.centres = centres;
    a.trk_off = dp->trk_off; a.obs_cam = dp->obs_cam; a.obs_xy = dp->obs_xy; a.n_tracks = dp->n_tracks;
    a.max_err = max_err; a.min_angle = min_angle; a.xyz = xyz; a.status = status; a.blk_cnt = blk_cnt;
    k_triangulate<<<(unsigned)nb, TRI_BLOCK, 0, st>>>(a);
    if (compact || n_accepted) {
        k_tri_scan<<<1, 1024, 0, st>>>(blk_cnt, (int)nb, blk_off, n_accepted);
        if (compact) k_tri_compact<<<(unsigned)nb, TRI_BLOCK, 0, st>>>(status, xyz, dp->n_tracks, blk_off, compact, compact_first);
    }
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

// Structure check on the host: offsets non-decreasing inside n_obs, at least two observations per track (the reference
// reads singularValues()(3): a 2 x 4 system has no fourth singular value), camera indices in range.
int rcn_int_triangulate_check(rcn_ctx *ctx, int32_t n_cams, int32_t n_tracks, int32_t n_obs, const int32_t *trk_off, const int32_t *obs_cam)
{
    if (n_tracks > 0) {
        if (trk_off[0] < 0) { ctx->set_error("rcn_triangulate: trk_off[0] < 0"); return RCN_ERR_ARG; }
        for (int j = 0; j < n_tracks; ++j) {
            if (trk_off[j + 1] < trk_off[j]) { ctx->set_error("rcn_triangulate: trk_off must be non-decreasing"); return RCN_ERR_ARG; }
            if (trk_off[j + 1] - trk_off[j] < 2) { ctx->set_error("rcn_triangulate: a track needs at least 2 observations"); return RCN_ERR_ARG; }
        }
        if (trk_off[n_tracks] > n_obs) { ctx->set_error("rcn_triangulate: trk_off exceeds n_obs"); return RCN_ERR_ARG; }
        for (int o = trk_off[0]; o < trk_off[n_tracks]; ++o)
            if (obs_cam[o] < 0 || obs_cam[o] >= n_cams) { ctx->set_error("rcn_triangulate: obs_cam out of range"); return RCN_ERR_ARG; }
    }
    return RCN_OK;
}

extern "C" int rcn_triangulate(rcn_ctx *ctx, const rcn_triangulation_problem *p, double max_projection_error,
                               double min_triangulation_angle, double *out_xyz, uint8_t *out_status, int32_t *out_n_accepted)
{
    int rc = validate(ctx, p, out_xyz, out_status);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rc = rcn_int_triangulate_check(ctx, p->n_cams, p->n_tracks, p->n_obs, p->trk_off, p->obs_cam);
    if (rc) return rc;
    if (p->n_tracks == 0) { if (out_n_accepted) *out_n_accepted = 0; return RCN_OK; }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nc = p->n_cams, nt = p->n_tracks, no = p->n_obs;
    const size_t b_pose = 96 * nc, b_intr = 48 * nc, b_off = 4 * (nt + 1), b_cam = 4 * no, b_xy = 8 * no, b_xyz = 24 * nt, b_st = nt;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_ws = rcn_int_triangulate_ws_bytes(p->n_cams, p->n_tracks);
    const size_t total = al(b_pose) + al(b_intr) + al(b_off) + al(b_cam) + al(b_xy) + al(b_xyz) + al(b_st) + al(b_ws) + 256;
    RCN_HIP(ctx->tri_ws.reserve(total));
    char *base = ctx->tri_ws.as<char>();
    size_t off = 0;
    auto take = [&](size_t b) { char *q = base + off; off += al(b); return q; };
    double *d_pose = (double *)take(b_pose), *d_intr = (double *)take(b_intr);
    int32_t *d_off = (int32_t *)take(b_off), *d_cam = (int32_t *)take(b_cam), *d_xy = (int32_t *)take(b_xy);
    double *d_xyz = (double *)take(b_xyz);
    uint8_t *d_st = (uint8_t *)take(b_st);
    void *d_ws = take(b_ws);
    int32_t *d_cnt = (int32_t *)take(4);
    auto H2D = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    RCN_HIP(H2D(d_pose, p->poses34, b_pose)); RCN_HIP(H2D(d_intr, p->intrinsics, b_intr)); RCN_HIP(H2D(d_off, p->trk_off, b_off));
    RCN_HIP(H2D(d_cam, p->obs_cam, b_cam)); RCN_HIP(H2D(d_xy, p->obs_xy, b_xy));
    rcn_triangulation_problem dp = *p;
    dp.poses34 = d_pose; dp.intrinsics = d_intr; dp.trk_off = d_off; dp.obs_cam = d_cam; dp.obs_xy = d_xy;
    rc = rcn_int_triangulate_launch(ctx, &dp, max_projection_error, min_triangulation_angle, d_ws, d_xyz, d_st, nullptr, 0,
                                    out_n_accepted ? d_cnt : nullptr);
    if (rc) return rc;
    int32_t cnt = 0;
    RCN_HIP(hipMemcpyAsync(out_xyz, d_xyz, b_xyz, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(out_status, d_st, b_st, hipMemcpyDeviceToHost, st));
    if (out_n_accepted) RCN_HIP(hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipStreamSynchronize(st));
    if (out_n_accepted) *out_n_accepted = cnt;
    return RCN_OK;
}

extern "C" int rcn_triangulate_device(rcn_ctx *ctx, const rcn_triangulation_problem *p_dev, double max_projection_error,
                                      double min_triangulation_angle, double *out_xyz_dev, uint8_t *out_status_dev,
                                      double *out_compact_dev, int32_t compact_first, int32_t *out_n_accepted_dev)
{
    int rc = validate(ctx, p_dev, out_xyz_dev, out_status_dev);
    if (rc) return rc;
    if (!out_n_accepted_dev || compact_first < 0) { ctx->set_error("rcn_triangulate_device: out_n_accepted_dev is required, compact_first >= 0"); return RCN_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(ctx->tri_dws.reserve(rcn_int_triangulate_ws_bytes(p_dev->n_cams, p_dev->n_tracks)));
    return rcn_int_triangulate_launch(ctx, p_dev, max_projection_error, min_triangulation_angle, ctx->tri_dws.p, out_xyz_dev,
                                      out_status_dev, out_compact_dev, compact_first, out_n_accepted_dev);
}
