// ba.hip -- bundle adjustment on MI355X (gfx950): kernels + C ABI (rcn_ba_solve).
//
// Replaces, behind include/rcn.h, what BundleAdjuster::adjust hands to Ceres
// (BundleAdjuster.cpp:72-146): Levenberg-Marquardt over camera poses, intrinsics and 3-d
// points with the reprojection residual of BundleAdjuster.h:27-58, point Schur complement
// and a dense Cholesky of the reduced camera system (DENSE_SCHUR, :132).  FP64 throughout.
//
// Kernels:
//   K4 k_ba_eval          residual (+ analytic 2x(10+3) tangent Jacobian) per observation   [HBM]
//      (with a robust loss, rcn_ba_solve_robust: its ROBUST form scales the observation's row by sqrt(rho'), k_ba_dirgrad's takes
//       rho' into the line search, k_ba_loss_report is the pass behind the solve; ba_loss.h)
//   K5 k_ba_point_raw / k_ba_cam_raw   J'J blocks and J'r per point / per camera             [HBM]
//      k_ba_point_solve   V = Vs + D^2/radius, V^-1, per point                               [HBM]
//   K6 k_ba_wy + k_ba_schur_mfma[_wg] + k_ba_schur_diag_mfma   point Schur complement as f64-MFMA
//      gathers over per-block observation-pair lists built once per solve (k_pair_*), written
//      straight into the dense reduced system; bit-reproducible                      [L2 gathers / f64 MFMA]
//      (k_ba_schur + k_ba_S_assemble + k_ba_cam_rhs: the atomic form, RCN_BA_SCHUR_ATOMICS=1)
//   K7 the dense Cholesky of the reduced system and the triangular solves behind it: chol.hip, reached through chol.h only
//   K8 k_ba_backsub, k_ba_model, k_ba_plus, reductions                                       [HBM]
// The LM control flow on the host follows Ceres' TrustRegionMinimizer / LevenbergMarquardt
// strategy step by step (same order of tests as the CPU restatement used for parity).
#include "rcn_internal.h"
#include "wgprim.h"
#include <utility>
#include "ba_linesearch.h"
#include "ba_loss.h"
#include "ba_tied.h"

#include <cfloat>
#include <chrono>
#include <cmath>

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// Observation rows.  Everything the solver keeps per observation -- 2x10 tangent camera Jacobian, 2x3 point Jacobian,
// residual -- is ONE 224-byte row, so that the per-camera gathers (k_ba_cam_raw) fetch whole rows, while the kernels
// that stream over all observations (k_ba_eval<true> writes the rows, k_ba_model reads them) move a wave's 64 rows as
// one contiguous 14-KiB block with 16-byte accesses and transpose through LDS: a lane-per-observation access to the
// rows themselves puts 64 lanes on 64 different lines per instruction (measured at 0.7 TB/s in round 2).
#define JROW 28          // doubles per row: [0..19] Jc (2 x 10), [20..25] Jp (2 x 3), [26..27] r
#define JCH (JROW / 2)   // 16-byte chunks per row
#define JLD 30           // LDS row stride in doubles: 240 B keeps rows 16-B aligned and ds_*_b128 by row conflict-free
#define WROW 30          // doubles per row of a W / Y plane
#define WCH (WROW / 2)

struct BaDev {
    int nc, np, no, n, npad, mode, use_wy;   // use_wy: unused (the per-observation W / Y table is always built)
    double ub;
    double *poses, *intr, *pts;        // current point
    double *poses2, *intr2, *pts2;     // candidate
    const double *uv;
    const int *ocam, *opt, *pt_off, *cam_obs_off, *cam_obs, *cam_off, *cam_dim, *cols;
    double *J;                         // per observation ONE row of JROW doubles: camera Jacobian 2x10 | point Jacobian 2x3 | residual 2
    double *Uraw, *gcraw, *Vraw, *gpraw; // unscaled J'J / J'r blocks
    double *sc, *sp, *dgc, *dgp;       // Jacobi scale, clamped diag(Js'Js)
    double *Vinv, *gps, *rhs, *S, *L, *Linv, *yc, *stc, *stp, *dlc, *dlp;   // S: reduced system, L: its sub-diagonal Cholesky tiles
    double *partial, *scal;            // reduction scratch, scalars
    double *csplit;                    // [n_cams][split][256] partial per-camera sums when a camera is split over workgroups
    double *WY;                        // two planes of [n_obs][3][10], camera index fastest: scaled W_o = Jc'Jp at WY, Y_o = W_o Vinv at WY + 30 n_obs
    double *tobs;                      // per observation W_o' y_c (3): the back-substitution's per-observation term
    double *crot;                      // per camera CROT doubles: the camera part of the rotation and its derivative (k_ba_cam_rot)
    unsigned *tickets;                 // 2 nc words, zero at rest: the workgroups a camera is split over finish their sums themselves (cam / Schur-diagonal kernels)
    double *crot2;                     // the same for the candidate poses (poses2), written by k_ba_plus; swapped with crot when the step is accepted
    int *flag;
};

// ---------------------------------------------------------------------------------------
// p = R(w) X as ceres::AngleAxisRotatePoint; R and d(RX)/dw = -R [X]x Jr(w)
__device__ __forceinline__ void rotate(const double *w, const double *X, double *p, double *R, double *dpdw, bool jac)
{
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (th2 > DBL_EPSILON) {
        const double th = sqrt(th2), c = cos(th), s = sin(th);
        const double n[3] = {w[0] / th, w[1] / th, w[2] / th};
        const double cr[3] = {n[1] * X[2] - n[2] * X[1], n[2] * X[0] - n[0] * X[2], n[0] * X[1] - n[1] * X[0]};
        const double tmp = (n[0] * X[0] + n[1] * X[1] + n[2] * X[2]) * (1.0 - c);
        for (int i = 0; i < 3; ++i) p[i] = X[i] * c + cr[i] * s + n[i] * tmp;
        if (!jac) return;
        const double hs = sin(0.5 * th), omc = 2.0 * hs * hs;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = omc * n[i] * n[j] + (i == j ? c : 0.0);
        R[1] -= s * n[2]; R[2] += s * n[1];
        R[3] += s * n[2]; R[5] -= s * n[0];
        R[6] -= s * n[1]; R[7] += s * n[0];
        double a, b;
        if (th < 1e-2) {
            a = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
            b = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0;
        } else {
            a = omc / th2;
            b = (th - s) / (th2 * th);
        }
        const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        double Jr[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                Jr[3 * i + j] = -a * K[3 * i + j] + b * (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j]) + (i == j ? 1.0 : 0.0);
        const double Xx[9] = {0, -X[2], X[1], X[2], 0, -X[0], -X[1], X[0], 0};
        double M[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                M[3 * i + j] = -(R[3 * i] * Xx[j] + R[3 * i + 1] * Xx[3 + j] + R[3 * i + 2] * Xx[6 + j]);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                dpdw[3 * i + j] = M[3 * i] * Jr[j] + M[3 * i + 1] * Jr[3 + j] + M[3 * i + 2] * Jr[6 + j];
    } else {
        p[0] = X[0] + w[1] * X[2] - w[2] * X[1];
        p[1] = X[1] + w[2] * X[0] - w[0] * X[2];
        p[2] = X[2] + w[0] * X[1] - w[1] * X[0];
        if (!jac) return;
        R[0] = 1; R[1] = -w[2]; R[2] = w[1]; R[3] = w[2]; R[4] = 1; R[5] = -w[0]; R[6] = -w[1]; R[7] = w[0]; R[8] = 1;
        dpdw[0] = 0; dpdw[1] = X[2]; dpdw[2] = -X[1]; dpdw[3] = -X[2]; dpdw[4] = 0; dpdw[5] = X[0];
        dpdw[6] = X[1]; dpdw[7] = -X[0]; dpdw[8] = 0;
    }
}

// The part of rotate() that depends on the camera alone -- R(w), Jr(w), cos, sin, the axis: trigonometry, a square root
// and divisions -- tabulated once per camera and evaluation (k_ba_cam_rot), so that the per-observation kernel is left
// with products: CROT doubles per camera, [0..8] R, [9..17] Jr, [18] cos, [19] sin, [20..22] axis, [23] 1 = small angle
// (first-order branch of ceres::AngleAxisRotatePoint), [24..26] w.
#define CROT 28
__device__ __noinline__ void cam_rot_entry(const double *w, double *o);
__global__ void k_ba_cam_rot(const double *__restrict__ poses, int nc, double *__restrict__ tab)
{
    const int cidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (cidx >= nc) return;
    cam_rot_entry(poses + 6 * (size_t)cidx, tab + CROT * (size_t)cidx);
}
// (one camera's entry: also called by k_ba_plus for the pose it has just written -- the table of a candidate that is accepted is then
//  already there when the evaluation with the Jacobian is queued: one launch less per iteration.  NOT inlined: both callers run the
//  same instructions, so a table does not depend on who wrote it -- inlined into k_ba_plus the compiler contracted other products
//  into FMAs than in k_ba_cam_rot, and long far-off solves took other paths than before)
__device__ __noinline__ void cam_rot_entry(const double *w, double *o)
{
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double R[9], Jr[9], c = 1.0, s = 0.0, n[3] = {0.0, 0.0, 0.0};
    const bool big = th2 > DBL_EPSILON;
    if (big) {
        const double th = sqrt(th2);
        c = cos(th); s = sin(th);
        n[0] = w[0] / th; n[1] = w[1] / th; n[2] = w[2] / th;
        const double hs = sin(0.5 * th), omc = 2.0 * hs * hs;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = omc * n[i] * n[j] + (i == j ? c : 0.0);
        R[1] -= s * n[2]; R[2] += s * n[1];
        R[3] += s * n[2]; R[5] -= s * n[0];
        R[6] -= s * n[1]; R[7] += s * n[0];
        double a, b;
        if (th < 1e-2) {
            a = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
            b = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0;
        } else {
            a = omc / th2;
            b = (th - s) / (th2 * th);
        }
        const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                Jr[3 * i + j] = -a * K[3 * i + j] + b * (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j]) + (i == j ? 1.0 : 0.0);
    } else {
        R[0] = 1; R[1] = -w[2]; R[2] = w[1]; R[3] = w[2]; R[4] = 1; R[5] = -w[0]; R[6] = -w[1]; R[7] = w[0]; R[8] = 1;
        for (int i = 0; i < 9; ++i) Jr[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    for (int i = 0; i < 9; ++i) { o[i] = R[i]; o[9 + i] = Jr[i]; }
    o[18] = c; o[19] = s; o[20] = n[0]; o[21] = n[1]; o[22] = n[2]; o[23] = big ? 0.0 : 1.0;
    o[24] = w[0]; o[25] = w[1]; o[26] = w[2]; o[27] = 0.0;
}

// rotate() with the camera part read from the table: the same expressions in the same order
__device__ __forceinline__ void rotate_tab(const double *__restrict__ cr, const double *X, double *p, double *R, double *dpdw)
{
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = cr[i];
    if (cr[23] == 0.0) {
        const double c = cr[18], s = cr[19];
        const double n[3] = {cr[20], cr[21], cr[22]};
        const double cx[3] = {n[1] * X[2] - n[2] * X[1], n[2] * X[0] - n[0] * X[2], n[0] * X[1] - n[1] * X[0]};
        const double tmp = (n[0] * X[0] + n[1] * X[1] + n[2] * X[2]) * (1.0 - c);
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = X[i] * c + cx[i] * s + n[i] * tmp;
        const double Xx[9] = {0, -X[2], X[1], X[2], 0, -X[0], -X[1], X[0], 0};
        double M[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                M[3 * i + j] = -(R[3 * i] * Xx[j] + R[3 * i + 1] * Xx[3 + j] + R[3 * i + 2] * Xx[6 + j]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                dpdw[3 * i + j] = M[3 * i] * cr[9 + j] + M[3 * i + 1] * cr[12 + j] + M[3 * i + 2] * cr[15 + j];
    } else {
        const double w[3] = {cr[24], cr[25], cr[26]};
        p[0] = X[0] + w[1] * X[2] - w[2] * X[1];
        p[1] = X[1] + w[2] * X[0] - w[0] * X[2];
        p[2] = X[2] + w[0] * X[1] - w[1] * X[0];
        dpdw[0] = 0; dpdw[1] = X[2]; dpdw[2] = -X[1]; dpdw[3] = -X[2]; dpdw[4] = 0; dpdw[5] = X[0];
        dpdw[6] = X[1]; dpdw[7] = -X[0]; dpdw[8] = 0;
    }
}

__device__ __forceinline__ double block_sum(double v, double *sh)
{
    const int t = threadIdx.x;
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
    if ((t & 63) == 0) sh[t >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (t == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[i];
    __syncthreads();
    return s;  // valid on thread 0
}

// The sums of a launch, finished BY the launch (round 4; a one-block k_finish_sum launch behind every reduction before: four launches
// of the ~35 of an LM iteration).  Every workgroup delivers its partial sums and takes a ticket; the one that draws the last
// ticket adds the partials up -- in index order, so the result does not depend on who that is -- and writes the scalars.
// The hand-off needs no L2-wide fence: a partial is an agent-coherent (sc1) store, drained (vmcnt(0)) before the ticket is
// taken, and the summing workgroup reads with agent-coherent loads (MI355X_MICROARCH.md, inter-workgroup visibility,
// valid forms).  The ticket word is left at zero for the next launch.
struct Fin {
    double *out;            // NS results (scaled), consecutive
    double *out2;           // optional second home of results 2 and 3 (k_ba_plus: gradient . delta, non-finite count)
    unsigned *ticket;
    const int *flag;        // optional: the factorisation's flag word rides home with the scalars of the step
    double *flag_out;
    double *zero;           // optional: a cell to clear (where the next gradient maximum is collected)
    double scale;
    // optional (round 5): the step's scalars straight into the host's pinned mirror -- scal[0 .. 14) as they stand when this, the
    // step's last reduction, is done, then the sequence number the host spins on.  A copy command plus a stream synchronisation took
    // ~27 us of a small problem's ~110-us iteration; a store over the fabric and a poll take a few.
    double *host;
    const double *scal;
    unsigned long long seq;
};
template <int NS>
__device__ __forceinline__ void finish_sums(const double (&mine)[NS], double *partial, int stride, const Fin &f, double *sh)
{
    __shared__ int s_last;
    const int t = threadIdx.x, nb = (int)gridDim.x;
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q)
            __hip_atomic_store(partial + (size_t)q * stride + blockIdx.x, mine[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned k = __hip_atomic_fetch_add(f.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = k == (unsigned)nb - 1u;
    }
    __syncthreads();
    if (!s_last) return;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        double v = 0.0;
        for (int i = t; i < nb; i += (int)blockDim.x) v += __hip_atomic_load(partial + (size_t)q * stride + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double s = block_sum(v, sh);
        if (t == 0) { f.out[q] = f.scale * s; if (f.out2 && q >= 2) f.out2[q - 2] = f.scale * s; }
    }
    if (t == 0) {
        __hip_atomic_store(f.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (f.flag) *f.flag_out = (double)__hip_atomic_load(f.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (f.zero) *f.zero = 0.0;
        if (f.host) {
            // (the other cells were written by earlier kernels of the stream, and by this thread just above)
            for (int i = 0; i < 14; ++i) __hip_atomic_store(f.host + i, f.scal[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(f.host + 15), f.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// residual of one observation and (JAC) its 2 x 15 Jacobian over [pose 6 | intrinsics 6 | point 3]
template <bool JAC>
__device__ __forceinline__ void obs_residual(const double *ps, const double *in, const double *X, const double *uv,
                                             double &r0, double &r1, double (*J)[15], const double *crot = nullptr)
{
    double p[3], R[9], dpdw[9];
    if (JAC && crot) rotate_tab(crot, X, p, R, dpdw);
    else rotate(ps, X, p, R, dpdw, JAC);
    p[0] += ps[3]; p[1] += ps[4]; p[2] += ps[5];
    const double iz = 1.0 / p[2];
    const double x = p[0] * iz, y = p[1] * iz;
    const double rr = x * x + y * y;
    const double dist = in[4] * rr + in[5] * rr * rr;
    const double xd = x + dist, yd = y + dist;
    r0 = in[0] * xd + in[2] - uv[0];
    r1 = in[1] * yd + in[3] - uv[1];
    if (JAC) {
        const double g = in[4] + 2.0 * in[5] * rr;
        const double a00 = 1.0 + 2.0 * g * x, a01 = 2.0 * g * y, a10 = 2.0 * g * x, a11 = 1.0 + 2.0 * g * y;
        const double b02 = -x * iz, b12 = -y * iz;
        double q[6];
        q[0] = in[0] * (a00 * iz); q[1] = in[0] * (a01 * iz); q[2] = in[0] * (a00 * b02 + a01 * b12);
        q[3] = in[1] * (a10 * iz); q[4] = in[1] * (a11 * iz); q[5] = in[1] * (a10 * b02 + a11 * b12);
        for (int i = 0; i < 2; ++i) {
            const double *qi = q + 3 * i;
            for (int k = 0; k < 3; ++k) {
                J[i][k] = qi[0] * dpdw[k] + qi[1] * dpdw[3 + k] + qi[2] * dpdw[6 + k];
                J[i][3 + k] = qi[k];
                J[i][12 + k] = qi[0] * R[k] + qi[1] * R[3 + k] + qi[2] * R[6 + k];
            }
        }
        J[0][6] = xd; J[0][7] = 0; J[0][8] = 1; J[0][9] = 0; J[0][10] = in[0] * rr; J[0][11] = in[0] * rr * rr;
        J[1][6] = 0; J[1][7] = yd; J[1][8] = 0; J[1][9] = 1; J[1][10] = in[1] * rr; J[1][11] = in[1] * rr * rr;
    }
}

// A wave's rows [row0, row0 + nrows) of a dense [rows][CH * 2] double array <-> its LDS block (row stride JLD), moved
// as 16-byte chunks in memory order: each instruction touches 1 KiB of consecutive addresses.
template <int CH>
__device__ __forceinline__ void rows_to_lds(const double *__restrict__ src, size_t row0, int nrows, double *__restrict__ lds, int lane)
{
    const f64x2 *g = reinterpret_cast<const f64x2 *>(src + row0 * (2 * CH));
    f64x2 v[CH];
#pragma unroll
    for (int it = 0; it < CH; ++it) {
        const int c = it * 64 + lane;
        v[it] = c < nrows * CH ? g[c] : (f64x2){0.0, 0.0};
    }
#pragma unroll
    for (int it = 0; it < CH; ++it) {
        const int c = it * 64 + lane, row = c / CH, part = c - row * CH;
        if (c < nrows * CH) *reinterpret_cast<f64x2 *>(lds + row * JLD + 2 * part) = v[it];
    }
}
template <int CH>
__device__ __forceinline__ void lds_to_rows(double *__restrict__ dst, size_t row0, int nrows, const double *__restrict__ lds, int lane)
{
    f64x2 *g = reinterpret_cast<f64x2 *>(dst + row0 * (2 * CH));
#pragma unroll
    for (int it = 0; it < CH; ++it) {
        const int c = it * 64 + lane, row = c / CH, part = c - row * CH;
        if (c < nrows * CH) g[c] = *reinterpret_cast<const f64x2 *>(lds + row * JLD + 2 * part);
    }
}

// K4: residual and tangent Jacobian per observation; per-block partial of sum r^2.  JAC: every lane builds its row in
// LDS, the wave stores its 64 rows as one contiguous block (HBM-bound: 224 B written per observation).
// ROBUST (a loss, section 7.4; `ls` is read by that form alone): the per-observation term of the sum is rho(s), and the 28 entries of
// the row are multiplied by sqrt(rho'(s)) AFTER they were built -- obs_residual and the column selection are the same expressions under
// every loss, so a weight of exactly 1 leaves exactly the bits of the plain form.  The kind is uniform over the launch: a scalar branch.
// Without a loss the solve launches ROBUST = false, which holds no loss code.
struct BaLoss { int kind; double a, b; };
template <bool JAC, bool ROBUST = false>
__global__ __launch_bounds__(JAC ? 128 : 256) void k_ba_eval(BaDev d, const double *poses, const double *intr,
                                                              const double *pts, double *partial, Fin fin, BaLoss ls)
{
    constexpr int NW = JAC ? 2 : 4;          // JAC: 30 KB of LDS per workgroup, five workgroups per CU
    __shared__ double sh[4];
    __shared__ __attribute__((aligned(16))) double stage[JAC ? NW * 64 * JLD : 2];
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double c2 = 0.0;
    if (o < d.no) {
        const int c = d.ocam[o], j = d.opt[o];
        double ps[6], in[6], X[3];
        for (int i = 0; i < 6; ++i) { ps[i] = poses[6 * c + i]; in[i] = intr[6 * c + i]; }
        for (int i = 0; i < 3; ++i) X[i] = pts[3 * j + i];
        double r0, r1, J[2][15];
        obs_residual<JAC>(ps, in, X, d.uv + 2 * (size_t)o, r0, r1, J, JAC ? d.crot + CROT * (size_t)c : nullptr);
        c2 = r0 * r0 + r1 * r1;
        double wt = 1.0;
        if (ROBUST) { wt = ba_loss_weight(ls.kind, ls.a, ls.b, c2); c2 = ba_loss_rho(ls.kind, ls.a, ls.b, c2); }
        if (JAC) {
            // tangent columns of this camera, WITHOUT indexing J by a run-time column (that would put J in scratch
            // memory): the host lays them out as the first `npose` pose columns (0, 3 or 6: camera 0 / camera 1 / the
            // others, BundleAdjuster.cpp:100-105) followed, in intrinsics mode 1, by fx fy k1 k2 = columns 6 7 10 11
            // (a camera whose group's intrinsics are held, ba_tied.h, has pose columns only in mode 1 too: 6, 3 or 0 columns where a
            //  camera with intrinsics columns has 10, 7 or 4 -- the two sets are apart, so the count says which)
            const int dc = d.cam_dim[c], nin = (d.mode == 1 && dc % 3 == 1) ? 4 : 0, npose = dc - nin;
            double row[JROW];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const double I4[4] = {nin ? J[i][6] : 0.0, nin ? J[i][7] : 0.0, nin ? J[i][10] : 0.0, nin ? J[i][11] : 0.0};
#pragma unroll
                for (int k = 0; k < 10; ++k) {
                    const double a6 = k < 6 ? J[i][k] : I4[k - 6 < 4 ? k - 6 : 3];                    // npose == 6
                    const double a3 = k < 3 ? J[i][k] : (k - 3 < 4 ? I4[k - 3 < 4 ? k - 3 : 3] : 0.0);   // npose == 3
                    const double a0 = k < 4 ? I4[k < 4 ? k : 3] : 0.0;                                  // npose == 0
                    row[10 * i + k] = k < dc ? (npose == 6 ? a6 : npose == 3 ? a3 : a0) : 0.0;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) row[20 + 3 * i + k] = J[i][12 + k];
            }
            row[26] = r0; row[27] = r1;
            if (ROBUST) {
#pragma unroll
                for (int k = 0; k < JROW; ++k) row[k] *= wt;
            }
            f64x2 *my = reinterpret_cast<f64x2 *>(stage + (w * 64 + lane) * JLD);
#pragma unroll
            for (int k = 0; k < JCH; ++k) my[k] = (f64x2){row[2 * k], row[2 * k + 1]};
        }
    }
    if (JAC) {
        __syncthreads();
        const size_t row0 = (size_t)blockIdx.x * blockDim.x + 64 * w;
        const int nrows = (int)min((long long)64, (long long)d.no - (long long)row0);
        if (nrows > 0) lds_to_rows<JCH>(d.J, row0, nrows, stage + w * 64 * JLD, lane);
    }
    const double mine[1] = {block_sum(c2, sh)};
    finish_sums<1>(mine, partial, 0, fin, sh);
}

// Line search (bounds present): directional derivative of the cost at a trial point along the step held in
// d.dlc / d.dlp,  sum_o r_o' (Jc_o dlc + Jp_o dlp)  -- the tangent-space gradient J'r against the direction
// (LineSearchFunction::Evaluate); nothing is stored, the Jacobian of an observation lives in registers.
// With a loss (ROBUST) the observation's term is rho'(s) r_o' (J_o d): rho', not its square root -- the derivative of 1/2 rho(s).
template <bool ROBUST>
__global__ __launch_bounds__(256) void k_ba_dirgrad(BaDev d, const double *poses, const double *intr,
                                                     const double *pts, double *partial, BaLoss ls)
{
    __shared__ double sh[4];
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    double acc = 0.0;
    if (o < d.no) {
        const int c = d.ocam[o], j = d.opt[o];
        double ps[6], in[6], X[3];
        for (int i = 0; i < 6; ++i) { ps[i] = poses[6 * c + i]; in[i] = intr[6 * c + i]; }
        for (int i = 0; i < 3; ++i) X[i] = pts[3 * j + i];
        double r[2], J[2][15];
        obs_residual<true>(ps, in, X, d.uv + 2 * (size_t)o, r[0], r[1], J);
        const int dc = d.cam_dim[c], off = d.cam_off[c];
        for (int i = 0; i < 2; ++i) {
            double m = 0.0;
            for (int k = 0; k < 10; ++k) if (k < dc) m += J[i][d.cols[10 * c + k]] * d.dlc[off + k];
            for (int k = 0; k < 3; ++k) m += J[i][12 + k] * d.dlp[3 * (size_t)j + k];
            acc += r[i] * m;
        }
        if (ROBUST) acc *= ba_loss_drho(ls.kind, ls.a, ls.b, r[0] * r[0] + r[1] * r[1]);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// The loss's report at one point (rcn_ba_loss_report): per observation rho'(s) into `weights` (optional), and over all observations
// the count of s > b and sum s (finish_sums, index order) and max s (one integer atomicMax per workgroup, as k_ba_absmax: *maxout
// zeroed by the caller).  s is the unweighted residual's, the expression of the evaluation kernels.
__global__ __launch_bounds__(256) void k_ba_loss_report(BaDev d, const double *poses, const double *intr, const double *pts,
                                                         BaLoss ls, double *weights, double *partial, Fin fin, double *maxout)
{
    __shared__ double sh[4];
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    double cnt = 0.0, ss = 0.0, m = 0.0;
    if (o < d.no) {
        const int c = d.ocam[o], j = d.opt[o];
        double ps[6], in[6], X[3];
        for (int i = 0; i < 6; ++i) { ps[i] = poses[6 * c + i]; in[i] = intr[6 * c + i]; }
        for (int i = 0; i < 3; ++i) X[i] = pts[3 * j + i];
        double r0, r1;
        obs_residual<false>(ps, in, X, d.uv + 2 * (size_t)o, r0, r1, nullptr);
        const double s = r0 * r0 + r1 * r1;
        if (weights) weights[o] = ba_loss_drho(ls.kind, ls.a, ls.b, s);
        cnt = s > ls.b ? 1.0 : 0.0;
        ss = s;
        m = s;
    }
    for (int k = 32; k; k >>= 1) { const double v = __shfl_down(m, k); if (v > m || v != v) m = v; }
    __shared__ double shm[4];
    if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) if (shm[i] > m || shm[i] != shm[i]) m = shm[i];
        atomicMax(reinterpret_cast<unsigned long long *>(maxout), (unsigned long long)__double_as_longlong(m));
    }
    const double c0 = block_sum(cnt, sh);
    const double mine[2] = {c0, block_sum(ss, sh)};
    finish_sums<2>(mine, partial, (int)gridDim.x, fin, sh);
}

// max |v| over two arrays (the line search's |direction|_inf); *out zeroed by the caller.  Non-negative doubles
// order like their bit patterns: one integer atomicMax per workgroup, order-independent.
__global__ __launch_bounds__(256) void k_ba_absmax(const double *a, size_t na, const double *b, size_t nb, double *out)
{
    __shared__ double sh[4];
    double m = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (size_t)gridDim.x * 256) {
        const double v = fabs(i < na ? a[i] : b[i - na]);
        if (v > m || v != v) m = v;
    }
    for (int o = 32; o; o >>= 1) { const double v = __shfl_down(m, o); if (v > m || v != v) m = v; }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) if (sh[i] > m || sh[i] != sh[i]) m = sh[i];
        atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(m));
    }
}

// out[slot] = scale * sum(partial[0..n)) in a fixed order (deterministic)
// (flag -> flag_out: the factorisation's flag word rides home with the scalars of the step instead of in a copy of its own)
__global__ __launch_bounds__(256) void k_finish_sum(const double *partial, int n, double *out, double scale, const int *flag = nullptr, double *flag_out = nullptr)
{
    __shared__ double sh[4];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += partial[i];
    const double s = block_sum(v, sh);
    if (threadIdx.x == 0) { *out = scale * s; if (flag) *flag_out = (double)*flag; }
}
// K5: per point  Vraw = sum Jp'Jp (3x3), gpraw = sum Jp'r
__device__ __forceinline__ void point_raw_body(const BaDev &d, int j)
{
    if (j >= d.np) return;
    double V[9] = {0}, g[3] = {0};
    for (int o = d.pt_off[j]; o < d.pt_off[j + 1]; ++o)
        for (int i = 0; i < 2; ++i) {
            const double *q = d.J + JROW * (size_t)o + 20 + 3 * i;       // Jp and r: 64 contiguous bytes of the row
            const double ri = d.J[JROW * (size_t)o + 26 + i];
            for (int a = 0; a < 3; ++a) {
                g[a] += q[a] * ri;
                for (int b = 0; b < 3; ++b) V[3 * a + b] += q[a] * q[b];
            }
        }
    for (int a = 0; a < 9; ++a) d.Vraw[9 * (size_t)j + a] = V[a];
    for (int a = 0; a < 3; ++a) d.gpraw[3 * (size_t)j + a] = g[a];
}
__global__ void k_ba_point_raw(BaDev d)
{
    point_raw_body(d, blockIdx.x * blockDim.x + threadIdx.x);
}

// K5: per camera  Uraw = sum Jc'Jc (10x10), gcraw = sum Jc'r ; one workgroup per camera, eight groups of
// 128 threads: group g stages and sums the 32-observation chunks g, g+8, ... (a camera of the reference's own
// regime sees thousands of observations), the eight partial sums are added in group order.
// With few cameras (the reference's regime) a camera is further split over `split` workgroups so that
// the launch fills the chip; their partial sums go to d.csplit and are added in order by the workgroup that finishes last.
#define CR_GROUPS 8
// (point_blocks > 0: the launch also carries K5's per-point part -- the two read the same rows and depend on nothing of each other --
//  in that many workgroups BEHIND the cameras': one launch less per evaluation with a Jacobian)
__global__ __launch_bounds__(128 * CR_GROUPS) void k_ba_cam_raw(BaDev d, int split, int cam_blocks)
{
    __shared__ __attribute__((aligned(16))) double sh[CR_GROUPS][32 * 22];
    __shared__ double part[CR_GROUPS][110];
    if ((int)blockIdx.x >= cam_blocks) {       // (uniform over the workgroup: no barrier is skipped by part of it)
        point_raw_body(d, ((int)blockIdx.x - cam_blocks) * (128 * CR_GROUPS) + (int)threadIdx.x);
        return;
    }
    const int c = blockIdx.x / split, sidx = blockIdx.x - c * split, g = threadIdx.x >> 7, t = threadIdx.x & 127;
    // thread t < 110 of a group owns one entry: 0..99 of U (a = t/10, b = t%10), 100..109 of g
    double acc = 0.0;
    const int e0 = d.cam_obs_off[c], e1 = d.cam_obs_off[c + 1];
    for (int base0 = e0 + 32 * CR_GROUPS * sidx; base0 < e1; base0 += 32 * CR_GROUPS * split) {      // uniform trip count over the groups
        const int base = base0 + 32 * g;
        // stage 32 observations' (Jc 20 + r 2) rows in LDS
        __syncthreads();
        {   // 32 observations x (Jc 10 chunks + r 1 chunk) of 16 bytes over 128 threads: three per thread, the index
            // loads and then the row loads issued together
            int oo[3], prt[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int i = t + 128 * q, e = base + i / 11;
                prt[q] = i % 11;
                oo[q] = (i < 32 * 11 && e < e1) ? d.cam_obs[e] : -1;
            }
            f64x2 vv[3];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                vv[q] = oo[q] < 0 ? (f64x2){0.0, 0.0}
                                  : *reinterpret_cast<const f64x2 *>(d.J + JROW * (size_t)oo[q] + (prt[q] < 10 ? 2 * prt[q] : 26));
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (t + 128 * q < 32 * 11) *reinterpret_cast<f64x2 *>(&sh[g][((t + 128 * q) / 11) * 22 + 2 * prt[q]]) = vv[q];
        }
        __syncthreads();
        if (t < 110) {
            const int a = t < 100 ? t / 10 : t - 100, b = t % 10;
            for (int oi = 0; oi < 32; ++oi) {
                const double *row = sh[g] + oi * 22;
                if (t < 100) acc += row[a] * row[b] + row[10 + a] * row[10 + b];
                else acc += row[a] * row[20] + row[10 + a] * row[21];
            }
        }
    }
    if (t < 110) part[g][t] = acc;
    __syncthreads();
    if (g == 0 && t < 110) {
        double s = 0.0;
        for (int k = 0; k < CR_GROUPS; ++k) s += part[k][t];
        if (split > 1) __hip_atomic_store(d.csplit + ((size_t)c * split + sidx) * 256 + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (t < 100) d.Uraw[100 * (size_t)c + t] = s;
        else d.gcraw[10 * (size_t)c + (t - 100)] = s;
    }
    if (split > 1) {
        // the camera's workgroups finish the sum themselves (k_ba_cam_fin, a launch of its own, before): partials delivered as
        // agent-coherent stores and drained, one ticket per workgroup, the one that draws the last adds them in index order --
        // the hand-off of finish_sums, per camera
        __shared__ int s_last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(d.tickets + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)split - 1u;
        __syncthreads();
        if (s_last && g == 0 && t < 110) {
            double s = 0.0;
            for (int k = 0; k < split; ++k) s += __hip_atomic_load(d.csplit + ((size_t)c * split + k) * 256 + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t < 100) d.Uraw[100 * (size_t)c + t] = s;
            else d.gcraw[10 * (size_t)c + (t - 100)] = s;
            if (t == 0) __hip_atomic_store(d.tickets + c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// Jacobi scaling (initial point) or clamped LM diagonal (scaled Jacobian) from the raw diagonals
__global__ void k_ba_diag(BaDev d, int what, double lo, double hi, int jacobi)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.n) {
        // reduced coordinate i -> (camera, k): binary search over cam_off
        int a = 0, b = d.nc - 1;
        while (a < b) { int m = (a + b + 1) >> 1; if (d.cam_off[m] <= i) a = m; else b = m - 1; }
        while (d.cam_dim[a] == 0 || d.cam_off[a] + d.cam_dim[a] <= i) ++a;
        const int k = i - d.cam_off[a];
        const double u = d.Uraw[100 * (size_t)a + 11 * k];
        if (what == 0) d.sc[i] = jacobi ? 1.0 / (1.0 + sqrt(u)) : 1.0;
        else d.dgc[i] = fmin(fmax(u * d.sc[i] * d.sc[i], lo), hi);
    }
    const int j = i;
    if (j < 3 * d.np) {
        const double v = d.Vraw[9 * (size_t)(j / 3) + 4 * (j % 3)];
        if (what == 0) d.sp[j] = jacobi ? 1.0 / (1.0 + sqrt(v)) : 1.0;
        else d.dgp[j] = fmin(fmax(v * d.sp[j] * d.sp[j], lo), hi);
    }
}

// Double-double arithmetic for the landmarks' 3 x 3 inverses (error-free sums and, through the fused multiply-add, products: Dekker /
// Knuth; Hida, Li, Bailey, "Algorithms for quad-double precision floating point arithmetic").  A landmark seen by two cameras has a
// badly conditioned V: det and the cofactors are differences of products that cancel three to four digits, and in plain FP64 every
// rounding of V, of a product or of a difference comes back multiplied by that factor -- up to 4e-13 of the block where the format
// gives 1e-16.  Carried in double-double from the FP64 inputs to the one final rounding, the inverse is the
// correctly rounded inverse of what the kernel was given.  About 300 additions and 70 FMAs per landmark and iteration, a dependent chain
// in a launch of one thread per landmark: 1 ... 4 us of an iteration, 0.3 ... 0.7 % at cfg 4 and below, inside the spread of the solves
// of one process.
// (every operation below must be the rounded FP64 operation it is written as: a product contracted into the sum that uses it makes that
//  sum more accurate and the error term computed behind it wrong -- measured: with the default contraction the inverses came out no
//  better than plain FP64)
#define DD_EXACT _Pragma("clang fp contract(off)")
struct dd { double h, l; };
__device__ __forceinline__ dd dd_fast_sum(double a, double b) { DD_EXACT const double s = a + b; return {s, b - (s - a)}; }      // |a| >= |b|
__device__ __forceinline__ dd dd_two_sum(double a, double b) { DD_EXACT const double s = a + b, bb = s - a; return {s, (a - (s - bb)) + (b - bb)}; }
__device__ __forceinline__ dd dd_two_prod(double a, double b) { DD_EXACT const double p = a * b; return {p, __builtin_fma(a, b, -p)}; }
__device__ __forceinline__ dd dd_add(dd a, dd b) { DD_EXACT const dd s = dd_two_sum(a.h, b.h); return dd_fast_sum(s.h, s.l + (a.l + b.l)); }
__device__ __forceinline__ dd dd_sub(dd a, dd b) { return dd_add(a, dd{-b.h, -b.l}); }
__device__ __forceinline__ dd dd_mul(dd a, dd b) { DD_EXACT const dd p = dd_two_prod(a.h, b.h); return dd_fast_sum(p.h, p.l + (a.h * b.l + a.l * b.h)); }
__device__ __forceinline__ dd dd_mul_d(dd a, double b) { DD_EXACT const dd p = dd_two_prod(a.h, b); return dd_fast_sum(p.h, p.l + a.l * b); }
// a / b rounded to FP64: two quotient digits
__device__ __forceinline__ double dd_div(dd a, dd b)
{
    DD_EXACT
    const double q1 = a.h / b.h;
    const dd r = dd_sub(a, dd_mul_d(b, q1));
    return q1 + r.h / b.h;
}

// per point: V = scaled Vraw + dgp/radius, V^-1, scaled g_p
__device__ __forceinline__ void point_solve_body(const BaDev &d, int j, double inv_radius)
{
    const double *s = d.sp + 3 * (size_t)j, *Vr = d.Vraw + 9 * (size_t)j, *dg = d.dgp + 3 * (size_t)j;
    // the upper triangle of V (the raw block is symmetric: the same products in the same order on both sides)
    auto entry = [&](int p, int q) {
        dd v = dd_mul_d(dd_two_prod(Vr[3 * p + q], s[p]), s[q]);
        return p == q ? dd_add(v, dd_two_prod(dg[p], inv_radius)) : v;
    };
    const dd a = entry(0, 0), b = entry(0, 1), c = entry(0, 2), e = entry(1, 1), f = entry(1, 2), g = entry(2, 2);
    const dd A = dd_sub(dd_mul(e, g), dd_mul(f, f)), B = dd_sub(dd_mul(c, f), dd_mul(b, g)), C = dd_sub(dd_mul(b, f), dd_mul(c, e));
    const dd det = dd_add(dd_add(dd_mul(a, A), dd_mul(b, B)), dd_mul(c, C));
    double Vi[9];
    if (!(det.h > 0.0) || !isfinite(det.h)) {
        d.flag[0] = 1;
        d.flag[1] = 1;      // (the trailing workgroups of the Schur diagonal launch -- k_ba_flag_reset where they do not run -- clear the flag words BEHIND this kernel: they restore [0] from this word)
        for (int i = 0; i < 9; ++i) Vi[i] = 0.0;
    } else {
        Vi[0] = dd_div(A, det); Vi[1] = dd_div(B, det); Vi[2] = dd_div(C, det);
        Vi[3] = Vi[1]; Vi[4] = dd_div(dd_sub(dd_mul(a, g), dd_mul(c, c)), det); Vi[5] = dd_div(dd_sub(dd_mul(b, c), dd_mul(a, f)), det);
        Vi[6] = Vi[2]; Vi[7] = Vi[5]; Vi[8] = dd_div(dd_sub(dd_mul(a, e), dd_mul(b, b)), det);
    }
    for (int i = 0; i < 9; ++i) d.Vinv[9 * (size_t)j + i] = Vi[i];
    for (int i = 0; i < 3; ++i) d.gps[3 * (size_t)j + i] = d.gpraw[3 * (size_t)j + i] * s[i];
}
__global__ void k_ba_point_solve(BaDev d, double inv_radius)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < d.np) point_solve_body(d, j, inv_radius);
}

// scaled W_o = (Jc' Jp) (10 x 3) of one observation
__device__ __forceinline__ void load_W(const BaDev &d, int o, int c, int j, double *W)
{
    const double *jc = d.J + JROW * (size_t)o, *jp = jc + 20;
    const int off = d.cam_off[c], dc = d.cam_dim[c];
    for (int a = 0; a < 10; ++a) {
        const double sa = a < dc ? d.sc[off + a] : 0.0;
        for (int b = 0; b < 3; ++b)
            W[3 * a + b] = (jc[a] * jp[b] + jc[10 + a] * jp[3 + b]) * sa * d.sp[3 * (size_t)j + b];
    }
}

// K6: Schur complement.  Contributions are accumulated in a camera-block-major buffer
// Sb[c][c2][10][10] (c2 <= c): one wave owns one observation pair (o,o2) of a point at a time and
// adds its 10x10 block -Y_o W_o2^T with two wave-wide f64 atomic instructions over 800
// contiguous bytes (full-rate shape: MI355X_MICROARCH.md, global float atomics).
__global__ __launch_bounds__(256) void k_ba_schur(BaDev d, double *Sb)
{
    const int j = blockIdx.x;                      // point
    const int o0 = d.pt_off[j], k = d.pt_off[j + 1] - o0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double *Vi = d.Vinv + 9 * (size_t)j;
    const double sp0 = d.sp[3 * (size_t)j], sp1 = d.sp[3 * (size_t)j + 1], sp2 = d.sp[3 * (size_t)j + 2];
    for (int pr = w; pr < k * k; pr += nw) {
        const int o = o0 + pr / k, o2 = o0 + pr % k;
        const int c = d.ocam[o], c2 = d.ocam[o2];
        if (c2 > c) continue;
        const int dc = d.cam_dim[c], dc2 = d.cam_dim[c2];
        if (dc == 0 || dc2 == 0) continue;
        const int off = d.cam_off[c], off2 = d.cam_off[c2];
        const double *jc = d.J + JROW * (size_t)o, *jp = jc + 20;
        const double *jc2 = d.J + JROW * (size_t)o2, *jp2 = jc2 + 20;
        double *blk = Sb + ((size_t)c * d.nc + c2) * 100;
#pragma unroll
        for (int rep = 0; rep < 2; ++rep) {
            const int e = lane + 64 * rep;
            if (e >= 100) break;
            const int a = e / 10, b = e % 10;
            if (a >= dc || b >= dc2) continue;
            const double sa = d.sc[off + a], sb = d.sc[off2 + b];
            const double ja0 = jc[a] * sa, ja1 = jc[10 + a] * sa, jb0 = jc2[b] * sb, jb1 = jc2[10 + b] * sb;
            // W[a][m] (this row of W_o), W2[b][m]
            const double wa0 = (ja0 * jp[0] + ja1 * jp[3]) * sp0, wa1 = (ja0 * jp[1] + ja1 * jp[4]) * sp1,
                         wa2 = (ja0 * jp[2] + ja1 * jp[5]) * sp2;
            const double wb0 = (jb0 * jp2[0] + jb1 * jp2[3]) * sp0, wb1 = (jb0 * jp2[1] + jb1 * jp2[4]) * sp1,
                         wb2 = (jb0 * jp2[2] + jb1 * jp2[5]) * sp2;
            const double y0 = wa0 * Vi[0] + wa1 * Vi[3] + wa2 * Vi[6];
            const double y1 = wa0 * Vi[1] + wa1 * Vi[4] + wa2 * Vi[7];
            const double y2 = wa0 * Vi[2] + wa1 * Vi[5] + wa2 * Vi[8];
            unsafeAtomicAdd(blk + e, -(y0 * wb0 + y1 * wb1 + y2 * wb2));
        }
    }
}

// ---- gather form of K6 (default): the structure of the observation graph is fixed for a
// solve, so the ordered observation pairs (o, o2) of every camera-pair block (c2 <= c) are
// listed once (count -> scan -> fill -> per-block sort = a fixed order), and every LM iteration
// one wave SUMS its block's contributions in registers and stores the 10x10 block once: no
// atomics, 0.4 GB of plain stores instead of 4.4 GB of atomic traffic, and the reduced system
// -- hence the whole solve -- is bit-reproducible from run to run.
__device__ __forceinline__ bool pair_key(const BaDev &d, int o, int o2, int &key)
{
    if (o == o2) return false;   // an observation with itself: walked from the per-camera list (k_ba_schur_diag_mfma)
    const int c = d.ocam[o], c2 = d.ocam[o2];
    if (c2 > c || d.cam_dim[c] == 0 || d.cam_dim[c2] == 0) return false;
    key = c * d.nc + c2;
    return true;
}

__global__ __launch_bounds__(256) void k_pair_count(BaDev d, int *cnt)
{
    const int j = blockIdx.x, o0 = d.pt_off[j], k = d.pt_off[j + 1] - o0;
    for (int pr = threadIdx.x; pr < k * k; pr += blockDim.x) {
        int key;
        if (pair_key(d, o0 + pr / k, o0 + pr % k, key)) atomicAdd(cnt + key, 1);
    }
}

// exclusive scan of n ints (n ~ nc^2) in three passes: per-chunk sums (one workgroup per 1024-element chunk, coalesced),
// scan of the chunk sums by one workgroup (in place; a contiguous run per thread once there are more than 1024 chunks),
// per-chunk scan with offset (coalesced)
__global__ __launch_bounds__(1024) void k_scan_sums(const int *in, int *sums, int n)
{
    __shared__ int sh[16];
    const int i = blockIdx.x * 1024 + threadIdx.x;
    int tot;
    (void)wg_scan_incl<int, 1024>(i < n ? in[i] : 0, sh, tot);
    if (threadIdx.x == 1023) sums[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void k_scan_top(int *sums, int nchunks, int *total)   // in place
{
    const int tot = wg_scan_array(sums, nchunks, sums, 0);
    if (threadIdx.x == 0) *total = tot;
}
__global__ __launch_bounds__(1024) void k_scan_apply(const int *in, const int *sums, int *out, int n)
{
    __shared__ int sh[16];
    const int i = blockIdx.x * 1024 + threadIdx.x;
    const int v = i < n ? in[i] : 0;
    int tot;
    const int inc = wg_scan_incl<int, 1024>(v, sh, tot);
    if (i < n) out[i] = sums[blockIdx.x] + inc - v;
}

__global__ __launch_bounds__(256) void k_pair_fill(BaDev d, const int *off, int *fill, unsigned long long *list)
{
    const int j = blockIdx.x, o0 = d.pt_off[j], k = d.pt_off[j + 1] - o0;
    for (int pr = threadIdx.x; pr < k * k; pr += blockDim.x) {
        const int o = o0 + pr / k, o2 = o0 + pr % k;
        int key;
        if (pair_key(d, o, o2, key)) list[off[key] + atomicAdd(fill + key, 1)] = ((unsigned long long)o << 32) | (unsigned)o2;
    }
}

// Count, scan and fill in ONE workgroup for the reference's own problem sizes (up to 32 cameras: nc^2 <= 1024 keys; round 5): the six
// launches above (clear, count, three scan passes, fill) were ~25 us of a solve that is ~400 us long, and the host spent as long again
// enqueueing them.  Per-key counters and fill cursors live in LDS; a thread walks the pairs of its landmarks.  The order inside a key
// is whatever the atomics gave -- as in k_pair_fill -- and the two sort kernels behind make it ascending.
__global__ __launch_bounds__(1024) void k_pair_small(BaDev d, int *off, unsigned long long *list, int nkeys, int *long_count)
{
    __shared__ int cnt[1024], cur[1024], sh[16];
    const int t = threadIdx.x;
    cnt[t] = 0; cur[t] = 0;
    if (t == 0) *long_count = 0;          // (the general path's clear covers this word)
    __syncthreads();
    // tp threads per landmark (a power of two): they share out its pairs
    int tp = 1;
    while (2 * tp * d.np <= 1024 && tp < 64) tp *= 2;
    const int sub = t & (tp - 1), jstep = 1024 / tp;
    for (int j = t / tp; j < d.np; j += jstep) {
        const int o0 = d.pt_off[j], k = d.pt_off[j + 1] - o0;
        for (int pr = sub; pr < k * k; pr += tp) {
            int key;
            if (pair_key(d, o0 + pr / k, o0 + pr % k, key)) atomicAdd(&cnt[key], 1);
        }
    }
    __syncthreads();
    const int v = t < nkeys ? cnt[t] : 0;
    int tot;
    const int inc = wg_scan_incl<int, 1024>(v, sh, tot);
    if (t < nkeys) off[t] = inc - v;
    if (t == 1023) off[nkeys] = tot;
    __syncthreads();
    cnt[t] = inc - v;
    __syncthreads();
    for (int j = t / tp; j < d.np; j += jstep) {
        const int o0 = d.pt_off[j], k = d.pt_off[j + 1] - o0;
        for (int pr = sub; pr < k * k; pr += tp) {
            const int o = o0 + pr / k, o2 = o0 + pr % k;
            int key;
            if (pair_key(d, o, o2, key)) list[cnt[key] + atomicAdd(&cur[key], 1)] = ((unsigned long long)o << 32) | (unsigned)o2;
        }
    }
}

// fixed order inside every block: ascending (o, o2); segments are short except the diagonal blocks
#define PAIR_SORT_SHORT 32
// (long_keys / long_count: the keys whose segments are too long for a thread, listed for k_pair_sort_long -- round 5: that kernel was
//  launched with a workgroup per KEY, a million workgroups at cfg 5 of which none had anything to do: 0.41 ms of every solve that
//  builds its lists)
__global__ void k_pair_sort(const int *off, unsigned long long *list, int nkeys, int *long_keys, int *long_count)
{
    const int key = blockIdx.x * blockDim.x + threadIdx.x;
    if (key >= nkeys) return;
    unsigned long long *a = list + off[key];
    const int n = off[key + 1] - off[key];
    if (n > PAIR_SORT_SHORT) { long_keys[atomicAdd(long_count, 1)] = key; return; }           // long segments: k_pair_sort_long
    for (int i = 1; i < n; ++i) {
        const unsigned long long v = a[i];
        int p = i - 1;
        while (p >= 0 && a[p] > v) { a[p + 1] = a[p]; --p; }
        a[p + 1] = v;
    }
}

// Long segments (few cameras sharing thousands of landmarks: the reference's own regime, 3..25 views):
// one workgroup per segment, bitonic sort -- in LDS up to 4096 entries, in global memory beyond.
__global__ __launch_bounds__(256) void k_pair_sort_long(const int *off, unsigned long long *list, const int *long_keys, const int *long_count)
{
    __shared__ unsigned long long sh[4096];
    const int t = threadIdx.x, nlong = *long_count;
    for (int idx = blockIdx.x; idx < nlong; idx += gridDim.x) {      // (uniform over the workgroup)
    const int key = long_keys[idx];
    const int n = off[key + 1] - off[key];
    __syncthreads();                                               // the staging of the last key is free
    unsigned long long *g = list + off[key];
    int P = 64;
    while (P < n) P <<= 1;
    const bool in_lds = n <= 4096;
    if (in_lds) {
        for (int i = t; i < n; i += 256) sh[i] = g[i];
        __syncthreads();
    }
    unsigned long long *a = in_lds ? sh : g;
    // normalised bitonic network: every comparator ascending, the first step of a merge pairs i with its
    // mirror image i ^ (k - 1); entries beyond n count as +infinity and therefore never move
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < n; i += 256) {
                const int l = j == (k >> 1) ? (i ^ (k - 1)) : (i ^ j);
                if (l > i && l < n) {
                    const unsigned long long x = a[i], y = a[l];
                    if (x > y) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
    if (in_lds) for (int i = t; i < n; i += 256) g[i] = sh[i];
    }
}

// ---- MFMA form of the gather (default).  k_ba_wy tabulates, per observation, the scaled
// W_o = Jc' Jp (10 x 3) and Y_o = W_o Vinv (both [m][a], camera coordinate fastest; rows beyond the
// camera's tangent size are zero).  A block (c, c2) is then  - [Y_o1 Y_o2 ...] [W_o1' W_o2' ...]^T,
// a 10 x 3P by 3P x 10 product: ceil(3P/4) v_mfma_f64_16x16x4_f64 steps per wave with two
// 8-byte gathers per lane and step, instead of ~30 loads and ~40 flops per lane and pair.
__global__ __launch_bounds__(256) void k_ba_wy(BaDev d)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int o = (int)(idx / 10), a = (int)(idx - 10 * (long)o);
    if (o >= d.no) return;
    const int c = d.ocam[o], j = d.opt[o];
    double w[3] = {0.0, 0.0, 0.0}, y[3] = {0.0, 0.0, 0.0};
    if (a < d.cam_dim[c]) {
        const double *jc = d.J + JROW * (size_t)o, *jp = jc + 20, *Vi = d.Vinv + 9 * (size_t)j;
        const double sa = d.sc[d.cam_off[c] + a];
        const double ja0 = jc[a] * sa, ja1 = jc[10 + a] * sa;
        for (int m = 0; m < 3; ++m) w[m] = (ja0 * jp[m] + ja1 * jp[3 + m]) * d.sp[3 * (size_t)j + m];
        for (int m = 0; m < 3; ++m) y[m] = w[0] * Vi[m] + w[1] * Vi[3 + m] + w[2] * Vi[6 + m];
    }
    double *outw = d.WY + WROW * (size_t)o, *outy = outw + WROW * (size_t)d.no;
    for (int m = 0; m < 3; ++m) { outw[10 * m + a] = w[m]; outy[10 * m + a] = y[m]; }
}

// acc -= [Y of the listed first observations] [W of the listed second observations]^T for `cnt`
// (<= 64) pairs held one per lane in `pr` (o << 32 | o2)
// RHS: column 10 of the B operand carries the scaled point gradient of the pair's landmark, so
// column 10 of the block comes out as  - sum Y_o gp_j(o)  -- the camera's reduced right-hand side.
// SMB: MFMA steps (of 4 k) per trip of the gather loop -- 4 for the short lists of the one-wave kernel,
// 12 (16 pairs' worth of gathers in flight) where a wave walks hundreds of pairs
template <bool RHS, int SMB>
__device__ __forceinline__ f64x4 schur_mfma_chunk(const double *__restrict__ Wt, const double *__restrict__ Yt, unsigned long long pr, int cnt, int lane, f64x4 acc,
                                                  const int *__restrict__ opt = nullptr, const double *__restrict__ gps = nullptr)
{
    const int i = lane & 15, kk = lane >> 4, K = 3 * cnt;
    for (int k0 = 0; k0 < K; k0 += 4 * SMB) {   // SMB MFMA steps per trip: 2 SMB gathers in flight per lane
        double a[SMB], b[SMB];
#pragma unroll
        for (int u = 0; u < SMB; ++u) {
            const int k = k0 + 4 * u + kk, p = k / 3, m = k - 3 * p;
            const unsigned long long e = __shfl(pr, p & 63);
            a[u] = 0.0; b[u] = 0.0;
            if (k < K && i < 10) {
                a[u] = Yt[WROW * (size_t)(e >> 32) + 10 * m + i];
                b[u] = Wt[WROW * (size_t)(e & 0xFFFFFFFFu) + 10 * m + i];
            }
            if (RHS && k < K && i == 10) b[u] = gps[3 * (size_t)opt[(unsigned)(e & 0xFFFFFFFFu)] + m];
        }
#pragma unroll
        for (int u = 0; u < SMB; ++u)
            if (k0 + 4 * u < K) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[u], b[u], acc, 0, 0, 0);
    }
    return acc;
}

// (Round 5, measured and not kept -- profiles/r05_experiments/stream_kernels_schur_*.txt, 515-541 us per cfg-5 launch as it stands: more
//  gathers in flight per block, SMB = 8 / 12: 557 / 675 us, the extra trips are predicated-off instructions; the operands fetched as
//  whole 240-byte rows, 16 bytes per lane, through LDS: 674 us, same bits; two / three / four blocks per wave with all their gathers in
//  flight at once: 689 / 819 / 883 us.  Neither latency nor the number of load instructions is what bounds it.)
// one wave per strictly-lower block (c, c2 < c), written straight into the dense reduced system
template <int SMB>
__global__ __launch_bounds__(256) void k_ba_schur_mfma(BaDev d, const int *off, const unsigned long long *list)
{
    // (Round 4 tried dealing whole block rows to one XCD -- row c on XCD c % 8, so that camera c's Y rows are fetched into one
    // L2 instead of eight: 547 us against 515 us per cfg-5 launch.  The gathers are 8 bytes per lane out of 240-byte rows; the
    // kernel is bound by the address rate of the gather path, not by what is behind it.  Removed.)
    const int lane = threadIdx.x & 63;
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nlow = d.nc * (d.nc - 1) / 2;
    if (blk >= nlow) return;
    int c = (int)((sqrt(8.0 * blk + 1.0) + 1.0) * 0.5);
    while (c * (c + 1) / 2 <= blk) ++c;
    while (c * (c - 1) / 2 > blk) --c;
    const int c2 = blk - c * (c - 1) / 2, key = c * d.nc + c2;
    const int dc = d.cam_dim[c], dc2 = d.cam_dim[c2];
    if (dc == 0 || dc2 == 0) return;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const int e0 = off[key], e1 = off[key + 1];
    for (int base = e0; base < e1; base += 64) {
        const int cnt = min(64, e1 - base);
        const unsigned long long pr = lane < cnt ? list[base + lane] : 0ull;
        acc = schur_mfma_chunk<false, SMB>(d.WY, d.WY + WROW * (size_t)d.no, pr, cnt, lane, acc);
    }
    // C/D layout: column = lane & 15, row = (lane >> 4) + 4 * reg
    const int col = lane & 15, r0 = lane >> 4;
    double *out = d.S + (size_t)d.cam_off[c] * d.npad + d.cam_off[c2];
    if (col < dc2)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            if (r0 + 4 * reg < dc) out[(size_t)(r0 + 4 * reg) * d.npad + col] = acc[reg];
}

// The same for long pair lists (few cameras sharing thousands of landmarks): one 8-wave workgroup per block,
// wave w takes the 64-pair chunks w, w+8, ...; the eight partial blocks are added in wave order.
__global__ __launch_bounds__(512) void k_ba_schur_mfma_wg(BaDev d, const int *off, const unsigned long long *list)
{
    __shared__ double part[8][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, blk = blockIdx.x;
    int c = (int)((sqrt(8.0 * blk + 1.0) + 1.0) * 0.5);
    while (c * (c + 1) / 2 <= blk) ++c;
    while (c * (c - 1) / 2 > blk) --c;
    const int c2 = blk - c * (c - 1) / 2, key = c * d.nc + c2;
    const int dc = d.cam_dim[c], dc2 = d.cam_dim[c2];
    if (dc == 0 || dc2 == 0) return;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const int e0 = off[key], e1 = off[key + 1];
    for (int base = e0 + 64 * w; base < e1; base += 64 * 8) {
        const int cnt = min(64, e1 - base);
        const unsigned long long pr = lane < cnt ? list[base + lane] : 0ull;
        acc = schur_mfma_chunk<false, 12>(d.WY, d.WY + WROW * (size_t)d.no, pr, cnt, lane, acc);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) part[w][((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
    __syncthreads();
    if (threadIdx.x < 256) {
        const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
        if (a < dc && b < dc2) {
            double v = 0.0;
            for (int k = 0; k < 8; ++k) v += part[k][threadIdx.x];
            d.S[(size_t)(d.cam_off[c] + a) * d.npad + d.cam_off[c2] + b] = v;
        }
    }
}

// diagonal blocks: one 16-wave workgroup per camera; wave w takes the observations w, w+16, ... of
// the camera (a pair (o, o)) and the listed pairs of the key (c, c); the 16 partial blocks are
// summed in wave order and  scaled U + D/radius  is added before the store into S; column 10 of
// the same product is the camera's reduced right-hand side.
// (fin: -1 the right-hand side stays in d.rhs; 0 / 1 it goes straight into row n of the padded system -- a launch of its own, k_ba_S_finish,
//  did that until round 5 -- and with 1 the cell in d.rhs takes the one-launch backward substitution's "not there yet" pattern)
__device__ __forceinline__ void schur_diag_finish(const BaDev &d, int c, int idx, double v, double inv_radius, int fin = -1)
{
    const int a = idx >> 4, b = idx & 15, dc = d.cam_dim[c], offc = d.cam_off[c];
    if (a < dc && b < dc) {
        v += d.Uraw[100 * (size_t)c + 10 * a + b] * d.sc[offc + a] * d.sc[offc + b];
        if (a == b) v += d.dgc[offc + a] * inv_radius;
        d.S[(size_t)(offc + a) * d.npad + offc + b] = v;
    } else if (a < dc && b == 10) {   // reduced right-hand side: scaled gc - sum_o Y_o gp
        const double r = d.gcraw[10 * (size_t)c + a] * d.sc[offc + a] + v;
        if (fin < 0) d.rhs[offc + a] = r;
        else {
            d.S[(size_t)d.n * d.npad + offc + a] = r;
            if (fin == 1) reinterpret_cast<unsigned long long *>(d.rhs)[offc + a] = 0xFFFFFFFFFFFFFFFFull;
            else d.rhs[offc + a] = r;
        }
    }
}
// (`split` > 1: a camera's observations are spread over that many workgroups, see k_ba_cam_raw; SMB: gather
// depth, 12 in that latency-bound regime, 4 when a thousand cameras keep the chip full anyway)
// (fin >= 0, round 5: the launch also does everything that lies between the Schur build and the factorisation (round 4's k_ba_S_finish) -- the cameras'
//  workgroups put their right-hand sides into row n themselves (schur_diag_finish), the workgroups BEHIND them write the rest of the
//  padded rows and the factorisation's flag word and stream counters: one launch less per LM iteration)
template <int SMB>
__global__ __launch_bounds__(1024) void k_ba_schur_diag_mfma(BaDev d, const int *off, const unsigned long long *list, double inv_radius, int split, int fin = -1)
{
    __shared__ double part[16][256];
    if ((int)blockIdx.x >= d.nc * split) {      // (uniform over the workgroup)
        const size_t idx = (size_t)((int)blockIdx.x - d.nc * split) * 1024 + threadIdx.x, cnt = (size_t)(d.npad - d.n) * d.npad;
        if (idx == 0) { const int ps = d.flag[1]; d.flag[1] = 0; d.flag[0] = ps ? 1 : 0; }
        else if ((idx >= 2 && idx < 8) || (idx >= 12 && idx < 24)) d.flag[idx] = 0;
        if (idx >= cnt) return;
        const int i = d.n + (int)(idx / d.npad), j = (int)(idx % d.npad);
        if (i == d.n && j < d.n) return;        // the cameras' workgroups'
        d.S[(size_t)i * d.npad + j] = i == j ? (i == d.n ? RCN_RHS_BETA : 1.0) : 0.0;
        return;
    }
    const int c = blockIdx.x / split, sidx = blockIdx.x - c * split, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int dc = d.cam_dim[c], key = c * d.nc + c;
    if (dc == 0) return;
    const int W = 16 * split, ww = 16 * sidx + w;          // this wave's rank among all the camera's waves
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const int o0 = d.cam_obs_off[c], o1 = d.cam_obs_off[c + 1];
    for (int base = o0 + ww; base < o1; base += W * 64) {
        const int cnt = min(64, (o1 - base + W - 1) / W);
        unsigned long long pr = 0ull;
        if (lane < cnt) { const unsigned o = (unsigned)d.cam_obs[base + W * lane]; pr = ((unsigned long long)o << 32) | o; }
        acc = schur_mfma_chunk<true, SMB>(d.WY, d.WY + WROW * (size_t)d.no, pr, cnt, lane, acc, d.opt, d.gps);
    }
    for (int base = off[key] + ww; base < off[key + 1]; base += W * 64) {   // the same camera seen twice by one landmark
        const int cnt = min(64, (off[key + 1] - base + W - 1) / W);
        const unsigned long long pr = lane < cnt ? list[base + W * lane] : 0ull;
        acc = schur_mfma_chunk<false, SMB>(d.WY, d.WY + WROW * (size_t)d.no, pr, cnt, lane, acc);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) part[w][((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
    __syncthreads();
    if (threadIdx.x < 256) {
        double v = 0.0;
        for (int k = 0; k < 16; ++k) v += part[k][threadIdx.x];
        if (split > 1) __hip_atomic_store(d.csplit + ((size_t)c * split + sidx) * 256 + threadIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else schur_diag_finish(d, c, threadIdx.x, v, inv_radius, fin);
    }
    if (split > 1) {      // as in k_ba_cam_raw: the last of the camera's workgroups adds the partial blocks, in index order (k_ba_schur_diag_fin before)
        __shared__ int s_last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(d.tickets + d.nc + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)split - 1u;
        __syncthreads();
        if (s_last && threadIdx.x < 256) {
            double v = 0.0;
            for (int k = 0; k < split; ++k) v += __hip_atomic_load(d.csplit + ((size_t)c * split + k) * 256 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            schur_diag_finish(d, c, threadIdx.x, v, inv_radius, fin);
            if (threadIdx.x == 0) __hip_atomic_store(d.tickets + d.nc + c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// The flag words of a step whose system is NOT finished by the launch above (fin < 0: n a multiple of the block, the forward substitution
// as a launch of its own, the atomic Schur build): what its trailing workgroups do, as one small launch BEHIND the landmark blocks'
// kernel -- [0] restored from the word that kernel raises for a singular block, [1] consumed, the factorisation's counters cleared.
// (a host-side memset of the words stood here: it ran behind k_ba_gradmax's fused launch, which solves the blocks of the first step and of
//  every step behind an accepted one, and wiped the flag of a singular block; the step then went on as a valid one)
__global__ void k_ba_flag_reset(BaDev d)
{
    const int idx = threadIdx.x;
    if (idx == 0) { const int ps = d.flag[1]; d.flag[1] = 0; d.flag[0] = ps ? 1 : 0; }
    else if ((idx >= 2 && idx < 8) || (idx >= 12 && idx < 24)) d.flag[idx] = 0;
}
// padded rows of the dense system: identity (the gather form writes every other lower block itself)
__global__ void k_ba_S_pad(BaDev d)
{
    const int i = d.n + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.npad) d.S[(size_t)i * d.npad + i] = 1.0;
}

// Forward substitution for free: the reduced right-hand side rides through the factorisation as
// row n of the padded system (a padding row: zero elsewhere) under a huge diagonal entry, so the
// panel kernels leave  y = L^-1 b  in that row of the factor:  [S b; b' beta] = [L 0; y' .][L 0; y' .]'.
__global__ void k_ba_S_rhs_row(BaDev d)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > d.n) return;
    d.S[(size_t)d.n * d.npad + j] = j < d.n ? d.rhs[j] : RCN_RHS_BETA;
}
// y out of row n of the factor: sub-diagonal tiles live in L, the last diagonal tile in S
__global__ void k_ba_y_from_row(BaDev d, int sentinel)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d.npad) return;
    const int last0 = (d.npad / chol::BLOCK - 1) * chol::BLOCK;
    d.yc[j] = j < d.n ? (j < last0 ? d.L : d.S)[(size_t)d.n * d.npad + j] : 0.0;
    if (sentinel) reinterpret_cast<unsigned long long *>(d.rhs)[j] = 0xFFFFFFFFFFFFFFFFull;      // the one-launch backward substitution's "not there yet" (the right-hand side itself went into the system's last row)
}

// dense padded reduced system from the block buffer: lower blocks (c2 <= c) of
// S = blockdiag(scaled U + dgc/radius) + Sb ; padded diagonal = 1.  One workgroup per camera row.
__global__ __launch_bounds__(256) void k_ba_S_assemble(BaDev d, const double *Sb, double inv_radius)
{
    const int c = blockIdx.x, t = threadIdx.x;
    if (c >= d.nc) {   // padded rows: identity
        for (int i = d.n + t; i < d.npad; i += 256)
            if (c == d.nc) d.S[(size_t)i * d.npad + i] = 1.0;
        return;
    }
    const int dc = d.cam_dim[c], off = d.cam_off[c];
    if (dc == 0) return;
    for (int idx = t; idx < (c + 1) * 100; idx += 256) {
        const int c2 = idx / 100, e = idx % 100, a = e / 10, b = e % 10;
        const int dc2 = d.cam_dim[c2];
        if (a >= dc || b >= dc2) continue;
        const int off2 = d.cam_off[c2];
        double v = Sb[((size_t)c * d.nc + c2) * 100 + e];
        if (c2 == c) {
            v += d.Uraw[100 * (size_t)c + e] * d.sc[off + a] * d.sc[off + b];
            if (a == b) v += d.dgc[off + a] * inv_radius;
        }
        d.S[(size_t)(off + a) * d.npad + off2 + b] = v;
    }
}

// reduced rhs per camera: scaled gc - sum_o Y_o gp_j(o)   (deterministic order)
__global__ __launch_bounds__(64) void k_ba_cam_rhs(BaDev d)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const int dc = d.cam_dim[c], off = d.cam_off[c];
    if (dc == 0) return;
    double acc[10] = {0};
    for (int e = d.cam_obs_off[c] + lane; e < d.cam_obs_off[c + 1]; e += 64) {
        const int o = d.cam_obs[e], j = d.opt[o];
        double W[30];
        load_W(d, o, c, j, W);
        const double *Vi = d.Vinv + 9 * (size_t)j, *g = d.gps + 3 * (size_t)j;
        const double t0 = Vi[0] * g[0] + Vi[1] * g[1] + Vi[2] * g[2];
        const double t1 = Vi[3] * g[0] + Vi[4] * g[1] + Vi[5] * g[2];
        const double t2 = Vi[6] * g[0] + Vi[7] * g[1] + Vi[8] * g[2];
        for (int a = 0; a < dc; ++a) acc[a] += W[3 * a] * t0 + W[3 * a + 1] * t1 + W[3 * a + 2] * t2;
    }
    for (int a = 0; a < 10; ++a)
        for (int o = 32; o; o >>= 1) acc[a] += __shfl_down(acc[a], o);
    if (lane == 0)
        for (int a = 0; a < dc; ++a) d.rhs[off + a] = d.gcraw[10 * (size_t)c + a] * d.sc[off + a] - acc[a];
}

// ---------------------------------------------------------------------------------------
// K8: point back-substitution, scaled step = -y.  Two passes: per observation  t_o = W_o' y_c  out of the W plane (a
// wave's 64 rows of 240 B staged through LDS as one contiguous block), then per point  -Vinv (g_p - sum_o t_o)  over the
// point's observations in order.
__global__ __launch_bounds__(128) void k_ba_backsub_obs(BaDev d)
{
    __shared__ __attribute__((aligned(16))) double stage[2 * 64 * JLD];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t row0 = (size_t)blockIdx.x * blockDim.x + 64 * w;
    const int nrows = (int)min((long long)64, (long long)d.no - (long long)row0);
    double *mine = stage + w * 64 * JLD;
    if (nrows > 0) rows_to_lds<WCH>(d.WY, row0, nrows, mine, lane);
    __syncthreads();
    if (lane >= nrows) return;
    const size_t o = row0 + lane;
    const int c = d.ocam[o], dc = d.cam_dim[c];
    const double *y = d.yc + d.cam_off[c];
    const f64x2 *Wr = reinterpret_cast<const f64x2 *>(mine + lane * JLD);
    double W[WROW];
#pragma unroll
    for (int k = 0; k < WCH; ++k) { const f64x2 v = Wr[k]; W[2 * k] = v[0]; W[2 * k + 1] = v[1]; }
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int a = 0; a < 10; ++a)
        if (a < dc) { const double ya = y[a]; t0 += W[a] * ya; t1 += W[10 + a] * ya; t2 += W[20 + a] * ya; }
    d.tobs[3 * o] = t0; d.tobs[3 * o + 1] = t1; d.tobs[3 * o + 2] = t2;
}
__global__ void k_ba_backsub(BaDev d)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < d.n) d.stc[j] = -d.yc[j];
    if (j >= d.np) return;
    double tt[3] = {d.gps[3 * (size_t)j], d.gps[3 * (size_t)j + 1], d.gps[3 * (size_t)j + 2]};
    for (int o = d.pt_off[j]; o < d.pt_off[j + 1]; ++o) {
        tt[0] -= d.tobs[3 * (size_t)o]; tt[1] -= d.tobs[3 * (size_t)o + 1]; tt[2] -= d.tobs[3 * (size_t)o + 2];
    }
    const double *Vi = d.Vinv + 9 * (size_t)j;
    for (int a = 0; a < 3; ++a) d.stp[3 * (size_t)j + a] = -(Vi[3 * a] * tt[0] + Vi[3 * a + 1] * tt[1] + Vi[3 * a + 2] * tt[2]);
}

// model: sum_o m (r + m/2), m = Js step  (partial per block); observation rows staged through LDS like k_ba_eval writes them
__global__ __launch_bounds__(128) void k_ba_model(BaDev d, double *partial, Fin fin)
{
    __shared__ double sh[4];
    __shared__ __attribute__((aligned(16))) double stage[2 * 64 * JLD];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t row0 = (size_t)blockIdx.x * blockDim.x + 64 * w;
    const int nrows = (int)min((long long)64, (long long)d.no - (long long)row0);
    double *mine = stage + w * 64 * JLD;
    if (nrows > 0) rows_to_lds<JCH>(d.J, row0, nrows, mine, lane);
    __syncthreads();
    double acc = 0.0;
    if (lane < nrows) {
        const size_t o = row0 + lane;
        const int c = d.ocam[o], j = d.opt[o], off = d.cam_off[c], dc = d.cam_dim[c];
        const f64x2 *Jr = reinterpret_cast<const f64x2 *>(mine + lane * JLD);
        double row[JROW];
#pragma unroll
        for (int k = 0; k < JCH; ++k) { const f64x2 v = Jr[k]; row[2 * k] = v[0]; row[2 * k + 1] = v[1]; }
        double sc[10], sp[3];
#pragma unroll
        for (int k = 0; k < 10; ++k) sc[k] = k < dc ? d.sc[off + k] * d.stc[off + k] : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) sp[k] = d.sp[3 * (size_t)j + k] * d.stp[3 * (size_t)j + k];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            double m = 0.0;
#pragma unroll
            for (int k = 0; k < 10; ++k) if (k < dc) m += row[10 * i + k] * sc[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) m += row[20 + 3 * i + k] * sp[k];
            acc += m * (row[26 + i] + 0.5 * m);
        }
    }
    const double tot[1] = {block_sum(acc, sh)};
    finish_sums<1>(tot, partial, 0, fin, sh);
}

// delta = alpha * step .* scale ; candidate = clamp(x + delta) ; partials of |dx|^2, |x|^2,
// gradient.delta and the finite check.  which: 0 -> also writes dlc/dlp (alpha = 1 first time)
__global__ __launch_bounds__(256) void k_ba_plus(BaDev d, double alpha, double *partial, int nblocks, Fin fin)
{
    __shared__ double sh[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double dn = 0.0, xn = 0.0, g0 = 0.0, bad = 0.0;
    if (i < d.nc) {   // one thread per camera: 12 ambient parameters
        const int c = i, off = d.cam_off[c], dc = d.cam_dim[c];
        double ps[6], in[6];
        // |x| over the reduced program only, as Ceres' minimizer (x_norm_): a constant block (camera 0's pose, the
        // intrinsics when they are all held) or one no residual uses is not part of the state; a block with a
        // subset manifold counts with all six coordinates
        const bool used = d.cam_obs_off[c + 1] > d.cam_obs_off[c];
        const bool pose_in = used && dc > 0 && d.cols[10 * c] < 6, intr_in = used && d.mode == 1 && dc > 0;      // (dc == 0 in mode 1: a constant camera)
        for (int k = 0; k < 6; ++k) {
            ps[k] = d.poses[6 * c + k]; in[k] = d.intr[6 * c + k];
            if (pose_in) xn += ps[k] * ps[k];
            if (intr_in) xn += in[k] * in[k];
        }
        double ps2[6], in2[6];
        for (int k = 0; k < 6; ++k) { ps2[k] = ps[k]; in2[k] = in[k]; }
        // (every input of the loop below is loaded BEFORE its first store -- round 5: with the loads inside the loop the compiler had to
        //  keep each behind the store to dlc of the step before (the arrays may alias for all it knows), ten dependent round trips to L2
        //  in a kernel of a few hundred threads: 14 of its 16 us on the reference's problem sizes)
        double stc_[10], sc_[10], gcr_[10];
        int col_[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const bool on = k < dc;
            stc_[k] = on ? d.stc[off + k] : 0.0;
            sc_[k] = on ? d.sc[off + k] : 0.0;
            gcr_[k] = on ? d.gcraw[10 * (size_t)c + k] : 0.0;
            col_[k] = on ? d.cols[10 * c + k] : 0;
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            if (k >= dc) break;
            const double dl = alpha * stc_[k] * sc_[k];
            d.dlc[off + k] = dl;
            if (!isfinite(dl)) bad = 1.0;
            const int col = col_[k];
            // unscaled gradient of this coordinate = gcraw
            g0 += gcr_[k] * dl;
            if (col < 6) ps2[col] += dl;
            else {
                in2[col - 6] += dl;
                if (d.mode == 1 && col - 6 < 2 && in2[col - 6] > d.ub) in2[col - 6] = d.ub;
            }
        }
        for (int k = 0; k < 6; ++k) {
            d.poses2[6 * c + k] = ps2[k]; d.intr2[6 * c + k] = in2[k];
            dn += (ps2[k] - ps[k]) * (ps2[k] - ps[k]) + (in2[k] - in[k]) * (in2[k] - in[k]);
        }
        cam_rot_entry(ps2, d.crot2 + CROT * (size_t)c);
    }
    if (i < d.np) {
        const bool used = d.pt_off[i + 1] > d.pt_off[i];
        double stp_[3], sp_[3], x_[3], gp_[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { const size_t e = 3 * (size_t)i + k; stp_[k] = d.stp[e]; sp_[k] = d.sp[e]; x_[k] = d.pts[e]; gp_[k] = d.gpraw[e]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t e = 3 * (size_t)i + k;
            const double dl = alpha * stp_[k] * sp_[k];
            d.dlp[e] = dl;
            if (!isfinite(dl)) bad = 1.0;
            const double x = x_[k];
            g0 += gp_[k] * dl;
            d.pts2[e] = x + dl;
            dn += dl * dl;
            if (used) xn += x * x;
        }
    }
    double mine[4];
    mine[0] = block_sum(dn, sh); mine[1] = block_sum(xn, sh); mine[2] = block_sum(g0, sh); mine[3] = block_sum(bad, sh);
    finish_sums<4>(mine, partial, nblocks, fin, sh);
}

// projected gradient max-norm of the unscaled gradient (gcraw / gpraw); *out zeroed by the caller.
// max is order-independent and non-negative doubles order like their bit patterns, so one
// integer atomicMax per workgroup keeps the result deterministic.
// (with_diag: the clamped LM diagonal of k_ba_diag(what = 1) in the same launch -- after an accepted step both are due, from the same raw
//  blocks: one launch less per iteration, the same arithmetic)
__device__ __forceinline__ void ba_lm_diag_entry(const BaDev &d, int i, double lo, double hi)
{
    if (i < d.n) {
        int a = 0, b = d.nc - 1;
        while (a < b) { int m = (a + b + 1) >> 1; if (d.cam_off[m] <= i) a = m; else b = m - 1; }
        while (d.cam_dim[a] == 0 || d.cam_off[a] + d.cam_dim[a] <= i) ++a;
        const int k = i - d.cam_off[a];
        const double u = d.Uraw[100 * (size_t)a + 11 * k];
        d.dgc[i] = fmin(fmax(u * d.sc[i] * d.sc[i], lo), hi);
    }
    if (i < 3 * d.np) {
        const double v = d.Vraw[9 * (size_t)(i / 3) + 4 * (i % 3)];
        d.dgp[i] = fmin(fmax(v * d.sp[i] * d.sp[i], lo), hi);
    }
}
// (with_diag = 2, round 5: and the damped 3 x 3 blocks of k_ba_point_solve at trust-region radius 1 / inv_radius -- a landmark's three
//  diagonal entries and its block by ONE thread, so nothing crosses threads: the step that follows an accepted one loses a launch)
__global__ __launch_bounds__(256) void k_ba_gradmax(BaDev d, double *out, int with_diag = 0, double lo = 0.0, double hi = 0.0, double inv_radius = 0.0)
{
    __shared__ double sh[4];
    const int t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (with_diag == 2) {
        for (int i = t0; i < d.n; i += stride) ba_lm_diag_entry(d, i, lo, hi);          // (i < n <= 3 np is not given: the camera part on its own)
        for (int j = t0; j < d.np; j += stride) {
            for (int a = 0; a < 3; ++a) {
                const int i = 3 * j + a;
                const double v = d.Vraw[9 * (size_t)j + 4 * a];
                d.dgp[i] = fmin(fmax(v * d.sp[i] * d.sp[i], lo), hi);
            }
            point_solve_body(d, j, inv_radius);
        }
    }
    else if (with_diag)
        for (int i = t0; i < d.n || i < 3 * d.np; i += stride) ba_lm_diag_entry(d, i, lo, hi);
    double m = 0.0;
    for (int i = t0; i < d.nc; i += stride)
        for (int k = 0; k < d.cam_dim[i]; ++k) {
            double g = d.gcraw[10 * (size_t)i + k];
            const int col = d.cols[10 * i + k];
            if (d.mode == 1 && (col == 6 || col == 7)) {
                const double x = d.intr[6 * i + col - 6];
                double xn = x - g;
                if (xn > d.ub) xn = d.ub;
                g = x - xn;
            }
            m = fmax(m, fabs(g));
        }
    for (int i = t0; i < 3 * d.np; i += stride) m = fmax(m, fabs(d.gpraw[i]));
    for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_down(m, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
        atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(m));
    }
}

// =========================================================================================
// host side
// =========================================================================================
namespace {

struct Ws {   // growable device workspace out of ctx->ba_ws
    rcn_ctx *ctx;
    int next = 0;
    hipError_t err = hipSuccess;
    template <class T> T *get(size_t count)
    {
        if (next >= (int)(sizeof(ctx->ba_ws) / sizeof(ctx->ba_ws[0]))) { err = hipErrorOutOfMemory; return nullptr; }
        DevBuf &b = ctx->ba_ws[next++];
        hipError_t e = b.reserve(std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) err = e;
        return b.as<T>();
    }
};

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

extern "C" {

void rcn_ba_default_options(int32_t n_cams, rcn_ba_options *o)
{
    if (!o) return;
    o->max_iterations = n_cams < 10 ? 150 : 50;   // BundleAdjuster.cpp:135-142
    o->intrinsics_mode = n_cams < 10 ? 0 : 1;     // :112-121
    o->fix_cam0_pose = 1;                         // :100-101
    o->fix_cam1_translation = 1;                  // :104-105
    o->focal_upper_bound = 1000.0;                // :120-121
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->max_consecutive_invalid_steps = 5;
    o->jacobi_scaling = 1;
}

int rcn_ba_solve(rcn_ctx *ctx, const rcn_ba_problem *pb, const rcn_ba_options *opt, rcn_ba_summary *sum)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return rcn_int_ba_solve(ctx, pb, opt, sum, nullptr);
}

int rcn_ba_solve_robust(rcn_ctx *ctx, const rcn_ba_problem *pb, const rcn_ba_options *opt, const rcn_ba_loss *loss, rcn_ba_summary *sum,
                        rcn_ba_loss_report *report, double *weights_host)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return rcn_int_ba_solve(ctx, pb, opt, sum, nullptr, loss, report, weights_host);
}

int rcn_ba_solve_constant(rcn_ctx *ctx, const rcn_ba_problem *pb, const rcn_ba_options *opt, const rcn_ba_loss *loss, const uint8_t *cam_constant,
                          rcn_ba_summary *sum, rcn_ba_loss_report *report, double *weights_host)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return rcn_int_ba_solve(ctx, pb, opt, sum, nullptr, loss, report, weights_host, cam_constant);
}

int rcn_ba_solve_tied(rcn_ctx *ctx, const rcn_ba_problem *pb, const rcn_ba_options *opt, const rcn_ba_loss *loss, const uint8_t *cam_constant,
                      const int32_t *cam_group, rcn_ba_summary *sum, rcn_ba_loss_report *report, double *weights_host)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (pb && cam_group)
        for (int32_t c = 0; c < pb->n_cams; ++c)      // (below -1: the library's own mark for a held camera, not a caller's)
            if (cam_group[c] < -1) { ctx->set_error("rcn_ba_solve_tied: camera " + std::to_string(c) + ": group id " + std::to_string(cam_group[c]) + " is below -1"); return RCN_ERR_ARG; }
    return rcn_int_ba_solve(ctx, pb, opt, sum, nullptr, loss, report, weights_host, cam_constant, cam_group);
}

}  // extern "C"

// The loss as the kernels take it.  NULL: no loss, and a report counts nothing beyond the scale (b = inf).
int rcn_int_ba_loss_check(rcn_ctx *ctx, const rcn_ba_loss *loss, const char *who, int *kind, double *a, double *b)
{
    *kind = RCN_BA_LOSS_TRIVIAL; *a = *b = HUGE_VAL;
    if (!loss) return RCN_OK;
    if (loss->kind < RCN_BA_LOSS_TRIVIAL || loss->kind > RCN_BA_LOSS_CAUCHY) { ctx->set_error(std::string(who) + ": unknown loss kind"); return RCN_ERR_ARG; }
    if (!std::isfinite(loss->scale)) { ctx->set_error(std::string(who) + ": the loss's scale is not finite"); return RCN_ERR_ARG; }
    if (loss->kind != RCN_BA_LOSS_TRIVIAL && !(loss->scale > 0.0)) { ctx->set_error(std::string(who) + ": the loss's scale must be positive"); return RCN_ERR_ARG; }
    if (loss->kind == RCN_BA_LOSS_TRIVIAL) return RCN_OK;      // (its scale means nothing)
    *kind = loss->kind; *a = loss->scale; *b = loss->scale * loss->scale;
    return RCN_OK;
}

// rcn_ba_loss_report at one point (ctx->mu held): everything in HBM except the results.  One launch of k_ba_loss_report; its scratch
// (block partials, three scalars, the ticket, the weights) is ctx->ba_loss_ws, not the solver's workspace.
int rcn_int_ba_loss_report(rcn_ctx *ctx, int no, const double *poses_dev, const double *intr_dev, const double *pts_dev, const double *uv_dev,
                           const int *ocam_dev, const int *opt_dev, const rcn_ba_loss *loss, rcn_ba_loss_report *report, double *weights_host)
{
    BaLoss ls;
    { const int rc = rcn_int_ba_loss_check(ctx, loss, "rcn_ba_loss_report", &ls.kind, &ls.a, &ls.b); if (rc) return rc; }
    if (report) memset(report, 0, sizeof(*report));
    if (no <= 0 || (!report && !weights_host)) return RCN_OK;
    hipStream_t st = ctx->stream;
    const int nb = (no + 255) / 256;
    const size_t head = 2 * (size_t)nb + 8;      // partials [2][nb], then [0] count [1] sum s [2] max s, [4] the ticket word
    RCN_HIP(ctx->ba_loss_ws.reserve((head + (weights_host ? (size_t)no : 0)) * sizeof(double)));
    double *base = ctx->ba_loss_ws.as<double>(), *out = base + 2 * (size_t)nb, *w = weights_host ? base + head : nullptr;
    RCN_HIP(hipMemsetAsync(out, 0, 8 * sizeof(double), st));
    BaDev d;
    memset(&d, 0, sizeof(d));
    d.no = no; d.uv = uv_dev; d.ocam = ocam_dev; d.opt = opt_dev;
    const Fin f{out, nullptr, reinterpret_cast<unsigned *>(out + 4), nullptr, nullptr, nullptr, 1.0, nullptr, nullptr, 0ull};
    k_ba_loss_report<<<nb, 256, 0, st>>>(d, poses_dev, intr_dev, pts_dev, ls, w, base, f, out + 2);
    RCN_HIP(hipGetLastError());
    double h[3];
    RCN_HIP(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, st));
    if (w) RCN_HIP(hipMemcpyAsync(weights_host, w, sizeof(double) * (size_t)no, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipStreamSynchronize(st));
    if (report) {
        report->n_obs = no;
        report->n_beyond_scale = (int64_t)h[0];
        report->plain_rms_px = std::sqrt(h[1] / no);
        report->max_residual_px = std::sqrt(h[2]);
    }
    return RCN_OK;
}

// The solve proper (ctx->mu held).  res == nullptr: everything comes from / goes back to the host arrays of the
// problem.  res != nullptr (rcn_ba_session, ba_session.hip): the points and the observation arrays are already in HBM
// and stay there -- pb->points may be NULL, pb->obs_* are the session's host mirror (structure only) -- and the pair
// lists of the Schur build are reused when the token says the graph has not changed since they were built.
// loss != nullptr with a non-trivial kind: the two kernels that evaluate observations run in their robust form (k_ba_eval<JAC, true>,
// k_ba_dirgrad<true>); nothing else in the loop changes.  report / weights_host: one pass over the observations at the final point.
// cam_constant != nullptr (n_cams bytes): a camera with a non-zero byte has no tangent column at all (cam_dim = 0, in intrinsics mode 1
// too) -- its observations are residuals of the landmarks alone, its 12 numbers come back as they went in.  The kernels read the
// tables, so nothing but the tables (and the three places marked "constant camera" below) knows of it.
// cam_group != nullptr (n_cams words): cameras that share one set of intrinsics (ba_tied.h, ba_tied.hip).  The
// Schur build still makes the per-camera system; the factorisation reads its fold, and the step is expanded again behind it.
int rcn_int_ba_solve(rcn_ctx *ctx, const rcn_ba_problem *pb, const rcn_ba_options *opt, rcn_ba_summary *sum, const BaResident *res,
                     const rcn_ba_loss *loss, rcn_ba_loss_report *report, double *weights_host, const uint8_t *cam_constant, const int32_t *cam_group)
{
    if (!pb || !opt || !sum || pb->n_cams <= 0 || pb->n_points < 0 || pb->n_obs < 0 || !pb->poses ||
        !pb->intrinsics || (pb->n_points > 0 && !pb->points && !res) ||
        (pb->n_obs > 0 && (!pb->obs_uv || !pb->obs_cam || !pb->obs_pt))) {
        ctx->set_error("rcn_ba_solve: bad argument");
        return RCN_ERR_ARG;
    }
    BaLoss ls;
    { const int rcl = rcn_int_ba_loss_check(ctx, loss, "rcn_ba_solve_robust", &ls.kind, &ls.a, &ls.b); if (rcl) return rcl; }
    const bool robust = ls.kind != RCN_BA_LOSS_TRIVIAL;
    const int nc = pb->n_cams, np = pb->n_points, no = pb->n_obs;
    // shared intrinsics (ba_tied.h): `tied` is false without a live group or a held camera, and the solve is then
    // the one without groups -- the same tables, the same launches.  Everything tied below sits behind that flag.
    ba_tied::Plan tp;
    if (cam_group && ba_tied::build(nc, opt->intrinsics_mode, opt->fix_cam0_pose != 0, opt->fix_cam1_translation != 0, cam_constant, cam_group, nc,
                                    pb->intrinsics, tp, true)) {
        ctx->set_error("rcn_ba_solve_tied: " + tp.error);
        return RCN_ERR_ARG;
    }
    const bool tied = tp.tied;
    memset(sum, 0, sizeof(*sum));
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // ---- host-side structure (BundleAdjuster.cpp:99-129 constraints -> tangent columns)
    std::vector<int> pt_off(np + 1, 0), cam_off(nc + 1, 0), cam_dim(nc, 0), cols(10 * (size_t)nc, 0),
        cam_obs_off(nc + 1, 0), cam_obs(std::max(no, 1));
    for (int o = 0; o < no; ++o) {
        const int j = pb->obs_pt[o], c = pb->obs_cam[o];
        if (j < 0 || j >= np || c < 0 || c >= nc || (o && j < pb->obs_pt[o - 1])) {
            ctx->set_error("rcn_ba_solve: observations must be landmark-major with valid indices");
            return RCN_ERR_ARG;
        }
        pt_off[j + 1]++;
        cam_obs_off[c + 1]++;
    }
    for (int j = 0; j < np; ++j) pt_off[j + 1] += pt_off[j];
    for (int c = 0; c < nc; ++c) cam_obs_off[c + 1] += cam_obs_off[c];
    {
        std::vector<int> fill(nc, 0);
        for (int o = 0; o < no; ++o) { const int c = pb->obs_cam[o]; cam_obs[cam_obs_off[c] + fill[c]++] = o; }
    }
    int n = 0, kmax = 0;
    for (int j = 0; j < np; ++j) kmax = std::max(kmax, pt_off[j + 1] - pt_off[j]);
    for (int c = 0; c < nc; ++c) {
        int dcm = 0;
        const bool constant = cam_constant && cam_constant[c];      // constant camera: no column, whatever the options say
        if (!constant && !(c == 0 && opt->fix_cam0_pose)) {
            const int npose = (c == 1 && opt->fix_cam1_translation) ? 3 : 6;
            for (int k = 0; k < npose; ++k) cols[10 * c + dcm++] = k;
        }
        if (!constant && opt->intrinsics_mode == 1) { cols[10 * c + dcm++] = 6; cols[10 * c + dcm++] = 7; cols[10 * c + dcm++] = 10; cols[10 * c + dcm++] = 11; }
        cam_off[c] = n; cam_dim[c] = dcm; n += dcm;
    }
    cam_off[nc] = n;
    if (tied) { cam_off = tp.cam_off; cam_dim = tp.cam_dim; cols = tp.cols; n = tp.n; }      // (a held camera has lost its intrinsics columns)
    if (n == 0) { ctx->set_error("rcn_ba_solve: the reduced system has no free parameter (every camera is constant)"); return RCN_ERR_ARG; }
    const int npad = std::max(chol::BLOCK, (n + chol::BLOCK - 1) / chol::BLOCK * chol::BLOCK);
    // the system the factorisation reads: the per-camera one, or (tied) its fold
    const int n_f = tied ? tp.n_tied : n, npad_f = std::max(chol::BLOCK, (n_f + chol::BLOCK - 1) / chol::BLOCK * chol::BLOCK), nblk_f = npad_f / chol::BLOCK;
    sum->reduced_dim = n_f;

    // ---- device workspace
    Ws ws{ctx};
    BaDev d;
    memset(&d, 0, sizeof(d));
    d.nc = nc; d.np = np; d.no = no; d.n = n; d.npad = npad; d.mode = opt->intrinsics_mode; d.ub = opt->focal_upper_bound;
    d.poses = ws.get<double>(6 * (size_t)nc); d.intr = ws.get<double>(6 * (size_t)nc); d.pts = ws.get<double>(3 * (size_t)np);
    d.poses2 = ws.get<double>(6 * (size_t)nc); d.intr2 = ws.get<double>(6 * (size_t)nc); d.pts2 = ws.get<double>(3 * (size_t)np);
    double *uv = ws.get<double>(2 * (size_t)no);
    int *ints = ws.get<int>((size_t)no * 3 + np + 1 + 2 * (nc + 1) + nc + 10 * (size_t)nc + 24);      // + flag words [0..7], reduction tickets [8..11], the factorisation's counters [12..23]
    int *p_ocam = ints, *p_opt = p_ocam + no, *p_camobs = p_opt + no, *p_ptoff = p_camobs + no,
        *p_camobsoff = p_ptoff + np + 1, *p_camoff = p_camobsoff + nc + 1, *p_camdim = p_camoff + nc + 1,
        *p_cols = p_camdim + nc, *p_flag = p_cols + 10 * (size_t)nc;
    d.J = ws.get<double>(JROW * (size_t)no + 2); d.tobs = ws.get<double>(3 * (size_t)no);
    d.crot = ws.get<double>(CROT * (size_t)nc);
    d.crot2 = ws.get<double>(CROT * (size_t)nc);
    d.tickets = ws.get<unsigned>(2 * (size_t)std::max(nc, 1));
    d.Uraw = ws.get<double>(100 * (size_t)nc); d.gcraw = ws.get<double>(10 * (size_t)nc);
    d.Vraw = ws.get<double>(9 * (size_t)np); d.gpraw = ws.get<double>(3 * (size_t)np);
    const size_t nvec = (size_t)npad + 3 * (size_t)np + 16;
    double *vecs = ws.get<double>(12 * nvec);
    d.sc = vecs; d.sp = vecs + nvec; d.dgc = vecs + 2 * nvec; d.dgp = vecs + 3 * nvec;
    d.rhs = vecs + 4 * nvec; d.yc = vecs + 5 * nvec; d.stc = vecs + 6 * nvec; d.stp = vecs + 7 * nvec;
    d.dlc = vecs + 8 * nvec; d.dlp = vecs + 9 * nvec; d.gps = vecs + 10 * nvec;
    d.Vinv = ws.get<double>(9 * (size_t)np);
    d.S = ws.get<double>((size_t)npad * npad);
    d.L = ws.get<double>((size_t)npad * npad);
    const CholWs cws = rcn_chol_ws(ctx, nblk_f);
    d.Linv = ws.get<double>(cws.linv);
    double *SI = ws.get<double>(cws.si);      // a super-block's inverse (two-level regime of the factorisation)
    double *Sb = ws.get<double>(100 * (size_t)nc * nc);
    // gather lists of the Schur build (RCN_BA_SCHUR_ATOMICS=1 falls back to the atomic form)
    const bool gather = !ctx->ba_atomics;
    d.use_wy = 1;
    size_t npairs_lower = 0;
    for (int j = 0; j < np; ++j) { const size_t k = pt_off[j + 1] - pt_off[j]; npairs_lower += k * k; }   // upper bound
    const int nkeys = nc * nc;
    int *pk = ws.get<int>(gather ? 3 * (size_t)nkeys + 4 + (nkeys + 1023) / 1024 : 4);
    int *pk_cnt = pk, *pk_off = pk + nkeys + 1, *pk_fill = pk + 2 * nkeys + 2, *pk_sums = pk + 3 * (size_t)nkeys + 4;
    unsigned long long *pk_list = ws.get<unsigned long long>(gather ? std::max<size_t>(npairs_lower, 1) : 1);
    d.WY = ws.get<double>(2 * WROW * (size_t)std::max(no, 1));        // W and Y planes: the Schur gathers and the back-substitution read them
    // few cameras: split every camera over several workgroups so that the per-camera kernels fill the chip
    // (round 5: and only as far as a camera's observations call for it -- a workgroup of the camera kernels takes 256 observations per trip
    //  (k_ba_cam_raw) / 1024 (k_ba_schur_diag_mfma); splitting the reference's own problem sizes, a few hundred observations per camera,
    //  over 16 workgroups bought nothing and cost the ticket hand-off: 14 -> ~7 us per launch at 6 cameras)
    int max_cam_obs = 0;
    for (int c = 0; c < nc; ++c) max_cam_obs = std::max(max_cam_obs, cam_obs_off[c + 1] - cam_obs_off[c]);
    const int csplit = nc >= 128 ? 1 : std::max(1, std::min(std::min(16, 512 / std::max(nc, 1)), (max_cam_obs + 767) / 768));
    d.csplit = ws.get<double>((size_t)std::max(nc, 1) * csplit * 256);
    const int eb = (no + 255) / 256, ebj = (no + 127) / 128, pbk = (std::max(nc, np) + 255) / 256;
    d.partial = ws.get<double>(4 * (size_t)std::max(std::max(ebj, pbk), 1) + 16);
    d.scal = ws.get<double>(32);
    ba_tied::Dev T;
    memset(&T, 0, sizeof(T));
    double *yc2 = nullptr;
    int *tints = nullptr;
    const size_t tints_n = (size_t)nc + 2 * (size_t)n + (size_t)n_f + 1 + tp.grp_off.size() + tp.grp_cam.size();
    if (tied) {
        T.S2 = ws.get<double>((size_t)npad_f * npad_f);
        double *tv = ws.get<double>(4 * (size_t)n * tp.n_groups + 4 * (size_t)tp.n_groups + 2 * (size_t)npad_f + 16);
        T.C = tv; T.dgt = tv + 4 * (size_t)n * tp.n_groups; T.rhs2 = T.dgt + 4 * (size_t)tp.n_groups; yc2 = T.rhs2 + npad_f;
        tints = ws.get<int>(tints_n);
    }
    if (ws.err != hipSuccess) { ctx->set_error(std::string("rcn_ba_solve: workspace: ") + hipGetErrorString(ws.err)); return RCN_ERR_HIP; }
    d.uv = uv; d.ocam = p_ocam; d.opt = p_opt; d.cam_obs = p_camobs; d.pt_off = p_ptoff; d.cam_obs_off = p_camobsoff;
    d.cam_off = p_camoff; d.cam_dim = p_camdim; d.cols = p_cols; d.flag = p_flag;

    auto H2D = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    RCN_HIP(H2D(d.poses, pb->poses, sizeof(double) * 6 * nc));
    // TrustRegionMinimizer::IterationZero: start from the projection onto the box
    std::vector<double> intr0(pb->intrinsics, pb->intrinsics + 6 * (size_t)nc);
    if (opt->intrinsics_mode == 1)
        for (int c = 0; c < nc; ++c)
            for (int k = 0; k < 2; ++k)      // (cam_dim == 0 in mode 1: a constant camera, not part of the box)
                if ((tied ? tp.intr_free[c] != 0 : cam_dim[c] > 0) && intr0[6 * c + k] > opt->focal_upper_bound) {
                    intr0[6 * c + k] = opt->focal_upper_bound;
                    if (!tied || tp.grp[c] < 0 || tp.grp_cam[tp.grp_off[tp.grp[c]]] == c) sum->bound_projections++;      // (a tied focal length counts once)
                }
    RCN_HIP(H2D(d.intr, intr0.data(), sizeof(double) * 6 * nc));
    if (res) {
        if (np > 0) RCN_HIP(hipMemcpyAsync(d.pts, res->pts, sizeof(double) * 3 * np, hipMemcpyDeviceToDevice, st));
        uv = const_cast<double *>(res->uv); p_ocam = const_cast<int *>(res->ocam); p_opt = const_cast<int *>(res->opt);
        d.uv = uv; d.ocam = p_ocam; d.opt = p_opt;
    } else {
        RCN_HIP(H2D(d.pts, pb->points, sizeof(double) * 3 * np));
        RCN_HIP(H2D(uv, pb->obs_uv, sizeof(double) * 2 * no));
        RCN_HIP(H2D(p_ocam, pb->obs_cam, sizeof(int) * no));
        RCN_HIP(H2D(p_opt, pb->obs_pt, sizeof(int) * no));
    }
    {   // the six structure arrays lie back to back on the device (p_camobs .. p_cols): one copy instead of six
        std::vector<int> stage((size_t)(p_flag - p_camobs));
        int *o = stage.data();
        auto put = [&](const std::vector<int> &v, size_t cnt) { if (cnt) memcpy(o, v.data(), cnt * sizeof(int)); o += cnt; };
        put(cam_obs, (size_t)no); put(pt_off, (size_t)np + 1); put(cam_obs_off, (size_t)nc + 1); put(cam_off, (size_t)nc + 1); put(cam_dim, (size_t)nc); put(cols, 10 * (size_t)nc);
        RCN_HIP(H2D(p_camobs, stage.data(), stage.size() * sizeof(int)));
        if (tied) {      // the tied tables, back to back: grp, map, src_off, src, grp_off, grp_cam
            std::vector<int> ts;
            ts.reserve(tints_n);
            for (const std::vector<int> *v : {&tp.grp, &tp.map, &tp.src_off, &tp.src, &tp.grp_off, &tp.grp_cam}) ts.insert(ts.end(), v->begin(), v->end());
            RCN_HIP(H2D(tints, ts.data(), ts.size() * sizeof(int)));
            T.nc = nc; T.n = n; T.npad = npad; T.n_tied = n_f; T.npad_tied = npad_f; T.n_own = tp.n_own; T.n_groups = tp.n_groups;
            T.mode = opt->intrinsics_mode; T.ub = opt->focal_upper_bound;
            T.cam_off = p_camoff; T.cam_dim = p_camdim; T.cols = p_cols; T.cam_obs_off = p_camobsoff;
            T.grp = tints; T.map = T.grp + nc; T.src_off = T.map + n; T.src = T.src_off + n_f + 1; T.grp_off = T.src + n; T.grp_cam = T.grp_off + tp.grp_off.size();
            RCN_HIP(hipMemsetAsync(T.S2, 0, sizeof(double) * (size_t)npad_f * npad_f, st));      // upper part never rewritten
            RCN_HIP(hipStreamSynchronize(st));      // `ts` leaves scope
        }
        RCN_HIP(hipStreamSynchronize(st));      // `stage` leaves scope
    }
    RCN_HIP(hipMemsetAsync(p_flag, 0, 24 * sizeof(int), st));
    RCN_HIP(hipMemsetAsync(d.tickets, 0, 2 * (size_t)std::max(nc, 1) * sizeof(unsigned), st));
    RCN_HIP(hipMemsetAsync(vecs, 0, sizeof(double) * 12 * nvec, st));
    RCN_HIP(hipMemsetAsync(d.S, 0, sizeof(double) * (size_t)npad * npad, st));   // upper part / padding never rewritten
    RCN_HIP(hipMemsetAsync(d.Linv, 0, sizeof(double) * cws.linv, st));   // upper triangles of the tile inverses stay zero
    if (nblk_f > 2) RCN_HIP(hipMemsetAsync(SI, 0, sizeof(double) * cws.si, st));   // blocks above a super-block inverse's diagonal stay zero (a column-0 pass reads 64 columns of one)
    { int rcm = rcn_chol_prepare(ctx); if (!rcm) rcm = rcn_chol_plan(ctx, nblk_f); if (rcm) return rcm; }
    uint64_t plain_token = 0;
    if (!res && no > 0) {
        const bool same = ctx->ba_graph_nc == nc && ctx->ba_graph_np == np && ctx->ba_graph_cam.size() == (size_t)no &&
                          memcmp(ctx->ba_graph_cam.data(), pb->obs_cam, sizeof(int) * (size_t)no) == 0 &&
                          memcmp(ctx->ba_graph_pt.data(), pb->obs_pt, sizeof(int) * (size_t)no) == 0;
        if (!same) {
            ctx->ba_graph_cam.assign(pb->obs_cam, pb->obs_cam + no);
            ctx->ba_graph_pt.assign(pb->obs_pt, pb->obs_pt + no);
            ctx->ba_graph_nc = nc; ctx->ba_graph_np = np;
            ctx->ba_graph_serial++;
        }
        plain_token = (1ull << 63) | ctx->ba_graph_serial;      // (a session's token carries its id in the upper half: never this large)
    }
    RCN_HIP(hipStreamSynchronize(st));   // host vectors go out of use; timing starts with inputs resident
    const double t_start = now_s();        // the pair lists of the Schur build are part of the solve (only the pack is not)
    // Whose lists these are: a session names its graph version (res->pair_token); a plain rcn_ba_solve is recognised by its observation
    // graph itself -- the arrays of the last plain solve are kept on the host and compared element by element (no hash: nothing to
    // collide), outside the timed region like the validation loop above.  The reference's loop never solves one graph twice
    // (SequentialReconstructor.cpp:1040-1094 adds a view before every adjust); a caller that re-solves after changing only the
    // estimates (another start, other options) skips the 0.75 ms the lists cost at 1M observations.
    const uint64_t pair_token = res ? res->pair_token : plain_token;
    // (the lists also depend on WHICH cameras have no free parameter -- pair_key drops their pairs -- i.e. on the options: ADVICE r4.  The
    //  per-camera dimensions the lists were built for are kept beside the token and compared; a session's token does not cover options either)
    const bool pairs_cached = pair_token != 0 && ctx->ba_pair_token == pair_token && ctx->ba_pair_camdim == cam_dim;
    // The lists are built on the panel stream, BESIDE the first evaluation (which needs nothing of them; both are eight launches or so, and
    // on the reference's problem sizes a solve is a few hundred launch-bound microseconds): the ctx stream waits for them in front of the loop.
    const bool pairs_build = gather && np > 0 && !pairs_cached;
    // (queued BEHIND the first evaluation's launches, below: on these sizes the host's enqueue rate is what the device waits for, and the
    //  evaluation is what the host waits for first)
    // (what was launched, for the probe's record: 0 lists reused / nothing, 1 k_pair_small, 2 count, scan and fill; 1 k_ba_schur_mfma<4>, 2 the
    //  workgroup form; the gather depth of the diagonal kernel)
    int pair_path = 0, offdiag_kernel = 0, diag_smb = 0;
    BaProbe *const probe = ctx->ba_probe;
    auto grab = [&](auto &vec, const void *src, size_t count) -> hipError_t {      // (probe only; the stream has been synchronised)
        vec.resize(count);
        return count ? hipMemcpy(vec.data(), src, count * sizeof(vec[0]), hipMemcpyDeviceToHost) : hipSuccess;
    };
    auto build_pairs = [&]() -> int {
        hipStream_t sp = rcn_chol_idle_stream(ctx);          // the factorisation's panel stream, idle: the stream was synchronised above and every factorisation joins its streams
        int *const long_keys = pk_cnt, *const long_count = pk_fill + nkeys;      // (the counts are dead once the lists are filled; a spare word behind the fill cursors)
        if (ctx->ba_pair_small && nkeys <= 1024 && npairs_lower <= 16384) { k_pair_small<<<1, 1024, 0, sp>>>(d, pk_off, pk_list, nkeys, long_count); pair_path = 1; }      // (the smallest of the reference's own sizes: one launch for six; beyond, one workgroup walks the pairs slower than six launches)
        else {
            pair_path = 2;
            RCN_HIP(hipMemsetAsync(pk, 0, sizeof(int) * (3 * (size_t)nkeys + 4 + (nkeys + 1023) / 1024), sp));
            const int thr = std::min(256, std::max(64, (kmax * kmax + 63) / 64 * 64));
            k_pair_count<<<np, thr, 0, sp>>>(d, pk_cnt);
            const int nchunks = (nkeys + 1023) / 1024;
            k_scan_sums<<<nchunks, 1024, 0, sp>>>(pk_cnt, pk_sums, nkeys);
            k_scan_top<<<1, 1024, 0, sp>>>(pk_sums, nchunks, pk_off + nkeys);
            k_scan_apply<<<nchunks, 1024, 0, sp>>>(pk_cnt, pk_sums, pk_off, nkeys);
            k_pair_fill<<<np, thr, 0, sp>>>(d, pk_off, pk_fill, pk_list);
        }
        k_pair_sort<<<(nkeys + 127) / 128, 128, 0, sp>>>(pk_off, pk_list, nkeys, long_keys, long_count);
        k_pair_sort_long<<<std::min(nkeys, 2048), 256, 0, sp>>>(pk_off, pk_list, long_keys, long_count);
        RCN_HIP(hipGetLastError());
        RCN_HIP(hipEventRecord(ctx->ba_pair_ev, sp));
        return RCN_OK;
    };
    ctx->ba_pair_token = (gather && np > 0) ? pair_token : 0;
    if (!pairs_cached) ctx->ba_pair_camdim = cam_dim;
    sum->pair_lists_reused = pairs_cached ? 1 : 0;

    // phase times (summary.schur_seconds ...: HIP events on the stream) only where a phase outlasts the six event records of an
    // iteration: a 25-camera solve is ~35 launches of a few microseconds each, and every record is one more
    const bool phase_times = no >= 50000;
    double hs[32];
    // The cost at an ACCEPTED point (scal[0], written by the evaluation that also refreshes the Jacobian there) is not waited for: the
    // host needs it only when the next step's scalars come home, and every read below starts at scal[0] -- so it rides with whichever
    // read comes next (round 4, second session: one host round trip per iteration instead of two; the round trip and the idle stream
    // behind it are ~35 us, an eighth of an iteration of the reference's own problem sizes).
    double cost = 0.0;
    bool cost_pending = false;
    int cost_iter = 0;
    // (the pinned mirror serves the small problems, where the round trip is a quarter of an iteration; the large ones time their phases
    //  with events, which want the stream synchronised)
    double *const mirror = (!phase_times && no > 0) ? ctx->ba_host_scal : nullptr;
    auto read_scal = [&](int cnt, bool mirrored = false) -> hipError_t {
        hipError_t e = hipSuccess;
        if (mirrored && mirror) {
            const unsigned long long want = ctx->ba_host_seq;
            const unsigned long long *seqp = reinterpret_cast<const unsigned long long *>(mirror + 15);
            const double t0 = now_s();
            unsigned spins = 0;
            while (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) != want) {
                if ((++spins & 0x3FFu) == 0) {
                    if (hipStreamQuery(st) == hipSuccess) break;                 // the stream has drained: the store is there or will never come
                    if (now_s() - t0 > 10.0) break;
                }
            }
            if (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) == want) for (int i = 0; i < cnt; ++i) hs[i] = mirror[i];
            else {      // not expected: the ordinary way, which also reports what went wrong
                e = hipMemcpyAsync(hs, d.scal, sizeof(double) * cnt, hipMemcpyDeviceToHost, st);
                if (e == hipSuccess) e = hipStreamSynchronize(st);
            }
        } else {
            e = hipMemcpyAsync(hs, d.scal, sizeof(double) * cnt, hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) return e;
            e = hipStreamSynchronize(st);
        }
        if (e == hipSuccess && cost_pending) {
            cost = hs[0];
            if (cost_iter < 160) sum->cost_trace[cost_iter] = cost;
            cost_pending = false;
        }
        return e;
    };
    // cost at (poses,intr,pts) -> scal[slot]; JAC also refreshes the observation rows and the raw blocks
    bool jac_pending = false;
    // tickets of the in-kernel reductions (finish_sums): d.flag + 8 .. 11, zero at rest
    auto fin = [&](double *out, double scale, int which, bool with_flag, double *zero, double *out2 = nullptr, bool home = false) {
        Fin f{out, out2, reinterpret_cast<unsigned *>(d.flag + 8 + which), with_flag ? d.flag : nullptr, d.scal + 13, zero, scale, nullptr, d.scal, 0ull};
        if ((with_flag || home) && mirror) { f.host = mirror; f.seq = ++ctx->ba_host_seq; }      // the step's last reduction (the candidate's cost), the start's cost: the scalars go home by themselves
        return f;
    };
    auto eval = [&](bool jac, const double *ps, const double *in, const double *x, int slot, bool with_flag = false, bool rot_ready = false, bool home = false) -> hipError_t {
        if (no > 0) {
            if (jac) {
                // the streaming kernel of the solve, timed on its own (summary.jacobian_seconds): 224 B written per observation
                if (jac_pending && phase_times) {       // the previous pair of events has long completed (a read of the scalars came after it)
                    float ms = 0.f;
                    if (hipEventElapsedTime(&ms, ctx->ba_tev[4], ctx->ba_tev[5]) == hipSuccess) { sum->jacobian_seconds += 1e-3 * ms; sum->jacobian_evals++; }
                    else (void)hipGetLastError();
                }
                if (!rot_ready) k_ba_cam_rot<<<(nc + 127) / 128, 128, 0, st>>>(ps, nc, d.crot);      // (an accepted candidate brings its table: k_ba_plus)
                if (phase_times) (void)hipEventRecord(ctx->ba_tev[4], st);
                if (robust) k_ba_eval<true, true><<<ebj, 128, 0, st>>>(d, ps, in, x, d.partial, fin(d.scal + slot, 0.5, 0, false, d.scal + 12, nullptr, home), ls);
                else k_ba_eval<true><<<ebj, 128, 0, st>>>(d, ps, in, x, d.partial, fin(d.scal + slot, 0.5, 0, false, d.scal + 12, nullptr, home), ls);
                if (phase_times) (void)hipEventRecord(ctx->ba_tev[5], st);
                jac_pending = true;
            } else if (robust) k_ba_eval<false, true><<<eb, 256, 0, st>>>(d, ps, in, x, d.partial, fin(d.scal + slot, 0.5, 0, with_flag, nullptr), ls);
            else k_ba_eval<false><<<eb, 256, 0, st>>>(d, ps, in, x, d.partial, fin(d.scal + slot, 0.5, 0, with_flag, nullptr), ls);
        } else {
            k_finish_sum<<<1, 256, 0, st>>>(d.partial, 0, d.scal + slot, 0.5, with_flag ? d.flag : nullptr, d.scal + 13);      // no observations: the sums are zero
            if (jac) (void)hipMemsetAsync(d.scal + 12, 0, sizeof(double), st);
        }
        if (jac) {
            const int pblocks = (np + 128 * CR_GROUPS - 1) / (128 * CR_GROUPS);
            k_ba_cam_raw<<<nc * csplit + pblocks, 128 * CR_GROUPS, 0, st>>>(d, csplit, nc * csplit);
        }
        return hipGetLastError();
    };

    RCN_HIP(eval(true, d.poses, d.intr, d.pts, 0, false, false, true));      // (its cost goes home by itself)
    const int dgrid = (std::max(n, 3 * np) + 255) / 256;
    k_ba_diag<<<std::max(dgrid, 1), 256, 0, st>>>(d, 0, 0.0, 0.0, opt->jacobi_scaling);
    RCN_HIP(hipGetLastError());
    if (tied) RCN_HIP(rcn_tied_scale(T, d.Uraw, d.sc, opt->jacobi_scaling, st));      // tied: one scale per group column, from the members' summed diagonal
    if (pairs_build) { const int rcp = build_pairs(); if (rcp) return rcp; }
    RCN_HIP(read_scal(1, true));
    cost = hs[0];
    sum->initial_cost = cost;
    sum->initial_rms_px = std::sqrt(2.0 * cost / std::max(no, 1));
    sum->cost_trace[0] = cost;

    bool pairs_awaited = !pairs_build;      // (the first Schur build waits for the lists -- not the gradient, the landmark blocks and W / Y in front of it)
    double radius = opt->initial_trust_region_radius, decrease = 2.0;
    bool reuse_diag = false, need_gradient = true, grad_pending = false, diag_fresh = false, points_fresh = false;
    int invalid_run = 0, termination = 0, iter = 0;
    for (;;) {
        if (need_gradient) {
            // max |gradient| at the new point.  Its test comes BEFORE the next step in Ceres' loop; here the kernel is queued
            // and the value rides home with the scalars of the step that follows (one host synchronisation per iteration
            // instead of two: a quarter of a small problem's iteration).  If it was below the tolerance after all, that step
            // is dropped unseen -- it has only written candidate buffers -- and the loop ends where Ceres' would have.
            // (its cell, scal[12], was cleared by the evaluation at this point: k_ba_eval<true>, finish_sums)
            // (whenever the gradient is due, so is the LM diagonal -- an accepted step, or the start -- and both come from the raw blocks
            //  of the evaluation just queued: one launch; a loop that ends below has written a diagonal nobody reads)
            // (... and with the diagonal the landmarks' damped blocks at the radius the next step will use: k_ba_point_solve's launch)
            if (tied) {      // tied: the gradient of a group column is the members' sum; the diagonal and the landmark blocks by their plain launches below
                RCN_HIP(rcn_tied_gradmax(T, d.gcraw, d.gpraw, np, d.intr, d.scal + 12, st));
                diag_fresh = points_fresh = false;
            } else {
            k_ba_gradmax<<<std::max(1, std::min(1024, (std::max(std::max(nc, n), 3 * np) + 255) / 256)), 256, 0, st>>>(d, d.scal + 12, reuse_diag ? 0 : 2,
                                                                                                                     opt->min_lm_diagonal, opt->max_lm_diagonal, 1.0 / radius);
            RCN_HIP(hipGetLastError());
            diag_fresh = !reuse_diag;
            points_fresh = !reuse_diag;
            }
            need_gradient = false;
            grad_pending = true;
        }
        if (iter >= opt->max_iterations || radius <= opt->min_trust_region_radius) {
            // no step follows: the gradient test still comes first
            if (grad_pending) {
                RCN_HIP(read_scal(13));
                grad_pending = false;
                if (hs[12] <= opt->gradient_tolerance) { termination = RCN_BA_CONVERGENCE_GRADIENT; break; }
            }
            termination = iter >= opt->max_iterations ? RCN_BA_NO_CONVERGENCE : RCN_BA_CONVERGENCE_RADIUS;
            break;
        }
        ++iter;

        // ---- LM step
        if (!reuse_diag && !diag_fresh) {
            k_ba_diag<<<std::max(dgrid, 1), 256, 0, st>>>(d, 1, opt->min_lm_diagonal, opt->max_lm_diagonal, opt->jacobi_scaling);
            RCN_HIP(hipGetLastError());
            if (tied) RCN_HIP(rcn_tied_diag(T, d.Uraw, d.sc, d.dgc, opt->min_lm_diagonal, opt->max_lm_diagonal, st));      // tied: the clamp of the sum, added by the fold; the members' own entries zero
        }
        diag_fresh = false;
        const double ir = 1.0 / radius;
        if (phase_times) RCN_HIP(hipEventRecord(ctx->ba_tev[0], st));
        // [0] breakdown / gate flag, [2..7] progress counters of the factorisation's streams.  In the default form (gather Schur build, the
        // right-hand side as row n of the padded system) the flag words, the padded rows and the right-hand-side row are all written by
        // the Schur diagonal launch (its cameras' workgroups and the workgroups behind them), and nothing has to be cleared up front: the Schur kernels write every entry of rhs below n.
        // (tied: the Schur launches write the per-camera system, the factorisation reads its fold -- no fused shortcut, the plain launches)
        const bool rhs_row = npad_f > n_f && !ctx->ba_trsv_fwd;
        const bool fused_finish = gather && rhs_row && !tied;
        const bool chain = rcn_chol_bwd_one_launch(ctx, nblk_f);      // backward substitution as one launch
        BaDev dt = d;      // tied: the folded system as the plain finishing kernels take it
        if (tied) { dt.n = n_f; dt.npad = npad_f; dt.S = T.S2; dt.rhs = T.rhs2; dt.yc = yc2; }
        if (!fused_finish) {
            if (!gather) RCN_HIP(hipMemsetAsync(Sb, 0, sizeof(double) * 100 * (size_t)nc * nc, st));
            if (npad > n) RCN_HIP(hipMemsetAsync(d.S + (size_t)n * npad, 0, sizeof(double) * (size_t)(npad - n) * npad, st));
            RCN_HIP(hipMemsetAsync(d.rhs, 0, sizeof(double) * npad, st));
            if (tied) {
                if (npad_f > n_f) RCN_HIP(hipMemsetAsync(T.S2 + (size_t)n_f * npad_f, 0, sizeof(double) * (size_t)(npad_f - n_f) * npad_f, st));
                RCN_HIP(hipMemsetAsync(T.rhs2, 0, sizeof(double) * npad_f, st));
            }
        }
        if (np > 0 && !points_fresh) k_ba_point_solve<<<(np + 127) / 128, 128, 0, st>>>(d, ir);      // (a step behind an accepted one: done in k_ba_gradmax's launch)
        points_fresh = false;
        if (!fused_finish) k_ba_flag_reset<<<1, 64, 0, st>>>(d);      // (behind the landmark blocks, whichever launch solved them: it consumes their word)
        if (no > 0) k_ba_wy<<<(unsigned)((10 * (size_t)no + 255) / 256), 256, 0, st>>>(d);
        if (gather) {
            if (!pairs_awaited) { RCN_HIP(hipStreamWaitEvent(st, ctx->ba_pair_ev, 0)); pairs_awaited = true; }
            if (nc > 1) {
                const int nlow = nc * (nc - 1) / 2;
                if (npairs_lower / (size_t)nlow > 128) { k_ba_schur_mfma_wg<<<nlow, 512, 0, st>>>(d, pk_off, pk_list); offdiag_kernel = 2; }   // long lists: a workgroup per block
                else { k_ba_schur_mfma<4><<<(nlow + 3) / 4, 256, 0, st>>>(d, pk_off, pk_list); offdiag_kernel = 1; }
            }
            // (fused_finish: the padded rows, the right-hand-side row and the flag words ride in the same launch)
            const int fin = fused_finish ? (chain ? 1 : 0) : -1;
            const int fin_blocks = fused_finish ? (int)(((size_t)(npad - n) * npad + 1023) / 1024) : 0;
            if (nc < 128) { k_ba_schur_diag_mfma<12><<<nc * csplit + fin_blocks, 1024, 0, st>>>(d, pk_off, pk_list, ir, csplit, fin); diag_smb = 12; }      // (few cameras: latency-bound, deep gathers)
            else { k_ba_schur_diag_mfma<4><<<nc + fin_blocks, 1024, 0, st>>>(d, pk_off, pk_list, ir, 1, fin); diag_smb = 4; }
            if (!fused_finish && !tied && npad > n) k_ba_S_pad<<<(npad - n + 127) / 128, 128, 0, st>>>(d);
        } else {
            if (np > 0) k_ba_schur<<<np, std::min(256, std::max(64, 64 * ((kmax * kmax + 7) / 8))), 0, st>>>(d, Sb);
            k_ba_S_assemble<<<nc + 1, 256, 0, st>>>(d, Sb, ir);
            k_ba_cam_rhs<<<nc, 64, 0, st>>>(d);
        }
        if (tied) {
            // the fold: S' = P' S P with the groups' damping, b' = P' b; then padding and the right-hand-side row as for any system
            RCN_HIP(rcn_tied_fold(T, d.S, d.rhs, ir, st));
            if (npad_f > n_f) k_ba_S_pad<<<(npad_f - n_f + 127) / 128, 128, 0, st>>>(dt);
            if (rhs_row) k_ba_S_rhs_row<<<(n_f + 1 + 255) / 256, 256, 0, st>>>(dt);
        } else if (rhs_row && !fused_finish) k_ba_S_rhs_row<<<(n + 1 + 255) / 256, 256, 0, st>>>(d);
        RCN_HIP(hipGetLastError());
        if (phase_times) RCN_HIP(hipEventRecord(ctx->ba_tev[1], st));
        if (probe && iter == probe->iteration) {
            // capture A: everything the step has built stands in HBM; the factorisation below overwrites the reduced system
            BaProbe &q = *probe;
            RCN_HIP(hipStreamSynchronize(st));
            q.n = n; q.npad = npad; q.csplit = csplit; q.offdiag_kernel = offdiag_kernel; q.diag_smb = diag_smb; q.pair_path = pair_path;
            q.fin = (gather && fused_finish) ? (chain ? 1 : 0) : -1; q.rhs_row = rhs_row; q.fused_finish = fused_finish; q.chain = chain; q.radius = radius;
            RCN_HIP(grab(q.J, d.J, JROW * (size_t)no)); RCN_HIP(grab(q.crot, d.crot, CROT * (size_t)nc));
            RCN_HIP(grab(q.Uraw, d.Uraw, 100 * (size_t)nc)); RCN_HIP(grab(q.gcraw, d.gcraw, 10 * (size_t)nc));
            RCN_HIP(grab(q.Vraw, d.Vraw, 9 * (size_t)np)); RCN_HIP(grab(q.gpraw, d.gpraw, 3 * (size_t)np));
            RCN_HIP(grab(q.sc, d.sc, (size_t)n)); RCN_HIP(grab(q.sp, d.sp, 3 * (size_t)np));
            RCN_HIP(grab(q.dgc, d.dgc, (size_t)n)); RCN_HIP(grab(q.dgp, d.dgp, 3 * (size_t)np));
            RCN_HIP(grab(q.Vinv, d.Vinv, 9 * (size_t)np)); RCN_HIP(grab(q.gps, d.gps, 3 * (size_t)np));
            RCN_HIP(grab(q.WY, d.WY, 2 * WROW * (size_t)no));
            RCN_HIP(grab(q.S, d.S, (size_t)npad * npad)); RCN_HIP(grab(q.rhs, d.rhs, (size_t)npad));
            RCN_HIP(grab(q.flag, d.flag, 24)); RCN_HIP(grab(q.tickets, d.tickets, 2 * (size_t)nc));
            RCN_HIP(grab(q.cam_off, d.cam_off, (size_t)nc + 1)); RCN_HIP(grab(q.cam_dim, d.cam_dim, (size_t)nc)); RCN_HIP(grab(q.cols, d.cols, 10 * (size_t)nc));
            q.pk_off.clear(); q.pk_list.clear();
            if (gather && np > 0) {
                RCN_HIP(grab(q.pk_off, pk_off, (size_t)nkeys + 1));
                RCN_HIP(grab(q.pk_list, pk_list, std::min((size_t)std::max(q.pk_off[nkeys], 0), npairs_lower)));      // (never past the allocation, whatever the total says)
            }
            q.got_a = 1;
        }
        // Dense Cholesky of the padded system and the triangular solves behind it (chol.h).  A hand-off between its streams that times out raises flag 3, read
        // below with the step's scalars: the factorisation is then repeated on ONE stream, and every later one runs that way (ctx->chol.safe).  Same bits either way.
        const CholSystem sys = {dt.S, d.L, d.Linv, SI, d.flag, dt.rhs, dt.yc, n_f, npad_f, nblk_f, rhs_row, chain, fused_finish};
        // (up to two blocks there is no panel rest, no column rest and no bulk update: nothing for the other two streams to do)
        RCN_HIP(rcn_chol_factorise(ctx, sys, ctx->chol.safe || nblk_f <= 2));
        if (phase_times) RCN_HIP(hipEventRecord(ctx->ba_tev[2], st));
        // (rhs_row + chain, the default: the substitution reads y out of the factor's last row itself; k_ba_y_from_row remains for the
        //  per-step kernels and the other ways to build the system)
        if (rhs_row && !(chain && fused_finish)) k_ba_y_from_row<<<(npad_f + 255) / 256, 256, 0, st>>>(dt, chain ? 1 : 0);
        RCN_HIP(rcn_chol_substitute(ctx, sys));
        if (tied) RCN_HIP(rcn_tied_expand(T, T.rhs2, d.rhs, st));      // delta = P delta': every member carries its group's step
        {   // the solution sits in d.rhs: the two kernels that read it take it from there (round 3 copied it to d.yc first)
            BaDev dx = d;
            dx.yc = d.rhs;
            if (no > 0) k_ba_backsub_obs<<<ebj, 128, 0, st>>>(dx);
            k_ba_backsub<<<std::max((std::max(n, np) + 127) / 128, 1), 128, 0, st>>>(dx);
        }
        if (no > 0) k_ba_model<<<ebj, 128, 0, st>>>(d, d.partial, fin(d.scal + 2, -1.0, 1, false, nullptr));
        else k_finish_sum<<<1, 256, 0, st>>>(d.partial, 0, d.scal + 2, -1.0);
        // candidate at alpha = 1 (+ norms, gradient.delta, finite check) and its cost
        // scal: [3] |dx|^2  [4] |x|^2  [5] g.delta, also in [8]  [6] non-finite count, also in [9]
        k_ba_plus<<<pbk, 256, 0, st>>>(d, 1.0, d.partial, pbk, fin(d.scal + 3, 1.0, 2, false, nullptr, d.scal + 8));
        RCN_HIP(hipGetLastError());
        if (tied) RCN_HIP(rcn_tied_norms(T, d.intr, d.intr2, d.scal, st));      // |dx|, |x| with a tied parameter counted once
        RCN_HIP(eval(false, d.poses2, d.intr2, d.pts2, 1, true));       // + the factorisation's flag word into scal[13]
        if (phase_times) RCN_HIP(hipEventRecord(ctx->ba_tev[3], st));
        RCN_HIP(read_scal(14, true));
        const int hflag = (int)hs[13];
        if (grad_pending) {
            grad_pending = false;
            if (hs[12] <= opt->gradient_tolerance) {      // converged before this step: it does not count and is not looked at
                --iter;
                termination = RCN_BA_CONVERGENCE_GRADIENT;
                break;
            }
        }
        if (phase_times) {
            float ms = 0.f;
            RCN_HIP(hipEventElapsedTime(&ms, ctx->ba_tev[0], ctx->ba_tev[1])); sum->schur_seconds += 1e-3 * ms;
            RCN_HIP(hipEventElapsedTime(&ms, ctx->ba_tev[1], ctx->ba_tev[2])); sum->cholesky_seconds += 1e-3 * ms;
            RCN_HIP(hipEventElapsedTime(&ms, ctx->ba_tev[2], ctx->ba_tev[3])); sum->trisolve_seconds += 1e-3 * ms;
        }
        if (hflag == 4 && rcn_chol_bwd_gave_up(ctx)) {
            // the one-launch backward substitution gave up on a flag (its workgroups were not all resident): per-step kernels from now on
            --iter;
            reuse_diag = true;
            continue;
        }
        if (hflag == 3 && !ctx->chol.safe) {
            // a cross-stream wait of the factorisation gave up: this runtime does not run the three streams side by side.
            // Not a numerical failure: switch to the one-stream schedule for good and redo this iteration's linear solve.
            ctx->chol.safe = true;
            --iter;
            reuse_diag = true;       // the LM diagonal of this iteration is already in place
            continue;
        }
        reuse_diag = true;
        const double model_change = hs[2];
        const bool solve_ok = hflag == 0 && hs[9] == 0.0 && std::isfinite(model_change);
        // capture B (probe only): what the step has left behind its candidate's evaluation; the solve ends with it
        auto capture_b = [&](int how) -> int {
            BaProbe &q = *probe;
            RCN_HIP(hipStreamSynchronize(st));
            RCN_HIP(grab(q.x, d.rhs, (size_t)npad)); RCN_HIP(grab(q.tobs, d.tobs, 3 * (size_t)no));
            RCN_HIP(grab(q.stc, d.stc, (size_t)n)); RCN_HIP(grab(q.stp, d.stp, 3 * (size_t)np));
            RCN_HIP(grab(q.dlc, d.dlc, (size_t)n)); RCN_HIP(grab(q.dlp, d.dlp, 3 * (size_t)np));
            RCN_HIP(grab(q.poses2, d.poses2, 6 * (size_t)nc)); RCN_HIP(grab(q.intr2, d.intr2, 6 * (size_t)nc)); RCN_HIP(grab(q.pts2, d.pts2, 3 * (size_t)np));
            RCN_HIP(grab(q.crot2, d.crot2, CROT * (size_t)nc)); RCN_HIP(grab(q.scal, d.scal, 16));
            RCN_HIP(grab(q.flag_b, d.flag, 24)); RCN_HIP(grab(q.tickets_b, d.tickets, 2 * (size_t)nc));      // (at rest again: every ticket word zero)
            q.got_b = how;
            return RCN_OK;
        };
        if (probe) { probe->log.insert(probe->log.end(), hs, hs + 14); probe->log.push_back(0.0); }
        if (!solve_ok || !(model_change > 0.0)) {
            if (probe && iter == probe->iteration) { const int rcb = capture_b(2); if (rcb) return rcb; termination = RCN_BA_NO_CONVERGENCE; break; }
            sum->invalid_steps++;
            if (++invalid_run >= opt->max_consecutive_invalid_steps) { termination = RCN_BA_FAILURE; break; }      // Ceres' HandleInvalidStep: pre-increment, `>=` (see the oracle)
            radius /= decrease; decrease *= 2.0; reuse_diag = false;
            if (iter < 160) sum->cost_trace[iter] = cost;
            continue;
        }
        invalid_run = 0;
        double cand_cost = hs[1], dn2 = hs[3], xn2 = hs[4];
        if (opt->intrinsics_mode == 1) {
            // bounds present: ArmijoLineSearch::DoSearch along delta, first trial the full step (already evaluated).
            // A trial that fails the sufficient-decrease test also gets its directional derivative
            // (k_ba_dirgrad against d.dlc / d.dlp = a * delta, hence the division by a).
            const double g0 = hs[8];
            rcn_ls::Sample start, prev, cur;
            start.x = 0.0; start.v = cost; start.g = g0; start.v_ok = start.g_ok = true;
            double a = 1.0, dmax = -1.0;
            int bt = 0;
            bool found = false;
            auto trial = [&](double alpha) -> hipError_t {   // candidate, its cost and the step norms at alpha
                k_ba_plus<<<pbk, 256, 0, st>>>(d, alpha, d.partial, pbk, fin(d.scal + 3, 1.0, 2, false, nullptr, d.scal + 14));      // ([14], [15]: nobody reads them here)
                if (tied) { const hipError_t et = rcn_tied_norms(T, d.intr, d.intr2, d.scal, st); if (et != hipSuccess) return et; }
                hipError_t e = eval(false, d.poses2, d.intr2, d.pts2, 1);
                if (e != hipSuccess) return e;
                e = read_scal(5);
                cand_cost = hs[1]; dn2 = hs[3]; xn2 = hs[4];
                return e;
            };
            for (int it = 0;;) {
                cur = rcn_ls::Sample();
                cur.x = a; cur.v = cand_cost; cur.v_ok = std::isfinite(cand_cost);
                if (cur.v_ok && cur.v <= cost + 1e-4 * g0 * a) {
                    if (probe && iter == probe->iteration) probe->trials.insert(probe->trials.end(), {a, cand_cost, std::nan(""), dmax});
                    found = true;
                    break;
                }
                if (cur.v_ok) {
                    if (no > 0 && robust) k_ba_dirgrad<true><<<eb, 256, 0, st>>>(d, d.poses2, d.intr2, d.pts2, d.partial, ls);
                    else if (no > 0) k_ba_dirgrad<false><<<eb, 256, 0, st>>>(d, d.poses2, d.intr2, d.pts2, d.partial, ls);
                    k_finish_sum<<<1, 256, 0, st>>>(d.partial, no > 0 ? eb : 0, d.scal + 10, 1.0);
                }
                if (dmax < 0.0) {                    // |delta|_inf, once per search (the first trial is a = 1)
                    RCN_HIP(hipMemsetAsync(d.scal + 11, 0, sizeof(double), st));
                    k_ba_absmax<<<std::max(1, std::min(1024, (std::max(n, 3 * np) + 255) / 256)), 256, 0, st>>>(
                        d.dlc, (size_t)n, d.dlp, 3 * (size_t)np, d.scal + 11);
                }
                RCN_HIP(hipGetLastError());
                RCN_HIP(read_scal(12));
                if (cur.v_ok) { cur.g = hs[10] / a; cur.g_ok = std::isfinite(cur.g); }
                if (dmax < 0.0) dmax = hs[11] / a;
                if (probe && iter == probe->iteration) probe->trials.insert(probe->trials.end(), {a, cand_cost, cur.g_ok ? cur.g : std::nan(""), dmax});
                if (++it >= 20) break;
                const double an = rcn_ls::next_step(start, prev, cur, 1e-3 * a, 0.6 * a);
                if (an * dmax < 1e-9) break;
                prev = cur;
                a = an;
                sum->line_search_backtracks++;
                ++bt;
                RCN_HIP(trial(a));
            }
            if (!found && bt) RCN_HIP(trial(1.0));   // the search gave up: the full step stands
            if (probe) probe->log.back() = (double)bt;
        }
        if (probe && iter == probe->iteration) { const int rcb = capture_b(1); if (rcb) return rcb; termination = RCN_BA_NO_CONVERGENCE; break; }
        if (!std::isfinite(cand_cost)) cand_cost = DBL_MAX;
        if (std::sqrt(dn2) <= opt->parameter_tolerance * (std::sqrt(xn2) + opt->parameter_tolerance)) {
            termination = RCN_BA_CONVERGENCE_PARAMETER;
            if (iter < 160) sum->cost_trace[iter] = cost;
            break;
        }
        const double cost_change = cost - cand_cost;
        if (std::fabs(cost_change) <= opt->function_tolerance * cost) {
            termination = RCN_BA_CONVERGENCE_FUNCTION;
            if (iter < 160) sum->cost_trace[iter] = cost;
            break;
        }
        const double rho = cost_change / model_change;
        if (rho > opt->min_relative_decrease) {
            std::swap(d.poses, d.poses2); std::swap(d.intr, d.intr2); std::swap(d.pts, d.pts2); std::swap(d.crot, d.crot2);
            RCN_HIP(eval(true, d.poses, d.intr, d.pts, 0, false, true));
            cost_pending = true;          // cost = scal[0] at the next read (read_scal, above)
            cost_iter = iter;
            need_gradient = true;
            sum->successful_steps++;
            const double t = 2.0 * rho - 1.0;
            radius = radius / std::max(1.0 / 3.0, 1.0 - t * t * t);
            radius = std::min(opt->max_trust_region_radius, radius);
            decrease = 2.0; reuse_diag = false;
        } else {
            sum->unsuccessful_steps++;
            radius /= decrease; decrease *= 2.0; reuse_diag = true;
        }
        if (iter < 160 && !cost_pending) sum->cost_trace[iter] = cost;
    }
    if (cost_pending) RCN_HIP(read_scal(1));       // (every exit of the loop has read the scalars since the last accepted step: not reached)
    if (!pairs_awaited) RCN_HIP(hipStreamWaitEvent(st, ctx->ba_pair_ev, 0));      // (a solve that ended before its first step: the lists it queued are kept for the next one)
    RCN_HIP(hipStreamSynchronize(st));
    sum->solve_seconds = now_s() - t_start;
    if (jac_pending && phase_times) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ba_tev[4], ctx->ba_tev[5]) == hipSuccess) { sum->jacobian_seconds += 1e-3 * ms; sum->jacobian_evals++; }
        else (void)hipGetLastError();
    }
    sum->iterations = iter;
    sum->factor_schedule = ctx->chol.safe ? 1 : 0;
    sum->termination = termination;
    sum->final_cost = cost;
    sum->final_rms_px = std::sqrt(2.0 * cost / std::max(no, 1));
    RCN_HIP(hipMemcpyAsync(pb->poses, d.poses, sizeof(double) * 6 * nc, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(pb->intrinsics, d.intr, sizeof(double) * 6 * nc, hipMemcpyDeviceToHost, st));
    if (np > 0) {
        if (res) RCN_HIP(hipMemcpyAsync(res->pts, d.pts, sizeof(double) * 3 * np, hipMemcpyDeviceToDevice, st));
        else RCN_HIP(hipMemcpyAsync(pb->points, d.pts, sizeof(double) * 3 * np, hipMemcpyDeviceToHost, st));
    }
    RCN_HIP(hipStreamSynchronize(st));
    if (report || weights_host) {
        const int rcr = rcn_int_ba_loss_report(ctx, no, d.poses, d.intr, d.pts, d.uv, d.ocam, d.opt, loss, report, weights_host);
        if (rcr) return rcr;
    }
    return termination == RCN_BA_FAILURE ? RCN_ERR_NUMERIC : RCN_OK;
}
