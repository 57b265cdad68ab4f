// mvs_geom.h -- the arithmetic of the plane sweep, one text for the GPU kernels (mvs.hip), for the host entry
// rcn_mvs_homographies and for plain host C++ (tests/cpp/mvs_host_test.cpp).  No HIP header is needed: without a HIP compiler the
// qualifiers vanish.  tests/mvs_ref.py states the same steps in numpy; the two must agree bit for bit.
//
// Every floating-point step is one separately rounded IEEE double in the order written here (contraction off); every sum over a window is
// an integer sum, exact in any order.  Cameras: P = 12 doubles, the rows of [R | t] (world -> camera); K = fx fy cx cy (k1 k2 follow in
// the session's rows of six and are not read here: the sweep is pinhole, the undistortion resample removes them beforehand).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MG_FN __host__ __device__ inline
#else
#define MG_FN inline
#endif

// Contraction off inside every function below.  clang (hipcc, device and host) takes the pragma; for g++ the including file says
// -ffp-contract=off or "#pragma GCC optimize" (tests/test_mvs_host.py, tests/cpp/mvs_adapter_test.cpp).
#if defined(__clang__)
#define MG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MG_NO_CONTRACT
#endif

#define MG_SUB 32                    // sub-pixel positions per pixel: samples sit on a 1/32 grid, the blend has 5-bit weights
#define MG_RMAX 5                    // largest window radius: n = 121, every sum below 2^53

// H = K_s (R_rel + t_rel e3^T inv) K_r^-1, row-major, R_rel = R_s R_r^T, t_rel = t_s - R_rel t_r; K_r^-1 in closed form.
MG_FN void mg_homography(const double *Pr, const double *Kr, const double *Ps, const double *Ks, double inv, double *H)
{
    MG_NO_CONTRACT
    double M[3][3];
    for (int i = 0; i < 3; ++i) {
        double Rrel[3];
        for (int j = 0; j < 3; ++j) Rrel[j] = (Ps[4 * i] * Pr[4 * j] + Ps[4 * i + 1] * Pr[4 * j + 1]) + Ps[4 * i + 2] * Pr[4 * j + 2];
        const double trel = Ps[4 * i + 3] - ((Rrel[0] * Pr[3] + Rrel[1] * Pr[7]) + Rrel[2] * Pr[11]);
        M[i][0] = Rrel[0];
        M[i][1] = Rrel[1];
        M[i][2] = Rrel[2] + trel * inv;
    }
    for (int j = 0; j < 3; ++j) {
        const double g0 = Ks[0] * M[0][j] + Ks[2] * M[2][j];
        const double g1 = Ks[1] * M[1][j] + Ks[3] * M[2][j];
        M[0][j] = g0;
        M[1][j] = g1;
    }
    for (int i = 0; i < 3; ++i) {
        H[3 * i] = M[i][0] / Kr[0];
        H[3 * i + 1] = M[i][1] / Kr[1];
        H[3 * i + 2] = (M[i][2] - (M[i][0] * Kr[2]) / Kr[0]) - (M[i][1] * Kr[3]) / Kr[1];
    }
}

// (u, v) -> the 1/32-pixel position (qu, qv); false outside 0 .. 32 (cols - 1) x 0 .. 32 (rows - 1) (a NaN is outside)
MG_FN bool mg_quantise(double u, double v, int rows, int cols, int *qu, int *qv)
{
    MG_NO_CONTRACT
    const double fu = floor(u * (double)MG_SUB + 0.5), fv = floor(v * (double)MG_SUB + 0.5);
    if (!(fu >= 0.0 && fu <= (double)(MG_SUB * (cols - 1)) && fv >= 0.0 && fv <= (double)(MG_SUB * (rows - 1)))) return false;
    *qu = (int)fu;
    *qv = (int)fv;
    return true;
}

// the sample position of reference pixel (x, y) in the source image behind H
MG_FN bool mg_warp(const double *H, int x, int y, int rows, int cols, int *qu, int *qv)
{
    MG_NO_CONTRACT
    const double fx = (double)x, fy = (double)y;
    const double w = (H[6] * fx + H[7] * fy) + H[8];
    if (!(w > 0.0)) return false;
    const double u = ((H[0] * fx + H[1] * fy) + H[2]) / w;
    const double v = ((H[3] * fx + H[4] * fy) + H[5]) / w;
    return mg_quantise(u, v, rows, cols, qu, qv);
}

// the integer bilinear blend at (qu, qv) of one channel: 0 .. 255 * 1024, the right / lower neighbour clamped to the last column / row
MG_FN int mg_sample(const uint8_t *img, int64_t stride_row, int64_t stride_px, int rows, int cols, int qu, int qv)
{
    const int x0 = qu >> 5, y0 = qv >> 5, wx = qu & 31, wy = qv & 31;
    const int x1 = x0 + 1 < cols ? x0 + 1 : cols - 1, y1 = y0 + 1 < rows ? y0 + 1 : rows - 1;
    const uint8_t *r0 = img + (int64_t)y0 * stride_row, *r1 = img + (int64_t)y1 * stride_row;
    const int top = (MG_SUB - wx) * (int)r0[x0 * stride_px] + wx * (int)r0[x1 * stride_px];
    const int bot = (MG_SUB - wx) * (int)r1[x0 * stride_px] + wx * (int)r1[x1 * stride_px];
    return (MG_SUB - wy) * top + wy * bot;
}

// the ZNCC cost of one source from the window's integer sums; Va = n Saa - Sa^2 > 0 is the caller's (it is the reference's alone)
MG_FN bool mg_cost(int n, int64_t Sa, int64_t Va, int64_t Sb, int64_t Sbb, int64_t Sab, double *cost)
{
    MG_NO_CONTRACT
    const int64_t Vb = (int64_t)n * Sbb - Sb * Sb;
    if (Vb <= 0) return false;
    const int64_t A = (int64_t)n * Sab - Sa * Sb;
    *cost = 1.0 - (double)A / sqrt((double)Va * (double)Vb);
    return true;
}

// the refined inverse depth: a parabola through the costs at k - 1, k, k + 1.  have_m / have_p: the neighbour exists and its cost is finite.
MG_FN double mg_refine(double cm, double c0, double cp, bool have_m, bool have_p, double inv_m, double inv_0, double inv_p)
{
    MG_NO_CONTRACT
    if (!(have_m && have_p)) return inv_0;
    const double den = (cm - 2.0 * c0) + cp;
    if (!(den > 0.0)) return inv_0;
    double off = (0.5 * (cm - cp)) / den;
    off = off > 0.5 ? 0.5 : (off < -0.5 ? -0.5 : off);
    if (off > 0.0) return inv_0 + off * (inv_p - inv_0);
    if (off < 0.0) return inv_0 + off * (inv_0 - inv_m);
    return inv_0;
}

// pixel (x, y) at camera-frame depth z -> the world point R^T (X_cam - t)
MG_FN void mg_lift(const double *P, const double *K, int x, int y, double z, double *Xw)
{
    MG_NO_CONTRACT
    const double d0 = (((double)x - K[2]) / K[0]) * z - P[3];
    const double d1 = (((double)y - K[3]) / K[1]) * z - P[7];
    const double d2 = z - P[11];
    for (int i = 0; i < 3; ++i) Xw[i] = (P[i] * d0 + P[4 + i] * d1) + P[8 + i] * d2;
}

// reproj_l1's projection (camgeom.h) without its distortion lines; *z the camera-frame depth.  The caller tests z > 0 first.
MG_FN void mg_project(const double *P, const double *K, const double *X, double *u, double *v, double *z)
{
    MG_NO_CONTRACT
    double l[3];
    for (int i = 0; i < 3; ++i) l[i] = ((P[4 * i] * X[0] + P[4 * i + 1] * X[1]) + P[4 * i + 2] * X[2]) + P[4 * i + 3];
    *u = K[0] * (l[0] / l[2]) + K[2];
    *v = K[1] * (l[1] / l[2]) + K[3];
    *z = l[2];
}

// the undistortion resample's source position of output pixel (x, y): the reference's additive model as reproj_l1 states it
MG_FN void mg_distort(const double *K6, int x, int y, double *u, double *v)
{
    MG_NO_CONTRACT
    const double xn = ((double)x - K6[2]) / K6[0], yn = ((double)y - K6[3]) / K6[1];
    const double rho = xn * xn + yn * yn;
    const double d = K6[4] * rho + (K6[5] * rho) * rho;
    *u = K6[0] * (xn + d) + K6[2];
    *v = K6[1] * (yn + d) + K6[3];
}

// inv[k] of the uniform-in-inverse-depth list over [near, far], ascending inverse depth from 1 / far; D == 1: the middle
MG_FN double mg_inv_depth(double near_z, double far_z, int k, int D)
{
    MG_NO_CONTRACT
    const double lo = 1.0 / far_z, hi = 1.0 / near_z;
    const double t = D > 1 ? (double)k / (double)(D - 1) : 0.5;
    return lo + (hi - lo) * t;
}

// rcn_mvs_inv_depths's body: false on a bad argument
MG_FN bool mg_inv_depths(double near_z, double far_z, int D, int max_planes, double *inv_out)
{
    if (!inv_out || D < 1 || D > max_planes || !(near_z > 0.0) || !(far_z >= near_z) || !(far_z < INFINITY)) return false;
    for (int k = 0; k < D; ++k) inv_out[k] = mg_inv_depth(near_z, far_z, k, D);
    return true;
}

// rcn_mvs_homographies's body: H_out [S][D][9], zeros for a source < 0; false on a bad argument (a reference among its sources included)
MG_FN bool mg_homographies(const double *poses34, const double *intrinsics, int ref, const int32_t *srcs, int S, const double *inv, int D, int max_sources,
                           int max_planes, double *H_out)
{
    if (!poses34 || !intrinsics || !srcs || !inv || !H_out || ref < 0 || S < 1 || S > max_sources || D < 1 || D > max_planes) return false;
    for (int s = 0; s < S; ++s)
        if (srcs[s] == ref) return false;
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < D; ++k) {
            double *H = H_out + ((int64_t)s * D + k) * 9;
            if (srcs[s] < 0) { for (int i = 0; i < 9; ++i) H[i] = 0.0; continue; }
            mg_homography(poses34 + 12 * (int64_t)ref, intrinsics + 6 * (int64_t)ref, poses34 + 12 * (int64_t)srcs[s], intrinsics + 6 * (int64_t)srcs[s], inv[k], H);
        }
    return true;
}
