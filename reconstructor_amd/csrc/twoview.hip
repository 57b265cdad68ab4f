// twoview.hip -- two-view initialisation behind rcn_twoview_init (include/rcn.h): batched 5-point RANSAC and pose recovery.
// gfx950, fp64.
//
// SequentialReconstructor::chooseInitialPair (SequentialReconstructor.cpp:325-375), i.e. cv::findEssentialMat in its
// two-camera form followed by cv::recoverPose, for a batch of pairs in one launch:
//
//   k_tv_pair   one workgroup of 256 threads per pair runs the pair's whole search:
//        gather   every entry's two pixels -> normalised coordinates (x1, y1, x2, y2), kept in LDS while they fit (TV_NLDS
//                 entries of 32 bytes) and in the pair's slice of the workspace otherwise
//        rounds of TV_B samples
//          draw     one lane replays the sequential cv::RNG index stream (5 distinct indices per sample)
//          solve    one lane per sample: null space of the 5 x 9 design matrix (Gauss-Jordan, complete pivoting), the
//                   10 x 20 constraint matrix, its elimination (partial pivoting), the degree-10 polynomial in z, its real
//                   roots through the derivative chain (bisection + guarded Newton), up to ten E per sample, each polished
//                   by Gauss-Newton steps against the constraints of E itself.  The lane's
//                   matrices live element-major in LDS (TV_LANE_D doubles per lane): every data-dependent index is an LDS
//                   address, never a register array
//          score    one wave per sample, its models in solver order, lanes over the entries; a model is dropped once
//                   good + remaining <= bound, bound counting earlier rounds and the wave's own earlier models of this
//                   round: the outcome is the sequential loop's (exact pruning, as k_pnp_view)
//          accept   one lane replays the acceptance rule in iteration order and discards what lies behind the stop
//        mask     the best model's inliers
//        pose     E -> t, R1, R2 in closed form (every thread, the same bits), four candidates x entries over the
//                 workgroup, ballot counts per wave added in wave order, OpenCV's >= cascade, the winner's mask
//
// Every operation is a separately rounded IEEE double (contraction off) in one fixed order built from + - * / sqrt;
// tests/twoview_ref.py restates that order and agrees bit for bit.  The one exception is pow / log in update_num_iters.
// The result depends neither on TV_B nor on the launch geometry.
//
// rng_next, update_num_iters and finite_d are ransac.h's, shared with the other two searches.
#include "rcn_internal.h"
#include "ransac.h"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int TV_BLOCK = 256;         // 4 waves
constexpr int TV_B = 32;              // samples per round
constexpr int TV_MAXM = 10;           // models per sample
constexpr int TV_NLDS = 2048;         // entries kept in LDS (32 bytes each)
constexpr int TV_LANE_D = 240;        // doubles of LDS per solving lane: 200 of the 10 x 20 matrix, 36 of the null space
constexpr int TV_BASIS = 200;
constexpr int TV_BISECT = 40, TV_NEWTON = 4, TV_POLISH = 3;
// the lane's area behind the elimination: derivative chain (level d at (d - 1)(d + 2) / 2, d + 1 coefficients), two root
// lists, p1, p2, p3
constexpr int TV_ROOTS0 = 65, TV_ROOTS1 = 75, TV_P1 = 85, TV_P2 = 93, TV_P3 = 101;
constexpr size_t TV_LDS_BYTES = 8 * ((size_t)TV_LANE_D * TV_B + (size_t)TV_B * TV_MAXM * 9 + 4 * (size_t)TV_NLDS);

struct TvArgs {
    const int64_t *off;
    const int32_t *xy1, *xy2;   // pixels of every entry
    const double *intr1, *intr2;
    double *norm;               // workspace: 4 doubles per entry
    double thr, conf, dist;
    int32_t max_iters;
    double *E, *pose;
    uint8_t *mask, *cmask;
    int32_t *count, *iters;
};

// Camera.h:79-93 unprojection of the pixel, scaled back by the mean camera matrix Km and normalised by it again
__device__ __forceinline__ void normalise(const double *K, const double *Km, int32_t ou, int32_t ov, double *x_out, double *y_out)
{
#pragma clang fp contract(off)
    double x = ((double)ou - K[2]) / K[0];
    double y = ((double)ov - K[3]) / K[1];
    const double radius = x * x + y * y;
    const double d = K[4] * radius + (K[5] * radius) * radius;
    x = x - d;
    y = y - d;
    const double pu = Km[0] * x + Km[2], pv = Km[1] * y + Km[3];
    *x_out = (pu - Km[2]) / Km[0];
    *y_out = (pv - Km[3]) / Km[1];
}

// monomial tables (tests/twoview_ref.py MONO1 / MONO2 / MONO3): product of a degree <= 1 monomial (x, y, z, 1) with a
// degree <= 1 one -> index among the ten of degree <= 2, with a degree <= 2 one -> index among the twenty of degree <= 3.
// Called with constants after unrolling.
__device__ constexpr int m12(int i, int j)
{
    constexpr int T[4][4] = {{0, 1, 2, 6}, {1, 3, 4, 7}, {2, 4, 5, 8}, {6, 7, 8, 9}};
    return T[i][j];
}
__device__ constexpr int m23(int i, int j)
{
    constexpr int T[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {3, 1, 6, 7}, {8, 6, 13, 14}, {10, 13, 16, 17},
                              {5, 9, 11, 12}, {9, 7, 14, 15}, {11, 14, 17, 18}, {12, 15, 18, 19}};
    return T[i][j];
}

__device__ __forceinline__ void mul11(const double *a, const double *b, double *out)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 0; m < 10; ++m) out[m] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[m12(i, j)] = out[m12(i, j)] + a[i] * b[j];
}

__device__ __forceinline__ void mul21(const double *a, const double *b, double *out)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 0; m < 20; ++m) out[m] = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[m23(i, j)] = out[m23(i, j)] + a[i] * b[j];
}

// out[0 .. NA + NB - 2] = a * b (ascending powers)
template <int NA, int NB>
__device__ __forceinline__ void conv(const double *a, const double *b, double *out)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 0; m < NA + NB - 1; ++m) out[m] = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) out[i + j] = out[i + j] + a[i] * b[j];
}

// the solving lane's view of its LDS area: element e of lane `lane`
struct LaneMem {
    double *base;
    __device__ __forceinline__ double &operator()(int e) const { return base[(size_t)e * TV_B]; }
};

// c[0] + c[1] x + ... + c[d] x^d, coefficients at L(at) .. L(at + d)
__device__ __forceinline__ double horner(const LaneMem &L, int at, int d, double x)
{
#pragma clang fp contract(off)
    double r = L(at + d);
    for (int i = d - 1; i >= 0; --i) r = r * x + L(at + i);
    return r;
}

// Null space of the 5 x 9 design matrix at L(9 r + c) into L(TV_BASIS + 9 b + i); perm: the lane's nine column indices in
// LDS (stride TV_B).  false: a pivot is zero or not finite.
__device__ bool nullspace4(const LaneMem &L, int32_t *perm)
{
#pragma clang fp contract(off)
    for (int c = 0; c < 9; ++c) perm[c * TV_B] = c;
    for (int k = 0; k < 5; ++k) {
        int pr = k, pc = k;
        double pa = -1.0;
        for (int r = k; r < 5; ++r)
            for (int c = k; c < 9; ++c) {
                const double a = fabs(L(9 * r + c));
                if (a > pa) { pr = r; pc = c; pa = a; }
            }
        if (!(pa > 0.0) || !finite_d(pa)) return false;
        if (pr != k)
            for (int c = 0; c < 9; ++c) { const double u = L(9 * k + c); L(9 * k + c) = L(9 * pr + c); L(9 * pr + c) = u; }
        if (pc != k) {
            for (int r = 0; r < 5; ++r) { const double u = L(9 * r + k); L(9 * r + k) = L(9 * r + pc); L(9 * r + pc) = u; }
            const int32_t u = perm[k * TV_B]; perm[k * TV_B] = perm[pc * TV_B]; perm[pc * TV_B] = u;
        }
        const double p = L(9 * k + k);
        for (int c = k + 1; c < 9; ++c) L(9 * k + c) = L(9 * k + c) / p;
        for (int r = 0; r < 5; ++r) {
            if (r == k) continue;
            const double f = L(9 * r + k);
            for (int c = k + 1; c < 9; ++c) L(9 * r + c) = L(9 * r + c) - f * L(9 * k + c);
        }
    }
    for (int i = 0; i < 36; ++i) L(TV_BASIS + i) = 0.0;
    for (int b = 0; b < 4; ++b) {
        L(TV_BASIS + 9 * b + perm[(5 + b) * TV_B]) = 1.0;
        for (int k = 0; k < 5; ++k) L(TV_BASIS + 9 * b + perm[k * TV_B]) = -L(9 * k + 5 + b);
    }
    // mixed by a fixed Hadamard matrix: the coordinate of E that is set to 1 is then a sum of four of E's entries, not one
    // entry that may be small by structure (section 18)
    for (int i = 0; i < 9; ++i) {
        const double X = L(TV_BASIS + i), Y = L(TV_BASIS + 9 + i), Z = L(TV_BASIS + 18 + i), W = L(TV_BASIS + 27 + i);
        L(TV_BASIS + i) = ((X + Y) + Z) + W;
        L(TV_BASIS + 9 + i) = ((X - Y) + Z) - W;
        L(TV_BASIS + 18 + i) = ((X + Y) - Z) - W;
        L(TV_BASIS + 27 + i) = ((X - Y) - Z) + W;
    }
    return true;
}

// The 10 x 20 constraint matrix of E = x X + y Y + z Z + W into L(20 r + c): rows 0 .. 8 the entries of
// (E E' - trace(E E') / 2 I) E row by row, row 9 det E.
__device__ void constraint_rows(const LaneMem &L)
{
#pragma clang fp contract(off)
    double E[3][3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) E[i][j][b] = L(TV_BASIS + 9 * b + 3 * i + j);
    double G[3][3][10];                 // E E' - trace / 2 I
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            double a[10], b[10], c[10];
            mul11(E[i][0], E[j][0], a); mul11(E[i][1], E[j][1], b); mul11(E[i][2], E[j][2], c);
#pragma unroll
            for (int m = 0; m < 10; ++m) { G[i][j][m] = (a[m] + b[m]) + c[m]; G[j][i][m] = G[i][j][m]; }
        }
    double tr[10];
#pragma unroll
    for (int m = 0; m < 10; ++m) tr[m] = (G[0][0][m] + G[1][1][m]) + G[2][2][m];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int m = 0; m < 10; ++m) G[i][i][m] = G[i][i][m] - 0.5 * tr[m];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double a[20], b[20], c[20];
            mul21(G[i][0], E[0][j], a); mul21(G[i][1], E[1][j], b); mul21(G[i][2], E[2][j], c);
#pragma unroll
            for (int m = 0; m < 20; ++m) L(20 * (3 * i + j) + m) = (a[m] + b[m]) + c[m];
        }
    double m0[10], m1[10], m2[10], u[10], v[10];
    mul11(E[1][1], E[2][2], u); mul11(E[1][2], E[2][1], v);
#pragma unroll
    for (int m = 0; m < 10; ++m) m0[m] = u[m] - v[m];
    mul11(E[1][0], E[2][2], u); mul11(E[1][2], E[2][0], v);
#pragma unroll
    for (int m = 0; m < 10; ++m) m1[m] = u[m] - v[m];
    mul11(E[1][0], E[2][1], u); mul11(E[1][1], E[2][0], v);
#pragma unroll
    for (int m = 0; m < 10; ++m) m2[m] = u[m] - v[m];
    double a[20], b[20], c[20];
    mul21(m0, E[0][0], a); mul21(m1, E[0][1], b); mul21(m2, E[0][2], c);
#pragma unroll
    for (int m = 0; m < 20; ++m) L(180 + m) = (a[m] - b[m]) + c[m];
}

// Gauss-Jordan on L(20 r + c) over the first ten columns, partial pivoting
__device__ bool eliminate(const LaneMem &L)
{
#pragma clang fp contract(off)
    for (int k = 0; k < 10; ++k) {
        int pr = k;
        double pa = -1.0;
        for (int r = k; r < 10; ++r) {
            const double a = fabs(L(20 * r + k));
            if (a > pa) { pr = r; pa = a; }
        }
        if (!(pa > 0.0) || !finite_d(pa)) return false;
        if (pr != k)
            for (int c = 0; c < 20; ++c) { const double u = L(20 * k + c); L(20 * k + c) = L(20 * pr + c); L(20 * pr + c) = u; }
        const double p = L(20 * k + k);
        for (int c = k + 1; c < 20; ++c) L(20 * k + c) = L(20 * k + c) / p;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = L(20 * r + k);
            for (int c = k + 1; c < 20; ++c) L(20 * r + c) = L(20 * r + c) - f * L(20 * k + c);
        }
    }
    return true;
}

// Rows 4 .. 9 of the eliminated matrix -> p1, p2, p3 at L(TV_P1 / TV_P2 / TV_P3) and the degree-10 polynomial, made
// monic, as level 10 of the derivative chain.  Returns the Cauchy bound R, or a NaN when there is no polynomial.
__device__ double z_polynomials(const LaneMem &L)
{
#pragma clang fp contract(off)
    double bx[3][4], by[3][4], b1[3][5];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double re[10], rf[10];
#pragma unroll
        for (int c = 0; c < 10; ++c) { re[c] = L(20 * (4 + 2 * q) + 10 + c); rf[c] = L(20 * (5 + 2 * q) + 10 + c); }
        bx[q][0] = re[2]; bx[q][1] = re[1] - rf[2]; bx[q][2] = re[0] - rf[1]; bx[q][3] = -rf[0];
        by[q][0] = re[5]; by[q][1] = re[4] - rf[5]; by[q][2] = re[3] - rf[4]; by[q][3] = -rf[3];
        b1[q][0] = re[9]; b1[q][1] = re[8] - rf[9]; b1[q][2] = re[7] - rf[8]; b1[q][3] = re[6] - rf[7]; b1[q][4] = -rf[6];
    }
    double p1[8], p2[8], p3[7], u[8], v[8];
    conv<4, 5>(by[0], b1[1], u); conv<5, 4>(b1[0], by[1], v);
#pragma unroll
    for (int m = 0; m < 8; ++m) p1[m] = u[m] - v[m];
    conv<5, 4>(b1[0], bx[1], u); conv<4, 5>(bx[0], b1[1], v);
#pragma unroll
    for (int m = 0; m < 8; ++m) p2[m] = u[m] - v[m];
    conv<4, 4>(bx[0], by[1], u); conv<4, 4>(by[0], bx[1], v);
#pragma unroll
    for (int m = 0; m < 7; ++m) p3[m] = u[m] - v[m];
    double ca[11], cb[11], cc[11], c[11];
    conv<8, 4>(p1, bx[2], ca); conv<8, 4>(p2, by[2], cb); conv<7, 5>(p3, b1[2], cc);
#pragma unroll
    for (int m = 0; m < 11; ++m) c[m] = (ca[m] + cb[m]) + cc[m];
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 11; ++m) s = s + c[m];
    if (!finite_d(s) || c[10] == 0.0) return __builtin_nan("");
#pragma unroll
    for (int m = 0; m < 8; ++m) { L(TV_P1 + m) = p1[m]; L(TV_P2 + m) = p2[m]; }
#pragma unroll
    for (int m = 0; m < 7; ++m) L(TV_P3 + m) = p3[m];
    double R = 0.0;
#pragma unroll
    for (int m = 0; m < 10; ++m) {
        const double a = c[m] / c[10];
        L(54 + m) = a;
        if (fabs(a) > R) R = fabs(a);
    }
    L(64) = 1.0;
    return 1.0 + R;
}

// Real roots of the monic degree-10 polynomial at level 10, ascending, through the derivative chain.  Returns their count;
// *at: where the list starts in the lane's area.
__device__ int real_roots(const LaneMem &L, double R, int *at)
{
#pragma clang fp contract(off)
    for (int d = 10; d > 1; --d) {
        const int od = (d - 1) * (d + 2) / 2, om = (d - 2) * (d + 1) / 2;
        for (int i = 0; i < d; ++i) L(om + i) = L(od + i + 1) * (double)(i + 1);
    }
    int nprev = 0, cur = TV_ROOTS0, prev = TV_ROOTS1;
    for (int d = 1; d <= 10; ++d) {
        const int od = (d - 1) * (d + 2) / 2, om = (d - 2) * (d + 1) / 2;
        { const int u = cur; cur = prev; prev = u; }
        int nr = 0;
        double lo = -R, flo = horner(L, od, d, lo);
        for (int i = 0; i <= nprev; ++i) {
            const double hi0 = i < nprev ? L(prev + i) : R;
            const double fhi0 = horner(L, od, d, hi0);
            if ((flo > 0.0) != (fhi0 > 0.0)) {
                double a = lo, b = hi0;
                for (int k = 0; k < TV_BISECT; ++k) {
                    const double mid = 0.5 * (a + b);
                    if ((horner(L, od, d, mid) > 0.0) == (flo > 0.0)) a = mid; else b = mid;
                }
                double x = 0.5 * (a + b), fx = horner(L, od, d, x);
                for (int k = 0; k < TV_NEWTON; ++k) {
                    const double df = d > 1 ? horner(L, om, d - 1, x) : L(1);
                    const double xn = x - fx / df;
                    if (xn >= a && xn <= b) {
                        const double fn = horner(L, od, d, xn);
                        if (fabs(fn) < fabs(fx)) { x = xn; fx = fn; }
                    }
                }
                L(cur + nr) = x;
                ++nr;
            }
            lo = hi0; flo = fhi0;
        }
        nprev = nr;
    }
    *at = cur;
    return nprev;
}

__device__ __forceinline__ void mm3(const double *A, const double *B, double *C)       // A B
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void mmt3(const double *A, const double *B, double *C)      // A B'
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1]) + A[3 * i + 2] * B[3 * j + 2];
}
__device__ __forceinline__ void cofactors(const double *e, double *c)
{
#pragma clang fp contract(off)
    c[0] = e[4] * e[8] - e[5] * e[7]; c[1] = e[5] * e[6] - e[3] * e[8]; c[2] = e[3] * e[7] - e[4] * e[6];
    c[3] = e[2] * e[7] - e[1] * e[8]; c[4] = e[0] * e[8] - e[2] * e[6]; c[5] = e[1] * e[6] - e[0] * e[7];
    c[6] = e[1] * e[5] - e[2] * e[4]; c[7] = e[2] * e[3] - e[0] * e[5]; c[8] = e[0] * e[4] - e[1] * e[3];
}

// the ten constraint values of E (nine of (E E' - trace(E E') / 2 I) E, then det E), M = E E' - trace / 2 I; returns
// their squared sum
__device__ __forceinline__ double constraints(const double *E, double *f, double *M)
{
#pragma clang fp contract(off)
    mmt3(E, E, M);
    const double h = 0.5 * ((M[0] + M[4]) + M[8]);
    M[0] = M[0] - h; M[4] = M[4] - h; M[8] = M[8] - h;
    mm3(M, E, f);
    f[9] = (E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6])) + E[2] * (E[3] * E[7] - E[4] * E[6]);
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) c = c + f[k] * f[k];
    return c;
}

// TV_POLISH Gauss-Newton steps on (x, y, z) against the constraints of E = x X + y Y + z Z + W itself; a step is kept
// only if it lowers their squared sum.  Bs: the four basis vectors (X, Y, Z, W).
__device__ void polish(const double (&Bs)[4][9], double x, double y, double z, double *E)
{
#pragma clang fp contract(off)
    double f[10], M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = ((x * Bs[0][i] + y * Bs[1][i]) + z * Bs[2][i]) + Bs[3][i];
    double c = constraints(E, f, M);
    for (int step = 0; step < TV_POLISH; ++step) {
        double cof[9], J[3][10];
        cofactors(E, cof);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double *D = Bs[q];
            double a[9], b[9], dM[9];
            mmt3(D, E, a); mmt3(E, D, b);
#pragma unroll
            for (int i = 0; i < 9; ++i) dM[i] = a[i] + b[i];
            const double h = 0.5 * ((dM[0] + dM[4]) + dM[8]);
            dM[0] = dM[0] - h; dM[4] = dM[4] - h; dM[8] = dM[8] - h;
            mm3(dM, E, a); mm3(M, D, b);
#pragma unroll
            for (int i = 0; i < 9; ++i) J[q][i] = a[i] + b[i];
            double dd = 0.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) dd = dd + cof[i] * D[i];
            J[q][9] = dd;
        }
        double N[3][3], g[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = a; b < 3; ++b) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 10; ++k) t = t + J[a][k] * J[b][k];
                N[a][b] = t;
            }
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 10; ++k) t = t + J[a][k] * f[k];
            g[a] = t;
        }
        const double c00 = N[1][1] * N[2][2] - N[1][2] * N[1][2];
        const double c01 = N[0][2] * N[1][2] - N[0][1] * N[2][2];
        const double c02 = N[0][1] * N[1][2] - N[0][2] * N[1][1];
        const double c11 = N[0][0] * N[2][2] - N[0][2] * N[0][2];
        const double c12 = N[0][1] * N[0][2] - N[0][0] * N[1][2];
        const double c22 = N[0][0] * N[1][1] - N[0][1] * N[0][1];
        const double det = (N[0][0] * c00 + N[0][1] * c01) + N[0][2] * c02;
        if (!(det > 0.0)) break;
        const double xn = x - ((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det;
        const double yn = y - ((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det;
        const double zn = z - ((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det;
        double En[9], fn[10], Mn[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) En[i] = ((xn * Bs[0][i] + yn * Bs[1][i]) + zn * Bs[2][i]) + Bs[3][i];
        const double cn = constraints(En, fn, Mn);
        if (!(cn < c)) break;
        x = xn; y = yn; z = zn; c = cn;
#pragma unroll
        for (int i = 0; i < 9; ++i) { E[i] = En[i]; M[i] = Mn[i]; }
#pragma unroll
        for (int i = 0; i < 10; ++i) f[i] = fn[i];
    }
}

// Step 4 of section 18: the models of one sample (entries idx[0 .. 4] of ent, x1 y1 x2 y2 each) into out (9 doubles each);
// returns their number.
__device__ int five_point(const LaneMem &L, int32_t *perm, const double *ent, const int32_t *idx, double *out)
{
#pragma clang fp contract(off)
    for (int k = 0; k < 5; ++k) {
        const double *s = ent + 4 * (size_t)idx[k];
        const double x1 = s[0], y1 = s[1], x2 = s[2], y2 = s[3];
        L(9 * k + 0) = x2 * x1; L(9 * k + 1) = x2 * y1; L(9 * k + 2) = x2;
        L(9 * k + 3) = y2 * x1; L(9 * k + 4) = y2 * y1; L(9 * k + 5) = y2;
        L(9 * k + 6) = x1; L(9 * k + 7) = y1; L(9 * k + 8) = 1.0;
    }
    if (!nullspace4(L, perm)) return 0;
    constraint_rows(L);
    if (!eliminate(L)) return 0;
    const double R = z_polynomials(L);
    if (!finite_d(R)) return 0;
    int at = 0;
    const int nr = real_roots(L, R, &at);
    int nm = 0;
    double Bs[4][9];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int i = 0; i < 9; ++i) Bs[b][i] = L(TV_BASIS + 9 * b + i);
    for (int r = 0; r < nr; ++r) {
        const double z = L(at + r);
        const double w = horner(L, TV_P3, 6, z);
        const double x = horner(L, TV_P1, 7, z) / w, y = horner(L, TV_P2, 7, z) / w;
        double E[9], ss = 0.0;
        polish(Bs, x, y, z, E);
#pragma unroll
        for (int i = 0; i < 9; ++i) ss = ss + E[i] * E[i];
        const double nrm = sqrt(ss);
        if (!finite_d(nrm) || nrm == 0.0) continue;
#pragma unroll
        for (int i = 0; i < 9; ++i) out[9 * nm + i] = E[i] / nrm;
        ++nm;
    }
    return nm;
}

// OpenCV's essential-matrix error (x2' E x1)^2 / (|E x1|_xy^2 + |E' x2|_xy^2), as float, against thr^2 as float
__device__ __forceinline__ bool is_inlier(const double *E, const double *p, float thr2)
{
#pragma clang fp contract(off)
    const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    const double a0 = (E[0] * x1 + E[1] * y1) + E[2];
    const double a1 = (E[3] * x1 + E[4] * y1) + E[5];
    const double a2 = (E[6] * x1 + E[7] * y1) + E[8];
    const double b0 = (E[0] * x2 + E[3] * y2) + E[6];
    const double b1 = (E[1] * x2 + E[4] * y2) + E[7];
    const double r = (x2 * a0 + y2 * a1) + a2;
    const double den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    return (float)((r * r) / den) <= thr2;        // a NaN compares false
}

// E = [t]x R without an SVD: t from the largest cross product of E's columns, R1 / R2 = cof(En) -/+ [t]x En
__device__ bool decompose(const double *E, double *R1, double *R2, double *t)
{
#pragma clang fp contract(off)
    double best[3] = {0.0, 0.0, 0.0}, bn = 0.0;
    bool have = false;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int a = q == 2 ? 1 : 0, b = q == 0 ? 1 : 2;
        const double p[3] = {E[a], E[3 + a], E[6 + a]}, r[3] = {E[b], E[3 + b], E[6 + b]};
        const double c[3] = {p[1] * r[2] - p[2] * r[1], p[2] * r[0] - p[0] * r[2], p[0] * r[1] - p[1] * r[0]};
        const double n2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
        if (n2 > bn) { best[0] = c[0]; best[1] = c[1]; best[2] = c[2]; bn = n2; have = true; }
    }
    if (!have || !finite_d(bn)) return false;
    const double nt = sqrt(bn);
    for (int i = 0; i < 3; ++i) t[i] = best[i] / nt;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) s = s + E[i] * E[i];
    const double sc = sqrt(0.5 * s);
    double e[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = E[i] / sc;
    const double cof[9] = {e[4] * e[8] - e[5] * e[7], e[5] * e[6] - e[3] * e[8], e[3] * e[7] - e[4] * e[6],
                           e[2] * e[7] - e[1] * e[8], e[0] * e[8] - e[2] * e[6], e[1] * e[6] - e[0] * e[7],
                           e[1] * e[5] - e[2] * e[4], e[2] * e[3] - e[0] * e[5], e[0] * e[4] - e[1] * e[3]};
    double tx[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        tx[j] = t[1] * e[6 + j] - t[2] * e[3 + j];
        tx[3 + j] = t[2] * e[j] - t[0] * e[6 + j];
        tx[6 + j] = t[0] * e[3 + j] - t[1] * e[j];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) { R1[i] = cof[i] - tx[i]; R2[i] = cof[i] + tx[i]; }
    return true;
}

// depths z1, z2 that bring z1 R (x1, y1, 1) + t closest to z2 (x2, y2, 1); good: both inside (0, dist)
__device__ __forceinline__ bool cheiral(const double *R, const double *t, const double *p, double dist)
{
#pragma clang fp contract(off)
    const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    const double a0 = (R[0] * x1 + R[1] * y1) + R[2];
    const double a1 = (R[3] * x1 + R[4] * y1) + R[5];
    const double a2 = (R[6] * x1 + R[7] * y1) + R[8];
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double bb = (x2 * x2 + y2 * y2) + 1.0;
    const double ab = (a0 * x2 + a1 * y2) + a2;
    const double at = (a0 * t[0] + a1 * t[1]) + a2 * t[2];
    const double bt = (x2 * t[0] + y2 * t[1]) + t[2];
    const double det = aa * bb - ab * ab;
    const double z1 = (ab * bt - at * bb) / det;
    const double z2 = (aa * bt - ab * at) / det;
    return z1 > 0.0 && z1 < dist && z2 > 0.0 && z2 < dist;
}

__global__ __launch_bounds__(TV_BLOCK) void k_tv_pair(TvArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char tv_smem[];
    double *s_lane = reinterpret_cast<double *>(tv_smem);                  // [TV_LANE_D][TV_B]
    double *s_model = s_lane + (size_t)TV_LANE_D * TV_B;                   // [TV_B][TV_MAXM][9]
    double *s_ent = s_model + (size_t)TV_B * TV_MAXM * 9;                  // [TV_NLDS][4]
    __shared__ double s_best[9], s_K1[6], s_K2[6], s_Km[4], s_R[2][9], s_t[2][3];
    __shared__ int32_t s_perm[9][TV_B];
    __shared__ int32_t s_idx[TV_B][5], s_nm[TV_B], s_good[TV_B][TV_MAXM], s_cnt[TV_BLOCK / 64][4];
    __shared__ int32_t s_niters, s_bestc, s_it, s_flag;

    const int v = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t o0 = a.off[v], n64 = a.off[v + 1] - o0;
    const int n = n64 < 0 ? 0 : (n64 > 0x7fffffff ? 0x7fffffff : (int)n64);
    double *E_out = a.E + 9 * (size_t)v, *pose_out = a.pose + 12 * (size_t)v;
    uint8_t *mask = a.mask + o0, *cmask = a.cmask + o0;
    int32_t *count = a.count + 2 * (size_t)v;

    if (t < 6) { s_K1[t] = a.intr1[6 * (size_t)v + t]; s_K2[t] = a.intr2[6 * (size_t)v + t]; }
    if (t < 4) s_Km[t] = (a.intr1[6 * (size_t)v + t] + a.intr2[6 * (size_t)v + t]) * 0.5;
    if (n < 5) {                                    // step 1
        for (int e = t; e < n; e += TV_BLOCK) { mask[e] = 0; cmask[e] = 0; }
        if (t < 9) E_out[t] = 0.0;
        if (t < 12) pose_out[t] = 0.0;
        if (t == 0) { count[0] = -2; count[1] = 0; if (a.iters) a.iters[v] = 0; }
        return;
    }
    __syncthreads();
    const double *ent;                              // the pair's normalised entries
    {
        double *dst = n <= TV_NLDS ? s_ent : a.norm + 4 * o0;
        for (int e = t; e < n; e += TV_BLOCK) {
            const size_t g = (size_t)(o0 + e);
            normalise(s_K1, s_Km, a.xy1[2 * g], a.xy1[2 * g + 1], &dst[4 * (size_t)e], &dst[4 * (size_t)e + 1]);
            normalise(s_K2, s_Km, a.xy2[2 * g], a.xy2[2 * g + 1], &dst[4 * (size_t)e + 2], &dst[4 * (size_t)e + 3]);
        }
        ent = dst;
    }
    if (t == 0) { s_niters = a.max_iters; s_bestc = 0; s_it = 0; s_flag = 0; }
    __syncthreads();                                // (the workspace slice is read back by this workgroup only)
    const double thr_n = a.thr / ((s_Km[0] + s_Km[1]) * 0.5);
    const float thr2 = (float)(thr_n * thr_n);

    unsigned long long rng = 0xffffffffffffffffULL;          // lane 0 owns the stream
    for (;;) {
        const int base = s_it, niters = s_niters, best0 = s_bestc;
        if (s_flag || base >= niters) break;
        __syncthreads();
        const int nd = min(TV_B, niters - base);
        if (t == 0) {                                         // draw
            for (int h = 0; h < nd; ++h) {
                for (int i = 0; i < 5;) {
                    const int r = (int)(rng_next(rng) % (unsigned)n);
                    bool dup = false;
                    for (int j = 0; j < i; ++j) dup |= s_idx[h][j] == r;
                    if (dup) continue;
                    s_idx[h][i++] = r;
                }
            }
        }
        __syncthreads();
        if (t < nd) {                                         // solve
            LaneMem L{s_lane + t};
            s_nm[t] = five_point(L, &s_perm[0][t], ent, s_idx[t], s_model + (size_t)t * TV_MAXM * 9);
        }
        __syncthreads();
        int bound = max(best0, 4);                            // score: wave wv takes samples wv, wv + 4, ...
        for (int h = wv; h < nd; h += TV_BLOCK / 64) {
            const int nm = s_nm[h];
            for (int m = 0; m < nm; ++m) {
                double E[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) E[i] = s_model[((size_t)h * TV_MAXM + m) * 9 + i];
                int good = 0;
                for (int e0 = 0; e0 < n; e0 += 64) {
                    if (good + (n - e0) <= bound) break;      // cannot be accepted any more (wave-uniform)
                    const int e = e0 + lane;
                    bool in = false;
                    if (e < n) in = is_inlier(E, ent + 4 * (size_t)e, thr2);
                    good += (int)__popcll(__ballot(in));
                }
                if (lane == 0) s_good[h][m] = good;
                bound = max(bound, good);
            }
        }
        __syncthreads();
        if (t == 0) {                                         // accept, in iteration order
            int nit = niters, best = best0, it = base;
            bool stop = false;
            for (int h = 0; h < nd; ++h) {
                if (base + h >= nit) { stop = true; break; }
                for (int m = 0; m < s_nm[h]; ++m) {
                    if (s_good[h][m] > max(best, 4)) {
                        best = s_good[h][m];
                        for (int i = 0; i < 9; ++i) s_best[i] = s_model[((size_t)h * TV_MAXM + m) * 9 + i];
                        nit = update_num_iters(a.conf, (double)(n - best) / n, 5, nit);
                    }
                }
                it = base + h + 1;
            }
            s_niters = nit; s_bestc = best; s_it = it; s_flag = stop ? 1 : 0;
        }
        __syncthreads();
    }
    __syncthreads();
    const int best = s_bestc;
    if (t == 0 && a.iters) a.iters[v] = s_it;
    if (best == 0) {                                          // no accepted model
        for (int e = t; e < n; e += TV_BLOCK) { mask[e] = 0; cmask[e] = 0; }
        if (t < 9) E_out[t] = 0.0;
        if (t < 12) pose_out[t] = 0.0;
        if (t == 0) { count[0] = -1; count[1] = 0; }
        return;
    }
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = s_best[i];
    if (t < 9) E_out[t] = s_best[t];
    if (t == 0) count[0] = best;

    double R1[9], R2[9], tt[3], nt[3];                        // pose recovery (every thread: the same bits)
    const bool have = decompose(E, R1, R2, tt);
    if (!have) {
        for (int e = t; e < n; e += TV_BLOCK) { mask[e] = is_inlier(E, ent + 4 * (size_t)e, thr2) ? 1 : 0; cmask[e] = 0; }
        if (t < 12) pose_out[t] = 0.0;
        if (t == 0) count[1] = 0;
        return;
    }
    for (int i = 0; i < 3; ++i) nt[i] = -tt[i];
    int g0 = 0, g1 = 0, g2 = 0, g3 = 0;
    for (int e0 = wv * 64; e0 < n; e0 += TV_BLOCK) {
        const int e = e0 + lane;
        bool in = false, c0 = false, c1 = false, c2 = false, c3 = false;
        if (e < n) {
            const double *p = ent + 4 * (size_t)e;
            in = is_inlier(E, p, thr2);
            mask[e] = in ? 1 : 0;
            c0 = in && cheiral(R1, tt, p, a.dist); c1 = in && cheiral(R2, tt, p, a.dist);
            c2 = in && cheiral(R1, nt, p, a.dist); c3 = in && cheiral(R2, nt, p, a.dist);
        }
        g0 += (int)__popcll(__ballot(c0)); g1 += (int)__popcll(__ballot(c1));
        g2 += (int)__popcll(__ballot(c2)); g3 += (int)__popcll(__ballot(c3));
    }
    if (lane == 0) { s_cnt[wv][0] = g0; s_cnt[wv][1] = g1; s_cnt[wv][2] = g2; s_cnt[wv][3] = g3; }
    if (t == 0) {                                             // the winner is picked by an LDS address, not a register index
#pragma unroll
        for (int i = 0; i < 9; ++i) { s_R[0][i] = R1[i]; s_R[1][i] = R2[i]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) { s_t[0][i] = tt[i]; s_t[1][i] = nt[i]; }
    }
    __syncthreads();
    int g[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        g[c] = 0;
#pragma unroll
        for (int w = 0; w < TV_BLOCK / 64; ++w) g[c] += s_cnt[w][c];
    }
    int win;                                                  // cv::recoverPose's cascade
    if (g[0] >= g[1] && g[0] >= g[2] && g[0] >= g[3]) win = 0;
    else if (g[1] >= g[0] && g[1] >= g[2] && g[1] >= g[3]) win = 1;
    else if (g[2] >= g[0] && g[2] >= g[1] && g[2] >= g[3]) win = 2;
    else win = 3;
    double Rs[9], ts[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rs[i] = s_R[win & 1][i];
#pragma unroll
    for (int i = 0; i < 3; ++i) ts[i] = s_t[win >> 1][i];
    for (int e = t; e < n; e += TV_BLOCK) {
        const double *p = ent + 4 * (size_t)e;
        cmask[e] = is_inlier(E, p, thr2) && cheiral(Rs, ts, p, a.dist) ? 1 : 0;
    }
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) pose_out[4 * i + j] = Rs[3 * i + j];
            pose_out[4 * i + 3] = ts[i];
        }
    }
    if (t == 0) count[1] = win == 0 ? g[0] : win == 1 ? g[1] : win == 2 ? g[2] : g[3];
}

int check_options(rcn_ctx *ctx, const char *who, const rcn_twoview_options *o)
{
    if (!(o->threshold > 0.0) || !(o->confidence > 0.0 && o->confidence < 1.0) || !(o->distance_threshold > 0.0) || o->max_iterations <= 0) {
        ctx->set_error(std::string(who) + ": threshold > 0, 0 < confidence < 1, distance_threshold > 0, max_iterations > 0");
        return RCN_ERR_ARG;
    }
    return RCN_OK;
}

void fill_args(TvArgs &a, const rcn_twoview_options *o)
{
    a.thr = o->threshold;
    a.conf = o->confidence;
    a.dist = o->distance_threshold;
    a.max_iters = o->max_iterations;
}

int launch(rcn_ctx *ctx, const TvArgs &a, int32_t n_pairs)
{
    static std::mutex once_mu;
    static std::vector<int> done;                     // devices whose copy of the kernel has the attribute
    {
        std::lock_guard<std::mutex> lk(once_mu);
        if (std::find(done.begin(), done.end(), ctx->device) == done.end()) {
            RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_tv_pair), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TV_LDS_BYTES));
            done.push_back(ctx->device);
        }
    }
    k_tv_pair<<<(unsigned)n_pairs, TV_BLOCK, TV_LDS_BYTES, ctx->stream>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

}  // namespace

// k_tv_pair on entries that already lie in device memory, with ctx->mu held (rcn_twoview_geometry, homography.hip): the
// options checked as rcn_twoview_init checks them; n_pairs == 0 checks them only.
int rcn_int_twoview_launch(rcn_ctx *ctx, const char *who, const rcn_twoview_options *opt, int32_t n_pairs, const int64_t *off_dev,
                           const int32_t *xy1_dev, const int32_t *xy2_dev, const double *intr6_1_dev, const double *intr6_2_dev,
                           double *norm_dev, double *E_dev, double *pose34_dev, uint8_t *mask_dev, uint8_t *cheir_mask_dev,
                           int32_t *count_dev, int32_t *iterations_dev)
{
    int rc = check_options(ctx, who, opt);
    if (rc || n_pairs == 0) return rc;
    TvArgs a{};
    a.off = off_dev; a.xy1 = xy1_dev; a.xy2 = xy2_dev; a.intr1 = intr6_1_dev; a.intr2 = intr6_2_dev; a.norm = norm_dev;
    a.E = E_dev; a.pose = pose34_dev; a.mask = mask_dev; a.cmask = cheir_mask_dev; a.count = count_dev; a.iters = iterations_dev;
    fill_args(a, opt);
    return launch(ctx, a, n_pairs);
}

// rcn_twoview_init with ctx->mu held (rcn_ba_session_init_pair)
int rcn_int_twoview_host(rcn_ctx *ctx, const char *who, int32_t n_pairs, const int64_t *off, const int32_t *xy1, const int32_t *xy2,
                         const double *intr6_1, const double *intr6_2, const rcn_twoview_options *opt, double *E_out,
                         double *pose34_out, uint8_t *mask_out, uint8_t *cheir_mask_out, int32_t *count_out, int32_t *iterations_out)
{
    rcn_twoview_options o;
    if (opt) o = *opt; else rcn_twoview_default_options(&o);
    int rc = check_options(ctx, who, &o);
    if (rc) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!off || !intr6_1 || !intr6_2 || !pose34_out || !count_out))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    if (n_pairs == 0) return RCN_OK;
    if (off[0] != 0) { ctx->set_error(std::string(who) + ": off[0] must be 0"); return RCN_ERR_ARG; }
    for (int32_t p = 0; p < n_pairs; ++p)
        if (off[p + 1] < off[p] || off[p + 1] - off[p] > 0x7fffffff) { ctx->set_error(std::string(who) + ": off must be non-decreasing"); return RCN_ERR_ARG; }
    const int64_t ne = off[n_pairs];
    if (ne > 0 && (!xy1 || !xy2 || !mask_out)) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t np = (size_t)n_pairs, nE = (size_t)ne;
    const size_t b_off = 8 * (np + 1), b_xy = 8 * nE, b_intr = 48 * np, b_norm = 32 * nE, b_E = 72 * np, b_pose = 96 * np, b_mask = nE,
                 b_cnt = 8 * np, b_it = 4 * np;
    RCN_HIP(ctx->tv_hws.reserve(al(b_off) + 2 * al(b_xy) + 2 * al(b_intr) + al(b_norm) + al(b_E) + al(b_pose) + 2 * al(b_mask) + al(b_cnt) + al(b_it) + 256));
    char *w = ctx->tv_hws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += al(b); return q; };
    int64_t *d_off = (int64_t *)take(b_off);
    int32_t *d_xy1 = (int32_t *)take(b_xy), *d_xy2 = (int32_t *)take(b_xy);
    double *d_i1 = (double *)take(b_intr), *d_i2 = (double *)take(b_intr), *d_norm = (double *)take(b_norm), *d_E = (double *)take(b_E),
           *d_pose = (double *)take(b_pose);
    uint8_t *d_mask = (uint8_t *)take(b_mask), *d_cmask = (uint8_t *)take(b_mask);
    int32_t *d_cnt = (int32_t *)take(b_cnt), *d_it = (int32_t *)take(b_it);
    auto H2D = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    RCN_HIP(H2D(d_off, off, b_off)); RCN_HIP(H2D(d_xy1, xy1, b_xy)); RCN_HIP(H2D(d_xy2, xy2, b_xy));
    RCN_HIP(H2D(d_i1, intr6_1, b_intr)); RCN_HIP(H2D(d_i2, intr6_2, b_intr));
    TvArgs a{};
    a.off = d_off; a.xy1 = d_xy1; a.xy2 = d_xy2; a.intr1 = d_i1; a.intr2 = d_i2; a.norm = d_norm;
    a.E = d_E; a.pose = d_pose; a.mask = d_mask; a.cmask = d_cmask; a.count = d_cnt; a.iters = d_it;
    fill_args(a, &o);
    rc = launch(ctx, a, n_pairs);
    if (rc) return rc;
    auto D2H = [&](void *dst, const void *src, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    RCN_HIP(D2H(E_out, d_E, b_E)); RCN_HIP(D2H(pose34_out, d_pose, b_pose)); RCN_HIP(D2H(mask_out, d_mask, b_mask));
    RCN_HIP(D2H(cheir_mask_out, d_cmask, b_mask)); RCN_HIP(D2H(count_out, d_cnt, b_cnt)); RCN_HIP(D2H(iterations_out, d_it, b_it));
    RCN_HIP(hipStreamSynchronize(st));
    return RCN_OK;
}

extern "C" {

void rcn_twoview_default_options(rcn_twoview_options *o)
{
    if (!o) return;
    o->threshold = 1.0;                 // cv::findEssentialMat's defaults
    o->confidence = 0.999;
    o->distance_threshold = 50.0;       // cv::recoverPose as the two-camera overload calls it
    o->max_iterations = 1000;
}

int rcn_twoview_init_device(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pairs, const double *intr6_1_dev, const double *intr6_2_dev,
                            const rcn_twoview_options *opt, int64_t capacity, int64_t *off_dev, int32_t *qt_dev, double *E_dev,
                            double *pose34_dev, uint8_t *mask_dev, uint8_t *cheir_mask_dev, int32_t *count_dev, int32_t *iterations_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_twoview_init_device";
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_twoview_options o;
    if (opt) o = *opt; else rcn_twoview_default_options(&o);
    int rc = check_options(ctx, who, &o);
    if (rc) return rc;
    if (n_pairs < 0 || capacity < 0 || !off_dev || (n_pairs > 0 && (!pairs || !intr6_1_dev || !intr6_2_dev || !pose34_dev || !count_dev)) ||
        (capacity > 0 && !mask_dev)) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    RCN_HIP(hipSetDevice(ctx->device));
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t np = (size_t)std::max(n_pairs, 1), cap = (size_t)std::max<int64_t>(capacity, 1);
    RCN_HIP(ctx->tv_dws.reserve(2 * al(8 * cap) + al(32 * cap) + al(72 * np) + al(cap) + 256));
    char *w = ctx->tv_dws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += al(b); return q; };
    int32_t *d_xy1 = (int32_t *)take(8 * cap), *d_xy2 = (int32_t *)take(8 * cap);
    double *d_norm = (double *)take(32 * cap), *d_E = (double *)take(72 * np);
    uint8_t *d_cmask = (uint8_t *)take(cap);
    rc = rcn_int_pair_fill(ctx, who, n_pairs, pairs, capacity, off_dev, d_xy1, d_xy2, qt_dev);
    if (rc || n_pairs == 0) return rc;
    TvArgs a{};
    a.off = off_dev; a.xy1 = d_xy1; a.xy2 = d_xy2; a.intr1 = intr6_1_dev; a.intr2 = intr6_2_dev; a.norm = d_norm;
    a.E = E_dev ? E_dev : d_E; a.pose = pose34_dev; a.mask = mask_dev; a.cmask = cheir_mask_dev ? cheir_mask_dev : d_cmask;
    a.count = count_dev; a.iters = iterations_dev;
    fill_args(a, &o);
    return launch(ctx, a, n_pairs);
}

// the camera block of rcn_ba_problem (angle-axis, translation) of rows of [R | t]: angle = acos((trace R - 1) / 2) clipped,
// axis from R - R', nothing below 1e-12 rad.  Pure host code.
int rcn_pose34_to_pose6(const double *pose34, double *pose6_out)
{
    if (!pose34 || !pose6_out) return RCN_ERR_ARG;
    const double *P = pose34;
    double c = ((P[0] + P[5] + P[10]) - 1.0) / 2.0;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double th = acos(c);
    if (th < 1e-12 || !(th == th)) pose6_out[0] = pose6_out[1] = pose6_out[2] = 0.0;
    else {
        const double d = 2.0 * sin(th);
        pose6_out[0] = (P[9] - P[6]) / d * th;
        pose6_out[1] = (P[2] - P[8]) / d * th;
        pose6_out[2] = (P[4] - P[1]) / d * th;
    }
    pose6_out[3] = P[3]; pose6_out[4] = P[7]; pose6_out[5] = P[11];
    return RCN_OK;
}

int rcn_twoview_init(rcn_ctx *ctx, int32_t n_pairs, const int64_t *off, const int32_t *xy1, const int32_t *xy2,
                     const double *intr6_1, const double *intr6_2, const rcn_twoview_options *opt, double *E_out,
                     double *pose34_out, uint8_t *mask_out, uint8_t *cheir_mask_out, int32_t *count_out, int32_t *iterations_out)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return rcn_int_twoview_host(ctx, "rcn_twoview_init", n_pairs, off, xy1, xy2, intr6_1, intr6_2, opt, E_out, pose34_out, mask_out,
                                cheir_mask_out, count_out, iterations_out);
}

}  // extern "C"
