// homography.hip -- batched homography RANSAC behind rcn_homography_ransac and the two-view classification behind
// rcn_twoview_geometry (include/rcn.h).  gfx950, fp64.
//
// cv::findHomography(src, dst, RANSAC, 3.0, mask, 2000, 0.995) on integer pixels, for a batch of
// pairs in one launch:
//
//   k_hg_pair   one workgroup of 256 threads per pair runs the pair's whole search:
//        gather   every entry's two pixels as doubles (X, Y, u, v), kept in LDS while they fit (HG_NLDS entries of 32
//                 bytes) and in the pair's slice of the workspace otherwise
//        rounds of HG_B samples
//          draw     one lane replays the sequential cv::RNG index stream (4 distinct indices per sample) and the subset
//                   check (no three points on a line in either image, equal orientation of the four triples), redrawing
//                   a rejected subset up to HG_ATTEMPTS times
//          solve    one lane per sample: per-axis Hartley normalisation, the 8 x 9 design matrix, its null vector by
//                   Gauss-Jordan with complete pivoting, denormalised, h33 = 1.  The lane's matrix lives element-major in
//                   LDS (HG_LANE_D doubles per lane): every data-dependent index is an LDS address, never a register array
//          score    one wave per sample, lanes over the entries; a model is dropped once good + remaining <= bound, bound
//                   counting earlier rounds and the wave's own earlier samples of this round (exact pruning, as k_tv_pair)
//          accept   one lane replays the acceptance rule in iteration order and discards what lies behind the stop
//        refit    over the inliers of the best model: centroid, mean absolute deviation, the 28 sums of the normal
//                 equations with h33 = 1, each by wg_sums (thread t adds entries t, t + 256, ... in order, a butterfly
//                 folds the wave, the four waves are added in order); lane 0 solves the 8 x 8 system as the null vector of
//                 [N | -g] with the minimal solver's elimination; then at most HG_REFINE Gauss-Newton steps on the
//                 forward transfer error in pixels, the same 28 sums per step, a step kept only if it lowers the cost
//        mask     the refitted model's inliers
//   k_tv_classify  one workgroup per pair: the parallax angle of every entry of the cheirality mask (acos from + - * /
//                 sqrt), its lower median by counting ranks, count_H / count_E, the label
//
// Every operation is a separately rounded IEEE double (contraction off) in one fixed order built from + - * / sqrt;
// tests/homography_ref.py restates that order and agrees bit for bit.  The one exception is pow / log in update_num_iters.
// No atomics.  The result depends neither on HG_B nor on the launch geometry.
#include "rcn_internal.h"
#include "ransac.h"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int HG_BLOCK = 256;         // 4 waves
constexpr int HG_B = 32;              // samples per round
constexpr int HG_NLDS = 2048;         // entries kept in LDS (32 bytes each)
constexpr int HG_LANE_D = 81;         // doubles of LDS per solving lane: the 8 x 9 matrix and its null vector
constexpr int HG_VEC = 72;
constexpr int HG_ATTEMPTS = 10000;    // cv::RANSACPointSetRegistrator::run calls getSubset with this cap
constexpr int HG_REFINE = 10;
constexpr int HG_NS = 28;             // sums of one pass of the refit
constexpr size_t HG_LDS_BYTES = 8 * ((size_t)HG_LANE_D * HG_B + (size_t)HG_B * 9 + 4 * (size_t)HG_NLDS);

struct HgArgs {
    const int64_t *off;
    const int32_t *xy1, *xy2;   // pixels of every entry
    double *ent;                // workspace: 4 doubles per entry
    double thr, conf;
    int32_t max_iters;
    double *H;
    uint8_t *mask;
    int32_t *count, *iters;
};

struct LaneMem {
    double *base;
    __device__ __forceinline__ double &operator()(int e) const { return base[(size_t)e * HG_B]; }
};

// haveCollinearPoints as the incremental sampler applied it: point 2 against (0, 1), point 3 against every earlier pair
__device__ __forceinline__ bool collinear(const double *x, const double *y)
{
#pragma clang fp contract(off)
    bool bad = false;
#pragma unroll
    for (int i = 2; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const double dx1 = x[j] - x[i], dy1 = y[j] - y[i];
#pragma unroll
            for (int k = 0; k < j; ++k) {
                const double dx2 = x[k] - x[i], dy2 = y[k] - y[i];
                bad |= fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (((fabs(dx1) + fabs(dy1)) + fabs(dx2)) + fabs(dy2));
            }
        }
    return bad;
}

__device__ __forceinline__ double det3(const double *x, const double *y, int a, int b, int c)
{
#pragma clang fp contract(off)
    return (x[a] * (y[b] - y[c]) - y[a] * (x[b] - x[c])) + (x[b] * y[c] - x[c] * y[b]);
}

// HomographyEstimatorCallback::checkSubset on the four entries X, Y -> u, v
__device__ __forceinline__ bool subset_ok(const double *X, const double *Y, const double *u, const double *v)
{
#pragma clang fp contract(off)
    if (collinear(X, Y) || collinear(u, v)) return false;
    int negative = 0;
    negative += det3(X, Y, 0, 1, 2) * det3(u, v, 0, 1, 2) < 0.0 ? 1 : 0;
    negative += det3(X, Y, 1, 2, 3) * det3(u, v, 1, 2, 3) < 0.0 ? 1 : 0;
    negative += det3(X, Y, 0, 2, 3) * det3(u, v, 0, 2, 3) < 0.0 ? 1 : 0;
    negative += det3(X, Y, 0, 1, 3) * det3(u, v, 0, 1, 3) < 0.0 ? 1 : 0;
    return negative == 0 || negative == 4;
}

// The null vector of the 8 x 9 matrix at L(9 r + c) into L(HG_VEC + i); perm: the lane's nine column indices in LDS (stride
// HG_B).  false: a pivot is zero or not finite.
__device__ bool nullvec8(const LaneMem &L, int32_t *perm)
{
#pragma clang fp contract(off)
    for (int c = 0; c < 9; ++c) perm[c * HG_B] = c;
    for (int k = 0; k < 8; ++k) {
        int pr = k, pc = k;
        double pa = -1.0;
        for (int r = k; r < 8; ++r)
            for (int c = k; c < 9; ++c) {
                const double a = fabs(L(9 * r + c));
                if (a > pa) { pr = r; pc = c; pa = a; }
            }
        if (!(pa > 0.0) || !finite_d(pa)) return false;
        if (pr != k)
            for (int c = 0; c < 9; ++c) { const double u = L(9 * k + c); L(9 * k + c) = L(9 * pr + c); L(9 * pr + c) = u; }
        if (pc != k) {
            for (int r = 0; r < 8; ++r) { const double u = L(9 * r + k); L(9 * r + k) = L(9 * r + pc); L(9 * r + pc) = u; }
            const int32_t u = perm[k * HG_B]; perm[k * HG_B] = perm[pc * HG_B]; perm[pc * HG_B] = u;
        }
        const double p = L(9 * k + k);
        for (int c = k + 1; c < 9; ++c) L(9 * k + c) = L(9 * k + c) / p;
        for (int r = 0; r < 8; ++r) {
            if (r == k) continue;
            const double f = L(9 * r + k);
            for (int c = k + 1; c < 9; ++c) L(9 * r + c) = L(9 * r + c) - f * L(9 * k + c);
        }
    }
    L(HG_VEC + perm[8 * HG_B]) = 1.0;
    for (int k = 0; k < 8; ++k) L(HG_VEC + perm[k * HG_B]) = -L(9 * k + 8);
    return true;
}

// inv(T_dst) H T_src for T = diag(s) (p - c), scaled so that h33 = 1; c, s: X Y u v.  false: h33 is zero or an entry is
// not finite.
__device__ __forceinline__ bool denormalise(const LaneMem &L, const double *c, const double *s, double *H)
{
#pragma clang fp contract(off)
    double T[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a = L(HG_VEC + 3 * r) * s[0], b = L(HG_VEC + 3 * r + 1) * s[1];
        T[3 * r] = a;
        T[3 * r + 1] = b;
        T[3 * r + 2] = (L(HG_VEC + 3 * r + 2) - a * c[0]) - b * c[1];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        H[q] = T[q] / s[2] + c[2] * T[6 + q];
        H[3 + q] = T[3 + q] / s[3] + c[3] * T[6 + q];
        H[6 + q] = T[6 + q];
    }
    const double d = H[8];
    if (!finite_d(d) || d == 0.0) return false;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) { H[i] = H[i] / d; ok &= finite_d(H[i]); }
    H[8] = 1.0;
    return ok;
}

// runKernel on the entries idx[0 .. 3] of ent (X Y u v each)
__device__ bool homography4(const LaneMem &L, int32_t *perm, const double *ent, const int32_t *idx, double *H)
{
#pragma clang fp contract(off)
    double q[4][4], c[4], s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k][i] = ent[4 * (size_t)idx[i] + k];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double m = (((q[k][0] + q[k][1]) + q[k][2]) + q[k][3]) / 4.0;
        const double d = ((fabs(q[k][0] - m) + fabs(q[k][1] - m)) + fabs(q[k][2] - m)) + fabs(q[k][3] - m);
        ok &= d >= DBL_EPSILON;
        c[k] = m;
        s[k] = 4.0 / d;
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double X = (q[0][i] - c[0]) * s[0], Y = (q[1][i] - c[1]) * s[1];
        const double x = (q[2][i] - c[2]) * s[2], y = (q[3][i] - c[3]) * s[3];
        const int r0 = 18 * i, r1 = 18 * i + 9;
        L(r0 + 0) = X; L(r0 + 1) = Y; L(r0 + 2) = 1.0; L(r0 + 3) = 0.0; L(r0 + 4) = 0.0; L(r0 + 5) = 0.0;
        L(r0 + 6) = -(x * X); L(r0 + 7) = -(x * Y); L(r0 + 8) = -x;
        L(r1 + 0) = 0.0; L(r1 + 1) = 0.0; L(r1 + 2) = 0.0; L(r1 + 3) = X; L(r1 + 4) = Y; L(r1 + 5) = 1.0;
        L(r1 + 6) = -(y * X); L(r1 + 7) = -(y * Y); L(r1 + 8) = -y;
    }
    if (!nullvec8(L, perm)) return false;
    return denormalise(L, c, s, H);
}

// forward transfer error |dst - proj(H src)|^2, as float, against thr^2 as float
__device__ __forceinline__ bool is_inlier(const double *H, const double *p, float thr2)
{
#pragma clang fp contract(off)
    const double X = p[0], Y = p[1], u = p[2], v = p[3];
    const double ww = 1.0 / ((H[6] * X + H[7] * Y) + H[8]);
    const double dx = ((H[0] * X + H[1] * Y) + H[2]) * ww - u;
    const double dy = ((H[3] * X + H[4] * Y) + H[5]) * ww - v;
    return (float)(dx * dx + dy * dy) <= thr2;        // a NaN compares false
}

// The workgroup's sums of K values per thread into tot[0 .. K): a butterfly folds the wave (xor 32 .. 1: every lane ends
// with the same bits), the four waves are added in order.  Called by all threads; ends with a barrier.
template <int K>
__device__ __forceinline__ void wg_sums(double *acc, double (*red)[HG_NS], double *tot)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double a = acc[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a = a + __shfl_xor(a, o);
        if (lane == 0) red[wv][k] = a;
    }
    __syncthreads();
    if (t < K) tot[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    __syncthreads();
}

// one entry's 28 terms of the normal equations of rows (a b c 0 0 0 -xa -xb | rx), (0 0 0 a b c -ya -yb | ry)
__device__ __forceinline__ void add28(double *acc, double a, double b, double c, double x, double y, double rx, double ry)
{
#pragma clang fp contract(off)
    const double aa = a * a, ab = a * b, ac = a * c, bb = b * b, bc = b * c, cc = c * c;
    const double q = x * x + y * y, p = x * rx + y * ry;
    acc[0] = acc[0] + aa; acc[1] = acc[1] + ab; acc[2] = acc[2] + ac; acc[3] = acc[3] + bb; acc[4] = acc[4] + bc; acc[5] = acc[5] + cc;
    acc[6] = acc[6] + x * aa; acc[7] = acc[7] + x * ab; acc[8] = acc[8] + x * bb; acc[9] = acc[9] + x * ac; acc[10] = acc[10] + x * bc;
    acc[11] = acc[11] + y * aa; acc[12] = acc[12] + y * ab; acc[13] = acc[13] + y * bb; acc[14] = acc[14] + y * ac; acc[15] = acc[15] + y * bc;
    acc[16] = acc[16] + q * aa; acc[17] = acc[17] + q * ab; acc[18] = acc[18] + q * bb;
    acc[19] = acc[19] + a * rx; acc[20] = acc[20] + b * rx; acc[21] = acc[21] + c * rx;
    acc[22] = acc[22] + a * ry; acc[23] = acc[23] + b * ry; acc[24] = acc[24] + c * ry;
    acc[25] = acc[25] + p * a; acc[26] = acc[26] + p * b;
    acc[27] = acc[27] + (rx * rx + ry * ry);
}

// where the sums sit in N: the 3 x 3 block of (a, b, c), the 3 x 2 block of x (a, b, c) (a, b); y's follows 5 later
__device__ constexpr int sys_tl(int i, int j)
{
    constexpr int T[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    return T[i][j];
}
__device__ constexpr int sys_r(int i, int j)
{
    constexpr int T[3][2] = {{6, 7}, {7, 8}, {9, 10}};
    return T[i][j];
}

// [N | -g] (8 x 9) of the 28 sums into L(9 r + c)
__device__ void put_system(const LaneMem &L, const double *S)
{
    for (int i = 0; i < 72; ++i) L(i) = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { L(9 * i + j) = S[sys_tl(i, j)]; L(9 * (3 + i) + 3 + j) = S[sys_tl(i, j)]; }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            L(9 * i + 6 + j) = -S[sys_r(i, j)]; L(9 * (6 + j) + i) = -S[sys_r(i, j)];
            L(9 * (3 + i) + 6 + j) = -S[5 + sys_r(i, j)]; L(9 * (6 + j) + 3 + i) = -S[5 + sys_r(i, j)];
        }
    }
    L(9 * 6 + 6) = S[16]; L(9 * 6 + 7) = S[17]; L(9 * 7 + 6) = S[17]; L(9 * 7 + 7) = S[18];
#pragma unroll
    for (int i = 0; i < 6; ++i) L(9 * i + 8) = -S[19 + i];
    L(9 * 6 + 8) = S[25]; L(9 * 7 + 8) = S[26];
}

// the 28 sums of one Gauss-Newton pass at h (h33 = 1) over the inliers flagged in mask
__device__ __forceinline__ void gn_pass(const double *h, const double *ent, const uint8_t *mask, int n, double (*red)[HG_NS], double *tot)
{
#pragma clang fp contract(off)
    double acc[HG_NS];
#pragma unroll
    for (int k = 0; k < HG_NS; ++k) acc[k] = 0.0;
    for (int e = threadIdx.x; e < n; e += HG_BLOCK) {
        if (!mask[e]) continue;
        const double *p = ent + 4 * (size_t)e;
        const double X = p[0], Y = p[1], u = p[2], v = p[3];
        const double c = 1.0 / ((h[6] * X + h[7] * Y) + 1.0);
        const double a = X * c, b = Y * c;
        const double px = ((h[0] * X + h[1] * Y) + h[2]) * c, py = ((h[3] * X + h[4] * Y) + h[5]) * c;
        add28(acc, a, b, c, px, py, px - u, py - v);
    }
    wg_sums<HG_NS>(acc, red, tot);
}

__global__ __launch_bounds__(HG_BLOCK) void k_hg_pair(HgArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char hg_smem[];
    double *s_lane = reinterpret_cast<double *>(hg_smem);                  // [HG_LANE_D][HG_B]
    double *s_model = s_lane + (size_t)HG_LANE_D * HG_B;                   // [HG_B][9]
    double *s_ent = s_model + (size_t)HG_B * 9;                            // [HG_NLDS][4]
    __shared__ double s_best[9], s_h[9], s_red[HG_BLOCK / 64][HG_NS], s_tot[HG_NS];
    __shared__ int32_t s_perm[9][HG_B];
    __shared__ int32_t s_idx[HG_B][4], s_ok[HG_B], s_good[HG_B], s_cnt[HG_BLOCK / 64];
    __shared__ int32_t s_niters, s_bestc, s_it, s_flag, s_nd, s_fail, s_go;

    const int v = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t o0 = a.off[v], n64 = a.off[v + 1] - o0;
    const int n = n64 < 0 ? 0 : (n64 > 0x7fffffff ? 0x7fffffff : (int)n64);
    double *H_out = a.H + 9 * (size_t)v;
    uint8_t *mask = a.mask + o0;

    if (n < 4) {
        for (int e = t; e < n; e += HG_BLOCK) mask[e] = 0;
        if (t < 9) H_out[t] = 0.0;
        if (t == 0) { a.count[v] = -2; if (a.iters) a.iters[v] = 0; }
        return;
    }
    double *entw = n <= HG_NLDS ? s_ent : a.ent + 4 * o0;
    for (int e = t; e < n; e += HG_BLOCK) {
        const size_t g = (size_t)(o0 + e);
        entw[4 * (size_t)e] = (double)a.xy1[2 * g]; entw[4 * (size_t)e + 1] = (double)a.xy1[2 * g + 1];
        entw[4 * (size_t)e + 2] = (double)a.xy2[2 * g]; entw[4 * (size_t)e + 3] = (double)a.xy2[2 * g + 1];
    }
    const double *ent = entw;
    if (t == 0) { s_niters = a.max_iters; s_bestc = 0; s_it = 0; s_flag = 0; }
    __syncthreads();                                // (the workspace slice is read back by this workgroup only)
    const float thr2 = (float)(a.thr * a.thr);

    if (n == 4) {                                   // the exact model, no search and no refit
        if (t == 0) {
            double X[4], Y[4], u[4], w[4], H[9];
#pragma unroll
            for (int i = 0; i < 4; ++i) { X[i] = ent[4 * i]; Y[i] = ent[4 * i + 1]; u[i] = ent[4 * i + 2]; w[i] = ent[4 * i + 3]; }
#pragma unroll
            for (int i = 0; i < 4; ++i) s_idx[0][i] = i;
            const bool ok = subset_ok(X, Y, u, w) && homography4(LaneMem{s_lane}, &s_perm[0][0], ent, s_idx[0], H);
#pragma unroll
            for (int i = 0; i < 9; ++i) H_out[i] = ok ? H[i] : 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) mask[i] = ok ? 1 : 0;
            a.count[v] = ok ? 4 : -1;
            if (a.iters) a.iters[v] = 0;
        }
        return;
    }

    unsigned long long rng = 0xffffffffffffffffULL;          // lane 0 owns the stream
    for (;;) {
        const int base = s_it, niters = s_niters, best0 = s_bestc;
        if (s_flag || base >= niters) break;
        __syncthreads();
        if (t == 0) {                                         // draw
            const int want = min(HG_B, niters - base);
            int nd = 0, fail = -1;
            for (int h = 0; h < want && fail < 0; ++h) {
                bool found = false;
                for (int att = 0; att < HG_ATTEMPTS && !found; ++att) {
                    for (int i = 0; i < 4;) {
                        const int r = (int)(rng_next(rng) % (unsigned)n);
                        bool dup = false;
                        for (int j = 0; j < i; ++j) dup |= s_idx[h][j] == r;
                        if (dup) continue;
                        s_idx[h][i++] = r;
                    }
                    double X[4], Y[4], u[4], w[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double *p = ent + 4 * (size_t)s_idx[h][i];
                        X[i] = p[0]; Y[i] = p[1]; u[i] = p[2]; w[i] = p[3];
                    }
                    found = subset_ok(X, Y, u, w);
                }
                if (found) nd = h + 1; else fail = h;
            }
            s_nd = nd; s_fail = fail;
        }
        __syncthreads();
        const int nd = s_nd;
        if (t < nd) {                                         // solve
            double H[9];
            const bool ok = homography4(LaneMem{s_lane + t}, &s_perm[0][t], ent, s_idx[t], H);
            s_ok[t] = ok ? 1 : 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) s_model[(size_t)t * 9 + i] = H[i];
        }
        __syncthreads();
        int bound = max(best0, 3);                            // score: wave wv takes samples wv, wv + 4, ...
        for (int h = wv; h < nd; h += HG_BLOCK / 64) {
            int good = 0;
            if (s_ok[h]) {
                double H[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) H[i] = s_model[(size_t)h * 9 + i];
                for (int e0 = 0; e0 < n; e0 += 64) {
                    if (good + (n - e0) <= bound) break;      // cannot be accepted any more (wave-uniform)
                    const int e = e0 + lane;
                    bool in = false;
                    if (e < n) in = is_inlier(H, ent + 4 * (size_t)e, thr2);
                    good += (int)__popcll(__ballot(in));
                }
            }
            if (lane == 0) s_good[h] = good;
            bound = max(bound, good);
        }
        __syncthreads();
        if (t == 0) {                                         // accept, in iteration order
            int nit = niters, best = best0, it = base;
            bool stop = false;
            for (int h = 0; h < nd; ++h) {
                if (base + h >= nit) { stop = true; break; }
                if (s_ok[h] && s_good[h] > max(best, 3)) {
                    best = s_good[h];
                    for (int i = 0; i < 9; ++i) s_best[i] = s_model[(size_t)h * 9 + i];
                    nit = update_num_iters(a.conf, (double)(n - best) / n, 4, nit);
                }
                it = base + h + 1;
            }
            if (!stop && s_fail >= 0) stop = true;            // the attempt cap: OpenCV's loop ends at that iteration
            s_niters = nit; s_bestc = best; s_it = it; s_flag = stop ? 1 : 0;
        }
        __syncthreads();
    }
    __syncthreads();
    const int best = s_bestc;
    if (t == 0 && a.iters) a.iters[v] = s_it;
    if (best == 0) {                                          // no accepted model
        for (int e = t; e < n; e += HG_BLOCK) mask[e] = 0;
        if (t < 9) H_out[t] = 0.0;
        if (t == 0) a.count[v] = -1;
        return;
    }

    // ---- refit on the inliers of the best model (the mask array holds them until the last pass) ----
    double H[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = s_best[i];
    for (int e = t; e < n; e += HG_BLOCK) mask[e] = is_inlier(H, ent + 4 * (size_t)e, thr2) ? 1 : 0;     // read back by the same thread only
    const double cnt = (double)best;
    {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int e = t; e < n; e += HG_BLOCK) {
            if (!mask[e]) continue;
            const double *p = ent + 4 * (size_t)e;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = acc[k] + p[k];
        }
        wg_sums<4>(acc, s_red, s_tot);
    }
    double c[4], s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = s_tot[k] / cnt;
    __syncthreads();
    {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int e = t; e < n; e += HG_BLOCK) {
            if (!mask[e]) continue;
            const double *p = ent + 4 * (size_t)e;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = acc[k] + fabs(p[k] - c[k]);
        }
        wg_sums<4>(acc, s_red, s_tot);
    }
    bool spread = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) { spread &= s_tot[k] >= DBL_EPSILON; s[k] = cnt / s_tot[k]; }
    __syncthreads();
    if (spread) {                                             // uniform over the workgroup
        double acc[HG_NS];
#pragma unroll
        for (int k = 0; k < HG_NS; ++k) acc[k] = 0.0;
        for (int e = t; e < n; e += HG_BLOCK) {
            if (!mask[e]) continue;
            const double *p = ent + 4 * (size_t)e;
            const double A = (p[0] - c[0]) * s[0], B = (p[1] - c[1]) * s[1], x = (p[2] - c[2]) * s[2], y = (p[3] - c[3]) * s[3];
            add28(acc, A, B, 1.0, x, y, x, y);
        }
        wg_sums<HG_NS>(acc, s_red, s_tot);
    }
    if (t == 0) {
        bool ok = spread;
        const LaneMem L{s_lane};
        if (ok) { put_system(L, s_tot); ok = nullvec8(L, &s_perm[0][0]); }
#pragma unroll
        for (int i = 0; i < 9; ++i) s_h[i] = H[i];          // kept when the DLT gives no model
        if (ok) {
            double Hd[9];
            if (denormalise(L, c, s, Hd)) {
#pragma unroll
                for (int i = 0; i < 9; ++i) s_h[i] = Hd[i];
            }
        }
    }
    __syncthreads();
    double h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = s_h[i];
    gn_pass(h, ent, mask, n, s_red, s_tot);
    double cost = s_tot[27];
    for (int step = 0; step < HG_REFINE; ++step) {
        if (t == 0) {
            const LaneMem L{s_lane};
            put_system(L, s_tot);
            bool ok = nullvec8(L, &s_perm[0][0]);
            const double z8 = ok ? L(HG_VEC + 8) : 0.0;
            ok = ok && z8 != 0.0;
            if (ok) {
#pragma unroll
                for (int i = 0; i < 8; ++i) { const double hn = h[i] - L(HG_VEC + i) / z8; ok &= finite_d(hn); s_h[i] = hn; }
            }
            s_go = ok ? 1 : 0;
        }
        __syncthreads();
        if (!s_go) break;
        double hn[9];
#pragma unroll
        for (int i = 0; i < 8; ++i) hn[i] = s_h[i];
        hn[8] = 1.0;
        __syncthreads();
        gn_pass(hn, ent, mask, n, s_red, s_tot);
        if (!(s_tot[27] < cost)) break;
        cost = s_tot[27];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = hn[i];
    }
    __syncthreads();
    int good = 0;
    for (int e0 = wv * 64; e0 < n; e0 += HG_BLOCK) {
        const int e = e0 + lane;
        bool in = false;
        if (e < n) { in = is_inlier(h, ent + 4 * (size_t)e, thr2); mask[e] = in ? 1 : 0; }
        good += (int)__popcll(__ballot(in));
    }
    if (lane == 0) s_cnt[wv] = good;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) H_out[i] = h[i];
        a.count[v] = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
    }
}

// ---- the classification ------------------------------------------------------------------------------------------------

constexpr int CL_NLDS = 4096;         // parallax keys kept in LDS
constexpr int HG_ASIN_TERMS = 30;

struct ClArgs {
    const int64_t *off;
    const int32_t *xy1, *xy2;
    const double *intr1, *intr2, *pose;
    const uint8_t *cmask;
    const int32_t *count_e, *count_h;   // n_pairs x 2, n_pairs
    double *keys;                       // workspace: 1 double per entry
    double max_h_ratio, min_angle;
    int32_t min_inliers;
    double *ratio, *angle;
    int32_t *label;
};

// asin on [0, 1/2]: the power series, summed in order
__device__ __forceinline__ double asin_series(double s)
{
#pragma clang fp contract(off)
    const double z = s * s;
    double t = s, r = s;
    for (int k = 0; k < HG_ASIN_TERMS; ++k) {
        t = (t * z) * ((double)((2 * k + 1) * (2 * k + 1)) / (double)((2 * k + 2) * (2 * k + 3)));
        r = r + t;
    }
    return r;
}

// acos on [0, 1]: 2 asin(sin(theta / 2)), through the complement above 60 degrees
__device__ __forceinline__ double acos_upper(double c)
{
#pragma clang fp contract(off)
    const double s = sqrt((1.0 - c) * 0.5);
    if (s <= 0.5) return 2.0 * asin_series(s);
    return 3.141592653589793 - 4.0 * asin_series(sqrt((1.0 - s) * 0.5));
}

// acos on [-1, 1] from + - * / sqrt only: the host restatement gives the same bits
__device__ __forceinline__ double acos_basic(double c)
{
#pragma clang fp contract(off)
    if (c < 0.0) return 3.141592653589793 - acos_upper(-c);
    return acos_upper(c);
}

__device__ __forceinline__ void bearing(const double *K, int32_t ou, int32_t ov, double *x_out, double *y_out)
{
#pragma clang fp contract(off)
    const double x = ((double)ou - K[2]) / K[0];
    const double y = ((double)ov - K[3]) / K[1];
    const double radius = x * x + y * y;
    const double d = K[4] * radius + (K[5] * radius) * radius;
    *x_out = x - d;
    *y_out = y - d;
}

__global__ __launch_bounds__(HG_BLOCK) void k_tv_classify(ClArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_keys[CL_NLDS], s_K1[6], s_K2[6], s_R[9], s_med;
    __shared__ int32_t s_cnt[HG_BLOCK / 64];
    const int v = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t o0 = a.off[v], n64 = a.off[v + 1] - o0;
    const int n = n64 < 0 ? 0 : (n64 > 0x7fffffff ? 0x7fffffff : (int)n64);
    const int ce = a.count_e[2 * (size_t)v], ch = a.count_h[v];
    if (t < 6) { s_K1[t] = a.intr1[6 * (size_t)v + t]; s_K2[t] = a.intr2[6 * (size_t)v + t]; }
    if (t < 9) s_R[t] = a.pose[12 * (size_t)v + 4 * (t / 3) + t % 3];
    if (t == 0) s_med = 0.0;
    __syncthreads();
    double *keys = n <= CL_NLDS ? s_keys : a.keys + o0;
    const uint8_t *cm = a.cmask + o0;
    const double nan = __builtin_nan("");
    int m = 0;
    for (int e0 = wv * 64; e0 < n; e0 += HG_BLOCK) {
        const int e = e0 + lane;
        bool in = false;
        if (e < n) {
            in = ce > 0 && cm[e] != 0;
            double key = nan;                       // not in the mask: neither counted nor ranked
            if (in) {
                const size_t g = (size_t)(o0 + e);
                double x1, y1, x2, y2;
                bearing(s_K1, a.xy1[2 * g], a.xy1[2 * g + 1], &x1, &y1);
                bearing(s_K2, a.xy2[2 * g], a.xy2[2 * g + 1], &x2, &y2);
                const double a0 = (s_R[0] * x1 + s_R[1] * y1) + s_R[2];
                const double a1 = (s_R[3] * x1 + s_R[4] * y1) + s_R[5];
                const double a2 = (s_R[6] * x1 + s_R[7] * y1) + s_R[8];
                const double dot = (a0 * x2 + a1 * y2) + a2;
                const double na = sqrt((a0 * a0 + a1 * a1) + a2 * a2), nb = sqrt((x2 * x2 + y2 * y2) + 1.0);
                double c = dot / (na * nb);
                if (c != c) key = __builtin_inf();
                else {
                    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
                    key = (180.0 * acos_basic(c)) / 3.1415;
                }
            }
            keys[e] = key;
        }
        m += (int)__popcll(__ballot(in));
    }
    if (lane == 0) s_cnt[wv] = m;
    __syncthreads();                                // (keys in the workspace are read back by this workgroup only)
    m = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
    const int want = (m - 1) / 2;
    for (int e = t; e < n && m > 0; e += HG_BLOCK) {            // rank by counting: exact, whatever the order
        const double ki = keys[e];
        if (ki != ki) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double kj = keys[j];
            rank += (kj < ki || (kj == ki && j < e)) ? 1 : 0;
        }
        if (rank == want) s_med = ki;               // one entry has this rank
    }
    __syncthreads();
    if (t == 0) {
        const double angle = s_med;
        const double ratio = ce > 0 ? (double)max(ch, 0) / (double)ce : 0.0;
        int label;
        if (ce < a.min_inliers || m < a.min_inliers) label = RCN_TV_NO_MODEL;
        else if (ratio >= a.max_h_ratio && angle < a.min_angle) label = RCN_TV_PANORAMIC;
        else if (ratio >= a.max_h_ratio) label = RCN_TV_PLANAR;
        else if (angle < a.min_angle) label = RCN_TV_SMALL_BASELINE;
        else label = RCN_TV_GENERAL;
        a.ratio[v] = ratio; a.angle[v] = angle; a.label[v] = label;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------

int check_h_options(rcn_ctx *ctx, const char *who, const rcn_homography_options *o)
{
    if (!(o->threshold > 0.0) || !(o->confidence > 0.0 && o->confidence < 1.0) || o->max_iterations <= 0) {
        ctx->set_error(std::string(who) + ": threshold > 0, 0 < confidence < 1, max_iterations > 0");
        return RCN_ERR_ARG;
    }
    return RCN_OK;
}

int check_g_options(rcn_ctx *ctx, const char *who, const rcn_twoview_geometry_options *o)
{
    if (!(o->max_h_ratio > 0.0) || o->top_m < 1 || !(o->min_angle == o->min_angle)) {
        ctx->set_error(std::string(who) + ": max_h_ratio > 0, top_m >= 1");
        return RCN_ERR_ARG;
    }
    return RCN_OK;
}

int check_offsets(rcn_ctx *ctx, const char *who, int32_t n_pairs, const int64_t *off)
{
    if (off[0] != 0) { ctx->set_error(std::string(who) + ": off[0] must be 0"); return RCN_ERR_ARG; }
    for (int32_t p = 0; p < n_pairs; ++p)
        if (off[p + 1] < off[p] || off[p + 1] - off[p] > 0x7fffffff) { ctx->set_error(std::string(who) + ": off must be non-decreasing"); return RCN_ERR_ARG; }
    return RCN_OK;
}

int launch_hg(rcn_ctx *ctx, HgArgs a, const rcn_homography_options *o, int32_t n_pairs)
{
    static std::mutex once_mu;
    static std::vector<int> done;                     // devices whose copy of the kernel has the attribute
    {
        std::lock_guard<std::mutex> lk(once_mu);
        if (std::find(done.begin(), done.end(), ctx->device) == done.end()) {
            RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_hg_pair), hipFuncAttributeMaxDynamicSharedMemorySize, (int)HG_LDS_BYTES));
            done.push_back(ctx->device);
        }
    }
    a.thr = o->threshold; a.conf = o->confidence; a.max_iters = o->max_iterations;
    k_hg_pair<<<(unsigned)n_pairs, HG_BLOCK, HG_LDS_BYTES, ctx->stream>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int launch_classify(rcn_ctx *ctx, ClArgs a, const rcn_twoview_geometry_options *g, int32_t n_pairs)
{
    a.max_h_ratio = g->max_h_ratio; a.min_angle = g->min_angle; a.min_inliers = g->min_inliers;
    k_tv_classify<<<(unsigned)n_pairs, HG_BLOCK, 0, ctx->stream>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

size_t al(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" {

void rcn_homography_default_options(rcn_homography_options *o)
{
    if (!o) return;
    o->threshold = 3.0;                 // cv::findHomography(src, dst, RANSAC, 3.0, mask, 2000, 0.995)
    o->confidence = 0.995;
    o->max_iterations = 2000;
    o->reserved = 0;
}

void rcn_twoview_geometry_default_options(rcn_twoview_geometry_options *o)
{
    if (!o) return;
    o->max_h_ratio = 0.8;
    o->min_angle = 1.0;
    o->min_inliers = 15;
    o->top_m = 10;
}

int rcn_homography_ransac(rcn_ctx *ctx, int32_t n_pairs, const int64_t *off, const int32_t *xy1, const int32_t *xy2,
                          const rcn_homography_options *opt, double *H_out, uint8_t *mask_out, int32_t *count_out, int32_t *iterations_out)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_homography_ransac";
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_homography_options o;
    if (opt) o = *opt; else rcn_homography_default_options(&o);
    int rc = check_h_options(ctx, who, &o);
    if (rc) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!off || !H_out || !count_out))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    if (n_pairs == 0) return RCN_OK;
    rc = check_offsets(ctx, who, n_pairs, off);
    if (rc) return rc;
    const int64_t ne = off[n_pairs];
    if (ne > 0 && (!xy1 || !xy2 || !mask_out)) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t np = (size_t)n_pairs, nE = (size_t)ne;
    const size_t b_off = 8 * (np + 1), b_xy = 8 * nE, b_ent = 32 * nE, b_H = 72 * np, b_mask = nE, b_cnt = 4 * np;
    RCN_HIP(ctx->hg_hws.reserve(al(b_off) + 2 * al(b_xy) + al(b_ent) + al(b_H) + al(b_mask) + 2 * al(b_cnt) + 256));
    char *w = ctx->hg_hws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += al(b); return q; };
    int64_t *d_off = (int64_t *)take(b_off);
    int32_t *d_xy1 = (int32_t *)take(b_xy), *d_xy2 = (int32_t *)take(b_xy);
    double *d_ent = (double *)take(b_ent), *d_H = (double *)take(b_H);
    uint8_t *d_mask = (uint8_t *)take(b_mask);
    int32_t *d_cnt = (int32_t *)take(b_cnt), *d_it = (int32_t *)take(b_cnt);
    auto H2D = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    RCN_HIP(H2D(d_off, off, b_off)); RCN_HIP(H2D(d_xy1, xy1, b_xy)); RCN_HIP(H2D(d_xy2, xy2, b_xy));
    HgArgs a{};
    a.off = d_off; a.xy1 = d_xy1; a.xy2 = d_xy2; a.ent = d_ent; a.H = d_H; a.mask = d_mask; a.count = d_cnt; a.iters = d_it;
    rc = launch_hg(ctx, a, &o, n_pairs);
    if (rc) return rc;
    auto D2H = [&](void *dst, const void *src, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    RCN_HIP(D2H(H_out, d_H, b_H)); RCN_HIP(D2H(mask_out, d_mask, b_mask)); RCN_HIP(D2H(count_out, d_cnt, b_cnt)); RCN_HIP(D2H(iterations_out, d_it, b_cnt));
    RCN_HIP(hipStreamSynchronize(st));
    return RCN_OK;
}

int rcn_homography_ransac_device(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pairs, const rcn_homography_options *opt, int64_t capacity,
                                 int64_t *off_dev, int32_t *qt_dev, double *H_dev, uint8_t *mask_dev, int32_t *count_dev, int32_t *iterations_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_homography_ransac_device";
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_homography_options o;
    if (opt) o = *opt; else rcn_homography_default_options(&o);
    int rc = check_h_options(ctx, who, &o);
    if (rc) return rc;
    if (n_pairs < 0 || capacity < 0 || !off_dev || (n_pairs > 0 && (!pairs || !H_dev || !count_dev)) || (capacity > 0 && !mask_dev)) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    RCN_HIP(hipSetDevice(ctx->device));
    const size_t cap = (size_t)std::max<int64_t>(capacity, 1);
    RCN_HIP(ctx->hg_dws.reserve(2 * al(8 * cap) + al(32 * cap) + 256));
    char *w = ctx->hg_dws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += al(b); return q; };
    int32_t *d_xy1 = (int32_t *)take(8 * cap), *d_xy2 = (int32_t *)take(8 * cap);
    double *d_ent = (double *)take(32 * cap);
    rc = rcn_int_pair_fill(ctx, who, n_pairs, pairs, capacity, off_dev, d_xy1, d_xy2, qt_dev);
    if (rc || n_pairs == 0) return rc;
    HgArgs a{};
    a.off = off_dev; a.xy1 = d_xy1; a.xy2 = d_xy2; a.ent = d_ent; a.H = H_dev; a.mask = mask_dev; a.count = count_dev; a.iters = iterations_dev;
    return launch_hg(ctx, a, &o, n_pairs);
}

int rcn_twoview_geometry(rcn_ctx *ctx, int32_t n_pairs, const int64_t *off, const int32_t *xy1, const int32_t *xy2,
                         const double *intr6_1, const double *intr6_2, const rcn_twoview_options *tv_opt,
                         const rcn_homography_options *h_opt, const rcn_twoview_geometry_options *g_opt, double *E_out,
                         double *pose34_out, uint8_t *mask_out, uint8_t *cheir_mask_out, int32_t *count_out, int32_t *iterations_out,
                         double *H_out, uint8_t *h_mask_out, int32_t *h_count_out, int32_t *h_iterations_out, double *ratio_out,
                         double *median_angle_out, int32_t *label_out)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_twoview_geometry";
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_homography_options ho;
    if (h_opt) ho = *h_opt; else rcn_homography_default_options(&ho);
    rcn_twoview_geometry_options go;
    if (g_opt) go = *g_opt; else rcn_twoview_geometry_default_options(&go);
    rcn_twoview_options to;
    if (tv_opt) to = *tv_opt; else rcn_twoview_default_options(&to);
    int rc = check_h_options(ctx, who, &ho);
    if (rc) return rc;
    rc = check_g_options(ctx, who, &go);
    if (rc) return rc;
    rc = rcn_int_twoview_launch(ctx, who, &to, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;                                  // the E search's options
    if (n_pairs < 0 || (n_pairs > 0 && (!off || !intr6_1 || !intr6_2 || !pose34_out || !count_out || !H_out || !h_count_out || !ratio_out || !median_angle_out || !label_out))) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    if (n_pairs == 0) return RCN_OK;
    rc = check_offsets(ctx, who, n_pairs, off);
    if (rc) return rc;
    const int64_t ne = off[n_pairs];
    if (ne > 0 && (!xy1 || !xy2 || !mask_out || !h_mask_out)) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t np = (size_t)n_pairs, nE = (size_t)ne;
    const size_t b_off = 8 * (np + 1), b_xy = 8 * nE, b_intr = 48 * np, b_norm = 32 * nE, b_E = 72 * np, b_pose = 96 * np, b_mask = nE,
                 b_cnt2 = 8 * np, b_cnt = 4 * np, b_d = 8 * np, b_keys = 8 * nE;
    RCN_HIP(ctx->hg_hws.reserve(al(b_off) + 2 * al(b_xy) + 2 * al(b_intr) + 2 * al(b_norm) + 2 * al(b_E) + al(b_pose) + 3 * al(b_mask) + al(b_cnt2) +
                                4 * al(b_cnt) + 2 * al(b_d) + al(b_keys) + 256));
    char *w = ctx->hg_hws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += al(b); return q; };
    int64_t *d_off = (int64_t *)take(b_off);
    int32_t *d_xy1 = (int32_t *)take(b_xy), *d_xy2 = (int32_t *)take(b_xy);
    double *d_i1 = (double *)take(b_intr), *d_i2 = (double *)take(b_intr), *d_norm = (double *)take(b_norm), *d_ent = (double *)take(b_norm),
           *d_E = (double *)take(b_E), *d_H = (double *)take(b_E), *d_pose = (double *)take(b_pose);
    uint8_t *d_mask = (uint8_t *)take(b_mask), *d_cmask = (uint8_t *)take(b_mask), *d_hmask = (uint8_t *)take(b_mask);
    int32_t *d_cnt = (int32_t *)take(b_cnt2), *d_it = (int32_t *)take(b_cnt), *d_hcnt = (int32_t *)take(b_cnt), *d_hit = (int32_t *)take(b_cnt),
            *d_label = (int32_t *)take(b_cnt);
    double *d_ratio = (double *)take(b_d), *d_angle = (double *)take(b_d), *d_keys = (double *)take(b_keys);
    auto H2D = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    RCN_HIP(H2D(d_off, off, b_off)); RCN_HIP(H2D(d_xy1, xy1, b_xy)); RCN_HIP(H2D(d_xy2, xy2, b_xy));
    RCN_HIP(H2D(d_i1, intr6_1, b_intr)); RCN_HIP(H2D(d_i2, intr6_2, b_intr));
    rc = rcn_int_twoview_launch(ctx, who, &to, n_pairs, d_off, d_xy1, d_xy2, d_i1, d_i2, d_norm, d_E, d_pose, d_mask, d_cmask, d_cnt, d_it);
    if (rc) return rc;
    HgArgs a{};
    a.off = d_off; a.xy1 = d_xy1; a.xy2 = d_xy2; a.ent = d_ent; a.H = d_H; a.mask = d_hmask; a.count = d_hcnt; a.iters = d_hit;
    rc = launch_hg(ctx, a, &ho, n_pairs);
    if (rc) return rc;
    ClArgs c{};
    c.off = d_off; c.xy1 = d_xy1; c.xy2 = d_xy2; c.intr1 = d_i1; c.intr2 = d_i2; c.pose = d_pose; c.cmask = d_cmask; c.count_e = d_cnt;
    c.count_h = d_hcnt; c.keys = d_keys; c.ratio = d_ratio; c.angle = d_angle; c.label = d_label;
    rc = launch_classify(ctx, c, &go, n_pairs);
    if (rc) return rc;
    auto D2H = [&](void *dst, const void *src, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    RCN_HIP(D2H(E_out, d_E, b_E)); RCN_HIP(D2H(pose34_out, d_pose, b_pose)); RCN_HIP(D2H(mask_out, d_mask, b_mask));
    RCN_HIP(D2H(cheir_mask_out, d_cmask, b_mask)); RCN_HIP(D2H(count_out, d_cnt, b_cnt2)); RCN_HIP(D2H(iterations_out, d_it, b_cnt));
    RCN_HIP(D2H(H_out, d_H, b_E)); RCN_HIP(D2H(h_mask_out, d_hmask, b_mask)); RCN_HIP(D2H(h_count_out, d_hcnt, b_cnt));
    RCN_HIP(D2H(h_iterations_out, d_hit, b_cnt)); RCN_HIP(D2H(ratio_out, d_ratio, b_d)); RCN_HIP(D2H(median_angle_out, d_angle, b_d));
    RCN_HIP(D2H(label_out, d_label, b_cnt));
    RCN_HIP(hipStreamSynchronize(st));
    return RCN_OK;
}

int rcn_twoview_geometry_device(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pairs, const double *intr6_1_dev, const double *intr6_2_dev,
                                const rcn_twoview_options *tv_opt, const rcn_homography_options *h_opt,
                                const rcn_twoview_geometry_options *g_opt, int64_t capacity, int64_t *off_dev, int32_t *qt_dev,
                                double *E_dev, double *pose34_dev, uint8_t *mask_dev, uint8_t *cheir_mask_dev, int32_t *count_dev,
                                int32_t *iterations_dev, double *H_dev, uint8_t *h_mask_dev, int32_t *h_count_dev,
                                int32_t *h_iterations_dev, double *ratio_dev, double *median_angle_dev, int32_t *label_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_twoview_geometry_device";
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_homography_options ho;
    if (h_opt) ho = *h_opt; else rcn_homography_default_options(&ho);
    rcn_twoview_geometry_options go;
    if (g_opt) go = *g_opt; else rcn_twoview_geometry_default_options(&go);
    rcn_twoview_options to;
    if (tv_opt) to = *tv_opt; else rcn_twoview_default_options(&to);
    int rc = check_h_options(ctx, who, &ho);
    if (rc) return rc;
    rc = check_g_options(ctx, who, &go);
    if (rc) return rc;
    rc = rcn_int_twoview_launch(ctx, who, &to, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;                                  // the E search's options
    if (n_pairs < 0 || capacity < 0 || !off_dev ||
        (n_pairs > 0 && (!pairs || !intr6_1_dev || !intr6_2_dev || !E_dev || !pose34_dev || !count_dev || !H_dev || !h_count_dev || !ratio_dev || !median_angle_dev || !label_dev)) ||
        (capacity > 0 && (!mask_dev || !cheir_mask_dev || !h_mask_dev))) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    RCN_HIP(hipSetDevice(ctx->device));
    const size_t cap = (size_t)std::max<int64_t>(capacity, 1);
    RCN_HIP(ctx->hg_dws.reserve(2 * al(8 * cap) + 2 * al(32 * cap) + al(8 * cap) + 256));
    char *w = ctx->hg_dws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += al(b); return q; };
    int32_t *d_xy1 = (int32_t *)take(8 * cap), *d_xy2 = (int32_t *)take(8 * cap);
    double *d_norm = (double *)take(32 * cap), *d_ent = (double *)take(32 * cap), *d_keys = (double *)take(8 * cap);
    rc = rcn_int_pair_fill(ctx, who, n_pairs, pairs, capacity, off_dev, d_xy1, d_xy2, qt_dev);
    if (rc || n_pairs == 0) return rc;
    rc = rcn_int_twoview_launch(ctx, who, &to, n_pairs, off_dev, d_xy1, d_xy2, intr6_1_dev, intr6_2_dev, d_norm, E_dev, pose34_dev, mask_dev,
                                cheir_mask_dev, count_dev, iterations_dev);
    if (rc) return rc;
    HgArgs a{};
    a.off = off_dev; a.xy1 = d_xy1; a.xy2 = d_xy2; a.ent = d_ent; a.H = H_dev; a.mask = h_mask_dev; a.count = h_count_dev; a.iters = h_iterations_dev;
    rc = launch_hg(ctx, a, &ho, n_pairs);
    if (rc) return rc;
    ClArgs c{};
    c.off = off_dev; c.xy1 = d_xy1; c.xy2 = d_xy2; c.intr1 = intr6_1_dev; c.intr2 = intr6_2_dev; c.pose = pose34_dev; c.cmask = cheir_mask_dev;
    c.count_e = count_dev; c.count_h = h_count_dev; c.keys = d_keys; c.ratio = ratio_dev; c.angle = median_angle_dev; c.label = label_dev;
    return launch_classify(ctx, c, &go, n_pairs);
}

}  // extern "C"
