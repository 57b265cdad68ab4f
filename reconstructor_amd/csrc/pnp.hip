// pnp.hip -- batched P3P-RANSAC view registration with refit behind rcn_pnp_ransac (include/rcn.h).  gfx950, fp64.
//
// SequentialReconstructor::registerImagePnP (SequentialReconstructor.cpp:559-638), i.e. cv::solvePnPRansac in its P3P mode
// followed by an iterative refit on the inliers, for a batch of views in one launch:
//
//   P1 k_pnp_view   one workgroup of 256 threads per view runs the view's whole search:
//        gather   the view's entries (world point, pixel) into LDS while they fit (PNP_NLDS entries of 32 bytes); larger
//                 views read them through the landmark / feature indices every time
//        rounds of PNP_B hypotheses (PNP_B0 in the first)
//          draw     one lane replays the sequential cv::RNG index stream (4 distinct indices per sample)
//          solve    one lane per hypothesis: bearings, Grunert's quartic by Ferrari's method (resolvent cubic by a fixed
//                   number of bisection and guarded Newton steps), rigid motion from the two triangles' frames, the
//                   solution that reprojects the fourth sample entry best
//          score    one wave per hypothesis, lanes over the entries; a hypothesis is dropped once good + remaining <= bound,
//                   bound counting earlier rounds and the wave's own earlier hypotheses of this round: the outcome is the
//                   sequential loop's (exact pruning, as k_fm_score)
//          accept   one lane replays the acceptance rule in iteration order and discards what lies behind the stop
//        mask     the best model's inliers
//        refit    damped Gauss-Newton over six parameters: per-chunk sums of J'J, J'r, r'r (PNP_CHUNK entries per chunk,
//                 one thread per chunk), chunk sums added in chunk order, 6 x 6 Cholesky on one lane
//
// Every operation is a separately rounded IEEE double (contraction off) in one fixed order built from + - * / sqrt;
// tests/pnp_ref.py restates that order and agrees bit for bit.  The one exception is pow / log in update_num_iters.
// The result depends neither on PNP_B nor on the launch geometry.
//
// rcn_pnp_ransac_device: after at most one small host-to-device copy (the coordinates' table, staged in the ctx) the
// entry is one kernel launch on the ctx stream: no host wait, no device-to-host copy, and no allocation once the table's
// buffer is sized (it grows only with the span of uploaded image ids).  The kernel needs no workspace in HBM.
//
// rng_next, update_num_iters and finite_d are ransac.h's, shared with the other two searches.
#include "camgeom.h"
#include "ransac.h"
#include <cstdlib>

#pragma clang fp contract(off)

namespace {

constexpr int PNP_BLOCK = 256;        // 4 waves
constexpr int PNP_B = 64;             // hypotheses per round
constexpr int PNP_NLDS = 4096;        // entries kept in LDS (32 bytes each)
constexpr int PNP_CHUNK = 8;          // entries per chunk of the refit's sums
constexpr int PNP_BISECT = 80, PNP_CUBIC_NEWTON = 3, PNP_QUARTIC_NEWTON = 2;
constexpr int PNP_B0 = 16;            // ... in the first round (most views stop within a few iterations)

struct PnpXY { const int32_t *xy; int32_t K, pad; };     // resident coordinates of one image id

struct PnpArgs {
    const int64_t *off;
    const int32_t *lm;
    const int32_t *xy;          // host entry: the pixel of every entry; NULL: feat / view_img / slots
    const int32_t *feat, *view_img;
    const PnpXY *slots;
    int32_t id_lo, id_span;
    int32_t n_points;
    const double *points, *intr;
    float thr2;
    double conf;
    int32_t max_iters, refine_iters;
    int32_t prune;              // 0 only in the diagnostic build (RCN_PNP_PRUNE=0): score every hypothesis to the end
    double *pose, *rpose;
    uint8_t *mask;
    int32_t *count, *iters;
};

struct Entry { double x, y, z; int32_t ox, oy; };

// the view's entries: LDS, or the arrays themselves
struct View {
    const Entry *lds;           // NULL: read through the indices
    const int32_t *lm, *xy, *feat, *cxy;
    const double *points;
    int32_t n_points, cK;
    __device__ __forceinline__ Entry fetch(int e) const
    {
        Entry r;
        const int32_t l = lm[e];
        bool ok = l >= 0 && l < n_points;
        r.ox = 0; r.oy = 0;
        if (xy) { r.ox = xy[2 * (size_t)e]; r.oy = xy[2 * (size_t)e + 1]; }
        else {
            const int32_t f = feat[e];
            if (f >= 0 && f < cK) { r.ox = cxy[2 * (size_t)f]; r.oy = cxy[2 * (size_t)f + 1]; }
            else ok = false;
        }
        if (ok) { r.x = points[3 * (size_t)l]; r.y = points[3 * (size_t)l + 1]; r.z = points[3 * (size_t)l + 2]; }
        else r.x = r.y = r.z = __builtin_nan("");            // never an inlier, never part of a model
        return r;
    }
    __device__ __forceinline__ Entry get(int e) const { return lds ? lds[e] : fetch(e); }
};

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double pymax(double a, double b) { return b > a ? b : a; }

// Camera.h:79-93 unprojection of the pixel, normalised
__device__ __forceinline__ void bearing(const double *K, int32_t ox, int32_t oy, double *f)
{
#pragma clang fp contract(off)
    double x = ((double)ox - K[2]) / K[0];
    double y = ((double)oy - K[3]) / K[1];
    const double radius = x * x + y * y;
    const double d = K[4] * radius + (K[5] * radius) * radius;
    x = x - d;
    y = y - d;
    const double nrm = sqrt((x * x + y * y) + 1.0);
    f[0] = x / nrm; f[1] = y / nrm; f[2] = 1.0 / nrm;
}

// orthonormal frame of the triangle (A0, A1, A2): rows e1, e2, e3
__device__ __forceinline__ void frame(const double *A0, const double *A1, const double *A2, double (&F)[3][3])
{
#pragma clang fp contract(off)
    double e1[3], d2[3], e3[3];
    for (int i = 0; i < 3; ++i) e1[i] = A1[i] - A0[i];
    const double n1 = sqrt(dot3(e1, e1));
    for (int i = 0; i < 3; ++i) e1[i] = e1[i] / n1;
    for (int i = 0; i < 3; ++i) d2[i] = A2[i] - A0[i];
    cross3(e1, d2, e3);
    const double n3 = sqrt(dot3(e3, e3));
    for (int i = 0; i < 3; ++i) e3[i] = e3[i] / n3;
    cross3(e3, e1, F[1]);
    for (int i = 0; i < 3; ++i) { F[0][i] = e1[i]; F[2][i] = e3[i]; }
}

__device__ __forceinline__ double cubic(double m, double c2, double c1, double c0) { return ((m + c2) * m + c1) * m + c0; }
__device__ __forceinline__ double quartic(double x, double b3, double b2, double b1, double b0) { return (((x + b3) * x + b2) * x + b1) * x + b0; }

// Step 3 of section 17: the model of the sample (entries s[0..3], landmarks l[0..3]) into out[12]; false: no model.
__device__ bool sample_model(const Entry *s, const int32_t *l, const double *K, double *out)
{
#pragma clang fp contract(off)
    for (int a = 1; a < 4; ++a)
        for (int b = 0; b < a; ++b)
            if (l[a] == l[b]) return false;
    double f[3][3], P[3][3];
    for (int k = 0; k < 3; ++k) {
        bearing(K, s[k].ox, s[k].oy, f[k]);
        P[k][0] = s[k].x; P[k][1] = s[k].y; P[k][2] = s[k].z;
    }
    double d12[3], d02[3], d01[3];
    for (int i = 0; i < 3; ++i) { d12[i] = P[1][i] - P[2][i]; d02[i] = P[0][i] - P[2][i]; d01[i] = P[0][i] - P[1][i]; }
    const double a2 = dot3(d12, d12), b2 = dot3(d02, d02), c2 = dot3(d01, d01);
    if (a2 == 0.0 || b2 == 0.0 || c2 == 0.0) return false;
    const double ca = dot3(f[1], f[2]), cb = dot3(f[0], f[2]), cg = dot3(f[0], f[1]);
    const double q = (a2 - c2) / b2, p = (a2 + c2) / b2, rc = c2 / b2, ra = a2 / b2;
    const double A4 = (q - 1.0) * (q - 1.0) - (4.0 * rc) * (ca * ca);
    const double A3 = 4.0 * (((q * (1.0 - q)) * cb - ((1.0 - p) * ca) * cg) + ((2.0 * rc) * (ca * ca)) * cb);
    const double A2 = 2.0 * (((((q * q - 1.0) + (2.0 * (q * q)) * (cb * cb)) + (2.0 * ((b2 - c2) / b2)) * (ca * ca)) - ((4.0 * p) * (ca * cb)) * cg)
                             + (2.0 * ((b2 - a2) / b2)) * (cg * cg));
    const double A1 = 4.0 * (((((-q) * (1.0 + q)) * cb) + ((2.0 * ra) * (cg * cg)) * cb) - ((1.0 - p) * ca) * cg);
    const double A0 = (1.0 + q) * (1.0 + q) - (4.0 * ra) * (cg * cg);
    const double sA = (((A4 + A3) + A2) + A1) + A0;
    if (!finite_d(sA) || A4 == 0.0) return false;
    const double b3 = A3 / A4, b2_ = A2 / A4, b1 = A1 / A4, b0 = A0 / A4;
    const double sh = b3 * 0.25, sh2 = sh * sh;
    const double pp = b2_ - 6.0 * sh2;
    const double qq = (b1 - (2.0 * b2_) * sh) + (8.0 * sh2) * sh;
    const double rr = ((b0 - b1 * sh) + b2_ * sh2) - (3.0 * sh2) * sh2;
    const double k2 = pp, k1 = (pp * pp) * 0.25 - rr, k0 = -((qq * qq) * 0.125);
    double lo = 0.0, hi = 1.0 + pymax(pymax(fabs(k2), fabs(k1)), fabs(k0));
    if (!finite_d(hi)) return false;
    for (int i = 0; i < PNP_BISECT; ++i) {
        const double mid = 0.5 * (lo + hi);
        if (cubic(mid, k2, k1, k0) > 0.0) hi = mid; else lo = mid;
    }
    double m = hi, gm = cubic(m, k2, k1, k0);
    for (int i = 0; i < PNP_CUBIC_NEWTON; ++i) {
        const double dg = (3.0 * m + 2.0 * k2) * m + k1;
        const double mn = m - gm / dg;
        const double gn = cubic(mn, k2, k1, k0);
        if (mn > 0.0 && fabs(gn) < fabs(gm)) { m = mn; gm = gn; }
    }
    const double w = sqrt(2.0 * m);
    const double hq = qq / (2.0 * w);
    const double base = 0.5 * pp + m;
    double Fp[3][3];
    bool have_fp = false, have = false;
    double best_e = __builtin_inf();
    for (int r = 0; r < 4; ++r) {               // y^2 - w y + (base + hq): roots 0, 1; y^2 + w y + (base - hq): roots 2, 3
        const double sign = r < 2 ? 1.0 : -1.0;
        const double cq = base + sign * hq;
        const double disc = w * w - 4.0 * cq;
        if (!(disc >= 0.0)) continue;
        const double sd = sqrt(disc);
        double v = (r & 1) ? 0.5 * (sign * w - sd) - sh : 0.5 * (sign * w + sd) - sh;
        double fv = quartic(v, b3, b2_, b1, b0);
        for (int i = 0; i < PNP_QUARTIC_NEWTON; ++i) {
            const double dv = ((4.0 * v + 3.0 * b3) * v + 2.0 * b2_) * v + b1;
            const double vn = v - fv / dv;
            const double fn = quartic(vn, b3, b2_, b1, b0);
            if (fabs(fn) < fabs(fv)) { v = vn; fv = fn; }
        }
        if (!(v > 0.0)) continue;
        const double den = 2.0 * (cg - v * ca);
        const double u = ((((q - 1.0) * v) * v - ((2.0 * q) * cb) * v) + (1.0 + q)) / den;
        if (!(u > 0.0)) continue;
        const double s1sq = b2 / ((1.0 + v * v) - (2.0 * v) * cb);
        if (!(s1sq > 0.0)) continue;
        const double s1 = sqrt(s1sq), s2 = u * s1, s3 = v * s1;
        double Y[3][3];
        for (int i = 0; i < 3; ++i) { Y[0][i] = s1 * f[0][i]; Y[1][i] = s2 * f[1][i]; Y[2][i] = s3 * f[2][i]; }
        if (!have_fp) { frame(P[0], P[1], P[2], Fp); have_fp = true; }
        double Fy[3][3];
        frame(Y[0], Y[1], Y[2], Fy);
        double pose[12];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) pose[4 * i + j] = (Fy[0][i] * Fp[0][j] + Fy[1][i] * Fp[1][j]) + Fy[2][i] * Fp[2][j];
        for (int i = 0; i < 3; ++i) pose[4 * i + 3] = Y[0][i] - ((pose[4 * i] * P[0][0] + pose[4 * i + 1] * P[0][1]) + pose[4 * i + 2] * P[0][2]);
        bool front = true;
        for (int k = 0; k < 3; ++k) {
            const double z = ((pose[8] * P[k][0] + pose[9] * P[k][1]) + pose[10] * P[k][2]) + pose[11];
            if (!(z > 0.0)) front = false;
        }
        if (!front) continue;
        const double X3[3] = {s[3].x, s[3].y, s[3].z};
        const double e = reproj_sq(pose, K, X3, s[3].ox, s[3].oy);
        if (e < best_e) {
            best_e = e; have = true;
            for (int i = 0; i < 12; ++i) out[i] = pose[i];
        }
    }
    return have;
}

__device__ __forceinline__ bool is_inlier(const double *P, const double *K, const Entry &en, float thr2)
{
    const double X[3] = {en.x, en.y, en.z};
    return (float)reproj_sq(P, K, X, en.ox, en.oy) <= thr2;        // a NaN compares false
}

// the 28 terms of one entry: upper triangle of J'J row by row (21), J'r (6), r'r
__device__ __forceinline__ void refit_terms(const double *P, const double *K, const Entry &en, double *t)
{
#pragma clang fp contract(off)
    double W[3], l[3];
    for (int i = 0; i < 3; ++i) {
        W[i] = (P[4 * i] * en.x + P[4 * i + 1] * en.y) + P[4 * i + 2] * en.z;
        l[i] = W[i] + P[4 * i + 3];
    }
    const double x = l[0] / l[2], y = l[1] / l[2];
    const double radius = x * x + y * y;
    const double d = K[4] * radius + (K[5] * radius) * radius;
    const double xd = x + d, yd = y + d;
    const double ru = (K[0] * xd + K[2]) - (double)en.ox, rv = (K[1] * yd + K[3]) - (double)en.oy;
    const double iz = 1.0 / l[2];
    const double g = 2.0 * (K[4] + (2.0 * K[5]) * radius);
    const double gx = g * x, gy = g * y;
    const double uxx = K[0] * (1.0 + gx), uxy = K[0] * gy, vxx = K[1] * gx, vxy = K[1] * (1.0 + gy);
    const double dY[3][6] = {{0.0, W[2], -W[1], 1.0, 0.0, 0.0}, {-W[2], 0.0, W[0], 0.0, 1.0, 0.0}, {W[1], -W[0], 0.0, 0.0, 0.0, 1.0}};
    double Ju[6], Jv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double dx = (dY[0][k] - x * dY[2][k]) * iz;
        const double dy = (dY[1][k] - y * dY[2][k]) * iz;
        Ju[k] = uxx * dx + uxy * dy;
        Jv[k] = vxx * dx + vxy * dy;
    }
    int q = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int j = k; j < 6; ++j) t[q++] = Ju[k] * Ju[j] + Jv[k] * Jv[j];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[21 + k] = Ju[k] * ru + Jv[k] * rv;
    t[27] = ru * ru + rv * rv;
}

// Sums of NT terms over the view's inliers: one thread per chunk of PNP_CHUNK consecutive entries (entry order, from 0.0),
// the chunk sums added in chunk order from 0.0 by one lane per term: the four waves hand their 64 chunk sums over in turn.
// tot[NT] in LDS is valid for every thread on return.
template <int NT>
__device__ void chunk_sums(const View &vw, int n, const uint8_t *mask, const double *P, const double *K,
                           double (*s_sum)[64], double *tot)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int nch = (n + PNP_CHUNK - 1) / PNP_CHUNK;
    double run = 0.0;                                   // lane t < NT: the running total of term t
    for (int c0 = 0; c0 < nch; c0 += PNP_BLOCK) {
        const int c = c0 + t;
        double acc[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) acc[k] = 0.0;
        if (c < nch) {
            const int e1 = min(n, (c + 1) * PNP_CHUNK);
            for (int e = c * PNP_CHUNK; e < e1; ++e) {
                if (!mask[e]) continue;
                const Entry en = vw.get(e);
                if constexpr (NT == 28) {
                    double tm[28];
                    refit_terms(P, K, en, tm);
#pragma unroll
                    for (int k = 0; k < 28; ++k) acc[k] = acc[k] + tm[k];
                } else {
                    const double X[3] = {en.x, en.y, en.z};
                    acc[0] = acc[0] + reproj_sq(P, K, X, en.ox, en.oy);
                }
            }
        }
        for (int g = 0; g < PNP_BLOCK / 64; ++g) {
            const int cnt = min(64, nch - c0 - 64 * g);
            if (cnt <= 0) break;                        // uniform
            __syncthreads();
            if (wv == g) {
#pragma unroll
                for (int k = 0; k < NT; ++k) s_sum[k][lane] = acc[k];
            }
            __syncthreads();
            if (t < NT) {
                double r = run;
#pragma unroll 8
                for (int i = 0; i < cnt; ++i) r = r + s_sum[t][i];
                run = r;
            }
        }
    }
    __syncthreads();
    if (t < NT) tot[t] = run;
    __syncthreads();
}

__global__ __launch_bounds__(PNP_BLOCK) void k_pnp_view(PnpArgs a)
{
#pragma clang fp contract(off)
    __shared__ Entry s_ent[PNP_NLDS];
    __shared__ double s_model[PNP_B][12];
    __shared__ double s_sum[28][64];
    __shared__ double s_best[12], s_pose[12], s_trial[12], s_tot[28], s_K[6], s_c1[1];
    __shared__ int32_t s_idx[PNP_B][4], s_has[PNP_B], s_good[PNP_B];
    __shared__ int32_t s_niters, s_bestc, s_it, s_flag;

    const int v = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t o0 = a.off[v], n64 = a.off[v + 1] - o0;
    const int n = n64 < 0 ? 0 : (n64 > 0x7fffffff ? 0x7fffffff : (int)n64);
    double *pose_out = a.pose + 12 * (size_t)v;
    double *rpose_out = a.rpose ? a.rpose + 12 * (size_t)v : nullptr;
    uint8_t *mask = a.mask + o0;

    View vw;
    vw.lm = a.lm + o0; vw.xy = a.xy ? a.xy + 2 * o0 : nullptr; vw.feat = a.xy ? nullptr : a.feat + o0;
    vw.points = a.points; vw.n_points = a.n_points; vw.cxy = nullptr; vw.cK = 0; vw.lds = nullptr;
    bool have_img = true;
    if (!a.xy) {
        const int32_t img = a.view_img[v];
        const int64_t s = (int64_t)img - a.id_lo;
        if (s >= 0 && s < a.id_span && a.slots[s].xy) { vw.cxy = a.slots[s].xy; vw.cK = a.slots[s].K; }
        else have_img = false;
    }
    if (t < 6) s_K[t] = a.intr[6 * (size_t)v + t];

    if (n < 4 || !have_img) {                       // step 1
        for (int e = t; e < n; e += PNP_BLOCK) mask[e] = 0;
        if (t < 12) { pose_out[t] = 0.0; if (rpose_out) rpose_out[t] = 0.0; }
        if (t == 0) { a.count[v] = -2; if (a.iters) a.iters[v] = 0; }
        return;
    }
    if (n <= PNP_NLDS) {
        for (int e = t; e < n; e += PNP_BLOCK) s_ent[e] = vw.fetch(e);
        vw.lds = s_ent;
    }
    if (t == 0) { s_niters = a.max_iters; s_bestc = 0; s_it = 0; s_flag = 0; }
    __syncthreads();
    const double *K = s_K;

    unsigned long long rng = 0xffffffffffffffffULL;          // lane 0 owns the stream
    for (;;) {
        const int base = s_it, niters = s_niters, best0 = s_bestc;
        if (s_flag || base >= niters) break;
        __syncthreads();
        const int nd = min(base == 0 ? PNP_B0 : PNP_B, niters - base);
        if (t == 0) {                                         // draw
            for (int h = 0; h < nd; ++h) {
                for (int i = 0; i < 4;) {
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
            Entry s[4];
            int32_t l[4];
            for (int i = 0; i < 4; ++i) { s[i] = vw.get(s_idx[t][i]); l[i] = vw.lm[s_idx[t][i]]; }
            double mdl[12];
            const bool ok = sample_model(s, l, K, mdl);
            s_has[t] = ok ? 1 : 0;
            s_good[t] = 0;
            if (ok) for (int i = 0; i < 12; ++i) s_model[t][i] = mdl[i];
        }
        __syncthreads();
        int bound = max(best0, 3);                            // score: wave wv takes hypotheses wv, wv + 4, ...
        for (int h = wv; h < nd; h += PNP_BLOCK / 64) {
            if (!s_has[h]) continue;
            double P[12];
            for (int i = 0; i < 12; ++i) P[i] = s_model[h][i];
            int good = 0;
            for (int e0 = 0; e0 < n; e0 += 64) {
                if (a.prune && good + (n - e0) <= bound) break;          // cannot be accepted any more (wave-uniform)
                const int e = e0 + lane;
                bool in = false;
                if (e < n) in = is_inlier(P, K, vw.get(e), a.thr2);
                good += (int)__popcll(__ballot(in));
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
                if (s_has[h] && s_good[h] > max(best, 3)) {
                    best = s_good[h];
                    for (int i = 0; i < 12; ++i) s_best[i] = s_model[h][i];
                    nit = update_num_iters(a.conf, (double)(n - best) / n, 4, nit);
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
    if (best == 0) {                                          // step 6: no accepted model
        for (int e = t; e < n; e += PNP_BLOCK) mask[e] = 0;
        if (t < 12) { pose_out[t] = 0.0; if (rpose_out) rpose_out[t] = 0.0; }
        if (t == 0) a.count[v] = -1;
        return;
    }
    {
        double P[12];
        for (int i = 0; i < 12; ++i) P[i] = s_best[i];
        for (int e = t; e < n; e += PNP_BLOCK) mask[e] = is_inlier(P, K, vw.get(e), a.thr2) ? 1 : 0;
    }
    if (t < 12) { s_pose[t] = s_best[t]; if (rpose_out) rpose_out[t] = s_best[t]; }
    if (t == 0) { a.count[v] = best; s_flag = 0; }
    __syncthreads();                                          // the mask bytes are read back below (same workgroup)

    double lam = 1e-3;                                        // refit (every thread tracks lam: uniform control flow)
    for (int it = 0; it < a.refine_iters; ++it) {
        double P[12];
        for (int i = 0; i < 12; ++i) P[i] = s_pose[i];
        chunk_sums<28>(vw, n, mask, P, K, s_sum, s_tot);
        if (t == 0) {
            double A[6][6], L[6][6], g[6], z[6], d[6];
            int q = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int j = k; j < 6; ++j) A[k][j] = s_tot[q++];
#pragma unroll
            for (int k = 0; k < 6; ++k) g[k] = s_tot[21 + k];
            bool pd = true;                                   // every index a constant after unrolling: registers
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double s = A[j][j] + lam * A[j][j];
#pragma unroll
                for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
                if (!(s > 0.0)) pd = false;                   // what follows is computed and thrown away
                L[j][j] = sqrt(s);
#pragma unroll
                for (int i = j + 1; i < 6; ++i) {
                    s = A[j][i];
#pragma unroll
                    for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
                    L[i][j] = s / L[j][j];
                }
            }
            if (!pd) s_flag = 2;
            else {
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    double s = -g[i];
#pragma unroll
                    for (int k = 0; k < i; ++k) s = s - L[i][k] * z[k];
                    z[i] = s / L[i][i];
                }
#pragma unroll
                for (int i = 5; i >= 0; --i) {
                    double s = z[i];
#pragma unroll
                    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * d[k];
                    d[i] = s / L[i][i];
                }
                const double qb = 0.5 * d[0], qc = 0.5 * d[1], qd = 0.5 * d[2];
                const double nrm = sqrt(((1.0 + qb * qb) + qc * qc) + qd * qd);
                const double w = 1.0 / nrm, b = qb / nrm, c = qc / nrm, dd = qd / nrm;
                const double Q[3][3] = {{((w * w + b * b) - c * c) - dd * dd, 2.0 * (b * c - w * dd), 2.0 * (b * dd + w * c)},
                                        {2.0 * (b * c + w * dd), ((w * w - b * b) + c * c) - dd * dd, 2.0 * (c * dd - w * b)},
                                        {2.0 * (b * dd - w * c), 2.0 * (c * dd + w * b), ((w * w - b * b) - c * c) + dd * dd}};
                for (int i = 0; i < 3; ++i) {
                    for (int j = 0; j < 3; ++j) s_trial[4 * i + j] = (Q[i][0] * P[j] + Q[i][1] * P[4 + j]) + Q[i][2] * P[8 + j];
                    s_trial[4 * i + 3] = P[4 * i + 3] + d[3 + i];
                }
            }
        }
        __syncthreads();
        if (s_flag == 2) break;                               // not positive definite: the RANSAC model
        const double c0 = s_tot[27];
        for (int i = 0; i < 12; ++i) P[i] = s_trial[i];
        chunk_sums<1>(vw, n, mask, P, K, s_sum, s_c1);
        const double c1 = s_c1[0];
        bool done = false;
        if (c1 < c0) {
            done = (c0 - c1) <= 1e-14 * c0;
            lam = lam / 10.0;
            __syncthreads();
            if (t < 12) s_pose[t] = s_trial[t];
        } else {
            if ((c1 - c0) <= 1e-14 * c0) done = true;         // rejected, but equal to rounding: converged
            lam = lam * 10.0;
        }
        __syncthreads();
        if (done) break;
    }
    __syncthreads();
    if (t < 12) pose_out[t] = s_flag == 2 ? s_best[t] : s_pose[t];
}

int check_options(rcn_ctx *ctx, const char *who, const rcn_pnp_options *o)
{
    if (!(o->max_projection_error > 0.0) || !(o->confidence > 0.0 && o->confidence < 1.0) || o->max_iterations <= 0 || o->refine_iterations < 0) {
        ctx->set_error(std::string(who) + ": max_projection_error > 0, 0 < confidence < 1, max_iterations > 0, refine_iterations >= 0");
        return RCN_ERR_ARG;
    }
    return RCN_OK;
}

void fill_args(PnpArgs &a, const rcn_pnp_options *o)
{
    a.thr2 = (float)(o->max_projection_error * o->max_projection_error);
    a.conf = o->confidence;
    a.max_iters = o->max_iterations;
    a.refine_iters = o->refine_iterations;
    a.prune = 1;
#ifdef RCN_DIAG
    const char *e = getenv("RCN_PNP_PRUNE");        // tools/pnp_timing.py: what the exact pruning saves
    if (e && e[0] == '0') a.prune = 0;
#endif
}

}  // namespace

// rcn_pnp_ransac with ctx->mu held.  points_dev != NULL: the points are already in HBM (rcn_ba_session_pnp);
// otherwise points_host (n_points x 3) is staged.
int rcn_int_pnp_host(rcn_ctx *ctx, const char *who, int32_t n_views, const int64_t *off, const int32_t *landmark, const int32_t *xy,
                     int32_t n_points, const double *points_host, const double *points_dev, const double *intr6,
                     const rcn_pnp_options *opt, double *pose34_out, double *ransac_pose34_out, uint8_t *mask_out,
                     int32_t *count_out, int32_t *iterations_out)
{
    rcn_pnp_options o;
    if (opt) o = *opt; else rcn_pnp_default_options(&o);
    int rc = check_options(ctx, who, &o);
    if (rc) return rc;
    if (n_views < 0 || n_points < 0 || (n_views > 0 && (!off || !intr6 || !pose34_out || !count_out))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    if (n_views == 0) return RCN_OK;
    if (off[0] != 0) { ctx->set_error(std::string(who) + ": off[0] must be 0"); return RCN_ERR_ARG; }
    for (int32_t v = 0; v < n_views; ++v)
        if (off[v + 1] < off[v] || off[v + 1] - off[v] > 0x7fffffff) { ctx->set_error(std::string(who) + ": off must be non-decreasing"); return RCN_ERR_ARG; }
    const int64_t ne = off[n_views];
    if (ne > 0 && (!landmark || !xy || !mask_out || (!points_host && !points_dev))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    for (int64_t e = 0; e < ne; ++e)
        if (landmark[e] < 0 || landmark[e] >= n_points) { ctx->set_error(std::string(who) + ": landmark index out of range"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t nv = (size_t)n_views, nE = (size_t)ne;
    const size_t b_off = 8 * (nv + 1), b_lm = 4 * nE, b_xy = 8 * nE, b_pts = points_dev ? 0 : 24 * (size_t)n_points, b_intr = 48 * nv,
                 b_pose = 96 * nv, b_mask = nE, b_cnt = 4 * nv;
    RCN_HIP(ctx->pnp_hws.reserve(al(b_off) + al(b_lm) + al(b_xy) + al(b_pts) + al(b_intr) + 2 * al(b_pose) + al(b_mask) + 2 * al(b_cnt) + 256));
    char *w = ctx->pnp_hws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += al(b); return q; };
    int64_t *d_off = (int64_t *)take(b_off);
    int32_t *d_lm = (int32_t *)take(b_lm), *d_xy = (int32_t *)take(b_xy);
    double *d_pts = (double *)take(b_pts), *d_intr = (double *)take(b_intr), *d_pose = (double *)take(b_pose), *d_rpose = (double *)take(b_pose);
    uint8_t *d_mask = (uint8_t *)take(b_mask);
    int32_t *d_cnt = (int32_t *)take(b_cnt), *d_it = (int32_t *)take(b_cnt);
    auto H2D = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    RCN_HIP(H2D(d_off, off, b_off)); RCN_HIP(H2D(d_lm, landmark, b_lm)); RCN_HIP(H2D(d_xy, xy, b_xy));
    RCN_HIP(H2D(d_pts, points_host, b_pts)); RCN_HIP(H2D(d_intr, intr6, b_intr));
    PnpArgs a{};
    a.off = d_off; a.lm = d_lm; a.xy = d_xy; a.n_points = n_points; a.points = points_dev ? points_dev : d_pts; a.intr = d_intr;
    a.pose = d_pose; a.rpose = d_rpose; a.mask = d_mask; a.count = d_cnt; a.iters = d_it;
    fill_args(a, &o);
    k_pnp_view<<<(unsigned)n_views, PNP_BLOCK, 0, st>>>(a);
    RCN_HIP(hipGetLastError());
    auto D2H = [&](void *dst, const void *src, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    RCN_HIP(D2H(pose34_out, d_pose, b_pose)); RCN_HIP(D2H(ransac_pose34_out, d_rpose, b_pose)); RCN_HIP(D2H(mask_out, d_mask, b_mask));
    RCN_HIP(D2H(count_out, d_cnt, b_cnt)); RCN_HIP(D2H(iterations_out, d_it, b_cnt));
    RCN_HIP(hipStreamSynchronize(st));
    return RCN_OK;
}

extern "C" {

void rcn_pnp_default_options(rcn_pnp_options *o)
{
    if (!o) return;
    o->max_projection_error = 4.0;      // SequentialReconstructor.cpp:596
    o->confidence = 0.99;
    o->max_iterations = 10000;
    o->refine_iterations = 20;
}

int rcn_pnp_ransac(rcn_ctx *ctx, int32_t n_views, const int64_t *off, const int32_t *landmark, const int32_t *xy,
                   int32_t n_points, const double *points, const double *intr6, const rcn_pnp_options *opt,
                   double *pose34_out, double *ransac_pose34_out, uint8_t *mask_out, int32_t *count_out, int32_t *iterations_out)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return rcn_int_pnp_host(ctx, "rcn_pnp_ransac", n_views, off, landmark, xy, n_points, points, nullptr, intr6, opt, pose34_out,
                            ransac_pose34_out, mask_out, count_out, iterations_out);
}

int rcn_pnp_ransac_device(rcn_ctx *ctx, int32_t n_views, const int64_t *off_dev, const int32_t *landmark_dev,
                          const int32_t *feat_dev, const int32_t *view_img_dev, int32_t n_points, const double *points_dev,
                          const double *intr6_dev, const rcn_pnp_options *opt, double *pose34_dev, double *ransac_pose34_dev,
                          uint8_t *mask_dev, int32_t *count_dev, int32_t *iterations_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_pnp_options o;
    if (opt) o = *opt; else rcn_pnp_default_options(&o);
    int rc = check_options(ctx, "rcn_pnp_ransac_device", &o);
    if (rc) return rc;
    if (n_views < 0 || n_points < 0 || (n_views > 0 && (!off_dev || !landmark_dev || !feat_dev || !view_img_dev || !intr6_dev || !pose34_dev ||
                                                        !mask_dev || !count_dev || (n_points > 0 && !points_dev)))) {
        ctx->set_error("rcn_pnp_ransac_device: bad argument");
        return RCN_ERR_ARG;
    }
    if (n_views == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the coordinates' table: image id -> (pixels in HBM, K), dense over the ids that have coordinates
    if (!ctx->pnp_ev && hipEventCreateWithFlags(&ctx->pnp_ev, hipEventDisableTiming) != hipSuccess) { ctx->pnp_ev = nullptr; RCN_HIP(hipGetLastError()); }
    if (ctx->pnp_slots_pending) { RCN_HIP(hipEventSynchronize(ctx->pnp_ev)); ctx->pnp_slots_pending = false; }   // the staging buffer is free again
    int32_t id_lo = 0;
    int64_t span = 0;
    if (!ctx->coords.empty()) { id_lo = ctx->coords.begin()->first; span = (int64_t)ctx->coords.rbegin()->first - id_lo + 1; }
    ctx->pnp_slots_host.assign((size_t)std::max<int64_t>(span, 1) * sizeof(PnpXY), 0);
    PnpXY *sd = reinterpret_cast<PnpXY *>(ctx->pnp_slots_host.data());
    for (auto &kv : ctx->coords) { sd[kv.first - id_lo].xy = kv.second.first.as<int32_t>(); sd[kv.first - id_lo].K = kv.second.second; }
    RCN_HIP(ctx->pnp_slots.reserve(ctx->pnp_slots_host.size()));
    RCN_HIP(hipMemcpyAsync(ctx->pnp_slots.p, sd, ctx->pnp_slots_host.size(), hipMemcpyHostToDevice, st));
    RCN_HIP(hipEventRecord(ctx->pnp_ev, st));
    ctx->pnp_slots_pending = true;
    PnpArgs a{};
    a.off = off_dev; a.lm = landmark_dev; a.xy = nullptr; a.feat = feat_dev; a.view_img = view_img_dev;
    a.slots = ctx->pnp_slots.as<PnpXY>(); a.id_lo = id_lo; a.id_span = (int32_t)std::min<int64_t>(span, 0x7fffffff);
    a.n_points = n_points; a.points = points_dev; a.intr = intr6_dev;
    a.pose = pose34_dev; a.rpose = ransac_pose34_dev; a.mask = mask_dev; a.count = count_dev; a.iters = iterations_dev;
    fill_args(a, &o);
    k_pnp_view<<<(unsigned)n_views, PNP_BLOCK, 0, st>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

}  // extern "C"
