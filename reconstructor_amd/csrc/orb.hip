// orb.hip -- FeatureClassic's second detector, cv::ORB::create() (FeatureDetector.cpp:9, :19), on gfx950.  The contract is
// tests/orb_ref.py; every output equals it bit for bit (angle, informative only: 1 fp32 ulp).
//
//   k_orb_base      level 0: the image as bytes (a float image rounded half to even, clamped), any element strides
//   k_orb_resize    level l from level l - 1: cv::resize's 8-bit INTER_LINEAR with the tables of rcn_img_resize_tables (host)
//   k_orb_fast      FAST-9/16 score map: a 64 x 16 tile and its 3-pixel halo in LDS; four-point reject, 16-bit brighter / darker
//                   masks tested for a run of 9 by shift-and-AND, the score from the per-arc minima
//   k_orb_nms       strict 3 x 3 maximum inside the edge border; candidates appended with one atomic per workgroup (wg_rank).
//                   The list's order is free: nothing later depends on it
//   k_orb_select    one workgroup per (image, level): the 2 quota-th largest FAST score from a 256-bin histogram in LDS, the
//                   Harris response of the survivors, the quota-th largest response and the (y, x) order by counting on keys
//   k_orb_emit      one workgroup per image: the cap K across levels (wg_scan_incl), the keypoint fields, the padding
//   k_orb_angle     one wavefront per keypoint: the angle field from the integer moments (the staged detect only: in the fused
//                   call k_orb_describe writes it from the moments it has)
//   k_orb_blur      separable fixed-point 7 x 7 through LDS: the level is read once, the row pass stays in the CU
//   k_orb_describe  one wavefront per keypoint: patch rows dealt to lanes, moments reduced by shuffles (integers: exact in any
//                   order), 4 tests per lane, bytes assembled by shuffles, the row one 128-byte store
//
// Floating point appears twice: the Harris response and the patch direction, both in single fp64 operations that are
// correctly rounded on host and device (+, -, *, /, sqrt); the unit is compiled without contraction.
#include "rcn_internal.h"
#include "wgprim.h"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

#include "orb_layout.h"      // after the pragma: its float arithmetic is part of the contract
#include "orb_pattern.h"

namespace {

constexpr int ORB_TW = 64, ORB_TH = 16;          // tile of the FAST and blur kernels: 256 threads, 4 rows each
constexpr int ORB_PATCH = 31;
constexpr int ORB_GRID = 1024;                   // workgroups per image of the per-keypoint kernels
__constant__ int ORB_UMAX[16] = ORB_UMAX_INIT;

struct OrbTab { int32_t idx; int16_t w0, w1; };

// geometry of one image's pyramid and of its lists, by value to every kernel
struct OrbGeom {
    int n_levels, edge, thr, pad;
    int h[RCN_ORB_MAX_LEVELS], w[RCN_ORB_MAX_LEVELS], quota[RCN_ORB_MAX_LEVELS], active[RCN_ORB_MAX_LEVELS];
    int cap[RCN_ORB_MAX_LEVELS], scap[RCN_ORB_MAX_LEVELS];     // candidates / survivors a level's lists hold
    float scale[RCN_ORB_MAX_LEVELS];
    long long off[RCN_ORB_MAX_LEVELS], bpi;                    // bytes
    long long coff[RCN_ORB_MAX_LEVELS], cper;                  // candidate entries
    long long soff[RCN_ORB_MAX_LEVELS], sper;                  // survivor entries
};

struct OrbLists {
    unsigned *cand;            // [nb][cper]  (y << 16) | x; reused as keep flags by k_orb_select
    unsigned *spos, *kpos;     // [nb][sper]  survivors of the FAST cut; the kept ones in (y, x) order
    double *sresp, *kresp;     // [nb][sper]
    int *ccnt, *kcnt;          // [nb][RCN_ORB_MAX_LEVELS]
    int *ovf;                  // [nb]
};

struct OrbPattern { int8_t t[1024]; };

// ---- pyramid ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_orb_base(const void *img, int dtype, long long si, long long sy, long long sx, int H, int W, uint8_t *pyr, long long bpi)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const long long e = (long long)blockIdx.z * si + (long long)y * sy + (long long)x * sx;
    uint8_t v;
    if (dtype == RCN_ORB_INPUT_U8) v = reinterpret_cast<const uint8_t *>(img)[e];
    else v = (uint8_t)fminf(fmaxf(rintf(reinterpret_cast<const float *>(img)[e]), 0.f), 255.f);
    pyr[(long long)blockIdx.z * bpi + i] = v;
}

__global__ __launch_bounds__(256) void k_orb_resize(uint8_t *pyr, long long bpi, long long src_off, long long dst_off, int sh, int sw, int h, int w,
                                                    const OrbTab *xt, const OrbTab *yt)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    const uint8_t *S = pyr + (long long)blockIdx.z * bpi + src_off;
    const OrbTab X = xt[x], Y = yt[y];
    const int r0 = min(max(Y.idx, 0), sh - 1), r1 = min(max(Y.idx + 1, 0), sh - 1);
    const int x0 = X.idx, x1 = min(X.idx + 1, sw - 1);
    const uint8_t *a = S + (long long)r0 * sw, *b = S + (long long)r1 * sw;
    const int h0 = a[x0] * X.w0 + a[x1] * X.w1, h1 = b[x0] * X.w0 + b[x1] * X.w1;
    const int v = ((Y.w0 * (h0 >> 4)) >> 16) + ((Y.w1 * (h1 >> 4)) >> 16);
    pyr[(long long)blockIdx.z * bpi + dst_off + i] = (uint8_t)min(max((v + 2) >> 2, 0), 255);
}

// ---- FAST ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool orb_run9(unsigned m16)
{
    const unsigned m = m16 | (m16 << 16);
    unsigned x = m & (m >> 1);
    x &= x >> 2;
    x &= x >> 4;
    x &= m >> 8;
    return (x & 0xFFFFu) != 0;
}

// max over the 16 arcs of 9 of the arc's minimum
__device__ __forceinline__ int orb_arc_score(const int *d)
{
    int m2[16], m4[16], best = -256;
#pragma unroll
    for (int i = 0; i < 16; ++i) m2[i] = min(d[i], d[(i + 1) & 15]);
#pragma unroll
    for (int i = 0; i < 16; ++i) m4[i] = min(m2[i], m2[(i + 2) & 15]);
#pragma unroll
    for (int i = 0; i < 16; ++i) best = max(best, min(min(m4[i], m4[(i + 4) & 15]), d[(i + 8) & 15]));
    return best;
}

// c: the pixel inside a tile of row stride S
template <int S>
__device__ __forceinline__ int orb_fast_score(const uint8_t *c, int thr)
{
    const int p = c[0];
    const int q0 = c[-3 * S] - p, q4 = c[3] - p, q8 = c[3 * S] - p, q12 = c[-3] - p;
    const int nb = (q0 > thr) + (q4 > thr) + (q8 > thr) + (q12 > thr), nd = (q0 < -thr) + (q4 < -thr) + (q8 < -thr) + (q12 < -thr);
    if (nb < 2 && nd < 2) return 0;               // a run of 9 holds at least two of the four compass points
    constexpr int OFF[16] = {-3 * S, -3 * S + 1, -2 * S + 2, -S + 3, 3, S + 3, 2 * S + 2, 3 * S + 1, 3 * S, 3 * S - 1, 2 * S - 2, S - 3, -3, -S - 3, -2 * S - 2, -3 * S - 1};
    int d[16];
    unsigned mb = 0, md = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        d[i] = c[OFF[i]] - p;
        mb |= (unsigned)(d[i] > thr) << i;
        md |= (unsigned)(d[i] < -thr) << i;
    }
    int s = 0;
    if (orb_run9(mb)) s = orb_arc_score(d) - 1;
    if (orb_run9(md)) {
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = -d[i];
        s = max(s, orb_arc_score(d) - 1);
    }
    return s;
}

__global__ __launch_bounds__(256) void k_orb_fast(const uint8_t *pyr, uint8_t *scores, long long bpi, long long off, int h, int w, int thr)
{
    constexpr int SW = ORB_TW + 6, SH = ORB_TH + 6;
    __shared__ uint8_t tile[SH * SW];
    const uint8_t *src = pyr + (long long)blockIdx.z * bpi + off;
    const int x0 = blockIdx.x * ORB_TW, y0 = blockIdx.y * ORB_TH, t = threadIdx.x;
    for (int i = t; i < SH * SW; i += 256) {
        const int r = i / SW, c = i - r * SW, gy = y0 - 3 + r, gx = x0 - 3 + c;
        tile[i] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? src[(long long)gy * w + gx] : (uint8_t)0;
    }
    __syncthreads();
    const int lx = t & 63, x = x0 + lx;
    if (x >= w) return;
    uint8_t *dst = scores + (long long)blockIdx.z * bpi + off;
    for (int ly = t >> 6; ly < ORB_TH; ly += 4) {
        const int y = y0 + ly;
        if (y >= h) break;
        int s = 0;
        if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) s = orb_fast_score<SW>(tile + (ly + 3) * SW + lx + 3, thr);
        dst[(long long)y * w + x] = (uint8_t)s;
    }
}

// one thread per pixel of the level's inner rectangle [edge, w - edge) x [edge, h - edge)
__global__ __launch_bounds__(256) void k_orb_nms(const uint8_t *scores, OrbGeom g, int l, OrbLists L)
{
    __shared__ int sh[4];
    __shared__ int s_base;
    const int w = g.w[l], iw = w - 2 * g.edge, ih = g.h[l] - 2 * g.edge;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const uint8_t *s = scores + (long long)blockIdx.z * g.bpi + g.off[l];
    bool keep = false;
    int x = 0, y = 0;
    if (i < (long long)iw * ih) {
        y = (int)(i / iw); x = (int)(i - (long long)y * iw) + g.edge; y += g.edge;
        const uint8_t *c = s + (long long)y * w + x;
        const int v = c[0];
        keep = v > 0 && v > c[-1] && v > c[1] && v > c[-w - 1] && v > c[-w] && v > c[-w + 1] && v > c[w - 1] && v > c[w] && v > c[w + 1];
    }
    int total;
    const int r = wg_rank<256>(keep, sh, total);
    if (threadIdx.x == 0 && total) s_base = atomicAdd(&L.ccnt[blockIdx.z * RCN_ORB_MAX_LEVELS + l], total);
    __syncthreads();
    if (keep && s_base + r < g.cap[l]) L.cand[(long long)blockIdx.z * g.cper + g.coff[l] + s_base + r] = ((unsigned)y << 16) | (unsigned)x;
}

// ---- selection ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double orb_harris(const uint8_t *p, int w, double s4)
{
    int a = 0, b = 0, c = 0;
    for (int dy = -3; dy <= 3; ++dy)
        for (int dx = -3; dx <= 3; ++dx) {
            const uint8_t *q = p + dy * w + dx;
            const int ix = 2 * (q[1] - q[-1]) + (q[-w + 1] - q[-w - 1]) + (q[w + 1] - q[w - 1]);
            const int iy = 2 * (q[w] - q[-w]) + (q[w - 1] - q[-w - 1]) + (q[w + 1] - q[-w + 1]);
            a += ix * ix; b += iy * iy; c += ix * iy;
        }
    const long long det = (long long)a * b - (long long)c * c, tr = (long long)a + b, tr2 = tr * tr;
    return ((double)det - 0.04 * (double)tr2) * s4;
}

__global__ __launch_bounds__(1024) void k_orb_select(const uint8_t *pyr, const uint8_t *scores, OrbGeom g, OrbLists L, double s4)
{
    __shared__ int hist[256];
    __shared__ int sh[16];
    __shared__ int s_cut, s_ns, s_nk;
    const int l = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    int *kcnt = &L.kcnt[img * RCN_ORB_MAX_LEVELS + l];
    const int q = g.quota[l];
    const int n = g.active[l] ? min(L.ccnt[img * RCN_ORB_MAX_LEVELS + l], g.cap[l]) : 0;
    if (n == 0 || q < 1) { if (t == 0) *kcnt = 0; return; }
    const int w = g.w[l];
    const uint8_t *lev = pyr + (long long)img * g.bpi + g.off[l], *sc = scores + (long long)img * g.bpi + g.off[l];
    unsigned *cand = L.cand + (long long)img * g.cper + g.coff[l];
    unsigned *spos = L.spos + (long long)img * g.sper + g.soff[l], *kpos = L.kpos + (long long)img * g.sper + g.soff[l];
    double *sresp = L.sresp + (long long)img * g.sper + g.soff[l], *kresp = L.kresp + (long long)img * g.sper + g.soff[l];

    // the 2 q-th largest FAST score
    if (t < 256) hist[t] = 0;
    if (t == 0) s_nk = 0;
    __syncthreads();
    for (int i = t; i < n; i += 1024) { const unsigned p = cand[i]; atomicAdd(&hist[sc[(long long)(p >> 16) * w + (p & 0xFFFFu)]], 1); }
    __syncthreads();
    if (t == 0) {
        int cut = 0, ns = n;
        if (n > 2 * q) { int acc = 0; for (int s = 255; s >= 0; --s) { acc += hist[s]; if (acc >= 2 * q) { cut = s; ns = acc; break; } } }
        s_cut = cut; s_ns = ns;
    }
    __syncthreads();
    const int cut = s_cut, ns = s_ns;
    if (ns > g.scap[l]) { if (t == 0) { *kcnt = 0; L.ovf[img] = 1; } return; }
    int run = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        unsigned p = 0;
        bool f = false;
        if (i < n) { p = cand[i]; f = (int)sc[(long long)(p >> 16) * w + (p & 0xFFFFu)] >= cut; }
        int total;
        const int r = wg_rank<1024>(f, sh, total);
        if (f) spos[run + r] = p;
        run += total;
    }
    __syncthreads();
    for (int i = t; i < ns; i += 1024) { const unsigned p = spos[i]; sresp[i] = orb_harris(lev + (long long)(p >> 16) * w + (p & 0xFFFFu), w, s4); }
    __syncthreads();
    // the q-th largest response: kept iff fewer than q are strictly larger.  cand now holds the flags.
    for (int i = t; i < ns; i += 1024) {
        const double r = sresp[i];
        int c = 0;
        for (int j = 0; j < ns; ++j) c += sresp[j] > r;
        cand[i] = c < q;
    }
    __syncthreads();
    int mine = 0;
    for (int i = t; i < ns; i += 1024) {
        if (!cand[i]) continue;
        const unsigned p = spos[i];
        int r = 0;
        for (int j = 0; j < ns; ++j) r += cand[j] && spos[j] < p;
        kpos[r] = p; kresp[r] = sresp[i];
        ++mine;
    }
    if (mine) atomicAdd(&s_nk, mine);
    __syncthreads();
    if (t == 0) *kcnt = s_nk;
}

struct OrbOut { float *xy; int32_t *xy_int; float *size, *angle, *resp; int32_t *oct, *counts; int K; };

__global__ __launch_bounds__(1024) void k_orb_emit(OrbGeom g, OrbLists L, OrbOut o)
{
    __shared__ int sh[16];
    __shared__ int pre[RCN_ORB_MAX_LEVELS + 1];
    const int img = blockIdx.x, t = threadIdx.x, K = o.K;
    if (t == 0) { int s = 0; for (int l = 0; l < g.n_levels; ++l) { pre[l] = s; s += L.kcnt[img * RCN_ORB_MAX_LEVELS + l]; } for (int l = g.n_levels; l <= RCN_ORB_MAX_LEVELS; ++l) pre[l] = s; }
    __syncthreads();
    const int total = L.ovf[img] ? 0 : pre[RCN_ORB_MAX_LEVELS];
    if (t == 0) o.counts[img] = L.ovf[img] ? -1 : total;
    const unsigned *kpos = L.kpos + (long long)img * g.sper;
    const double *kresp = L.kresp + (long long)img * g.sper;
    const size_t ob = (size_t)img * K;
    int run = 0;
    for (int base = 0; base < total; base += 1024) {
        const int e = base + t;
        int l = 0, r = 0;
        bool keep = false;
        if (e < total) {
            while (e >= pre[l + 1]) ++l;
            r = e - pre[l];
            keep = true;
            if (total > K) {                          // among the K largest by (response descending, canonical rank ascending)
                const double v = kresp[g.soff[l] + r];
                int c = 0;
                for (int m = 0; m < g.n_levels; ++m) {
                    const double *kr = kresp + g.soff[m];
                    const int nm = pre[m + 1] - pre[m];
                    for (int j = 0; j < nm; ++j) c += kr[j] > v || (kr[j] == v && pre[m] + j < e);
                }
                keep = c < K;
            }
        }
        int tot;
        const int k = run + wg_scan_incl<int, 1024>(keep ? 1 : 0, sh, tot) - 1;
        if (keep) {
            const unsigned p = kpos[g.soff[l] + r];
            const float s = g.scale[l], x = (float)(p & 0xFFFFu) * s, y = (float)(p >> 16) * s;
            o.xy[(ob + k) * 2] = x; o.xy[(ob + k) * 2 + 1] = y;
            o.xy_int[(ob + k) * 2] = (int32_t)x; o.xy_int[(ob + k) * 2 + 1] = (int32_t)y;
            o.size[ob + k] = (float)ORB_PATCH * s;
            o.angle[ob + k] = 0.f;
            o.resp[ob + k] = (float)kresp[g.soff[l] + r];
            o.oct[ob + k] = l;
        }
        run += tot;
    }
    for (int k = min(total, K) + t; k < K; k += 1024) {
        o.xy[(ob + k) * 2] = -1.f; o.xy[(ob + k) * 2 + 1] = -1.f;
        o.xy_int[(ob + k) * 2] = -1; o.xy_int[(ob + k) * 2 + 1] = -1;
        o.size[ob + k] = 0.f; o.angle[ob + k] = 0.f; o.resp[ob + k] = 0.f; o.oct[ob + k] = 0;
    }
}

// ---- direction and descriptor -------------------------------------------------------------------------------------------

// integer moments of the circular patch around c, by the 64 lanes of a wavefront; every lane receives both
__device__ __forceinline__ void orb_wave_moments(const uint8_t *c, int w, int lane, int &m10, int &m01)
{
    int a = 0, b = 0;
    if (lane < ORB_PATCH) {
        const int v = lane - ORB_HALF, d = ORB_UMAX[v < 0 ? -v : v];
        const uint8_t *row = c + v * w;
        int sum = 0;
        for (int u = -d; u <= d; ++u) { const int p = row[u]; a += u * p; sum += p; }
        b = v * sum;
    }
    for (int o = 32; o; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    m10 = a; m01 = b;
}

// the level pixel an emitted keypoint stands on
__device__ __forceinline__ void orb_level_xy(const float *xy, float scale, int &x, int &y)
{
    x = (int)rint((double)xy[0] / (double)scale);
    y = (int)rint((double)xy[1] / (double)scale);
}

__device__ __forceinline__ bool orb_inside(const OrbGeom &g, int l, int x, int y)
{
    return l >= 0 && l < g.n_levels && g.active[l] && x >= g.edge && x < g.w[l] - g.edge && y >= g.edge && y < g.h[l] - g.edge;
}

// the angle field: fp64 atan2 in degrees in [0, 360), rounded to fp32.  Informative: no decision reads it
__device__ __forceinline__ float orb_angle(int m10, int m01)
{
    double a = atan2((double)m01, (double)m10) * 57.29577951308232;
    if (a < 0.0) a = a + 360.0;
    const float f = (float)a;
    return f >= 360.f ? 0.f : f;
}

__global__ __launch_bounds__(64) void k_orb_angle(const uint8_t *pyr, OrbGeom g, const float *xy, const int32_t *oct, const int32_t *counts, float *angle, int K)
{
    const int img = blockIdx.y, lane = threadIdx.x, m = min(max(counts[img], 0), K);
    for (int k = blockIdx.x; k < m; k += gridDim.x) {
        const size_t e = (size_t)img * K + k;
        const int l = oct[e];
        int x, y, m10, m01;
        orb_level_xy(xy + 2 * e, g.scale[min(max(l, 0), RCN_ORB_MAX_LEVELS - 1)], x, y);
        if (!orb_inside(g, l, x, y)) continue;
        orb_wave_moments(pyr + (long long)img * g.bpi + g.off[l] + (long long)y * g.w[l] + x, g.w[l], lane, m10, m01);
        if (lane == 0) angle[e] = orb_angle(m10, m01);
    }
}

__global__ __launch_bounds__(256) void k_orb_blur(const uint8_t *pyr, uint8_t *blur, long long bpi, long long off, int h, int w)
{
    constexpr int SW = ORB_TW + 6, SH = ORB_TH + 6;
    __shared__ uint8_t tile[SH * SW];
    __shared__ uint16_t rows[SH * ORB_TW];
    const uint8_t *src = pyr + (long long)blockIdx.z * bpi + off;
    const int x0 = blockIdx.x * ORB_TW, y0 = blockIdx.y * ORB_TH, t = threadIdx.x;
    for (int i = t; i < SH * SW; i += 256) {
        const int r = i / SW, c = i - r * SW;
        int gy = y0 - 3 + r, gx = x0 - 3 + c;
        gy = gy < 0 ? -gy : gy >= h ? 2 * h - 2 - gy : gy;           // reflect-101
        gx = gx < 0 ? -gx : gx >= w ? 2 * w - 2 - gx : gx;
        gy = min(max(gy, 0), h - 1); gx = min(max(gx, 0), w - 1);    // beyond the reflection: a pixel no output reads
        tile[i] = src[(long long)gy * w + gx];
    }
    __syncthreads();
    for (int i = t; i < SH * ORB_TW; i += 256) {
        const int r = i >> 6, c = i & 63;
        const uint8_t *p = tile + r * SW + c;
        int s = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) s += ORB_BLUR_W[k] * p[k];
        rows[i] = (uint16_t)s;
    }
    __syncthreads();
    const int lx = t & 63, x = x0 + lx;
    if (x >= w) return;
    uint8_t *dst = blur + (long long)blockIdx.z * bpi + off;
    for (int ly = t >> 6; ly < ORB_TH; ly += 4) {
        const int y = y0 + ly;
        if (y >= h) break;
        int v = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) v += ORB_BLUR_W[k] * rows[(ly + k) * ORB_TW + lx];
        dst[(long long)y * w + x] = (uint8_t)((v + (1 << 15)) >> 16);
    }
}

__global__ __launch_bounds__(64) void k_orb_describe(const uint8_t *pyr, const uint8_t *blur, OrbGeom g, OrbPattern pat, const float *xy, const int32_t *oct,
                                                     const int32_t *counts, float *rows, uint8_t *bytes, float *angle, int K)
{
    const int img = blockIdx.y, lane = threadIdx.x, m = min(max(counts[img], 0), K);
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const size_t e = (size_t)img * K + k;
        unsigned byte = 0;
        if (k < m) {
            const int l = oct[e];
            int x, y, m10, m01;
            orb_level_xy(xy + 2 * e, g.scale[min(max(l, 0), RCN_ORB_MAX_LEVELS - 1)], x, y);
            if (orb_inside(g, l, x, y)) {
                const int w = g.w[l];
                const long long at = (long long)img * g.bpi + g.off[l] + (long long)y * w + x;
                orb_wave_moments(pyr + at, w, lane, m10, m01);
                if (angle && lane == 0) angle[e] = orb_angle(m10, m01);      // the fused call: the moments are here already
                const long long h2 = (long long)m10 * m10 + (long long)m01 * m01;
                double cs = 1.0, sn = 0.0;
                if (h2) { const double r = sqrt((double)h2); cs = (double)m10 / r; sn = (double)m01 / r; }
                const uint8_t *c = blur + at;
                unsigned nib = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int8_t *q = pat.t + (lane * 4 + j) * 4;
                    const double ax = q[0], ay = q[1], bx = q[2], by = q[3];
                    const int ix0 = (int)rint(ax * cs - ay * sn), iy0 = (int)rint(ax * sn + ay * cs);
                    const int ix1 = (int)rint(bx * cs - by * sn), iy1 = (int)rint(bx * sn + by * cs);
                    nib |= (unsigned)(c[iy0 * w + ix0] < c[iy1 * w + ix1]) << j;
                }
                const unsigned hi = __shfl_down(nib, 1);
                const unsigned b2 = nib | (hi << 4);              // valid in the even lanes: byte lane / 2
                byte = __shfl(b2, (lane & 31) * 2);
            }
        }
        if (lane < 32) {
            rows[e * 32 + lane] = (float)byte;
            if (bytes) bytes[e * 32 + lane] = (uint8_t)byte;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

size_t orb_align(size_t b) { return (b + 255) & ~(size_t)255; }

void orb_geom(const rcn_orb_pyramid_layout &L, const rcn_orb_options &o, OrbGeom *g)
{
    std::memset(g, 0, sizeof *g);
    g->n_levels = L.n_levels; g->edge = o.edge_threshold; g->thr = o.fast_threshold; g->bpi = L.bytes_per_image;
    long long c = 0, s = 0;
    for (int l = 0; l < L.n_levels; ++l) {
        g->h[l] = L.level_h[l]; g->w[l] = L.level_w[l]; g->quota[l] = L.quota[l]; g->active[l] = L.active[l];
        g->scale[l] = L.scale[l]; g->off[l] = L.level_offset[l];
        // strict 3 x 3 maxima are at most one per 2 x 2 block of the inner rectangle
        const long long iw = std::max(L.level_w[l] - 2 * o.edge_threshold, 0), ih = std::max(L.level_h[l] - 2 * o.edge_threshold, 0);
        g->cap[l] = L.active[l] ? (int)(((iw + 1) / 2) * ((ih + 1) / 2)) : 0;
        g->scap[l] = std::min(g->cap[l], RCN_ORB_MAX_SURVIVORS);
        g->coff[l] = c; c += (g->cap[l] + 3) & ~3;
        g->soff[l] = s; s += (g->scap[l] + 3) & ~3;
    }
    g->cper = c; g->sper = s;
}

// per-image bytes of the workspace behind the pyramid: score map, blurred levels, lists
size_t orb_ws_per_image(const OrbGeom &g) { return 2 * (size_t)g.bpi + (size_t)g.cper * 4 + (size_t)g.sper * 24 + 2 * RCN_ORB_MAX_LEVELS * 4 + 4; }

struct OrbWs { uint8_t *scores, *blur; OrbLists l; };
size_t orb_ws_total(const OrbGeom &g, int32_t nb)
{
    const size_t n = (size_t)nb;
    return 2 * orb_align(n * g.bpi) + orb_align(n * g.cper * 4) + 2 * orb_align(n * g.sper * 4) + 2 * orb_align(n * g.sper * 8) +
           2 * orb_align(n * RCN_ORB_MAX_LEVELS * 4) + orb_align(n * 4);
}
OrbWs orb_ws_at(char *p, const OrbGeom &g, int32_t nb)
{
    const size_t n = (size_t)nb;
    OrbWs w;
    w.scores = reinterpret_cast<uint8_t *>(p);   p += orb_align(n * g.bpi);
    w.blur = reinterpret_cast<uint8_t *>(p);     p += orb_align(n * g.bpi);
    w.l.sresp = reinterpret_cast<double *>(p);   p += orb_align(n * g.sper * 8);
    w.l.kresp = reinterpret_cast<double *>(p);   p += orb_align(n * g.sper * 8);
    w.l.cand = reinterpret_cast<unsigned *>(p);  p += orb_align(n * g.cper * 4);
    w.l.spos = reinterpret_cast<unsigned *>(p);  p += orb_align(n * g.sper * 4);
    w.l.kpos = reinterpret_cast<unsigned *>(p);  p += orb_align(n * g.sper * 4);
    w.l.ccnt = reinterpret_cast<int *>(p);       p += orb_align(n * RCN_ORB_MAX_LEVELS * 4);
    w.l.kcnt = reinterpret_cast<int *>(p);       p += orb_align(n * RCN_ORB_MAX_LEVELS * 4);
    w.l.ovf = reinterpret_cast<int *>(p);
    return w;
}

int32_t orb_chunk(rcn_ctx *ctx, int32_t n, size_t per_image)
{
    const int32_t cap = 65535;                                           // grid.z
    if (ctx->orb_chunk_images > 0) return std::min({n, ctx->orb_chunk_images, cap});
    const size_t budget = (size_t)1 << 30;
    return (int32_t)std::max<size_t>(1, std::min<size_t>({(size_t)n, budget / std::max<size_t>(per_image, 1), (size_t)cap}));
}

// the resize tables of levels 1 .. n - 1 in ctx->orb_tab: level l's x table, then its y table.  Built and uploaded when the
// level sizes differ from the last call's (waits for the stream on both sides of the copy: the host copy dies here).
int orb_tables(rcn_ctx *ctx, const rcn_orb_pyramid_layout &L, std::vector<size_t> *at)
{
    std::vector<int64_t> key;
    size_t n = 0;
    at->assign((size_t)L.n_levels, 0);
    for (int l = 0; l < L.n_levels; ++l) { key.push_back(L.level_h[l]); key.push_back(L.level_w[l]); if (l) { (*at)[(size_t)l] = n; n += (size_t)L.level_w[l] + L.level_h[l]; } }
    if (key == ctx->orb_tab_key || n == 0) return RCN_OK;
    std::vector<OrbTab> host(n);
    std::vector<int32_t> idx;
    std::vector<int16_t> wt;
    auto fill = [&](int src, int dst, int horizontal, OrbTab *out) {
        idx.resize((size_t)dst); wt.resize(2 * (size_t)dst);
        if (rcn_img_resize_tables(src, dst, horizontal, idx.data(), wt.data(), nullptr) != RCN_OK) return false;
        for (int i = 0; i < dst; ++i) out[i] = OrbTab{idx[(size_t)i], wt[2 * (size_t)i], wt[2 * (size_t)i + 1]};
        return true;
    };
    for (int l = 1; l < L.n_levels; ++l)
        if (!fill(L.level_w[l - 1], L.level_w[l], 1, host.data() + (*at)[(size_t)l]) ||
            !fill(L.level_h[l - 1], L.level_h[l], 0, host.data() + (*at)[(size_t)l] + L.level_w[l])) {
            ctx->set_error("rcn_orb: the resize tables could not be built");
            return RCN_ERR_ARG;
        }
    RCN_HIP(rcn_int_stream_wait(ctx));
    ctx->orb_tab_key.clear();
    RCN_HIP(ctx->orb_tab.reserve(n * sizeof(OrbTab)));
    RCN_HIP(hipMemcpyAsync(ctx->orb_tab.p, host.data(), n * sizeof(OrbTab), hipMemcpyHostToDevice, ctx->stream));
    RCN_HIP(rcn_int_stream_wait(ctx));
    ctx->orb_tab_key = key;
    return RCN_OK;
}

unsigned orb_blocks(long long items) { return (unsigned)((items + 255) / 256); }

int orb_pyramid_launch(rcn_ctx *ctx, const rcn_orb_pyramid_layout &L, const std::vector<size_t> &at, const void *img, int32_t dtype, int64_t si, int64_t sy,
                       int64_t sx, int32_t first, int32_t m, uint8_t *pyr)
{
    const int H = L.level_h[0], W = L.level_w[0];
    const size_t esz = dtype == RCN_ORB_INPUT_U8 ? 1 : 4;
    const void *src = reinterpret_cast<const char *>(img) + (int64_t)first * si * (int64_t)esz;
    k_orb_base<<<dim3(orb_blocks((long long)H * W), 1, (unsigned)m), 256, 0, ctx->stream>>>(src, dtype, si, sy, sx, H, W, pyr, L.bytes_per_image);
    const OrbTab *tab = ctx->orb_tab.as<OrbTab>();
    for (int l = 1; l < L.n_levels; ++l)
        k_orb_resize<<<dim3(orb_blocks((long long)L.level_h[l] * L.level_w[l]), 1, (unsigned)m), 256, 0, ctx->stream>>>(
            pyr, L.bytes_per_image, L.level_offset[l - 1], L.level_offset[l], L.level_h[l - 1], L.level_w[l - 1], L.level_h[l], L.level_w[l],
            tab + at[(size_t)l], tab + at[(size_t)l] + L.level_w[l]);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

dim3 orb_tiles(const OrbGeom &g, int l, int32_t m) { return dim3((unsigned)((g.w[l] + ORB_TW - 1) / ORB_TW), (unsigned)((g.h[l] + ORB_TH - 1) / ORB_TH), (unsigned)m); }

int orb_fast_launch(rcn_ctx *ctx, const OrbGeom &g, const uint8_t *pyr, int32_t m, uint8_t *scores, bool all_levels)
{
    for (int l = 0; l < g.n_levels; ++l)
        if (all_levels || g.active[l]) k_orb_fast<<<orb_tiles(g, l, m), 256, 0, ctx->stream>>>(pyr, scores, g.bpi, g.off[l], g.h[l], g.w[l], g.thr);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

double orb_s4()
{
    const double s = 1.0 / (4 * 7 * 255.0);
    return s * s * s * s;
}

// with_angle: false in the fused call, where k_orb_describe writes the angle field from the moments it computes anyway
int orb_detect_launch(rcn_ctx *ctx, const OrbGeom &g, const uint8_t *pyr, int32_t m, const OrbWs &ws, const OrbOut &o, bool with_angle)
{
    const size_t counters = (size_t)m * RCN_ORB_MAX_LEVELS * 4;
    RCN_HIP(hipMemsetAsync(ws.l.ccnt, 0, counters, ctx->stream));
    RCN_HIP(hipMemsetAsync(ws.l.ovf, 0, (size_t)m * 4, ctx->stream));
    if (int rc = orb_fast_launch(ctx, g, pyr, m, ws.scores, false)) return rc;
    for (int l = 0; l < g.n_levels; ++l) {
        if (!g.active[l]) continue;
        const long long inner = (long long)(g.w[l] - 2 * g.edge) * (g.h[l] - 2 * g.edge);
        k_orb_nms<<<dim3(orb_blocks(inner), 1, (unsigned)m), 256, 0, ctx->stream>>>(ws.scores, g, l, ws.l);
    }
    k_orb_select<<<dim3((unsigned)g.n_levels, (unsigned)m), 1024, 0, ctx->stream>>>(pyr, ws.scores, g, ws.l, orb_s4());
    k_orb_emit<<<(unsigned)m, 1024, 0, ctx->stream>>>(g, ws.l, o);
    if (with_angle) k_orb_angle<<<dim3((unsigned)std::min(o.K, ORB_GRID), (unsigned)m), 64, 0, ctx->stream>>>(pyr, g, o.xy, o.oct, o.counts, o.angle, o.K);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int orb_describe_launch(rcn_ctx *ctx, const OrbGeom &g, const OrbPattern &pat, const uint8_t *pyr, int32_t m, uint8_t *blur, int32_t K, const float *xy,
                        const int32_t *oct, const int32_t *counts, float *rows, uint8_t *bytes, float *angle)
{
    for (int l = 0; l < g.n_levels; ++l)
        if (g.active[l]) k_orb_blur<<<orb_tiles(g, l, m), 256, 0, ctx->stream>>>(pyr, blur, g.bpi, g.off[l], g.h[l], g.w[l]);
    k_orb_describe<<<dim3((unsigned)std::min(K, ORB_GRID), (unsigned)m), 64, 0, ctx->stream>>>(pyr, blur, g, pat, xy, oct, counts, rows, bytes, angle, K);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

// the checks every device entry shares; fills the layout, the options in use, the geometry and the pattern
bool orb_common(rcn_ctx *ctx, const char *who, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, int32_t K, bool nulls, rcn_orb_pyramid_layout *L,
                OrbGeom *g, OrbPattern *pat)
{
    rcn_orb_options use;
    const char *why = n < 0 ? "n < 0" : orb_layout_fill(H, W, opt, L, &use);
    if (!why) why = K < 1 ? "K < 1" : nulls ? "null pointer" : nullptr;
    if (why) { ctx->set_error(std::string(who) + ": bad argument (" + why + ")"); return false; }
    orb_geom(*L, use, g);
    if (pat) std::memcpy(pat->t, use.pattern ? use.pattern : orb_default_pattern_table, 1024);
    return true;
}

bool orb_dtype_ok(rcn_ctx *ctx, const char *who, int32_t dtype)
{
    if (dtype == RCN_ORB_INPUT_F32 || dtype == RCN_ORB_INPUT_U8) return true;
    ctx->set_error(std::string(who) + ": bad argument (unknown input dtype)");
    return false;
}

}  // namespace

extern "C" void rcn_orb_default_options(rcn_orb_options *opt)
{
    if (opt) orb_defaults(opt);
}

extern "C" const int8_t *rcn_orb_default_pattern(void) { return orb_default_pattern_table; }

extern "C" int rcn_orb_layout(int32_t H, int32_t W, const rcn_orb_options *opt, rcn_orb_pyramid_layout *out)
{
    if (!out) return RCN_ERR_ARG;
    rcn_orb_pyramid_layout L;
    if (orb_layout_fill(H, W, opt, &L, nullptr)) return RCN_ERR_ARG;
    *out = L;
    return RCN_OK;
}

extern "C" int rcn_orb_set_chunk_images(rcn_ctx *ctx, int32_t images)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->orb_chunk_images = images > 0 ? images : 0;
    return RCN_OK;
}

extern "C" int rcn_orb_pyramid_device(rcn_ctx *ctx, const void *images_dev, int32_t input_dtype, int64_t stride_img, int64_t stride_y,
                                      int64_t stride_x, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, uint8_t *pyr_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_orb_pyramid_device";
    rcn_orb_pyramid_layout L;
    OrbGeom g;
    if (!orb_common(ctx, who, n, H, W, opt, 1, n > 0 && (!images_dev || !pyr_out_dev), &L, &g, nullptr)) return RCN_ERR_ARG;
    if (!orb_dtype_ok(ctx, who, input_dtype)) return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    std::vector<size_t> at;
    if (int rc = orb_tables(ctx, L, &at)) return rc;
    for (int32_t first = 0; first < n; first += 65535)
        if (int rc = orb_pyramid_launch(ctx, L, at, images_dev, input_dtype, stride_img, stride_y, stride_x, first, std::min(65535, n - first),
                                        pyr_out_dev + (int64_t)first * L.bytes_per_image)) return rc;
    return RCN_OK;
}

extern "C" int rcn_orb_fast_device(rcn_ctx *ctx, const uint8_t *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, uint8_t *scores_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_orb_pyramid_layout L;
    OrbGeom g;
    if (!orb_common(ctx, "rcn_orb_fast_device", n, H, W, opt, 1, n > 0 && (!pyr_dev || !scores_out_dev), &L, &g, nullptr)) return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(hipMemsetAsync(scores_out_dev, 0, (size_t)n * L.bytes_per_image, ctx->stream));      // the padding between levels
    for (int32_t first = 0; first < n; first += 65535)
        if (int rc = orb_fast_launch(ctx, g, pyr_dev + (int64_t)first * L.bytes_per_image, std::min(65535, n - first),
                                     scores_out_dev + (int64_t)first * L.bytes_per_image, true)) return rc;
    return RCN_OK;
}

extern "C" int rcn_orb_detect_device(rcn_ctx *ctx, const uint8_t *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, int32_t K,
                                     float *xy_dev, int32_t *xy_int_dev, float *size_dev, float *angle_dev, float *response_dev, int32_t *octave_dev,
                                     int32_t *counts_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_orb_pyramid_layout L;
    OrbGeom g;
    if (!orb_common(ctx, "rcn_orb_detect_device", n, H, W, opt, K,
                    n > 0 && (!pyr_dev || !xy_dev || !xy_int_dev || !size_dev || !angle_dev || !response_dev || !octave_dev || !counts_dev), &L, &g, nullptr))
        return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    const int32_t nb = orb_chunk(ctx, n, orb_ws_per_image(g));
    RCN_HIP(ctx->orb_ws.reserve(orb_ws_total(g, nb)));
    const OrbWs ws = orb_ws_at(ctx->orb_ws.as<char>(), g, nb);
    for (int32_t first = 0; first < n; first += nb) {
        const size_t ob = (size_t)first * K;
        const OrbOut o{xy_dev + ob * 2, xy_int_dev + ob * 2, size_dev + ob, angle_dev + ob, response_dev + ob, octave_dev + ob, counts_dev + first, K};
        if (int rc = orb_detect_launch(ctx, g, pyr_dev + (int64_t)first * L.bytes_per_image, std::min(nb, n - first), ws, o, true)) return rc;
    }
    return RCN_OK;
}

extern "C" int rcn_orb_describe_device(rcn_ctx *ctx, const uint8_t *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, int32_t K,
                                       const float *xy_dev, const int32_t *octave_dev, const int32_t *counts_dev, float *rows_out_dev, uint8_t *bytes_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rcn_orb_pyramid_layout L;
    OrbGeom g;
    OrbPattern pat;
    if (!orb_common(ctx, "rcn_orb_describe_device", n, H, W, opt, K, n > 0 && (!pyr_dev || !xy_dev || !octave_dev || !counts_dev || !rows_out_dev), &L, &g, &pat))
        return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    const int32_t nb = orb_chunk(ctx, n, orb_ws_per_image(g));
    RCN_HIP(ctx->orb_ws.reserve(orb_ws_total(g, nb)));
    const OrbWs ws = orb_ws_at(ctx->orb_ws.as<char>(), g, nb);
    for (int32_t first = 0; first < n; first += nb) {
        const size_t ob = (size_t)first * K;
        if (int rc = orb_describe_launch(ctx, g, pat, pyr_dev + (int64_t)first * L.bytes_per_image, std::min(nb, n - first), ws.blur, K, xy_dev + ob * 2,
                                         octave_dev + ob, counts_dev + first, rows_out_dev + ob * 32, bytes_out_dev ? bytes_out_dev + ob * 32 : nullptr, nullptr)) return rc;
    }
    return RCN_OK;
}

extern "C" int rcn_orb_detect_and_compute_device(rcn_ctx *ctx, const void *images_dev, int32_t input_dtype, int64_t stride_img, int64_t stride_y,
                                                 int64_t stride_x, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, int32_t K,
                                                 float *xy_dev, int32_t *xy_int_dev, float *size_dev, float *angle_dev, float *response_dev,
                                                 int32_t *octave_dev, int32_t *counts_dev, float *rows_out_dev, uint8_t *bytes_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_orb_detect_and_compute_device";
    rcn_orb_pyramid_layout L;
    OrbGeom g;
    OrbPattern pat;
    if (!orb_common(ctx, who, n, H, W, opt, K,
                    n > 0 && (!images_dev || !xy_dev || !xy_int_dev || !size_dev || !angle_dev || !response_dev || !octave_dev || !counts_dev || !rows_out_dev),
                    &L, &g, &pat)) return RCN_ERR_ARG;
    if (!orb_dtype_ok(ctx, who, input_dtype)) return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    std::vector<size_t> at;
    if (int rc = orb_tables(ctx, L, &at)) return rc;
    const int32_t nb = orb_chunk(ctx, n, orb_ws_per_image(g) + (size_t)g.bpi);
    RCN_HIP(ctx->orb_pyr.reserve((size_t)g.bpi * (size_t)nb));
    RCN_HIP(ctx->orb_ws.reserve(orb_ws_total(g, nb)));
    uint8_t *pyr = ctx->orb_pyr.as<uint8_t>();
    const OrbWs ws = orb_ws_at(ctx->orb_ws.as<char>(), g, nb);
    for (int32_t first = 0; first < n; first += nb) {
        const int32_t m = std::min(nb, n - first);
        const size_t ob = (size_t)first * K;
        const OrbOut o{xy_dev + ob * 2, xy_int_dev + ob * 2, size_dev + ob, angle_dev + ob, response_dev + ob, octave_dev + ob, counts_dev + first, K};
        if (int rc = orb_pyramid_launch(ctx, L, at, images_dev, input_dtype, stride_img, stride_y, stride_x, first, m, pyr)) return rc;
        if (int rc = orb_detect_launch(ctx, g, pyr, m, ws, o, false)) return rc;
        if (int rc = orb_describe_launch(ctx, g, pat, pyr, m, ws.blur, K, o.xy, o.oct, o.counts, rows_out_dev + ob * 32,
                                         bytes_out_dev ? bytes_out_dev + ob * 32 : nullptr, o.angle)) return rc;
    }
    return RCN_OK;
}
