// sift.hip -- FeatureClassic::detect on the GPU: cv::SIFT::create()->detectAndCompute
// (FeatureDetector.cpp:13-35) with create()'s defaults, batched over the images of one call, on the ctx stream, nothing but
// the caller's own reads of counts[] visiting the host.  The contract is the restatement in tests/sift_ref.py.
//
//   pyramid      k_sift_blur: one 32 x 32 tile of one layer per workgroup -- the source tile with its reflect-101 halo into
//                LDS (the producer folds in the 2x bilinear upsample of the input image, or the nearest-neighbour halving
//                of the previous octave, whose result it also stores as layer 0), row pass into LDS, column pass out.
//                fp32, fmaf chains in ascending tap order, the same sequence for every pixel.
//   extrema      k_sift_extrema: one lane per pixel and DoG layer (the DoG is recomputed: one rounded subtraction), fp32
//                comparisons only, one atomic per workgroup.
//   keypoints    k_sift_keypoints: one wavefront per candidate -- adjustLocalExtrema in fp64 (every lane the same chain),
//                the orientation histogram by integer fixed-point LDS atomics (order independent), smoothing and peaks on
//                36 lanes.
//   select       k_sift_select: one workgroup per image -- rank by counting under a total order (ties broken by the
//                discrete identity), duplicates dropped, top K by response when more than K, canonical order out.
//   descriptor   k_sift_describe: one wavefront per keypoint over its sample window, the 4 x 4 x 8 (+ border) histogram by
//                the same fixed-point atomics, normalisation in a fixed order.
#include "rcn_internal.h"
#include "wgprim.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

#pragma clang fp contract(off)

constexpr int ST = 32;                        // tile side of k_sift_blur
constexpr int SIFT_BORDER = 5, SIFT_STEPS = 5, SIFT_BINS = 36;
constexpr size_t SIFT_BLUR_LDS = 96 * 1024;   // enough for RCN_SIFT_MAX_TAPS
constexpr double SIFT_FIX = 1099511627776.0;  // 2^40: histogram votes are rounded to multiples of 2^-40
constexpr int SIFT_GRID = 256;                // workgroups per image of the wavefront-per-item kernels

struct SiftOct { long long off[RCN_SIFT_MAX_LAYERS]; int h, w; };

struct SiftBlurArgs {
    const void *img; long long si, sy, sx; int dtype, H, W;     // mode 1: the input images
    float *pyr; long long fpi;                                  // packed pyramids, floats per image
    long long src_off, dst_off, dst0_off;
    int sh, sw, h, w;                                           // source layer (mode 2: of the previous octave), this layer
    int mode, taps;                                             // 0 plain, 1 upsample from the image, 2 halve the source layer
    double ry, rx;                                              // mode 2: sh / h, sw / w
    float wt[RCN_SIFT_MAX_TAPS];
};

__device__ __forceinline__ int sift_reflect(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

__device__ __forceinline__ float sift_pixel(const SiftBlurArgs &a, int img, int y, int x)
{
    const long long o = (long long)img * a.si + (long long)y * a.sy + (long long)x * a.sx;
    return a.dtype == RCN_SIFT_INPUT_U8 ? (float)reinterpret_cast<const uint8_t *>(a.img)[o] : reinterpret_cast<const float *>(a.img)[o];
}

// INTER_LINEAR at scale 2: source coordinate (d + 0.5) / 2 - 0.5, clamped at both ends with weight 0
__device__ __forceinline__ void sift_up(int d, int n, int &i0, int &i1, float &f)
{
    i0 = (d & 1) ? (d - 1) / 2 : d / 2 - 1;
    f = (d & 1) ? 0.25f : 0.75f;
    if (i0 < 0) { i0 = 0; f = 0.f; }
    if (i0 >= n - 1) { i0 = n - 1; f = 0.f; }
    i1 = min(i0 + 1, n - 1);
}

__device__ __forceinline__ float sift_fetch(const SiftBlurArgs &a, const float *P, int img, int y, int x)
{
    if (a.mode == 0) return P[a.src_off + (long long)y * a.w + x];
    if (a.mode == 2) {
        const int sy = min((int)floor((double)y * a.ry), a.sh - 1), sx = min((int)floor((double)x * a.rx), a.sw - 1);
        return P[a.src_off + (long long)sy * a.sw + sx];
    }
    int y0, y1, x0, x1;
    float fy, fx;
    sift_up(y, a.H, y0, y1, fy);
    sift_up(x, a.W, x0, x1, fx);
    const float h0 = sift_pixel(a, img, y0, x0) * (1.f - fx) + sift_pixel(a, img, y0, x1) * fx;     // horizontal pass first
    const float h1 = sift_pixel(a, img, y1, x0) * (1.f - fx) + sift_pixel(a, img, y1, x1) * fx;
    return h0 * (1.f - fy) + h1 * fy;
}

__global__ __launch_bounds__(256) void k_sift_blur(SiftBlurArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sift_smem[];
    const int R = a.taps >> 1, SW = ST + 2 * R, pitch = SW + 1;
    float *s_src = sift_smem, *s_row = sift_smem + SW * pitch;
    const int tid = threadIdx.x, img = blockIdx.z;
    const int x0 = blockIdx.x * ST, y0 = blockIdx.y * ST;
    float *P = a.pyr + (long long)img * a.fpi;
    for (int i = tid; i < SW * SW; i += 256) {
        const int ly = i / SW, lx = i - ly * SW;
        const int uy = y0 + ly - R, ux = x0 + lx - R;
        const float v = sift_fetch(a, P, img, sift_reflect(uy, a.h), sift_reflect(ux, a.w));
        s_src[ly * pitch + lx] = v;
        if (a.mode == 2 && ly >= R && ly < R + ST && lx >= R && lx < R + ST && uy < a.h && ux < a.w)
            P[a.dst0_off + (long long)uy * a.w + ux] = v;
    }
    __syncthreads();
    for (int i = tid; i < SW * ST; i += 256) {
        const int ly = i / ST, lx = i - ly * ST;
        const float *s = s_src + ly * pitch + lx;
        float acc = a.wt[0] * s[0];
        for (int t = 1; t < a.taps; ++t) acc = fmaf(a.wt[t], s[t], acc);
        s_row[ly * ST + lx] = acc;
    }
    __syncthreads();
    for (int i = tid; i < ST * ST; i += 256) {
        const int ly = i / ST, lx = i - ly * ST;
        const float *s = s_row + ly * ST + lx;
        float acc = a.wt[0] * s[0];
        for (int t = 1; t < a.taps; ++t) acc = fmaf(a.wt[t], s[t * ST], acc);
        const int y = y0 + ly, x = x0 + lx;
        if (y < a.h && x < a.w) P[a.dst_off + (long long)y * a.w + x] = acc;
    }
}

// ---- behind the pyramid -------------------------------------------------------------------------------------------------

// one keypoint before the selection: the emitted fields and the discrete identity (final r, c; octave, layer, peak bin)
struct SiftKp { float x, y, size, angle, resp; int32_t oct; uint32_t r, c, olb, pad; };

struct SiftDetArgs {
    const float *pyr; long long fpi;
    int n_oct, S;
    float thr;                                  // floor(0.5 contrast / S * 255)
    double contrast, edge, sigma;
    unsigned long long *cand; unsigned *ccnt;   // [nb][cap], [nb]
    SiftKp *kps; unsigned *kcnt;               // [nb][cap], [nb]
    unsigned cap;
    SiftOct oc[RCN_SIFT_MAX_OCTAVES];
};

__device__ __forceinline__ float sift_dog(const float *P, const SiftOct &oc, int l, int y, int x)
{
    const long long p = (long long)y * oc.w + x;
    return P[oc.off[l + 1] + p] - P[oc.off[l] + p];
}

// one launch per octave: grid (pixels / 256, S, images)
__global__ __launch_bounds__(256) void k_sift_extrema(SiftDetArgs a, int o)
{
    __shared__ unsigned s_wave[4], s_base;
    const SiftOct &oc = a.oc[o];
    const int img = blockIdx.z, l = blockIdx.y + 1;
    const float *P = a.pyr + (long long)img * a.fpi;
    const int iw = oc.w - 2 * SIFT_BORDER, ih = oc.h - 2 * SIFT_BORDER;
    const int q = blockIdx.x * 256 + threadIdx.x;
    bool is = false;
    int y = 0, x = 0;
    if (q < iw * ih) {
        y = q / iw + SIFT_BORDER;
        x = q - (y - SIFT_BORDER) * iw + SIFT_BORDER;
        const float v = sift_dog(P, oc, l, y, x);
        if (fabsf(v) > a.thr) {
            bool mx = v > 0.f, mn = v < 0.f;
            for (int dl = -1; dl <= 1 && (mx || mn); ++dl)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const float u = sift_dog(P, oc, l + dl, y + dy, x + dx);
                        mx = mx && v >= u;
                        mn = mn && v <= u;
                    }
            is = mx || mn;
        }
    }
    const unsigned long long bal = __ballot(is);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_wave[w] = (unsigned)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        s_base = total ? atomicAdd(a.ccnt + img, total) : 0u;
    }
    __syncthreads();
    if (is) {
        unsigned pos = s_base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        for (int i = 0; i < w; ++i) pos += s_wave[i];
        if (pos < a.cap)
            a.cand[(size_t)img * a.cap + pos] = ((unsigned long long)o << 56) | ((unsigned long long)l << 52) | ((unsigned long long)y << 26) | (unsigned long long)x;
    }
}

// x = -H^-1 g by elimination with partial pivoting; a singular H gives 0 (cv::Mat::solve then leaves the zero vector)
__device__ __forceinline__ void sift_solve3(double A[3][4], double X[3])
{
    for (int k = 0; k < 3; ++k) {
        int p = k;
        for (int i = k + 1; i < 3; ++i)
            if (fabs(A[i][k]) > fabs(A[p][k])) p = i;
        if (A[p][k] == 0.0) { X[0] = X[1] = X[2] = 0.0; return; }
        if (p != k)
            for (int j = 0; j < 4; ++j) { const double t = A[k][j]; A[k][j] = A[p][j]; A[p][j] = t; }
        for (int i = k + 1; i < 3; ++i) {
            const double f = A[i][k] / A[k][k];
            for (int j = k; j < 4; ++j) A[i][j] -= f * A[k][j];
        }
    }
    for (int k = 2; k >= 0; --k) {
        double s = A[k][3];
        for (int j = k + 1; j < 3; ++j) s -= A[k][j] * X[j];
        X[k] = s / A[k][k];
    }
}

// grid (SIFT_GRID, images), one wavefront per workgroup and candidate
__global__ __launch_bounds__(64) void k_sift_keypoints(SiftDetArgs a)
{
    __shared__ unsigned long long s_fix[SIFT_BINS];
    __shared__ double s_raw[SIFT_BINS], s_hist[SIFT_BINS];
    __shared__ unsigned s_pos;
    const int img = blockIdx.y, lane = threadIdx.x;
    const float *P = a.pyr + (long long)img * a.fpi;
    const unsigned nc = a.ccnt[img];
    if (nc > a.cap) return;                         // overflow: k_sift_select reports it
    const double img_scale = 1.0 / 255.0, d1 = img_scale * 0.5, d2 = img_scale, dc = img_scale * 0.25;
    for (unsigned ci = blockIdx.x; ci < nc; ci += gridDim.x) {
        const unsigned long long rec = a.cand[(size_t)img * a.cap + ci];
        const int o = (int)(rec >> 56), S = a.S;
        int layer = (int)((rec >> 52) & 15u), r = (int)((rec >> 26) & 0x3FFFFFFu), c = (int)(rec & 0x3FFFFFFu);
        const SiftOct &oc = a.oc[o];
        double xi = 0, xr = 0, xc = 0, g[3] = {0, 0, 0}, dxx = 0, dyy = 0, dxy = 0, v0 = 0;
        int it = 0;
        bool ok = true;
        for (; it < SIFT_STEPS; ++it) {
#define DG(dl, dy, dx) ((double)sift_dog(P, oc, layer + (dl), r + (dy), c + (dx)))
            v0 = DG(0, 0, 0);
            g[0] = (DG(0, 0, 1) - DG(0, 0, -1)) * d1;
            g[1] = (DG(0, 1, 0) - DG(0, -1, 0)) * d1;
            g[2] = (DG(1, 0, 0) - DG(-1, 0, 0)) * d1;
            const double v2 = v0 * 2.0;
            dxx = (DG(0, 0, 1) + DG(0, 0, -1) - v2) * d2;
            dyy = (DG(0, 1, 0) + DG(0, -1, 0) - v2) * d2;
            const double dss = (DG(1, 0, 0) + DG(-1, 0, 0) - v2) * d2;
            dxy = (DG(0, 1, 1) - DG(0, 1, -1) - DG(0, -1, 1) + DG(0, -1, -1)) * dc;
            const double dxs = (DG(1, 0, 1) - DG(1, 0, -1) - DG(-1, 0, 1) + DG(-1, 0, -1)) * dc;
            const double dys = (DG(1, 1, 0) - DG(1, -1, 0) - DG(-1, 1, 0) + DG(-1, -1, 0)) * dc;
#undef DG
            double A[3][4] = {{dxx, dxy, dxs, g[0]}, {dxy, dyy, dys, g[1]}, {dxs, dys, dss, g[2]}}, X[3];
            sift_solve3(A, X);
            xc = -X[0]; xr = -X[1]; xi = -X[2];
            if (fabs(xi) < 0.5 && fabs(xr) < 0.5 && fabs(xc) < 0.5) break;
            const double big = 2147483647.0 / 3.0;
            if (!(fabs(xi) <= big && fabs(xr) <= big && fabs(xc) <= big)) { ok = false; break; }
            c += (int)rint(xc); r += (int)rint(xr); layer += (int)rint(xi);
            if (layer < 1 || layer > S || c < SIFT_BORDER || c >= oc.w - SIFT_BORDER || r < SIFT_BORDER || r >= oc.h - SIFT_BORDER) { ok = false; break; }
        }
        if (!ok || it >= SIFT_STEPS) continue;
        const double t = g[0] * xc + g[1] * xr + g[2] * xi;
        const double contr = v0 * img_scale + t * 0.5;
        if (fabs(contr) * S < a.contrast) continue;
        const double tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
        if (det <= 0.0 || tr * tr * a.edge >= (a.edge + 1.0) * (a.edge + 1.0) * det) continue;
        const double po = (double)(1 << o);
        const double size = a.sigma * exp2((layer + xi) / S) * po * 2.0;
        const double scl = size * 0.5 / po;
        const int rad = (int)rint(4.5 * scl), side = 2 * rad + 1;
        const double es = -1.0 / (2.0 * (1.5 * scl) * (1.5 * scl));
        const float *G = P + oc.off[layer];
        if (lane < SIFT_BINS) s_fix[lane] = 0ull;
        __syncthreads();
        for (int q = lane; q < side * side; q += 64) {
            const int i = q / side - rad, j = q - (i + rad) * side - rad;
            const int y = r + i, x = c + j;
            if (y <= 0 || y >= oc.h - 1 || x <= 0 || x >= oc.w - 1) continue;
            const long long p = (long long)y * oc.w + x;
            const double dx = (double)G[p + 1] - (double)G[p - 1], dy = (double)G[p - oc.w] - (double)G[p + oc.w];
            const double wgt = exp((double)(i * i + j * j) * es), mag = sqrt(dx * dx + dy * dy);
            double ori = atan2(dy, dx) * (180.0 / 3.14159265358979323846);
            if (ori < 0.0) ori += 360.0;
            int bin = (int)rint(ori * ((double)SIFT_BINS / 360.0));
            if (bin >= SIFT_BINS) bin -= SIFT_BINS;
            if (bin < 0) bin += SIFT_BINS;
            atomicAdd(&s_fix[bin], (unsigned long long)__double2ull_rn(wgt * mag * SIFT_FIX));
        }
        __syncthreads();
        if (lane < SIFT_BINS) s_raw[lane] = (double)s_fix[lane] * (1.0 / SIFT_FIX);
        if (lane == 0) s_pos = 0u;
        __syncthreads();
        if (lane < SIFT_BINS) {
            const int k = lane, n = SIFT_BINS;
            s_hist[k] = (s_raw[(k + n - 2) % n] + s_raw[(k + 2) % n]) * (1.0 / 16.0) + (s_raw[(k + n - 1) % n] + s_raw[(k + 1) % n]) * (4.0 / 16.0) +
                        s_raw[k] * (6.0 / 16.0);
        }
        __syncthreads();
        double omax = s_hist[0];
        for (int k = 1; k < SIFT_BINS; ++k) omax = fmax(omax, s_hist[k]);
        bool peak = false;
        double hl = 0, hj = 0, hr = 0;
        if (lane < SIFT_BINS) {
            hl = s_hist[lane > 0 ? lane - 1 : SIFT_BINS - 1];
            hj = s_hist[lane];
            hr = s_hist[lane < SIFT_BINS - 1 ? lane + 1 : 0];
            peak = hj > hl && hj > hr && hj >= omax * 0.8;
        }
        const unsigned long long bal = __ballot(peak);
        if (lane == 0 && bal) s_pos = atomicAdd(a.kcnt + img, (unsigned)__popcll(bal));
        __syncthreads();
        if (peak) {
            const unsigned pos = s_pos + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
            if (pos < a.cap) {
                double bin = lane + 0.5 * (hl - hr) / (hl - 2.0 * hj + hr);
                bin = bin < 0.0 ? SIFT_BINS + bin : bin >= SIFT_BINS ? bin - SIFT_BINS : bin;
                float ang = (float)(360.0 - (360.0 / SIFT_BINS) * bin);
                if (fabsf(ang - 360.f) < FLT_EPSILON) ang = 0.f;
                SiftKp k;
                k.x = (float)((c + xc) * po * 0.5);            // first octave -1: coordinates and size halved
                k.y = (float)((r + xr) * po * 0.5);
                k.size = (float)(size * 0.5);
                k.angle = ang;
                k.resp = (float)fabs(contr);
                const int packed = o + (layer << 8) + ((int)rint((xi + 0.5) * 255.0) << 16);
                k.oct = (packed & ~255) | ((packed - 1) & 255);
                k.r = (uint32_t)r; k.c = (uint32_t)c; k.olb = ((uint32_t)o << 16) | ((uint32_t)layer << 8) | (uint32_t)lane; k.pad = 0;
                a.kps[(size_t)img * a.cap + pos] = k;
            }
        }
        __syncthreads();
    }
}

struct SiftSelArgs {
    const SiftKp *kps; const unsigned *ccnt, *kcnt; unsigned cap;
    unsigned *ord, *uniq, *keep;          // [nb][cap] each
    int K;
    float *xy; int32_t *xy_int; float *size, *angle, *resp; int32_t *oct, *counts;
};

__device__ __forceinline__ bool sift_same(const SiftKp &a, const SiftKp &b) { return a.r == b.r && a.c == b.c && a.olb == b.olb; }
// the canonical order: (x, y, size, angle, response, packed octave) ascending, ties by the discrete identity
__device__ __forceinline__ int sift_cmp(const SiftKp &a, const SiftKp &b)
{
#define SIFT_C(f) if (a.f != b.f) return a.f < b.f ? -1 : 1;
    SIFT_C(x) SIFT_C(y) SIFT_C(size) SIFT_C(angle) SIFT_C(resp) SIFT_C(oct) SIFT_C(r) SIFT_C(c) SIFT_C(olb)
#undef SIFT_C
    return 0;
}

__global__ __launch_bounds__(1024) void k_sift_select(SiftSelArgs a)
{
    __shared__ int s_scan[16];
    const int img = blockIdx.x, tid = threadIdx.x, K = a.K;
    const SiftKp *kp = a.kps + (size_t)img * a.cap;
    unsigned *ord = a.ord + (size_t)img * a.cap, *uniq = a.uniq + (size_t)img * a.cap, *keep = a.keep + (size_t)img * a.cap;
    float *xy = a.xy + (size_t)img * K * 2;
    int32_t *xi = a.xy_int + (size_t)img * K * 2;
    const size_t ob = (size_t)img * K;
    const bool over = a.ccnt[img] > a.cap || a.kcnt[img] > a.cap;
    const int N = over ? 0 : (int)a.kcnt[img];
    for (int i = tid; i < N; i += 1024) {
        const SiftKp me = kp[i];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            const int cm = sift_cmp(kp[j], me);
            rank += (cm < 0 || (cm == 0 && j < i)) ? 1 : 0;
        }
        ord[rank] = (unsigned)i;
    }
    __syncthreads();
    // (the ranks are a permutation: the order is total unless a field is a NaN, which no finite pyramid gives; the clamp keeps
    // an index read from a slot no rank reached inside the list all the same)
    const int per = (N + 1023) / 1024;
    int p0 = min(N, tid * per), p1 = min(N, p0 + per), mine = 0;
    for (int p = p0; p < p1; ++p) {
        const unsigned cur = min(ord[p], (unsigned)(N - 1)), prev = p ? min(ord[p - 1], (unsigned)(N - 1)) : 0u;
        mine += (p == 0 || !sift_same(kp[cur], kp[prev])) ? 1 : 0;
    }
    int M;
    int pos = wg_scan_incl<int, 1024>(mine, s_scan, M) - mine;
    for (int p = p0; p < p1; ++p) {
        const unsigned cur = min(ord[p], (unsigned)(N - 1)), prev = p ? min(ord[p - 1], (unsigned)(N - 1)) : 0u;
        if (p == 0 || !sift_same(kp[cur], kp[prev])) uniq[pos++] = cur;
    }
    if (tid == 0) a.counts[img] = over ? -1 : M;
    __syncthreads();
    for (int u = tid; u < M; u += 1024) {
        unsigned k = 1u;
        if (M > K) {
            const float ru = kp[uniq[u]].resp;
            int rk = 0;
            for (int v = 0; v < M; ++v) {
                const float rv = kp[uniq[v]].resp;
                rk += (rv > ru || (rv == ru && v < u)) ? 1 : 0;
            }
            k = rk < K ? 1u : 0u;
        }
        keep[u] = k;
    }
    __syncthreads();
    const int per2 = (M + 1023) / 1024;
    p0 = min(M, tid * per2); p1 = min(M, p0 + per2); mine = 0;
    for (int p = p0; p < p1; ++p) mine += (int)keep[p];
    int E;
    pos = wg_scan_incl<int, 1024>(mine, s_scan, E) - mine;
    for (int p = p0; p < p1; ++p)
        if (keep[p]) {
            const SiftKp k = kp[uniq[p]];
            xy[2 * pos] = k.x; xy[2 * pos + 1] = k.y;
            xi[2 * pos] = (int32_t)k.x; xi[2 * pos + 1] = (int32_t)k.y;
            a.size[ob + pos] = k.size; a.angle[ob + pos] = k.angle; a.resp[ob + pos] = k.resp; a.oct[ob + pos] = k.oct;
            ++pos;
        }
    for (int i = E + tid; i < K; i += 1024) {
        xy[2 * i] = -1.f; xy[2 * i + 1] = -1.f;
        xi[2 * i] = -1; xi[2 * i + 1] = -1;
        a.size[ob + i] = 0.f; a.angle[ob + i] = 0.f; a.resp[ob + i] = 0.f; a.oct[ob + i] = 0;
    }
}

struct SiftDescArgs {
    const float *pyr; long long fpi;
    int n_oct, n_layers, K;
    const float *xy, *size, *angle; const int32_t *oct, *counts;
    float *rows;
    SiftOct oc[RCN_SIFT_MAX_OCTAVES];
};

// grid (SIFT_GRID, images), one wavefront per workgroup and keypoint row
__global__ __launch_bounds__(64) void k_sift_describe(SiftDescArgs a)
{
    constexpr int D = 4, NB = 8, HL = (D + 2) * (D + 2) * (NB + 2);
    __shared__ unsigned long long s_fix[HL];
    __shared__ double s_dst[D * D * NB];
    const int img = blockIdx.y, lane = threadIdx.x, K = a.K;
    const float *P = a.pyr + (long long)img * a.fpi;
    const int cnt = min(max(a.counts[img], 0), K);
    for (int kk = blockIdx.x; kk < K; kk += gridDim.x) {
        float *row = a.rows + ((size_t)img * K + kk) * 128;
        const int packed = kk < cnt ? a.oct[(size_t)img * K + kk] : 0;
        int o8 = packed & 255;
        const int layer = (packed >> 8) & 255;
        o8 = o8 < 128 ? o8 : o8 - 256;
        const int o = o8 + 1;
        if (kk >= cnt || o < 0 || o >= a.n_oct || layer < 0 || layer >= a.n_layers) {      // padding (or a keypoint that names no layer)
            row[lane] = 0.f; row[lane + 64] = 0.f;
            continue;
        }
        const SiftOct &oc = a.oc[o];
        const float *G = P + oc.off[layer];
        const double scale = o8 >= 0 ? 1.0 / (double)(1 << o8) : (double)(1 << -o8);
        const double scl = (double)a.size[(size_t)img * K + kk] * scale * 0.5;
        const double px = (double)a.xy[((size_t)img * K + kk) * 2] * scale, py = (double)a.xy[((size_t)img * K + kk) * 2 + 1] * scale;
        double ang = 360.0 - (double)a.angle[(size_t)img * K + kk];
        if (fabs(ang - 360.0) < (double)FLT_EPSILON) ang = 0.0;
        const int ptx = (int)rint(px), pty = (int)rint(py);
        const double hw = 3.0 * scl;
        int rad = (int)rint(hw * 1.4142135623730951 * (D + 1) * 0.5);
        rad = min(rad, (int)sqrt((double)oc.w * oc.w + (double)oc.h * oc.h));
        const double ct = cos(ang * (3.14159265358979323846 / 180.0)) / hw, st = sin(ang * (3.14159265358979323846 / 180.0)) / hw;
        const double es = -1.0 / (D * D * 0.5), bpr = NB / 360.0;
        for (int i = lane; i < HL; i += 64) s_fix[i] = 0ull;
        __syncthreads();
        const long long side = 2ll * rad + 1;
        for (long long q = lane; q < side * side; q += 64) {
            const int i = (int)(q / side) - rad, j = (int)(q - (long long)(i + rad) * side) - rad;
            const double c_rot = j * ct - i * st, r_rot = j * st + i * ct;
            double rbin = r_rot + D / 2 - 0.5, cbin = c_rot + D / 2 - 0.5;
            const int r = pty + i, c = ptx + j;
            if (!(rbin > -1.0 && rbin < D && cbin > -1.0 && cbin < D && r > 0 && r < oc.h - 1 && c > 0 && c < oc.w - 1)) continue;
            const long long p = (long long)r * oc.w + c;
            const double dx = (double)G[p + 1] - (double)G[p - 1], dy = (double)G[p - oc.w] - (double)G[p + oc.w];
            double ori = atan2(dy, dx) * (180.0 / 3.14159265358979323846);
            if (ori < 0.0) ori += 360.0;
            const double mag = sqrt(dx * dx + dy * dy) * exp((c_rot * c_rot + r_rot * r_rot) * es);
            double obin = (ori - ang) * bpr;
            const int r0 = (int)floor(rbin), c0 = (int)floor(cbin);
            int o0 = (int)floor(obin);
            rbin -= r0; cbin -= c0; obin -= o0;
            o0 %= NB;                                              // one wrap for a keypoint of the detector's; any angle handed in stays inside
            if (o0 < 0) o0 += NB;
            const double v_r1 = mag * rbin, v_r0 = mag - v_r1;
            const double v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11, v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
            const double v111 = v_rc11 * obin, v110 = v_rc11 - v111, v101 = v_rc10 * obin, v100 = v_rc10 - v101;
            const double v011 = v_rc01 * obin, v010 = v_rc01 - v011, v001 = v_rc00 * obin, v000 = v_rc00 - v001;
            const int idx = ((r0 + 1) * (D + 2) + c0 + 1) * (NB + 2) + o0;
#define SIFT_V(off, v) atomicAdd(&s_fix[idx + (off)], (unsigned long long)__double2ull_rn(fmax(v, 0.0) * SIFT_FIX))
            SIFT_V(0, v000); SIFT_V(1, v001); SIFT_V(NB + 2, v010); SIFT_V(NB + 3, v011);
            SIFT_V((D + 2) * (NB + 2), v100); SIFT_V((D + 2) * (NB + 2) + 1, v101);
            SIFT_V((D + 3) * (NB + 2), v110); SIFT_V((D + 3) * (NB + 2) + 1, v111);
#undef SIFT_V
        }
        __syncthreads();
        for (int e = lane; e < D * D * NB; e += 64) {
            const int i = e / (D * NB), j = (e / NB) % D, k = e % NB;
            const int idx = ((i + 1) * (D + 2) + (j + 1)) * (NB + 2);
            unsigned long long h = s_fix[idx + k];
            if (k < 2) h += s_fix[idx + NB + k];                  // the circular orientation axis
            s_dst[e] = (double)h * (1.0 / SIFT_FIX);
        }
        __syncthreads();
        double nrm2 = 0.0;
        for (int e = 0; e < D * D * NB; ++e) nrm2 += s_dst[e] * s_dst[e];
        const double thr = sqrt(nrm2) * 0.2;
        nrm2 = 0.0;
        for (int e = 0; e < D * D * NB; ++e) { const double v = fmin(s_dst[e], thr); nrm2 += v * v; }
        const double f = 512.0 / fmax(sqrt(nrm2), (double)FLT_EPSILON);
        for (int e = lane; e < D * D * NB; e += 64) row[e] = (float)fmin(fmax(rint(fmin(s_dst[e], thr) * f), 0.0), 255.0);
        __syncthreads();
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

size_t sift_align(size_t b) { return (b + 255) & ~(size_t)255; }

int sift_taps(double sigma) { return (int)std::nearbyint(8.0 * sigma + 1.0) | 1; }

void sift_weights(double sigma, int taps, float *out)
{
    std::vector<double> w((size_t)taps);
    double sum = 0.0;
    for (int i = 0; i < taps; ++i) {
        const double x = (double)(i - taps / 2);
        w[(size_t)i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
        sum += w[(size_t)i];
    }
    for (int i = 0; i < taps; ++i) out[i] = (float)(w[(size_t)i] / sum);
}

const char *sift_layout_fill(int32_t H, int32_t W, const rcn_sift_options *opt, rcn_sift_pyramid_layout *L)
{
    rcn_sift_options d;
    rcn_sift_default_options(&d);
    if (!opt) opt = &d;
    if (H < 16 || W < 16) return "min(H, W) < 16";
    if (4ll * H * W > 0x7FFFFFFFll) return "4 H W exceeds 2^31 - 1";
    const int S = opt->n_octave_layers;
    if (S < 1 || S > 5) return "n_octave_layers outside 1..5";
    if (!(opt->contrast_threshold >= 0.0) || !(opt->edge_threshold > 0.0) || !(opt->sigma > 0.0)) return "option out of range";
    std::memset(L, 0, sizeof *L);
    const int m = std::min(2 * H, 2 * W);
    L->n_octaves = (int)std::nearbyint(std::log((double)m) / std::log(2.0) - 2.0) + 1;
    L->n_layers = S + 3;
    L->base_sigma = std::sqrt(std::max(opt->sigma * opt->sigma - 1.0, 0.01));
    L->base_taps = sift_taps(L->base_sigma);
    const double k = std::pow(2.0, 1.0 / S);
    L->layer_sigma[0] = opt->sigma;
    int max_taps = L->base_taps;
    for (int i = 1; i < S + 3; ++i) {
        const double prev = std::pow(k, (double)(i - 1)) * opt->sigma, total = prev * k;
        L->layer_sigma[i] = std::sqrt(total * total - prev * prev);
        L->layer_taps[i] = sift_taps(L->layer_sigma[i]);
        max_taps = std::max(max_taps, L->layer_taps[i]);
    }
    if (max_taps > RCN_SIFT_MAX_TAPS || L->n_octaves > RCN_SIFT_MAX_OCTAVES) return "sigma out of range (a blur needs too many taps)";
    int h = 2 * H, w = 2 * W;
    int64_t off = 0;
    for (int o = 0; o < L->n_octaves; ++o) {
        if (h < 1 || w < 1) { L->n_octaves = o; break; }
        L->oct_h[o] = h; L->oct_w[o] = w;
        for (int i = 0; i < S + 3; ++i) { L->layer_offset[o][i] = off; off += (int64_t)h * w; }
        h /= 2; w /= 2;
    }
    L->floats_per_image = off;
    return nullptr;
}

bool sift_layout_checked(rcn_ctx *ctx, const char *who, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, rcn_sift_pyramid_layout *L)
{
    const char *why = n < 0 ? "n < 0" : sift_layout_fill(H, W, opt, L);
    if (why) ctx->set_error(std::string(who) + ": bad argument (" + why + ")");
    return !why;
}

int sift_setup(rcn_ctx *ctx)
{
    static std::mutex once_mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> lk(once_mu);
    if (std::find(done.begin(), done.end(), ctx->device) == done.end()) {
        RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sift_blur), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SIFT_BLUR_LDS));
        done.push_back(ctx->device);
    }
    return RCN_OK;
}

void sift_octaves(const rcn_sift_pyramid_layout &L, SiftOct *oc)
{
    for (int o = 0; o < L.n_octaves; ++o) {
        for (int i = 0; i < RCN_SIFT_MAX_LAYERS; ++i) oc[o].off[i] = L.layer_offset[o][i];
        oc[o].h = L.oct_h[o]; oc[o].w = L.oct_w[o];
    }
}

// candidates / keypoints an image may have before its result is declared an overflow
unsigned sift_cap(const rcn_sift_pyramid_layout &L)
{
    int64_t px = 0;
    for (int o = 0; o < L.n_octaves; ++o) px += (int64_t)L.oct_h[o] * L.oct_w[o];
    return (unsigned)std::min<int64_t>(px * (L.n_layers - 3) / 8 + 4096, 1ll << 26);
}
size_t sift_list_bytes(unsigned cap) { return sift_align((size_t)cap * 8) + sift_align((size_t)cap * sizeof(SiftKp)) + 3 * sift_align((size_t)cap * 4); }

int32_t sift_chunk(rcn_ctx *ctx, int32_t n, size_t per_image)
{
    if (ctx->sift_chunk_images > 0) return std::min(n, ctx->sift_chunk_images);
    const size_t budget = (size_t)1 << 30;
    return (int32_t)std::max<size_t>(1, std::min<size_t>({(size_t)n, budget / std::max<size_t>(per_image, 1), (size_t)32768}));
}

int sift_pyramid_launch(rcn_ctx *ctx, const rcn_sift_pyramid_layout &L, const void *img, int32_t dtype, int64_t si, int64_t sy, int64_t sx,
                        int32_t first, int32_t m, int32_t H, int32_t W, float *pyr)
{
    SiftBlurArgs a;
    std::memset(&a, 0, sizeof a);
    const size_t esz = dtype == RCN_SIFT_INPUT_U8 ? 1 : 4;
    a.img = reinterpret_cast<const char *>(img) + (int64_t)first * si * (int64_t)esz;
    a.si = si; a.sy = sy; a.sx = sx; a.dtype = dtype; a.H = H; a.W = W;
    a.pyr = pyr; a.fpi = L.floats_per_image;
    const int S = L.n_layers - 3;
    auto launch = [&](int o, int mode, int64_t src, int64_t dst, int64_t dst0, double sigma, int taps) {
        a.mode = mode; a.src_off = src; a.dst_off = dst; a.dst0_off = dst0; a.taps = taps;
        a.h = L.oct_h[o]; a.w = L.oct_w[o];
        a.sh = mode == 2 ? L.oct_h[o - 1] : a.h; a.sw = mode == 2 ? L.oct_w[o - 1] : a.w;
        a.ry = (double)a.sh / a.h; a.rx = (double)a.sw / a.w;
        sift_weights(sigma, taps, a.wt);
        const int SW = ST + 2 * (taps >> 1);
        const size_t lds = ((size_t)SW * (SW + 1) + (size_t)SW * ST) * 4;
        k_sift_blur<<<dim3((unsigned)((a.w + ST - 1) / ST), (unsigned)((a.h + ST - 1) / ST), (unsigned)m), 256, lds, ctx->stream>>>(a);
    };
    for (int o = 0; o < L.n_octaves; ++o) {
        if (o == 0) launch(0, 1, 0, L.layer_offset[0][0], 0, L.base_sigma, L.base_taps);
        else launch(o, 2, L.layer_offset[o - 1][S], L.layer_offset[o][1], L.layer_offset[o][0], L.layer_sigma[1], L.layer_taps[1]);
        for (int i = o == 0 ? 1 : 2; i < S + 3; ++i) launch(o, 0, L.layer_offset[o][i - 1], L.layer_offset[o][i], 0, L.layer_sigma[i], L.layer_taps[i]);
    }
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

// lists of one chunk inside ws (sift_list_bytes(cap) * nb + two counter arrays); image i's part of an array starts at i * cap elements
struct SiftLists { unsigned long long *cand; SiftKp *kps; unsigned *ord, *uniq, *keep, *ccnt, *kcnt; };
size_t sift_lists_total(unsigned cap, int32_t nb) { return sift_list_bytes(cap) * (size_t)nb + 2 * sift_align((size_t)nb * 4); }
SiftLists sift_lists_at(char *ws, unsigned cap, int32_t nb)
{
    SiftLists l;
    l.cand = reinterpret_cast<unsigned long long *>(ws); ws += sift_align((size_t)cap * 8) * nb;
    l.kps = reinterpret_cast<SiftKp *>(ws);              ws += sift_align((size_t)cap * sizeof(SiftKp)) * nb;
    l.ord = reinterpret_cast<unsigned *>(ws);            ws += sift_align((size_t)cap * 4) * nb;
    l.uniq = reinterpret_cast<unsigned *>(ws);           ws += sift_align((size_t)cap * 4) * nb;
    l.keep = reinterpret_cast<unsigned *>(ws);           ws += sift_align((size_t)cap * 4) * nb;
    l.ccnt = reinterpret_cast<unsigned *>(ws);           ws += sift_align((size_t)nb * 4);
    l.kcnt = reinterpret_cast<unsigned *>(ws);
    return l;
}

int sift_detect_launch(rcn_ctx *ctx, const rcn_sift_pyramid_layout &L, const rcn_sift_options &opt, const float *pyr, int32_t m, int32_t K,
                       const SiftLists &l, unsigned cap, float *xy, int32_t *xy_int, float *size, float *angle, float *resp, int32_t *oct, int32_t *counts)
{
    SiftDetArgs a;
    std::memset(&a, 0, sizeof a);
    a.pyr = pyr; a.fpi = L.floats_per_image; a.n_oct = L.n_octaves; a.S = L.n_layers - 3;
    a.thr = (float)std::floor(0.5 * opt.contrast_threshold / a.S * 255.0);
    a.contrast = opt.contrast_threshold; a.edge = opt.edge_threshold; a.sigma = opt.sigma;
    a.cand = l.cand; a.ccnt = l.ccnt; a.kps = l.kps; a.kcnt = l.kcnt; a.cap = cap;
    sift_octaves(L, a.oc);
    RCN_HIP(hipMemsetAsync(l.ccnt, 0, (size_t)m * 4, ctx->stream));
    RCN_HIP(hipMemsetAsync(l.kcnt, 0, (size_t)m * 4, ctx->stream));
    for (int o = 0; o < L.n_octaves; ++o) {
        const int64_t iw = L.oct_w[o] - 2 * SIFT_BORDER, ih = L.oct_h[o] - 2 * SIFT_BORDER;
        if (iw < 1 || ih < 1) continue;
        k_sift_extrema<<<dim3((unsigned)((iw * ih + 255) / 256), (unsigned)a.S, (unsigned)m), 256, 0, ctx->stream>>>(a, o);
    }
    k_sift_keypoints<<<dim3(SIFT_GRID, (unsigned)m), 64, 0, ctx->stream>>>(a);
    SiftSelArgs s{l.kps, l.ccnt, l.kcnt, cap, l.ord, l.uniq, l.keep, K, xy, xy_int, size, angle, resp, oct, counts};
    k_sift_select<<<(unsigned)m, 1024, 0, ctx->stream>>>(s);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int sift_describe_launch(rcn_ctx *ctx, const rcn_sift_pyramid_layout &L, const float *pyr, int32_t m, int32_t K, const float *xy, const float *size,
                         const float *angle, const int32_t *oct, const int32_t *counts, float *rows)
{
    SiftDescArgs a;
    std::memset(&a, 0, sizeof a);
    a.pyr = pyr; a.fpi = L.floats_per_image; a.n_oct = L.n_octaves; a.n_layers = L.n_layers; a.K = K;
    a.xy = xy; a.size = size; a.angle = angle; a.oct = oct; a.counts = counts; a.rows = rows;
    sift_octaves(L, a.oc);
    k_sift_describe<<<dim3((unsigned)std::min(K, SIFT_GRID), (unsigned)m), 64, 0, ctx->stream>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

bool sift_common(rcn_ctx *ctx, const char *who, int32_t K, bool nulls, const rcn_sift_options *opt, rcn_sift_options *use)
{
    rcn_sift_default_options(use);
    if (opt) *use = *opt;
    const char *why = K < 1 ? "K < 1" : nulls ? "null pointer" : nullptr;      // callers pass nulls only for n > 0: an empty batch needs no buffer
    if (why) ctx->set_error(std::string(who) + ": bad argument (" + why + ")");
    return !why;
}

}  // namespace

extern "C" void rcn_sift_default_options(rcn_sift_options *opt)
{
    if (!opt) return;
    opt->n_octave_layers = 3;
    opt->reserved = 0;
    opt->contrast_threshold = 0.04;
    opt->edge_threshold = 10.0;
    opt->sigma = 1.6;
}

extern "C" int rcn_sift_layout(int32_t H, int32_t W, const rcn_sift_options *opt, rcn_sift_pyramid_layout *out)
{
    if (!out) return RCN_ERR_ARG;
    rcn_sift_pyramid_layout L;
    if (sift_layout_fill(H, W, opt, &L)) return RCN_ERR_ARG;
    *out = L;
    return RCN_OK;
}

extern "C" int rcn_sift_set_chunk_images(rcn_ctx *ctx, int32_t images)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->sift_chunk_images = images > 0 ? images : 0;
    return RCN_OK;
}

extern "C" int rcn_sift_pyramid_device(rcn_ctx *ctx, const void *images_dev, int32_t input_dtype, int64_t stride_img, int64_t stride_y,
                                       int64_t stride_x, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, float *pyr_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sift_pyramid_device";
    rcn_sift_pyramid_layout L;
    if (!sift_layout_checked(ctx, who, n, H, W, opt, &L)) return RCN_ERR_ARG;
    if (input_dtype != RCN_SIFT_INPUT_F32 && input_dtype != RCN_SIFT_INPUT_U8) {
        ctx->set_error(std::string(who) + ": bad argument (unknown input dtype)");
        return RCN_ERR_ARG;
    }
    if (n > 0 && (!images_dev || !pyr_out_dev)) {
        ctx->set_error(std::string(who) + ": bad argument (null pointer)");
        return RCN_ERR_ARG;
    }
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = sift_setup(ctx)) return rc;
    const int32_t nb = std::min<int32_t>(n, 65535);                       // grid.z
    for (int32_t first = 0; first < n; first += nb)
        if (int rc = sift_pyramid_launch(ctx, L, images_dev, input_dtype, stride_img, stride_y, stride_x, first, std::min(nb, n - first), H, W,
                                         pyr_out_dev + (int64_t)first * L.floats_per_image)) return rc;
    return RCN_OK;
}

extern "C" int rcn_sift_candidates_device(rcn_ctx *ctx, const float *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt,
                                          int32_t capacity, uint64_t *cand_out_dev, int32_t *counts_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sift_candidates_device";
    rcn_sift_pyramid_layout L;
    rcn_sift_options use;
    if (!sift_layout_checked(ctx, who, n, H, W, opt, &L)) return RCN_ERR_ARG;
    if (!sift_common(ctx, who, capacity, n > 0 && (!pyr_dev || !cand_out_dev || !counts_dev), opt, &use)) return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    SiftDetArgs a;
    std::memset(&a, 0, sizeof a);
    a.fpi = L.floats_per_image; a.n_oct = L.n_octaves; a.S = L.n_layers - 3;
    a.thr = (float)std::floor(0.5 * use.contrast_threshold / a.S * 255.0);
    a.cap = (unsigned)capacity;
    sift_octaves(L, a.oc);
    RCN_HIP(hipMemsetAsync(counts_dev, 0, (size_t)n * 4, ctx->stream));
    for (int32_t first = 0; first < n; first += 65535) {
        const int32_t m = std::min(65535, n - first);
        a.pyr = pyr_dev + (int64_t)first * L.floats_per_image;
        a.cand = reinterpret_cast<unsigned long long *>(cand_out_dev) + (size_t)first * a.cap;
        a.ccnt = reinterpret_cast<unsigned *>(counts_dev) + first;
        for (int o = 0; o < L.n_octaves; ++o) {
            const int64_t iw = L.oct_w[o] - 2 * SIFT_BORDER, ih = L.oct_h[o] - 2 * SIFT_BORDER;
            if (iw < 1 || ih < 1) continue;
            k_sift_extrema<<<dim3((unsigned)((iw * ih + 255) / 256), (unsigned)a.S, (unsigned)m), 256, 0, ctx->stream>>>(a, o);
        }
    }
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

extern "C" int rcn_sift_detect_device(rcn_ctx *ctx, const float *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, int32_t K,
                                      float *xy_dev, int32_t *xy_int_dev, float *size_dev, float *angle_dev, float *response_dev,
                                      int32_t *octave_dev, int32_t *counts_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sift_detect_device";
    rcn_sift_pyramid_layout L;
    rcn_sift_options use;
    if (!sift_layout_checked(ctx, who, n, H, W, opt, &L)) return RCN_ERR_ARG;
    if (!sift_common(ctx, who, K, n > 0 && (!pyr_dev || !xy_dev || !xy_int_dev || !size_dev || !angle_dev || !response_dev || !octave_dev || !counts_dev), opt, &use))
        return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    const unsigned cap = sift_cap(L);
    const int32_t nb = std::min<int32_t>(sift_chunk(ctx, n, sift_list_bytes(cap)), 65535);
    RCN_HIP(ctx->sift_ws.reserve(sift_lists_total(cap, nb)));
    const SiftLists l = sift_lists_at(ctx->sift_ws.as<char>(), cap, nb);
    for (int32_t first = 0; first < n; first += nb) {
        const size_t ob = (size_t)first * K;
        if (int rc = sift_detect_launch(ctx, L, use, pyr_dev + (int64_t)first * L.floats_per_image, std::min(nb, n - first), K, l, cap, xy_dev + ob * 2,
                                        xy_int_dev + ob * 2, size_dev + ob, angle_dev + ob, response_dev + ob, octave_dev + ob, counts_dev + first)) return rc;
    }
    return RCN_OK;
}

extern "C" int rcn_sift_describe_device(rcn_ctx *ctx, const float *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, int32_t K,
                                        const float *xy_dev, const float *size_dev, const float *angle_dev, const int32_t *octave_dev,
                                        const int32_t *counts_dev, float *rows_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sift_describe_device";
    rcn_sift_pyramid_layout L;
    rcn_sift_options use;
    if (!sift_layout_checked(ctx, who, n, H, W, opt, &L)) return RCN_ERR_ARG;
    if (!sift_common(ctx, who, K, n > 0 && (!pyr_dev || !xy_dev || !size_dev || !angle_dev || !octave_dev || !counts_dev || !rows_out_dev), opt, &use)) return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    const int32_t nb = std::min<int32_t>(n, 65535);
    for (int32_t first = 0; first < n; first += nb) {
        const size_t ob = (size_t)first * K;
        if (int rc = sift_describe_launch(ctx, L, pyr_dev + (int64_t)first * L.floats_per_image, std::min(nb, n - first), K, xy_dev + ob * 2, size_dev + ob,
                                          angle_dev + ob, octave_dev + ob, counts_dev + first, rows_out_dev + ob * 128)) return rc;
    }
    return RCN_OK;
}

extern "C" int rcn_sift_detect_and_compute_device(rcn_ctx *ctx, const void *images_dev, int32_t input_dtype, int64_t stride_img, int64_t stride_y,
                                                  int64_t stride_x, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, int32_t K,
                                                  float *xy_dev, int32_t *xy_int_dev, float *size_dev, float *angle_dev, float *response_dev,
                                                  int32_t *octave_dev, int32_t *counts_dev, float *rows_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sift_detect_and_compute_device";
    rcn_sift_pyramid_layout L;
    rcn_sift_options use;
    if (!sift_layout_checked(ctx, who, n, H, W, opt, &L)) return RCN_ERR_ARG;
    if (input_dtype != RCN_SIFT_INPUT_F32 && input_dtype != RCN_SIFT_INPUT_U8) {
        ctx->set_error(std::string(who) + ": bad argument (unknown input dtype)");
        return RCN_ERR_ARG;
    }
    if (!sift_common(ctx, who, K, n > 0 && (!images_dev || !xy_dev || !xy_int_dev || !size_dev || !angle_dev || !response_dev || !octave_dev || !counts_dev || !rows_out_dev),
                     opt, &use)) return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = sift_setup(ctx)) return rc;
    const unsigned cap = sift_cap(L);
    const size_t pyr_bytes = sift_align((size_t)L.floats_per_image * 4);
    const int32_t nb = std::min<int32_t>(sift_chunk(ctx, n, pyr_bytes + sift_list_bytes(cap)), 65535);
    RCN_HIP(ctx->sift_pyr.reserve((size_t)L.floats_per_image * 4 * (size_t)nb));
    RCN_HIP(ctx->sift_ws.reserve(sift_lists_total(cap, nb)));
    float *pyr = ctx->sift_pyr.as<float>();
    const SiftLists l = sift_lists_at(ctx->sift_ws.as<char>(), cap, nb);
    for (int32_t first = 0; first < n; first += nb) {
        const int32_t m = std::min(nb, n - first);
        const size_t ob = (size_t)first * K;
        if (int rc = sift_pyramid_launch(ctx, L, images_dev, input_dtype, stride_img, stride_y, stride_x, first, m, H, W, pyr)) return rc;
        if (int rc = sift_detect_launch(ctx, L, use, pyr, m, K, l, cap, xy_dev + ob * 2, xy_int_dev + ob * 2, size_dev + ob, angle_dev + ob,
                                        response_dev + ob, octave_dev + ob, counts_dev + first)) return rc;
        if (int rc = sift_describe_launch(ctx, L, pyr, m, K, xy_dev + ob * 2, size_dev + ob, angle_dev + ob, octave_dev + ob, counts_dev + first,
                                          rows_out_dev + ob * 128)) return rc;
    }
    return RCN_OK;
}
