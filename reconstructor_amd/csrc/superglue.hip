// superglue.hip -- SuperGlue's optimal-matching layer on the GPU: what
// FeatureMatcherSuperglue::matchFeatures (FeatureMatcherSuperglue.cpp:51-101) runs behind the graph network, batched over the
// pairs of one call, on the ctx stream, nothing visiting the host.
//
//   scores    k_sg_scores: S = d0 d1^T / sqrt(D), LDS-tiled fp32 FMA, operands read in place through element strides.
//   Sinkhorn  fused path  k_sg_fused: one workgroup per pair, the matrix loaded once, every iteration out of LDS.
//             banded path k_sg_rows + k_sg_cols per iteration: a workgroup owns a band of SG_BAND rows, holds it in LDS, gives
//             each row its logsumexp (one wavefront per row) and from the same data the band's (max, sum) of Z + u for every
//             column; k_sg_cols merges those in band order.  Stream order is the only synchronisation between workgroups.
//   selection k_sg_rowarg, k_sg_colarg (argmax of logP, lowest index on ties), k_sg_select (mutual check, scores, the two
//             thresholds, table, counts, status), k_sg_logp (the dense logP for diagnostics and tests).
//
// The dustbin row and column are the constant alpha and enter each logsumexp as one extra term.  u[b][M] and v[b][N] hold
// the dustbin entries whatever m and n.  Every reduction has an order fixed by (m, n) alone and independent of the row or
// column it serves: a pair's result is a function of the pair, and exact ties stay ties.
#include "rcn_internal.h"

#include <algorithm>
#include <cmath>

namespace {

#pragma clang fp contract(off)

constexpr int SG_MAX = RCN_SG_MAX_POINTS;
constexpr size_t SG_LDS = RCN_SG_LDS_BYTES;
constexpr int SG_BAND = 8;                    // rows of a band: one per wavefront of k_sg_rows
constexpr int SG_ROWS_T = 64 * SG_BAND;       // threads of k_sg_rows
constexpr int SG_COLS_T = 256;                // threads of k_sg_cols, k_sg_colarg, k_sg_select
constexpr int SG_FUSED_T = 1024;              // threads of k_sg_fused
constexpr int SG_SUB = 16;                    // lanes that share one row or column in k_sg_fused
constexpr size_t SG_PART_BYTES = (size_t)256 << 20;   // cap of the partials workspace: bounds a chunk too
constexpr int SG_SLICE = 32768;               // pairs per launch at most (grid dimension y / z)
constexpr float SG_NINF = -INFINITY;

struct SgArgs {
    const float *S;
    long long sp, sr, sc;
    const int32_t *m_dev, *n_dev;
    int M, N, b0, path, nbmax;
    float alpha;
    float *u, *v;              // [B][M + 1], [B][N + 1]
    float2 *part;              // [pairs of a chunk][nbmax][N]
    int32_t *i0, *i1;          // [B][M], [B][N]
    float *rmax;               // [B][M]
    double mt, st;
    int32_t *matches0, *matches1;
    float *ms0, *ms1;
    int32_t *table;
    long long ts;
    int32_t *counts;
    float *logp;
    int32_t *status;
};

__device__ __forceinline__ int sg_count(const int32_t *p, int b, int cap)
{
    const int c = p ? p[b] : cap;
    return min(max(c, 0), cap);
}
__device__ __forceinline__ bool sg_fits(int m, int n) { return (size_t)(m + 1) * (size_t)(n + 1) * 4 <= SG_LDS; }
// which path runs pair (m, n): 0 none (an empty pair), 1 fused, 2 banded
__device__ __forceinline__ int sg_path(int m, int n, int path)
{
    if (m == 0 || n == 0) return 0;
    if (path == RCN_SG_PATH_BANDED) return 2;
    if (path == RCN_SG_PATH_FUSED) return 1;
    return sg_fits(m, n) ? 1 : 2;
}
struct SgMarg { float norm, mu_d, nu_d; };      // log_mu / log_nu of the inner entries, of the two dustbins
__device__ __forceinline__ SgMarg sg_marg(int m, int n)
{
    const float norm = -logf((float)(m + n));
    return {norm, logf((float)n) + norm, logf((float)m) + norm};
}

__device__ __forceinline__ float sg_wave_max(float x)
{
    for (int off = 32; off; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
    return x;
}
__device__ __forceinline__ float sg_wave_sum(float x)
{
    for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
// reductions over a workgroup of T threads (a power of two), fixed tree; every thread calls them and gets the result
template <int T, bool MAX> __device__ __forceinline__ float sg_block_reduce(float x, float *s)
{
    __syncthreads();
    s[threadIdx.x] = x;
    __syncthreads();
    for (int off = T / 2; off; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] = MAX ? fmaxf(s[threadIdx.x], s[threadIdx.x + off]) : s[threadIdx.x] + s[threadIdx.x + off];
        __syncthreads();
    }
    return s[0];
}
// log of the sum over t < len of exp(alpha + w[t]) and of exp(alpha + wd): a dustbin row or column, by one workgroup
template <int T> __device__ __forceinline__ float sg_dustbin_lse(const float *w, int len, float wd, float alpha, float *s)
{
    float mx = threadIdx.x == 0 ? alpha + wd : SG_NINF;
    for (int t = threadIdx.x; t < len; t += T) mx = fmaxf(mx, alpha + w[t]);
    mx = sg_block_reduce<T, true>(mx, s);
    float sum = threadIdx.x == 0 ? expf((alpha + wd) - mx) : 0.f;
    for (int t = threadIdx.x; t < len; t += T) sum += expf((alpha + w[t]) - mx);
    sum = sg_block_reduce<T, false>(sum, s);
    return mx + logf(sum);
}

// ---- scores -------------------------------------------------------------------------------------------------------------

constexpr int SC_T = 32, SC_K = 32;
__device__ __forceinline__ void sg_load_tile(float (*t)[SC_T + 1], const float *d, long long sr, long long sd, int r0, int rows, int k0, int D)
{
    for (int e = threadIdx.x; e < SC_T * SC_K; e += 256) {
        const int r = sd == 1 ? e >> 5 : e & 31, k = sd == 1 ? e & 31 : e >> 5;       // the unit stride varies fastest over the lanes
        t[k][r] = (r0 + r < rows && k0 + k < D) ? d[(long long)(r0 + r) * sr + (long long)(k0 + k) * sd] : 0.f;
    }
}
// 32 x 32 scores per workgroup, 2 x 2 per lane; products accumulated by fmaf in ascending d; then one division by sqrt(D)
__global__ __launch_bounds__(256) void k_sg_scores(const float *__restrict__ d0, long long sp0, long long sr0, long long sd0,
                                                   const float *__restrict__ d1, long long sp1, long long sr1, long long sd1,
                                                   const int32_t *__restrict__ m_dev, const int32_t *__restrict__ n_dev, int b0, int M, int N, int D,
                                                   float *__restrict__ out)
{
    __shared__ float sa[SC_K][SC_T + 1], sb[SC_K][SC_T + 1];
    const int b = b0 + blockIdx.z;
    const int m = sg_count(m_dev, b, M), n = sg_count(n_dev, b, N);
    const int i0 = blockIdx.y * SC_T, j0 = blockIdx.x * SC_T;
    if (i0 >= m || j0 >= n) return;
    const float *a = d0 + (long long)b * sp0, *c = d1 + (long long)b * sp1;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    for (int k0 = 0; k0 < D; k0 += SC_K) {
        sg_load_tile(sa, a, sr0, sd0, i0, m, k0, D);
        sg_load_tile(sb, c, sr1, sd1, j0, n, k0, D);
        __syncthreads();
        for (int k = 0; k < SC_K; ++k) {
            const float a0 = sa[k][2 * ty], a1 = sa[k][2 * ty + 1], c0 = sb[k][2 * tx], c1 = sb[k][2 * tx + 1];
            acc[0][0] = fmaf(a0, c0, acc[0][0]);
            acc[0][1] = fmaf(a0, c1, acc[0][1]);
            acc[1][0] = fmaf(a1, c0, acc[1][0]);
            acc[1][1] = fmaf(a1, c1, acc[1][1]);
        }
        __syncthreads();
    }
    const float root = sqrtf((float)D);
    for (int y = 0; y < 2; ++y)
        for (int x = 0; x < 2; ++x) {
            const int i = i0 + 2 * ty + y, j = j0 + 2 * tx + x;
            if (i < m && j < n) out[((size_t)b * M + i) * N + j] = __fdiv_rn(acc[y][x], root);
        }
}

// ---- Sinkhorn: fused path -----------------------------------------------------------------------------------------------

// One row (COL = false) or column (COL = true) of the bordered matrix for each group of SG_SUB lanes: its logsumexp with the
// other side's potential w (other-side length len, dustbin entry w[len]).  Line `lines` is this side's dustbin.  The matrix is
// tile[i * ld + j], ld odd.  Every lane of the workgroup runs the same trip count (the shuffles need whole groups).
template <bool COL> __device__ __forceinline__ void sg_fused_pass(const float *tile, int ld, int lines, int len, const float *w, float *out,
                                                                 float alpha, float lg_inner, float lg_dust)
{
    const int sub = threadIdx.x & (SG_SUB - 1), grp = threadIdx.x / SG_SUB;
    for (int base = 0; base <= lines; base += SG_FUSED_T / SG_SUB) {
        const int line = base + grp;
        const bool live = line <= lines, dust = line == lines;
        const float *z = tile + (COL ? line : line * ld);
        const int step = COL ? ld : 1;
        float mx = (live && sub == 0) ? alpha + w[len] : SG_NINF;
        if (live)
            for (int t = sub; t < len; t += SG_SUB) mx = fmaxf(mx, (dust ? alpha : z[t * step]) + w[t]);
        for (int off = SG_SUB / 2; off; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        float sum = (live && sub == 0) ? expf((alpha + w[len]) - mx) : 0.f;
        if (live)
            for (int t = sub; t < len; t += SG_SUB) sum += expf(((dust ? alpha : z[t * step]) + w[t]) - mx);
        for (int off = SG_SUB / 2; off; off >>= 1) sum += __shfl_xor(sum, off);
        if (live && sub == 0) out[line] = (dust ? lg_dust : lg_inner) - (mx + logf(sum));
    }
}

__global__ __launch_bounds__(SG_FUSED_T) void k_sg_fused(SgArgs a, int iterations)
{
    extern __shared__ __attribute__((aligned(16))) float sg_smem[];
    const int b = a.b0 + blockIdx.x;
    const int m = sg_count(a.m_dev, b, a.M), n = sg_count(a.n_dev, b, a.N);
    if (sg_path(m, n, a.path) != 1) return;
    const int ld = n | 1;
    float *tile = sg_smem, *su = tile + (size_t)m * ld, *sv = su + (m + 1);
    const float *S = a.S + (long long)b * a.sp;
    for (int e = threadIdx.x; e < m * n; e += SG_FUSED_T) {
        const int i = e / n, j = e - i * n;
        tile[i * ld + j] = S[(long long)i * a.sr + (long long)j * a.sc];
    }
    for (int t = threadIdx.x; t <= m; t += SG_FUSED_T) su[t] = 0.f;
    for (int t = threadIdx.x; t <= n; t += SG_FUSED_T) sv[t] = 0.f;
    __syncthreads();
    const SgMarg g = sg_marg(m, n);
    for (int it = 0; it < iterations; ++it) {
        sg_fused_pass<false>(tile, ld, m, n, sv, su, a.alpha, g.norm, g.mu_d);
        __syncthreads();
        sg_fused_pass<true>(tile, ld, n, m, su, sv, a.alpha, g.norm, g.nu_d);
        __syncthreads();
    }
    float *u = a.u + (size_t)b * (a.M + 1), *v = a.v + (size_t)b * (a.N + 1);
    for (int t = threadIdx.x; t < m; t += SG_FUSED_T) u[t] = su[t];
    for (int t = threadIdx.x; t < n; t += SG_FUSED_T) v[t] = sv[t];
    if (threadIdx.x == 0) { u[a.M] = su[m]; v[a.N] = sv[n]; }
}

// ---- Sinkhorn: banded path ----------------------------------------------------------------------------------------------

// grid (nbmax + 1, pairs of the chunk).  Band blocks: wavefront r owns row band * SG_BAND + r -- loads it once into LDS, takes
// the maximum of Z + v (the dustbin term in lane 0), then the sum of exponentials, and writes u; then lane t of the
// workgroup owns columns t, t + SG_ROWS_T, ...: (max, sum) of Z + u over the band's rows in ascending order.  The last block
// of a pair is the dustbin row.
__global__ __launch_bounds__(SG_ROWS_T) void k_sg_rows(SgArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sg_smem[];
    __shared__ float s_u[SG_BAND], s_red[SG_ROWS_T];
    const int b = a.b0 + blockIdx.y;
    const int m = sg_count(a.m_dev, b, a.M), n = sg_count(a.n_dev, b, a.N);
    if (sg_path(m, n, a.path) != 2) return;
    float *u = a.u + (size_t)b * (a.M + 1);
    const float *v = a.v + (size_t)b * (a.N + 1);
    const float vd = v[a.N];
    const SgMarg g = sg_marg(m, n);
    if (blockIdx.x == gridDim.x - 1) {
        const float lse = sg_dustbin_lse<SG_ROWS_T>(v, n, vd, a.alpha, s_red);
        if (threadIdx.x == 0) u[a.M] = g.mu_d - lse;
        return;
    }
    const int band = blockIdx.x, r0 = band * SG_BAND;
    if (r0 >= m) return;
    const int rows = min(SG_BAND, m - r0);
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    float *tile = sg_smem;                       // [SG_BAND][n]
    if (r < rows) {
        const float *z = a.S + (long long)b * a.sp + (long long)(r0 + r) * a.sr;
        float *t = tile + (size_t)r * n;
        float mx = lane == 0 ? a.alpha + vd : SG_NINF;
        for (int j = lane; j < n; j += 64) {
            const float x = z[(long long)j * a.sc];
            t[j] = x;
            mx = fmaxf(mx, x + v[j]);
        }
        mx = sg_wave_max(mx);
        float sum = lane == 0 ? expf((a.alpha + vd) - mx) : 0.f;
        for (int j = lane; j < n; j += 64) sum += expf((t[j] + v[j]) - mx);
        sum = sg_wave_sum(sum);
        const float ui = g.norm - (mx + logf(sum));
        if (lane == 0) { u[r0 + r] = ui; s_u[r] = ui; }
    }
    __syncthreads();
    float2 *part = a.part + ((size_t)blockIdx.y * a.nbmax + band) * a.N;
    for (int j = threadIdx.x; j < n; j += SG_ROWS_T) {
        float x[SG_BAND], mx = SG_NINF;
#pragma unroll
        for (int q = 0; q < SG_BAND; ++q) {
            x[q] = q < rows ? tile[(size_t)q * n + j] + s_u[q] : SG_NINF;
            mx = fmaxf(mx, x[q]);
        }
        float sum = 0.f;
        if (mx > SG_NINF) {                      // a column that is -inf over the whole band: (-inf, 0), not exp((-inf) - (-inf))
#pragma unroll
            for (int q = 0; q < SG_BAND; ++q)
                if (q < rows) sum += expf(x[q] - mx);
        }
        part[j] = make_float2(mx, sum);
    }
}

// grid (ceil(N / SG_COLS_T) + 1, pairs of the chunk): one lane per column merges the dustbin row's term and the bands'
// partials in band order; the last block of a pair is the dustbin column.
__global__ __launch_bounds__(SG_COLS_T) void k_sg_cols(SgArgs a)
{
    __shared__ float s_red[SG_COLS_T];
    const int b = a.b0 + blockIdx.y;
    const int m = sg_count(a.m_dev, b, a.M), n = sg_count(a.n_dev, b, a.N);
    if (sg_path(m, n, a.path) != 2) return;
    const float *u = a.u + (size_t)b * (a.M + 1);
    float *v = a.v + (size_t)b * (a.N + 1);
    const float ud = u[a.M];
    const SgMarg g = sg_marg(m, n);
    if (blockIdx.x == gridDim.x - 1) {
        const float lse = sg_dustbin_lse<SG_COLS_T>(u, m, ud, a.alpha, s_red);
        if (threadIdx.x == 0) v[a.N] = g.nu_d - lse;
        return;
    }
    const int j = blockIdx.x * SG_COLS_T + threadIdx.x;
    if (j >= n) return;
    const int nb = (m + SG_BAND - 1) / SG_BAND;
    const float2 *part = a.part + (size_t)blockIdx.y * a.nbmax * a.N + j;
    const float top = a.alpha + ud;
    float mx = top;
    for (int k = 0; k < nb; ++k) mx = fmaxf(mx, part[(size_t)k * a.N].x);
    float sum = expf(top - mx);
    for (int k = 0; k < nb; ++k) {
        const float2 p = part[(size_t)k * a.N];
        if (p.x > SG_NINF) sum += p.y * expf(p.x - mx);      // an empty partial adds nothing (and no 0 * exp(-inf - mx) either)
    }
    v[j] = g.norm - (mx + logf(sum));
}

// ---- selection ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float sg_logp(float z, float ui, float vj, float norm) { return ((z + ui) + vj) - norm; }

// grid (ceil(M / SG_BAND), pairs): one wavefront per row: the largest logP of the inner block and its lowest column
__global__ __launch_bounds__(SG_ROWS_T) void k_sg_rowarg(SgArgs a)
{
    const int b = a.b0 + blockIdx.y;
    const int m = sg_count(a.m_dev, b, a.M), n = sg_count(a.n_dev, b, a.N);
    const int lane = threadIdx.x & 63, i = blockIdx.x * SG_BAND + (threadIdx.x >> 6);
    if (n == 0 || i >= m) return;
    const float *z = a.S + (long long)b * a.sp + (long long)i * a.sr;
    const float *v = a.v + (size_t)b * (a.N + 1);
    const float ui = a.u[(size_t)b * (a.M + 1) + i], norm = sg_marg(m, n).norm;
    float best = SG_NINF;
    int idx = 0x7FFFFFFF;
    for (int j = lane; j < n; j += 64) {
        const float x = sg_logp(z[(long long)j * a.sc], ui, v[j], norm);
        if (x > best || (x == best && j < idx)) { best = x; idx = j; }
    }
    for (int off = 32; off; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(idx, off);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (lane == 0) {
        a.i0[(size_t)b * a.M + i] = idx == 0x7FFFFFFF ? 0 : idx;
        a.rmax[(size_t)b * a.M + i] = best;
    }
}

// grid (ceil(N / SG_COLS_T), pairs): one lane per column walks the rows in ascending order
__global__ __launch_bounds__(SG_COLS_T) void k_sg_colarg(SgArgs a)
{
    const int b = a.b0 + blockIdx.y;
    const int m = sg_count(a.m_dev, b, a.M), n = sg_count(a.n_dev, b, a.N);
    const int j = blockIdx.x * SG_COLS_T + threadIdx.x;
    if (m == 0 || j >= n) return;
    const float *z = a.S + (long long)b * a.sp + (long long)j * a.sc;
    const float *u = a.u + (size_t)b * (a.M + 1);
    const float vj = a.v[(size_t)b * (a.N + 1) + j], norm = sg_marg(m, n).norm;
    float best = SG_NINF;
    int idx = 0;
    for (int i = 0; i < m; ++i) {
        const float x = sg_logp(z[(long long)i * a.sr], u[i], vj, norm);
        if (x > best) { best = x; idx = i; }
    }
    a.i1[(size_t)b * a.N + j] = idx;
}

// grid ((M + 1)(N + 1) / 256, pairs): the dense logP; dustbin row at M, dustbin column at N, padding 0
__global__ __launch_bounds__(256) void k_sg_logp(SgArgs a)
{
    const int b = a.b0 + blockIdx.y;
    const int m = sg_count(a.m_dev, b, a.M), n = sg_count(a.n_dev, b, a.N);
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, W = (size_t)a.N + 1;
    if (e >= ((size_t)a.M + 1) * W) return;
    const int i = (int)(e / W), j = (int)(e - (size_t)i * W);
    const bool ri = i < m, rd = i == a.M, ci = j < n, cd = j == a.N;
    float x = 0.f;
    if (m > 0 && n > 0 && (ri || rd) && (ci || cd)) {
        const float z = (ri && ci) ? a.S[(long long)b * a.sp + (long long)i * a.sr + (long long)j * a.sc] : a.alpha;
        x = sg_logp(z, a.u[(size_t)b * (a.M + 1) + i], a.v[(size_t)b * (a.N + 1) + j], sg_marg(m, n).norm);
    }
    a.logp[(size_t)b * (a.M + 1) * W + e] = x;
}

// grid (pairs): status, mutual check, scores, thresholds, table, count
__global__ __launch_bounds__(SG_COLS_T) void k_sg_select(SgArgs a)
{
    __shared__ int s_count;
    const int b = a.b0 + blockIdx.x, tid = threadIdx.x;
    const int m = sg_count(a.m_dev, b, a.M), n = sg_count(a.n_dev, b, a.N);
    const float *u = a.u + (size_t)b * (a.M + 1), *v = a.v + (size_t)b * (a.N + 1);
    int bad = 0;
    if (m > 0 && n > 0) {
        for (int i = tid; i < m; i += SG_COLS_T) bad |= !isfinite(u[i]);
        for (int j = tid; j < n; j += SG_COLS_T) bad |= !isfinite(v[j]);
        if (tid == 0) bad |= !isfinite(u[a.M]) || !isfinite(v[a.N]);
    }
    if (tid == 0) s_count = 0;
    bad = __syncthreads_or(bad);
    const bool live = m > 0 && n > 0 && !bad;
    const int32_t *i0 = a.i0 + (size_t)b * a.M, *i1 = a.i1 + (size_t)b * a.N;
    const float *rmax = a.rmax + (size_t)b * a.M;
    int mine = 0;
    for (int i = tid; i < a.M; i += SG_COLS_T) {
        int32_t m0 = -1, t = -1;
        float ms = 0.f;
        if (live && i < m) {
            const int j = i0[i];
            if (i1[j] == i) {
                ms = expf(rmax[i]);
                if ((double)ms > a.mt) m0 = j;
                if (m0 >= 0 && (double)ms > a.st) t = j;
            }
        }
        a.matches0[(size_t)b * a.M + i] = m0;
        if (a.ms0) a.ms0[(size_t)b * a.M + i] = ms;
        if (a.table) a.table[(size_t)b * a.ts + i] = t;
        mine += t >= 0;
    }
    if (a.table)
        for (long long i = a.M + tid; i < a.ts; i += SG_COLS_T) a.table[(size_t)b * a.ts + i] = -1;
    if (a.matches1 || a.ms1)
        for (int j = tid; j < a.N; j += SG_COLS_T) {
            int32_t m1 = -1;
            float ms = 0.f;
            if (live && j < n) {
                const int i = i1[j];
                if (i0[i] == j) {
                    ms = expf(rmax[i]);
                    if ((double)ms > a.mt) m1 = i;
                }
            }
            if (a.matches1) a.matches1[(size_t)b * a.N + j] = m1;
            if (a.ms1) a.ms1[(size_t)b * a.N + j] = ms;
        }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (tid == 0) {
        if (a.counts) a.counts[b] = s_count;
        if (a.status) a.status[b] = bad ? 1 : 0;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

size_t sg_align(size_t b) { return (b + 255) & ~(size_t)255; }
bool sg_fits_host(int64_t m, int64_t n) { return (size_t)(m + 1) * (size_t)(n + 1) * 4 <= SG_LDS; }
size_t sg_fused_lds(int32_t M, int32_t N) { return std::min<size_t>(SG_LDS, (size_t)(M + 1) * (N + 1) * 4) + 4 * ((size_t)M + 2); }

int sg_setup(rcn_ctx *ctx)
{
    static std::mutex once_mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> lk(once_mu);
    if (std::find(done.begin(), done.end(), ctx->device) == done.end()) {
        RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sg_fused), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sg_fused_lds(SG_MAX, SG_MAX)));
        RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sg_rows), hipFuncAttributeMaxDynamicSharedMemorySize, SG_BAND * SG_MAX * 4));
        done.push_back(ctx->device);
    }
    return RCN_OK;
}

bool sg_fail(rcn_ctx *ctx, const char *who, const char *why)
{
    ctx->set_error(std::string(who) + ": bad argument (" + why + ")");
    return false;
}
bool sg_check_shape(rcn_ctx *ctx, const char *who, int32_t B, int32_t M, int32_t N, int *rc)
{
    *rc = RCN_ERR_ARG;
    if (B < 0) return sg_fail(ctx, who, "B < 0");
    if (M < 1 || N < 1) return sg_fail(ctx, who, "M and N must be positive");
    if (M > SG_MAX || N > SG_MAX) {
        *rc = RCN_ERR_UNSUPPORTED;
        ctx->set_error(std::string(who) + ": M or N above " + std::to_string(SG_MAX));
        return false;
    }
    return true;
}
bool sg_check_options(rcn_ctx *ctx, const char *who, const rcn_sg_options &o)
{
    if (!std::isfinite(o.alpha)) return sg_fail(ctx, who, "alpha is not finite");
    if (!(o.match_threshold >= 0.0 && o.match_threshold < 1.0) || !(o.score_threshold >= 0.0 && o.score_threshold < 1.0))
        return sg_fail(ctx, who, "a threshold outside [0, 1)");
    if (o.iterations < 0) return sg_fail(ctx, who, "iterations < 0");
    if (o.path != RCN_SG_PATH_AUTO && o.path != RCN_SG_PATH_FUSED && o.path != RCN_SG_PATH_BANDED) return sg_fail(ctx, who, "unknown path");
    return true;
}

int sg_scores(rcn_ctx *ctx, const float *d0, int64_t sp0, int64_t sr0, int64_t sd0, const float *d1, int64_t sp1, int64_t sr1, int64_t sd1,
              const int32_t *m_dev, const int32_t *n_dev, int32_t B, int32_t M, int32_t N, int32_t D, float *out)
{
    for (int32_t b0 = 0; b0 < B; b0 += SG_SLICE) {
        const dim3 grid((unsigned)((N + SC_T - 1) / SC_T), (unsigned)((M + SC_T - 1) / SC_T), (unsigned)std::min(SG_SLICE, B - b0));
        k_sg_scores<<<grid, 256, 0, ctx->stream>>>(d0, sp0, sr0, sd0, d1, sp1, sr1, sd1, m_dev, n_dev, b0, M, N, D, out);
    }
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

struct SgOut {
    int32_t *matches0, *matches1;
    float *ms0, *ms1;
    int32_t *table;
    int64_t ts;
    int32_t *counts;
    float *logp;
    int32_t *status;
};
bool sg_check_out(rcn_ctx *ctx, const char *who, const SgOut &o, int32_t M)
{
    if (!o.matches0) return sg_fail(ctx, who, "null pointer");
    if (o.table && !o.counts) return sg_fail(ctx, who, "a table without counts");
    if (o.table && o.ts < M) return sg_fail(ctx, who, "table_stride < M");
    return true;
}

// with ctx->mu held and the arguments checked
int sg_assign(rcn_ctx *ctx, const char *who, const float *S, int64_t sp, int64_t sr, int64_t sc, const int32_t *m_dev, const int32_t *n_dev,
              int32_t B, int32_t M, int32_t N, const rcn_sg_options &opt, const SgOut &o)
{
    const bool all_fit = sg_fits_host(M, N);
    if (opt.path == RCN_SG_PATH_FUSED && !all_fit) {
        ctx->set_error(std::string(who) + ": the fused path needs (M + 1)(N + 1) floats to fit " + std::to_string(SG_LDS) + " bytes of LDS");
        return RCN_ERR_UNSUPPORTED;
    }
    if (int rc = sg_setup(ctx)) return rc;
    const bool run_fused = opt.path != RCN_SG_PATH_BANDED && (all_fit || m_dev || n_dev);
    const bool run_banded = opt.path == RCN_SG_PATH_BANDED || (opt.path == RCN_SG_PATH_AUTO && !all_fit);
    const int nbmax = (M + SG_BAND - 1) / SG_BAND;
    // pairs per chunk: the budget of score matrices, the cap of the partials, the launch slice
    const size_t mat = (size_t)M * N * 4, part1 = (size_t)nbmax * N * sizeof(float2);
    size_t chunk = SG_SLICE;
    if (ctx->sg_chunk_bytes > 0) chunk = std::min(chunk, std::max<size_t>(1, (size_t)ctx->sg_chunk_bytes / mat));
    if (run_banded) chunk = std::min(chunk, std::max<size_t>(1, SG_PART_BYTES / part1));
    chunk = std::min(chunk, (size_t)B);
    const size_t b_u = sg_align((size_t)B * (M + 1) * 4), b_v = sg_align((size_t)B * (N + 1) * 4), b_m = sg_align((size_t)B * M * 4),
                 b_n = sg_align((size_t)B * N * 4), b_p = run_banded ? sg_align(chunk * part1) : 0;
    RCN_HIP(ctx->sg_ws.reserve(b_u + b_v + 2 * b_m + b_n + b_p));
    char *ws = ctx->sg_ws.as<char>();
    SgArgs a{};
    a.S = S; a.sp = sp; a.sr = sr; a.sc = sc;
    a.m_dev = m_dev; a.n_dev = n_dev;
    a.M = M; a.N = N; a.path = opt.path; a.nbmax = nbmax;
    a.alpha = (float)opt.alpha;
    a.u = reinterpret_cast<float *>(ws);             ws += b_u;
    a.v = reinterpret_cast<float *>(ws);             ws += b_v;
    a.i0 = reinterpret_cast<int32_t *>(ws);          ws += b_m;
    a.rmax = reinterpret_cast<float *>(ws);          ws += b_m;
    a.i1 = reinterpret_cast<int32_t *>(ws);          ws += b_n;
    a.part = reinterpret_cast<float2 *>(ws);
    a.mt = opt.match_threshold; a.st = opt.score_threshold;
    a.matches0 = o.matches0; a.matches1 = o.matches1; a.ms0 = o.ms0; a.ms1 = o.ms1;
    a.table = o.table; a.ts = o.ts; a.counts = o.counts; a.logp = o.logp; a.status = o.status;
    RCN_HIP(hipMemsetAsync(a.u, 0, b_u + b_v, ctx->stream));        // u = v = 0
    for (int32_t b0 = 0; b0 < B; b0 += (int32_t)chunk) {
        const unsigned nb = (unsigned)std::min<size_t>(chunk, (size_t)(B - b0));
        a.b0 = b0;
        if (run_fused) k_sg_fused<<<nb, SG_FUSED_T, sg_fused_lds(M, N), ctx->stream>>>(a, opt.iterations);
        if (run_banded)
            for (int it = 0; it < opt.iterations; ++it) {
                k_sg_rows<<<dim3((unsigned)nbmax + 1, nb), SG_ROWS_T, (size_t)SG_BAND * N * 4, ctx->stream>>>(a);
                k_sg_cols<<<dim3((unsigned)((N + SG_COLS_T - 1) / SG_COLS_T) + 1, nb), SG_COLS_T, 0, ctx->stream>>>(a);
            }
        k_sg_rowarg<<<dim3((unsigned)nbmax, nb), SG_ROWS_T, 0, ctx->stream>>>(a);
        k_sg_colarg<<<dim3((unsigned)((N + SG_COLS_T - 1) / SG_COLS_T), nb), SG_COLS_T, 0, ctx->stream>>>(a);
        if (o.logp) k_sg_logp<<<dim3((unsigned)(((size_t)(M + 1) * (N + 1) + 255) / 256), nb), 256, 0, ctx->stream>>>(a);
        k_sg_select<<<nb, SG_COLS_T, 0, ctx->stream>>>(a);
        RCN_HIP(hipGetLastError());
    }
    return RCN_OK;
}

}  // namespace

extern "C" void rcn_sg_default_options(rcn_sg_options *o)
{
    if (!o) return;
    o->alpha = 1.0;
    o->match_threshold = 0.2;
    o->score_threshold = 0.5;
    o->iterations = 100;
    o->path = RCN_SG_PATH_AUTO;
}

extern "C" int rcn_sg_set_chunk_bytes(rcn_ctx *ctx, int64_t bytes)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->sg_chunk_bytes = bytes;
    return RCN_OK;
}

extern "C" int rcn_sg_scores_device(rcn_ctx *ctx, const float *d0_dev, int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0,
                                    const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                                    const int32_t *m_dev, const int32_t *n_dev, int32_t B, int32_t M, int32_t N, int32_t D, float *scores_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sg_scores_device";
    int rc;
    if (!sg_check_shape(ctx, who, B, M, N, &rc)) return rc;
    if (D < 1) { sg_fail(ctx, who, "D < 1"); return RCN_ERR_ARG; }
    if (!d0_dev || !d1_dev || !scores_out_dev) { sg_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    if (B == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    return sg_scores(ctx, d0_dev, stride_pair0, stride_row0, stride_d0, d1_dev, stride_pair1, stride_row1, stride_d1, m_dev, n_dev, B, M, N, D, scores_out_dev);
}

extern "C" int rcn_sg_assign_device(rcn_ctx *ctx, const float *scores_dev, int64_t stride_pair, int64_t stride_row, int64_t stride_col,
                                    const int32_t *m_dev, const int32_t *n_dev, int32_t B, int32_t M, int32_t N, const rcn_sg_options *opt,
                                    int32_t *matches0_dev, int32_t *matches1_dev, float *mscores0_dev, float *mscores1_dev,
                                    int32_t *table_dev, int64_t table_stride, int32_t *counts_dev, float *logP_out_dev, int32_t *status_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sg_assign_device";
    rcn_sg_options o;
    rcn_sg_default_options(&o);
    if (opt) o = *opt;
    const SgOut out{matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, table_dev, table_stride, counts_dev, logP_out_dev, status_dev};
    int rc;
    if (!sg_check_shape(ctx, who, B, M, N, &rc)) return rc;
    if (!sg_check_options(ctx, who, o) || !sg_check_out(ctx, who, out, M)) return RCN_ERR_ARG;
    if (!scores_dev) { sg_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    if (B == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    return sg_assign(ctx, who, scores_dev, stride_pair, stride_row, stride_col, m_dev, n_dev, B, M, N, o, out);
}

int rcn_int_sg_match(rcn_ctx *ctx, const char *who, const float *d0_dev, int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0,
                     const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                     const int32_t *m_dev, const int32_t *n_dev, int32_t B, int32_t M, int32_t N, int32_t D, const rcn_sg_options *opt,
                     int32_t *matches0_dev, int32_t *matches1_dev, float *mscores0_dev, float *mscores1_dev,
                     int32_t *table_dev, int64_t table_stride, int32_t *counts_dev, float *logP_out_dev, int32_t *status_dev, bool check_only)
{
    rcn_sg_options o;
    rcn_sg_default_options(&o);
    if (opt) o = *opt;
    const SgOut out{matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, table_dev, table_stride, counts_dev, logP_out_dev, status_dev};
    int rc;
    if (!sg_check_shape(ctx, who, B, M, N, &rc)) return rc;
    if (D < 1) { sg_fail(ctx, who, "D < 1"); return RCN_ERR_ARG; }
    if (!sg_check_options(ctx, who, o) || !sg_check_out(ctx, who, out, M)) return RCN_ERR_ARG;
    if (check_only) return RCN_OK;
    if (!d0_dev || !d1_dev) { sg_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    if (B == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(ctx->sg_scores.reserve((size_t)B * M * N * 4));
    float *S = ctx->sg_scores.as<float>();
    if ((rc = sg_scores(ctx, d0_dev, stride_pair0, stride_row0, stride_d0, d1_dev, stride_pair1, stride_row1, stride_d1, m_dev, n_dev, B, M, N, D, S))) return rc;
    return sg_assign(ctx, who, S, (int64_t)M * N, N, 1, m_dev, n_dev, B, M, N, o, out);
}

extern "C" int rcn_sg_match_device(rcn_ctx *ctx, const float *d0_dev, int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0,
                                   const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                                   const int32_t *m_dev, const int32_t *n_dev, int32_t B, int32_t M, int32_t N, int32_t D, const rcn_sg_options *opt,
                                   int32_t *matches0_dev, int32_t *matches1_dev, float *mscores0_dev, float *mscores1_dev,
                                   int32_t *table_dev, int64_t table_stride, int32_t *counts_dev, float *logP_out_dev, int32_t *status_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return rcn_int_sg_match(ctx, "rcn_sg_match_device", d0_dev, stride_pair0, stride_row0, stride_d0, d1_dev, stride_pair1, stride_row1, stride_d1, m_dev, n_dev,
                            B, M, N, D, opt, matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, table_dev, table_stride, counts_dev, logP_out_dev,
                            status_dev, false);
}
