// guided.hip -- guided matching: the exact 2-NN of every query row inside the epipolar band of its pair.
//
//   k_gd_top2    one wave per (pair, GD_Q query rows).  The wave sweeps the train image's coordinates 64 rows at a time: each lane computes
//                its train point's line (gb_line: a', b', c', thr2 q1) once per tile and tests it against the GD_Q query lines kept in LDS
//                (gb_test: ~10 fp64 operations), ballots the candidates and appends them to a pending list in LDS.  Whenever 64
//                candidates are pending, every lane takes one: the 64 train rows and the wave's query rows are staged in LDS 32 floats
//                at a time with whole 128-byte segments (8 lanes per row, k_exact_rows_lds's staging, match.hip), and each lane walks
//                the canonical fp64 chain of its own (query, train) entry across the chunks; lane r then folds the results of query
//                row r into its top-2 under (d2, row), merge_top2's rule.  D % 4 != 0: the same list, every lane walks its chain out of
//                global memory (the same bits).  The whole-row gather of exact_gather.h was measured first and lost: section 30.
//   k_gd_claim   lowest query row per train row (uniqueness, FeatureMatcher.cpp:58-62)
//   k_gd_emit    keeps out[q] = t iff ws[t] == q, -1 elsewhere and in the tail, counts.  ws is the owner table of k_gd_claim, or -- cross
//                check -- the accepted train -> query choices of the reversed pair (k_gd_top2 with the roles swapped and F transposed)
// No K1 x K2 array exists: the only workspace is one int32 per train row of a chunk of pairs.
#include "rcn_internal.h"
#include "guided_band.h"

#include <algorithm>
#include <cmath>

namespace {

#define GD_Q 16                    // query rows of a wave
#define GD_B 64                    // entries of a batch of chains: one per lane
#define GD_PEND (GD_B + 64)        // pending candidates: fewer than GD_B before a sweep step, which adds at most 64
#define GD_LD 36                   // floats per staged row: a chunk of 32 + 4 of padding (rows 144 bytes apart: conflict-free b128 reads)
#define GD_NONE 0x7FFFFFFF

struct GdPair {
    const float *q, *t;            // fp32 rows of the query / train image
    const int32_t *xyq, *xyt;      // their integer pixel coordinates
    int32_t Kq, Kt;
    int64_t ws_off;                // first slot of the pair's train rows in the chunk's workspace
};

struct GdArgs {
    const GdPair *pairs;
    const double *F;               // [n_pairs][9]
    const int32_t *verdict;        // may be NULL; a pair whose verdict is <= 0 is skipped by every kernel
    int32_t *out;                  // may be NULL: accepted train row per query row, before uniqueness ([pair][out_stride]); reversed: ws
    int64_t out_stride;
    int32_t *ws;
    int32_t *idx;                  // may be NULL: (j0, j1, candidates, 0) per query row
    double *d2;                    //              their squared distances
    int64_t knn_stride;
    unsigned long long *cand;      // may be NULL: in-band combinations per pair (zeroed by the caller)
    double thr2;
    float ratio, max_distance;
    int32_t D, qblocks, reversed;
};

__device__ __forceinline__ void top2_insert(double &b0, int &i0, double &b1, int &i1, double c, int j)
{
    const bool first = c < b0 || (c == b0 && j < i0);
    const bool second = !first && (c < b1 || (c == b1 && j < i1));
    const double n1 = first ? b0 : (second ? c : b1);
    const int m1 = first ? i0 : (second ? j : i1);
    b0 = first ? c : b0; i0 = first ? j : i0;
    b1 = n1; i1 = m1;
}

template <bool VEC4>
__global__ __launch_bounds__(64) void k_gd_top2(GdArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_t[VEC4 ? GD_B * GD_LD : 4], s_q[VEC4 ? GD_Q * GD_LD : 4];
    __shared__ GbLine s_line[GD_Q];
    __shared__ double s_x[GD_Q], s_y[GD_Q], s_d[GD_B];
    __shared__ int s_pq[GD_PEND], s_pt[GD_PEND];
    const int lane = threadIdx.x;
    const int pair = blockIdx.x / a.qblocks, q0 = (blockIdx.x - pair * a.qblocks) * GD_Q;
    if (a.verdict && a.verdict[pair] <= 0) return;
    const GdPair pr = a.pairs[pair];
    const int rev = a.reversed;
    const float *qrows = rev ? pr.t : pr.q, *trows = rev ? pr.q : pr.t;
    const int32_t *xyq = rev ? pr.xyt : pr.xyq, *xyt = rev ? pr.xyq : pr.xyt;
    const int Kq = rev ? pr.Kt : pr.Kq, Kt = rev ? pr.Kq : pr.Kt;
    if (q0 >= Kq) return;
    const int nq = min(GD_Q, Kq - q0), D = a.D;
    double F[9];
    for (int k = 0; k < 9; ++k) F[k] = a.F[9 * (size_t)pair + k];

    // the wave's query rows: their lines
    if (lane < GD_Q) {
        GbLine l; l.a = l.b = l.c = 0.0; l.lim = -1.0;
        double x = 0.0, y = 0.0;
        if (lane < nq) {
            x = (double)xyq[2 * (size_t)(q0 + lane)]; y = (double)xyq[2 * (size_t)(q0 + lane) + 1];
            l = gb_line(F, rev, x, y, a.thr2);
        }
        s_line[lane] = l; s_x[lane] = x; s_y[lane] = y;
    }
    __syncthreads();

    double b0 = INFINITY, b1 = INFINITY;       // lane r < nq: the top-2 of query row q0 + r
    int i0 = GD_NONE, i1 = GD_NONE, cnt = 0;
    unsigned np = 0;                           // uniform over the wave

    // the canonical chains of pending entries [base, base + n), n <= GD_B, one per lane, folded into the owning lanes' top-2
    auto batch = [&](unsigned base, unsigned n) {
        __syncthreads();                       // the list as the sweep left it
        const bool live = (unsigned)lane < n;
        int qi = 0, t = 0;
        if (live) { qi = s_pq[base + lane]; t = s_pt[base + lane]; }
        double d = 0.0;
        if (VEC4) {
            const int sub = lane >> 3, c4 = (lane & 7) * 4;
            const int nchunk = (D + 31) / 32;
            for (int ch = 0; ch < nchunk; ++ch) {
                const int col = ch * 32 + c4;
                float4 v[8], w[GD_Q / 8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {              // entry i * 8 + sub: 8 lanes read one 128-byte segment of its train row
                    const unsigned e = (unsigned)(i * 8 + sub);
                    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (e < n && col < D) v[i] = *reinterpret_cast<const float4 *>(trows + (size_t)s_pt[base + e] * D + col);
                }
#pragma unroll
                for (int i = 0; i < GD_Q / 8; ++i) {
                    const int r = i * 8 + sub;
                    w[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (r < nq && col < D) w[i] = *reinterpret_cast<const float4 *>(qrows + (size_t)(q0 + r) * D + col);
                }
                __syncthreads();                           // the previous chunk's LDS reads are done
#pragma unroll
                for (int i = 0; i < 8; ++i) *reinterpret_cast<float4 *>(s_t + (i * 8 + sub) * GD_LD + c4) = v[i];
#pragma unroll
                for (int i = 0; i < GD_Q / 8; ++i) *reinterpret_cast<float4 *>(s_q + (i * 8 + sub) * GD_LD + c4) = w[i];
                __syncthreads();
                const int kmax = min(32, D - ch * 32);
                const float *x = s_q + qi * GD_LD, *y = s_t + lane * GD_LD;
                for (int k4 = 0; k4 < kmax; k4 += 4) {
                    const float4 xv = *reinterpret_cast<const float4 *>(x + k4), yv = *reinterpret_cast<const float4 *>(y + k4);
                    double e;
                    e = (double)xv.x - (double)yv.x; d = fma(e, e, d);
                    e = (double)xv.y - (double)yv.y; d = fma(e, e, d);
                    e = (double)xv.z - (double)yv.z; d = fma(e, e, d);
                    e = (double)xv.w - (double)yv.w; d = fma(e, e, d);
                }
            }
        } else if (live) {
            const float *x = qrows + (size_t)(q0 + qi) * D, *y = trows + (size_t)t * D;
            for (int k = 0; k < D; ++k) {
                const double e = (double)x[k] - (double)y[k];
                d = fma(e, e, d);
            }
        }
        s_d[lane] = d;
        __syncthreads();
        if (lane < nq)
            for (unsigned i = 0; i < n; ++i)
                if (s_pq[base + i] == lane) top2_insert(b0, i0, b1, i1, s_d[i], s_pt[base + i]);
        __syncthreads();                       // before the staged rows, s_d and the list's tail are written again
    };

    for (int t0 = 0; t0 < Kt; t0 += 64) {
        const int t = t0 + lane;
        GbLine lt; lt.a = lt.b = lt.c = 0.0; lt.lim = -1.0;
        double x2 = 0.0, y2 = 0.0;
        if (t < Kt) {
            x2 = (double)xyt[2 * (size_t)t]; y2 = (double)xyt[2 * (size_t)t + 1];
            lt = gb_line(F, !rev, x2, y2, a.thr2);
        }
        for (int qi = 0; qi < nq; ++qi) {
            const bool c = gb_test(s_line[qi], s_x[qi], s_y[qi], lt, x2, y2);      // lt.lim = -1 past the image: never a candidate
            const unsigned long long m = __ballot(c);
            if (!m) continue;
            const unsigned add = (unsigned)__popcll(m);
            if (lane == qi) cnt += (int)add;
            if (c) {
                const unsigned slot = np + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                s_pq[slot] = qi; s_pt[slot] = t;
            }
            np += add;
            while (np >= GD_B) { batch(np - GD_B, GD_B); np -= GD_B; }
        }
    }
    if (np) batch(0, np);

    if (lane < nq) {
        const int q = q0 + lane;
        const bool have = i0 != GD_NONE;
        if (a.out) {
            int r = -1;
            if (have) {
                const float dist0 = sqrtf((float)b0), dist1 = sqrtf((float)b1);      // b1 = +inf for a lone candidate
                bool ok = dist0 < a.ratio * dist1;
                if (a.max_distance > 0.f) ok = ok && dist0 <= a.max_distance;
                if (ok) r = i0;
            }
            if (rev) a.ws[pr.ws_off + q] = r;
            else a.out[(size_t)pair * a.out_stride + q] = r;
        }
        if (a.idx) {
            const size_t o = (size_t)pair * a.knn_stride + q;
            reinterpret_cast<int4 *>(a.idx)[o] = make_int4(have ? i0 : -1, i1 != GD_NONE ? i1 : -1, cnt, 0);
            reinterpret_cast<double2 *>(a.d2)[o] = make_double2(b0, b1);
        }
    }
    if (a.cand) {
        int s = lane < nq ? cnt : 0;
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0 && s) atomicAdd(a.cand + pair, (unsigned long long)s);
    }
}

__global__ __launch_bounds__(256) void k_gd_knn_fill(int4 *idx, double2 *d2, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        idx[i] = make_int4(-1, -1, 0, 0);
        d2[i] = make_double2(INFINITY, INFINITY);
    }
}

__global__ __launch_bounds__(256) void k_gd_claim(const GdPair *pairs, const int32_t *verdict, const int32_t *out, int64_t out_stride, int32_t *ws)
{
    const int pair = blockIdx.x;
    if (verdict && verdict[pair] <= 0) return;
    const GdPair pr = pairs[pair];
    const int32_t *row = out + (size_t)pair * out_stride;
    for (int q = blockIdx.y * 256 + threadIdx.x; q < pr.Kq; q += gridDim.y * 256) {
        const int t = row[q];
        if (t >= 0) atomicMin(ws + pr.ws_off + t, q);
    }
}

__global__ __launch_bounds__(256) void k_gd_emit(const GdPair *pairs, const int32_t *verdict, int32_t *out, int64_t out_stride, const int32_t *ws,
                                                 int32_t *counts)
{
    __shared__ int wsum[4];
    const int pair = blockIdx.x, t = threadIdx.x;
    if (verdict && verdict[pair] <= 0) return;
    const GdPair pr = pairs[pair];
    int32_t *row = out + (size_t)pair * out_stride;
    int kept = 0;
    for (int64_t q0 = 0; q0 < out_stride; q0 += 256) {
        const int64_t q = q0 + t;
        bool keep = false;
        if (q < out_stride) {
            const int tr = q < pr.Kq ? row[q] : -1;
            keep = tr >= 0 && ws[pr.ws_off + tr] == (int)q;
            if (!keep) row[q] = -1;
        }
        kept += (int)__popcll(__ballot(keep));
    }
    if ((t & 63) == 0) wsum[t >> 6] = kept;
    __syncthreads();
    if (t == 0) counts[pair] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

struct GdPlan {
    std::vector<GdPair> pairs;
    int32_t kq_max = 0, kt_max = 0;
};

int gd_check_options(rcn_ctx *ctx, const char *who, float ratio, float max_error_px)
{
    if (!(ratio > 0.f) || !std::isfinite(ratio)) { ctx->set_error(std::string(who) + ": the ratio must be finite and positive"); return RCN_ERR_ARG; }
    if (!(max_error_px > 0.f)) { ctx->set_error(std::string(who) + ": max_error_px must be positive (+inf is allowed)"); return RCN_ERR_ARG; }
    return RCN_OK;
}

// the caller's pair list over the resident descriptors and coordinates
int gd_plan(rcn_ctx *ctx, const char *who, const int32_t *pairs_host, int32_t n_pairs, int64_t stride, GdPlan &pl)
{
    pl.pairs.resize((size_t)n_pairs);
    for (int32_t p = 0; p < n_pairs; ++p) {
        GdPair &g = pl.pairs[p];
        const int32_t id[2] = {pairs_host[2 * p], pairs_host[2 * p + 1]};
        for (int s = 0; s < 2; ++s) {
            auto im = ctx->images.find(id[s]);
            auto xy = ctx->coords.find(id[s]);
            if (im == ctx->images.end()) { ctx->set_error(std::string(who) + ": image " + std::to_string(id[s]) + " has no resident descriptors"); return RCN_ERR_NOT_FOUND; }
            if (xy == ctx->coords.end()) { ctx->set_error(std::string(who) + ": coordinates of image " + std::to_string(id[s]) + " are not resident"); return RCN_ERR_NOT_FOUND; }
            if (im->second.K != xy->second.second) { ctx->set_error(std::string(who) + ": an image's coordinate count differs from its descriptor count"); return RCN_ERR_ARG; }
            (s ? g.t : g.q) = im->second.f32;
            (s ? g.xyt : g.xyq) = xy->second.first.as<int32_t>();
            (s ? g.Kt : g.Kq) = im->second.K;
        }
        if (g.Kq > stride) { ctx->set_error(std::string(who) + ": the row stride is smaller than a query image"); return RCN_ERR_ARG; }
        g.ws_off = 0;
        pl.kq_max = std::max(pl.kq_max, g.Kq);
        pl.kt_max = std::max(pl.kt_max, g.Kt);
    }
    return RCN_OK;
}

// pl.pairs -> the match table and counts (out_dev != NULL) and / or the knn tables (idx_dev != NULL), chunk by chunk
int gd_run(rcn_ctx *ctx, GdPlan &pl, int32_t D, const double *F_dev, const int32_t *verdict_dev, double thr2, float ratio, float max_distance,
           int cross_check, int32_t *out_dev, int64_t out_stride, int32_t *counts_dev, int64_t *cand_dev, int32_t *idx_dev, double *d2_dev,
           int64_t knn_stride)
{
    const int32_t n_pairs = (int32_t)pl.pairs.size();
    if (n_pairs == 0) return RCN_OK;
    hipStream_t st = ctx->stream;
    // chunks of consecutive pairs whose train rows fit the workspace budget (one pair always fits: the buffer grows to it)
    const int64_t rows_cap = std::max<int64_t>(1, ctx->chunk_rows);
    std::vector<int32_t> first(1, 0);
    int64_t used = 0, ws_rows = 1;
    for (int32_t p = 0; p < n_pairs; ++p) {
        if (used > 0 && used + pl.pairs[p].Kt > rows_cap) { first.push_back(p); used = 0; }
        pl.pairs[p].ws_off = used;
        used += pl.pairs[p].Kt;
        ws_rows = std::max(ws_rows, used);
    }
    first.push_back(n_pairs);
    const size_t pair_bytes = sizeof(GdPair) * (size_t)n_pairs;
    ctx->gd_pairs_host.assign(reinterpret_cast<const char *>(pl.pairs.data()), reinterpret_cast<const char *>(pl.pairs.data()) + pair_bytes);
    RCN_HIP(ctx->gd_pairs.reserve(pair_bytes));
    if (out_dev) RCN_HIP(ctx->gd_ws.reserve((size_t)ws_rows * 4));
    RCN_HIP(hipMemcpyAsync(ctx->gd_pairs.p, ctx->gd_pairs_host.data(), pair_bytes, hipMemcpyHostToDevice, st));
    if (cand_dev) RCN_HIP(hipMemsetAsync(cand_dev, 0, 8 * (size_t)n_pairs, st));
    if (idx_dev) {
        const size_t n = (size_t)n_pairs * (size_t)knn_stride;
        if (n) k_gd_knn_fill<<<(unsigned)std::min<size_t>((n + 255) / 256, 4096), 256, 0, st>>>(reinterpret_cast<int4 *>(idx_dev), reinterpret_cast<double2 *>(d2_dev), n);
        RCN_HIP(hipGetLastError());
    }
    const bool vec4 = D % 4 == 0;
    for (size_t c = 0; c + 1 < first.size(); ++c) {
        const int32_t p0 = first[c], np = first[c + 1] - p0;
        int32_t kq_max = 0, kt_max = 0;
        int64_t rows = 0;
        for (int32_t p = p0; p < p0 + np; ++p) { kq_max = std::max(kq_max, pl.pairs[p].Kq); kt_max = std::max(kt_max, pl.pairs[p].Kt); rows += pl.pairs[p].Kt; }
        GdArgs a;
        a.pairs = ctx->gd_pairs.as<GdPair>() + p0;
        a.F = F_dev + 9 * (size_t)p0;
        a.verdict = verdict_dev ? verdict_dev + p0 : nullptr;
        a.out = out_dev ? out_dev + (size_t)p0 * out_stride : nullptr;
        a.out_stride = out_stride;
        a.ws = ctx->gd_ws.as<int32_t>();
        a.idx = idx_dev ? idx_dev + 4 * (size_t)p0 * knn_stride : nullptr;
        a.d2 = d2_dev ? d2_dev + 2 * (size_t)p0 * knn_stride : nullptr;
        a.knn_stride = knn_stride;
        a.cand = cand_dev ? reinterpret_cast<unsigned long long *>(cand_dev) + p0 : nullptr;
        a.thr2 = thr2; a.ratio = ratio; a.max_distance = max_distance; a.D = D;
        auto sweep = [&](int reversed, int32_t kmax) {
            if (kmax <= 0) return;
            a.reversed = reversed;
            a.qblocks = (kmax + GD_Q - 1) / GD_Q;
            const dim3 g((unsigned)((int64_t)np * a.qblocks));
            if (vec4) k_gd_top2<true><<<g, 64, 0, st>>>(a);
            else k_gd_top2<false><<<g, 64, 0, st>>>(a);
        };
        sweep(0, kq_max);
        RCN_HIP(hipGetLastError());
        if (!out_dev) continue;
        if (cross_check) {
            GdArgs b = a;
            a.idx = nullptr; a.d2 = nullptr; a.cand = nullptr;      // the reversed sweep writes the workspace alone
            sweep(1, kt_max);
            a = b;
        } else {
            if (rows) RCN_HIP(hipMemsetAsync(ctx->gd_ws.p, 0x7F, (size_t)rows * 4, st));
            if (kq_max > 0) k_gd_claim<<<dim3((unsigned)np, (unsigned)std::min((kq_max + 255) / 256, 64)), 256, 0, st>>>(a.pairs, a.verdict, a.out, out_stride, a.ws);
        }
        RCN_HIP(hipGetLastError());
        k_gd_emit<<<(unsigned)np, 256, 0, st>>>(a.pairs, a.verdict, a.out, out_stride, a.ws, counts_dev + p0);
        RCN_HIP(hipGetLastError());
    }
    return RCN_OK;
}

int gd_check_opt(rcn_ctx *ctx, const char *who, const rcn_guided_options *opt)
{
    if (!opt) { ctx->set_error(std::string(who) + ": null options"); return RCN_ERR_ARG; }
    if (int rc = gd_check_options(ctx, who, opt->ratio, opt->max_error_px)) return rc;
    if (std::isnan(opt->max_distance)) { ctx->set_error(std::string(who) + ": max_distance is not a number"); return RCN_ERR_ARG; }
    return RCN_OK;
}

double gd_thr2(float max_error_px) { return (double)max_error_px * (double)max_error_px; }

}  // namespace

void rcn_int_guided_release(rcn_ctx *ctx)
{
    ctx->gd_pairs.release(); ctx->gd_ws.release(); ctx->gd_hws.release(); ctx->gd_F.release();
}

extern "C" {

int rcn_guided_default_options(rcn_guided_options *o)
{
    if (!o) return RCN_ERR_ARG;
    o->ratio = 0.7f; o->max_error_px = 3.0f; o->max_distance = 0.f; o->cross_check = 0;
    return RCN_OK;
}

int rcn_match_guided_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, const double *F_dev, const rcn_guided_options *opt,
                            int32_t *out_dev, int64_t out_stride, int32_t *counts_dev, int64_t *cand_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_match_guided_device";
    if (int rc = gd_check_opt(ctx, who, opt)) return rc;
    if (n_pairs < 0 || out_stride < 0 || (n_pairs > 0 && (!pairs_host || !F_dev || !out_dev || !counts_dev))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    if (n_pairs == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    GdPlan pl;
    if (int rc = gd_plan(ctx, who, pairs_host, n_pairs, out_stride, pl)) return rc;
    return gd_run(ctx, pl, ctx->D, F_dev, nullptr, gd_thr2(opt->max_error_px), opt->ratio, opt->max_distance, opt->cross_check, out_dev, out_stride,
                  counts_dev, cand_dev, nullptr, nullptr, 0);
}

int rcn_match_guided(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, const double *F_host, const rcn_guided_options *opt,
                     int32_t *out_host, int64_t out_stride, int32_t *counts_host, int64_t *cand_host)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_match_guided";
    if (int rc = gd_check_opt(ctx, who, opt)) return rc;
    if (n_pairs < 0 || out_stride < 0 || (n_pairs > 0 && (!pairs_host || !F_host || !out_host || !counts_host))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    if (n_pairs == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    GdPlan pl;
    if (int rc = gd_plan(ctx, who, pairs_host, n_pairs, out_stride, pl)) return rc;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t P = (size_t)n_pairs, stride = (size_t)std::max<int64_t>(out_stride, 1);
    const size_t b_F = al(72 * P), b_out = al(4 * P * stride), b_cnt = al(4 * P), b_cand = al(8 * P);
    RCN_HIP(ctx->gd_hws.reserve(b_F + b_out + b_cnt + b_cand));
    char *base = ctx->gd_hws.as<char>();
    double *d_F = (double *)base;
    int32_t *d_out = (int32_t *)(base + b_F), *d_cnt = (int32_t *)(base + b_F + b_out);
    int64_t *d_cand = (int64_t *)(base + b_F + b_out + b_cnt);
    hipStream_t st = ctx->stream;
    RCN_HIP(hipMemcpyAsync(d_F, F_host, 72 * P, hipMemcpyHostToDevice, st));
    if (int rc = gd_run(ctx, pl, ctx->D, d_F, nullptr, gd_thr2(opt->max_error_px), opt->ratio, opt->max_distance, opt->cross_check, d_out, (int64_t)stride,
                        d_cnt, cand_host ? d_cand : nullptr, nullptr, nullptr, 0)) return rc;
    if (out_stride > 0) RCN_HIP(hipMemcpyAsync(out_host, d_out, 4 * P * (size_t)out_stride, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(counts_host, d_cnt, 4 * P, hipMemcpyDeviceToHost, st));
    if (cand_host) RCN_HIP(hipMemcpyAsync(cand_host, d_cand, 8 * P, hipMemcpyDeviceToHost, st));
    RCN_HIP(rcn_int_stream_wait(ctx));
    return RCN_OK;
}

int rcn_match_pair_guided(rcn_ctx *ctx, const float *q_host, int32_t K1, const int32_t *xy1_host, const float *t_host, int32_t K2,
                          const int32_t *xy2_host, int32_t D, const double *F, const rcn_guided_options *opt,
                          int32_t *out_train_for_query, int32_t *out_count)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_match_pair_guided";
    if (int rc = gd_check_opt(ctx, who, opt)) return rc;
    if (K1 < 0 || K2 < 0 || D <= 0 || !F || !out_count || (K1 > 0 && (!q_host || !xy1_host || !out_train_for_query)) || (K2 > 0 && (!t_host || !xy2_host))) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    *out_count = 0;
    if (K1 == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_q = al(4 * (size_t)K1 * D), b_t = al(4 * (size_t)std::max(K2, 1) * D), b_x1 = al(8 * (size_t)K1), b_x2 = al(8 * (size_t)std::max(K2, 1));
    RCN_HIP(ctx->gd_hws.reserve(b_q + b_t + b_x1 + b_x2 + 256 + al(4 * (size_t)K1) + 256));
    char *base = ctx->gd_hws.as<char>();
    float *d_q = (float *)base, *d_t = (float *)(base + b_q);
    int32_t *d_x1 = (int32_t *)(base + b_q + b_t), *d_x2 = (int32_t *)(base + b_q + b_t + b_x1);
    double *d_F = (double *)(base + b_q + b_t + b_x1 + b_x2);
    int32_t *d_out = (int32_t *)(base + b_q + b_t + b_x1 + b_x2 + 256), *d_cnt = (int32_t *)((char *)d_out + al(4 * (size_t)K1));
    hipStream_t st = ctx->stream;
    RCN_HIP(hipMemcpyAsync(d_q, q_host, 4 * (size_t)K1 * D, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(d_x1, xy1_host, 8 * (size_t)K1, hipMemcpyHostToDevice, st));
    if (K2 > 0) {
        RCN_HIP(hipMemcpyAsync(d_t, t_host, 4 * (size_t)K2 * D, hipMemcpyHostToDevice, st));
        RCN_HIP(hipMemcpyAsync(d_x2, xy2_host, 8 * (size_t)K2, hipMemcpyHostToDevice, st));
    }
    RCN_HIP(hipMemcpyAsync(d_F, F, 72, hipMemcpyHostToDevice, st));
    GdPlan pl;
    pl.pairs.resize(1);
    GdPair &g = pl.pairs[0];
    g.q = d_q; g.t = d_t; g.xyq = d_x1; g.xyt = d_x2; g.Kq = K1; g.Kt = K2; g.ws_off = 0;
    pl.kq_max = K1; pl.kt_max = K2;
    if (int rc = gd_run(ctx, pl, D, d_F, nullptr, gd_thr2(opt->max_error_px), opt->ratio, opt->max_distance, opt->cross_check, d_out, K1, d_cnt, nullptr,
                        nullptr, nullptr, 0)) return rc;
    RCN_HIP(hipMemcpyAsync(out_train_for_query, d_out, 4 * (size_t)K1, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(out_count, d_cnt, 4, hipMemcpyDeviceToHost, st));
    RCN_HIP(rcn_int_stream_wait(ctx));       // the host rows are borrowed for the call only
    return RCN_OK;
}

int rcn_guided_knn2_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, const double *F_dev, float max_error_px,
                           int32_t *idx_dev, double *d2_dev, int64_t stride)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_guided_knn2_device";
    if (int rc = gd_check_options(ctx, who, 1.f, max_error_px)) return rc;
    if (n_pairs < 0 || stride < 0 || (n_pairs > 0 && (!pairs_host || !F_dev || !idx_dev || !d2_dev))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    if (n_pairs == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    GdPlan pl;
    if (int rc = gd_plan(ctx, who, pairs_host, n_pairs, stride, pl)) return rc;
    return gd_run(ctx, pl, ctx->D, F_dev, nullptr, gd_thr2(max_error_px), 1.f, 0.f, 0, nullptr, 0, nullptr, nullptr, idx_dev, d2_dev, stride);
}

int rcn_match_grid_guided(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio, const rcn_guided_options *opt,
                          int32_t *out_host, int64_t out_stride, int32_t *counts_host, int32_t *status_host)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_match_grid_guided";
    if (int rc = gd_check_opt(ctx, who, opt)) return rc;
    if (n_pairs < 0 || out_stride < 1 || (n_pairs > 0 && (!pairs_host || !out_host || !counts_host))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    if (n_pairs == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    GdPlan pl;
    if (int rc = gd_plan(ctx, who, pairs_host, n_pairs, out_stride, pl)) return rc;      // before anything is launched
    const size_t P = (size_t)n_pairs;
    RCN_HIP(ctx->out_tmp.reserve(P * (size_t)out_stride * 4));
    RCN_HIP(ctx->cnt_tmp.reserve(2 * P * 4));       // counts, then the verdicts
    RCN_HIP(ctx->gd_F.reserve(72 * P));
    int32_t *tab = ctx->out_tmp.as<int32_t>(), *cnt = ctx->cnt_tmp.as<int32_t>(), *ver = cnt + n_pairs;
    ++ctx->own_table_gen;
    if (int rc = rcn_int_match_grid(ctx, pairs_host, n_pairs, ratio, tab, out_stride, cnt)) return rc;
    if (int rc = rcn_int_table_filter(ctx, pairs_host, n_pairs, tab, out_stride, cnt, ver, ctx->gd_F.as<double>())) return rc;
    if (int rc = gd_run(ctx, pl, ctx->D, ctx->gd_F.as<double>(), ver, gd_thr2(opt->max_error_px), opt->ratio, opt->max_distance, opt->cross_check, tab,
                        out_stride, cnt, nullptr, nullptr, nullptr, 0)) return rc;
    hipStream_t st = ctx->stream;
    RCN_HIP(hipMemcpyAsync(out_host, tab, P * (size_t)out_stride * 4, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(counts_host, cnt, P * 4, hipMemcpyDeviceToHost, st));
    if (status_host) RCN_HIP(hipMemcpyAsync(status_host, ver, P * 4, hipMemcpyDeviceToHost, st));
    RCN_HIP(rcn_int_stream_wait(ctx));
    return RCN_OK;
}

}  // extern "C"
