// retrieval.hip -- the ImageMatcher stage (ImageMatcher.h:14-33) by global descriptor: Lloyd's k-means on the call's own local
// descriptors, VLAD, dense similarities, top-k neighbours, the symmetric pair list rcn_match_grid takes.  DESIGN.md section 24;
// the definition is restated in tests/retr_ref.py and every stage here equals it bit for bit.
//
// All arithmetic is fp64 on fp32 inputs widened to double, and UNFUSED: a product is rounded, then added (numpy cannot fuse).
// Contraction is therefore off for this translation unit -- and for this one only; the build's flags stay as they are.
//
//   k_retr_assign         lane = centroid, centroid tile transposed in LDS, 64 rows per wavefront in groups of 8 accumulators,
//                         the rows' values fetched 64 at a time and handed round by readlane
//   k_retr_segment_sums   one workgroup per (image, slice of D, chunk of C): a lane owns a column and walks the rows upwards
//   k_retr_merge/_update  Lloyd: the per-image sums merged in ascending image order, then mu = float(sum / count)
//   k_retr_init           prefix over the images' training-row counts, then the C evenly spaced training rows
//   k_retr_encode         residual, signed root, two-level norm, division
//   k_retr_similarity     upper triangle in 16 x 16 tiles through LDS, mirrored
//   k_retr_topk           one workgroup per image, rank by counting
//   k_retr_pairs_*        neighbour table -> n x n mask -> per-row counts -> prefix -> ascending list
#include "rcn_internal.h"
#include "wgprim.h"
#include <algorithm>

#pragma clang fp contract(off)

struct rcn_retr_codebook {
    rcn_ctx *ctx;
    int32_t C, D;
    float *mu;        // [C][D] in HBM
};

namespace {

constexpr int kMaxImages = 8192, kMaxD = 256, kMaxL = 65536;
constexpr int kTileFloats = 16384;        // centroid tile of k_retr_assign: 64 KiB (+ one padding column)
constexpr int kRowsPerBlock = 256;        // k_retr_assign: 4 wavefronts x 64 rows
constexpr int kGroup = 8;                 // ... rows held as accumulators at a time
constexpr int kSegDoubles = 8192;         // k_retr_segment_sums: [CC][W] fp64 accumulators (64 KiB) + CC counts
constexpr size_t kChunkBytes = (size_t)1 << 30;   // workspace per chunk of images

__device__ __forceinline__ int clampi(int v, long long K) { return v < 0 ? 0 : (v > K ? (int)K : v); }

// Rows are addressed as slots: image i has spi = ceil(K / s) slots, slot j is row j * s (s = 1: every row).  A slot whose row is
// past counts[i] is skipped.  assign[i * K + row] receives the centroid.
struct AssignArgs {
    const float *x; const int32_t *counts; const float *mu; int32_t *assign;
    long long K, spi, total; int32_t D, s, C, TC;
};

__global__ __launch_bounds__(256) void k_retr_assign(AssignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float retr_tile[];     // [D][TC + 1]: transposed, lanes read consecutive words
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = a.D, TC = a.TC, TS = TC + 1;
    const long long wslot0 = (long long)blockIdx.x * kRowsPerBlock + wave * 64;
    double best_d = __builtin_inf();      // lane l: the running best of slot wslot0 + l
    int best_c = 0;
    for (int c0 = 0; c0 < a.C; c0 += TC) {
        const int tc = min(TC, a.C - c0);
        __syncthreads();
        for (int idx = threadIdx.x; idx < TC * D; idx += 256) {
            const int c = idx / D, k = idx - c * D;
            retr_tile[k * TS + c] = c < tc ? a.mu[(long long)(c0 + c) * D + k] : 0.f;
        }
        __syncthreads();
        for (int g = 0; g < 64; g += kGroup) {
            const float *xr[kGroup];
            bool any = false;
#pragma unroll
            for (int r = 0; r < kGroup; ++r) {
                const long long slot = wslot0 + g + r;
                xr[r] = a.x;
                if (slot < a.total) {
                    const long long img = slot / a.spi, row = (slot - img * a.spi) * a.s;
                    const int cnt = a.counts ? clampi(a.counts[img], a.K) : (int)a.K;
                    if (row < cnt) { xr[r] = a.x + (img * a.K + row) * D; any = true; }
                }
            }
            if (!any) continue;
            for (int cs = 0; cs < tc; cs += 64) {
                double acc[kGroup];
#pragma unroll
                for (int r = 0; r < kGroup; ++r) acc[r] = 0.0;
                const float *col = retr_tile + cs + lane;
                for (int k0 = 0; k0 < D; k0 += 64) {          // 64 values of each row, a lane each; then lane kk's value to everybody
                    int xv[kGroup];
#pragma unroll
                    for (int r = 0; r < kGroup; ++r) xv[r] = k0 + lane < D ? __float_as_int(xr[r][k0 + lane]) : 0;
#pragma unroll
                    for (int kk = 0; kk < 64; ++kk) {
                        if (k0 + kk >= D) break;
                        const double m = (double)col[(k0 + kk) * TS];
#pragma unroll
                        for (int r = 0; r < kGroup; ++r) {
                            const double d = (double)__int_as_float(__builtin_amdgcn_readlane(xv[r], kk)) - m;
                            acc[r] = acc[r] + d * d;
                        }
                    }
                }
                const int cg = c0 + cs + lane;
#pragma unroll
                for (int r = 0; r < kGroup; ++r) {
                    double d2 = cs + lane < tc ? acc[r] : __builtin_inf();
                    int c = cg;
                    for (int off = 32; off; off >>= 1) {          // lexicographic minimum of (d2, c)
                        const double od = __shfl_xor(d2, off);
                        const int oc = __shfl_xor(c, off);
                        if (od < d2 || (od == d2 && oc < c)) { d2 = od; c = oc; }
                    }
                    if (lane == g + r && d2 < best_d) { best_d = d2; best_c = c; }    // strict: the lowest index wins across tiles too
                }
            }
        }
    }
    const long long slot = wslot0 + lane;
    if (slot < a.total) {
        const long long img = slot / a.spi, row = (slot - img * a.spi) * a.s;
        const int cnt = a.counts ? clampi(a.counts[img], a.K) : (int)a.K;
        if (row < cnt) a.assign[img * a.K + row] = best_c;
    }
}

struct SegArgs {
    const float *x; const int32_t *counts; const int32_t *assign; double *S; int32_t *cnt;
    long long K; int32_t D, s, C, W, CC;
};

// grid (slices of D, images, chunks of C), W threads: S[i][c][d] = sum of the rows of image i assigned to c, ascending; cnt[i][c] their number
__global__ __launch_bounds__(256) void k_retr_segment_sums(SegArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double retr_acc[];    // [CC][W] doubles, then CC counts
    int *lcnt = reinterpret_cast<int *>(retr_acc + (size_t)a.CC * a.W);
    const int t = threadIdx.x, W = a.W, d = blockIdx.x * W + t, c0 = blockIdx.z * a.CC, cc = min(a.CC, a.C - c0);
    const long long i = blockIdx.y;
    for (int idx = t; idx < cc * W; idx += W) retr_acc[idx] = 0.0;
    for (int idx = t; idx < cc; idx += W) lcnt[idx] = 0;
    __syncthreads();
    const int rows = a.counts ? clampi(a.counts[i], a.K) : (int)a.K;
    const bool counting = t == 0 && blockIdx.x == 0, live = d < a.D;
    const int32_t *as = a.assign + i * a.K;
    const float *x = a.x + i * a.K * a.D + d;
#pragma unroll 4
    for (long long r = 0; r < rows; r += a.s) {
        const unsigned c = (unsigned)(as[r] - c0);
        if (c < (unsigned)cc) {
            if (live) retr_acc[c * W + t] = retr_acc[c * W + t] + (double)x[r * a.D];
            if (counting) ++lcnt[c];
        }
    }
    __syncthreads();
    if (live)
        for (int c = 0; c < cc; ++c) a.S[(i * a.C + c0 + c) * a.D + d] = retr_acc[c * W + t];
    if (blockIdx.x == 0)
        for (int c = t; c < cc; c += W) a.cnt[i * a.C + c0 + c] = lcnt[c];
}

// Lloyd: acc[c][d] += S[i][c][d] for the m images of a chunk in ascending order (the chain carries on from chunk to chunk), tot[c] += cnt[i][c]
__global__ __launch_bounds__(256) void k_retr_merge(const double *S, const int32_t *cnt, int32_t m, int32_t C, int32_t D, double *acc, long long *tot)
{
    const long long L = (long long)C * D, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= L) return;
    double s = acc[idx];
    for (int i = 0; i < m; ++i) s = s + S[i * L + idx];
    acc[idx] = s;
    if (idx < C) {
        long long t = tot[idx];
        for (int i = 0; i < m; ++i) t += cnt[(long long)i * C + idx];
        tot[idx] = t;
    }
}

__global__ __launch_bounds__(256) void k_retr_update(const double *acc, const long long *tot, int32_t C, int32_t D, float *mu)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)C * D) return;
    const long long t = tot[idx / D];
    if (t > 0) mu[idx] = (float)(acc[idx] / (double)t);       // an empty cluster keeps its centroid
}

// one workgroup: prefix[i] = training rows of the images before i, *M_out their total; M >= C: mu_c = training row floor(c M / C)
__global__ __launch_bounds__(256) void k_retr_init(const float *x, const int32_t *counts, int32_t n, long long K, int32_t D, int32_t s, int32_t C,
                                                   long long *prefix, long long *M_out, float *mu)
{
    if (threadIdx.x == 0) {
        long long p = 0;
        for (int i = 0; i < n; ++i) {
            prefix[i] = p;
            const int cnt = counts ? clampi(counts[i], K) : (int)K;
            p += (cnt + s - 1) / s;
        }
        prefix[n] = p;
        *M_out = p;
    }
    __syncthreads();
    const long long M = prefix[n];
    if (M < C) return;
    for (int idx = threadIdx.x; idx < C * D; idx += 256) {
        const int c = idx / D, k = idx - c * D;
        const long long g = (long long)c * M / C;
        int lo = 0, hi = n;                                   // the last image with prefix <= g (it has a training row: prefix[lo + 1] > g)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= g) lo = mid; else hi = mid;
        }
        mu[idx] = x[((long long)lo * K + (g - prefix[lo]) * s) * D + k];
    }
}

// one workgroup per image; S holds the segment sums and receives the signed roots; b: C doubles per image
__global__ __launch_bounds__(256) void k_retr_encode(double *S, const int32_t *cnt, const float *mu, int32_t C, int32_t D, double *b, float *G)
{
    __shared__ double nrm_s;
    const long long L = (long long)C * D, i = blockIdx.x;
    double *V = S + i * L;
    for (long long idx = threadIdx.x; idx < L; idx += 256) {
        const double v = V[idx] - (double)cnt[i * C + idx / D] * (double)mu[idx];
        V[idx] = copysign(__dsqrt_rn(fabs(v)), v);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double acc = 0.0;
        for (int d = 0; d < D; ++d) { const double v = V[(long long)c * D + d]; acc = acc + v * v; }
        b[i * C + c] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int c = 0; c < C; ++c) tot = tot + b[i * C + c];
        nrm_s = __dsqrt_rn(tot);
    }
    __syncthreads();
    const double nrm = nrm_s;
    for (long long idx = threadIdx.x; idx < L; idx += 256) G[i * L + idx] = nrm == 0.0 ? 0.f : (float)(V[idx] / nrm);
}

// grid (T, T), T = ceil(n / 16); tiles below the diagonal leave at once.  The product of two floats is exact in double and
// commutes, so the mirrored entry has the same bits.
__global__ __launch_bounds__(256) void k_retr_similarity(const float *G, int32_t n, int32_t C, int32_t D, double *sim)
{
    if (blockIdx.y < blockIdx.x) return;
    extern __shared__ __attribute__((aligned(16))) float retr_g[];       // two tiles [16][D + 1]
    const int DS = D + 1, ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    float *gi = retr_g, *gj = retr_g + 16 * DS;
    const long long L = (long long)C * D, i0 = (long long)blockIdx.x * 16, j0 = (long long)blockIdx.y * 16;
    double total = 0.0;
    for (int c = 0; c < C; ++c) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < 16 * D; idx += 256) {
            const int r = idx / D, d = idx - r * D;
            gi[r * DS + d] = i0 + r < n ? G[(i0 + r) * L + (long long)c * D + d] : 0.f;
            gj[r * DS + d] = j0 + r < n ? G[(j0 + r) * L + (long long)c * D + d] : 0.f;
        }
        __syncthreads();
        double acc = 0.0;
        const float *pi = gi + ti * DS, *pj = gj + tj * DS;
        for (int d = 0; d < D; ++d) acc = acc + (double)pi[d] * (double)pj[d];
        total = total + acc;
    }
    const long long i = i0 + ti, j = j0 + tj;
    if (i < n && j < n) {
        sim[i * n + j] = total;
        if (blockIdx.x != blockIdx.y) sim[j * n + i] = total;
    }
}

// one workgroup per image: j != i ordered by (sim descending, j ascending); the first kk into nbr[i][.]
__global__ __launch_bounds__(256) void k_retr_topk(const double *sim, int32_t n, int32_t kk, int32_t *nbr)
{
    extern __shared__ __attribute__((aligned(16))) double retr_row[];
    const int i = blockIdx.x;
    for (int j = threadIdx.x; j < n; j += 256) retr_row[j] = sim[(long long)i * n + j];
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += 256) {
        if (j == i) continue;
        const double v = retr_row[j];
        int rank = 0;
        for (int o = 0; o < n; ++o) {
            const double w = retr_row[o];
            rank += (o != i) & ((w > v) | ((w == v) & (o < j)));
        }
        if (rank < kk) nbr[(long long)i * kk + rank] = j;
    }
}

__global__ __launch_bounds__(256) void k_retr_pairs_mark(const int32_t *nbr, int32_t n, int32_t kk, uint8_t *mask)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * kk) return;
    const int i = (int)(idx / kk), j = nbr[idx];
    if (j < 0 || j >= n || j == i) return;                    // a table that is not one of k_retr_topk's marks nothing outside the mask
    mask[(long long)min(i, j) * n + max(i, j)] = 1;
}

// one wavefront per row a of the mask.  FILL = false: rowcnt[a]; FILL = true: the pairs (a, b), b ascending, from rowoff[a] on
template <bool FILL>
__global__ __launch_bounds__(64) void k_retr_pairs_rows(const uint8_t *mask, int32_t n, int32_t *rowcnt, const long long *rowoff, int32_t first_img_id,
                                                        int32_t *pairs, long long capacity)
{
    const int a = blockIdx.x, lane = threadIdx.x;
    long long base = FILL ? rowoff[a] : 0;
    for (int b0 = a + 1; b0 < n; b0 += 64) {
        const int b = b0 + lane;
        const bool on = b < n && mask[(long long)a * n + b];
        const unsigned long long m = __ballot(on);
        if (FILL && on) {
            const long long pos = base + __popcll(m & ((1ull << lane) - 1));
            if (pos < capacity) { pairs[2 * pos] = first_img_id + a; pairs[2 * pos + 1] = first_img_id + b; }
        }
        base += __popcll(m);
    }
    if (!FILL && lane == 0) rowcnt[a] = (int32_t)base;
}

__global__ __launch_bounds__(1024) void k_retr_pairs_scan(const int32_t *rowcnt, int32_t n, long long *rowoff, int32_t *n_pairs)
{
    const long long p = wg_scan_array(rowcnt, n, rowoff, 0ll);
    if (threadIdx.x == 0) *n_pairs = (int32_t)p;              // at most n (n - 1) / 2 < 2^25
}

// ---------------------------------------------------------------------------------------------------------------- host side

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

int retr_fail(rcn_ctx *ctx, const char *who, const char *why, int code = RCN_ERR_ARG)
{
    ctx->set_error(std::string(who) + (code == RCN_ERR_ARG ? ": bad argument (" : ": unsupported (") + why + ")");
    return code;
}

int retr_setup(rcn_ctx *ctx)
{
    static std::mutex once_mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> lk(once_mu);
    if (std::find(done.begin(), done.end(), ctx->device) == done.end()) {
        RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_retr_assign), hipFuncAttributeMaxDynamicSharedMemorySize, (kTileFloats + kMaxD) * 4));
        RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_retr_segment_sums), hipFuncAttributeMaxDynamicSharedMemorySize, kSegDoubles * 12));
        RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_retr_topk), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxImages * 8));
        done.push_back(ctx->device);
    }
    return RCN_OK;
}

// the shape checks every entry point with an image block shares (NULL: fine)
const char *retr_shape(int32_t n, int32_t K, int32_t D, bool null_ptr)
{
    if (n < 0) return "n < 0";
    if (K < 0) return "K < 0";
    if (D < 1 || D > kMaxD) return "D outside 1..256";
    if (n > 0 && null_ptr) return "null pointer";
    return nullptr;
}

int retr_assign_launch(rcn_ctx *ctx, const float *mu, int32_t C, const float *x, const int32_t *counts, int64_t n, int64_t K, int32_t D, int32_t s, int32_t *assign)
{
    AssignArgs a;
    a.x = x; a.counts = counts; a.mu = mu; a.assign = assign;
    a.K = K; a.spi = (K + s - 1) / s; a.total = n * a.spi; a.D = D; a.s = s; a.C = C;
    a.TC = std::min((C + 63) / 64 * 64, kTileFloats / D / 64 * 64);
    if (a.total == 0) return RCN_OK;
    const int64_t blocks = (a.total + kRowsPerBlock - 1) / kRowsPerBlock;
    k_retr_assign<<<dim3((unsigned)blocks), 256, (size_t)(a.TC + 1) * D * 4, ctx->stream>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int retr_segsum_launch(rcn_ctx *ctx, int32_t C, const float *x, const int32_t *counts, const int32_t *assign, int32_t m, int32_t K, int32_t D, int32_t s,
                       double *S, int32_t *cnt)
{
    SegArgs a;
    a.x = x; a.counts = counts; a.assign = assign; a.S = S; a.cnt = cnt; a.K = K; a.D = D; a.s = s; a.C = C;
    a.W = std::max(1, std::min({D, 256, kSegDoubles / C}));
    a.CC = std::min(C, kSegDoubles / a.W);
    const dim3 grid((unsigned)((D + a.W - 1) / a.W), (unsigned)m, (unsigned)((C + a.CC - 1) / a.CC));
    k_retr_segment_sums<<<grid, a.W, (size_t)a.CC * a.W * 8 + (size_t)a.CC * 4, ctx->stream>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

// workspace of one chunk of nb images
struct RetrWs { int32_t *assign; double *S; int32_t *cnt; double *b; double *acc; long long *tot, *prefix, *M; int32_t nb; };
int retr_ws(rcn_ctx *ctx, int32_t n, int32_t K, int32_t C, int32_t D, RetrWs *w)
{
    const size_t L = (size_t)C * D, per = al((size_t)K * 4) + al(L * 8) + 2 * al((size_t)C * 8);
    const int32_t nb = (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)n, kChunkBytes / per));
    const size_t fixed = al(L * 8) + al((size_t)C * 8) + al(((size_t)n + 1) * 8) + 256;
    RCN_HIP(ctx->retr_ws.reserve((size_t)nb * ((size_t)K * 4 + L * 8 + (size_t)C * 12) + 1024 + fixed));
    char *p = ctx->retr_ws.as<char>();
    w->nb = nb;
    w->assign = reinterpret_cast<int32_t *>(p); p += al((size_t)nb * K * 4);
    w->S = reinterpret_cast<double *>(p);       p += al((size_t)nb * L * 8);
    w->cnt = reinterpret_cast<int32_t *>(p);    p += al((size_t)nb * C * 4);
    w->b = reinterpret_cast<double *>(p);       p += al((size_t)nb * C * 8);
    w->acc = reinterpret_cast<double *>(p);     p += al(L * 8);
    w->tot = reinterpret_cast<long long *>(p);  p += al((size_t)C * 8);
    w->prefix = reinterpret_cast<long long *>(p); p += al(((size_t)n + 1) * 8);
    w->M = reinterpret_cast<long long *>(p);
    return RCN_OK;
}

const char *retr_cb_check(const rcn_ctx *ctx, const rcn_retr_codebook *cb, int32_t D)
{
    if (!cb) return "null codebook";
    if (cb->ctx != ctx) return "a codebook of another ctx";
    if (D > 0 && cb->D != D) return "the codebook has another D";
    return nullptr;
}

int retr_encode(rcn_ctx *ctx, const rcn_retr_codebook *cb, const float *desc, const int32_t *counts, int32_t n, int32_t K, int32_t D, float *G)
{
    if (n == 0) return RCN_OK;
    const int32_t C = cb->C;
    const int64_t L = (int64_t)C * D;
    RetrWs w;
    if (int rc = retr_ws(ctx, n, K, C, D, &w)) return rc;
    for (int32_t first = 0; first < n; first += w.nb) {
        const int32_t m = std::min(w.nb, n - first);
        const float *x = desc + (int64_t)first * K * D;
        const int32_t *cn = counts ? counts + first : nullptr;
        if (K > 0) {
            if (int rc = retr_assign_launch(ctx, cb->mu, C, x, cn, m, K, D, 1, w.assign)) return rc;
        }
        if (int rc = retr_segsum_launch(ctx, C, x, cn, w.assign, m, K, D, 1, w.S, w.cnt)) return rc;
        k_retr_encode<<<(unsigned)m, 256, 0, ctx->stream>>>(w.S, w.cnt, cb->mu, C, D, w.b, G + (int64_t)first * L);
        RCN_HIP(hipGetLastError());
    }
    return RCN_OK;
}

int retr_similarity(rcn_ctx *ctx, const float *G, int32_t n, int32_t C, int32_t D, double *sim)
{
    if (n == 0) return RCN_OK;
    const unsigned T = (unsigned)((n + 15) / 16);
    k_retr_similarity<<<dim3(T, T), 256, (size_t)32 * (D + 1) * 4, ctx->stream>>>(G, n, C, D, sim);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int retr_topk(rcn_ctx *ctx, const double *sim, int32_t n, int32_t kk, int32_t *nbr)
{
    if (n == 0 || kk == 0) return RCN_OK;
    k_retr_topk<<<(unsigned)n, 256, (size_t)n * 8, ctx->stream>>>(sim, n, kk, nbr);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

// the list into pairs_dev (at most `capacity` pairs are stored), its length into n_pairs_dev; asynchronous
int retr_pairs(rcn_ctx *ctx, const int32_t *nbr, int32_t n, int32_t kk, int32_t first_img_id, int32_t *pairs, int64_t capacity, int32_t *n_pairs)
{
    if (n == 0 || kk == 0) {
        RCN_HIP(hipMemsetAsync(n_pairs, 0, 4, ctx->stream));
        return RCN_OK;
    }
    const size_t nn = (size_t)n * n;
    RCN_HIP(ctx->retr_ws.reserve(al(nn) + al((size_t)n * 4) + al((size_t)n * 8)));
    uint8_t *mask = ctx->retr_ws.as<uint8_t>();
    int32_t *rowcnt = reinterpret_cast<int32_t *>(mask + al(nn));
    long long *rowoff = reinterpret_cast<long long *>(mask + al(nn) + al((size_t)n * 4));
    RCN_HIP(hipMemsetAsync(mask, 0, nn, ctx->stream));
    k_retr_pairs_mark<<<(unsigned)(((int64_t)n * kk + 255) / 256), 256, 0, ctx->stream>>>(nbr, n, kk, mask);
    k_retr_pairs_rows<false><<<(unsigned)n, 64, 0, ctx->stream>>>(mask, n, rowcnt, nullptr, first_img_id, nullptr, 0);
    k_retr_pairs_scan<<<1, 1024, 0, ctx->stream>>>(rowcnt, n, rowoff, n_pairs);
    k_retr_pairs_rows<true><<<(unsigned)n, 64, 0, ctx->stream>>>(mask, n, nullptr, rowoff, first_img_id, pairs, capacity);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

void retr_defaults(rcn_retr_options *o)
{
    std::memset(o, 0, sizeof *o);
    o->n_centroids = 64; o->iterations = 10; o->train_row_stride = 0; o->top_k = 20;
}

int retr_new_codebook(rcn_ctx *ctx, int32_t C, int32_t D, rcn_retr_codebook **out)
{
    rcn_retr_codebook *cb = new rcn_retr_codebook{ctx, C, D, nullptr};
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&cb->mu), (size_t)C * D * 4);
    if (e != hipSuccess) {
        delete cb;
        ctx->set_error(std::string("hipMalloc of the codebook: ") + hipGetErrorString(e));
        return RCN_ERR_HIP;
    }
    *out = cb;
    return RCN_OK;
}

}  // namespace

extern "C" void rcn_retr_default_options(rcn_retr_options *o)
{
    if (o) retr_defaults(o);
}

extern "C" int rcn_retr_codebook_train_device(rcn_ctx *ctx, const float *desc_dev, const int32_t *counts_dev, int32_t n, int32_t K, int32_t D,
                                              const rcn_retr_options *opt, rcn_retr_codebook **out)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_retr_codebook_train_device";
    rcn_retr_options o;
    if (opt) o = *opt; else retr_defaults(&o);
    if (!out) return retr_fail(ctx, who, "null pointer");
    *out = nullptr;
    if (const char *why = retr_shape(n, K, D, !desc_dev)) return retr_fail(ctx, who, why);
    if (o.n_centroids < 1 || o.iterations < 0 || o.train_row_stride < 0) return retr_fail(ctx, who, "n_centroids < 1, iterations < 0 or train_row_stride < 0");
    if ((int64_t)o.n_centroids * D > kMaxL) return retr_fail(ctx, who, "n_centroids * D above 65536", RCN_ERR_UNSUPPORTED);
    if (n > kMaxImages) return retr_fail(ctx, who, "more than 8192 images", RCN_ERR_UNSUPPORTED);
    const int32_t C = o.n_centroids;
    int32_t s = o.train_row_stride;
    if (s == 0)
        for (s = 1; (int64_t)n * ((K + s - 1) / s) > (1ll << 18); ++s) {}
    if (n == 0 || K == 0) return retr_fail(ctx, who, "fewer training rows than centroids");
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = retr_setup(ctx)) return rc;
    RetrWs w;
    if (int rc = retr_ws(ctx, n, K, C, D, &w)) return rc;
    rcn_retr_codebook *cb = nullptr;
    if (int rc = retr_new_codebook(ctx, C, D, &cb)) return rc;
    auto drop = [&](int rc) { (void)hipFree(cb->mu); delete cb; return rc; };
    k_retr_init<<<1, 256, 0, ctx->stream>>>(desc_dev, counts_dev, n, K, D, s, C, w.prefix, w.M, cb->mu);
    long long M = 0;
    hipError_t e = hipMemcpyAsync(&M, w.M, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = rcn_int_stream_wait(ctx);       // the one count that must reach the host
    if (e != hipSuccess) {
        ctx->set_error(std::string(who) + ": " + hipGetErrorString(e));
        return drop(RCN_ERR_HIP);
    }
    if (M < C) return drop(retr_fail(ctx, who, "fewer training rows than centroids"));
    const int64_t L = (int64_t)C * D;
    for (int it = 0; it < o.iterations; ++it) {
        e = hipMemsetAsync(w.acc, 0, (size_t)L * 8, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(w.tot, 0, (size_t)C * 8, ctx->stream);
        for (int32_t first = 0; first < n && e == hipSuccess; first += w.nb) {
            const int32_t m = std::min(w.nb, n - first);
            const float *x = desc_dev + (int64_t)first * K * D;
            const int32_t *cn = counts_dev ? counts_dev + first : nullptr;
            int rc = retr_assign_launch(ctx, cb->mu, C, x, cn, m, K, D, s, w.assign);
            if (!rc) rc = retr_segsum_launch(ctx, C, x, cn, w.assign, m, K, D, s, w.S, w.cnt);
            if (rc) return drop(rc);
            k_retr_merge<<<(unsigned)((L + 255) / 256), 256, 0, ctx->stream>>>(w.S, w.cnt, m, C, D, w.acc, w.tot);
        }
        k_retr_update<<<(unsigned)((L + 255) / 256), 256, 0, ctx->stream>>>(w.acc, w.tot, C, D, cb->mu);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->set_error(std::string(who) + ": " + hipGetErrorString(e));
            return drop(RCN_ERR_HIP);
        }
    }
    *out = cb;
    return RCN_OK;
}

extern "C" int rcn_retr_codebook_create(rcn_ctx *ctx, const float *centroids_host, int32_t C, int32_t D, rcn_retr_codebook **out)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_retr_codebook_create";
    if (!out || !centroids_host) return retr_fail(ctx, who, "null pointer");
    *out = nullptr;
    if (C < 1 || D < 1 || D > kMaxD) return retr_fail(ctx, who, "C < 1 or D outside 1..256");
    if ((int64_t)C * D > kMaxL) return retr_fail(ctx, who, "C * D above 65536", RCN_ERR_UNSUPPORTED);
    RCN_HIP(hipSetDevice(ctx->device));
    rcn_retr_codebook *cb = nullptr;
    if (int rc = retr_new_codebook(ctx, C, D, &cb)) return rc;
    const hipError_t e = hipMemcpy(cb->mu, centroids_host, (size_t)C * D * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ctx->set_error(std::string(who) + ": " + hipGetErrorString(e));
        (void)hipFree(cb->mu);
        delete cb;
        return RCN_ERR_HIP;
    }
    *out = cb;
    return RCN_OK;
}

extern "C" int rcn_retr_codebook_read(const rcn_retr_codebook *cb, float *centroids_host, int32_t *C, int32_t *D)
{
    if (!cb) return RCN_ERR_ARG;
    rcn_ctx *ctx = cb->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (C) *C = cb->C;
    if (D) *D = cb->D;
    if (!centroids_host) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(hipMemcpyAsync(centroids_host, cb->mu, (size_t)cb->C * cb->D * 4, hipMemcpyDeviceToHost, ctx->stream));
    RCN_HIP(rcn_int_stream_wait(ctx));
    return RCN_OK;
}

extern "C" void rcn_retr_codebook_destroy(rcn_retr_codebook *cb)
{
    if (!cb) return;
    {
        std::lock_guard<std::mutex> lk(cb->ctx->mu);
        (void)hipSetDevice(cb->ctx->device);
        (void)hipStreamSynchronize(cb->ctx->stream);
        (void)hipFree(cb->mu);
    }
    delete cb;
}

extern "C" int rcn_retr_assign_device(rcn_ctx *ctx, const rcn_retr_codebook *cb, const float *rows_dev, int64_t n_rows, int32_t *assign_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_retr_assign_device";
    if (const char *why = retr_cb_check(ctx, cb, 0)) return retr_fail(ctx, who, why);
    if (n_rows < 0) return retr_fail(ctx, who, "n_rows < 0");
    if (n_rows > 0 && (!rows_dev || !assign_dev)) return retr_fail(ctx, who, "null pointer");
    if (n_rows > (1ll << 31) - 1) return retr_fail(ctx, who, "more than 2^31 - 1 rows", RCN_ERR_UNSUPPORTED);
    if (n_rows == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = retr_setup(ctx)) return rc;
    return retr_assign_launch(ctx, cb->mu, cb->C, rows_dev, nullptr, 1, n_rows, cb->D, 1, assign_dev);
}

extern "C" int rcn_retr_encode_device(rcn_ctx *ctx, const rcn_retr_codebook *cb, const float *desc_dev, const int32_t *counts_dev, int32_t n, int32_t K,
                                      int32_t D, float *global_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_retr_encode_device";
    if (const char *why = retr_shape(n, K, D, !global_dev || (K > 0 && !desc_dev))) return retr_fail(ctx, who, why);
    if (const char *why = retr_cb_check(ctx, cb, D)) return retr_fail(ctx, who, why);
    if (n > kMaxImages) return retr_fail(ctx, who, "more than 8192 images", RCN_ERR_UNSUPPORTED);
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = retr_setup(ctx)) return rc;
    return retr_encode(ctx, cb, desc_dev, counts_dev, n, K, D, global_dev);
}

extern "C" int rcn_retr_similarity_device(rcn_ctx *ctx, const float *global_dev, int32_t n, int32_t L, int32_t D, double *sim_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_retr_similarity_device";
    if (n < 0 || D < 1 || D > kMaxD || L < 1 || L % D) return retr_fail(ctx, who, "n < 0, D outside 1..256 or L no positive multiple of D");
    if (n > 0 && (!global_dev || !sim_dev)) return retr_fail(ctx, who, "null pointer");
    if (n > kMaxImages) return retr_fail(ctx, who, "more than 8192 images", RCN_ERR_UNSUPPORTED);
    if (L > kMaxL) return retr_fail(ctx, who, "L above 65536", RCN_ERR_UNSUPPORTED);
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    return retr_similarity(ctx, global_dev, n, L / D, D, sim_dev);
}

extern "C" int rcn_retr_topk_device(rcn_ctx *ctx, const double *sim_dev, int32_t n, int32_t k, int32_t *nbr_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_retr_topk_device";
    if (n < 0 || k < 1) return retr_fail(ctx, who, "n < 0 or k < 1");
    if (n > 1 && (!sim_dev || !nbr_dev)) return retr_fail(ctx, who, "null pointer");
    if (n > kMaxImages) return retr_fail(ctx, who, "more than 8192 images", RCN_ERR_UNSUPPORTED);
    if (n < 2) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = retr_setup(ctx)) return rc;
    return retr_topk(ctx, sim_dev, n, std::min(k, n - 1), nbr_dev);
}

extern "C" int rcn_retr_pairs_device(rcn_ctx *ctx, const int32_t *nbr_dev, int32_t n, int32_t k, int32_t first_img_id, int32_t *pairs_dev, int64_t capacity,
                                     int32_t *n_pairs_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_retr_pairs_device";
    if (n < 0 || k < 1 || capacity < 0) return retr_fail(ctx, who, "n < 0, k < 1 or capacity < 0");
    if (!n_pairs_dev || (n > 1 && !nbr_dev) || (capacity > 0 && !pairs_dev)) return retr_fail(ctx, who, "null pointer");
    if (n > kMaxImages) return retr_fail(ctx, who, "more than 8192 images", RCN_ERR_UNSUPPORTED);
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = retr_pairs(ctx, nbr_dev, n, n < 2 ? 0 : std::min(k, n - 1), first_img_id, pairs_dev, capacity, n_pairs_dev)) return rc;
    int32_t total = 0;
    RCN_HIP(hipMemcpyAsync(&total, n_pairs_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    RCN_HIP(rcn_int_stream_wait(ctx));
    if (total > capacity) return retr_fail(ctx, who, ("capacity below the " + std::to_string(total) + " pairs of the list").c_str());
    return RCN_OK;
}

extern "C" int rcn_retr_image_pairs(rcn_ctx *ctx, const rcn_retr_codebook *cb, const float *desc_dev, const int32_t *counts_dev, int32_t n, int32_t K,
                                    int32_t D, int32_t first_img_id, int32_t top_k, int32_t *pairs_host, int64_t capacity, int32_t *n_pairs_out)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_retr_image_pairs";
    if (const char *why = retr_shape(n, K, D, K > 0 && !desc_dev)) return retr_fail(ctx, who, why);
    if (const char *why = retr_cb_check(ctx, cb, D)) return retr_fail(ctx, who, why);
    if (top_k < 1 || capacity < 0) return retr_fail(ctx, who, "top_k < 1 or capacity < 0");
    if (!n_pairs_out || (capacity > 0 && !pairs_host)) return retr_fail(ctx, who, "null pointer");
    if (n > kMaxImages) return retr_fail(ctx, who, "more than 8192 images", RCN_ERR_UNSUPPORTED);
    *n_pairs_out = 0;
    if (n < 2) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = retr_setup(ctx)) return rc;
    const int32_t kk = std::min(top_k, n - 1), C = cb->C;
    const size_t L = (size_t)C * D, nn = (size_t)n * n, maxp = std::min<size_t>((size_t)n * kk, nn / 2);
    RCN_HIP(ctx->retr_out.reserve(al(nn * 8) + al((size_t)n * L * 4) + al((size_t)n * kk * 4) + al(maxp * 8) + 256));
    char *p = ctx->retr_out.as<char>();
    double *sim = reinterpret_cast<double *>(p);   p += al(nn * 8);
    float *G = reinterpret_cast<float *>(p);       p += al((size_t)n * L * 4);
    int32_t *nbr = reinterpret_cast<int32_t *>(p); p += al((size_t)n * kk * 4);
    int32_t *pairs = reinterpret_cast<int32_t *>(p); p += al(maxp * 8);
    int32_t *count = reinterpret_cast<int32_t *>(p);
    if (int rc = retr_encode(ctx, cb, desc_dev, counts_dev, n, K, D, G)) return rc;
    if (int rc = retr_similarity(ctx, G, n, C, D, sim)) return rc;
    if (int rc = retr_topk(ctx, sim, n, kk, nbr)) return rc;
    if (int rc = retr_pairs(ctx, nbr, n, kk, first_img_id, pairs, (int64_t)maxp, count)) return rc;
    int32_t total = 0;
    RCN_HIP(hipMemcpyAsync(&total, count, 4, hipMemcpyDeviceToHost, ctx->stream));
    RCN_HIP(rcn_int_stream_wait(ctx));
    *n_pairs_out = total;
    if (total > capacity) return retr_fail(ctx, who, ("capacity below the " + std::to_string(total) + " pairs of the list").c_str());
    if (total > 0) RCN_HIP(hipMemcpy(pairs_host, pairs, (size_t)total * 8, hipMemcpyDeviceToHost));
    return RCN_OK;
}
