// keypoints.hip -- the keypoint half of FeatureSuperPoint::detect on the GPU: processKeypoints
// (FeatureSuperPoint.cpp:145-179) = extractHeatMap (:95-140), the threshold scan (:155-166), nmsFast (:15-70) and
// removeBorderKeypoints (:73-89), batched over the images of one call, on the ctx stream, nothing but the caller's own
// reads of counts[] visiting the host.
//
//   heat stage   k_kp_plane (reference mode: the serial S_r chain per channel plane) or k_kp_cell (softmax mode: maximum
//                and fp64 denominator per cell), then k_kp_heat: division, depth-to-space, threshold, candidate list (one atomic per workgroup).
//   exact stages k_kp_threshold (rcn_kp_nms_device only: candidates of a heat map the caller has) and k_kp_nms: one
//                workgroup per image -- fixed-point NMS over the candidate list, border filter, top-K by radix select
//                when more than K survive, raster-order emission by a prefix sum over the kept bitmap.
//
// Canonical order: confidence descending, raster index ascending; as a key (fp32 bits << 32) | (2^31 - 1 - raster),
// larger first.  The heat stage carries a tolerance (expf, the order of sums); everything behind it is exact.
#include "rcn_internal.h"
#include "wgprim.h"

#include <algorithm>

namespace {

#pragma clang fp contract(off)

constexpr int KP_BLOCK = 1024;                 // threads of the one workgroup an image's NMS runs in
constexpr size_t KP_LDS_STATUS = RCN_KP_LDS_STATUS_BYTES;   // dynamic LDS of k_kp_nms: the status map when it fits
constexpr unsigned KP_DEAD = 0xFFFFFFFFu;      // list entry: decided in an earlier round
constexpr unsigned KP_PEND = 0x80000000u;      // list entry: found suppressed in phase A of this round (raster < 2^31)

// ---- heat stage ---------------------------------------------------------------------------------------------------------

// Reference mode, one workgroup per (channel < 64, image): R_k = sum of row k of expf(plane) in fp64, ascending columns (one
// lane per row); then one lane runs the chain  S_r = sum_{k<r} R_k / S_k + sum_{k>=r} R_k + 1e-5  and writes (float)S_r.
__global__ __launch_bounds__(64) void k_kp_plane(const float *__restrict__ lg, long long si, long long sc, long long sy, long long sx,
                                                 int Hc, int Wc, double *__restrict__ R, double *__restrict__ suf, float *__restrict__ S)
{
    const int c = blockIdx.x, img = blockIdx.y;
    const float *p = lg + (long long)img * si + (long long)c * sc;
    const size_t o = ((size_t)img * 64 + c) * Hc;
    for (int r = threadIdx.x; r < Hc; r += 64) {
        double s = 0.0;
        for (int x = 0; x < Wc; ++x) s = __dadd_rn(s, (double)expf(p[(long long)r * sy + (long long)x * sx]));
        R[o + r] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int r = Hc - 1; r >= 0; --r) { t = __dadd_rn(t, R[o + r]); suf[o + r] = t; }
        double pre = 0.0;
        for (int r = 0; r < Hc; ++r) {
            const double s = __dadd_rn(__dadd_rn(pre, suf[o + r]), 1e-5);
            S[o + r] = (float)s;
            pre = __dadd_rn(pre, R[o + r] / s);
        }
    }
}

// Softmax mode, one lane per cell: the maximum over the 65 channels and the fp64 sum of exp(l - max), ascending channels.
// The difference of two floats is exact in fp64 and so is taken there: rounded to fp32 it would alone cost up to 2^-21
// relative at |l - max| >= 8, the whole tolerance of the stage.
__global__ __launch_bounds__(256) void k_kp_cell(const float *__restrict__ lg, long long si, long long sc, long long sy, long long sx,
                                                 int Hc, int Wc, double2 *__restrict__ cell)
{
    const int img = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Hc * Wc) return;
    const float *p = lg + (long long)img * si + (long long)(i / Wc) * sy + (long long)(i % Wc) * sx;
    float m = p[0];
    for (int c = 1; c < 65; ++c) m = fmaxf(m, p[(long long)c * sc]);
    double den = 0.0;
    for (int c = 0; c < 65; ++c) den = __dadd_rn(den, exp((double)p[(long long)c * sc] - (double)m));
    cell[(size_t)img * Hc * Wc + i] = make_double2((double)m, den);
}

// Candidates of one workgroup's tile -- KP_PIX pixels per lane, pixel `it` of a lane is first + it * 256 and bit `it` of
// mask says whether it is a candidate -- behind ONE atomic on the image's counter: a scan of the lanes' counts (shuffles
// inside a wavefront, LDS across the four), then every lane writes its own.  (One atomic per wavefront, all on the image's
// one word, made the two grid-wide kernels atomic-bound: 570 us for 25 VGA images.)  Every lane of the workgroup calls it.
constexpr int KP_PIX = 8;
__device__ __forceinline__ void kp_append(unsigned mask, unsigned first, unsigned *cnt, unsigned *list)
{
    __shared__ unsigned s_wave[4], s_base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned c = __popc(mask);
    unsigned incl = c;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_wave[w] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        s_base = total ? atomicAdd(cnt, total) : 0u;
    }
    __syncthreads();
    unsigned pos = s_base + incl - c;
    for (int i = 0; i < w; ++i) pos += s_wave[i];
    for (int it = 0; it < KP_PIX; ++it)
        if ((mask >> it) & 1u) list[pos++] = first + it * 256u;
}

// heat[8 yc + c / 8][8 xc + c % 8] = e / scale, one lane per pixel of the full-resolution map; candidate iff (double)heat >=
// thresh (false for a NaN); KP_PIX pixels per lane, a tile of KP_PIX * 256 consecutive pixels per workgroup.
// REF: expf(l) / (float)S_r of its plane row in fp32; else (float)(exp(l - max) / the cell's sum) in fp64.
template <bool REF>
__global__ __launch_bounds__(256) void k_kp_heat(const float *__restrict__ lg, long long si, long long sc, long long sy, long long sx,
                                                 int H, int W, const float *__restrict__ S, const double2 *__restrict__ cell, double thresh,
                                                 float *__restrict__ heat, unsigned *__restrict__ cnt, unsigned *__restrict__ list)
{
    const int img = blockIdx.y;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const unsigned first = blockIdx.x * (KP_PIX * 256u) + threadIdx.x;
    const int Hc = H >> 3, Wc = W >> 3;
    unsigned mask = 0;
    for (int it = 0; it < KP_PIX; ++it) {
        const unsigned q = first + it * 256u;
        if (q >= HW) break;
        const int y = q / W, x = q - (unsigned)y * W;
        const int c = (y & 7) * 8 + (x & 7), yc = y >> 3, xc = x >> 3;
        const float l = lg[(long long)img * si + (long long)c * sc + (long long)yc * sy + (long long)xc * sx];
        float h;
        if (REF) h = __fdiv_rn(expf(l), S[((size_t)img * 64 + c) * Hc + yc]);
        else {
            const double2 md = cell[((size_t)img * Hc + yc) * Wc + xc];
            h = (float)(exp((double)l - md.x) / md.y);
        }
        heat[(size_t)img * HW + q] = h;
        if ((double)h >= thresh) mask |= 1u << it;
    }
    kp_append(mask, first, cnt + img, list + (size_t)img * HW);
}

// ---- exact stages -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_kp_threshold(const float *__restrict__ heat, unsigned HW, double thresh,
                                                      unsigned *__restrict__ cnt, unsigned *__restrict__ list)
{
    const int img = blockIdx.y;
    const unsigned first = blockIdx.x * (KP_PIX * 256u) + threadIdx.x;
    unsigned mask = 0;
    for (int it = 0; it < KP_PIX; ++it) {
        const unsigned q = first + it * 256u;
        if (q < HW && (double)heat[(size_t)img * HW + q] >= thresh) mask |= 1u << it;
    }
    kp_append(mask, first, cnt + img, list + (size_t)img * HW);
}

struct KpNmsArgs {
    const float *heat;        // [nb][H W]
    unsigned *list;           // [nb][H W]   candidates (raster indices) of each image, any order; consumed
    const unsigned *cnt;      // [nb]
    unsigned *st_glob;        // [nb][words] status when it does not fit the LDS budget, else unused
    int H, W, r, border, K, use_lds;
    int32_t *xy;              // [nb][K][2]
    float *conf;              // [nb][K] or NULL
    int32_t *counts;          // [nb]
    int32_t *rounds;          // [nb] or NULL
};

// status words are read past the L1 (the global form is written by atomics of other wavefronts of the workgroup)
__device__ __forceinline__ unsigned kp_ld(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long kp_key(float conf, unsigned q)
{
    return ((unsigned long long)__float_as_uint(conf) << 32) | (unsigned long long)(0x7FFFFFFFu - q);
}
// pixels of a status word whose two bits say "kept" (10), as a mask on the even bits
__device__ __forceinline__ unsigned kp_kept(unsigned w) { return (w >> 1) & ~w & 0x55555555u; }

// One workgroup per image.  Status, two bits per pixel, 16 pixels per word: 00 no candidate / suppressed (a suppressed
// candidate kills nothing and blocks nobody: the same as none), 01 undecided, 10 kept; 11 only inside a round (kept, not yet
// published: read as undecided).  A round: phase A reads the status as the last round left it -- an undecided candidate
// with a kept larger-key neighbour in its window is marked in its list entry, one whose larger-key neighbours are all gone
// sets its second bit; phase B publishes both.  So the number of rounds is that of the synchronous iteration, whatever the
// order of the list and of the wavefronts.
__global__ __launch_bounds__(KP_BLOCK) void k_kp_nms(KpNmsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned kp_smem[];
    __shared__ int s_scan[KP_BLOCK / 64];
    __shared__ unsigned s_hist[256];
    __shared__ int s_any, s_remaining;
    __shared__ unsigned long long s_prefix;

    const int img = blockIdx.x, tid = threadIdx.x;
    const int H = a.H, W = a.W, r = a.r, K = a.K;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const int nw = (int)((HW + 15u) >> 4);
    const float *heat = a.heat + (size_t)img * HW;
    unsigned *list = a.list + (size_t)img * HW;
    unsigned *st = a.use_lds ? kp_smem : a.st_glob + (size_t)img * nw;
    const unsigned ncand = a.cnt[img];

    for (int w = tid; w < nw; w += KP_BLOCK) st[w] = 0u;
    __syncthreads();
    for (unsigned i = tid; i < ncand; i += KP_BLOCK) {
        const unsigned q = list[i];
        atomicOr(&st[q >> 4], 1u << ((q & 15u) * 2));
    }
    __syncthreads();

    unsigned rounds = 0;
    bool more = ncand > 0;
    while (more) {
        if (tid == 0) s_any = 0;
        for (unsigned i = tid; i < ncand; i += KP_BLOCK) {
            const unsigned q = list[i];
            if (q == KP_DEAD) continue;
            const int y = q / W, x = q - (unsigned)y * W;
            const unsigned bp = __float_as_uint(heat[q]);
            const int y0 = max(0, y - r), y1 = min(H - 1, y + r), x0 = max(0, x - r), x1 = min(W - 1, x + r);
            bool blocked = false, sup = false;
            const int len = x1 - x0 + 1;                                  // <= 17 pixels: at most two status words per window row
            for (int yy = y0; yy <= y1 && !sup; ++yy) {
                const unsigned n0 = (unsigned)yy * W + x0, wi = n0 >> 4, sh = (n0 & 15u) * 2;
                unsigned long long bits = kp_ld(&st[wi]);
                if (sh + 2 * len > 32) bits |= (unsigned long long)kp_ld(&st[wi + 1]) << 32;
                bits = (bits >> sh) & ((1ull << (2 * len)) - 1ull);
                unsigned long long occ = (bits | (bits >> 1)) & 0x5555555555555555ull;      // pixels whose status is not 00
                while (occ) {
                    const int j = __ffsll((long long)occ) - 1;
                    occ &= occ - 1;
                    const unsigned n = n0 + (j >> 1);
                    if (n == q) continue;
                    const unsigned bn = __float_as_uint(heat[n]);
                    if (bn > bp || (bn == bp && n < q)) {
                        if (((bits >> j) & 3ull) == 2ull) { sup = true; break; }
                        blocked = true;
                    }
                }
            }
            if (sup) list[i] = q | KP_PEND;
            else if (!blocked) atomicOr(&st[q >> 4], 2u << ((q & 15u) * 2));
        }
        __syncthreads();
        for (unsigned i = tid; i < ncand; i += KP_BLOCK) {
            const unsigned e = list[i];
            if (e == KP_DEAD) continue;
            const unsigned q = e & ~KP_PEND, sh = (q & 15u) * 2;
            if (e & KP_PEND) { atomicAnd(&st[q >> 4], ~(3u << sh)); list[i] = KP_DEAD; }
            else if (((kp_ld(&st[q >> 4]) >> sh) & 3u) == 3u) { atomicAnd(&st[q >> 4], ~(1u << sh)); list[i] = KP_DEAD; }
            else s_any = 1;
        }
        __syncthreads();
        ++rounds;
        more = s_any != 0 && rounds <= ncand;       // every round decides the largest undecided key at least
        __syncthreads();
    }

    // border filter (a border point has suppressed its neighbours by now) and the uncapped count; each lane owns a run of words
    const int per = (nw + KP_BLOCK - 1) / KP_BLOCK;
    const int w0 = min(nw, tid * per), w1 = min(nw, w0 + per);
    const int b = a.border;
    int mine = 0;
    for (int w = w0; w < w1; ++w) {
        unsigned k = kp_kept(kp_ld(&st[w])), keep = k;
        while (k) {
            const int j = __ffs((int)k) - 1;
            k &= k - 1;
            const unsigned q = (unsigned)w * 16u + (j >> 1);
            const int y = q / W, x = q - (unsigned)y * W;
            if (x < b || x >= W - b || y < b || y >= H - b) keep &= ~(1u << j);
        }
        st[w] = keep << 1;
        mine += __popc(keep);
    }
    int total;
    (void)wg_scan_incl<int, KP_BLOCK>(mine, s_scan, total);
    if (tid == 0) {
        a.counts[img] = total;
        if (a.rounds) a.rounds[img] = (int32_t)rounds;
    }

    if (total > K) {
        // the K-th largest key by a radix select, most significant byte first (keys are distinct: the raster is part of them)
        if (tid == 0) { s_prefix = 0ull; s_remaining = K; }
        for (int byte = 7; byte >= 0; --byte) {
            for (int i = tid; i < 256; i += KP_BLOCK) s_hist[i] = 0u;
            __syncthreads();
            const unsigned long long prefix = s_prefix;
            for (int w = w0; w < w1; ++w) {
                unsigned k = kp_kept(kp_ld(&st[w]));
                while (k) {
                    const int j = __ffs((int)k) - 1;
                    k &= k - 1;
                    const unsigned q = (unsigned)w * 16u + (j >> 1);
                    const unsigned long long key = kp_key(heat[q], q);
                    if (byte == 7 || (key >> (8 * (byte + 1))) == prefix) atomicAdd(&s_hist[(unsigned)(key >> (8 * byte)) & 255u], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {
                int rem = s_remaining, d = 255;
                for (; d > 0; --d) {
                    if ((int)s_hist[d] >= rem) break;
                    rem -= (int)s_hist[d];
                }
                s_remaining = rem;
                s_prefix = (prefix << 8) | (unsigned long long)d;
            }
            __syncthreads();
        }
        const unsigned long long kth = s_prefix;
        for (int w = w0; w < w1; ++w) {
            const unsigned k0 = kp_kept(kp_ld(&st[w]));
            unsigned k = k0, keep = k0;
            while (k) {
                const int j = __ffs((int)k) - 1;
                k &= k - 1;
                const unsigned q = (unsigned)w * 16u + (j >> 1);
                if (kp_key(heat[q], q) < kth) keep &= ~(1u << j);
            }
            if (keep != k0) st[w] = keep << 1;
        }
        __syncthreads();
    }

    // raster order: words ascend with the lane, pixels with the bit
    mine = 0;
    for (int w = w0; w < w1; ++w) mine += __popc(kp_kept(kp_ld(&st[w])));
    int kept;
    int pos = wg_scan_incl<int, KP_BLOCK>(mine, s_scan, kept) - mine;
    int32_t *xy = a.xy + (size_t)img * K * 2;
    float *conf = a.conf ? a.conf + (size_t)img * K : nullptr;
    for (int w = w0; w < w1; ++w) {
        unsigned k = kp_kept(kp_ld(&st[w]));
        while (k) {
            const int j = __ffs((int)k) - 1;
            k &= k - 1;
            const unsigned q = (unsigned)w * 16u + (j >> 1);
            if (pos < K) {
                const int y = q / W;
                xy[2 * pos] = (int32_t)(q - (unsigned)y * W);
                xy[2 * pos + 1] = y;
                if (conf) conf[pos] = heat[q];
            }
            ++pos;
        }
    }
    for (int i = min(kept, K) + tid; i < K; i += KP_BLOCK) {
        xy[2 * i] = -1;
        xy[2 * i + 1] = -1;
        if (conf) conf[i] = 0.f;
    }
}

size_t kp_align(size_t b) { return (b + 255) & ~(size_t)255; }

// argument rules shared by the two entries; detect: H and W are multiples of the 8 x 8 cell
bool kp_check(rcn_ctx *ctx, const char *who, bool detect, const void *in, int32_t n, int32_t H, int32_t W, int32_t r, int32_t border, int32_t K,
              const void *xy, const void *counts)
{
    const char *why = nullptr;
    if (n < 0) why = "n < 0";
    else if (H < 1 || W < 1) why = "H and W must be positive";
    else if (detect && (H % 8 || W % 8)) why = "H and W must be multiples of 8";
    else if ((int64_t)H * W > 0x7FFFFFFFll) why = "H * W exceeds 2^31 - 1";
    else if (K < 1) why = "K < 1";
    else if (r < 0 || r > 8) why = "nms_radius outside 0..8";
    else if (border < 0) why = "border < 0";
    else if (!in || !xy || !counts) why = "null pointer";
    if (why) ctx->set_error(std::string(who) + ": bad argument (" + why + ")");
    return !why;
}

// images per pass over the workspace (the passes follow one another on the stream and share it)
int32_t kp_chunk(int32_t n, size_t per_image)
{
    const size_t budget = (size_t)1 << 30;
    return (int32_t)std::max<size_t>(1, std::min<size_t>({(size_t)n, budget / std::max<size_t>(per_image, 1), (size_t)32768}));
}

int kp_nms_setup(rcn_ctx *ctx)
{
    static std::mutex once_mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> lk(once_mu);
    if (std::find(done.begin(), done.end(), ctx->device) == done.end()) {
        RCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_kp_nms), hipFuncAttributeMaxDynamicSharedMemorySize, (int)KP_LDS_STATUS));
        done.push_back(ctx->device);
    }
    return RCN_OK;
}

}  // namespace

extern "C" int rcn_kp_detect_device(rcn_ctx *ctx, const float *logits_dev, int64_t stride_img, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                                    int32_t n, int32_t H, int32_t W, int32_t heat_mode, double conf_thresh, int32_t nms_radius, int32_t border,
                                    int32_t K, int32_t *kp_xy_dev, float *conf_dev, int32_t *counts_dev, float *heat_out_dev, int32_t *rounds_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return rcn_int_kp_detect(ctx, logits_dev, stride_img, stride_c, stride_y, stride_x, n, H, W, heat_mode, conf_thresh, nms_radius, border, K,
                             kp_xy_dev, conf_dev, counts_dev, heat_out_dev, rounds_dev, false);
}

int rcn_int_kp_detect(rcn_ctx *ctx, const float *logits_dev, int64_t stride_img, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                      int32_t n, int32_t H, int32_t W, int32_t heat_mode, double conf_thresh, int32_t nms_radius, int32_t border,
                      int32_t K, int32_t *kp_xy_dev, float *conf_dev, int32_t *counts_dev, float *heat_out_dev, int32_t *rounds_dev, bool check_only)
{
    if (!kp_check(ctx, "rcn_kp_detect_device", true, logits_dev, n, H, W, nms_radius, border, K, kp_xy_dev, counts_dev)) return RCN_ERR_ARG;
    if (heat_mode != RCN_KP_HEAT_REFERENCE && heat_mode != RCN_KP_HEAT_SOFTMAX) {
        ctx->set_error("rcn_kp_detect_device: bad argument (unknown heat mode)");
        return RCN_ERR_ARG;
    }
    if (n == 0 || check_only) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = kp_nms_setup(ctx)) return rc;
    const bool ref = heat_mode == RCN_KP_HEAT_REFERENCE;
    const size_t HW = (size_t)H * W, words = (HW + 15) / 16;
    const int Hc = H / 8, Wc = W / 8;
    const bool use_lds = words * 4 <= KP_LDS_STATUS;
    const size_t b_list = kp_align(HW * 4), b_heat = heat_out_dev ? 0 : kp_align(HW * 4), b_st = use_lds ? 0 : kp_align(words * 4);
    const size_t b_scale = ref ? kp_align((size_t)64 * Hc * 4) + 2 * kp_align((size_t)64 * Hc * 8) : kp_align((size_t)Hc * Wc * 16);
    const int32_t nb = kp_chunk(n, b_list + b_heat + b_st + b_scale);
    // every array starts on a 256-byte boundary: sizes per image are multiples of 256, the count words come last
    RCN_HIP(ctx->kp_ws.reserve((b_list + b_heat + b_st + b_scale) * (size_t)nb + kp_align((size_t)nb * 4)));
    char *ws = ctx->kp_ws.as<char>();
    unsigned *list = reinterpret_cast<unsigned *>(ws);                ws += b_list * nb;
    float *heat_ws = reinterpret_cast<float *>(ws);                   ws += b_heat * nb;
    unsigned *st = reinterpret_cast<unsigned *>(ws);                  ws += b_st * nb;
    double *R = reinterpret_cast<double *>(ws), *suf = R + (size_t)nb * 64 * Hc;
    float *S = reinterpret_cast<float *>(ws + 2 * kp_align((size_t)64 * Hc * 8) * nb);
    double2 *cell = reinterpret_cast<double2 *>(ws);                    ws += b_scale * nb;
    unsigned *cnt = reinterpret_cast<unsigned *>(ws);
    for (int32_t first = 0; first < n; first += nb) {
        const int32_t m = std::min(nb, n - first);
        const float *lg = logits_dev + (int64_t)first * stride_img;
        float *heat = heat_out_dev ? heat_out_dev + (size_t)first * HW : heat_ws;
        RCN_HIP(hipMemsetAsync(cnt, 0, (size_t)m * 4, ctx->stream));
        const dim3 gpix((unsigned)((HW + KP_PIX * 256 - 1) / (KP_PIX * 256)), (unsigned)m);
        if (ref) {
            k_kp_plane<<<dim3(64, (unsigned)m), 64, 0, ctx->stream>>>(lg, stride_img, stride_c, stride_y, stride_x, Hc, Wc, R, suf, S);
            k_kp_heat<true><<<gpix, 256, 0, ctx->stream>>>(lg, stride_img, stride_c, stride_y, stride_x, H, W, S, nullptr, conf_thresh, heat, cnt, list);
        } else {
            k_kp_cell<<<dim3((unsigned)((Hc * Wc + 255) / 256), (unsigned)m), 256, 0, ctx->stream>>>(lg, stride_img, stride_c, stride_y, stride_x, Hc, Wc, cell);
            k_kp_heat<false><<<gpix, 256, 0, ctx->stream>>>(lg, stride_img, stride_c, stride_y, stride_x, H, W, nullptr, cell, conf_thresh, heat, cnt, list);
        }
        KpNmsArgs a{heat, list, cnt, st, H, W, nms_radius, border, K, use_lds ? 1 : 0, kp_xy_dev + (size_t)first * K * 2,
                    conf_dev ? conf_dev + (size_t)first * K : nullptr, counts_dev + first, rounds_dev ? rounds_dev + first : nullptr};
        k_kp_nms<<<(unsigned)m, KP_BLOCK, use_lds ? words * 4 : 0, ctx->stream>>>(a);
        RCN_HIP(hipGetLastError());
    }
    return RCN_OK;
}

extern "C" int rcn_kp_nms_device(rcn_ctx *ctx, const float *heat_dev, int32_t n, int32_t H, int32_t W, double conf_thresh, int32_t nms_radius,
                                 int32_t border, int32_t K, int32_t *kp_xy_dev, float *conf_dev, int32_t *counts_dev, int32_t *rounds_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!kp_check(ctx, "rcn_kp_nms_device", false, heat_dev, n, H, W, nms_radius, border, K, kp_xy_dev, counts_dev)) return RCN_ERR_ARG;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    if (int rc = kp_nms_setup(ctx)) return rc;
    const size_t HW = (size_t)H * W, words = (HW + 15) / 16;
    const bool use_lds = words * 4 <= KP_LDS_STATUS;
    const size_t b_list = kp_align(HW * 4), b_st = use_lds ? 0 : kp_align(words * 4);
    const int32_t nb = kp_chunk(n, b_list + b_st);
    RCN_HIP(ctx->kp_ws.reserve((b_list + b_st) * (size_t)nb + kp_align((size_t)nb * 4)));
    char *ws = ctx->kp_ws.as<char>();
    unsigned *list = reinterpret_cast<unsigned *>(ws);                ws += b_list * nb;
    unsigned *st = reinterpret_cast<unsigned *>(ws);                  ws += b_st * nb;
    unsigned *cnt = reinterpret_cast<unsigned *>(ws);
    for (int32_t first = 0; first < n; first += nb) {
        const int32_t m = std::min(nb, n - first);
        const float *heat = heat_dev + (size_t)first * HW;
        RCN_HIP(hipMemsetAsync(cnt, 0, (size_t)m * 4, ctx->stream));
        k_kp_threshold<<<dim3((unsigned)((HW + KP_PIX * 256 - 1) / (KP_PIX * 256)), (unsigned)m), 256, 0, ctx->stream>>>(heat, (unsigned)HW, conf_thresh, cnt, list);
        KpNmsArgs a{heat, list, cnt, st, H, W, nms_radius, border, K, use_lds ? 1 : 0, kp_xy_dev + (size_t)first * K * 2,
                    conf_dev ? conf_dev + (size_t)first * K : nullptr, counts_dev + first, rounds_dev ? rounds_dev + first : nullptr};
        k_kp_nms<<<(unsigned)m, KP_BLOCK, use_lds ? words * 4 : 0, ctx->stream>>>(a);
        RCN_HIP(hipGetLastError());
    }
    return RCN_OK;
}
