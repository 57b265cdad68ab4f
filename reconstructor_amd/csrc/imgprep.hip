// imgprep.hip -- what detectFeatures does to a decoded photograph before a detector sees it, and what becomes of the colours
// afterwards: Utils::readImg's BGR -> RGB swap and reshapeImg (cv::resize, INTER_LINEAR on 8-bit data),
// cv::cvtColor(RGB2GRAY), the colour under every feature, a landmark's colour, Utils::saveCloud.  The contract is the
// restatement in tests/img_ref.py; every output byte equals it.
//
//   tables       built on the HOST in resize.cpp's own float / double operations (this file is compiled without contraction),
//                uploaded per call: {index, w0, w1} per output column and row.  The kernels do integer arithmetic only.
//   prepare      k_img_prepare: one workgroup per tile of IMG_TW x tile_rows output pixels.  The spans of the two (clipped)
//                source rows every output row reads are staged into LDS with 16-byte loads from addresses aligned down
//                (3-byte pixels are never dword aligned); source rows no output row reads are never touched.  One lane per
//                output pixel: the swap, the horizontal pass (int32, in registers), the vertical pass, the grey value.  Each
//                wave gathers its 64 pixels in LDS and writes them out in whole dwords.
//                tile_rows follows the horizontal scale (img_plan); when not even one row's spans fit, the one-row tile
//                reads its source pixels from memory directly (k_img_prepare<true>).
//   colours      k_feat_colors / k_landmark_colors: one lane per feature / landmark, gathers.
//   cloud        k_cloud_vertices: one lane per vertex; the camera centres in fp64, rounded products added in ascending order.
#include "rcn_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace {

#pragma clang fp contract(off)

constexpr int IMG_TW = 64;                       // output columns per tile: one wavefront per output row
constexpr int IMG_TH_MAX = 8;                    // output rows per tile at most
constexpr int IMG_LDS_BUDGET = 60 * 1024;        // staged source spans per workgroup
constexpr int IMG_OBUF = 256;                    // per wave: 192 bytes of colour, 64 of grey
constexpr int IMG_ONE = 2048;                    // INTER_RESIZE_COEF_SCALE
constexpr int64_t IMG_MAX_BLOCKS = 0xFFFFFFFFll / 256;   // a launch holds fewer than 2^32 work-items per dimension

struct ImgTab { int32_t idx; int16_t w0, w1; };

struct ImgArgs {
    const uint8_t *src; long long si, sr;
    int ch, src_rows, src_cols, rows, cols;
    const ImgTab *xt, *yt;
    uint8_t *rgb, *gray;
    int swap, gbits, area;                       // area: both axes halve -- (a + b + c + d + 2) >> 2
    int th, rowalloc, maxchunks, tiles_x;
};

// `bytes` bytes of a wave's LDS buffer to global memory: leading bytes up to the first aligned dword, whole dwords, the rest
__device__ __forceinline__ void img_wave_store(const uint8_t *buf, int bytes, uint8_t *dst, int lane)
{
    const int head = min((int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3), bytes);
    const int ndw = (bytes - head) >> 2, tail0 = head + 4 * ndw;
    if (lane < head) dst[lane] = buf[lane];
    for (int i = lane; i < ndw; i += 64) {
        const uint8_t *b = buf + head + 4 * i;
        *reinterpret_cast<uint32_t *>(dst + head + 4 * i) = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    if (lane < bytes - tail0) dst[tail0 + lane] = buf[tail0 + lane];
}

template <bool DIRECT>
__global__ __launch_bounds__(256) void k_img_prepare(ImgArgs a)
{
    extern __shared__ uint4 img_lds4[];
    uint8_t *lds = reinterpret_cast<uint8_t *>(img_lds4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * IMG_TW, y0 = ty * a.th;
    const int xl = min(x0 + IMG_TW, a.cols) - 1;                         // last column of the tile
    const int nrows = min(a.th, a.rows - y0);
    const uint8_t *base = a.src + (long long)blockIdx.y * a.si;
    const int c_first = a.xt[x0].idx, c_last = min(a.xt[xl].idx + 1, a.src_cols - 1);
    const int b0 = c_first * a.ch, span = (c_last - c_first + 1) * a.ch;

    if (!DIRECT) {
        // staged row r = 2 * (output row of the tile) + (0: upper, 1: lower source row); chunk k of it at lds[r * rowalloc + 16 k]
        const int items = 2 * nrows * a.maxchunks;
        for (int it = tid; it < items; it += 256) {
            const int r = it / a.maxchunks, k = it - r * a.maxchunks;
            const int s = min(max(a.yt[y0 + (r >> 1)].idx + (r & 1), 0), a.src_rows - 1);
            const uint8_t *p = base + (long long)s * a.sr + b0;
            const int lead = (int)(reinterpret_cast<uintptr_t>(p) & 15);
            if (16 * k < lead + span)                                     // every chunk loaded holds at least one byte of the span
                *reinterpret_cast<uint4 *>(lds + (size_t)r * a.rowalloc + 16 * k) = *reinterpret_cast<const uint4 *>(p - lead + 16 * k);
        }
        __syncthreads();
    }

    uint8_t *ob = lds + (DIRECT ? 0 : (size_t)2 * a.th * a.rowalloc) + wave * IMG_OBUF;
    const int x = min(x0 + lane, xl);
    const ImgTab cx = a.xt[x];
    const int o0 = (cx.idx - c_first) * a.ch, o1 = (min(cx.idx + 1, a.src_cols - 1) - c_first) * a.ch;
    const int wx0 = cx.w0, wx1 = cx.w1;
    const int r2y = a.gbits == 14 ? 4899 : 9798, g2y = a.gbits == 14 ? 9617 : 19235, b2y = a.gbits == 14 ? 1868 : 3735;

    for (int ry0 = 0; ry0 < a.th; ry0 += 4) {                            // the same trips for every wave: the barrier below
        const int ry = ry0 + wave;
        const bool rin = ry < nrows;
        if (rin) {
            const ImgTab cy = a.yt[y0 + ry];
            const int s0 = min(max(cy.idx, 0), a.src_rows - 1), s1 = min(max(cy.idx + 1, 0), a.src_rows - 1);
            const uint8_t *q0, *q1;
            if (DIRECT) {
                q0 = base + (long long)s0 * a.sr + b0;
                q1 = base + (long long)s1 * a.sr + b0;
            } else {
                const int l0 = (int)(reinterpret_cast<uintptr_t>(base + (long long)s0 * a.sr + b0) & 15);
                const int l1 = (int)(reinterpret_cast<uintptr_t>(base + (long long)s1 * a.sr + b0) & 15);
                q0 = lds + (size_t)(2 * ry) * a.rowalloc + l0;
                q1 = lds + (size_t)(2 * ry + 1) * a.rowalloc + l1;
            }
            const int wy0 = cy.w0, wy1 = cy.w1;
            int v[3] = {0, 0, 0};
            for (int c = 0; c < a.ch; ++c) {
                const int cs = a.swap ? a.ch - 1 - c : c;
                const int p00 = q0[o0 + cs], p01 = q0[o1 + cs], p10 = q1[o0 + cs], p11 = q1[o1 + cs];
                if (a.area) {
                    v[c] = (p00 + p01 + p10 + p11 + 2) >> 2;
                } else {
                    const int h0 = p00 * wx0 + p01 * wx1, h1 = p10 * wx0 + p11 * wx1;
                    const int t = ((wy0 * (h0 >> 4)) >> 16) + ((wy1 * (h1 >> 4)) >> 16);
                    v[c] = min(max((t + 2) >> 2, 0), 255);
                }
            }
            if (a.ch == 3) {
                ob[3 * lane] = (uint8_t)v[0]; ob[3 * lane + 1] = (uint8_t)v[1]; ob[3 * lane + 2] = (uint8_t)v[2];
                ob[192 + lane] = (uint8_t)((r2y * v[0] + g2y * v[1] + b2y * v[2] + (1 << (a.gbits - 1))) >> a.gbits);
            } else {
                ob[192 + lane] = (uint8_t)v[0];
            }
        }
        __syncthreads();
        if (rin) {
            const long long px = ((long long)blockIdx.y * a.rows + (y0 + ry)) * a.cols + x0;
            const int w = xl - x0 + 1;
            if (a.rgb) img_wave_store(ob, 3 * w, a.rgb + 3 * px, lane);
            if (a.gray) img_wave_store(ob + 192, w, a.gray + px, lane);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_feat_colors(const uint8_t *rgb, int rows, int cols, const int2 *xy, const int *counts, int K, long long total, uchar4 *out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int i = (int)(t / K), k = (int)(t - (long long)i * K);
    uchar4 o = make_uchar4(0, 0, 0, 0);
    if (k < counts[i]) {
        const int2 p = xy[t];
        if (p.x >= 0 && p.x < cols && p.y >= 0 && p.y < rows) {
            const uint8_t *s = rgb + (((long long)i * rows + p.y) * cols + p.x) * 3;
            o = make_uchar4(s[0], s[1], s[2], 0);
        }
    }
    out[t] = o;
}

__global__ __launch_bounds__(256) void k_landmark_colors(const uchar4 *feat, int n, int K, int L, const int *first_img, const int *first_feat, uchar4 *out)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int i = first_img[l], k = first_feat[l];
    out[l] = (i >= 0 && i < n && k >= 0 && k < K) ? feat[(long long)i * K + k] : make_uchar4(0, 0, 0, 0);
}

struct CloudVertex { float x, y, z; uchar4 c; };

__global__ __launch_bounds__(256) void k_cloud_vertices(const double *xyz, const uchar4 *col, const uint8_t *inl, int L, const double *poses, int C, CloudVertex *out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nl = inl ? 2ll * L : L;
    if (t >= nl + C) return;
    CloudVertex v;
    if (t < nl) {
        const int l = (int)(t < L ? t : t - L);
        v.x = (float)xyz[3 * l]; v.y = (float)xyz[3 * l + 1]; v.z = (float)xyz[3 * l + 2];
        const uchar4 c = col[l];
        v.c = (inl && t < L && !inl[l]) ? make_uchar4(253, 0, 0, 255) : make_uchar4(c.x, c.y, c.z, 255);
    } else {
        const double *P = poses + 12 * (t - nl);
        double cen[3];
        for (int j = 0; j < 3; ++j)
            cen[j] = -__dadd_rn(__dadd_rn(__dmul_rn(P[j], P[3]), __dmul_rn(P[4 + j], P[7])), __dmul_rn(P[8 + j], P[11]));
        v.x = (float)cen[0]; v.y = (float)cen[1]; v.z = (float)cen[2];
        v.c = make_uchar4(0, 250, 0, 255);
    }
    out[t] = v;
}

// one axis of cv::resize's INTER_LINEAR tables (resize.cpp), in its own operations: double position, float fraction
void img_tables(int32_t src, int32_t dst, bool horizontal, ImgTab *t, int32_t *xmax_out)
{
    const double scale = 1.0 / ((double)dst / (double)src);
    int32_t xmax = dst;
    for (int32_t d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int32_t s = (int32_t)std::floor(f);
        f -= (float)s;
        if (horizontal) {
            if (s < 0) { s = 0; f = 0.f; }
            if (s + 1 >= src) { xmax = std::min(xmax, d); s = src - 1; f = 0.f; }
        }
        t[d].idx = s;
        t[d].w0 = (int16_t)std::nearbyint((1.f - f) * (float)IMG_ONE);       // round half to even (the default rounding mode)
        t[d].w1 = (int16_t)std::nearbyint(f * (float)IMG_ONE);
    }
    if (xmax_out) *xmax_out = xmax;
}

void img_area_tables(int32_t dst, ImgTab *t)
{
    for (int32_t d = 0; d < dst; ++d) { t[d].idx = 2 * d; t[d].w0 = IMG_ONE / 2; t[d].w1 = IMG_ONE / 2; }
}

struct ImgPlan { int th, rowalloc, maxchunks, lds; };

// the tile height the staged spans allow: the widest span of any tile's two border columns, rounded to the 16-byte chunks an
// unaligned start can add
ImgPlan img_plan(const ImgTab *xt, int32_t src_cols, int32_t cols, int32_t ch)
{
    int64_t maxspan = 0;
    for (int32_t x0 = 0; x0 < cols; x0 += IMG_TW) {
        const int32_t xl = std::min(x0 + IMG_TW, cols) - 1;
        maxspan = std::max<int64_t>(maxspan, ((int64_t)std::min(xt[xl].idx + 1, src_cols - 1) - xt[x0].idx + 1) * ch);
    }
    ImgPlan p;
    const int64_t chunks = (15 + maxspan + 15) / 16, rowalloc = 16 * chunks + 16;
    p.th = IMG_TH_MAX;
    while (p.th >= 1 && 2 * p.th * rowalloc > IMG_LDS_BUDGET) p.th >>= 1;
    p.maxchunks = p.th ? (int)chunks : 0;
    p.rowalloc = p.th ? (int)rowalloc : 0;
    p.lds = 2 * p.th * p.rowalloc + 4 * IMG_OBUF;
    return p;
}

int img_fail(rcn_ctx *ctx, const char *who, const char *why)
{
    ctx->set_error(std::string(who) + ": bad argument (" + why + ")");
    return RCN_ERR_ARG;
}

}  // namespace

extern "C" int rcn_img_reshape_size(int32_t rows, int32_t cols, int32_t max_size, int32_t *rows_out, int32_t *cols_out, double *factor_out)
{
    if (rows < 1 || cols < 1 || max_size < 1 || !rows_out || !cols_out) return RCN_ERR_ARG;
    int32_t r = rows, c = cols;
    double factor = 1.0;
    if (rows > cols) {
        if (rows > max_size) {
            const double aspect = static_cast<double>(cols) / rows;
            double col_size = max_size * aspect;
            col_size = col_size - std::fmod(col_size, 8);
            r = max_size; c = (int32_t)col_size;
            factor = static_cast<double>(max_size) / rows;
        }
    } else if (cols > max_size) {
        const double aspect = static_cast<double>(rows) / cols;
        double row_size = max_size * aspect;
        row_size = row_size - std::fmod(row_size, 8);
        c = max_size; r = (int32_t)row_size;
        factor = static_cast<double>(max_size) / cols;
    }
    if (r < 1 || c < 1) return RCN_ERR_ARG;
    *rows_out = r; *cols_out = c;
    if (factor_out) *factor_out = factor;
    return RCN_OK;
}

extern "C" int rcn_img_resize_tables(int32_t src, int32_t dst, int32_t horizontal, int32_t *index_out, int16_t *weights_out, int32_t *xmax_out)
{
    if (src < 1 || dst < 1 || !index_out || !weights_out) return RCN_ERR_ARG;
    std::vector<ImgTab> t((size_t)dst);
    img_tables(src, dst, horizontal != 0, t.data(), xmax_out);
    for (int32_t d = 0; d < dst; ++d) { index_out[d] = t[d].idx; weights_out[2 * d] = t[d].w0; weights_out[2 * d + 1] = t[d].w1; }
    return RCN_OK;
}

extern "C" void rcn_img_default_options(rcn_img_options *opt)
{
    if (!opt) return;
    opt->order = RCN_IMG_BGR;
    opt->gray_bits = 14;
}

extern "C" int rcn_img_prepare_plan(int32_t src_cols, int32_t cols, int32_t channels, int32_t *tile_cols, int32_t *tile_rows, int32_t *lds_bytes)
{
    if (src_cols < 1 || cols < 1 || (channels != 1 && channels != 3) || (int64_t)src_cols * channels > INT32_MAX) return RCN_ERR_ARG;
    std::vector<ImgTab> t((size_t)cols);
    img_tables(src_cols, cols, true, t.data(), nullptr);
    const ImgPlan p = img_plan(t.data(), src_cols, cols, channels);
    if (tile_cols) *tile_cols = IMG_TW;
    if (tile_rows) *tile_rows = p.th;
    if (lds_bytes) *lds_bytes = p.lds;
    return RCN_OK;
}

extern "C" int rcn_img_prepare_device(rcn_ctx *ctx, const uint8_t *src_dev, int64_t stride_img_bytes, int64_t stride_row_bytes, int32_t channels,
                                      int32_t n, int32_t src_rows, int32_t src_cols, int32_t rows, int32_t cols, const rcn_img_options *opt,
                                      uint8_t *rgb_out_dev, uint8_t *gray_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_img_prepare_device";
    rcn_img_options use;
    rcn_img_default_options(&use);
    if (opt) use = *opt;
    if (channels != 1 && channels != 3) return img_fail(ctx, who, "channels must be 1 or 3");
    if (n < 0) return img_fail(ctx, who, "n < 0");
    if (src_rows < 1 || src_cols < 1 || rows < 1 || cols < 1) return img_fail(ctx, who, "a size is not positive");
    if ((int64_t)src_cols * channels > INT32_MAX) return img_fail(ctx, who, "a source row of more than 2^31 - 1 bytes");
    if (stride_row_bytes < (int64_t)src_cols * channels) return img_fail(ctx, who, "row stride below src_cols * channels");
    if ((int64_t)rows * cols * 3 > INT32_MAX) return img_fail(ctx, who, "rows * cols * 3 > 2^31 - 1");
    if (use.order != RCN_IMG_RGB && use.order != RCN_IMG_BGR) return img_fail(ctx, who, "unknown channel order");
    if (use.gray_bits != 14 && use.gray_bits != 15) return img_fail(ctx, who, "gray_bits must be 14 or 15");
    if (!rgb_out_dev && !gray_out_dev) return img_fail(ctx, who, "both outputs are null");
    if (channels == 1 && rgb_out_dev) return img_fail(ctx, who, "a single-channel source has no colour output");
    if (n > 0 && !src_dev) return img_fail(ctx, who, "null pointer");
    if (n == 0) return RCN_OK;
    // the horizontal table alone fixes the tile: the launch is sized, and refused when it cannot be made, before anything of
    // the size of the output is built
    const bool area = src_rows == 2 * (int64_t)rows && src_cols == 2 * (int64_t)cols;
    std::vector<ImgTab> xtab((size_t)cols);
    if (area) img_area_tables(cols, xtab.data());
    else img_tables(src_cols, cols, true, xtab.data(), nullptr);
    const ImgPlan p = img_plan(xtab.data(), src_cols, cols, channels);
    const int32_t th = std::max(p.th, 1), tiles_x = (cols + IMG_TW - 1) / IMG_TW;
    const int64_t tiles = (int64_t)tiles_x * ((rows + th - 1) / th);
    if (tiles > IMG_MAX_BLOCKS) return img_fail(ctx, who, "more than 2^24 - 1 tiles: the destination is too thin for its size");
    RCN_HIP(hipSetDevice(ctx->device));

    if (ctx->img_stage_pending) { RCN_HIP(hipEventSynchronize(ctx->img_ev)); ctx->img_stage_pending = false; }     // the staging buffer is free again
    ctx->img_stage_host.resize(((size_t)cols + rows) * sizeof(ImgTab));
    ImgTab *xt = reinterpret_cast<ImgTab *>(ctx->img_stage_host.data()), *yt = xt + cols;
    std::copy(xtab.begin(), xtab.end(), xt);
    if (area) img_area_tables(rows, yt);
    else img_tables(src_rows, rows, false, yt, nullptr);
    if (!ctx->img_ev && hipEventCreateWithFlags(&ctx->img_ev, hipEventDisableTiming) != hipSuccess) { ctx->img_ev = nullptr; RCN_HIP(hipGetLastError()); }
    RCN_HIP(ctx->img_ws.reserve(ctx->img_stage_host.size()));
    RCN_HIP(hipMemcpyAsync(ctx->img_ws.p, xt, ctx->img_stage_host.size(), hipMemcpyHostToDevice, ctx->stream));
    RCN_HIP(hipEventRecord(ctx->img_ev, ctx->stream));
    ctx->img_stage_pending = true;

    ImgArgs a;
    std::memset(&a, 0, sizeof a);
    a.si = stride_img_bytes; a.sr = stride_row_bytes;
    a.ch = channels; a.src_rows = src_rows; a.src_cols = src_cols; a.rows = rows; a.cols = cols;
    a.xt = ctx->img_ws.as<ImgTab>(); a.yt = a.xt + cols;
    a.swap = channels == 3 && use.order == RCN_IMG_BGR; a.gbits = use.gray_bits; a.area = area;
    a.th = th; a.rowalloc = p.rowalloc; a.maxchunks = p.maxchunks; a.tiles_x = tiles_x;
    for (int32_t first = 0; first < n; first += 65535) {
        const int32_t m = std::min(65535, n - first);
        a.src = src_dev + (int64_t)first * stride_img_bytes;
        a.rgb = rgb_out_dev ? rgb_out_dev + (int64_t)first * rows * cols * 3 : nullptr;
        a.gray = gray_out_dev ? gray_out_dev + (int64_t)first * rows * cols : nullptr;
        if (p.th) k_img_prepare<false><<<dim3((unsigned)tiles, (unsigned)m), 256, (size_t)p.lds, ctx->stream>>>(a);
        else k_img_prepare<true><<<dim3((unsigned)tiles, (unsigned)m), 256, (size_t)p.lds, ctx->stream>>>(a);
    }
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

extern "C" int rcn_feat_colors_device(rcn_ctx *ctx, const uint8_t *rgb_dev, int32_t n, int32_t rows, int32_t cols, const int32_t *xy_int_dev,
                                      const int32_t *counts_dev, int32_t K, uint8_t *rgba_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_feat_colors_device";
    if (n < 0) return img_fail(ctx, who, "n < 0");
    if (rows < 1 || cols < 1 || K < 1) return img_fail(ctx, who, "a size is not positive");
    if ((int64_t)rows * cols * 3 > INT32_MAX) return img_fail(ctx, who, "rows * cols * 3 > 2^31 - 1");
    if (n > 0 && (!rgb_dev || !xy_int_dev || !counts_dev || !rgba_out_dev)) return img_fail(ctx, who, "null pointer");
    const long long total = (long long)n * K;
    if ((total + 255) / 256 > IMG_MAX_BLOCKS) return img_fail(ctx, who, "n * K is more than one launch holds (2^32 - 256 slots)");
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    k_feat_colors<<<(unsigned)((total + 255) / 256), 256, 0, ctx->stream>>>(rgb_dev, rows, cols, reinterpret_cast<const int2 *>(xy_int_dev), counts_dev, K, total,
                                                                              reinterpret_cast<uchar4 *>(rgba_out_dev));
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

extern "C" int rcn_landmark_colors_device(rcn_ctx *ctx, const uint8_t *feat_rgba_dev, int32_t n, int32_t K, int32_t L, const int32_t *first_img_dev,
                                          const int32_t *first_feat_dev, uint8_t *rgba_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_landmark_colors_device";
    if (n < 0 || K < 0 || L < 0) return img_fail(ctx, who, "a negative size");
    if (L > 0 && (!first_img_dev || !first_feat_dev || !rgba_out_dev || ((int64_t)n * K > 0 && !feat_rgba_dev))) return img_fail(ctx, who, "null pointer");
    if (L == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    k_landmark_colors<<<(unsigned)((L + 255) / 256), 256, 0, ctx->stream>>>(reinterpret_cast<const uchar4 *>(feat_rgba_dev), n, K, L, first_img_dev, first_feat_dev,
                                                                            reinterpret_cast<uchar4 *>(rgba_out_dev));
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

extern "C" int rcn_cloud_vertices_device(rcn_ctx *ctx, const double *xyz_dev, const uint8_t *lm_rgba_dev, const uint8_t *inlier_dev, int32_t L,
                                         const double *poses34_dev, int32_t C, void *vertices_out_dev, int64_t *n_vertices_out)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_cloud_vertices_device";
    if (L < 0 || C < 0) return img_fail(ctx, who, "a negative size");
    if (!n_vertices_out) return img_fail(ctx, who, "null pointer");
    const int64_t total = (inlier_dev ? 2ll : 1ll) * L + C;
    if ((total + 255) / 256 > IMG_MAX_BLOCKS) return img_fail(ctx, who, "more vertices than one launch holds (2^32 - 256)");
    if ((L > 0 && (!xyz_dev || !lm_rgba_dev)) || (C > 0 && !poses34_dev) || (total > 0 && !vertices_out_dev)) return img_fail(ctx, who, "null pointer");
    *n_vertices_out = total;
    if (total == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    k_cloud_vertices<<<(unsigned)((total + 255) / 256), 256, 0, ctx->stream>>>(xyz_dev, reinterpret_cast<const uchar4 *>(lm_rgba_dev), inlier_dev, L, poses34_dev, C,
                                                                               reinterpret_cast<CloudVertex *>(vertices_out_dev));
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

extern "C" int rcn_cloud_write_ply(const char *path, const void *vertices_host, int64_t n_vertices, int32_t binary)
{
    if (!path || n_vertices < 0 || (n_vertices > 0 && !vertices_host)) return RCN_ERR_ARG;
    FILE *f = std::fopen(path, "wb");
    if (!f) return RCN_ERR_IO;
    bool ok = std::fprintf(f, "ply\nformat %s 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
                              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n",
                           binary ? "binary_little_endian" : "ascii", (long long)n_vertices) > 0;
    const CloudVertex *v = static_cast<const CloudVertex *>(vertices_host);
    if (ok && binary) {
        ok = n_vertices == 0 || std::fwrite(v, sizeof(CloudVertex), (size_t)n_vertices, f) == (size_t)n_vertices;     // the host is little endian, as the device
    } else if (ok) {
        for (int64_t i = 0; i < n_vertices && ok; ++i)
            ok = std::fprintf(f, "%.9g %.9g %.9g %u %u %u %u\n", (double)v[i].x, (double)v[i].y, (double)v[i].z, (unsigned)v[i].c.x, (unsigned)v[i].c.y,
                              (unsigned)v[i].c.z, (unsigned)v[i].c.w) > 0;
    }
    if (std::fclose(f) != 0) ok = false;
    if (!ok) { std::remove(path); return RCN_ERR_IO; }
    return RCN_OK;
}
