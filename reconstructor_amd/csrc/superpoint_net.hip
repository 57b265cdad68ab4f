// superpoint_net.hip -- SuperPoint's convolutional network on the GPU, weights supplied by the caller:
// the forward pass of FeatureSuperPoint::detect (FeatureSuperPoint.cpp:228-263, superNet.forward) in front of keypoints.hip and
// desc.hip, batched over the images of one call, on the ctx stream, nothing visiting the host.
//
//   k_sp_conv1a  the 1 -> 64 first layer (K = 9), plain VALU code; reads the caller's image through its strides, fp32 or bytes,
//                64 pixels of a row per workgroup, their 3 x 66 patch through LDS
//   k_sp_conv    implicit GEMM of a 3 x 3 (or 1 x 1) convolution: M = the pixels of a 2-D tile, N = cout, K = taps x CIN.  A
//                workgroup of four wavefronts owns 128 pixels x 64 channels or 64 pixels x 128 channels; the input tile with its
//                one-pixel halo goes through LDS in slices of 32 input channels (outside the image it is written as zeros, so the
//                product loop has no border branch), the weights of one (slice, tap) at a time, fetched into registers while the
//                step before is multiplied; __builtin_amdgcn_mfma_f32_32x32x2f32 (a k-ordered fmaf chain).  Bias, ReLU and -- in
//                conv1b, conv2b, conv3b -- the 2 x 2 max pool in the epilogue: a 32-pixel block is 4 rows x 8 columns, and pixel
//                (2 wy + dy, 2 wx + dx) is accumulator row dx + 2 dy + 4 (wx + 4 wy), which puts the four partners of a pool
//                window into four consecutive registers of one lane.
//   k_sp_l2norm  the descriptor normalisation: one wavefront per cell, one lane adds the squares in ascending channel order
//
// Activations are channel-last [image][y][x][c] fp32 in two ping-pong buffers of the ctx's workspace (256 and 64 bytes per
// input pixel).  Every reduction runs in an order fixed at compile time (ascending cin slices, ascending taps inside a slice,
// ascending cin inside a tap); an image's result depends on the image alone, never on the batch, the chunk, the tile position
// or the run.
#include "rcn_internal.h"

#include <algorithm>

struct rcn_sp_net {
    rcn_ctx *ctx = nullptr;
    float *dev = nullptr;            // the re-laid-out weights (one allocation)
    size_t w[12], b[12];             // offsets into dev, in floats; convDa ([10]) follows convPa ([8]): one layer of 512 channels
};

namespace {

#pragma clang fp contract(off)

constexpr int SP_LAYERS = 12;
// conv1a 1b 2a 2b 3a 3b 4a 4b Pa Pb Da Db
constexpr int SP_CIN[SP_LAYERS] = {1, 64, 64, 64, 64, 128, 128, 128, 128, 256, 128, 256};
constexpr int SP_COUT[SP_LAYERS] = {64, 64, 64, 64, 128, 128, 128, 128, 256, 65, 256, 256};
constexpr int SP_TAPS[SP_LAYERS] = {9, 9, 9, 9, 9, 9, 9, 9, 9, 1, 9, 1};
constexpr size_t SP_WS_BYTES = (size_t)512 << 20;    // default cap of the activations of one chunk of images
constexpr int SP_SLICE = 32768;                      // images per launch at most (grid dimension z)
constexpr int SP_K = 32, SP_LD = SP_K + 1;           // input channels per LDS slice; floats per LDS row
constexpr int SP_TW = 8;                             // tile width in pixels

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr size_t sp_param_count()
{
    size_t n = 0;
    for (int i = 0; i < SP_LAYERS; ++i) n += (size_t)SP_COUT[i] * SP_CIN[i] * SP_TAPS[i] + SP_COUT[i];
    return n;
}
static_assert(sp_param_count() == RCN_SP_N_PARAMS, "the layer table and RCN_SP_N_PARAMS disagree");

// max that keeps a NaN (torch's max_pool2d does)
__device__ __forceinline__ float sp_max(float a, float b) { return (b > a || b != b) ? b : a; }

// ---- first layer ----------------------------------------------------------------------------------------------------------------

struct SpImages {
    const void *p;
    long long si, sy, sx;             // element strides
    int u8;
};
__device__ __forceinline__ float sp_pixel(const SpImages &im, int img, int y, int x)
{
    const long long at = (long long)img * im.si + (long long)y * im.sy + (long long)x * im.sx;
    if (im.u8) return (float)((double)reinterpret_cast<const unsigned char *>(im.p)[at] / 255.0);
    return reinterpret_cast<const float *>(im.p)[at];
}
// grid (H * ceil(W / 64), images), 256 threads: a workgroup takes 64 consecutive pixels of one row, whose 3 x 66 patch goes
// through LDS (zeros outside the image); lane = output channel, a wavefront takes 16 of the pixels
__global__ __launch_bounds__(256) void k_sp_conv1a(SpImages im, int img0, int H, int W, int segs, const float *__restrict__ Wt /*[64][9]*/,
                                                   const float *__restrict__ bias, float *__restrict__ out /*[img][H][W][64]*/)
{
    __shared__ float patch[3][68];
    const int img = blockIdx.y, co = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = blockIdx.x / segs, x0 = (blockIdx.x % segs) * 64;
    if (threadIdx.x < 3 * 66) {
        const int r = threadIdx.x / 66, c = threadIdx.x % 66, yy = y + r - 1, xx = x0 + c - 1;
        patch[r][c] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? sp_pixel(im, img0 + img, yy, xx) : 0.f;
    }
    float w[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = Wt[co * 9 + t];
    const float b = bias[co];
    __syncthreads();
    float *row = out + (((size_t)img * H + y) * W) * 64 + co;
    for (int i = 0; i < 16; ++i) {
        const int xl = wave * 16 + i, x = x0 + xl;
        if (x >= W) break;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) acc = fmaf(patch[t / 3][xl + t % 3], w[t], acc);
        const float r = acc + b;
        row[(size_t)x * 64] = r < 0.f ? 0.f : r;                          // (a NaN stays a NaN)
    }
}

// ---- implicit-GEMM convolution ----------------------------------------------------------------------------------------------------

struct SpConvArgs {
    const float *X;                   // [img][H][W][in_ld], channels in_c0 .. in_c0 + CIN - 1 are read
    const float *Wt, *b;              // [COUT][TAPS][CIN], [COUT]
    float *Y;                         // [img][Ho][Wo][COUT]; Ho = H / 2, Wo = W / 2 when pooled
    int H, W, in_ld, in_c0, relu, tiles_x;
};

template <int COUT> struct SpShape {
    static constexpr int TC = COUT >= 128 ? 128 : 64;     // output channels of a workgroup
    static constexpr int WN = TC / 64, WM = 4 / WN;       // wavefronts along the channels / along the pixel blocks
    static constexpr int TH = 4 * WM;                     // tile height: WM blocks of 4 rows x 8 columns
};

// grid (tiles, ceil(COUT / TC), images), 256 threads: wavefront (wm, wn) owns rows 4 wm .. 4 wm + 3 of the tile and the
// channels 64 wn .. 64 wn + 63 of the workgroup's
template <int CIN, int COUT, int TAPS, bool POOL>
__global__ __launch_bounds__(256) void k_sp_conv(SpConvArgs a)
{
    using S = SpShape<COUT>;
    constexpr int HALO = TAPS == 9 ? 1 : 0;
    constexpr int PH = S::TH + 2 * HALO, PW = SP_TW + 2 * HALO;
    constexpr int KT = TAPS * CIN;                         // floats per weight row
    constexpr int WV = S::TC * SP_K / 4 / 256;             // float4 of a weight tile per thread
    constexpr int STEPS = (CIN / SP_K) * TAPS;
    static_assert(CIN % SP_K == 0 && WV >= 1, "shape");
    __shared__ float xs[PH * PW][SP_LD], ws[S::TC][SP_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave % S::WM, wn = wave / S::WM;
    const int l31 = lane & 31, half = lane >> 5;
    const int img = blockIdx.z, c0 = blockIdx.y * S::TC;
    const int ty0 = (blockIdx.x / a.tiles_x) * S::TH, tx0 = (blockIdx.x % a.tiles_x) * SP_TW;
    const float *X = a.X + (size_t)img * a.H * a.W * a.in_ld + a.in_c0;
    // the lane's pixel as the A operand: row l31 of the block = (2 wy + dy, 2 wx + dx)
    const int py = 4 * wm + 2 * (l31 >> 4) + ((l31 >> 1) & 1), px = 2 * ((l31 >> 2) & 3) + (l31 & 1);
    const bool live = c0 + wn * 64 < COUT && ty0 + 4 * wm < a.H;       // the wavefront has something to compute

    float4 wreg[WV];
    auto fetch = [&](int step) {
        const int k0 = (step / TAPS) * SP_K, tap = step % TAPS;
#pragma unroll
        for (int i = 0; i < WV; ++i) {
            const int e = tid + 256 * i, r = e >> 3, c4 = (e & 7) * 4;
            wreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 + r < COUT) wreg[i] = *reinterpret_cast<const float4 *>(a.Wt + (size_t)(c0 + r) * KT + tap * CIN + k0 + c4);
        }
    };
    fetch(0);
    f32x16 acc0 = {0}, acc1 = {0};
    for (int step = 0; step < STEPS; ++step) {
        const int tap = step % TAPS;
        if (tap == 0) {
            const int k0 = (step / TAPS) * SP_K;
            for (int e = tid; e < PH * PW * (SP_K / 4); e += 256) {
                const int r = e >> 3, c4 = (e & 7) * 4;
                const int gy = ty0 + r / PW - HALO, gx = tx0 + r % PW - HALO;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = *reinterpret_cast<const float4 *>(X + ((size_t)gy * a.W + gx) * a.in_ld + k0 + c4);
                xs[r][c4] = v.x; xs[r][c4 + 1] = v.y; xs[r][c4 + 2] = v.z; xs[r][c4 + 3] = v.w;
            }
        }
#pragma unroll
        for (int i = 0; i < WV; ++i) {
            const int e = tid + 256 * i, r = e >> 3, c4 = (e & 7) * 4;
            ws[r][c4] = wreg[i].x; ws[r][c4 + 1] = wreg[i].y; ws[r][c4 + 2] = wreg[i].z; ws[r][c4 + 3] = wreg[i].w;
        }
        __syncthreads();
        if (step + 1 < STEPS) fetch(step + 1);
        if (live) {
            const int ky = TAPS == 9 ? tap / 3 : 0, kx = TAPS == 9 ? tap % 3 : 0;
            const float *xa = &xs[(py + ky) * PW + px + kx][half], *wb = &ws[wn * 64 + l31][half];
#pragma unroll
            for (int k = 0; k < SP_K; k += 2) {
                const float x = xa[k];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, wb[k], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, wb[32 * SP_LD + k], acc1, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (!live) return;
    // accumulator register r of the lane is row (r & 3) + 8 (r >> 2) + 4 half of the block: window 2 (r >> 2) + half, partner r & 3
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int co = c0 + wn * 64 + t * 32 + l31;
        if (co >= COUT) continue;
        const float bias = a.b[co];
        if (POOL) {
            const int Ho = a.H >> 1, Wo = a.W >> 1;
            float *Y = a.Y + (size_t)img * Ho * Wo * COUT;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int w = 2 * g + half, oy = ((ty0 + 4 * wm) >> 1) + (w >> 2), ox = (tx0 >> 1) + (w & 3);
                float m = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float y = (t ? acc1[4 * g + j] : acc0[4 * g + j]) + bias;
                    if (a.relu) y = y < 0.f ? 0.f : y;
                    m = j ? sp_max(m, y) : y;
                }
                if (oy < Ho && ox < Wo) Y[((size_t)oy * Wo + ox) * COUT + co] = m;
            }
        } else {
            float *Y = a.Y + (size_t)img * a.H * a.W * COUT;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = (r & 3) + 8 * (r >> 2) + 4 * half;
                const int y = ty0 + 4 * wm + 2 * (p >> 4) + ((p >> 1) & 1), x = tx0 + 2 * ((p >> 2) & 3) + (p & 1);
                if (y >= a.H || x >= a.W) continue;
                float v = (t ? acc1[r] : acc0[r]) + bias;
                if (a.relu) v = v < 0.f ? 0.f : v;
                Y[((size_t)y * a.W + x) * COUT + co] = v;
            }
        }
    }
}

// ---- descriptor normalisation ---------------------------------------------------------------------------------------------------

// grid ceil(cells / 4), 256 threads: one wavefront per cell of [cells][256], in place
__global__ __launch_bounds__(256) void k_sp_l2norm(float *__restrict__ d, long long cells)
{
    __shared__ float sq[4][256 + 8];
    __shared__ float nrm[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long cell = (long long)blockIdx.x * 4 + w;
    const bool in = cell < cells;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (in) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = d[cell * 256 + lane + 64 * i];
            sq[w][lane + 64 * i] = __fmul_rn(v[i], v[i]);
        }
    }
    __syncthreads();
    if (in && lane == 0) {
        float sum = 0.f;
        for (int c = 0; c < 256; ++c) sum = __fadd_rn(sum, sq[w][c]);
        nrm[w] = sqrtf(sum);
    }
    __syncthreads();
    if (in) {
        const float n = nrm[w];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[cell * 256 + lane + 64 * i] = v[i] / n;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

bool sp_fail(rcn_ctx *ctx, const char *who, const char *why)
{
    ctx->set_error(std::string(who) + ": bad argument (" + why + ")");
    return false;
}

template <int CIN, int COUT, int TAPS, bool POOL>
void sp_conv(rcn_ctx *ctx, const rcn_sp_net *net, int layer, const float *X, int in_ld, int in_c0, int H, int W, int imgs, bool relu, float *Y)
{
    using S = SpShape<COUT>;
    SpConvArgs a{};
    a.X = X; a.Wt = net->dev + net->w[layer]; a.b = net->dev + net->b[layer]; a.Y = Y;
    a.H = H; a.W = W; a.in_ld = in_ld; a.in_c0 = in_c0; a.relu = relu;
    a.tiles_x = (W + SP_TW - 1) / SP_TW;
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((H + S::TH - 1) / S::TH);
    k_sp_conv<CIN, COUT, TAPS, POOL><<<dim3(tiles, (unsigned)((COUT + S::TC - 1) / S::TC), (unsigned)imgs), 256, 0, ctx->stream>>>(a);
}

struct SpIn {
    const void *images;
    int32_t dtype;
    int64_t si, sy, sx;
    int32_t n, H, W, flags;
};

bool sp_check(rcn_ctx *ctx, const char *who, const rcn_sp_net *net, const SpIn &in)
{
    if (!net || net->ctx != ctx) return sp_fail(ctx, who, "the net does not belong to this ctx");
    if (in.n < 0) return sp_fail(ctx, who, "n < 0");
    if (in.H < 8 || in.W < 8 || in.H % 8 || in.W % 8) return sp_fail(ctx, who, "H and W must be positive multiples of 8");
    if ((int64_t)in.H * in.W > 0x7FFFFFFFll) return sp_fail(ctx, who, "H * W exceeds 2^31 - 1");
    if (in.dtype != RCN_SP_INPUT_F32 && in.dtype != RCN_SP_INPUT_U8) return sp_fail(ctx, who, "unknown input dtype");
    if (in.flags & ~RCN_SP_NORMALIZE_DESC) return sp_fail(ctx, who, "unknown flag");
    if (!in.images) return sp_fail(ctx, who, "null pointer");
    return true;
}

// with ctx->mu held and the arguments checked: logits [n][Hc][Wc][65] and descriptors [n][Hc][Wc][256]
int sp_forward(rcn_ctx *ctx, const rcn_sp_net *net, const SpIn &in, float *logits, float *desc)
{
    const int H = in.H, W = in.W, Hc = H / 8, Wc = W / 8;
    const size_t HW = (size_t)H * W, cells = (size_t)Hc * Wc;
    const size_t img_floats = 80 * HW;                    // buffer 0: 64 per pixel (conv1a's output), buffer 1: 16 (the pooled conv1b)
    size_t chunk = std::max<size_t>(1, SP_WS_BYTES / (img_floats * 4));
    if (ctx->sp_chunk_images > 0) chunk = (size_t)ctx->sp_chunk_images;
    chunk = std::min(std::min(chunk, (size_t)SP_SLICE), (size_t)in.n);
    RCN_HIP(ctx->sp_ws.reserve(chunk * img_floats * 4));
    float *b0 = ctx->sp_ws.as<float>(), *b1 = b0 + chunk * 64 * HW;
    const SpImages im{in.images, in.si, in.sy, in.sx, in.dtype == RCN_SP_INPUT_U8};
    const float *w = net->dev;
    for (int32_t i0 = 0; i0 < in.n; i0 += (int32_t)chunk) {
        const int m = (int)std::min<size_t>(chunk, (size_t)(in.n - i0));
        const int segs = (W + 63) / 64;
        k_sp_conv1a<<<dim3((unsigned)segs * (unsigned)H, (unsigned)m), 256, 0, ctx->stream>>>(im, i0, H, W, segs, w + net->w[0], w + net->b[0], b0);
        sp_conv<64, 64, 9, true>(ctx, net, 1, b0, 64, 0, H, W, m, true, b1);                      // conv1b + pool
        sp_conv<64, 64, 9, false>(ctx, net, 2, b1, 64, 0, H / 2, W / 2, m, true, b0);             // conv2a
        sp_conv<64, 64, 9, true>(ctx, net, 3, b0, 64, 0, H / 2, W / 2, m, true, b1);              // conv2b + pool
        sp_conv<64, 128, 9, false>(ctx, net, 4, b1, 64, 0, H / 4, W / 4, m, true, b0);            // conv3a
        sp_conv<128, 128, 9, true>(ctx, net, 5, b0, 128, 0, H / 4, W / 4, m, true, b1);           // conv3b + pool
        sp_conv<128, 128, 9, false>(ctx, net, 6, b1, 128, 0, Hc, Wc, m, true, b0);                // conv4a
        sp_conv<128, 128, 9, false>(ctx, net, 7, b0, 128, 0, Hc, Wc, m, true, b1);                // conv4b
        sp_conv<128, 512, 9, false>(ctx, net, 8, b1, 128, 0, Hc, Wc, m, true, b0);                // convPa and convDa
        float *lg = logits + (size_t)i0 * cells * 65, *ds = desc + (size_t)i0 * cells * 256;
        sp_conv<256, 65, 1, false>(ctx, net, 9, b0, 512, 0, Hc, Wc, m, false, lg);                // convPb
        sp_conv<256, 256, 1, false>(ctx, net, 11, b0, 512, 256, Hc, Wc, m, false, ds);            // convDb
        if (in.flags & RCN_SP_NORMALIZE_DESC) {
            const long long nc = (long long)m * (long long)cells;
            k_sp_l2norm<<<(unsigned)((nc + 3) / 4), 256, 0, ctx->stream>>>(ds, nc);
        }
        RCN_HIP(hipGetLastError());
    }
    return RCN_OK;
}

}  // namespace

extern "C" int rcn_sp_net_create(rcn_ctx *ctx, const float *params_host, int64_t n_params, rcn_sp_net **net_out)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sp_net_create";
    if (!net_out) { sp_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    *net_out = nullptr;
    if (!params_host) { sp_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    if (n_params != (int64_t)RCN_SP_N_PARAMS) {
        ctx->set_error(std::string(who) + ": bad argument (the network takes " + std::to_string(RCN_SP_N_PARAMS) + " parameters)");
        return RCN_ERR_ARG;
    }
    RCN_HIP(hipSetDevice(ctx->device));
    // re-layout: [Cout][Cin][tap] -> [Cout][tap][Cin], the k order the kernel streams; convPa and convDa become one layer of
    // 512 output channels (rows 0..255 convPa, 256..511 convDa); conv1a stays [64][9]
    std::vector<float> h((size_t)RCN_SP_N_PARAMS);
    rcn_sp_net *net = new rcn_sp_net;
    net->ctx = ctx;
    const float *src = params_host;
    size_t at = 0;
    auto weights = [&](int l) {            // appends layer l's re-laid-out weights, returns their offset
        const int co = SP_COUT[l], ci = SP_CIN[l], tp = SP_TAPS[l];
        const size_t o = at;
        for (int c = 0; c < co; ++c)
            for (int k = 0; k < ci; ++k)
                for (int t = 0; t < tp; ++t) h[o + ((size_t)c * tp + t) * ci + k] = src[((size_t)c * ci + k) * tp + t];
        at += (size_t)co * ci * tp;
        return o;
    };
    auto bias = [&](int l) {               // the bias follows the weights in the caller's block
        const size_t o = at;
        std::memcpy(h.data() + o, src + (size_t)SP_COUT[l] * SP_CIN[l] * SP_TAPS[l], SP_COUT[l] * sizeof(float));
        at += SP_COUT[l];
        return o;
    };
    const float *layer_src[SP_LAYERS];
    for (int l = 0; l < SP_LAYERS; ++l) {
        layer_src[l] = src;
        src += (size_t)SP_COUT[l] * SP_CIN[l] * SP_TAPS[l] + SP_COUT[l];
    }
    // every weight block first (each a multiple of four floats: the kernel loads float4), the biases behind them
    for (int l : {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 9, 11}) { src = layer_src[l]; net->w[l] = weights(l); }
    for (int l : {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 9, 11}) { src = layer_src[l]; net->b[l] = bias(l); }
    hipError_t e = hipMalloc((void **)&net->dev, h.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(net->dev, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (net->dev) (void)hipFree(net->dev);
        delete net;
        ctx->set_error(std::string(who) + ": " + hipGetErrorString(e));
        return RCN_ERR_HIP;
    }
    *net_out = net;
    return RCN_OK;
}

extern "C" void rcn_sp_net_destroy(rcn_sp_net *net)
{
    if (!net) return;
    {
        std::lock_guard<std::mutex> lk(net->ctx->mu);
        (void)hipSetDevice(net->ctx->device);
        (void)hipStreamSynchronize(net->ctx->stream);      // a forward may still read the weights
        (void)hipFree(net->dev);
    }
    delete net;
}

extern "C" int rcn_sp_net_set_chunk_images(rcn_ctx *ctx, int32_t images)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->sp_chunk_images = images > 0 ? images : 0;
    return RCN_OK;
}

extern "C" int rcn_sp_net_forward_device(rcn_ctx *ctx, const rcn_sp_net *net, const void *images_dev, int32_t input_dtype, int64_t stride_img,
                                         int64_t stride_y, int64_t stride_x, int32_t n, int32_t H, int32_t W, int32_t flags,
                                         float *logits_out_dev, float *desc_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sp_net_forward_device";
    const SpIn in{images_dev, input_dtype, stride_img, stride_y, stride_x, n, H, W, flags};
    if (!sp_check(ctx, who, net, in)) return RCN_ERR_ARG;
    if (!logits_out_dev || !desc_out_dev) { sp_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    return sp_forward(ctx, net, in, logits_out_dev, desc_out_dev);
}

extern "C" int rcn_sp_net_detect_device(rcn_ctx *ctx, const rcn_sp_net *net, const void *images_dev, int32_t input_dtype, int64_t stride_img,
                                        int64_t stride_y, int64_t stride_x, int32_t n, int32_t H, int32_t W, int32_t flags, int32_t heat_mode,
                                        double conf_thresh, int32_t nms_radius, int32_t border, int32_t K, int32_t D, int32_t *kp_xy_dev,
                                        float *conf_dev, int32_t *counts_dev, float *rows_out_dev, float *heat_out_dev, int32_t *rounds_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sp_net_detect_device";
    const SpIn in{images_dev, input_dtype, stride_img, stride_y, stride_x, n, H, W, flags};
    if (!sp_check(ctx, who, net, in)) return RCN_ERR_ARG;
    const int Hc = H / 8, Wc = W / 8;
    const size_t cells = (size_t)Hc * Wc;
    // the two stages behind the network check their own arguments before anything is launched (the addresses of the maps,
    // which do not exist yet, are not looked at beyond being non-null)
    const float *probe = reinterpret_cast<const float *>(images_dev);
    int rc;
    if ((rc = rcn_int_kp_detect(ctx, probe, (int64_t)cells * 65, 1, (int64_t)Wc * 65, 65, n, H, W, heat_mode, conf_thresh, nms_radius, border, K,
                                kp_xy_dev, conf_dev, counts_dev, heat_out_dev, rounds_dev, true)))
        return rc;
    if ((rc = rcn_int_desc_sample_batch(ctx, probe, (int64_t)cells * 256, 1, (int64_t)Wc * 256, 256, Hc, Wc, kp_xy_dev, counts_dev, n, K, D,
                                        rows_out_dev, true)))
        return rc;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    const size_t n_lg = (size_t)n * cells * 65, n_ds = (size_t)n * cells * 256;
    RCN_HIP(ctx->sp_out.reserve((n_lg + 3 + n_ds) * 4));
    float *lg = ctx->sp_out.as<float>(), *ds = lg + ((n_lg + 3) & ~(size_t)3);
    if ((rc = sp_forward(ctx, net, in, lg, ds))) return rc;
    if ((rc = rcn_int_kp_detect(ctx, lg, (int64_t)cells * 65, 1, (int64_t)Wc * 65, 65, n, H, W, heat_mode, conf_thresh, nms_radius, border, K,
                                kp_xy_dev, conf_dev, counts_dev, heat_out_dev, rounds_dev, false)))
        return rc;
    return rcn_int_desc_sample_batch(ctx, ds, (int64_t)cells * 256, 1, (int64_t)Wc * 256, 256, Hc, Wc, kp_xy_dev, counts_dev, n, K, D, rows_out_dev,
                                     false);
}
