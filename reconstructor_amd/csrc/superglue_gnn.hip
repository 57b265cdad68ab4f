// superglue_gnn.hip -- SuperGlue's attentional graph network on the GPU, weights supplied by the caller:
// what FeatureMatcherSuperglue::matchFeatures (FeatureMatcherSuperglue.cpp:51-101) runs in front of the optimal-matching layer
// of superglue.hip -- normalizeFeatCoords (utils.cpp:119-149), the keypoint encoder, L self / cross attention layers and the
// final projection -- batched over the pairs of one call, on the ctx stream, nothing visiting the host.
//
//   k_gnn_enc0   the 3-wide first encoder layer, plain VALU code; normalises the coordinates when image shapes are given
//   k_gnn_linear Y = act(W [X1; X2] + b) (+ R): 64 points x 128 channels per workgroup, 32-wide k tiles staged through LDS,
//                __builtin_amdgcn_mfma_f32_32x32x2f32 (a k-ordered fmaf chain); all 2B point sets of a chunk in one launch
//   k_gnn_attn   one workgroup per (point set, head, 128 queries), one wavefront per 32 queries; key blocks of 32 in ascending
//                order; S^T = K Q^T on MFMA puts a query on a lane and its keys in the lane's registers, so the online
//                maximum and sum are per-lane and P is already the B operand of O^T = V^T P^T: it never leaves the registers
//
// Storage and arithmetic are fp32 throughout.  Every reduction runs in an order fixed at compile time (ascending k tiles,
// ascending key blocks); a point's result depends on its pair alone, never on the batch, the chunk or the run.
#include "rcn_internal.h"

#include <algorithm>
#include <cmath>

struct rcn_sg_net {
    rcn_ctx *ctx = nullptr;
    int L = 0;
    std::vector<int32_t> types;
    double bin_score = 0.0;
    float *dev = nullptr;            // the repacked weights (one allocation)
    // offsets into dev, in floats
    size_t enc_w[5], enc_b[5];
    std::vector<size_t> qkv_w, qkv_b, mrg_w, mrg_b, m0_w, m0_b, m1_w, m1_b;
    size_t fin_w = 0, fin_b = 0;
};

namespace {

#pragma clang fp contract(off)

constexpr int GD = 256;                       // feature dimension
constexpr int GH = 4, GHD = 64;               // heads, channels of a head
constexpr int ENC[6] = {3, 32, 64, 128, 256, 256};
constexpr int LIN_P = 64, LIN_C = 128, LIN_K = 32, LIN_LD = LIN_K + 1;
constexpr int ATT_Q = 128, ATT_KB = 32, ATT_KLD = GHD + 1, ATT_VLD = GHD + 8;
constexpr size_t GNN_WS_BYTES = (size_t)512 << 20;   // default cap of the activations of one chunk of pairs
constexpr int GNN_SLICE = 16384;              // pairs per launch at most (grid dimension z carries two sets per pair)
constexpr int WS_FLOATS = 2048;               // per point: x 256, qkv 768, o 256, msg 256, hidden 512

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct GnnCounts { const int32_t *m_dev, *n_dev; int M, N, b0; };
// points of set `s` of the chunk (pair b0 + s / 2, side s & 1); an empty pair has no points on either side
__device__ __forceinline__ int gnn_count(const GnnCounts &c, int s)
{
    const int b = c.b0 + (s >> 1);
    int m = c.m_dev ? c.m_dev[b] : c.M, n = c.n_dev ? c.n_dev[b] : c.N;
    m = min(max(m, 0), c.M);
    n = min(max(n, 0), c.N);
    if (m == 0 || n == 0) return 0;
    return (s & 1) ? n : m;
}

// where a [set][point][channel] array lives: the chunk's workspace (by_pair = 0: set-major, stride ss[0]) or two arrays of
// the caller, one per side, addressed by (pair, row, channel) element strides
struct GnnAddr {
    float *p[2];
    long long ss[2], sr[2], sc[2];
    int by_pair;
};
__device__ __forceinline__ float *gnn_at(const GnnAddr &a, int b0, int s, int pt, int c)
{
    if (!a.by_pair) return a.p[0] + (long long)s * a.ss[0] + (long long)pt * a.sr[0] + (long long)c * a.sc[0];
    const int side = s & 1;
    return a.p[side] + (long long)(b0 + (s >> 1)) * a.ss[side] + (long long)pt * a.sr[side] + (long long)c * a.sc[side];
}

// ---- encoder, first layer ---------------------------------------------------------------------------------------------------

struct Enc0Args {
    GnnCounts cnt;
    const float *kp[2], *sc[2];       // [B][M][2], [B][M] and the same for image 1 in N
    const int32_t *shape[2];          // [B][2] (H, W) or NULL: the coordinates are normalised already
    const float *W, *b;               // [32][3], [32]
    float *out;                       // [set][P][32]
    int P;
};
// grid (ceil(P / 8), sets): lane (point, channel)
__global__ __launch_bounds__(256) void k_gnn_enc0(Enc0Args a)
{
    const int s = blockIdx.y, side = s & 1, b = a.cnt.b0 + (s >> 1);
    const int cnt = gnn_count(a.cnt, s);
    const int pt = blockIdx.x * 8 + (threadIdx.x >> 5), co = threadIdx.x & 31;
    if (pt >= cnt) return;
    const int cap = side ? a.cnt.N : a.cnt.M;
    const float *kp = a.kp[side] + ((size_t)b * cap + pt) * 2;
    float kx = kp[0], ky = kp[1];
    if (a.shape[side]) {
        const int H = a.shape[side][2 * b], W = a.shape[side][2 * b + 1];
        const double scale = (double)max(H, W) * 0.7;
        kx = (float)(((double)kx - (double)(W / 2)) / scale);
        ky = (float)(((double)ky - (double)(H / 2)) / scale);
    }
    const float sc = a.sc[side][(size_t)b * cap + pt];
    const float *w = a.W + co * 3;
    float y = fmaf(w[2], sc, fmaf(w[1], ky, w[0] * kx)) + a.b[co];
    a.out[((size_t)s * a.P + pt) * 32 + co] = y < 0.f ? 0.f : y;        // (a NaN stays a NaN)
}

// ---- batched linear layer -----------------------------------------------------------------------------------------------------

struct LinArgs {
    GnnCounts cnt;
    const float *X1, *X2;             // [set][P][C1], [set][P][Cin - C1] (X2 unused when C1 == Cin)
    int P, C1, Cin, Cout, relu;
    const float *W, *b;               // [Cout][Cin] row-major, [Cout]
    GnnAddr Y, R;                     // output; residual added behind the activation (R.p[0] == NULL: none)
};
// grid (ceil(P / 64), ceil(Cout / 128), sets), 256 threads: wavefront (wm, wn) owns points wm * 32 .., channels wn * 64 ..
__global__ __launch_bounds__(256) void k_gnn_linear(LinArgs a)
{
    __shared__ float xs[LIN_P][LIN_LD], ws[LIN_C][LIN_LD];
    const int s = blockIdx.z, cnt = gnn_count(a.cnt, s);
    const int p0 = blockIdx.x * LIN_P, c0 = blockIdx.y * LIN_C;
    if (p0 >= cnt) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int C2 = a.Cin - a.C1;
    const bool live = p0 + wm * 32 < cnt && c0 + wn * 64 < a.Cout;      // the wavefront has something to compute
    f32x16 acc0 = {0}, acc1 = {0};
    for (int k0 = 0; k0 < a.Cin; k0 += LIN_K) {
        const bool second = k0 >= a.C1;
        const float *X = second ? a.X2 + (size_t)s * a.P * C2 + (k0 - a.C1) : a.X1 + (size_t)s * a.P * a.C1 + k0;
        const int ldx = second ? C2 : a.C1;
        for (int e = tid; e < LIN_P * LIN_K / 4; e += 256) {
            const int r = e >> 3, c4 = (e & 7) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p0 + r < cnt) v = *reinterpret_cast<const float4 *>(X + (size_t)(p0 + r) * ldx + c4);
            xs[r][c4] = v.x; xs[r][c4 + 1] = v.y; xs[r][c4 + 2] = v.z; xs[r][c4 + 3] = v.w;
        }
        for (int e = tid; e < LIN_C * LIN_K / 4; e += 256) {
            const int r = e >> 3, c4 = (e & 7) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 + r < a.Cout) v = *reinterpret_cast<const float4 *>(a.W + (size_t)(c0 + r) * a.Cin + k0 + c4);
            ws[r][c4] = v.x; ws[r][c4 + 1] = v.y; ws[r][c4 + 2] = v.z; ws[r][c4 + 3] = v.w;
        }
        __syncthreads();
        if (live) {
            const float *xa = &xs[wm * 32 + l31][half], *wb = &ws[wn * 64 + l31][half];
#pragma unroll
            for (int k = 0; k < LIN_K; k += 2) {
                const float x = xa[k];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, wb[k], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, wb[32 * LIN_LD + k], acc1, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int co = c0 + wn * 64 + t * 32 + l31;
        if (co >= a.Cout) continue;
        const float bias = a.b[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int pt = p0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (pt >= cnt) continue;
            float y = (t ? acc1[r] : acc0[r]) + bias;
            if (a.relu) y = y < 0.f ? 0.f : y;
            if (a.R.p[0]) y = *gnn_at(a.R, a.cnt.b0, s, pt, co) + y;
            *gnn_at(a.Y, a.cnt.b0, s, pt, co) = y;
        }
    }
}

// ---- fused attention ------------------------------------------------------------------------------------------------------------

struct AttArgs {
    GnnCounts cnt;
    const float *qkv;                 // [set][P][768]: q (scaled by 1 / 8), k, v; a head's 64 channels contiguous
    float *o;                         // [set][P][256]
    int P, cross;
};
// grid (ceil(P / 128), heads, sets), 256 threads.  Wavefront w owns queries q0 + 32 w ..; lane l holds query l & 31, its half
// l >> 5 the channels 32 half .. of q (the B operand of S^T = K Q^T, k index = (channel & 31, channel >> 5)).  After the
// product the lane holds S^T[key][query] for the keys (r & 3) + 8 (r >> 2) + 4 half, r = 0..15: the accumulator layout, which
// is the B operand of O^T = V^T P^T when k-step r pairs exactly those two keys.
__global__ __launch_bounds__(256) void k_gnn_attn(AttArgs a)
{
    __shared__ float ks[ATT_KB][ATT_KLD], vs[ATT_KB][ATT_VLD];
    const int s = blockIdx.z, h = blockIdx.y, src = a.cross ? s ^ 1 : s;
    const int nq = gnn_count(a.cnt, s), nk = gnn_count(a.cnt, src);
    const int q0 = blockIdx.x * ATT_Q;
    if (q0 >= nq) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int qi = q0 + wave * 32 + l31;
    const bool live = q0 + wave * 32 < nq;
    float q[32];
    {
        const float *qp = a.qkv + ((size_t)s * a.P + qi) * (3 * GD) + h * GHD + 32 * half;
#pragma unroll
        for (int c = 0; c < 32; c += 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qi < nq) v = *reinterpret_cast<const float4 *>(qp + c);
            q[c] = v.x; q[c + 1] = v.y; q[c + 2] = v.z; q[c + 3] = v.w;
        }
    }
    f32x16 o0 = {0}, o1 = {0};
    float mx = -INFINITY, sum = 0.f;           // running maximum (both halves agree), this half's share of the sum
    const float *kv = a.qkv + (size_t)src * a.P * (3 * GD) + GD + h * GHD;
    for (int j0 = 0; j0 < nk; j0 += ATT_KB) {
        for (int e = tid; e < ATT_KB * GHD / 4; e += 256) {
            const int r = e >> 4, c4 = (e & 15) * 4;
            float4 k4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = k4;
            if (j0 + r < nk) {
                const float *row = kv + (size_t)(j0 + r) * (3 * GD) + c4;
                k4 = *reinterpret_cast<const float4 *>(row);
                v4 = *reinterpret_cast<const float4 *>(row + GD);
            }
            ks[r][c4] = k4.x; ks[r][c4 + 1] = k4.y; ks[r][c4 + 2] = k4.z; ks[r][c4 + 3] = k4.w;
            vs[r][c4] = v4.x; vs[r][c4 + 1] = v4.y; vs[r][c4 + 2] = v4.z; vs[r][c4 + 3] = v4.w;
        }
        __syncthreads();
        if (live) {
            f32x16 st = {0};
            const float *ka = &ks[l31][32 * half];
#pragma unroll
            for (int c = 0; c < 32; ++c) st = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[c], q[c], st, 0, 0, 0);
            float bm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = j0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (key >= nk) st[r] = -INFINITY;
                bm = fmaxf(bm, st[r]);
            }
            bm = fmaxf(bm, __shfl_xor(bm, 32));
            const float mnew = fmaxf(mx, bm);       // (a NaN score is dropped here and comes back through its own expf)
            const float scale = expf(mx - mnew);
            mx = mnew;
            float part = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                st[r] = expf(st[r] - mnew);
                part += st[r];
            }
            sum = sum * scale + part;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o0[r] *= scale; o1[r] *= scale; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float *va = &vs[(r & 3) + 8 * (r >> 2) + 4 * half][l31];
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[0], st[r], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[32], st[r], o1, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (qi >= nq) return;
    const float den = sum + __shfl_xor(sum, 32);
    float *op = a.o + ((size_t)s * a.P + qi) * GD + h * GHD + 4 * half;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4 *>(op + 8 * g) = make_float4(o0[4 * g] / den, o0[4 * g + 1] / den, o0[4 * g + 2] / den, o0[4 * g + 3] / den);
        *reinterpret_cast<float4 *>(op + 32 + 8 * g) = make_float4(o1[4 * g] / den, o1[4 * g + 1] / den, o1[4 * g + 2] / den, o1[4 * g + 3] / den);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

bool gnn_fail(rcn_ctx *ctx, const char *who, const char *why)
{
    ctx->set_error(std::string(who) + ": bad argument (" + why + ")");
    return false;
}

size_t gnn_param_count(int L)
{
    size_t n = 0;
    for (int i = 0; i < 5; ++i) n += (size_t)ENC[i + 1] * ENC[i] + ENC[i + 1];
    n += (size_t)L * (4 * ((size_t)GD * GD + GD) + ((size_t)2 * GD * 2 * GD + 2 * GD) + ((size_t)GD * 2 * GD + GD));
    return n + (size_t)GD * GD + GD;
}

// published channel c is head c % 4 at depth c / 4 (view(b, 64, 4, n)); the device keeps a head's channels contiguous
inline int gnn_perm(int c) { return (c % GH) * GHD + c / GH; }

struct GnnIn {
    const float *kp[2], *sc[2], *d[2];
    int64_t sp[2], sr[2], sd[2];
    const int32_t *shape[2], *m_dev, *n_dev;
    int32_t B, M, N;
};

GnnAddr gnn_ws_addr(float *p, int P, int ld)
{
    GnnAddr a{};
    a.p[0] = p; a.ss[0] = (long long)P * ld; a.sr[0] = ld; a.sc[0] = 1;
    return a;
}

void gnn_linear(rcn_ctx *ctx, const GnnCounts &cnt, int sets, int P, const float *X1, int C1, const float *X2, int Cin, int Cout, const float *W,
                const float *b, bool relu, const GnnAddr &Y, const GnnAddr *R)
{
    LinArgs a{};
    a.cnt = cnt; a.X1 = X1; a.X2 = X2; a.P = P; a.C1 = C1; a.Cin = Cin; a.Cout = Cout; a.relu = relu;
    a.W = W; a.b = b; a.Y = Y;
    if (R) a.R = *R;
    const dim3 grid((unsigned)((P + LIN_P - 1) / LIN_P), (unsigned)((Cout + LIN_C - 1) / LIN_C), (unsigned)sets);
    k_gnn_linear<<<grid, 256, 0, ctx->stream>>>(a);
}

// with ctx->mu held and the arguments checked: mdesc of every pair into out0 [B][M][256], out1 [B][N][256]
int gnn_forward(rcn_ctx *ctx, const rcn_sg_net *net, const GnnIn &in, float *out0, float *out1)
{
    const int P = std::max(in.M, in.N);
    const size_t pair_bytes = (size_t)2 * P * WS_FLOATS * 4;
    size_t chunk = std::max<size_t>(1, GNN_WS_BYTES / pair_bytes);
    if (ctx->gnn_chunk_pairs > 0) chunk = (size_t)ctx->gnn_chunk_pairs;
    chunk = std::min(std::min(chunk, (size_t)GNN_SLICE), (size_t)in.B);
    RCN_HIP(ctx->gnn_ws.reserve(chunk * pair_bytes));
    const size_t S = 2 * chunk;
    float *x = ctx->gnn_ws.as<float>(), *qkv = x + S * P * GD, *o = qkv + S * P * 3 * GD, *msg = o + S * P * GD, *hid = msg + S * P * GD;
    const float *w = net->dev;
    for (int32_t b0 = 0; b0 < in.B; b0 += (int32_t)chunk) {
        const int sets = 2 * (int)std::min<size_t>(chunk, (size_t)(in.B - b0));
        const GnnCounts cnt{in.m_dev, in.n_dev, in.M, in.N, b0};
        Enc0Args e{};
        e.cnt = cnt;
        for (int sd = 0; sd < 2; ++sd) { e.kp[sd] = in.kp[sd]; e.sc[sd] = in.sc[sd]; e.shape[sd] = in.shape[sd]; }
        e.W = w + net->enc_w[0]; e.b = w + net->enc_b[0]; e.out = o; e.P = P;
        k_gnn_enc0<<<dim3((unsigned)((P + 7) / 8), (unsigned)sets), 256, 0, ctx->stream>>>(e);
        // 32 -> 64 -> 128 -> 256 through o, msg, o, msg; the last layer adds the descriptors and lands in x
        gnn_linear(ctx, cnt, sets, P, o, 32, nullptr, 32, 64, w + net->enc_w[1], w + net->enc_b[1], true, gnn_ws_addr(msg, P, 64), nullptr);
        gnn_linear(ctx, cnt, sets, P, msg, 64, nullptr, 64, 128, w + net->enc_w[2], w + net->enc_b[2], true, gnn_ws_addr(o, P, 128), nullptr);
        gnn_linear(ctx, cnt, sets, P, o, 128, nullptr, 128, 256, w + net->enc_w[3], w + net->enc_b[3], true, gnn_ws_addr(msg, P, 256), nullptr);
        GnnAddr desc{};
        for (int sd = 0; sd < 2; ++sd) { desc.p[sd] = const_cast<float *>(in.d[sd]); desc.ss[sd] = in.sp[sd]; desc.sr[sd] = in.sr[sd]; desc.sc[sd] = in.sd[sd]; }
        desc.by_pair = 1;
        const GnnAddr xa = gnn_ws_addr(x, P, GD);
        gnn_linear(ctx, cnt, sets, P, msg, 256, nullptr, 256, 256, w + net->enc_w[4], w + net->enc_b[4], false, xa, &desc);
        for (int l = 0; l < net->L; ++l) {
            gnn_linear(ctx, cnt, sets, P, x, GD, nullptr, GD, 3 * GD, w + net->qkv_w[l], w + net->qkv_b[l], false, gnn_ws_addr(qkv, P, 3 * GD), nullptr);
            AttArgs at{cnt, qkv, o, P, net->types[l]};
            k_gnn_attn<<<dim3((unsigned)((P + ATT_Q - 1) / ATT_Q), GH, (unsigned)sets), 256, 0, ctx->stream>>>(at);
            gnn_linear(ctx, cnt, sets, P, o, GD, nullptr, GD, GD, w + net->mrg_w[l], w + net->mrg_b[l], false, gnn_ws_addr(msg, P, GD), nullptr);
            gnn_linear(ctx, cnt, sets, P, x, GD, msg, 2 * GD, 2 * GD, w + net->m0_w[l], w + net->m0_b[l], true, gnn_ws_addr(hid, P, 2 * GD), nullptr);
            gnn_linear(ctx, cnt, sets, P, hid, 2 * GD, nullptr, 2 * GD, GD, w + net->m1_w[l], w + net->m1_b[l], false, xa, &xa);
        }
        GnnAddr out{};
        out.p[0] = out0; out.ss[0] = (long long)in.M * GD; out.p[1] = out1; out.ss[1] = (long long)in.N * GD;
        out.sr[0] = out.sr[1] = GD; out.sc[0] = out.sc[1] = 1;
        out.by_pair = 1;
        gnn_linear(ctx, cnt, sets, P, x, GD, nullptr, GD, GD, w + net->fin_w, w + net->fin_b, false, out, nullptr);
        RCN_HIP(hipGetLastError());
    }
    return RCN_OK;
}

bool gnn_check(rcn_ctx *ctx, const char *who, const rcn_sg_net *net, const GnnIn &in, int32_t D, int *rc)
{
    *rc = RCN_ERR_ARG;
    if (!net || net->ctx != ctx) return gnn_fail(ctx, who, "the net does not belong to this ctx");
    if (in.B < 0) return gnn_fail(ctx, who, "B < 0");
    if (in.M < 1 || in.N < 1) return gnn_fail(ctx, who, "M and N must be positive");
    if (in.M > RCN_SG_MAX_POINTS || in.N > RCN_SG_MAX_POINTS) {
        *rc = RCN_ERR_UNSUPPORTED;
        ctx->set_error(std::string(who) + ": M or N above " + std::to_string(RCN_SG_MAX_POINTS));
        return false;
    }
    if (D != GD) {
        *rc = RCN_ERR_UNSUPPORTED;
        ctx->set_error(std::string(who) + ": the network is built for descriptors of 256 channels");
        return false;
    }
    for (int sd = 0; sd < 2; ++sd)
        if (!in.kp[sd] || !in.sc[sd] || !in.d[sd]) return gnn_fail(ctx, who, "null pointer");
    if ((in.shape[0] == nullptr) != (in.shape[1] == nullptr)) return gnn_fail(ctx, who, "image shapes for one side only");
    return true;
}

}  // namespace

extern "C" int rcn_sg_net_create(rcn_ctx *ctx, const int32_t *layer_types, int32_t n_layers, const float *params_host, int64_t n_params,
                                 double bin_score, rcn_sg_net **net_out)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sg_net_create";
    if (!net_out) { gnn_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    *net_out = nullptr;
    if (n_layers < 0 || n_layers > 1024) { gnn_fail(ctx, who, "layer count outside 0..1024"); return RCN_ERR_ARG; }
    if (!params_host || (n_layers > 0 && !layer_types)) { gnn_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    for (int l = 0; l < n_layers; ++l)
        if (layer_types[l] != RCN_SG_LAYER_SELF && layer_types[l] != RCN_SG_LAYER_CROSS) { gnn_fail(ctx, who, "unknown layer type"); return RCN_ERR_ARG; }
    if (n_params != (int64_t)gnn_param_count(n_layers)) {
        ctx->set_error(std::string(who) + ": bad argument (" + std::to_string(n_layers) + " layers take " + std::to_string(gnn_param_count(n_layers)) + " parameters)");
        return RCN_ERR_ARG;
    }
    if (!std::isfinite(bin_score)) { gnn_fail(ctx, who, "bin_score is not finite"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    // repack: q, k, v of a layer as one [768][256] block, a head's channels contiguous (rows of Wq, Wk, Wv, columns of Wm),
    // Wq and bq times 1 / 8 (exact); everything else as it came
    std::vector<float> h(gnn_param_count(n_layers));
    rcn_sg_net *net = new rcn_sg_net;
    net->ctx = ctx; net->L = n_layers; net->bin_score = bin_score;
    net->types.assign(layer_types, layer_types + n_layers);
    const float *src = params_host;
    size_t at = 0;
    auto plain = [&](size_t n) { std::memcpy(h.data() + at, src, n * sizeof(float)); src += n; const size_t o = at; at += n; return o; };
    for (int i = 0; i < 5; ++i) { net->enc_w[i] = plain((size_t)ENC[i + 1] * ENC[i]); net->enc_b[i] = plain(ENC[i + 1]); }
    for (int l = 0; l < n_layers; ++l) {
        const size_t w0 = at, b0 = at + (size_t)3 * GD * GD;
        for (int j = 0; j < 3; ++j) {
            const float f = j == 0 ? 0.125f : 1.f;
            for (int c = 0; c < GD; ++c) {
                const int r = j * GD + gnn_perm(c);
                for (int k = 0; k < GD; ++k) h[w0 + (size_t)r * GD + k] = f * src[(size_t)c * GD + k];
                h[b0 + r] = f * src[(size_t)GD * GD + c];
            }
            src += (size_t)GD * GD + GD;
        }
        at = b0 + 3 * GD;
        net->qkv_w.push_back(w0); net->qkv_b.push_back(b0);
        const size_t mw = at;
        for (int r = 0; r < GD; ++r)
            for (int c = 0; c < GD; ++c) h[mw + (size_t)r * GD + gnn_perm(c)] = src[(size_t)r * GD + c];
        src += (size_t)GD * GD; at += (size_t)GD * GD;
        net->mrg_w.push_back(mw); net->mrg_b.push_back(plain(GD));
        net->m0_w.push_back(plain((size_t)2 * GD * 2 * GD)); net->m0_b.push_back(plain(2 * GD));
        net->m1_w.push_back(plain((size_t)GD * 2 * GD)); net->m1_b.push_back(plain(GD));
    }
    net->fin_w = plain((size_t)GD * GD); net->fin_b = plain(GD);
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

extern "C" void rcn_sg_net_destroy(rcn_sg_net *net)
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

extern "C" int rcn_sg_net_set_chunk_pairs(rcn_ctx *ctx, int32_t pairs)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->gnn_chunk_pairs = pairs > 0 ? pairs : 0;
    return RCN_OK;
}

extern "C" int rcn_sg_net_forward_device(rcn_ctx *ctx, const rcn_sg_net *net, const float *kpts0_dev, const float *scores0_dev, const float *d0_dev,
                                         int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0, const float *kpts1_dev, const float *scores1_dev,
                                         const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                                         const int32_t *shape0_dev, const int32_t *shape1_dev, const int32_t *m_dev, const int32_t *n_dev,
                                         int32_t B, int32_t M, int32_t N, int32_t D, float *mdesc0_out_dev, float *mdesc1_out_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sg_net_forward_device";
    const GnnIn in{{kpts0_dev, kpts1_dev}, {scores0_dev, scores1_dev}, {d0_dev, d1_dev}, {stride_pair0, stride_pair1}, {stride_row0, stride_row1},
                   {stride_d0, stride_d1}, {shape0_dev, shape1_dev}, m_dev, n_dev, B, M, N};
    int rc;
    if (!gnn_check(ctx, who, net, in, D, &rc)) return rc;
    if (!mdesc0_out_dev || !mdesc1_out_dev) { gnn_fail(ctx, who, "null pointer"); return RCN_ERR_ARG; }
    if (B == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    return gnn_forward(ctx, net, in, mdesc0_out_dev, mdesc1_out_dev);
}

extern "C" int rcn_sg_net_match_device(rcn_ctx *ctx, const rcn_sg_net *net, const float *kpts0_dev, const float *scores0_dev, const float *d0_dev,
                                       int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0, const float *kpts1_dev, const float *scores1_dev,
                                       const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                                       const int32_t *shape0_dev, const int32_t *shape1_dev, const int32_t *m_dev, const int32_t *n_dev,
                                       int32_t B, int32_t M, int32_t N, int32_t D, const rcn_sg_options *opt,
                                       int32_t *matches0_dev, int32_t *matches1_dev, float *mscores0_dev, float *mscores1_dev,
                                       int32_t *table_dev, int64_t table_stride, int32_t *counts_dev, float *logP_out_dev, int32_t *status_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const char *who = "rcn_sg_net_match_device";
    const GnnIn in{{kpts0_dev, kpts1_dev}, {scores0_dev, scores1_dev}, {d0_dev, d1_dev}, {stride_pair0, stride_pair1}, {stride_row0, stride_row1},
                   {stride_d0, stride_d1}, {shape0_dev, shape1_dev}, m_dev, n_dev, B, M, N};
    int rc;
    if (!gnn_check(ctx, who, net, in, D, &rc)) return rc;
    rcn_sg_options o;
    rcn_sg_default_options(&o);
    if (opt) o = *opt;
    o.alpha = net->bin_score;
    // the optimal-matching layer checks its own arguments before anything is launched
    if ((rc = rcn_int_sg_match(ctx, who, nullptr, 0, 0, 0, nullptr, 0, 0, 0, m_dev, n_dev, B, M, N, GD, &o, matches0_dev, matches1_dev, mscores0_dev,
                               mscores1_dev, table_dev, table_stride, counts_dev, logP_out_dev, status_dev, true)))
        return rc;
    if (B == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    const size_t n0 = (size_t)B * M * GD, n1 = (size_t)B * N * GD;
    RCN_HIP(ctx->gnn_mdesc.reserve((n0 + n1) * 4));
    float *md0 = ctx->gnn_mdesc.as<float>(), *md1 = md0 + n0;
    if ((rc = gnn_forward(ctx, net, in, md0, md1))) return rc;
    return rcn_int_sg_match(ctx, who, md0, (int64_t)M * GD, GD, 1, md1, (int64_t)N * GD, GD, 1, m_dev, n_dev, B, M, N, GD, &o, matches0_dev, matches1_dev,
                            mscores0_dev, mscores1_dev, table_dev, table_stride, counts_dev, logP_out_dev, status_dev, false);
}
