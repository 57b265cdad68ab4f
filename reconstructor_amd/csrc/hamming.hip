// hamming.hip -- brute-force 2-NN under the Hamming distance on 256-bit rows (ORB's packed descriptors), ratio test and
// uniqueness: cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) behind FeatureMatcher.cpp:53-64.
//
//   k_ham_expand   once per image: a packed 32-byte row becomes 256 int8 of +-1 (bit j % 8 of byte j / 8 is dimension j), sixteen 16-byte
//                  chunks, chunk c of row t stored at chunk c ^ (t & 15) -- the layout of the int8 coarse pass (coarse_i8_addr.h), so a tile
//                  is copied into LDS as it lies and every fragment read is one conflict-free ds_read_b128.  Rows past rows_i =
//                  clamp(counts[i], 0, K) are zero rows with a large bias; rows_i is read from device memory and stays there.
//   k_ham_top2     v_mfma_i32_16x16x64_i8 on (train tile) x (negated query fragments): with the row's bias as the accumulator's initial
//                  value, acc = bias - t.q = 256 - (256 - 2 d) = 2 d for a real row, exactly, and 1023 for a padded one.  The key is
//                  (acc << 22) | train row, folded four at a time (top2_fold.h): its two smallest ARE the two neighbours under (d, j).
//   k_ham_claim / k_ham_emit / k_ham_knn
//                  ratio test in fp32, atomic-min claim of a train row by the lowest passing query, the dense table and its counts;
//                  the raw (j0, d0, j1, d1) table.
// Tiles are staged with plain loads through registers into two LDS buffers (one barrier per tile), not by the LDS-DMA ring of the int8
// coarse kernel.  No grid-wide barrier, no spin.  Everything runs on ctx->stream.
#include "rcn_internal.h"
#include "top2_fold.h"
#include "coarse_i8_addr.h"

#include <algorithm>
#include <memory>

namespace {

constexpr int HAM_B = 32;                 // bytes per packed row
constexpr int HAM_ROWB = 256;             // bytes per expanded row
constexpr int HAM_MAX_K = 32768;
constexpr int HAM_KP_ALIGN = 256;         // padded rows per image: a multiple of the query tile (and so of the train tile)
constexpr int HAM_QT = 256;               // query rows per work item: 4 waves x 4 column blocks x 16
constexpr int HAM_BT = 64;                // train rows per tile
constexpr int HAM_TILEB = HAM_BT * HAM_ROWB;
constexpr int HAM_BUFB = HAM_TILEB + HAM_BT * 4;      // a tile and its 64 biases
constexpr int HAM_IDX_BITS = 22;
constexpr unsigned HAM_IDX_MASK = (1u << HAM_IDX_BITS) - 1;
constexpr int HAM_BIAS_REAL = 256;        // acc = 2 d
constexpr int HAM_BIAS_PAD = 1023;        // behind every real row (2 d <= 512), and the key stays below the empty key 0xFFFFFFFF
constexpr int HAM_ACC_MAX = 512;
constexpr int64_t HAM_MAX_CHUNK_ROWS = 1ll << 25;     // query-row slots of the top-2 workspace per chunk, at most (256 MiB)
static_assert(HAM_ROWB == (int)i8addr::ROW_BYTES, "the expanded row has the int8 coarse pass's layout");

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct HamImgDev {
    const char *x8;      // [Kp][256] int8 +-1, swizzled chunks; rows past rows[0] are zero
    const int32_t *bias; // [Kp] 256 for a real row, 1023 for a padded one
    const int32_t *rows; // [1]  clamp(counts, 0, K), written by k_ham_expand
    int32_t K, Kp;
};

// four bits -> four bytes, +1 where the bit is set and -1 where it is not
__device__ __forceinline__ unsigned ham_ex4(unsigned n)
{
    const unsigned s = (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21);
    return 0xFFFFFFFFu ^ (s * 0xFEu);
}

// bytewise negation of four int8 (no byte is -128)
__device__ __forceinline__ unsigned ham_neg4(unsigned w)
{
    const unsigned x = ~w;
    return ((x & 0x7F7F7F7Fu) + 0x01010101u) ^ (x & 0x80808080u);
}

// grid (Kp / 16, n images), 256 threads: thread (row of 16, chunk of 16)
__global__ __launch_bounds__(256) void k_ham_expand(const uint8_t *__restrict__ bytes, const int32_t *__restrict__ counts, int K, int Kp,
                                                    char *__restrict__ x8, int32_t *__restrict__ bias, int32_t *__restrict__ rows_out)
{
    const int img = blockIdx.y, row = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
    const int cnt = counts ? counts[img] : K;
    const int rows = min(max(cnt, 0), K);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < rows) {
        const uint8_t *src = bytes + ((size_t)img * K + row) * HAM_B + 2 * c;
        const unsigned b0 = src[0], b1 = src[1];
        v = make_uint4(ham_ex4(b0 & 15u), ham_ex4(b0 >> 4), ham_ex4(b1 & 15u), ham_ex4(b1 >> 4));
    }
    *reinterpret_cast<uint4 *>(x8 + ((size_t)img * Kp + row) * HAM_ROWB + ((c ^ (row & 15)) << 4)) = v;
    if (c == 0) bias[(size_t)img * Kp + row] = row < rows ? HAM_BIAS_REAL : HAM_BIAS_PAD;
    if (row == 0 && c == 0) rows_out[img] = rows;
}

struct HamTop2Args {
    const HamImgDev *imgs;
    const int2 *pairs;        // (query slot, train slot) of the chunk's pairs
    uint2 *cand;              // [n_pairs][kq_stride] the two smallest keys
    int n_pairs, tiles_per_pair, kq_stride, items_per_xcd;
};

// One work item = (pair, 256 query rows).  Wave w holds the negated fragments of query rows 64 w .. 64 w + 63 (four column blocks) in
// registers; the train image streams through LDS in tiles of 64 rows.  Lane (r, h): r = lane & 15 the query inside a column block / the
// train row inside a 16-row block for the A fragment, h = lane >> 4 the k group; accumulator element reg is train row 4 h + reg of the block.
__global__ __launch_bounds__(256) void k_ham_top2(HamTop2Args a)
{
    __shared__ __attribute__((aligned(16))) char smem[2 * HAM_BUFB];
    const int b = blockIdx.x;
    const int item = (b & 7) * a.items_per_xcd + (b >> 3);       // XCD x walks a contiguous item range
    if (item >= a.n_pairs * a.tiles_per_pair) return;
    const int p = item / a.tiles_per_pair, qt = item - p * a.tiles_per_pair;
    const int2 pr = a.pairs[p];
    const HamImgDev qi = a.imgs[pr.x], ti = a.imgs[pr.y];
    const int rows_q = *qi.rows, rows_t = *ti.rows;
    if (qt * HAM_QT >= rows_q) return;                           // uniform: the whole workgroup leaves in front of every barrier
    const int nT = (rows_t + HAM_BT - 1) / HAM_BT;               // <= Kp / 64

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, h = lane >> 4;

    i32x4 bq[4][4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const int qrow = qt * HAM_QT + w * 64 + cb * 16 + r;     // < Kp: Kp is a multiple of 256 and qt * 256 < rows_q <= Kp
        const char *base = qi.x8 + (size_t)qrow * HAM_ROWB;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 v = *reinterpret_cast<const uint4 *>(base + (((ks * 4 + h) ^ (qrow & 15)) << 4));
            v.x = ham_neg4(v.x); v.y = ham_neg4(v.y); v.z = ham_neg4(v.z); v.w = ham_neg4(v.w);
            bq[cb][ks] = __builtin_bit_cast(i32x4, v);
        }
    }

    unsigned m1[4], m2[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) m1[cb] = m2[cb] = 0xFFFFFFFFu;

    // Staging: every thread carries 64 bytes of the next tile (and a quarter of the threads' worth of its biases, read by all) in registers
    // while the current tile computes.  The last iteration fetches its own tile again instead of branching: a redundant park is harmless.
    uint4 st0, st1, st2, st3, sb;
    const int so = tid * 16, bo = (tid & 15) * 16;
#define HAM_FETCH(t)                                                                              \
    do {                                                                                          \
        const char *src_ = ti.x8 + (size_t)(t) * HAM_TILEB + so;      /* rows 64 t .. 64 t + 63 <= Kp - 1 */ \
        st0 = *reinterpret_cast<const uint4 *>(src_);                                             \
        st1 = *reinterpret_cast<const uint4 *>(src_ + 4096);                                      \
        st2 = *reinterpret_cast<const uint4 *>(src_ + 8192);                                      \
        st3 = *reinterpret_cast<const uint4 *>(src_ + 12288);                                     \
        sb = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(ti.bias + (t) * HAM_BT) + bo); \
    } while (0)
#define HAM_PARK(buf)                                                                             \
    do {                                                                                          \
        char *dst_ = smem + (buf) * HAM_BUFB;                                                     \
        *reinterpret_cast<uint4 *>(dst_ + so) = st0;                                              \
        *reinterpret_cast<uint4 *>(dst_ + so + 4096) = st1;                                       \
        *reinterpret_cast<uint4 *>(dst_ + so + 8192) = st2;                                       \
        *reinterpret_cast<uint4 *>(dst_ + so + 12288) = st3;                                      \
        if (tid < HAM_BT / 4) *reinterpret_cast<uint4 *>(dst_ + HAM_TILEB + bo) = sb;             \
    } while (0)
    if (nT > 0) { HAM_FETCH(0); HAM_PARK(0); }
    __syncthreads();
    for (int t = 0; t < nT; ++t) {
        const int tn = min(t + 1, nT - 1);
        HAM_FETCH(tn);                                           // in flight while tile t computes
        const char *tile = smem + (t & 1) * HAM_BUFB;
#pragma unroll
        for (int rb = 0; rb < HAM_BT / 16; ++rb) {
            const i32x4 hn = *reinterpret_cast<const i32x4 *>(tile + HAM_TILEB + (16 * rb + 4 * h) * 4);
            i32x4 c[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const i32x4 av = *reinterpret_cast<const i32x4 *>(tile + i8addr::frag_lane((unsigned)r, (unsigned)h, (unsigned)ks) + 16 * rb * HAM_ROWB);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
                    c[cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bq[cb][ks], ks == 0 ? hn : c[cb], 0, 0, 0);
            }
            const unsigned rowbase = (unsigned)(t * HAM_BT + 16 * rb);     // 4 h joins at the very end
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                top2_fold4(m1[cb], m2[cb], ((unsigned)c[cb][0] << HAM_IDX_BITS) | rowbase, ((unsigned)c[cb][1] << HAM_IDX_BITS) | (rowbase + 1u),
                           ((unsigned)c[cb][2] << HAM_IDX_BITS) | (rowbase + 2u), ((unsigned)c[cb][3] << HAM_IDX_BITS) | (rowbase + 3u));
        }
        HAM_PARK((t + 1) & 1);                                   // the buffer tile t - 1 was read from: everybody passed the barrier behind it
        __syncthreads();
    }
#undef HAM_FETCH
#undef HAM_PARK
    // lanes l, l ^ 16, l ^ 32, l ^ 48 hold the same query and disjoint train rows (4 h + reg of every 16): two merges
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        unsigned a1 = m1[cb] | (unsigned)(4 * h), a2 = m2[cb] | (unsigned)(4 * h);
        if (m1[cb] == 0xFFFFFFFFu) a1 = 0xFFFFFFFFu;
        if (m2[cb] == 0xFFFFFFFFu) a2 = 0xFFFFFFFFu;
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const unsigned b1 = __shfl_xor(a1, o), b2 = __shfl_xor(a2, o);
            const unsigned r1 = min(a1, b1);
            a2 = min(max(a1, b1), min(a2, b2));
            a1 = r1;
        }
        const int qrow = qt * HAM_QT + w * 64 + cb * 16 + r;
        if (h == 0 && qrow < qi.K) a.cand[(size_t)p * a.kq_stride + qrow] = make_uint2(a1, a2);      // K <= kq_stride
    }
}

// a key's neighbour: false when there is none (the empty key, or a padded row)
__device__ __forceinline__ bool ham_key(unsigned key, int &j, int &d)
{
    const unsigned acc = key >> HAM_IDX_BITS;
    j = (int)(key & HAM_IDX_MASK);
    d = (int)(acc >> 1);
    return acc <= (unsigned)HAM_ACC_MAX;
}

// FeatureMatcher.cpp:55: one fp32 product, one fp32 comparison
__device__ __forceinline__ bool ham_pass(uint2 c, float ratio, int &j0)
{
    int j1, d0, d1;
    if (!ham_key(c.x, j0, d0) || !ham_key(c.y, j1, d1)) return false;
    return (float)d0 < __fmul_rn(ratio, (float)d1);
}

// grid (pairs of the chunk, ceil(kq_stride / 256))
__global__ __launch_bounds__(256) void k_ham_claim(const HamImgDev *__restrict__ imgs, const int2 *__restrict__ pairs, const uint2 *__restrict__ cand,
                                                   int kq_stride, int kt_stride, float ratio, int32_t *__restrict__ owner)
{
    const int p = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
    const int rows_q = *imgs[pairs[p].x].rows;
    if (i >= rows_q) return;
    int j0;
    if (ham_pass(cand[(size_t)p * kq_stride + i], ratio, j0)) atomicMin(&owner[(size_t)p * kt_stride + j0], i);      // j0 < rows_t <= kt_stride
}

// one workgroup per pair of the chunk
__global__ __launch_bounds__(256) void k_ham_emit(const HamImgDev *__restrict__ imgs, const int2 *__restrict__ pairs, const uint2 *__restrict__ cand,
                                                  int kq_stride, int kt_stride, float ratio, const int32_t *__restrict__ owner,
                                                  int32_t *__restrict__ out, int64_t out_stride, int32_t *__restrict__ counts)
{
    __shared__ int total;
    const int p = blockIdx.x;
    const int rows_q = *imgs[pairs[p].x].rows;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int n = 0;
    for (int64_t i = threadIdx.x; i < out_stride; i += 256) {
        int v = -1, j0;
        if (i < rows_q && ham_pass(cand[(size_t)p * kq_stride + i], ratio, j0) && owner[(size_t)p * kt_stride + j0] == (int)i) { v = j0; ++n; }
        out[(size_t)p * out_stride + i] = v;
    }
    if (n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0) counts[p] = total;
}

// grid (pairs of the chunk, row blocks): (j0, d0, j1, d1) per query row, -1 where absent
__global__ __launch_bounds__(256) void k_ham_knn(const HamImgDev *__restrict__ imgs, const int2 *__restrict__ pairs, const uint2 *__restrict__ cand,
                                                 int kq_stride, int4 *__restrict__ knn, int64_t stride)
{
    const int p = blockIdx.x;
    const int rows_q = *imgs[pairs[p].x].rows;
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < stride; i += (int64_t)gridDim.y * 256) {
        int4 v = make_int4(-1, -1, -1, -1);
        if (i < rows_q) {
            const uint2 c = cand[(size_t)p * kq_stride + i];
            int j, d;
            if (ham_key(c.x, j, d)) { v.x = j; v.y = d; }
            if (ham_key(c.y, j, d)) { v.z = j; v.w = d; }
        }
        knn[(size_t)p * stride + i] = v;
    }
}

struct HamBlock {
    void *p = nullptr;
    ~HamBlock() { if (p) (void)hipFree(p); }
};

struct HamImg {
    std::shared_ptr<HamBlock> blk;      // one allocation per upload call, shared by the images of a batch
    HamImgDev dev;
};

}  // namespace

// The binary residency of a ctx: a set of its own beside the float descriptors of rcn_desc_* (same image ids).
struct HamState {
    std::map<int32_t, HamImg> images;
    bool table_dirty = true;
    std::map<int32_t, int32_t> slot_of;
    std::vector<HamImgDev> table_host;
    std::vector<int2> pairs_host;
    std::vector<int32_t> kq_host, kt_host;
    DevBuf table, pair_table, pairs, cand, owner, out_tmp, cnt_tmp, stage;
};

void rcn_int_ham_release(rcn_ctx *ctx)
{
    if (!ctx->ham) return;
    HamState *h = ctx->ham;
    for (DevBuf *b : {&h->table, &h->pair_table, &h->pairs, &h->cand, &h->owner, &h->out_tmp, &h->cnt_tmp, &h->stage}) b->release();
    delete h;
    ctx->ham = nullptr;
}

namespace {

HamState *ham_state(rcn_ctx *ctx)
{
    if (!ctx->ham) ctx->ham = new HamState();
    return ctx->ham;
}

int ham_check_shape(rcn_ctx *ctx, const char *who, int32_t K, int32_t n_bytes)
{
    if (n_bytes != HAM_B) { ctx->set_error(std::string(who) + ": rows of 32 bytes only (256 bits)"); return RCN_ERR_ARG; }
    if (K < 0 || K > HAM_MAX_K) { ctx->set_error(std::string(who) + ": between 0 and 32768 rows per image"); return RCN_ERR_ARG; }
    return RCN_OK;
}

// n images of K rows from bytes_dev [n][K][32] (counts_dev [n] or NULL) into one new block; out[i] is image i's record
int ham_ingest(rcn_ctx *ctx, const uint8_t *bytes_dev, const int32_t *counts_dev, int32_t n, int32_t K, std::vector<HamImg> &out)
{
    const int32_t Kp = std::max(HAM_KP_ALIGN, (K + HAM_KP_ALIGN - 1) / HAM_KP_ALIGN * HAM_KP_ALIGN);
    const size_t x8_bytes = (size_t)n * Kp * HAM_ROWB, bias_bytes = (size_t)n * Kp * 4, rows_bytes = ((size_t)n * 4 + 255) / 256 * 256;
    auto blk = std::make_shared<HamBlock>();
    RCN_HIP(hipMalloc(&blk->p, x8_bytes + bias_bytes + rows_bytes));
    char *x8 = static_cast<char *>(blk->p);
    int32_t *bias = reinterpret_cast<int32_t *>(x8 + x8_bytes);
    int32_t *rows = reinterpret_cast<int32_t *>(x8 + x8_bytes + bias_bytes);
    hipLaunchKernelGGL(k_ham_expand, dim3(Kp / 16, n), dim3(256), 0, ctx->stream, bytes_dev, counts_dev, K, Kp, x8, bias, rows);
    RCN_HIP(hipGetLastError());
    out.resize(n);
    for (int32_t i = 0; i < n; ++i) {
        out[i].blk = blk;
        out[i].dev = HamImgDev{x8 + (size_t)i * Kp * HAM_ROWB, bias + (size_t)i * Kp, rows + i, K, Kp};
    }
    return RCN_OK;
}

// the device image table of the resident set, slot = rank of the id
int ham_table(rcn_ctx *ctx, HamState *h)
{
    if (!h->table_dirty) return RCN_OK;
    h->slot_of.clear();
    h->table_host.clear();
    for (auto &kv : h->images) {
        h->slot_of[kv.first] = (int32_t)h->table_host.size();
        h->table_host.push_back(kv.second.dev);
    }
    if (!h->table_host.empty()) {
        RCN_HIP(h->table.reserve(h->table_host.size() * sizeof(HamImgDev)));
        RCN_HIP(hipMemcpyAsync(h->table.p, h->table_host.data(), h->table_host.size() * sizeof(HamImgDev), hipMemcpyHostToDevice, ctx->stream));
    }
    h->table_dirty = false;
    return RCN_OK;
}

// h->pairs_host (table slots) with h->kq_host / kt_host (row capacities) -> the match table and / or the knn table, chunk by chunk
int ham_run(rcn_ctx *ctx, HamState *h, const HamImgDev *table_dev, float ratio, int32_t *out_dev, int64_t out_stride, int32_t *counts_dev,
            int32_t *knn_dev, int64_t knn_stride)
{
    const int32_t n_pairs = (int32_t)h->pairs_host.size();
    if (n_pairs == 0) return RCN_OK;
    int32_t kq_stride = 1, kt_stride = 1;
    for (int32_t p = 0; p < n_pairs; ++p) { kq_stride = std::max(kq_stride, h->kq_host[p]); kt_stride = std::max(kt_stride, h->kt_host[p]); }
    const int64_t rows_cap = std::max<int64_t>(1, std::min<int64_t>(ctx->chunk_rows, HAM_MAX_CHUNK_ROWS));
    const int32_t chunk = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n_pairs, rows_cap / kq_stride));
    RCN_HIP(h->pairs.reserve((size_t)n_pairs * sizeof(int2)));
    RCN_HIP(h->cand.reserve((size_t)chunk * kq_stride * sizeof(uint2)));
    if (out_dev) RCN_HIP(h->owner.reserve((size_t)chunk * kt_stride * 4));
    RCN_HIP(hipMemcpyAsync(h->pairs.p, h->pairs_host.data(), (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
    const int tiles_per_pair = (kq_stride + HAM_QT - 1) / HAM_QT;
    for (int32_t p0 = 0; p0 < n_pairs; p0 += chunk) {
        const int32_t np = std::min(chunk, n_pairs - p0);
        const int2 *pairs = h->pairs.as<int2>() + p0;
        HamTop2Args a;
        a.imgs = table_dev;
        a.pairs = pairs;
        a.cand = h->cand.as<uint2>();
        a.n_pairs = np;
        a.tiles_per_pair = tiles_per_pair;
        a.kq_stride = kq_stride;
        const int64_t items = (int64_t)np * tiles_per_pair;
        a.items_per_xcd = (int)((items + 7) / 8);
        hipLaunchKernelGGL(k_ham_top2, dim3((unsigned)(a.items_per_xcd * 8)), dim3(256), 0, ctx->stream, a);
        RCN_HIP(hipGetLastError());
        if (out_dev) {
            RCN_HIP(hipMemsetAsync(h->owner.p, 0x7F, (size_t)np * kt_stride * 4, ctx->stream));
            hipLaunchKernelGGL(k_ham_claim, dim3(np, (kq_stride + 255) / 256), dim3(256), 0, ctx->stream, table_dev, pairs, h->cand.as<uint2>(),
                               kq_stride, kt_stride, ratio, h->owner.as<int32_t>());
            RCN_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_ham_emit, dim3(np), dim3(256), 0, ctx->stream, table_dev, pairs, h->cand.as<uint2>(), kq_stride, kt_stride, ratio,
                               h->owner.as<int32_t>(), out_dev + (size_t)p0 * out_stride, out_stride, counts_dev + p0);
            RCN_HIP(hipGetLastError());
        }
        if (knn_dev) {
            hipLaunchKernelGGL(k_ham_knn, dim3(np, (unsigned)std::min<int64_t>((knn_stride + 255) / 256, 1024)), dim3(256), 0, ctx->stream, table_dev, pairs, h->cand.as<uint2>(),
                               kq_stride, reinterpret_cast<int4 *>(knn_dev) + (size_t)p0 * knn_stride, knn_stride);
            RCN_HIP(hipGetLastError());
        }
    }
    return RCN_OK;
}

// the caller's pair list (image ids; NULL: every i < j over the resident ids) as table slots; stride >= K of every query image
int ham_plan(rcn_ctx *ctx, HamState *h, const char *who, const int32_t *pairs_host, int32_t n_pairs, int64_t stride)
{
    if (n_pairs < 0) { ctx->set_error(std::string(who) + ": negative pair count"); return RCN_ERR_ARG; }
    if (int rc = ham_table(ctx, h)) return rc;
    h->pairs_host.clear(); h->kq_host.clear(); h->kt_host.clear();
    const int32_t n = (int32_t)h->table_host.size();
    auto add = [&](int32_t qs, int32_t ts) -> int {
        if (h->table_host[qs].K > stride) { ctx->set_error(std::string(who) + ": the row stride is smaller than a query image"); return RCN_ERR_ARG; }
        h->pairs_host.push_back(make_int2(qs, ts));
        h->kq_host.push_back(h->table_host[qs].K);
        h->kt_host.push_back(h->table_host[ts].K);
        return RCN_OK;
    };
    if (!pairs_host) {
        if ((int64_t)n_pairs != (int64_t)n * (n - 1) / 2) { ctx->set_error(std::string(who) + ": without a pair list the count must be n (n - 1) / 2 of the resident binary images"); return RCN_ERR_ARG; }
        for (int32_t i = 0; i < n; ++i)
            for (int32_t j = i + 1; j < n; ++j)
                if (int rc = add(i, j)) return rc;
        return RCN_OK;
    }
    for (int32_t p = 0; p < n_pairs; ++p) {
        auto q = h->slot_of.find(pairs_host[2 * p]), t = h->slot_of.find(pairs_host[2 * p + 1]);
        if (q == h->slot_of.end() || t == h->slot_of.end()) { ctx->set_error(std::string(who) + ": image id without resident binary rows"); return RCN_ERR_NOT_FOUND; }
        if (int rc = add(q->second, t->second)) return rc;
    }
    return RCN_OK;
}

}  // namespace

extern "C" {

int rcn_bits_upload_batch_device(rcn_ctx *ctx, int32_t first_img_id, int32_t n_images, const uint8_t *bytes_dev, const int32_t *counts_dev,
                                 int32_t K, int32_t n_bytes)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = ham_check_shape(ctx, "rcn_bits_upload_batch_device", K, n_bytes)) return rc;
    if (n_images < 0 || (n_images > 0 && !bytes_dev)) { ctx->set_error("rcn_bits_upload_batch_device: null rows or a negative image count"); return RCN_ERR_ARG; }
    if (n_images > 65535) { ctx->set_error("rcn_bits_upload_batch_device: at most 65535 images per call"); return RCN_ERR_ARG; }
    if (n_images == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    HamState *h = ham_state(ctx);
    std::vector<HamImg> made;
    if (int rc = ham_ingest(ctx, bytes_dev, counts_dev, n_images, K, made)) return rc;
    for (int32_t i = 0; i < n_images; ++i) h->images[first_img_id + i] = made[i];
    h->table_dirty = true;
    return RCN_OK;
}

int rcn_bits_upload(rcn_ctx *ctx, int32_t img_id, const uint8_t *bytes_host, int32_t K, int32_t n_bytes)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = ham_check_shape(ctx, "rcn_bits_upload", K, n_bytes)) return rc;
    if (K > 0 && !bytes_host) { ctx->set_error("rcn_bits_upload: null rows"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    HamState *h = ham_state(ctx);
    RCN_HIP(h->stage.reserve((size_t)std::max(K, 1) * HAM_B));
    if (K > 0) RCN_HIP(hipMemcpyAsync(h->stage.p, bytes_host, (size_t)K * HAM_B, hipMemcpyHostToDevice, ctx->stream));
    std::vector<HamImg> made;
    if (int rc = ham_ingest(ctx, h->stage.as<uint8_t>(), nullptr, 1, K, made)) return rc;
    RCN_HIP(rcn_int_stream_wait(ctx));       // the host rows are borrowed for the call only, and the staging buffer is free again
    h->images[img_id] = made[0];
    h->table_dirty = true;
    return RCN_OK;
}

int rcn_bits_remove(rcn_ctx *ctx, int32_t img_id)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->ham) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(rcn_int_stream_wait(ctx));
    if (ctx->ham->images.erase(img_id)) ctx->ham->table_dirty = true;
    return RCN_OK;
}

int rcn_bits_clear(rcn_ctx *ctx)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->ham) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(rcn_int_stream_wait(ctx));
    ctx->ham->images.clear();
    ctx->ham->table_dirty = true;
    return RCN_OK;
}

int rcn_bits_count(const rcn_ctx *ctx)
{
    if (!ctx) return RCN_ERR_ARG;
    return ctx->ham ? (int)ctx->ham->images.size() : 0;
}

int rcn_match_grid_hamming_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio, int32_t *out_dev, int64_t out_stride,
                                  int32_t *counts_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (n_pairs > 0 && (!out_dev || !counts_dev)) { ctx->set_error("rcn_match_grid_hamming_device: null output"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    HamState *h = ham_state(ctx);
    if (int rc = ham_plan(ctx, h, "rcn_match_grid_hamming_device", pairs_host, n_pairs, out_stride)) return rc;
    return ham_run(ctx, h, h->table.as<HamImgDev>(), ratio, out_dev, out_stride, counts_dev, nullptr, 0);
}

int rcn_match_grid_hamming(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio, int32_t *out_host, int64_t out_stride,
                           int32_t *counts_host)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (n_pairs > 0 && (!out_host || !counts_host)) { ctx->set_error("rcn_match_grid_hamming: null output"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    HamState *h = ham_state(ctx);
    if (int rc = ham_plan(ctx, h, "rcn_match_grid_hamming", pairs_host, n_pairs, out_stride)) return rc;
    if (n_pairs == 0) return RCN_OK;
    const size_t table_bytes = (size_t)n_pairs * out_stride * 4;
    RCN_HIP(h->out_tmp.reserve(table_bytes));
    RCN_HIP(h->cnt_tmp.reserve((size_t)n_pairs * 4));
    if (int rc = ham_run(ctx, h, h->table.as<HamImgDev>(), ratio, h->out_tmp.as<int32_t>(), out_stride, h->cnt_tmp.as<int32_t>(), nullptr, 0)) return rc;
    RCN_HIP(hipMemcpyAsync(out_host, h->out_tmp.p, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RCN_HIP(hipMemcpyAsync(counts_host, h->cnt_tmp.p, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
    RCN_HIP(rcn_int_stream_wait(ctx));
    return RCN_OK;
}

int rcn_hamming_knn2_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, int32_t *knn_dev, int64_t stride)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (n_pairs > 0 && !knn_dev) { ctx->set_error("rcn_hamming_knn2_device: null output"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    HamState *h = ham_state(ctx);
    if (int rc = ham_plan(ctx, h, "rcn_hamming_knn2_device", pairs_host, n_pairs, stride)) return rc;
    return ham_run(ctx, h, h->table.as<HamImgDev>(), 0.0f, nullptr, 0, nullptr, knn_dev, stride);
}

int rcn_match_pair_hamming(rcn_ctx *ctx, const uint8_t *q_host, int32_t K1, const uint8_t *t_host, int32_t K2, int32_t n_bytes, float ratio,
                           int32_t *out_train_for_query, int32_t *out_count)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = ham_check_shape(ctx, "rcn_match_pair_hamming", K1, n_bytes)) return rc;
    if (int rc = ham_check_shape(ctx, "rcn_match_pair_hamming", K2, n_bytes)) return rc;
    if ((K1 > 0 && (!q_host || !out_train_for_query)) || (K2 > 0 && !t_host) || !out_count) { ctx->set_error("rcn_match_pair_hamming: null pointer"); return RCN_ERR_ARG; }
    *out_count = 0;
    if (K1 == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    HamState *h = ham_state(ctx);
    const size_t qb = (size_t)K1 * HAM_B, tb = (size_t)std::max(K2, 1) * HAM_B;
    RCN_HIP(h->stage.reserve(qb + tb));
    RCN_HIP(hipMemcpyAsync(h->stage.p, q_host, qb, hipMemcpyHostToDevice, ctx->stream));
    if (K2 > 0) RCN_HIP(hipMemcpyAsync(h->stage.as<char>() + qb, t_host, (size_t)K2 * HAM_B, hipMemcpyHostToDevice, ctx->stream));
    std::vector<HamImg> q, t;
    if (int rc = ham_ingest(ctx, h->stage.as<uint8_t>(), nullptr, 1, K1, q)) return rc;
    if (int rc = ham_ingest(ctx, h->stage.as<uint8_t>() + qb, nullptr, 1, K2, t)) return rc;
    const HamImgDev two[2] = {q[0].dev, t[0].dev};
    RCN_HIP(h->pair_table.reserve(sizeof(two)));
    RCN_HIP(hipMemcpyAsync(h->pair_table.p, two, sizeof(two), hipMemcpyHostToDevice, ctx->stream));
    h->pairs_host.assign(1, make_int2(0, 1));
    h->kq_host.assign(1, K1);
    h->kt_host.assign(1, K2);
    RCN_HIP(h->out_tmp.reserve(qb));
    RCN_HIP(h->cnt_tmp.reserve(4));
    if (int rc = ham_run(ctx, h, h->pair_table.as<HamImgDev>(), ratio, h->out_tmp.as<int32_t>(), K1, h->cnt_tmp.as<int32_t>(), nullptr, 0)) return rc;
    RCN_HIP(hipMemcpyAsync(out_train_for_query, h->out_tmp.p, (size_t)K1 * 4, hipMemcpyDeviceToHost, ctx->stream));
    RCN_HIP(hipMemcpyAsync(out_count, h->cnt_tmp.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    RCN_HIP(rcn_int_stream_wait(ctx));       // ... and the two temporary images may go
    return RCN_OK;
}

}  // extern "C"
