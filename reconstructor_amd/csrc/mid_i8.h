// mid_i8.h -- the middle tier's sweep on the resident int8 rows (included by match.hip behind MidArgs).
//
// On the int8 path a row that leaves the re-rank carries an INTEGER threshold thr_acc (mid_thr_acc, match.hip: from the exact second
// candidate distance eb), and the rows of its train image that can be among its two nearest neighbours are exactly those with
//     acc(q, t) = hn[t] - qq.tq <= thr_acc,
// the number K1 computed: no fp32 rows are read and no error model is evaluated.  k_mid_eval_i8 computes it as K1 does, on
// v_mfma_i32_16x16x64_i8 with the train rows as A, the bytewise NEGATED query rows (neg_i8x4) as B and the half-norms as C: the accumulator
// is that exact int32, so the emitted rows are those of the dot4 form (k_mid_eval_i8_dot4 below, diagnostic build, RCN_MID_I8_MFMA=0).
//
// Work item = (train image bin, tile of MI8_TR train rows, slab of the bin's query rows).  The tile is STATIONARY IN REGISTERS: each of
// the four waves holds 128 of its rows as A fragments (8 row blocks x 4 k-steps x 4 VGPRs = 128 VGPRs, loaded straight from the swizzled
// image) and their half-norms as C operands (8 x 4 VGPRs).  The bin's query rows stream past in batches of MI8_QB = 32 (two column blocks)
// through LDS, negated at staging, chunk c of slot s at c ^ (s & 15) (exact_gather.h's layout: the B-fragment ds_read_b128s are
// conflict-free); the next batch is fetched into registers while this one is computed, plain __syncthreads() double buffering.  Per batch
// a wave issues 8 ds_read_b128 and 64 MFMAs and compares every accumulator with its query's threshold (held per lane, one per column
// block); a batch without a thresholded row is skipped.  Index arithmetic: mid_i8_addr.h.
// Rows without an integer threshold (tacc = 0) belong to k_mid_eval, which in turn skips the rows that have one.
// Padded train rows are zero with hn = RCN_I8_PAD_ACC and thr_acc < RCN_I8_PAD_ACC: they fail every test.  Kp is a multiple of RCN_QT, hence
// of MI8_TR: a tile that starts below Kp lies below it whole.
// The kernel returns at once unless fix_scale chose the int8 path for the resident set (ScaleDev::coarse_i8).
// Registers (hipcc, gfx950): 256 VGPRs (160 of them the stationary tile), no AGPRs, no scratch, 16.6 KB of LDS -- two waves per SIMD, two
// workgroups per CU, the occupancy of the dot4 form (214 VGPRs) and what __launch_bounds__(256, 2) asks for.
#pragma once
#include "mid_i8_addr.h"

#define MI8_QB 32              // query rows per LDS batch (MI8_TR, the train rows per tile, and MI8_TILES: grid_plan.h -- the host plan sizes the grid by them)
static_assert(MI8_QB == (int)mi8addr::BATCH_ROWS && MI8_TR == (int)mi8addr::TILE_ROWS && RCN_QT % MI8_TR == 0, "mid_i8_addr.h describes this tile");

// a batch of query rows, shared by both forms of the sweep: eight threads per row, two chunks each.  NEG: bytes negated (the MFMA form's B operand);
// SWZ: chunk c of slot s stored at c ^ (s & 15), else in logical order
template <bool NEG, bool SWZ> struct Mi8Batch {
    uint4 f0, f1;
    int fthr;
    __device__ __forceinline__ void fetch(const MidArgs &a, unsigned first, unsigned h, int b)
    {
        const int t = threadIdx.x, qr = t >> 3, c0 = (t & 7) * 2;
        const unsigned i = (unsigned)b * MI8_QB + (unsigned)qr;
        f0 = make_uint4(0u, 0u, 0u, 0u); f1 = f0; fthr = -1;
        if (i < h) {
            const unsigned ta = a.tacc[first + i];
            if (ta) {
                const unsigned long long e = a.sorted[first + i];
                const int pair = (int)(e >> 32), q = (int)(e & 0xFFFFFFFFu);
                const char *row = reinterpret_cast<const char *>(a.imgs[a.pairs[2 * pair]].f16) + (size_t)q * 256;
                f0 = *reinterpret_cast<const uint4 *>(row + ((c0 ^ (q & 15)) << 4));
                f1 = *reinterpret_cast<const uint4 *>(row + (((c0 + 1) ^ (q & 15)) << 4));
                if (NEG) {
                    f0.x = neg_i8x4(f0.x); f0.y = neg_i8x4(f0.y); f0.z = neg_i8x4(f0.z); f0.w = neg_i8x4(f0.w);
                    f1.x = neg_i8x4(f1.x); f1.y = neg_i8x4(f1.y); f1.z = neg_i8x4(f1.z); f1.w = neg_i8x4(f1.w);
                }
                fthr = (int)ta;
            }
        }
    }
    __device__ __forceinline__ void stage(uint4 *qs, int *qthr) const
    {
        const int t = threadIdx.x, qr = t >> 3, c0 = (t & 7) * 2;
        if (SWZ) {
            qs[mi8addr::q_off((unsigned)qr, (unsigned)c0) >> 4] = f0;
            qs[mi8addr::q_off((unsigned)qr, (unsigned)c0 + 1u) >> 4] = f1;
        } else {
            qs[qr * 16 + c0] = f0;
            qs[qr * 16 + c0 + 1] = f1;
        }
        if ((t & 7) == 0) qthr[qr] = fthr;
    }
};

__global__ __launch_bounds__(256, 2) void k_mid_eval_i8(MidArgs a)
{
    __shared__ uint4 qs[2][MI8_QB * 16];
    __shared__ int qthr[2][MI8_QB];
    if (!a.sc->coarse_i8) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 15, h4 = lane >> 4;
    const int bin = blockIdx.x / MI8_TILES, tile = blockIdx.x - bin * MI8_TILES;
    const unsigned first = a.offs[bin], h = a.offs[bin + 1] - first;
    const int nb = (int)((h + MI8_QB - 1) / MI8_QB);                 // batches of the bin
    if ((int)blockIdx.y >= nb) return;                               // (also: a bin without rows)
    const ImgDev ti = a.imgs[bin];
    if (tile * MI8_TR >= ti.Kp) return;

    // the wave's 128 rows as A fragments, their half-norms as C operands (accumulator element reg = row 4 h + reg of the block)
    i32x4 av[8][4], hnv[8];
    {
        const char *tb = reinterpret_cast<const char *>(ti.f16) + (size_t)tile * MI8_TR * 256;
        const int *hb = reinterpret_cast<const int *>(ti.hn) + tile * MI8_TR;
#pragma unroll
        for (int rb = 0; rb < 8; ++rb) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                av[rb][ks] = *reinterpret_cast<const i32x4 *>(tb + mi8addr::a_off((unsigned)w, (unsigned)rb, (unsigned)r, (unsigned)h4, (unsigned)ks));
            const int *hp = hb + mi8addr::tile_row((unsigned)w, (unsigned)rb, 4u * (unsigned)h4);
            hnv[rb] = i32x4{hp[0], hp[1], hp[2], hp[3]};
        }
    }
    const int row0 = tile * MI8_TR + (int)mi8addr::tile_row((unsigned)w, 0u, 4u * (unsigned)h4);      // + 16 rb + reg

    Mi8Batch<true, true> f;
    int b = (int)blockIdx.y, buf = 0;
    f.fetch(a, first, h, b);
    f.stage(qs[0], qthr[0]);
    __syncthreads();
    for (; b < nb; b += (int)gridDim.y, buf ^= 1) {
        const bool more = b + (int)gridDim.y < nb;
        if (more) f.fetch(a, first, h, b + (int)gridDim.y);
        int thr[2];                                                  // the thresholds of the lane's two queries; none: no accumulator is that small
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int v = qthr[buf][16 * cb + r];
            thr[cb] = v < 0 ? (int)0x80000000 : v;
        }
        if (__ballot(thr[0] != (int)0x80000000 || thr[1] != (int)0x80000000)) {      // the same verdict in all four waves
            i32x4 bq[2][4];
            const char *qb = reinterpret_cast<const char *>(qs[buf]);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    bq[cb][ks] = *reinterpret_cast<const i32x4 *>(qb + mi8addr::b_off((unsigned)cb, (unsigned)r, (unsigned)h4, (unsigned)ks));
            const unsigned slot0 = first + (unsigned)b * MI8_QB + (unsigned)r;        // + 16 cb
#pragma unroll
            for (int rp = 0; rp < 4; ++rp) {                         // two row blocks x two column blocks: four independent MFMA chains
                i32x4 c[2][2];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int cb = 0; cb < 2; ++cb)
                            c[i][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[2 * rp + i][ks], bq[cb][ks], ks == 0 ? hnv[2 * rp + i] : c[i][cb], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        const i32x4 v = c[i][cb];
                        if (min(min(v[0], v[1]), min(v[2], v[3])) > thr[cb]) continue;
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int j = row0 + 16 * (2 * rp + i) + reg;
                            if (v[reg] <= thr[cb] && j < ti.K) {
                                const unsigned slot = slot0 + 16u * (unsigned)cb;
                                const unsigned pos = atomicAdd(a.ccount + slot, 1u);
                                if (pos < (unsigned)RCN_MIDCAP) a.clist[(size_t)slot * RCN_MIDCAP + pos] = j;
                            }
                        }
                    }
            }
        }
        if (more) f.stage(qs[buf ^ 1], qthr[buf ^ 1]);
        __syncthreads();
    }
}

#ifdef RCN_DIAG
// The sweep on v_dot4_i32_i8, the form before the MFMA one and its differential reference (RCN_MID_I8_MFMA=0): thread t holds rows t and
// t + 256 of the tile whole (2 x 64 VGPRs, de-swizzled on load); every thread reads the same query chunk at the same time, a broadcast
// ds_read_b128 that feeds eight dot4.
__global__ __launch_bounds__(256, 2) void k_mid_eval_i8_dot4(MidArgs a)
{
    __shared__ uint4 qs[2][MI8_QB * 16];
    __shared__ int qthr[2][MI8_QB];
    if (!a.sc->coarse_i8) return;
    const int t = threadIdx.x;
    const int bin = blockIdx.x / MI8_TILES, tile = blockIdx.x - bin * MI8_TILES;
    const unsigned first = a.offs[bin], h = a.offs[bin + 1] - first;
    const int nb = (int)((h + MI8_QB - 1) / MI8_QB);                 // batches of the bin
    if ((int)blockIdx.y >= nb) return;                               // (also: a bin without rows)
    const ImgDev ti = a.imgs[bin];
    if (tile * MI8_TR >= ti.Kp) return;

    // the tile: two whole rows per thread, chunks in logical order
    unsigned tr[2][64];
    int hn[2], jrow[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = tile * MI8_TR + k * 256 + t;
        jrow[k] = j;
        const bool in = j < ti.Kp;
        hn[k] = in ? reinterpret_cast<const int *>(ti.hn)[j] : RCN_I8_PAD_ACC;
        const char *row = reinterpret_cast<const char *>(ti.f16) + (size_t)(in ? j : 0) * 256;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (in) v = *reinterpret_cast<const uint4 *>(row + ((c ^ (j & 15)) << 4));
            tr[k][4 * c] = v.x; tr[k][4 * c + 1] = v.y; tr[k][4 * c + 2] = v.z; tr[k][4 * c + 3] = v.w;
        }
    }

    Mi8Batch<false, false> f;
    int b = (int)blockIdx.y, buf = 0;
    f.fetch(a, first, h, b);
    f.stage(qs[0], qthr[0]);
    __syncthreads();
    for (; b < nb; b += (int)gridDim.y, buf ^= 1) {
        const bool more = b + (int)gridDim.y < nb;
        if (more) f.fetch(a, first, h, b + (int)gridDim.y);
        for (int r = 0; r < MI8_QB; ++r) {
            const int thr = __builtin_amdgcn_readfirstlane(qthr[buf][r]);
            if (thr < 0) continue;                                   // no such row, or a row of k_mid_eval's
            int d0 = 0, d1 = 0;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const uint4 x = qs[buf][r * 16 + c];                 // one address for the whole workgroup: a broadcast
                d0 = __builtin_amdgcn_sdot4((int)x.x, (int)tr[0][4 * c], d0, false);
                d1 = __builtin_amdgcn_sdot4((int)x.x, (int)tr[1][4 * c], d1, false);
                d0 = __builtin_amdgcn_sdot4((int)x.y, (int)tr[0][4 * c + 1], d0, false);
                d1 = __builtin_amdgcn_sdot4((int)x.y, (int)tr[1][4 * c + 1], d1, false);
                d0 = __builtin_amdgcn_sdot4((int)x.z, (int)tr[0][4 * c + 2], d0, false);
                d1 = __builtin_amdgcn_sdot4((int)x.z, (int)tr[1][4 * c + 2], d1, false);
                d0 = __builtin_amdgcn_sdot4((int)x.w, (int)tr[0][4 * c + 3], d0, false);
                d1 = __builtin_amdgcn_sdot4((int)x.w, (int)tr[1][4 * c + 3], d1, false);
            }
            const unsigned slot = first + (unsigned)b * MI8_QB + (unsigned)r;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int acc = hn[k] - (k ? d1 : d0);
                if (acc <= thr && jrow[k] < ti.K) {
                    const unsigned pos = atomicAdd(a.ccount + slot, 1u);
                    if (pos < (unsigned)RCN_MIDCAP) a.clist[(size_t)slot * RCN_MIDCAP + pos] = jrow[k];
                }
            }
        }
        if (more) f.stage(qs[buf ^ 1], qthr[buf ^ 1]);
        __syncthreads();
    }
}
#endif
