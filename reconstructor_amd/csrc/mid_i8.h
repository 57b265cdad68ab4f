// mid_i8.h -- the middle tier's sweep on the resident int8 rows (included by match.hip behind MidArgs).
//
// On the int8 path a row that leaves the re-rank carries an INTEGER threshold thr_acc (mid_thr_acc, match.hip: from the exact second
// candidate distance eb), and the rows of its train image that can be among its two nearest neighbours are exactly those with
//     acc(q, t) = hn[t] - qq.tq <= thr_acc,
// the number K1 computed: no fp32 rows are read, no error model is evaluated, and v_dot4_i32_i8 does four of the multiply-adds
// per lane operation where the fp32 sweep (k_mid_eval) spends two operations on one element.
//
// Work item = (train image bin, tile of MI8_TR train rows, slab of the bin's query rows).  The tile is STATIONARY IN REGISTERS:
// thread t holds rows t and t + 256 of the tile whole (2 x 64 VGPRs, de-swizzled on load) and their half-norms.  The bin's query rows
// stream past in batches of MI8_QB through LDS (de-swizzled there too; the next batch is fetched into registers while this one is
// computed); every thread reads the same query chunk at the same time -- a broadcast ds_read_b128 (4 LDS cycles) that feeds eight
// dot4 (32 VALU cycles), so the LDS pipe is a quarter busy with four waves per CU and half busy with eight.  A query's accumulator
// completes in one go: there is no per-query accumulator array and no limit of RCN_MIDQ rows per sweep.
// Rows without an integer threshold (tacc = 0) belong to k_mid_eval, which in turn skips the rows that have one.
// Padded train rows are zero with hn = RCN_I8_PAD_ACC and thr_acc < RCN_I8_PAD_ACC: they fail every test.
// The kernel returns at once unless fix_scale chose the int8 path for the resident set (ScaleDev::coarse_i8).
#pragma once

#define MI8_QB 32              // query rows per LDS batch (MI8_TR, the train rows per tile, and MI8_TILES: grid_plan.h -- the host plan sizes the grid by them)

__global__ __launch_bounds__(256, 2) void k_mid_eval_i8(MidArgs a)
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

    // a batch of query rows: eight threads per row, two chunks each
    const int qr = t >> 3, c0 = (t & 7) * 2;
    uint4 f0, f1;
    int fthr;
    auto fetch = [&](int b) {
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
                fthr = (int)ta;
            }
        }
    };
    auto stage = [&](int buf) {
        qs[buf][qr * 16 + c0] = f0;
        qs[buf][qr * 16 + c0 + 1] = f1;
        if ((t & 7) == 0) qthr[buf][qr] = fthr;
    };
    int b = (int)blockIdx.y, buf = 0;
    fetch(b);
    stage(0);
    __syncthreads();
    for (; b < nb; b += (int)gridDim.y, buf ^= 1) {
        const bool more = b + (int)gridDim.y < nb;
        if (more) fetch(b + (int)gridDim.y);
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
        if (more) stage(buf ^ 1);
        __syncthreads();
    }
}
