// coarse_i8.h -- K1 on int8 MFMA at D = 256 (included by match.hip behind k_coarse_top2).
//
// The int8 image of a row is 256 bytes = sixteen 16-byte chunks, swizzled like the fp16 image of a D = 128 row, and an int8
// MFMA lane fragment is 16 bytes like an fp16 one: in BYTES this kernel walks memory, LDS and registers exactly as
// k_coarse_top2<128> does (128-row tiles of 32 KB, the same ring, LDS-DMA, counted vmcnt and XCD item walk) with half
// the MFMAs per pair-distance of the fp16 kernel at D = 256.  What differs:
//   * v_mfma_i32_32x32x32_i8 (SH 0) / v_mfma_i32_16x16x64_i8 (SH 1): the accumulator is an EXACT integer,
//         acc(q, t) = hn[t] - qq.tq,   hn[t] = rint(s^2 |t|^2 / 2) + BIAS   (k_prepare_i8),
//     0 <= acc < 2^20 - 1 for every pair of resident rows (fix_scale caps s for that), padded rows have acc = 2^20 - 1;
//   * the key is (acc << 12) | train row: ONE v_lshl_or_b32 with the shift as an inline constant, no truncation; the keys
//     are folded four at a time (top2_fold.h), one key behind every MFMA of the 16x16x64 shape;
//   * query fragments are negated bytewise once per item (the grid is [-127, 127], so the negation cannot overflow).
//   * ONE half-norm image per ring buffer (512 bytes behind the tile), not one per wave: of the eight waves the one with
//     w == (tile number & 7) brings it with a single 16-byte-wide LDS-DMA on lanes 0..31, after its four tile pieces.  The issuer rotates
//     with the tile, so no wave is the straggler at every barrier.
//     The counted waits are vmcnt(2 NINST) / vmcnt(NINST), the same immediates for every wave, and they are never too small: a wave has
//     issued, behind the pieces of the tile it is about to read, NINST operations per later tile plus at most ONE half-norm piece (two
//     consecutive tiles have different issuers).  If that piece belongs to a later tile, the wave waits for one operation more than it
//     needs -- the oldest piece of the next tile, issued a whole tile of MFMAs ago; if it belongs to the tile about to be read, it is
//     older than the 2 NINST (NINST) youngest and the wait covers it.  The barrier behind the wait then orders every other wave's pieces,
//     the issuer's half-norm piece among them.  (hn holds Kp >= nT BT integers per image: the piece never reads past the image.)
//   * on the 16x16x64 shape every LDS read is  ds_read_b128 v, base offset:imm  (coarse_i8_addr.h): four fragment bases and one half-norm
//     base per lane, added to the ring buffer's address once per tile, row block and 16-row half in the immediate; and the four
//     reads that open row block rb + 1 of a tile (two half-norm quads, the first fragment of each half) are issued in the last k-step
//     of row block rb into registers of their own, so that only the first row block of a tile waits for LDS with nothing to do.
//     The reads are asm with an early-clobber result ("=&v", EXPERIMENTS.md section 4): the result lands when the data returns and must
//     never share a register with an address that a later read still uses.
// The kernel returns at once unless fix_scale chose the int8 path for the resident set (ScaleDev::coarse_i8).
#pragma once

#include "coarse_i8_addr.h"

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));


template <int V> struct I8Const { static constexpr int value = V; };

// ds_read_b128 with the row block's part of the address as the instruction's immediate; no s_waitcnt vmcnt(0) in front (asm)
template <unsigned IMM> __device__ __forceinline__ u32x4 lds_read_imm(unsigned base)
{
    static_assert(IMM < i8addr::OFFSET_LIMIT && IMM % 16 == 0, "offset field");
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(v) : "v"(base), "n"(IMM));
    return v;
}

// bytewise two's-complement negation of four int8 (no byte is -128)
__device__ __forceinline__ unsigned neg_i8x4(unsigned w)
{
    const unsigned x = ~w;
    return ((x & 0x7F7F7F7Fu) + 0x01010101u) ^ (x & 0x80808080u);
}

template <int ABL, int SH>
__global__ __launch_bounds__(512, 2) void k_coarse_top2_i8(CoarseArgs a)
{
    constexpr int ROWB = 256;                       // bytes per row
    constexpr int NCB = SH ? 4 : 2;                 // column (query) blocks per wave
    constexpr int CW = SH ? 16 : 32;                // their width
    constexpr int NKS = SH ? 4 : 8;                 // k-steps per tile row block (64 / 32 elements each)
    constexpr int CPK = SH ? 4 : 2;                 // 16-byte chunks of a row one k-step consumes
    constexpr int BT = RCN_I8_BT;
    constexpr int TILEB = BT * ROWB;
    constexpr int PIECE = 64 * 16;
    constexpr int NINST = TILEB / 8 / PIECE;         // tile pieces per wave
    constexpr int BUFB = i8addr::BUF_BYTES;          // tile + one half-norm image
    static_assert(ROWB == i8addr::ROW_BYTES && BT == i8addr::TILE_ROWS && BT * 4 == 32 * 16, "coarse_i8_addr.h describes another tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    if (!a.sc->coarse_i8) return;
    const int b = blockIdx.x;
    const int item = (b & 7) * a.items_per_xcd + (b >> 3);  // XCD x walks a contiguous item range
    if (item >= a.n_groups * a.tiles_per_pair) return;
    const int grp = item / a.tiles_per_pair, qt = item - grp * a.tiles_per_pair;
    const int2 g = a.groups[grp];
    const int p0 = g.x, R = g.y;
    if (R == 0) return;                                      // padding slot of the item order
    const ImgDev qi = a.imgs[a.pairs[2 * p0]];
    if (qt * RCN_QT >= qi.K) return;

    const int tid = threadIdx.x, lane = tid & 63;
    const int r = SH ? (lane & 15) : (lane & 31), h = SH ? (lane >> 4) : (lane >> 5);   // row / column in the block, k group
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    // query fragments, negated, resident for the whole item
    i32x4 bq[NCB][NKS];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int qrow = qt * RCN_QT + w * 64 + cb * CW + r;  // < Kp (Kp is a multiple of 512)
        const char *base = reinterpret_cast<const char *>(qi.f16) + (size_t)qrow * ROWB;
        const int sw = qrow & 15;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            uint4 v = *reinterpret_cast<const uint4 *>(base + (((ks * CPK + h) ^ sw) << 4));
            v.x = neg_i8x4(v.x); v.y = neg_i8x4(v.y); v.z = neg_i8x4(v.z); v.w = neg_i8x4(v.w);
            bq[cb][ks] = __builtin_bit_cast(i32x4, v);
        }
    }

    // per-pair train image records, read once with ordinary loads and parked in LDS: inside the
    // tile loop nothing but LDS-DMA may sit on the vector-memory queue (counted vmcnt)
    struct TrainRec { const char *img; const int *hn; int nT; int pad; };
    static_assert(sizeof(TrainRec) * RCN_GROUP <= RCN_TBL_BYTES, "train-record table does not fit its LDS slot");
    TrainRec *tbl = reinterpret_cast<TrainRec *>(smem + RCN_NBUF * BUFB);
    if (tid < R) {
        const ImgDev ti = a.imgs[a.pairs[2 * (p0 + tid) + 1]];
        TrainRec rec;
        rec.img = reinterpret_cast<const char *>(ti.f16);
        rec.hn = reinterpret_cast<const int *>(ti.hn);
        rec.nT = ti.K >= 2 ? (ti.K + BT - 1) / BT : 0;
        rec.pad = 0;
        tbl[tid] = rec;
    }
    __syncthreads();
    auto tiles_of = [&](int rr) -> int { return __builtin_amdgcn_readfirstlane(tbl[rr].nT); };

    // ---- staging cursor (runs RCN_PD tiles ahead of the compute cursor, across pairs)
    int s_pair = 0, s_tile = 0, s_nT = 0, staged = 0;
    const char *s_timg = nullptr;
    const int *s_hn = nullptr;
    auto s_seek = [&]() {   // move to the next pair that has tiles
        while (s_pair < R) {
            s_nT = tiles_of(s_pair);
            if (s_nT > 0) {
                const unsigned long long pf = reinterpret_cast<unsigned long long>(tbl[s_pair].img);
                const unsigned long long ph = reinterpret_cast<unsigned long long>(tbl[s_pair].hn);
                s_timg = reinterpret_cast<const char *>(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(pf >> 32)) << 32) |
                                                        (unsigned)__builtin_amdgcn_readfirstlane((unsigned)pf));
                s_hn = reinterpret_cast<const int *>(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(ph >> 32)) << 32) |
                                                     (unsigned)__builtin_amdgcn_readfirstlane((unsigned)ph));
                s_tile = 0;
                return;
            }
            ++s_pair;
        }
    };
    auto stage_next = [&]() {
        if (s_pair >= R) return;
        char *bbase = smem + (staged % RCN_NBUF) * BUFB;
#pragma unroll
        for (int i = 0; i < NINST; ++i) {
            const int off = (w * NINST + i) * PIECE;
            const char *src = s_timg + (size_t)s_tile * TILEB + off + lane * 16;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)(bbase + off), 16, 0, 0);
        }
        if (w == (staged & 7) && lane < 32)         // the tile's 128 half-norms, once for the workgroup
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)(s_hn + s_tile * BT + 4 * lane),
                (__attribute__((address_space(3))) void *)(bbase + TILEB), 16, 0, 0);
        ++staged;
        if (++s_tile == s_nT) { ++s_pair; s_seek(); }
    };
    s_seek();
#pragma unroll
    for (int i = 0; i < RCN_PD; ++i) stage_next();

    unsigned m1[NCB], m2[NCB];
    i32x16 pX0, pX1, pY0, pY1;          // SH 0: current / previous row block, two column blocks
    i32x4 qX[2][4], qY[2][4];           // SH 1: [16-row half][column block]
    auto top2 = [&](int cb, unsigned u) {
        if constexpr ((ABL & 1) != 0) return;
        // med3(m1,m2,u) spelled so that isel forms v_med3_u32 (scheduler sees a plain VALU op)
        const unsigned lo = min(m1[cb], m2[cb]), hi = max(m1[cb], m2[cb]);
        m2[cb] = max(lo, min(hi, u));
        m1[cb] = min(m1[cb], u);
    };
    // the shipping fold: four keys of a column block at a time, as in k_coarse_top2 (ABL 16 / 32 and LATE as there; on the 16x16 shape
    // that ships the two placements measure the same)
    constexpr bool LATE = ((ABL & 32) != 0) != (SH == 0);
    unsigned fk[NCB][3], fs[NCB];
    auto push = [&](int cb, int j, unsigned u) {
        if constexpr ((ABL & 1) != 0) return;
        if constexpr ((ABL & 16) != 0) { top2(cb, u); return; }
        if constexpr (LATE) {
            if ((j & 3) < 3) fk[cb][j & 3] = u;
            else top2_fold4(m1[cb], m2[cb], fk[cb][0], fk[cb][1], fk[cb][2], u);
            return;
        }
        switch (j & 3) {
        case 0: case 2: fk[cb][0] = u; break;
        case 1: fs[cb] = top2_fold_pair(m1[cb], fk[cb][0], u); break;
        default: m2[cb] = umin3(m2[cb], fs[cb], top2_fold_pair(m1[cb], fk[cb][0], u)); break;
        }
    };
    // the key of an accumulator: the shift is an inline constant, the row an SGPR or a literal -> one v_lshl_or_b32
    auto key = [&](int acc, unsigned idx) -> unsigned { return ((unsigned)acc << RCN_I8_IDX_BITS) | idx; };
    // LDS reads of the ring go through inline asm (see k_coarse_top2): no s_waitcnt vmcnt(0) in front of them
    auto lds_read = [&](unsigned addr) -> u32x4 {
        u32x4 v;
        asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
        return v;
    };
    // cur <- hn + A.B for row block (tile, rb); prev (row block before it) is folded into top-2
    auto step = [&](i32x16 &c0, i32x16 &c1, const i32x16 &p0v, const i32x16 &p1v, unsigned tile,
                    unsigned hnl, int rb, unsigned prev_rowbase) {
        if constexpr (SH == 0) {
        const int lrow = rb * 32 + r;
        const unsigned arow = tile + lrow * ROWB;
        const int sw = lrow & 15;
        u32x4 h0, h1, h2, h3, f0, f1;
        h0 = lds_read(hnl + (rb * 32 + 0 + 4 * h) * 4);
        h1 = lds_read(hnl + (rb * 32 + 8 + 4 * h) * 4);
        h2 = lds_read(hnl + (rb * 32 + 16 + 4 * h) * 4);
        h3 = lds_read(hnl + (rb * 32 + 24 + 4 * h) * 4);
        f0 = lds_read(arow + ((h ^ sw) << 4));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h0), "+v"(h1), "+v"(h2), "+v"(h3), "+v"(f0));
        i32x16 hnv;
        hnv[0] = (int)h0.x; hnv[1] = (int)h0.y; hnv[2] = (int)h0.z; hnv[3] = (int)h0.w;
        hnv[4] = (int)h1.x; hnv[5] = (int)h1.y; hnv[6] = (int)h1.z; hnv[7] = (int)h1.w;
        hnv[8] = (int)h2.x; hnv[9] = (int)h2.y; hnv[10] = (int)h2.z; hnv[11] = (int)h2.w;
        hnv[12] = (int)h3.x; hnv[13] = (int)h3.y; hnv[14] = (int)h3.z; hnv[15] = (int)h3.w;
        auto kstep = [&](int ks, u32x4 &cur, u32x4 &nxt) {
            // naming c1 ties the wait BEHIND the previous k-step's second MFMA
            if (ks > 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cur), "+v"(c1));
            // fragment of k-step ks+1 is in flight while ks computes
            if (ks + 1 < NKS) nxt = lds_read(arow + ((((ks + 1) * 2 + h) ^ sw) << 4));
            const i32x4 av = __builtin_bit_cast(i32x4, cur);
            c0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bq[0][ks], ks == 0 ? hnv : c0, 0, 0, 0);
#pragma unroll
            for (int reg = ks * 16 / NKS; reg < (ks + 1) * 16 / NKS; ++reg)
                push(0, reg, key(p0v[reg], prev_rowbase + (reg & 3) + 8 * (reg >> 2)));
            c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bq[1][ks], ks == 0 ? hnv : c1, 0, 0, 0);
#pragma unroll
            for (int reg = ks * 16 / NKS; reg < (ks + 1) * 16 / NKS; ++reg)
                push(1, reg, key(p1v[reg], prev_rowbase + (reg & 3) + 8 * (reg >> 2)));
        };
#pragma unroll
        for (int ks = 0; ks < NKS; ks += 2) {
            kstep(ks, f0, f1);
            kstep(ks + 1, f1, f0);
        }
        }
    };
    // SH 1.  cur <- hn + A.B for row block (tile, rb) as 2 halves x 4 column blocks of 16x16x64 MFMAs; the 32 values a
    // lane holds of the row block before it are folded into the top-2 between them.  Element (half s, block cb, reg)
    // is train row 16 s + 4 h + reg of the block: 16 s + reg goes into the packed index here, 4 h at the very end.
    // Addresses (coarse_i8_addr.h): fl[ks] / hl are the lane's constants, set once per item; fb[ks] / hb add the ring buffer's address once
    // per tile; the row block and the half are the read's immediate, so rb and ks are compile-time here (I8Const).
    // open[] holds the block's opening reads {hA, hB, f0a, f0b}: issued here behind the barrier for the first block of a tile, by the
    // last k-step of the block before for the others, which in turn issues the next block's into next[].
    unsigned fl[4], hl = 0, fb[4], hb = 0;
    if constexpr (SH == 1) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) fl[ks] = i8addr::frag_lane((unsigned)r, (unsigned)h, (unsigned)ks);
        hl = i8addr::hn_lane((unsigned)h);
        asm volatile("" : "+v"(fl[0]), "+v"(fl[1]), "+v"(fl[2]), "+v"(fl[3]), "+v"(hl));   // five resident registers, not recomputed per read
    }
    constexpr bool EARLY = RCN_I8_EARLY_OPEN != 0;
    auto step16 = [&](auto RB, i32x4 (&c)[2][4], i32x4 (&pv)[2][4], u32x4 (&open)[4], u32x4 (&next)[4], unsigned prev_rowbase) {
        if constexpr (SH == 1) {
            constexpr int rb = decltype(RB)::value;
            constexpr bool opened = EARLY && rb > 0;         // the block before issued open[]
            if constexpr (!opened) {
                open[0] = lds_read_imm<i8addr::hn_imm(rb, 0)>(hb);
                open[1] = lds_read_imm<i8addr::hn_imm(rb, 1)>(hb);
                open[2] = lds_read_imm<i8addr::frag_imm(rb, 0)>(fb[0]);
                open[3] = lds_read_imm<i8addr::frag_imm(rb, 1)>(fb[0]);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(open[0]), "+v"(open[1]), "+v"(open[2]), "+v"(open[3]));
            } else {
                // naming the block before's last accumulator ties the wait BEHIND its MFMAs
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(open[0]), "+v"(open[1]), "+v"(open[2]), "+v"(open[3]), "+v"(pv[1][3]));
            }
            i32x4 hn[2];
            hn[0] = __builtin_bit_cast(i32x4, open[0]);
            hn[1] = __builtin_bit_cast(i32x4, open[1]);
            u32x4 &f0a = open[2], &f0b = open[3];
            u32x4 f1a, f1b;
            constexpr int EPK = 32 / NKS;                    // previous-block elements folded per k-step
            auto kstep = [&](auto KS, u32x4 &ca_, u32x4 &cb_, u32x4 &na_, u32x4 &nb_) {
                constexpr int ks = decltype(KS)::value;
                // naming the last accumulator ties the wait BEHIND the previous k-step's MFMAs
                if constexpr (ks > 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ca_), "+v"(cb_), "+v"(c[1][3]));
                if constexpr (ks + 1 < NKS) {
                    na_ = lds_read_imm<i8addr::frag_imm(rb, 0)>(fb[(ks + 1) & 3]);
                    nb_ = lds_read_imm<i8addr::frag_imm(rb, 1)>(fb[(ks + 1) & 3]);
                } else if constexpr (EARLY && rb + 1 < BT / 32) {
                    next[0] = lds_read_imm<i8addr::hn_imm(rb + 1, 0)>(hb);
                    next[1] = lds_read_imm<i8addr::hn_imm(rb + 1, 1)>(hb);
                    next[2] = lds_read_imm<i8addr::frag_imm(rb + 1, 0)>(fb[0]);
                    next[3] = lds_read_imm<i8addr::frag_imm(rb + 1, 1)>(fb[0]);
                }
                const i32x4 av[2] = {__builtin_bit_cast(i32x4, ca_), __builtin_bit_cast(i32x4, cb_)};
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const int sh = m >> 2, cb = m & 3;
                    c[sh][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[sh], bq[cb][ks], ks == 0 ? hn[sh] : c[sh][cb], 0, 0, 0);
#pragma unroll
                    for (int e = ks * EPK + m * EPK / 8; e < ks * EPK + (m + 1) * EPK / 8; ++e) {
                        const int es = e >> 4, ecb = (e >> 2) & 3, er = e & 3;
                        push(ecb, er, key(pv[es][ecb][er], prev_rowbase + 16 * es + er));
                    }
                }
            };
            kstep(I8Const<0>{}, f0a, f0b, f1a, f1b);
            kstep(I8Const<1>{}, f1a, f1b, f0a, f0b);
            kstep(I8Const<2>{}, f0a, f0b, f1a, f1b);
            kstep(I8Const<3>{}, f1a, f1b, f0a, f0b);
        }
    };
    const unsigned smem_base = (unsigned)(size_t)(const __attribute__((address_space(3))) char *)smem;

    int done = 0;   // tiles computed so far (flat over the item's pairs)
    for (int rr = 0; rr < R; ++rr) {
        const int nT = tiles_of(rr);
        if (nT == 0) continue;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) m1[cb] = m2[cb] = 0xFFFFFFFFu;
        // "the row block before the first": accumulators of padded rows (their index wraps, the key still ranks behind every row)
        if constexpr (SH == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) { pY0[i] = RCN_I8_PAD_ACC; pY1[i] = RCN_I8_PAD_ACC; }
        } else {
#pragma unroll
            for (int i = 0; i < 32; ++i) qY[i >> 4][(i >> 2) & 3][i & 3] = RCN_I8_PAD_ACC;
        }
        for (int t = 0; t < nT; ++t, ++done) {
            stage_next();
            const int ahead = staged - done - 1;   // tiles issued after the one about to be read
            if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * NINST) : "memory");
            else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NINST) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const unsigned tile = smem_base + (done % RCN_NBUF) * BUFB;
            const unsigned base = (unsigned)(t * BT);
            if constexpr (SH == 0) {
                const unsigned hnl = tile + TILEB;
#pragma unroll
                for (int rb = 0; rb < BT / 32; rb += 2) {
                    step(pX0, pX1, pY0, pY1, tile, hnl, rb, base + 32u * rb - 32u);   // epilogue of the row block before (t, rb)
                    step(pY0, pY1, pX0, pX1, tile, hnl, rb + 1, base + 32u * rb);     // epilogue of (t, rb)
                }
            } else {
                static_assert(BT / 32 == 4, "four row blocks per tile are spelled out");
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) fb[ks] = tile + fl[ks];
                hb = tile + hl;
                u32x4 oA[4], oB[4];
                step16(I8Const<0>{}, qX, qY, oA, oB, base - 32u);
                step16(I8Const<1>{}, qY, qX, oB, oA, base);
                step16(I8Const<2>{}, qX, qY, oA, oB, base + 32u);
                step16(I8Const<3>{}, qY, qX, oB, oA, base + 64u);
            }
        }
        if (ABL & 1) {
            if constexpr (SH == 0) asm volatile("" ::"v"(pY0), "v"(pY1), "v"(pX0), "v"(pX1));
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i) asm volatile("" ::"v"(qY[i >> 2][i & 3]), "v"(qX[i >> 2][i & 3]));
            }
        }
        {   // drain: epilogue of the pair's last row block
            const unsigned rowbase = (unsigned)((nT - 1) * BT + BT - 32);
            if constexpr (SH == 0) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const unsigned idx = rowbase + (reg & 3) + 8 * (reg >> 2);
                    push(0, reg, key(pY0[reg], idx));
                    push(1, reg, key(pY1[reg], idx));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 32; ++e) {
                    const int es = e >> 4, ecb = (e >> 2) & 3, er = e & 3;
                    push(ecb, er, key(qY[es][ecb][er], rowbase + 16 * es + er));
                }
            }
        }
        if constexpr (SH == 0) {
            // lane l and l^32 hold the same query, disjoint train rows: merge, then lanes 0..31 store
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                unsigned a1 = m1[cb] | (unsigned)(4 * h), a2 = m2[cb] | (unsigned)(4 * h);
                if (m1[cb] == 0xFFFFFFFFu) a1 = 0xFFFFFFFFu;
                if (m2[cb] == 0xFFFFFFFFu) a2 = 0xFFFFFFFFu;
                unsigned b1 = __shfl_xor(a1, 32), b2 = __shfl_xor(a2, 32);
                unsigned r1 = min(a1, b1);
                unsigned r2 = min(max(a1, b1), min(a2, b2));
                const int qrow = qt * RCN_QT + w * 64 + cb * 32 + r;
                if (h == 0 && qrow < qi.K) a.cand[(size_t)(p0 + rr) * a.kq_stride + qrow] = make_uint2(r1, r2);
            }
        } else {
            // lanes l, l^16, l^32, l^48 hold the same query, disjoint train rows (4 h + reg of every 16): two merges
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
                const int qrow = qt * RCN_QT + w * 64 + cb * 16 + r;
                if (h == 0 && qrow < qi.K) a.cand[(size_t)(p0 + rr) * a.kq_stride + qrow] = make_uint2(a1, a2);
            }
        }
    }
}
