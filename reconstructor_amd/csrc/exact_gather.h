// Whole-row gather for the exact stages (included by match.hip; D % 4 == 0, D <= XG_ROWF).
//
// The exact re-rank reads random 1-KiB fp32 rows of a buffer far larger than the Infinity Cache, each row once.  The hardware does
// that at HBM speed only when a row is requested whole (one wave instruction = 64 lanes x 16 B = the row's 1 KiB, contiguous) and
// when enough such requests are in flight per CU to cover an HBM miss.  So a wave here owns a tile of XG_ROWS whole rows:
//   xg_issue   requests the XG_ROWS rows back to back, one global_load_dwordx4 of the whole wave per row, into registers;
//   xg_store   writes them to the wave's own LDS tile (nobody else reads it: no workgroup barrier anywhere);
//   xg_chain   is the canonical fp64 chain of DESIGN.md section 3 -- acc = fma(d, d, acc), d = (double)x[k] - (double)y[k],
//              k ascending from 0 to D - 1, from 0.0 -- of ONE lane over two rows of the tile.
// The caller issues the next tile's rows before it runs the chains of the present one (register double buffer), so a wave keeps
// XG_ROWS KiB in flight while it computes.  Few lanes own a chain (the arithmetic is a few per cent of the memory time).
//
// LDS image: row r is 1 KiB; its 16-byte chunk c sits at chunk position c ^ (r & 15).  A chain lane reads chunk c of its row with
// one ds_read_b128, which the LDS serves in groups of 16 lanes: 16 rows with distinct r & 15 touch 16 distinct chunk positions of
// the 256-byte bank line, and lanes that read the same row read the same address.  The store is a permutation inside each row.
#pragma once

#define XG_ROWS 24             // rows of a wave's tile
#define XG_ROWF 256            // floats per tile row
#define XG_TILEF (XG_ROWS * XG_ROWF)

// lane i (< XG_ROWS) holds row i's address in `ptr`, nullptr = no row: nothing is requested and the tile row keeps what it holds.
// Returns the mask of the rows requested, for xg_store.
__device__ __forceinline__ unsigned xg_issue(float4 (&v)[XG_ROWS], const float *ptr, int D)
{
    const int col = (threadIdx.x & 63) * 4;
    const unsigned long long pv = reinterpret_cast<unsigned long long>(ptr);
    const int lo = (int)(unsigned)pv, hi = (int)(unsigned)(pv >> 32);
#pragma unroll
    for (int i = 0; i < XG_ROWS; ++i) {
        const unsigned long long p = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, i) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, i);
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p && col < D) v[i] = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(p) + col);
    }
    return (unsigned)__ballot(ptr != nullptr) & ((1u << XG_ROWS) - 1u);
}

__device__ __forceinline__ void xg_store(float *tile, const float4 (&v)[XG_ROWS], unsigned rows)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < XG_ROWS; ++i)
        if (rows >> i & 1u) *reinterpret_cast<float4 *>(tile + i * XG_ROWF + ((lane ^ (i & 15)) << 2)) = v[i];
}

__device__ __forceinline__ double xg_chain(const float *tile, int xr, int yr, int D)
{
    const float *x = tile + xr * XG_ROWF, *y = tile + yr * XG_ROWF;
    const int sx = xr & 15, sy = yr & 15;
    double acc = 0.0;
#pragma unroll 4
    for (int c = 0; c < D / 4; ++c) {
        const float4 a = *reinterpret_cast<const float4 *>(x + ((c ^ sx) << 2));
        const float4 b = *reinterpret_cast<const float4 *>(y + ((c ^ sy) << 2));
        double d;
        d = (double)a.x - (double)b.x; acc = fma(d, d, acc);
        d = (double)a.y - (double)b.y; acc = fma(d, d, acc);
        d = (double)a.z - (double)b.z; acc = fma(d, d, acc);
        d = (double)a.w - (double)b.w; acc = fma(d, d, acc);
    }
    return acc;
}

// Entries for a device list, collected in LDS by one wave and appended with one atomic per XG_PEND_FLUSH or more of them: a tile
// holds few rows, and a single counter word takes only ~88 atomics per microsecond.
#define XG_PEND 64
#define XG_PEND_FLUSH (XG_PEND - XG_ROWS)
struct XgPend {
    unsigned long long e[XG_PEND];
    unsigned side[XG_PEND];
};
__device__ __forceinline__ void xg_pend_flush(XgPend &p, unsigned &np, unsigned long long *list, unsigned *count, unsigned *side)
{
    if (!np) return;
    const int lane = threadIdx.x & 63;
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(count, np);
    base = __builtin_amdgcn_readfirstlane(base);
    if ((unsigned)lane < np) {
        list[base + lane] = p.e[lane];
        if (side) side[base + lane] = p.side[lane];
    }
    np = 0;
}
// np is uniform over the wave; at most XG_ROWS lanes want
__device__ __forceinline__ void xg_pend_add(XgPend &p, unsigned &np, bool want, unsigned long long entry, unsigned side_value,
                                            unsigned long long *list, unsigned *count, unsigned *side)
{
    const unsigned long long m = __ballot(want);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    if (want) {
        const unsigned slot = np + __popcll(m & ((1ull << lane) - 1ull));
        p.e[slot] = entry;
        p.side[slot] = side_value;
    }
    np += (unsigned)__popcll(m);
    if (np > XG_PEND_FLUSH) xg_pend_flush(p, np, list, count, side);
}
