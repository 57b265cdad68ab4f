// tracks_key.h -- the (component root, image slot) keys of the track builder's conflict table, one text for the GPU
// kernels and the host sizing (tracks.hip) and for plain host C++ (tests/cpp/tracks_key_test.cpp).  No HIP header is needed: without a
// HIP compiler the qualifiers vanish.
//
// A node is a non-negative int32 (at most 2^31 - 2), an image slot is below 2^14 (rcn_match_lists_upload refuses more than 16384 list
// images), so (root << 14) | slot is below 2^45 and never the empty word.  The table is open addressing with linear probing over a
// power-of-two number of cells, at most half full: trk_table_cells(n) >= 2 n for the n items the host can bound, so a probe always ends.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TRK_FN __host__ __device__ inline
#else
#define TRK_FN inline
#endif

#define TRK_SLOT_BITS 14
#define TRK_MAX_SLOTS (1 << TRK_SLOT_BITS)
#define TRK_EMPTY (~0ull)
#define TRK_MIN_CELLS 64ull

TRK_FN unsigned long long trk_key(int32_t root, int32_t slot)
{
    return ((unsigned long long)(uint32_t)root << TRK_SLOT_BITS) | (unsigned long long)(uint32_t)slot;
}
TRK_FN int32_t trk_key_root(unsigned long long key) { return (int32_t)(key >> TRK_SLOT_BITS); }
TRK_FN int32_t trk_key_slot(unsigned long long key) { return (int32_t)(key & (TRK_MAX_SLOTS - 1)); }

// the finaliser of splitmix64: every input bit reaches every output bit, so consecutive roots do not cluster
TRK_FN unsigned long long trk_hash(unsigned long long key)
{
    key ^= key >> 30; key *= 0xbf58476d1ce4e5b9ull;
    key ^= key >> 27; key *= 0x94d049bb133111ebull;
    key ^= key >> 31;
    return key;
}

// cells of the table for at most n_items distinct keys: the smallest power of two >= max(2 n_items, TRK_MIN_CELLS)
TRK_FN unsigned long long trk_table_cells(unsigned long long n_items)
{
    unsigned long long c = TRK_MIN_CELLS;
    while (c < 2 * n_items) c <<= 1;
    return c;
}

TRK_FN unsigned long long trk_cell(unsigned long long key, unsigned long long cells) { return trk_hash(key) & (cells - 1); }
TRK_FN unsigned long long trk_next_cell(unsigned long long cell, unsigned long long cells) { return (cell + 1) & (cells - 1); }
