// coarse_i8_addr.h -- LDS addresses of k_coarse_top2_i8's 16x16x64 shape (coarse_i8.h), split into what changes when.
//
// A ring buffer holds a 128-row tile (256 bytes per row, sixteen 16-byte chunks, chunk c of row t stored at chunk c ^ (t & 15)) and,
// behind it, the tile's 128 integer half-norms.  Lane (r, h) of a wave -- r = lane & 15 the row inside a 16-row half, h = lane >> 4
// the k group -- reads for row block rb (32 rows), half (16 rows) and k-step ks
//     fragment:   buffer + (32 rb + 16 half + r) * 256 + (((4 ks + h) ^ r) << 4)          (the row's swizzle is r: 32 rb + 16 half is a multiple of 16)
//     half-norms: buffer + TILE_BYTES + (32 rb + 16 half + 4 h) * 4                        (rows 4 h .. 4 h + 3 of the half: the lane's accumulator rows)
// Only `buffer` changes from tile to tile, rb and half are compile-time inside the unrolled tile: each address is
//     (buffer + a per-lane constant)  +  an immediate of the ds_read's 16-bit offset field,
// five per-lane constants in all (one per k-step, one for the half-norms), added to the buffer's address once per tile.
// Plain integer functions, no HIP types: tests/cpp/coarse_i8_addr_test.cpp checks them against the formulas above on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RCN_I8A_FN __host__ __device__ constexpr
#else
#define RCN_I8A_FN constexpr
#endif

namespace i8addr {

constexpr unsigned ROW_BYTES = 256;                         // an int8 row
constexpr unsigned TILE_ROWS = 128;                         // RCN_I8_BT
constexpr unsigned TILE_BYTES = TILE_ROWS * ROW_BYTES;
constexpr unsigned HN_BYTES = TILE_ROWS * 4;                // ONE half-norm image per ring buffer, read by all eight waves
constexpr unsigned BUF_BYTES = TILE_BYTES + HN_BYTES;       // 33 280, a multiple of 16
constexpr unsigned OFFSET_LIMIT = 1u << 16;                 // ds_read_b128 offset: field

// per-lane part of a fragment address: lane (r, h), k-step ks
RCN_I8A_FN unsigned frag_lane(unsigned r, unsigned h, unsigned ks) { return r * ROW_BYTES + (((4u * ks + h) ^ r) << 4); }
// its immediate: row block rb, 16-row half
RCN_I8A_FN unsigned frag_imm(unsigned rb, unsigned half) { return (32u * rb + 16u * half) * ROW_BYTES; }
// per-lane part of a half-norm address (the same for every r)
RCN_I8A_FN unsigned hn_lane(unsigned h) { return 16u * h; }
// its immediate: the half-norm image sits right behind the tile
RCN_I8A_FN unsigned hn_imm(unsigned rb, unsigned half) { return TILE_BYTES + (32u * rb + 16u * half) * 4u; }
// a ring buffer's offset from the start of the ring
RCN_I8A_FN unsigned buffer_base(unsigned buf) { return buf * BUF_BYTES; }

static_assert(BUF_BYTES % 16 == 0, "ring buffers stay 16-byte aligned");
static_assert(frag_imm(3, 1) < OFFSET_LIMIT && hn_imm(3, 1) < OFFSET_LIMIT, "an immediate does not fit the offset field");

}  // namespace i8addr
