// mid_i8_addr.h -- who holds what in k_mid_eval_i8's v_mfma_i32_16x16x64_i8 form (mid_i8.h): the fragment and LDS index arithmetic.
//
// Lane (r, h) of a wave: r = lane & 15, h = lane >> 4.  An int8 row is 256 bytes = sixteen 16-byte chunks; in memory chunk c of row j
// sits at chunk position c ^ (j & 15) (the resident images), and the query batch in LDS uses the same rule with the row's slot in the
// batch (the layout of exact_gather.h: the sixteen lanes a ds_read_b128 serves together hit sixteen different positions of the bank line).
//   A fragment (train):  wave w, row block rb, k-step ks -> row  tile_row(w, rb, r)  of the tile, logical chunk 4 ks + h
//   B fragment (query):  column block cb, k-step ks      -> slot 16 cb + r           of the batch, logical chunk 4 ks + h
//   accumulator element reg of lane (r, h), row block rb, column block cb
//                                                        -> train row tile_row(w, rb, 4 h + reg), query slot 16 cb + r
// Plain integer functions, no HIP types: tests/cpp/mid_i8_addr_test.cpp checks them on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RCN_MI8A_FN __host__ __device__ constexpr
#else
#define RCN_MI8A_FN constexpr
#endif

namespace mi8addr {

constexpr unsigned ROW_BYTES = 256;       // an int8 row
constexpr unsigned TILE_ROWS = 512;       // MI8_TR
constexpr unsigned WAVES = 4;
constexpr unsigned WAVE_ROWS = TILE_ROWS / WAVES;      // 128: a wave's stationary share
constexpr unsigned ROW_BLOCKS = WAVE_ROWS / 16;        // 8
constexpr unsigned BATCH_ROWS = 32;       // MI8_QB
constexpr unsigned COL_BLOCKS = BATCH_ROWS / 16;       // 2
constexpr unsigned K_STEPS = ROW_BYTES / 64;           // 4

// row of the tile: wave w, row block rb, row i of the block
RCN_MI8A_FN unsigned tile_row(unsigned w, unsigned rb, unsigned i) { return w * WAVE_ROWS + rb * 16u + i; }
// byte offset inside a swizzled row (row number or batch slot `row`) of logical chunk c
RCN_MI8A_FN unsigned chunk_off(unsigned row, unsigned c) { return ((c ^ (row & 15u)) << 4); }
// the chunk lane (., h) holds of k-step ks
RCN_MI8A_FN unsigned frag_chunk(unsigned h, unsigned ks) { return 4u * ks + h; }
// A fragment: byte offset from the tile's first row in the resident image
RCN_MI8A_FN unsigned a_off(unsigned w, unsigned rb, unsigned r, unsigned h, unsigned ks) { return tile_row(w, rb, r) * ROW_BYTES + chunk_off(tile_row(w, rb, r), frag_chunk(h, ks)); }
// staging: byte offset in a batch buffer of logical chunk c of slot s
RCN_MI8A_FN unsigned q_off(unsigned s, unsigned c) { return s * ROW_BYTES + chunk_off(s, c); }
// B fragment: byte offset in a batch buffer
RCN_MI8A_FN unsigned b_off(unsigned cb, unsigned r, unsigned h, unsigned ks) { return q_off(16u * cb + r, frag_chunk(h, ks)); }

static_assert(TILE_ROWS % (16 * WAVES) == 0 && BATCH_ROWS % 16 == 0, "whole 16-row blocks");
static_assert(b_off(COL_BLOCKS - 1, 15, 3, K_STEPS - 1) < BATCH_ROWS * ROW_BYTES, "a B fragment stays inside its buffer");

}  // namespace mi8addr
