// mid_i8_addr_test.cpp -- csrc/mid_i8_addr.h, the index arithmetic of k_mid_eval_i8's MFMA form, on the host:
//   * the A fragments of the four waves cover every 16-byte chunk of the 512-row tile exactly once, and lane (r, h) of k-step ks reads
//     logical chunk 4 ks + h of its row through the resident images' swizzle;
//   * staging a batch is a bijection onto the 8-KiB buffer, and the B fragment of lane (r, h) is logical chunk 4 ks + h of slot 16 cb + r:
//     the same k range as the A fragment it meets, the sixteen (ks, h) a permutation of the row's sixteen chunks;
//   * the sixteen lanes a ds_read_b128 serves together hit sixteen different 16-byte positions of the 256-byte bank line.
// Host only, no HIP types.
#include <cstdio>
#include <set>
#include <vector>

#include "../../reconstructor_amd/csrc/mid_i8_addr.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, unsigned a, unsigned b, unsigned c, unsigned d)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s at (%u, %u, %u, %u)\n", what, a, b, c, d);
}

// the lanes one LDS cycle of a ds_read_b128 serves
const unsigned GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

}  // namespace

int main()
{
    using namespace mi8addr;
    long checked = 0;
    // A fragments
    std::vector<int> seen(TILE_ROWS * 16, 0);
    for (unsigned w = 0; w < WAVES; ++w)
        for (unsigned rb = 0; rb < ROW_BLOCKS; ++rb)
            for (unsigned lane = 0; lane < 64; ++lane)
                for (unsigned ks = 0; ks < K_STEPS; ++ks) {
                    const unsigned r = lane & 15, h = lane >> 4, off = a_off(w, rb, r, h, ks);
                    expect(off % 16 == 0 && off + 16 <= TILE_ROWS * ROW_BYTES, "A range", w, rb, lane, ks);
                    const unsigned row = off / ROW_BYTES, pos = (off % ROW_BYTES) / 16;
                    expect(row == w * 128 + rb * 16 + r, "A row", w, rb, lane, ks);
                    expect((pos ^ (row & 15)) == 4 * ks + h, "A chunk", w, rb, lane, ks);
                    if (off + 16 <= TILE_ROWS * ROW_BYTES) ++seen[off / 16];
                    // the accumulator rows of this lane: 4 h + reg of the block
                    for (unsigned reg = 0; reg < 4; ++reg) expect(tile_row(w, rb, 4 * h + reg) == w * 128 + rb * 16 + 4 * h + reg, "C row", w, rb, lane, reg);
                    ++checked;
                }
    for (unsigned i = 0; i < seen.size(); ++i) expect(seen[i] == 1, "every chunk of the tile in exactly one fragment", i / 16, i % 16, 0, 0);
    // staging
    std::set<unsigned> staged;
    for (unsigned s = 0; s < BATCH_ROWS; ++s)
        for (unsigned c = 0; c < 16; ++c) {
            const unsigned off = q_off(s, c);
            expect(off % 16 == 0 && off + 16 <= BATCH_ROWS * ROW_BYTES && off / ROW_BYTES == s, "staging range", s, c, 0, 0);
            staged.insert(off);
        }
    expect(staged.size() == BATCH_ROWS * 16, "staging is a bijection", 0, 0, 0, 0);
    // B fragments
    for (unsigned cb = 0; cb < COL_BLOCKS; ++cb)
        for (unsigned ks = 0; ks < K_STEPS; ++ks) {
            for (unsigned lane = 0; lane < 64; ++lane) {
                const unsigned r = lane & 15, h = lane >> 4, off = b_off(cb, r, h, ks);
                expect(off == q_off(16 * cb + r, 4 * ks + h), "B fragment = the staged chunk", cb, ks, lane, 0);
                expect(frag_chunk(h, ks) == 4 * ks + h, "A and B meet on the same k range", cb, ks, lane, 0);
                ++checked;
            }
            for (const auto &g : GROUPS) {
                std::set<unsigned> pos;
                for (unsigned lane : g) pos.insert((b_off(cb, lane & 15, lane >> 4, ks) / 16) % 16);
                expect(pos.size() == 16, "sixteen distinct positions of the bank line per ds_read_b128 group", cb, ks, g[0], 0);
            }
        }
    std::set<unsigned> ksteps;
    for (unsigned ks = 0; ks < K_STEPS; ++ks)
        for (unsigned h = 0; h < 4; ++h) ksteps.insert(frag_chunk(h, ks));
    expect(ksteps.size() == 16 && *ksteps.rbegin() == 15, "the k-steps cover the row once", 0, 0, 0, 0);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("%ld addresses checked: all cases pass\n", checked);
    return 0;
}
