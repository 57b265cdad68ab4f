// coarse_i8_addr_test.cpp -- csrc/coarse_i8_addr.h against the address formulas the int8 coarse kernel used before the split:
// for every lane (r, h), k-step, row block, 16-row half and ring buffer, (buffer + per-lane constant) + immediate must be the address
// computed in one piece; every immediate must fit the ds_read offset field; the sixteen lanes of one ds_read_b128 group must hit
// sixteen distinct 16-byte chunks.  Host only, no HIP types.
#include <cstdio>
#include <set>

#include "../../reconstructor_amd/csrc/coarse_i8_addr.h"

namespace {

constexpr unsigned ROWB = 256, BT = 128, TILEB = BT * ROWB, NBUF = 4;
constexpr unsigned BUFB = TILEB + BT * 4;       // one half-norm image per ring buffer

// the formulas in one piece, as k_coarse_top2_i8's step16 had them (tile = address of the ring buffer, hnl = tile + TILEB)
unsigned frag_whole(unsigned tile, unsigned rb, unsigned half, unsigned r, unsigned h, unsigned ks)
{
    const unsigned lrow = rb * 32 + r;
    const unsigned arow = tile + lrow * ROWB + half * 16 * ROWB;
    const unsigned sw = lrow & 15;
    return arow + (((ks * 4 + h) ^ sw) << 4);
}

unsigned hn_whole(unsigned tile, unsigned rb, unsigned half, unsigned h)
{
    const unsigned hnl = tile + TILEB;
    return hnl + (rb * 32 + 16 * half + 4 * h) * 4;
}

int failures = 0;

void expect(bool ok, const char *what, unsigned a, unsigned b, unsigned c, unsigned d)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s at (%u, %u, %u, %u)\n", what, a, b, c, d);
}

}  // namespace

int main()
{
    static_assert(i8addr::BUF_BYTES == BUFB && i8addr::TILE_BYTES == TILEB, "buffer geometry");
    long checked = 0;
    for (unsigned smem_base : {0u, 16u, 1024u}) {
        for (unsigned buf = 0; buf < NBUF; ++buf) {
            const unsigned tile = smem_base + i8addr::buffer_base(buf);
            expect(tile == smem_base + buf * BUFB, "buffer base", buf, 0, 0, 0);
            expect(tile % 16 == 0, "buffer alignment", buf, 0, 0, 0);
            for (unsigned rb = 0; rb < 4; ++rb) {
                for (unsigned half = 0; half < 2; ++half) {
                    expect(i8addr::frag_imm(rb, half) < 65536u, "fragment immediate", rb, half, 0, 0);
                    expect(i8addr::hn_imm(rb, half) < 65536u, "half-norm immediate", rb, half, 0, 0);
                    expect(i8addr::frag_imm(rb, half) % 16 == 0 && i8addr::hn_imm(rb, half) % 16 == 0, "immediate alignment", rb, half, 0, 0);
                    for (unsigned h = 0; h < 4; ++h) {
                        const unsigned got = tile + i8addr::hn_lane(h) + i8addr::hn_imm(rb, half);
                        expect(got == hn_whole(tile, rb, half, h), "half-norm address", rb, half, h, buf);
                        // inside this buffer's half-norm image, a whole quad
                        expect(got >= tile + TILEB && got + 16 <= tile + BUFB, "half-norm range", rb, half, h, buf);
                        ++checked;
                    }
                    for (unsigned ks = 0; ks < 4; ++ks) {
                        for (unsigned h = 0; h < 4; ++h) {
                            std::set<unsigned> chunks;
                            for (unsigned r = 0; r < 16; ++r) {
                                const unsigned got = tile + i8addr::frag_lane(r, h, ks) + i8addr::frag_imm(rb, half);
                                expect(got == frag_whole(tile, rb, half, r, h, ks), "fragment address", rb, half, 16 * h + r, ks);
                                expect(got % 16 == 0 && got >= tile && got + 16 <= tile + TILEB, "fragment range", rb, half, 16 * h + r, ks);
                                chunks.insert(got / 16);
                                // un-swizzled, the lane reads chunk 4 ks + h of row 32 rb + 16 half + r
                                const unsigned row = (got - tile) / ROWB, chunk = ((got - tile) % ROWB) / 16;
                                expect(row == 32 * rb + 16 * half + r && (chunk ^ (row & 15)) == 4 * ks + h, "fragment meaning", rb, half, 16 * h + r, ks);
                                ++checked;
                            }
                            expect(chunks.size() == 16, "sixteen distinct chunks per ds_read_b128 group", rb, half, h, ks);
                            // ... and sixteen distinct 16-byte bank groups of the 64-bank LDS (chunk index modulo 16)
                            std::set<unsigned> banks;
                            for (unsigned c : chunks) banks.insert(c % 16);
                            expect(banks.size() == 16, "sixteen distinct bank groups", rb, half, h, ks);
                        }
                    }
                }
            }
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("%ld addresses checked: all cases pass\n", checked);
    return 0;
}
