// packBinaryRows (reconstructor_amd/host/PackBinaryRows.h) alone, no device: the round trip of every byte value, the refusals, wrong row
// lengths, the empty input.  Built with the address and undefined-behaviour sanitizers by tests/test_hamming_host.py.
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../reconstructor_amd/host/PackBinaryRows.h"

using namespace reconstructor::Core;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool refuses(const std::vector<std::vector<float>> &rows)
{
    try {
        (void)packBinaryRows(rows);
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

int main()
{
    // every byte value, at every position of a row: eight rows of 32 cover 0 .. 255, a second set shifts them by 13 places
    for (int shift : {0, 13}) {
        std::vector<std::vector<float>> rows(8, std::vector<float>(32));
        for (int v = 0; v < 256; ++v) rows[(size_t)(v / 32)][(size_t)((v + shift) % 32)] = (float)v;
        const std::vector<uint8_t> got = packBinaryRows(rows);
        CHECK(got.size() == 256);
        for (int v = 0; v < 256; ++v) CHECK(got[(size_t)(v / 32) * 32 + (size_t)((v + shift) % 32)] == (uint8_t)v);
    }
    // the empty input
    CHECK(packBinaryRows(std::vector<std::vector<float>>{}).empty());
    // values that are no byte
    const float bad[] = {0.5f, -1.0f, 256.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                         -std::numeric_limits<float>::infinity(), 254.99998f, -0.25f, 1e9f};
    for (float b : bad)
        for (size_t pos : {(size_t)0, (size_t)17, (size_t)31}) {
            std::vector<std::vector<float>> rows(3, std::vector<float>(32, 7.0f));
            rows[1][pos] = b;
            CHECK(refuses(rows));
        }
    // -0.0 is the integer 0
    {
        std::vector<std::vector<float>> rows(1, std::vector<float>(32, -0.0f));
        CHECK(!refuses(rows) && packBinaryRows(rows)[5] == 0);
    }
    // wrong row lengths, alone and among good rows
    for (size_t len : {(size_t)0, (size_t)1, (size_t)31, (size_t)33, (size_t)64, (size_t)128}) {
        CHECK(refuses({std::vector<float>(len, 1.0f)}));
        CHECK(refuses({std::vector<float>(32, 1.0f), std::vector<float>(len, 1.0f)}));
    }
    // packBinaryRow writes exactly 32 bytes
    {
        std::vector<float> row(32, 255.0f);
        std::vector<uint8_t> out(32, 0);
        packBinaryRow(row.data(), row.size(), out.data());
        for (uint8_t b : out) CHECK(b == 255);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("all cases pass\n");
    return 0;
}
