// PackBinaryRows.h -- a binary descriptor that crossed the reference's boundary as floats (FeatDesc::desc, one float per byte: the
// CV_8U -> CV_32F conversion of FeatureDetector.cpp:24) packed back into its bytes.  Pure C++, no device, no other header of the
// project: tests/cpp/hamming_host_test.cpp includes it alone.
//   packBinaryRow    one row of exactly 32 floats, each an integer in 0 .. 255, into 32 bytes
//   packBinaryRows   K such rows into K x 32 bytes, row-major
// std::invalid_argument: a row that is not 32 long, a value that is not an integer in 0 .. 255 (0.5, -1, 256, NaN, infinity).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace reconstructor::Core {

constexpr size_t kBinaryRowBytes = 32;

inline void packBinaryRow(const float *row, size_t length, uint8_t *out)
{
    if (length != kBinaryRowBytes) throw std::invalid_argument("packBinaryRows: a row of " + std::to_string(length) + " values, not 32");
    for (size_t k = 0; k < kBinaryRowBytes; ++k) {
        const float v = row[k];
        if (!(v >= 0.0f && v <= 255.0f) || v != std::floor(v))      // the first test is false for NaN
            throw std::invalid_argument("packBinaryRows: value " + std::to_string(k) + " of a row is not an integer in 0..255");
        out[k] = (uint8_t)(int)v;
    }
}

inline std::vector<uint8_t> packBinaryRows(const std::vector<std::vector<float>> &rows)
{
    std::vector<uint8_t> out(rows.size() * kBinaryRowBytes);
    for (size_t i = 0; i < rows.size(); ++i) packBinaryRow(rows[i].data(), rows[i].size(), out.data() + i * kBinaryRowBytes);
    return out;
}

}  // namespace reconstructor::Core
