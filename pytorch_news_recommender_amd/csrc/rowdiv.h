// Exact row -> sequence (row / S) for every row index the C ABI admits (n_seq * seq_len < 2^31), as one 32 x 32 -> 64-bit
// multiply and a shift (Granlund & Montgomery, "Division by invariant integers using multiplication", 1994).
//
// With l = ceil(log2 d), mul = ceil(2^(31+l) / d) and shift = 31 + l:
//     2^(31+l) <= mul * d < 2^(31+l) + d <= 2^(31+l) + 2^l,
// which is their condition for floor(n * mul / 2^(31+l)) == floor(n / d) for every 0 <= n < 2^31.  mul fits 32 bits
// (d > 2^(l-1), so 2^(31+l) / d < 2^32) and n * mul fits 64.
//
// Plain C++ with no HIP in it: the host test compiles this header on its own (tests/test_hip_extents.py) and walks the sequence
// boundaries up to 2^31 through it.  It replaces a float reciprocal, (long)((row + 0.5f) * (1.0f / S)), that was exact only
// below row 4 397 273 (S = 63; 5 093 099 at S = 30) and picked a neighbouring sequence past it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NRMS_HD __host__ __device__
#else
#define NRMS_HD
#endif

namespace nrms {

struct RowDiv { uint32_t mul, shift; };

// 1 <= d < 2^31
NRMS_HD inline RowDiv make_row_div(uint32_t d) {
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    RowDiv r;
    r.shift = 31 + l;
    r.mul = (uint32_t)(((1ull << r.shift) + d - 1) / d);
    return r;
}

// n / d for 0 <= n < 2^31
NRMS_HD inline uint32_t row_div(uint32_t n, RowDiv r) { return (uint32_t)(((uint64_t)n * r.mul) >> r.shift); }

}  // namespace nrms
