// What the catalogue kernels share (topk.hip: the k best items per user; rankdot.hip: the exact rank of given items in that
// order): the tile constants of the score chain and the uint64 entry that carries the order.
//
// An entry is the score as an order-preserving 32-bit key (-0.0 canonicalised to +0.0) above the complement of the 32-bit
// item id, so larger entry = higher score, then smaller id.  Entry 0 lies below every real entry and is padding.
#pragma once
#include "common.h"

namespace nrms {

constexpr int TK_UT = 32;                      // users per block (the MFMA's 32 rows)
constexpr int TK_WAVES = 8;                    // waves per block (k <= 192; 2 for larger k, whose buffers fill the LDS)
constexpr int TK_TN = 2;                       // 32-item column tiles per wave
constexpr int TK_BP = 36;                      // LDS row pitch (floats) of a wave's staged 64 x 32 item block
constexpr int TK_IT = 32 * TK_TN * TK_WAVES;   // catalogue items per block step at the largest wave count
constexpr int TK_TARGET_BLOCKS = 256;          // one 8-wave block per CU on 256 CUs
constexpr int TK_MAX_N = 0x7FFF0000;           // ids are held in 32 bits

typedef float tk_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint64_t tk_entry(float s, uint32_t id) {
    uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);       // -0.0 == +0.0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - id);
}

__device__ __forceinline__ float tk_entry_score(uint64_t e) {
    const uint32_t u = (uint32_t)(e >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

__device__ __forceinline__ int64_t tk_entry_id(uint64_t e) { return (int64_t)(0xFFFFFFFFu - (uint32_t)e); }

__device__ __forceinline__ void tk_wave_sync() {
    // LDS operations of one wave execute in issue order; this only stops the compiler from moving LDS accesses across
    // the passes of a sort
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float tk_ld(const float* p, int kk, int d) { return kk < d ? p[kk] : 0.0f; }

}  // namespace nrms
