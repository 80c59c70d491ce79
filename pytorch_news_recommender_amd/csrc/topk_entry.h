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

// The eligibility window of nrms_topk_dot_windowed / nrms_rank_dot_windowed (include/nrms_hip.h states it): item n is open to
// user b iff window[2 b] <= item_time[n] < window[2 b + 1], signed.  Null window = none, the kernels are the unwindowed ones.
struct TkWindow {
    const int32_t* item_time;    // [N]
    const int32_t* window;       // [B, 2]
};

// The TkWindow of a kernel whose trailing argument pack holds one, the null window of a kernel whose pack is empty.
template <class... WIN>
__device__ __forceinline__ TkWindow tk_window_arg(WIN... w) {
    if constexpr (sizeof...(WIN) == 1) return (w, ...);
    else return TkWindow{nullptr, nullptr};
}

// The dead-tile skip of the WINDOW kernels: a wave none of whose 64 item times lies in its block's [blo, bhi) runs no chain
// for that step.  false compiles the skip out (every wave runs its chain, the filter alone decides): same results, bit for bit
// (a diagnostic build with -DNRMS_TK_WINDOW_SKIP=0, e.g. through NRMS_HIPCC_EXTRA, passes tests/test_hip_topk_window.py unchanged).
#ifndef NRMS_TK_WINDOW_SKIP
#define NRMS_TK_WINDOW_SKIP 1
#endif
constexpr bool TK_WINDOW_SKIP = NRMS_TK_WINDOW_SKIP != 0;

// One block's windows (WINDOW kernels).  Threads [0, 32) write user u0 + threadIdx.x's (lo, hi) to win[threadIdx.x]; rows at or
// past B get the empty window (0, 0).  Call before the block's first barrier.
__device__ __forceinline__ void tk_window_stage(int2* win, const int32_t* __restrict__ window, int u0, int B) {
    if (threadIdx.x < TK_UT) {
        const int b = u0 + (int)threadIdx.x;
        win[threadIdx.x] = b < B ? make_int2(window[2 * (long)b], window[2 * (long)b + 1]) : make_int2(0, 0);
    }
}

// After that barrier, every thread: blo = min lo, bhi = max hi over the block's non-empty windows (INT32_MAX, INT32_MIN when
// there is none: no time lies in it).  An item outside [blo, bhi) is open to none of the block's users.
__device__ __forceinline__ void tk_window_hull(const int2* win, int& blo, int& bhi) {
    blo = 0x7FFFFFFF;
    bhi = -0x7FFFFFFF - 1;
    for (int u = 0; u < TK_UT; ++u) {
        const int2 w = win[u];
        if (w.x < w.y) {
            blo = min(blo, w.x);
            bhi = max(bhi, w.y);
        }
    }
}

__device__ __forceinline__ float tk_ld(const float* p, int kk, int d) { return kk < d ? p[kk] : 0.0f; }

}  // namespace nrms
