// What the catalogue kernels share (topk.hip and topksec.hip: the k best items per user; softmaxsample.hip: a Gumbel-top-S draw;
// rankdot.hip: the exact rank of given items in that order): the tile constants, the uint64 entry that carries the order, the
// one score chain every one of their kernels runs (tk_chain), the time window, the tag set, the per-user adjustments, and the host side every entry point shares:
// the launch geometry, the argument checks and the choice of a kernel instantiation.
//
// An entry is the score as an order-preserving 32-bit key (-0.0 canonicalised to +0.0) above the complement of the 32-bit
// item id, so larger entry = higher score, then smaller id.  Entry 0 lies below every real entry and is padding.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace nrms {

constexpr int TK_UT = 32;                      // users per block (the MFMA's 32 rows)
constexpr int TK_WAVES = 8;                    // waves per block (k <= 192; 2 for larger k, whose buffers fill the LDS)
constexpr int TK_TN = 2;                       // 32-item column tiles per wave
constexpr int TK_BP = 36;                      // LDS row pitch (floats) of a wave's staged 64 x 32 item block
constexpr int TK_IT = 32 * TK_TN * TK_WAVES;   // catalogue items per block step at the largest wave count
constexpr int TK_TARGET_BLOCKS = 256;          // one 8-wave block per CU on 256 CUs
constexpr int TK_MIN_SLICE = 4 * TK_IT;        // top-k: no slice shorter than this, each slice list costs k workspace entries
constexpr int TK_MAX_N = 0x7FFF0000;           // ids are held in 32 bits

typedef float tk_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint64_t tk_entry(float s, uint32_t id) {
    uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);       // -0.0 == +0.0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - id);
}

// The upper half of tk_entry(s, .): the score as an order-preserving 32-bit key.
__device__ __forceinline__ uint32_t tk_score_key(float s) {
    const uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
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

// The cursor of nrms_topk_dot_after / nrms_topk_dot_deep (include/nrms_hip.h states it): user b is offered only what comes
// strictly after the position (after_scores[b * stride], after_ids[b * stride]) of the order.  stride 1: the caller's [B] arrays;
// stride K: a column of a [B, K] result (the deep call's pages read the page before).  Null after_ids = none.
struct TkCursor {
    const float* after_scores;
    const int64_t* after_ids;
    long stride;
};
constexpr int64_t TK_CURSOR_BEGIN = -2;        // after_ids value: no cursor, the row of the uncursored call (NRMS_CURSOR_BEGIN)

// The T of a kernel whose trailing argument pack holds one (TkWindow, TkCursor), the null T of a kernel whose pack has none.
template <class T, class... EXT>
__device__ __forceinline__ T tk_pack_arg(EXT... e) {
    T out{};
    ([&] { if constexpr (std::is_same<EXT, T>::value) out = e; }(), ...);
    return out;
}
template <class... WIN>
__device__ __forceinline__ TkWindow tk_window_arg(WIN... w) {
    return tk_pack_arg<TkWindow>(w...);
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

// The all-END exit of the CURSOR kernels: a block whose 32 users have all reached the end of their lists writes its empty slice
// lists and returns before its first item row.  false compiles the exit out (the block scans its slice, the filter refuses every
// score): same results, bit for bit (a diagnostic build with -DNRMS_TK_CURSOR_EXIT=0, e.g. through NRMS_HIPCC_EXTRA, passes
// tests/test_hip_topk_after.py unchanged).
#ifndef NRMS_TK_CURSOR_EXIT
#define NRMS_TK_CURSOR_EXIT 1
#endif
constexpr bool TK_CURSOR_EXIT = NRMS_TK_CURSOR_EXIT != 0;

// A cursor as a key in the entries' order: user b is offered the entries strictly below it.  BEGIN (id -2) is the largest key,
// which only a NaN score's entry could reach, and NaN scores are never offered; END (any other negative id, a NaN score) is 0,
// below which nothing lies.  An id above TK_MAX_N is read as TK_MAX_N, which follows every item of the same score.
__device__ __forceinline__ uint64_t tk_cursor_key(float s, int64_t id) {
    if (id == TK_CURSOR_BEGIN) return ~0ull;
    if (id < 0 || s != s) return 0;
    return tk_entry(s, (uint32_t)(id > TK_MAX_N ? (int64_t)TK_MAX_N : id));
}

// One block's cursor keys (CURSOR kernels).  Threads [0, 32) write user u0 + threadIdx.x's key to cur[threadIdx.x]; rows at or
// past B are at END.  Call before the block's first barrier.
__device__ __forceinline__ void tk_cursor_stage(uint64_t* cur, TkCursor c, int u0, int B) {
    if (threadIdx.x < TK_UT) {
        const int b = u0 + (int)threadIdx.x;
        cur[threadIdx.x] = b < B ? tk_cursor_key(c.after_scores[b * c.stride], c.after_ids[b * c.stride]) : 0;
    }
}

// After that barrier, every thread: has every user of the block reached the end of its list?  Block-uniform.
__device__ __forceinline__ bool tk_cursor_all_end(const uint64_t* cur) {
    uint64_t any = 0;
    for (int u = 0; u < TK_UT; ++u) any |= cur[u];
    return any == 0;
}

// The per-user tag set of nrms_topk_dot_tagged / nrms_rank_dot_tagged (include/nrms_hip.h states it): item n is open to user b iff
// 0 <= item_tag[n] < n_tags and bit item_tag[n] & 31 of allow[b * W + (item_tag[n] >> 5)] is set, W = ceil(n_tags / 32).  Null
// allow = none, the kernels are the untagged ones.
struct TkTags {
    const int32_t* item_tag;     // [N]
    const uint32_t* allow;       // [B, W]
    int n_tags;
};
constexpr int TK_MAX_TAGS = 512;

// The dead-wave skip of the TAGS kernels: a wave none of whose 64 items carries a tag that a user of its block allows runs no
// chain for that step.  false compiles the skip out: same results, bit for bit (a diagnostic build with -DNRMS_TK_TAGS_SKIP=0,
// e.g. through NRMS_HIPCC_EXTRA, passes tests/test_hip_topk_tags.py unchanged).
#ifndef NRMS_TK_TAGS_SKIP
#define NRMS_TK_TAGS_SKIP 1
#endif
constexpr bool TK_TAGS_SKIP = NRMS_TK_TAGS_SKIP != 0;

// One block's transposed tag bitmap (TAGS kernels): bit i of ubt[t] is set iff user u0 + i allows tag t, t in [0, n_tags); rows at
// or past B allow nothing.  Every thread of the block (nthreads of them) takes part; call before the block's first barrier.  The
// bits of allow's last word at positions >= n_tags are never read.
__device__ __forceinline__ void tk_tags_stage(uint32_t* ubt, TkTags t, int u0, int B, int nthreads) {
    const int W = (t.n_tags + 31) >> 5;
    const int nu = min(TK_UT, B - u0);
    for (int tag = threadIdx.x; tag < t.n_tags; tag += nthreads) {
        const uint32_t* col = t.allow + (long)u0 * W + (tag >> 5);
        uint32_t m = 0;
        for (int i = 0; i < nu; ++i) m |= ((col[(long)i * W] >> (tag & 31)) & 1u) << i;
        ubt[tag] = m;
    }
}

// The block's users that item tag `tag` is open to, as a 32-bit mask (0 for a tag outside [0, n_tags): open to nobody).
__device__ __forceinline__ uint32_t tk_tags_mask(const uint32_t* ubt, int tag, int n_tags) {
    return (uint32_t)tag < (uint32_t)n_tags ? ubt[tag] : 0u;
}

// Is tag `tag` open to user b (read from global memory: the gathered ids of rank_entries_kernel).
__device__ __forceinline__ bool tk_tags_open(TkTags t, long b, int tag) {
    if ((uint32_t)tag >= (uint32_t)t.n_tags) return false;
    const int W = (t.n_tags + 31) >> 5;
    return (t.allow[b * W + (tag >> 5)] >> (tag & 31)) & 1u;
}

// The per-user tag caps of nrms_topk_dot_capped (include/nrms_hip.h states it): walking user b's ranking, item n is taken iff
// 0 <= item_tag[n] < n_tags and fewer than cap[b * n_tags + item_tag[n]] items of that tag were taken before it.
struct TkCaps {
    const int32_t* item_tag;     // [N]
    const int32_t* cap;          // [B, n_tags]
    int n_tags;
};

// One block's transposed bitmap of the tags that are not closed (CAPS kernels; tk_tags_stage's layout and rules): bit i of ubt[t]
// is set iff cap[u0 + i, t] > 0.
__device__ __forceinline__ void tk_caps_stage(uint32_t* ubt, TkCaps t, int u0, int B, int nthreads) {
    const int nu = min(TK_UT, B - u0);
    for (int tag = threadIdx.x; tag < t.n_tags; tag += nthreads) {
        const int32_t* col = t.cap + (long)u0 * t.n_tags + tag;
        uint32_t m = 0;
        for (int i = 0; i < nu; ++i) m |= (uint32_t)(col[(long)i * t.n_tags] > 0) << i;
        ubt[tag] = m;
    }
}

// REQ + CAPS kernels: tk_tags_stage with the caps applied: bit i of ubt[t] is set iff cap[u0 + i, t] > 0 and, where there is a tag
// set (a.allow not null), user u0 + i allows tag t.  The tags and their number are the caps'.
__device__ __forceinline__ void tk_tags_stage(uint32_t* ubt, TkTags a, TkCaps t, int u0, int B, int nthreads) {
    const int W = (t.n_tags + 31) >> 5;
    const int nu = min(TK_UT, B - u0);
    for (int tag = threadIdx.x; tag < t.n_tags; tag += nthreads) {
        const int32_t* col = t.cap + (long)u0 * t.n_tags + tag;
        const uint32_t* acol = a.allow ? a.allow + (long)u0 * W + (tag >> 5) : nullptr;
        uint32_t m = 0;
        for (int i = 0; i < nu; ++i) {
            uint32_t open = (uint32_t)(col[(long)i * t.n_tags] > 0);
            if (acol) open &= acol[(long)i * W] >> (tag & 31);
            m |= open << i;
        }
        ubt[tag] = m;
    }
}

// One wave: k_b = min(k, sum over tags of min(max(cap_row[t], 0), k)), the length the capped list of user row cap_row can reach,
// in bits 0 .. 15, and in bit 16 whether any tag is rationed at all (0 < cap_row[t] < k_b; if none is, the capped list is the
// best k_b of the open tags).  Once a capped list holds k_b entries nothing below its smallest entry can enter it: k_b = k: k taken
// items precede it; k_b < k: every open tag is saturated.  Wave-uniform.
__device__ __forceinline__ int tk_caps_reach(const int32_t* __restrict__ cap_row, int n_tags, int k, int lane) {
    int sum = 0;
    for (int t = lane; t < n_tags; t += 64) sum += min(max(cap_row[t], 0), k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const int kb = min(sum, k);
    bool rationed = false;
    for (int t = lane; t < n_tags; t += 64) rationed |= cap_row[t] > 0 && cap_row[t] < kb;
    return __builtin_amdgcn_readfirstlane(kb | (__ballot(rationed) != 0 ? 0x10000 : 0));
}

// The per-user score adjustments of nrms_topk_dot_adjusted / nrms_rank_dot_adjusted (include/nrms_hip.h states them): slot (b, e)
// names catalogue row adj_ids[b, e] (a value outside [0, N): an empty slot) and moves that row's score for user b by
// adj_delta[b, e], one fp32 add on the finished s'; of several slots of one user that name one row the LOWEST e counts.
struct TkAdjust {
    const int64_t* adj_ids;      // [B, E]
    const float* adj_delta;      // [B, E]
    int n_adjust;                // E
};
constexpr int TK_ADJ_MAX = 256;
// A block's staged slots (ADJ kernels) are 32-bit words: (row - the slice's first row) << 5 | user row of the block.  A slice
// longer than 2^27 rows (only a catalogue beyond 2^27 rows cut into very few slices) is not staged: its block walks the global
// lists, like a block whose slots overflow its LDS list.
constexpr int TK_ADJ_ROW_BITS = 27;
// The staged slots that fit beside a P class's buffers (top-k slice kernels; the rank count kernel has no buffers and holds
// every slot its 32 users can have).
constexpr int tk_adjust_cap(int P) { return P <= 256 ? 2048 : 1024; }
constexpr int RK_ADJ_CAP = TK_UT * TK_ADJ_MAX;

// The parts of nrms_topk_dot_request / nrms_rank_dot_request (include/nrms_hip.h states their composition): a window, a tag set,
// adjustments and a cursor in ONE kernel form (the REQ instantiations), each with the rules of its own call.  A part whose
// pointer (win.window, tags.allow, adj.adj_ids, cur.after_ids) is null is absent: the kernels branch on it, block-uniformly.
struct TkRequest {
    TkWindow win;
    TkTags tags;
    TkAdjust adj;
    TkCursor cur;        // top-k only
};
// The staged slots of a REQ slice kernel: at P = 512 half of tk_adjust_cap's, which pays for the tag bitmap, the windows and the
// cursor keys that lie beside the list there (any capacity is correct: a list that overflows is not used, tk_adjust_mark).
constexpr int tk_request_adjust_cap(int P) { return P <= 256 ? 2048 : 512; }

// One block's staged slots: the slots of users [u0, u0 + 32) that name a row of [n_begin, n_end), in any order, appended to
// xl[0, CAP); *xl_n counts them (past CAP: the list overflowed and is not used).  *xl_n is 0 on entry and a barrier lies between
// that store and this call; every thread of the block (nthreads of them) takes part; the caller's next barrier publishes it.
template <int CAP>
__device__ __forceinline__ void tk_adjust_stage(uint32_t* xl, int* xl_n, TkAdjust a, int u0, int B, int n_begin, int n_end,
                                                int nthreads) {
    if (n_end - n_begin > (1 << TK_ADJ_ROW_BITS)) {          // block-uniform: nobody appends
        if (threadIdx.x == 0) *xl_n = CAP + 1;
        return;
    }
    const int E = a.n_adjust;
    const int total = min(TK_UT, B - u0) * E;
    for (int i = threadIdx.x; i < total; i += nthreads) {
        const int64_t v = a.adj_ids[(long)u0 * E + i];
        if (v >= n_begin && v < n_end) {
            const int at = atomicAdd(xl_n, 1);
            if (at < CAP) xl[at] = ((uint32_t)(v - n_begin) << 5) | (uint32_t)(i / E);
        }
    }
}

// One wave, one step: xmask[c] = the block's user rows (bit i: user u0 + i) with a slot that names this lane's item nw + 32 c +
// (lane & 31) of column tile c.  n_xl: the block's *xl_n after the publishing barrier (0: no slot names a row of the slice, nothing
// is read; at most CAP: the staged list is scanned; more: the global lists of the block's users are walked, correct and slow on
// purpose).  xm: the wave's private row of 64 words, all 0 between calls.  Marks are a set, so the order of xl does not matter;
// which slot counts is decided where the delta is read (tk_adjust_find).  Wave-level syncs only; nw < n_end.
template <int CAP>
__device__ __forceinline__ void tk_adjust_mark(uint32_t (&xmask)[TK_TN], uint32_t* xm, const uint32_t* xl, int n_xl, TkAdjust a,
                                               int u0, int B, int n_begin, int nw, int n_end, int lane) {
#pragma unroll
    for (int c = 0; c < TK_TN; ++c) xmask[c] = 0;
    if (n_xl == 0) return;
    if (n_xl <= CAP) {
        const uint32_t base = (uint32_t)(nw - n_begin);
        for (int i = lane; i < n_xl; i += 64) {
            const uint32_t e = xl[i];
            const uint32_t off = (e >> 5) - base;
            if (off < 64u) atomicOr(&xm[off], 1u << (e & 31u));
        }
    } else {
        const int E = a.n_adjust;
        const int total = min(TK_UT, B - u0) * E;
        const int64_t hi = min((int64_t)nw + 64, (int64_t)n_end);
        for (int i = lane; i < total; i += 64) {
            const int64_t v = a.adj_ids[(long)u0 * E + i];
            if (v >= nw && v < hi) atomicOr(&xm[(int)(v - nw)], 1u << (i / E));
        }
    }
    tk_wave_sync();
#pragma unroll
    for (int c = 0; c < TK_TN; ++c) xmask[c] = xm[32 * c + (lane & 31)];
    tk_wave_sync();
#pragma unroll
    for (int c = 0; c < TK_TN; ++c)
        if (xmask[c]) xm[32 * c + (lane & 31)] = 0;
    tk_wave_sync();
}

// The delta of user b's LOWEST slot that names row n >= 0 (read from global memory: hits are rare and the lists L2-resident).  The
// list is read eight slots at a time, so that eight loads are in flight per round trip, and compared in slot order.
__device__ __forceinline__ bool tk_adjust_find(TkAdjust a, long b, int64_t n, float& delta) {
    const int E = a.n_adjust;
    const int64_t* row = a.adj_ids + b * E;
    for (int e0 = 0; e0 < E; e0 += 8) {
        int64_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = e0 + j < E ? row[e0 + j] : -1;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (v[j] == n) {
                delta = a.adj_delta[b * E + e0 + j];
                return true;
            }
    }
    return false;
}

// One wave, after the chain (and the prior's add): the lane that holds a marked pair adds the pair's delta to its accumulator
// register, one fp32 add; every other register is left as it is.  C/D layout: user row i = (q & 3) + 8 (q >> 2) + 4 (lane >> 5),
// so this lane holds the rows with bit 2 of i equal to its half, in register q = (i & 3) + 4 (i >> 3).
__device__ __forceinline__ void tk_adjust_apply(tk_f32x16 (&acc)[TK_TN], const uint32_t (&xmask)[TK_TN], TkAdjust a, int u0, int nw,
                                                int lane) {
    const uint32_t half = (lane >> 5) ? 0xF0F0F0F0u : 0x0F0F0F0Fu;
#pragma unroll
    for (int c = 0; c < TK_TN; ++c) {
        uint32_t m = xmask[c] & half;
        while (m) {
            const int i = __builtin_ctz(m);
            m &= m - 1;
            float dl;
            if (!tk_adjust_find(a, u0 + i, nw + 32 * c + (lane & 31), dl)) continue;
            const int qw = (i & 3) + 4 * (i >> 3);
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q == qw) acc[c][q] = acc[c][q] + dl;
        }
    }
}

__device__ __forceinline__ float tk_ld(const float* p, int kk, int d) { return kk < d ? p[kk] : 0.0f; }

// The score chain of every catalogue kernel.  One wave: acc[c] += the 32 x 32 score tile of A rows (lane (r, h): the row of
// user r; arow[c] feeds column tile c when NA = TK_TN, arow[0] feeds both when NA = 1) against item rows row_of(32 c + 0 .. 31),
// c = 0, 1.  row_of(i), i in [0, 64): a valid row of `items` (callers clamp).
//
// Operands: each whole block of 32 floats of k is staged in the wave's private LDS block st through coalesced loads (lane l of
// load j reads row 8j + l / 8, floats 4 (l % 8) .. + 3: eight full 128-byte row segments per instruction) and read back in the
// MFMA layout; the A rows come straight from global memory (shared by the block's waves in L1).  The next block of k is loaded
// into registers while the MFMAs of this one run.  Lane (r, h) feeds A[user r][k'=h] and B[k'=h][item r]; MFMA t of block m sums
// k = 32m + t (h = 0) and 32m + 16 + t (h = 1).  The rest of d goes in groups of 8 (8g + t and 8g + 4 + t, zero past d).  The
// same fixed chain for every (user, item) pair of every caller: their score bits are equal.  It touches only st and wave-level
// syncs, never a block barrier.
template <bool VEC, int NA, class RowOf>
__device__ __forceinline__ void tk_chain(tk_f32x16 (&acc)[TK_TN], const float* const (&arow)[NA], const float* __restrict__ items,
                                         int d, float* st, int lane, RowOf row_of) {
    static_assert(NA == 1 || NA == TK_TN, "one A operand, or one per column tile");
    const int r = lane & 31, h = lane >> 5;
    const int m_full = d / 32;
    const float* srow[8];           // rows this lane stages: 8j + lane / 8
#pragma unroll
    for (int j = 0; j < 8; ++j) srow[j] = items + (long)row_of(8 * j + (lane >> 3)) * d + 4 * (lane & 7);
    auto gload = [&](int m, float (&g)[8][4], float (&a)[NA][16]) {
        const int k0 = 32 * m;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if constexpr (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(srow[j] + k0);
                g[j][0] = v.x; g[j][1] = v.y; g[j][2] = v.z; g[j][3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) g[j][e] = srow[j][k0 + e];
            }
        }
#pragma unroll
        for (int c = 0; c < NA; ++c)
#pragma unroll
            for (int t = 0; t < 16; ++t) a[c][t] = arow[c][k0 + 16 * h + t];
    };
    if (m_full > 0) {
        float g[8][4];
        float a[NA][16];
        gload(0, g, a);
        for (int m = 0; m < m_full; ++m) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                *reinterpret_cast<float4*>(st + (8 * j + (lane >> 3)) * TK_BP + 4 * (lane & 7)) =
                    make_float4(g[j][0], g[j][1], g[j][2], g[j][3]);
            tk_wave_sync();
            float b[TK_TN][16];
#pragma unroll
            for (int c = 0; c < TK_TN; ++c)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float4 v = *reinterpret_cast<const float4*>(st + (32 * c + r) * TK_BP + 16 * h + 4 * t);
                    b[c][4 * t] = v.x; b[c][4 * t + 1] = v.y; b[c][4 * t + 2] = v.z; b[c][4 * t + 3] = v.w;
                }
            float acur[NA][16];
#pragma unroll
            for (int c = 0; c < NA; ++c)
#pragma unroll
                for (int t = 0; t < 16; ++t) acur[c][t] = a[c][t];
            if (m + 1 < m_full) gload(m + 1, g, a);
#pragma unroll
            for (int t = 0; t < 16; ++t)
#pragma unroll
                for (int c = 0; c < TK_TN; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(acur[NA == 1 ? 0 : c][t], b[c][t], acc[c], 0, 0, 0);
            tk_wave_sync();        // this block's LDS reads stay ahead of the next block's writes
        }
    }
    for (int g8 = 4 * m_full; 8 * g8 < d; ++g8) {       // zero-padded groups of 8 past the last whole block
        const int k0 = 8 * g8 + 4 * h;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float at[NA];
#pragma unroll
            for (int c = 0; c < NA; ++c) at[c] = tk_ld(arow[c], k0 + t, d);
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) {
                const float* brow = items + (long)row_of(32 * c + r) * d;
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(at[NA == 1 ? 0 : c], tk_ld(brow, k0 + t, d), acc[c], 0, 0, 0);
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// The launch geometry of the slice and count kernels: 32-user tiles x S catalogue slices of slice_len items (whole block
// steps), about one 8-wave block per CU.  min_slice (the top-k calls, whose workspace grows with S): no slice shorter than
// TK_MIN_SLICE.
struct TkGeom {
    int tiles, S, slice_len;
};

static TkGeom tk_geom(int32_t B, int64_t N, bool min_slice) {
    TkGeom g{cdiv(B, TK_UT), 0, 0};
    if (N == 0 || B == 0) return g;
    int s = std::max(1, cdiv(TK_TARGET_BLOCKS, g.tiles));
    if (min_slice) s = std::min(s, std::max(1, cdiv(N, TK_MIN_SLICE)));
    g.slice_len = cdiv(cdiv(N, s), TK_IT) * TK_IT;
    g.S = cdiv(N, g.slice_len);
    return g;
}

// The extent checks every entry point starts with, in this order: B, N in [0, n_max], d, the list length (kname "k", "S" or
// "T", in [1, k_max]) and n_exclude.
static int tk_check_dims(const char* who, int32_t B, int64_t N, int64_t n_max, int32_t d, const char* kname, int32_t k,
                         int32_t k_max, int32_t n_exclude) {
    NRMS_REQUIRE(B >= 0, "%s: B must be >= 0 (B=%d)", who, B);
    NRMS_REQUIRE(N >= 0 && N <= n_max, "%s: N must be in [0, %lld] (N=%lld)", who, (long long)n_max, (long long)N);
    NRMS_REQUIRE(d >= 1, "%s: d must be >= 1 (d=%d)", who, d);
    NRMS_REQUIRE(k >= 1 && k <= k_max, "%s: %s must be in [1, %d] (%s=%d)", who, kname, k_max, kname, k);
    NRMS_REQUIRE(n_exclude >= 0, "%s: n_exclude must be >= 0 (n_exclude=%d)", who, n_exclude);
    return NRMS_OK;
}

// One pointer argument: required (else it may be null), and aligned to align bytes when align > 1.
struct TkPtr {
    const char* name;
    const void* p;
    bool required;
    unsigned align;
};

// The pointer checks (after the B == 0 return), in list order, then the workspace: not null, at least `need` bytes
// (NRMS_EWORKSPACE otherwise), aligned to ws_align.
static int tk_check_ptrs(const char* who, std::initializer_list<TkPtr> ptrs, const void* workspace, size_t workspace_bytes,
                         size_t need, unsigned ws_align) {
    for (const TkPtr& a : ptrs) {
        NRMS_REQUIRE(a.p || !a.required, "%s: %s is null", who, a.name);
        NRMS_REQUIRE(a.align <= 1 || ((uintptr_t)a.p & (a.align - 1)) == 0, "%s: %s must be %u-byte aligned", who, a.name, a.align);
    }
    NRMS_REQUIRE(workspace, "%s: workspace is null", who);
    if (workspace_bytes < need) {
        set_error("%s: workspace %zu < required %zu bytes", who, workspace_bytes, need);
        return NRMS_EWORKSPACE;
    }
    NRMS_REQUIRE(((uintptr_t)workspace & (ws_align - 1)) == 0, "%s: workspace must be %u-byte aligned", who, ws_align);
    return NRMS_OK;
}

// E and the two lists of the adjusted calls: 0 <= E <= TK_ADJ_MAX; with E > 0 the lists come together or not at all (neither: no
// adjustment).
static int adjust_check(const char* who, int32_t n_adjust, const int64_t* adj_ids, const float* adj_delta) {
    NRMS_REQUIRE(n_adjust >= 0 && n_adjust <= TK_ADJ_MAX, "%s: n_adjust must be in [0, %d] (n_adjust=%d)", who, TK_ADJ_MAX, n_adjust);
    NRMS_REQUIRE(n_adjust == 0 || (adj_ids != nullptr) == (adj_delta != nullptr), "%s: %s is null (n_adjust=%d)", who,
                 adj_ids ? "adj_delta" : "adj_ids", n_adjust);
    NRMS_REQUIRE(n_adjust == 0 || !adj_ids || ((uintptr_t)adj_ids & 7) == 0, "%s: adj_ids must be 8-byte aligned", who);
    NRMS_REQUIRE(n_adjust == 0 || !adj_delta || ((uintptr_t)adj_delta & 3) == 0, "%s: adj_delta must be 4-byte aligned", who);
    return NRMS_OK;
}

// nrms_rank_dot_tagged's body: rankdot.hip defines it beside the rank kernels, topktags.hip holds the C entry point.
int rank_dot_tagged_call(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items, const float* bias,
                         TkTags tags, const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                         float* target_scores, void* workspace, size_t workspace_bytes, void* stream);

// nrms_rank_dot_adjusted's body: rankdot.hip defines it beside the rank kernels, topkadjust.hip holds the C entry point.
int rank_dot_adjusted_call(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items, const float* bias,
                           TkAdjust adj, const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                           float* target_scores, void* workspace, size_t workspace_bytes, void* stream);

// nrms_rank_dot_request's body for two or more parts: rankdot.hip defines it beside the rank kernels, topkrequest.hip holds the C
// entry point, which has checked the parts' pairs, n_tags and E.
int rank_dot_request_call(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items, const float* bias,
                          TkRequest req, const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                          float* target_scores, void* workspace, size_t workspace_bytes, void* stream);

// The chain's loads are float4 when every row starts on 16 bytes.
static bool tk_vec_ok(int32_t d, const float* user, const float* items) {
    return (d & 3) == 0 && ((uintptr_t)user & 15) == 0 && ((uintptr_t)items & 15) == 0;
}

// f(std::bool_constant<b>...) for run-time flags: picks the <VEC, BIAS, WINDOW, ...> instantiation of a kernel.
template <class F>
static void tk_with_flags(F f) {
    f();
}
template <class F, class... Rest>
static void tk_with_flags(F f, bool b, Rest... rest) {
    if (b) tk_with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else tk_with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// f(P, W) as integral constants: the buffer length P >= k + 64 (a power of two) of the slice and merge kernels and the waves
// per block W of the slice kernels (2 at the largest P, whose buffers fill the LDS).
template <class F>
static void tk_with_pw(int k, F f) {
    if (k + 64 <= 128) f(std::integral_constant<int, 128>{}, std::integral_constant<int, TK_WAVES>{});
    else if (k + 64 <= 256) f(std::integral_constant<int, 256>{}, std::integral_constant<int, TK_WAVES>{});
    else f(std::integral_constant<int, 512>{}, std::integral_constant<int, 2>{});
}

}  // namespace nrms
