// The pieces of the catalogue selections, each written once: the candidate filter of a slice kernel's block (TkFilter), the
// one-wave merge of slice lists (tk_merge), the tiles of a grouped catalogue (TkTile, TkWaveTiles), and the slice and merge
// kernels with their launcher.  topk.hip (whose head comment describes the two kernels): nrms_topk_dot, its biased and windowed
// forms and nrms_topk_grouped_dot; softmaxsample.hip: nrms_softmax_sample_dot, the same slices and merge with a keyed Gumbel
// perturbation added to every score before it meets the threshold; topksec.hip: nrms_topk_sections_dot, a slice kernel of its
// own (one slice-table entry per block) and a merge kernel of its own (one section per block) over the same pieces.
#pragma once
#include "topk_entry.h"      // the entry, the tile constants, the score chain and the host helpers rankdot.hip shares

namespace nrms {

constexpr int TK_EX_LDS = 64;                  // exclude lists up to this long are staged in LDS, longer ones read globally
constexpr int TK_MAX_K = 256;

// The perturbation of nrms_softmax_sample_dot (include/nrms_hip.h states it): null row_key = none, the kernels are top-k's.
struct TkNoise {
    const int64_t* row_key;      // [B]
    float inv_temperature;
    uint64_t seed;
};

// Level one: the 64-bit seed of a row key.  Level two: item n's word, word n & 3 of the call that n's group of four shares.
__host__ __device__ __forceinline__ uint64_t tk_noise_row_seed(uint64_t seed, uint64_t row_key) {
    uint32_t r[4];
    philox4x32_7(seed, row_key, PHILOX_SITE_SOFTMAX_ROW, r);
    return (uint64_t)r[0] | ((uint64_t)r[1] << 32);
}
__host__ __device__ __forceinline__ uint32_t tk_noise_word(uint64_t row_seed, uint32_t n) {
    uint32_t r[4];
    philox4x32_7(row_seed, (uint64_t)(n >> 2), PHILOX_SITE_SOFTMAX_ITEM, r);
    const uint32_t lo = (n & 1) ? r[1] : r[0], hi = (n & 1) ? r[3] : r[2];
    return (n & 2) ? hi : lo;
}
// Standard Gumbel of a word: u = (2 (w >> 9) + 1) 2^-24 is exact in fp32 and strictly inside (0, 1), g = -log(-log(u)) < 17.4.
__device__ __forceinline__ float tk_gumbel(uint32_t w) {
    const float u = (float)(2u * (w >> 9) + 1u) * 0x1p-24f;
    return -logf(-logf(u));
}

// One 32-row tile of a grouped catalogue: rows [row, row + len) of group grp (len 0: an unused tile past the last group).
struct TkTile {
    int row, len, grp, pad;
};

// One wave sorts buf[0, P) descending (bitonic network; P a power of two).
template <int P>
__device__ void tk_sort_desc(uint64_t* buf, int lane) {
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < P / 2; t += 64) {
                const int i = 2 * t - (t & (stride - 1));       // the lower index of the pair, bit `stride` clear
                const int j = i + stride;
                const uint64_t a = buf[i], b = buf[j];
                const bool desc = (i & size) == 0;
                if (desc ? a < b : a > b) {
                    buf[i] = b;
                    buf[j] = a;
                }
            }
            tk_wave_sync();
        }
    }
}

// One wave: pads buf[cnt, P) with 0 and sorts buf descending; returns the k-th entry.
template <int P>
__device__ uint64_t tk_flush(uint64_t* buf, int cnt, int k, int lane) {
    for (int j = cnt + lane; j < P; j += 64) buf[j] = 0;
    tk_wave_sync();
    tk_sort_desc<P>(buf, lane);
    return buf[k - 1];
}

// One wave: keeps the best k of buf[0, cnt) (unsorted, compacted to the front; entries 0 are dropped) and returns their
// count in cnt and the threshold T: at most the k-th entry (0 when fewer than k remain), with exactly k entries >= T.  T is
// found by a bitwise search over the 64-bit entries held in registers (towards the largest T with #{e >= T} >= k, stopping
// as soon as exactly k entries are >= T), not by sorting.  Accepting later candidates above T rather than above the k-th
// entry only lets a few more through.
template <int P>
__device__ uint64_t tk_select(uint64_t* buf, int& cnt, int k, int lane) {
    constexpr int E = P / 64;
    uint64_t v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = lane + 64 * e < cnt ? buf[lane + 64 * e] : 0;
    uint64_t T = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const uint64_t c = T | (1ull << bit);
        int n = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) n += __popcll(__ballot(v[e] >= c));
        if (n >= k) T = c;
        if (n == k) break;           // exactly k entries >= T: T <= the k-th entry is threshold enough, and keeps exactly k
    }
    tk_wave_sync();
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const bool keep = v[e] != 0 && v[e] >= T;
        const unsigned long long m = __ballot(keep);
        if (keep) buf[base + __popcll(m & below)] = v[e];
        base += __popcll(m);
    }
    tk_wave_sync();
    cnt = base;
    return T;
}

// The selection a filter cuts a full buffer down with: tk_select (the best k), or tk_select_capped (CAPS kernels: the capped best
// k of one user; cap_row = the user's row of cap, reach = its tk_caps_reach).
//
// TkSelectCapped also holds the block's tag thresholds: ttag[i * TT + t], 16 bits per (user row, tag), 0 at the start.  When a flush
// takes the cap-th entry x of tag t for user i it stores the upper 16 bits of x's score key there (never lowering it): cap items of
// tag t that beat x have been seen, so an item of tag t whose key's upper 16 bits are BELOW that value lies below all of them and can
// never be taken; TkFilter::above_tags refuses it before it is offered.  Without this, every item of a saturated tag that beats the
// user's one threshold (the k_b-th best TAKEN entry, which a cap pushes far down the ranking) floods the buffers only to be dropped
// by the next flush.  TT tags fit the LDS the P class leaves free (tk_caps_table); a call with more tags runs without the table
// (ttag null), with the same results.
struct TkSelectBest {
    static constexpr bool capped = false;
};
template <int TT, bool OUTLINE = false>
struct TkSelectCapped {
    static constexpr bool capped = true;
    static constexpr bool outline = OUTLINE;          // REQ + CAPS kernels: the capped selection is a call, not inlined into the scan
    static constexpr int table = TT;
    const int32_t* item_tag;     // [N]
    const int32_t* cap;          // [B, n_tags]
    int n_tags;
    const int* reach;            // LDS: the block's 32 tk_caps_reach words
    uint16_t* ttag;              // LDS: the block's [32][TT] tag thresholds, or null
};
// The tags whose thresholds fit beside a P class's buffers: 32 x TT x 2 bytes of the LDS the class leaves free.
constexpr int tk_caps_table(int P) { return P <= 128 ? 512 : P <= 256 ? 192 : 48; }
// The same beside the parts of a request (REQ + CAPS kernels): what the REQ form leaves free; none at P = 512.
constexpr int tk_request_caps_table(int P) { return P <= 128 ? 512 : P <= 256 ? 43 : 0; }

typedef uint16_t __attribute__((may_alias)) tk_u16_alias;

// One wave: cuts buf[0, cnt) (unsorted, distinct entries, 0 = dropped) down to its capped list C(buf): walking the entries in
// descending order, an entry is taken iff its tag t lies in [0, n_tags), fewer than cap_row[t] entries of tag t were taken before
// it and fewer than k entries were taken before it.  reach: the user's tk_caps_reach word, k_b and whether any open tag is
// rationed at all (0 < cap < k_b).
//
// No rationed tag (the caller's filter only ever admits entries of open tags): C(buf) is the best k_b, tk_select's problem.
// Otherwise: the buffer is sorted descending in place (tk_sort_desc) and read back into registers, 64 ranks per register and E
// registers per lane, each lane fetching its entries' tags; buf itself then serves as the scratch of n_tags 16-bit counters "room
// left for this tag", loaded from the user's cap row (P * 8 >= 1024 bytes = 512 counters; no LDS beyond the buffer).  The E chunks
// are walked in order: a lane whose tag still has room counts the same-tag lanes below it among those that have room too (lane
// reads over that ballot only: a saturated tag costs nothing), is taken if that count is below the room left, and the last lane
// of a tag stores what is left after the chunk.  The taken entries are compacted in rank order, so they come out sorted, the first k_b of them.
//
// Returns the threshold: 0 until k_b entries are kept, then (at most) the smallest kept entry, below which nothing can enter this
// user's list any more (tk_caps_reach says why).  Wave-level syncs only: TkFilter::offer calls it between block barriers.
template <int P, bool FLAT = false>          // FLAT (tk_select_capped_call): the sort is inlined, so that the function holds no call
__device__ uint64_t tk_select_capped(uint64_t* buf, int& cnt, int reach, int lane, const int32_t* __restrict__ item_tag,
                                     const int32_t* __restrict__ cap_row, int n_tags, uint16_t* ttag_row = nullptr) {
    constexpr int E = P / 64;
    static_assert(P * 8 >= 2 * TK_MAX_TAGS, "the buffer holds one 16-bit counter per tag");
    const int kb = max(reach & 0xFFFF, 1);
    if (!(reach >> 16)) return tk_select<P>(buf, cnt, kb, lane);
    if constexpr (FLAT) {
        [[clang::always_inline]] tk_flush<P>(buf, __builtin_amdgcn_readfirstlane(cnt), 1, lane);
    } else tk_flush<P>(buf, __builtin_amdgcn_readfirstlane(cnt), 1, lane);          // padded with 0, sorted descending
    uint64_t v[E];
    int tg[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        v[e] = buf[64 * e + lane];
        tg[e] = -1;
        if (v[e]) {
            const int t = item_tag[tk_entry_id(v[e])];
            if ((uint32_t)t < (uint32_t)n_tags) tg[e] = t;
        }
    }
    tk_wave_sync();                                  // every entry is in a register: buf becomes the counters
    tk_u16_alias* room = reinterpret_cast<tk_u16_alias*>(buf);          // room[t]: how many more entries of tag t may be taken
    for (int t = lane; t < n_tags; t += 64) room[t] = (uint16_t)min(max(cap_row[t], 0), 0xFFFF);
    tk_wave_sync();
    bool take[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int left = tg[e] >= 0 ? (int)room[tg[e]] : 0;
        const bool live = left > 0;
        int lower = 0;
        bool last = true;
        for (unsigned long long m = __ballot(live); m; m &= m - 1) {
            const int l = __builtin_ctzll(m);
            const bool same = __builtin_amdgcn_readlane(tg[e], l) == tg[e];
            lower += (same && l < lane) ? 1 : 0;
            last = last && !(same && l > lane);
        }
        take[e] = live && lower < left;
        tk_wave_sync();
        if (live && last) room[tg[e]] = (uint16_t)(left - min(left, lower + 1));
        if (ttag_row && take[e] && lower + 1 == left) {          // the cap-th taken of its tag: one lane per tag at most
            const uint16_t key = (uint16_t)(v[e] >> 48);
            if (key > ttag_row[tg[e]]) ttag_row[tg[e]] = key;
        }
        tk_wave_sync();
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned long long m = __ballot(take[e]);
        const int pos = base + __popcll(m & below);
        if (take[e] && pos < kb) buf[pos] = v[e];     // (the counters are dead: the loop above ended on a sync)
        base += __popcll(m);
    }
    tk_wave_sync();
    cnt = min(base, kb);
    return base >= kb ? buf[kb - 1] : 0;
}

// tk_select_capped as a function of its own (REQ + CAPS kernels, which have no register to spare in their scan: the flush is a
// phase of its own, and as a call its live set stays out of the scan's).
// The count goes in and comes back by value: a reference would put it in scratch memory.
struct TkCut {
    uint64_t thr;
    int cnt;
};
// The buffer crosses the call as an LDS pointer, so that the selection keeps its LDS instructions, and the sort is inlined into it
// (FLAT): a call inside it would need a stack frame.  The threshold row stays a generic pointer, null where there is no table (a
// null pointer must not be cast between address spaces by hand); it is read and written a few times per flush.
typedef __attribute__((address_space(3))) uint64_t tk_lds_u64;
template <int P>
__device__ __noinline__ TkCut tk_select_capped_call(tk_lds_u64* buf, int cnt, int reach, int lane, const int32_t* __restrict__ item_tag,
                                                    const int32_t* __restrict__ cap_row, int n_tags, uint16_t* ttag_row) {
    const uint64_t thr = tk_select_capped<P, true>((uint64_t*)buf, cnt, reach, lane, item_tag, cap_row, n_tags, ttag_row);
    return TkCut{thr, cnt};
}

// One wave: zeroes the entries of buf[0, cnt) whose id user b excludes (ex: the block's LDS copy of its exclude ids in
// this slice, or the global list when it is longer than TK_EX_LDS).
__device__ inline void tk_drop_excluded(uint64_t* buf, int cnt, const int32_t* ex, const int64_t* xl, int n_exclude, int lane) {
    if (n_exclude == 0) return;
    for (int j = lane; j < cnt; j += 64) {
        const uint64_t e = buf[j];
        if (!e) continue;
        const int64_t id = tk_entry_id(e);
        bool out = false;
        if (ex) {
            for (int x = 0; x < n_exclude; ++x) out |= ex[x] == (int32_t)id;
        } else {
            for (int x = 0; x < n_exclude; ++x) out |= xl[x] == id;
        }
        if (out) buf[j] = 0;
    }
    tk_wave_sync();
}

// Group (or section) g of a catalogue stored group after group: rows [ptr[g], ptr[g + 1]), clamped to [0, N], so that a ptr
// that is not nondecreasing from 0 to N cannot name a row outside the catalogue.  N = 0: empty (ptr may be null).
__device__ __forceinline__ void tk_group_span(const int64_t* __restrict__ ptr, int g, int N, int& row, int& len) {
    row = 0;
    len = 0;
    if (N == 0) return;
    const long a = min((long)N, max(0L, (long)ptr[g]));
    const long e = min((long)N, max(0L, (long)ptr[g + 1]));
    row = (int)a;
    len = (int)max(0L, e - a);
}

// The wave's two 32-row tiles of a grouped or sectioned catalogue in the step that starts at tile row nw (tiles at or past
// t_end: none, len 0).  Wave-uniform.
struct TkWaveTiles {
    int row[TK_TN], len[TK_TN], grp[TK_TN];

    __device__ __forceinline__ TkWaveTiles(const TkTile* __restrict__ tiles, int t_end, int nw) {
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            const int t = nw / 32 + c;
            TkTile tl{0, 0, 0, 0};
            if (t < t_end) tl = tiles[t];
            row[c] = __builtin_amdgcn_readfirstlane(tl.row);
            len[c] = __builtin_amdgcn_readfirstlane(tl.len);
            grp[c] = __builtin_amdgcn_readfirstlane(tl.grp);
        }
    }
    // the clamped catalogue row of staged position i in [0, 64)
    __device__ __forceinline__ int row_of(int i, int N) const { return min((i < 32 ? row[0] : row[1]) + (i & 31), N - 1); }
    // is row r of column tile c a real item of the slice [.., n_end), and if so its id
    __device__ __forceinline__ bool live(int c, int nw, int n_end, int r, const int32_t* __restrict__ item_ids, uint32_t& id) const {
        const bool l = nw + 32 * c + r < n_end && r < len[c];
        if (l) id = (uint32_t)item_ids[row[c] + r];
        return l;
    }
};

// The candidate filter of a slice kernel's block: per user an LDS buffer of P entries, a threshold and a count, and the
// block's exclude ids.  Scores that beat their user's threshold are appended to the user's buffer; the exclude lists are
// applied when a buffer is cut down, so the filter is one compare per score.  A candidate that finds its user's buffer full
// stays pending in its lane (its score is still in the accumulator); the block then cuts the full buffers down to k, raises
// their thresholds and offers the pending candidates again, until none is left.
//
// Its LDS: buf [32][P] entries, thr [32] thresholds, cnt [32] counts (past P: that many candidates are pending), ex [32][64]
// staged exclude ids.  A slice kernel declares them with TK_FILTER_LDS as four separate __shared__ objects, so that the
// compiler knows they do not overlap (as one struct they cost every slice kernel 30 to 50 VGPRs).
template <int P>
struct TkFilterLds {
    uint64_t (*buf)[P];
    uint64_t* thr;
    int* cnt;
    int32_t (*ex)[TK_EX_LDS];
};
#define TK_FILTER_LDS(name, P)                 \
    __shared__ uint64_t name##_buf[TK_UT][P];  \
    __shared__ uint64_t name##_thr[TK_UT];     \
    __shared__ int name##_cnt[TK_UT];          \
    __shared__ int32_t name##_ex[TK_UT][TK_EX_LDS]; \
    const TkFilterLds<P> name{name##_buf, name##_thr, name##_cnt, name##_ex}

// Which (user, item) pairs of a step the filter may take: user(i) reads what user row i of the block contributes, item(c, w)
// tests this lane's item of column tile c against it.  Every pair, or the pairs with lo <= time < hi (WINDOW kernels: win is
// the block's 32 staged (lo, hi), tv the times of this lane's two items), or the pairs whose user allows the item's tag (TAGS
// kernels: tm[c] is the block's transposed bitmap word of this lane's item of column tile c, bit i = user row i allows its tag).
struct TkOpenAll {
    __device__ __forceinline__ int user(int) const { return 0; }
    __device__ __forceinline__ bool item(int, int) const { return true; }
};
struct TkOpenWindow {
    const int2* win;
    const int (&tv)[TK_TN];
    __device__ __forceinline__ int2 user(int i) const { return win[i]; }
    __device__ __forceinline__ bool item(int c, int2 w) const { return tv[c] >= w.x && tv[c] < w.y; }
};

struct TkOpenTags {
    const uint32_t (&tm)[TK_TN];
    __device__ __forceinline__ int user(int i) const { return i; }
    __device__ __forceinline__ bool item(int c, int i) const { return (tm[c] >> i) & 1u; }
};

// REQ kernels: TkOpenWindow AND TkOpenTags (user row i reads its window from LDS; its tag bit is tested in the register).
struct TkOpenBoth {
    TkOpenWindow w;
    TkOpenTags t;
    struct User {
        int2 win;
        int row;
    };
    __device__ __forceinline__ User user(int i) const { return User{w.user(i), t.user(i)}; }
    __device__ __forceinline__ bool item(int c, User u) const { return w.item(c, u.win) && t.item(c, u.row); }
};

template <int P, int W, class SEL = TkSelectBest>
struct TkFilter {
    TkFilterLds<P> s;
    const int64_t* __restrict__ exclude;
    int n_exclude, k, u0, B, lane, wave;
    SEL sel;          // how a full buffer is cut down (TkSelectBest: nothing to hold)

    __device__ __forceinline__ bool ex_lds() const { return n_exclude <= TK_EX_LDS; }

    // Empty buffers, and the block's exclude lists in LDS when they are short enough: only the ids in [id_lo, id_hi) matter
    // (a plain catalogue: the rows of this slice; item ids: every 31-bit id, in any slice), everything else becomes -1.  The
    // caller's next __syncthreads() publishes it.
    __device__ __forceinline__ void start(int64_t id_lo, int64_t id_hi) {
        if (threadIdx.x < TK_UT) {
            s.thr[threadIdx.x] = 0;
            s.cnt[threadIdx.x] = 0;
        }
        if (ex_lds())
            for (int i = threadIdx.x; i < TK_UT * n_exclude; i += 64 * W) {
                const int u = i / n_exclude, e = i - u * n_exclude;
                const int64_t v = u0 + u < B ? exclude[(long)(u0 + u) * n_exclude + e] : -1;
                s.ex[u][e] = (v >= id_lo && v < id_hi) ? (int32_t)v : -1;
            }
    }

    // one wave: cut user i's buffer (c entries) down to its best k (TkSelectCapped: its capped best k), excluded ids dropped;
    // returns the new threshold, sets c.  Only ever called for a user row below B.
    __device__ __forceinline__ uint64_t flush(int i, int& c) {
        tk_drop_excluded(s.buf[i], c, ex_lds() ? s.ex[i] : nullptr, exclude + (long)(u0 + i) * n_exclude, n_exclude, lane);
        if constexpr (SEL::capped) {
            if constexpr (SEL::outline) {
                const TkCut cut = tk_select_capped_call<P>((tk_lds_u64*)s.buf[i], c, sel.reach[i], lane, sel.item_tag,
                                                           sel.cap + (long)(u0 + i) * sel.n_tags, sel.n_tags,
                                                           sel.ttag ? sel.ttag + i * SEL::table : nullptr);
                c = cut.cnt;
                return cut.thr;
            } else
                return tk_select_capped<P>(s.buf[i], c, sel.reach[i], lane, sel.item_tag, sel.cap + (long)(u0 + i) * sel.n_tags,
                                           sel.n_tags, sel.ttag ? sel.ttag + i * SEL::table : nullptr);
        } else return tk_select<P>(s.buf[i], c, k, lane);
    }

    // The scores of a step that have to be offered, bit 16 c + q of the result.  C/D layout: item = lane & 31 of column tile
    // c, user row i = (q & 3) + 8 (q >> 2) + 4 (lane >> 5).  live[c]: this lane's item of tile c is a real one; open: which
    // (user, item) pairs are eligible (TkOpenAll, TkOpenWindow).  NaN scores are never offered.
    template <class Open>
    __device__ __forceinline__ uint32_t pending(const tk_f32x16 (&acc)[TK_TN], const bool (&live)[TK_TN], Open open) const {
        uint32_t pend = 0;
#pragma unroll
        for (int c = 0; c < TK_TN; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                const auto w = open.user(i);          // read ahead of the tests, not inside them
                if (live[c] && u0 + i < B && open.item(c, w) && !__builtin_isnan(acc[c][q])) pend |= 1u << (16 * c + q);
            }
        return pend;
    }

    // CURSOR kernels: of the pending scores, those whose entry lies strictly below their user's cursor key (cur: the block's 32
    // keys, tk_cursor_stage): one 64-bit compare per pending score, on the entry the offer forms from the same score and id.
    template <class IdOf>
    __device__ __forceinline__ uint32_t after(const tk_f32x16 (&acc)[TK_TN], uint32_t pend, const uint64_t* cur, IdOf id_of) const {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint64_t key = cur[(q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)];          // read ahead of the tests, not inside them
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) {
                const uint32_t bit = 1u << (16 * c + q);
                if ((pend & bit) && !(tk_entry(acc[c][q], id_of(c)) < key)) pend &= ~bit;
            }
        }
        return pend;
    }

    // CAPS kernels: of the pending scores, those that do not lie below their (user, tag) threshold (TkSelectCapped; tag_of(c): the
    // tag of this lane's item in column tile c).  One 16-bit LDS read and one compare per score, on the upper half of the score key
    // the offer's entry will carry.  A threshold a flush raises during this step's offer is seen from the next step on.
    template <class TagOf>
    __device__ __forceinline__ uint32_t above_tags(const tk_f32x16 (&acc)[TK_TN], uint32_t pend, TagOf tag_of) const {
        if (!sel.ttag) return pend;
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            const uint16_t* row = sel.ttag + tag_of(c);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const uint16_t t = row[((q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)) * SEL::table];          // read ahead of the tests
                const uint32_t bit = 1u << (16 * c + q);
                if ((pend & bit) && (uint16_t)(tk_score_key(acc[c][q]) >> 16) < t) pend &= ~bit;
            }
        }
        return pend;
    }

    // Offers the pending scores of a step; id_of(c): the id of this lane's item in column tile c.  This holds block barriers:
    // EVERY wave of the block calls it on EVERY step, with pend == 0 when it has nothing to offer (a wave past the slice's
    // end, a WINDOW or TAGS wave that skipped its chain), so that all waves meet the same barriers the same number of times.
    template <class IdOf>
    __device__ __forceinline__ void offer(const tk_f32x16 (&acc)[TK_TN], uint32_t pend, IdOf id_of) {
        bool first = true;
        while (__syncthreads_or(pend != 0)) {
            if (!first) {
                // cut every full buffer down to its best k (cnt may have run past P: those candidates are pending)
                for (int i = wave; i < TK_UT; i += W) {
                    if (s.cnt[i] >= P) {
                        int c = P;
                        const uint64_t t = flush(i, c);
                        if (lane == 0) {
                            s.thr[i] = t;
                            s.cnt[i] = c;
                        }
                    }
                }
                __syncthreads();
            }
            first = false;
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint32_t bit = 1u << (16 * c + q);
                    if (!(pend & bit)) continue;
                    const int i = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                    const uint64_t e = tk_entry(acc[c][q], id_of(c));
                    bool keep = false;
                    if (e > s.thr[i]) {
                        const int slot = atomicAdd(&s.cnt[i], 1);
                        if (slot < P) s.buf[i][slot] = e;
                        else keep = true;
                    }
                    if (!keep) pend &= ~bit;
                }
            }
        }
    }

    // The slice's list of every user of the block: its best k, unsorted, 0-padded, at ws[user][slice of S][k].
    __device__ __forceinline__ void write(uint64_t* __restrict__ ws, int S, int slice) {
        for (int i = wave; i < TK_UT; i += W) {
            const int b = u0 + i;
            if (b >= B) break;
            int c = min(s.cnt[i], P);
            flush(i, c);
            uint64_t* dst = ws + ((long)b * S + slice) * k;
            for (int j = lane; j < k; j += 64) dst[j] = j < c ? s.buf[i][j] : 0;
        }
    }
};

// Per block: users [u0, u0 + 32) x items [n_begin, n_end) of slice blockIdx.y, 64 W items per step (two 32-item column
// tiles per wave): tk_chain (topk_entry.h) forms the scores from the block's 32 user rows and the wave's 64 item rows, and
// they go through the block's TkFilter.  The block writes one k-list per (user, slice).
//
// GROUPED (nrms_topk_grouped_dot): the slices run over the tiles of `tiles` (32 rows each, slice_len and IT are whole tiles),
// user = the query [B, G, d], and each of a wave's two column tiles takes its A operand from query[user, the tile's group];
// rows past a tile's len are masked, and the id of row n is item_ids[n].
//
// NOISE (nrms_softmax_sample_dot): before the filter every accumulator element becomes its perturbed key
// fmaf(score, inv_temperature, g(row key, item)); the block's 32 row seeds are formed once, in LDS.
//
// BIAS (nrms_topk_dot_biased): lane (r, h) loads bias[n] of its item in each of its two column tiles (one coalesced 128-byte
// read per tile, issued before the chain so that it hides the latency) and, before the filter, adds it to the tile's 16
// finished accumulator registers: one fp32 add per score, after the chain, never folded into it.  A NaN sum fails the filter's
// NaN test like a NaN score; entries simply carry s'.
//
// WINDOW (nrms_topk_dot_windowed; with or without BIAS): the block stages its 32 users' (lo, hi) in LDS once and forms their
// hull [blo, bhi).  Lane (r, h) loads item_time[n] of its item in each of its two column tiles where bv[] is loaded, and the
// filter takes (user, item) only if lo <= time < hi (hi <= INT32_MAX, so a time of INT32_MAX is open to nobody).  Dead-tile
// skip: one __ballot over "my item's time lies in [blo, bhi)" decides, wave-uniformly, whether the wave has anything to offer
// in this step; if not it issues no item loads, no LDS staging and no MFMA and goes to the filter's offer with pend == 0.  The
// skipped region holds the chain alone, which touches only the wave's private stage[wave] and wave-level syncs: every wave
// still meets every block barrier, the same number of times.
//
// CURSOR (nrms_topk_dot_after, the later pages of nrms_topk_dot_deep; with or without BIAS and WINDOW): the block stages its 32
// users' cursors once, as 64-bit keys in LDS (tk_cursor_stage), and a pending score is offered only if its entry, formed from s'
// where there is a prior, lies strictly below its user's key (TkFilter::after).  Everything else is the uncursored kernel's.
// All-END exit: a block whose 32 keys are all 0 writes its empty slice lists and returns before its first item row; the test
// reads LDS after a barrier, so it is block-uniform and no wave is left waiting at a later barrier.
//
// TAGS (nrms_topk_dot_tagged; with or without BIAS): the block builds, once, the transposed bitmap ubt[t] of its 32 users' tag
// sets in LDS (tk_tags_stage: bit i of ubt[t] = user u0 + i allows tag t; n_tags words, at most 2 KB).  Lane (r, h) loads
// item_tag[n] of its item in each of its two column tiles where bv[] is loaded and reads ONE LDS word per item, tm[c] =
// ubt[tag] (0 for a tag outside [0, n_tags) and for a row past the slice); the filter takes (user i, item) iff bit i of tm[c] is
// set, a register test, not 32 LDS reads per score.  Dead-wave skip: __ballot(tm[0] | tm[1]) == 0, wave-uniform, under exactly the
// WINDOW skip's barrier discipline: the skipping wave still calls offer with pend == 0.
//
// CAPS (nrms_topk_dot_capped; with or without BIAS): the TAGS form with two differences.  The bitmap is built from cap > 0
// (tk_caps_stage), so a closed tag costs the same register bit test and a wave whose 64 items are closed to its whole block still
// skips its chain; and the filter cuts a full buffer down with tk_select_capped instead of tk_select (TkSelectCapped), whose k_b per
// user the block forms once in LDS (32 ints; tk_caps_reach), and which raises the block's 16-bit tag thresholds (TkSelectCapped)
// that above_tags() tests before the offer.  The slice lists are capped lists of at most k entries, and
// topk_merge_capped_kernel runs the same selection over them.
//
// ADJ (nrms_topk_dot_adjusted; with or without BIAS): the block compacts, once, the slots of its 32 users that name a row of its
// slice into an LDS list of 32-bit words (tk_adjust_stage; tk_adjust_cap(P) of them fit beside the P class's buffers, and a block
// whose slots overflow the list walks the global lists instead, dropping none).  Per step a wave marks its 64 items' hits in its
// private LDS row of 32-bit user masks (tk_adjust_mark), and the lane that holds a marked pair reads the delta of the pair's
// LOWEST slot from global memory and adds it to its accumulator register (tk_adjust_apply): one fp32 add on the finished s',
// after the prior's, before pend is formed, so a boosted score below its user's threshold is offered and no entry is adjusted
// twice.  A block none of whose slots names a row of its slice reads nothing per step.  A NaN sum fails the filter's NaN test.
//
// REQ (nrms_topk_dot_request; with or without BIAS): WINDOW, TAGS, ADJ and CURSOR in one form, for a request that holds two or more of
// them.  The pack's one member is a TkRequest; every part's LDS is declared, and a part whose pointer is null (a kernel argument, so
// the branch is uniform over the block) stages nothing, loads nothing per step and is not tested.  The open predicate is TkOpenBoth,
// the window's AND the tag set's (TkOpenTags alone without a window; tm[c] is all ones for a real item where there is no tag set).
// The wave is dead when the window hull OR the tag bitmap closes its 64 items to the whole block, each decided by a ballot of its own,
// so a stretch closed half by the one and half by the other is not skipped: the filter refuses its scores.  The delta is added after
// the prior's and before pend, the cursor's compare follows, on s''.  The staged slot list holds tk_request_adjust_cap(P) words: at
// P = 512 half of the ADJ form's, which pays for the bitmap, the windows and the cursor keys beside it.  Only topkrequest.hip
// instantiates these kernels, and one family serves every subset of the parts.
//
// REQ + CAPS (nrms_topk_dot_request_capped; with or without BIAS): the pack holds a TkRequest AND a TkCaps, the one pair of members
// that is allowed.  It is the REQ form with the CAPS differences: the bitmap is always built, from (cap > 0) & allow (cap > 0 alone
// where there is no tag set; tk_tags_stage with a TkCaps); the tag of every item is kept for above_tags(), which runs on s'', after
// the prior's add, tk_adjust_apply and the cursor's compare; the filter cuts a full buffer down with tk_select_capped, as a call
// (tk_select_capped_call: these kernels have no register to spare in their scan), with tk_caps_reach's k_b; the thresholds take the
// LDS the request's parts leave free (tk_request_caps_table: none at P = 512).  Both statements that make one scan exact, C(S1 u S2)
// = C(C(S1) u C(S2)) and the k_b threshold, are about a set of eligible items under a total order and do not ask which filters made
// the set, so the slice lists are capped lists of s'' entries and topk_merge_capped_kernel merges them unchanged.  Only
// topkrequestcaps.hip instantiates these kernels.
//
// The window's two pointers are a kernel argument of the WINDOW instantiations alone, the adjustments' of the ADJ instantiations alone, the cursor's of the CURSOR instantiations
// alone, the tag set's of the TAGS instantiations alone and the caps' of the CAPS instantiations alone (WIN holds a TkWindow, a
// TkCursor, both in that order, a TkTags, a TkCaps, or nothing; CURSOR, TAGS and CAPS are read off the pack), so every other instantiation keeps its name, its signature and its kernarg
// layout.
template <int P, int W, bool VEC, bool GROUPED, bool NOISE, bool BIAS, bool WINDOW, class... WIN>
__global__ __launch_bounds__(64 * W) void topk_slice_kernel(int B, int N, int d, int k, int slice_len, int S,
                                                            const float* __restrict__ user, const float* __restrict__ items,
                                                            const int64_t* __restrict__ exclude, int n_exclude,
                                                            uint64_t* __restrict__ ws, int G, int n_tiles,
                                                            const TkTile* __restrict__ tiles,
                                                            const int32_t* __restrict__ item_ids, TkNoise noise,
                                                            const float* __restrict__ bias, WIN... win_arg) {
    constexpr bool CURSOR = (std::is_same<WIN, TkCursor>::value || ...);
    constexpr bool TAGS = (std::is_same<WIN, TkTags>::value || ...);
    constexpr bool CAPS = (std::is_same<WIN, TkCaps>::value || ...);
    constexpr bool ADJ = (std::is_same<WIN, TkAdjust>::value || ...);
    constexpr bool REQ = (std::is_same<WIN, TkRequest>::value || ...);
    static_assert(sizeof...(WIN) == (WINDOW ? 1 : 0) + (CURSOR ? 1 : 0) + (TAGS ? 1 : 0) + (CAPS ? 1 : 0) + (ADJ ? 1 : 0) + (REQ ? 1 : 0),
                  "WINDOW kernels take one TkWindow, CURSOR kernels one TkCursor, TAGS kernels one TkTags, CAPS kernels one TkCaps, "
                  "ADJ kernels one TkAdjust, REQ kernels one TkRequest, the others none");
    static_assert(!(REQ && (GROUPED || NOISE || WINDOW || CURSOR || TAGS || ADJ)),
                  "a request holds its window, tag set, adjustments and cursor itself, over the plain and the biased top-k only; the "
                  "one member it pairs with is a TkCaps (nrms_topk_dot_request_capped)");
    static_assert(!(ADJ && (GROUPED || NOISE || WINDOW || CURSOR || TAGS || CAPS)), "the adjustments are for the plain and the biased top-k only");
    static_assert(!(CAPS && (GROUPED || NOISE || WINDOW || CURSOR || TAGS)), "the tag caps are for the plain and the biased top-k only");
    static_assert(!(TAGS && (GROUPED || NOISE || WINDOW || CURSOR)), "the tag set is for the plain and the biased top-k only");
    const TkWindow win = tk_window_arg(win_arg...);
    static_assert(!(NOISE && GROUPED), "the perturbation is keyed by the item's row");
    static_assert(!(WINDOW && (GROUPED || NOISE)), "the window is for the plain and the biased top-k only");
    static_assert(!(BIAS && (GROUPED || NOISE)), "the prior is for the plain top-k only");
    static_assert(!(CURSOR && (GROUPED || NOISE)), "the cursor is for the plain, the biased and the windowed top-k only");
    TK_FILTER_LDS(lds, P);
    __shared__ uint64_t rseed[NOISE ? TK_UT : 1];
    __shared__ __attribute__((aligned(16))) float stage[W][64 * TK_BP];
    constexpr int IT = 64 * W;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u0 = blockIdx.x * TK_UT;
    const int slice = blockIdx.y;
    const int n_begin = slice * slice_len;
    const int n_end = min(GROUPED ? 32 * n_tiles : N, n_begin + slice_len);      // (grouped: tile rows, not catalogue rows)
    constexpr int TT = REQ ? tk_request_caps_table(P) : tk_caps_table(P);
    TkFilter<P, W, std::conditional_t<CAPS, TkSelectCapped<TT, REQ>, TkSelectBest>> flt{lds, exclude, n_exclude, k, u0, B, lane, wave};
    int2* wwin = nullptr;          // WINDOW: the block's 32 (lo, hi)
    if constexpr (WINDOW) {
        __shared__ int2 wwin_lds[TK_UT];
        wwin = wwin_lds;
        tk_window_stage(wwin, win.window, u0, B);
    }
    uint64_t* cur = nullptr;       // CURSOR: the block's 32 cursor keys
    if constexpr (CURSOR) {
        __shared__ uint64_t cur_lds[TK_UT];
        cur = cur_lds;
        tk_cursor_stage(cur, tk_pack_arg<TkCursor>(win_arg...), u0, B);
    }
    uint32_t* ubt = nullptr;       // TAGS: the block's transposed tag bitmap
    [[maybe_unused]] int n_tags = 0;
    [[maybe_unused]] const int32_t* item_tag = nullptr;
    if constexpr (TAGS) {
        __shared__ uint32_t ubt_lds[TK_MAX_TAGS];
        ubt = ubt_lds;
        const TkTags tags = tk_pack_arg<TkTags>(win_arg...);
        n_tags = tags.n_tags;
        item_tag = tags.item_tag;
        tk_tags_stage(ubt, tags, u0, B, 64 * W);
    }
    if constexpr (CAPS && !REQ) {          // the bitmap of the tags with cap > 0, the block's 32 k_b and its tag thresholds
        __shared__ uint32_t ubt_lds[TK_MAX_TAGS];
        __shared__ int reach_lds[TK_UT];
        __shared__ uint16_t ttag_lds[TK_UT * TT];
        for (int i = threadIdx.x; i < TK_UT * TT; i += 64 * W) ttag_lds[i] = 0;
        ubt = ubt_lds;
        const TkCaps caps = tk_pack_arg<TkCaps>(win_arg...);
        n_tags = caps.n_tags;
        item_tag = caps.item_tag;
        tk_caps_stage(ubt, caps, u0, B, 64 * W);
        for (int i = wave; i < TK_UT; i += W) {
            const int kb = u0 + i < B ? tk_caps_reach(caps.cap + (long)(u0 + i) * n_tags, n_tags, k, lane) : 0;
            if (lane == 0) reach_lds[i] = kb;
        }
        flt.sel = TkSelectCapped<TT>{caps.item_tag, caps.cap, n_tags, reach_lds, n_tags <= TT ? ttag_lds : nullptr};
    }
    constexpr int AC = REQ ? tk_request_adjust_cap(P) : tk_adjust_cap(P);
    [[maybe_unused]] TkAdjust adj{nullptr, nullptr, 0};
    [[maybe_unused]] uint32_t* axl = nullptr;       // ADJ: the block's staged slots, their count and one row of marks per wave
    [[maybe_unused]] int* axl_n = nullptr;
    [[maybe_unused]] uint32_t* axm = nullptr;
    if constexpr (ADJ) {
        __shared__ uint32_t axl_lds[AC];
        __shared__ int axl_n_lds;
        __shared__ uint32_t axm_lds[W][64];
        axl = axl_lds;
        axl_n = &axl_n_lds;
        axm = axm_lds[wave];
        adj = tk_pack_arg<TkAdjust>(win_arg...);
        if (threadIdx.x == 0) axl_n_lds = 0;
        for (int i = threadIdx.x; i < 64 * W; i += 64 * W) axm_lds[i / 64][i % 64] = 0;
        __syncthreads();
        tk_adjust_stage<AC>(axl, axl_n, adj, u0, B, n_begin, n_end, 64 * W);
    }
    [[maybe_unused]] TkRequest req{};
    if constexpr (REQ) {           // every part's LDS is there, a part that is absent (a null pointer, block-uniform) stages nothing
        __shared__ int2 wwin_lds[TK_UT];
        __shared__ uint64_t cur_lds[TK_UT];
        __shared__ uint32_t ubt_lds[TK_MAX_TAGS];
        __shared__ uint32_t axl_lds[AC];
        __shared__ int axl_n_lds;
        __shared__ uint32_t axm_lds[W][64];
        req = tk_pack_arg<TkRequest>(win_arg...);
        if (req.win.window) {
            wwin = wwin_lds;
            tk_window_stage(wwin, req.win.window, u0, B);
        }
        if (req.cur.after_ids) {
            cur = cur_lds;
            tk_cursor_stage(cur, req.cur, u0, B);
        }
        if constexpr (CAPS) {      // REQ + CAPS: the bitmap of (cap > 0) & allow (allow null: cap > 0), the 32 k_b, the thresholds that fit
            __shared__ int reach_lds[TK_UT];
            __shared__ uint16_t ttag_lds[TT > 0 ? TK_UT * TT : 1];
            for (int i = threadIdx.x; i < TK_UT * TT; i += 64 * W) ttag_lds[i] = 0;
            const TkCaps caps = tk_pack_arg<TkCaps>(win_arg...);
            ubt = ubt_lds;
            n_tags = caps.n_tags;
            item_tag = caps.item_tag;
            tk_tags_stage(ubt, req.tags, caps, u0, B, 64 * W);
            for (int i = wave; i < TK_UT; i += W) {
                const int kb = u0 + i < B ? tk_caps_reach(caps.cap + (long)(u0 + i) * n_tags, n_tags, k, lane) : 0;
                if (lane == 0) reach_lds[i] = kb;
            }
            flt.sel = TkSelectCapped<TT, true>{caps.item_tag, caps.cap, n_tags, reach_lds, TT > 0 && n_tags <= TT ? ttag_lds : nullptr};
        } else if (req.tags.allow) {
            ubt = ubt_lds;
            n_tags = req.tags.n_tags;
            item_tag = req.tags.item_tag;
            tk_tags_stage(ubt, req.tags, u0, B, 64 * W);
        }
        if (req.adj.adj_ids) {
            axl = axl_lds;
            axl_n = &axl_n_lds;
            axm = axm_lds[wave];
            adj = req.adj;
            if (threadIdx.x == 0) axl_n_lds = 0;
            for (int i = threadIdx.x; i < 64 * W; i += 64 * W) axm_lds[i / 64][i % 64] = 0;
            __syncthreads();
            tk_adjust_stage<AC>(axl, axl_n, adj, u0, B, n_begin, n_end, 64 * W);
        }
    }
    if constexpr (NOISE) {
        if (threadIdx.x < TK_UT) rseed[threadIdx.x] = tk_noise_row_seed(noise.seed, (uint64_t)noise.row_key[min(u0 + (int)threadIdx.x, B - 1)]);
    }
    if constexpr (GROUPED) flt.start(0, 0x80000000L);
    else flt.start(n_begin, n_end);
    __syncthreads();
    if constexpr (CAPS) {          // a block none of whose users rations a tag needs no tag thresholds: it runs as the TAGS kernel does
        int any = 0;
        for (int u = 0; u < TK_UT; ++u) any |= flt.sel.reach[u] >> 16;
        if (!any) flt.sel.ttag = nullptr;
    }
    [[maybe_unused]] int n_axl = 0;
    if constexpr (ADJ) n_axl = *axl_n;
    int blo = 0, bhi = 0;
    if constexpr (WINDOW) tk_window_hull(wwin, blo, bhi);
    if constexpr (CURSOR) {
        if (TK_CURSOR_EXIT && tk_cursor_all_end(cur)) {
            flt.write(ws, S, slice);
            return;
        }
    }
    if constexpr (REQ) {
        if (adj.adj_ids) n_axl = *axl_n;
        if (wwin) tk_window_hull(wwin, blo, bhi);
        if (cur && TK_CURSOR_EXIT && tk_cursor_all_end(cur)) {
            flt.write(ws, S, slice);
            return;
        }
    }

    const int r = lane & 31, h = lane >> 5;
    constexpr int NA = GROUPED ? TK_TN : 1;           // A operands per k-block: one per column tile when grouped
    const float* arow[NA];
    if constexpr (!GROUPED) arow[0] = user + (long)min(u0 + r, B - 1) * d;
    float* st = stage[wave];
    for (int n0 = n_begin; n0 < n_end; n0 += IT) {
        const int nw = n0 + 64 * wave;
        tk_f32x16 acc[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
        const TkWaveTiles tl(tiles, GROUPED ? n_tiles : 0, nw);          // grouped only
        if constexpr (GROUPED) {
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) arow[c] = user + ((long)min(u0 + r, B - 1) * G + tl.grp[c]) * d;
        }
        float bv[BIAS ? TK_TN : 1] = {};          // BIAS: loaded here so that the chain hides the latency, added after it
        if constexpr (BIAS) {
            if (nw < n_end) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) bv[c] = bias[min(nw + 32 * c + r, N - 1)];
            }
        }
        int tv[WINDOW || REQ ? TK_TN : 1] = {};         // WINDOW: the time of this lane's item in column tile c
        bool dead = false;                       // WINDOW, TAGS: no item of this wave's step is open to any user of the block (wave-uniform)
        if constexpr (WINDOW) {
            if (nw < n_end) {
                bool any = false;
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) {
                    const int n = nw + 32 * c + r;
                    tv[c] = win.item_time[min(n, N - 1)];
                    any |= n < n_end && tv[c] >= blo && tv[c] < bhi;
                }
                dead = TK_WINDOW_SKIP && __ballot(any) == 0;
            }
        }
        [[maybe_unused]] int tgv[CAPS ? TK_TN : 1] = {};        // CAPS: the tag of this lane's item of column tile c (0 where tm[c] is 0)
        uint32_t tm[TAGS || CAPS || REQ ? TK_TN : 1] = {};      // TAGS, CAPS: the block's users that this lane's item of column tile c is open to
        if constexpr ((TAGS || CAPS) && !REQ) {          // (REQ + CAPS: the REQ block below loads the tags)
            if (nw < n_end) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) {
                    const int n = nw + 32 * c + r;
                    const int tg = item_tag[min(n, N - 1)];
                    const uint32_t m = tk_tags_mask(ubt, tg, n_tags);
                    tm[c] = n < n_end ? m : 0u;
                    if constexpr (CAPS) tgv[c] = (uint32_t)tg < (uint32_t)n_tags ? tg : 0;
                }
                dead = TK_TAGS_SKIP && __ballot((tm[0] | tm[1]) != 0) == 0;
            }
        }
        if constexpr (REQ) {          // the window's and the tag set's loads and skips, each only where the part is there: the wave is dead
                                      // when the hull OR the bitmap closes all its 64 items to the whole block
            if (nw < n_end) {
                if (wwin) {
                    bool any = false;
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) {
                        const int n = nw + 32 * c + r;
                        tv[c] = req.win.item_time[min(n, N - 1)];
                        any |= n < n_end && tv[c] >= blo && tv[c] < bhi;
                    }
                    dead = TK_WINDOW_SKIP && __ballot(any) == 0;
                }
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) tm[c] = nw + 32 * c + r < n_end ? ~0u : 0u;
                if (ubt) {
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) {
                        const int tg = item_tag[min(nw + 32 * c + r, N - 1)];
                        tm[c] &= tk_tags_mask(ubt, tg, n_tags);
                        if constexpr (CAPS) tgv[c] = (uint32_t)tg < (uint32_t)n_tags ? tg : 0;
                    }
                    dead = dead || (TK_TAGS_SKIP && __ballot((tm[0] | tm[1]) != 0) == 0);
                }
            }
        }
        if (nw < n_end && (!GROUPED || tl.len[0] + tl.len[1] > 0) && !((WINDOW || TAGS || CAPS || REQ) && dead)) {
            if constexpr (GROUPED) tk_chain<VEC>(acc, arow, items, d, st, lane, [&](int i) { return tl.row_of(i, N); });
            else tk_chain<VEC>(acc, arow, items, d, st, lane, [&](int i) { return min(nw + i, N - 1); });
        }
        if constexpr (NOISE) {
            if (nw < n_end) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint64_t rs = rseed[(q & 3) + 8 * (q >> 2) + 4 * h];
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c)
                        acc[c][q] = __builtin_fmaf(acc[c][q], noise.inv_temperature, tk_gumbel(tk_noise_word(rs, (uint32_t)(nw + 32 * c + r))));
                }
            }
        }
        if constexpr (BIAS) {
            if (nw < n_end) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[c][q] = acc[c][q] + bv[c];
            }
        }
        if constexpr (ADJ) {          // after the prior's add, before pend is formed: the filter sees s''
            if (nw < n_end) {
                uint32_t am[TK_TN];
                tk_adjust_mark<AC>(am, axm, axl, n_axl, adj, u0, B, n_begin, nw, n_end, lane);
                tk_adjust_apply(acc, am, adj, u0, nw, lane);
            }
        }
        if constexpr (REQ) {          // the ADJ step, where there are adjustments and the wave has scores
            if (nw < n_end && adj.adj_ids && !dead) {
                uint32_t am[TK_TN];
                tk_adjust_mark<AC>(am, axm, axl, n_axl, adj, u0, B, n_begin, nw, n_end, lane);
                tk_adjust_apply(acc, am, adj, u0, nw, lane);
            }
        }
        bool live[TK_TN];
        uint32_t id[TK_TN] = {};            // the id of this lane's item in column tile c
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            if constexpr (GROUPED) live[c] = tl.live(c, nw, n_end, r, item_ids, id[c]);
            else {
                id[c] = (uint32_t)(nw + 32 * c + r);
                live[c] = nw + 32 * c + r < n_end && !((WINDOW || TAGS || CAPS || REQ) && dead);       // a skipped wave's accumulators hold no score
            }
        }
        uint32_t pend;
        if constexpr (REQ) {
            if (wwin) pend = flt.pending(acc, live, TkOpenBoth{TkOpenWindow{wwin, tv}, TkOpenTags{tm}});
            else pend = flt.pending(acc, live, TkOpenTags{tm});          // (no tag set: tm is all ones for a real item)
            if (cur) pend = flt.after(acc, pend, cur, [&](int c) { return id[c]; });
        } else if constexpr (WINDOW) pend = flt.pending(acc, live, TkOpenWindow{wwin, tv});
        else if constexpr (TAGS || CAPS) pend = flt.pending(acc, live, TkOpenTags{tm});
        else pend = flt.pending(acc, live, TkOpenAll{});
        if constexpr (CURSOR) pend = flt.after(acc, pend, cur, [&](int c) { return id[c]; });
        if constexpr (CAPS) pend = flt.above_tags(acc, pend, [&](int c) { return tgv[c]; });
        // unconditional: the offer holds the block's barriers, and a wave with pend == 0 has to meet them too
        flt.offer(acc, pend, [&](int c) { return id[c]; });
    }
    flt.write(ws, S, slice);
}

// One wave: the best k of src[0, total) (entries of slice lists, 0 = padding), sorted at the end in buf[0, P), P >= k + 64;
// their scores (-inf for padding; `scores` may be null) and ids (-1 for padding) go to scores[0, k) and ids[0, k).
template <int P>
__device__ __forceinline__ void tk_merge(uint64_t* buf, const uint64_t* __restrict__ src, long total, int k, int lane,
                                         float* __restrict__ scores, int64_t* __restrict__ ids) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt = 0;
    uint64_t thr = 0;
    for (long c0 = 0; c0 < total; c0 += 64) {
        const long c = c0 + lane;
        const uint64_t e = c < total ? src[c] : 0;
        const bool take = e > thr;
        const unsigned long long m = __ballot(take);
        if (take) buf[cnt + __popcll(m & below)] = e;
        cnt += __popcll(m);
        if (cnt + 64 > P) {
            tk_wave_sync();
            thr = tk_select<P>(buf, cnt, k, lane);
        }
    }
    tk_wave_sync();
    tk_flush<P>(buf, cnt, k, lane);
    for (int j = lane; j < k; j += 64) {
        const uint64_t e = buf[j];
        if (scores) scores[j] = e ? tk_entry_score(e) : -__builtin_huge_valf();
        ids[j] = e ? tk_entry_id(e) : -1;
    }
}

// One wave per user: the best k of the user's S slice lists, written to row b of outputs whose rows are out_stride >= k elements
// apart (k: a [B, k] result; K: columns [c0, c0 + k) of a [B, K] one, the pointers already at column c0).  top_scores may be null.
template <int P>
__global__ __launch_bounds__(64) void topk_merge_kernel(int B, int k, int S, const uint64_t* __restrict__ ws,
                                                        float* __restrict__ top_scores, int64_t* __restrict__ top_ids,
                                                        int out_stride) {
    __shared__ uint64_t buf[P];
    const long b = blockIdx.x;
    tk_merge<P>(buf, ws + b * S * k, (long)S * k, k, threadIdx.x, top_scores ? top_scores + b * out_stride : nullptr,
                top_ids + b * out_stride);
}

// One wave per user: tk_merge with the capped selection (CAPS: nrms_topk_dot_capped).  The user's S slice lists are capped lists;
// the capped list of their union is the capped list of the catalogue (C(S1 u S2) = C(C(S1) u C(S2))).  The last selection leaves at
// most k entries, which are sorted and written like tk_merge's.
template <int P>
__global__ __launch_bounds__(64) void topk_merge_capped_kernel(int B, int k, int S, const uint64_t* __restrict__ ws, TkCaps caps,
                                                               float* __restrict__ top_scores, int64_t* __restrict__ top_ids) {
    __shared__ uint64_t buf[P];
    const long b = blockIdx.x;
    const int lane = threadIdx.x;
    const int32_t* cap_row = caps.cap + b * caps.n_tags;
    const int reach = tk_caps_reach(cap_row, caps.n_tags, k, lane);
    const uint64_t* src = ws + b * S * k;
    const long total = (long)S * k;
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt = 0;
    uint64_t thr = 0;
    for (long c0 = 0; c0 < total; c0 += 64) {
        const long c = c0 + lane;
        const uint64_t e = c < total ? src[c] : 0;
        const bool take = e > thr;
        const unsigned long long m = __ballot(take);
        if (take) buf[cnt + __popcll(m & below)] = e;
        cnt += __popcll(m);
        if (cnt + 64 > P) {
            tk_wave_sync();
            thr = tk_select_capped<P>(buf, cnt, reach, lane, caps.item_tag, cap_row, caps.n_tags);
        }
    }
    tk_wave_sync();
    tk_select_capped<P>(buf, cnt, reach, lane, caps.item_tag, cap_row, caps.n_tags);
    tk_flush<P>(buf, cnt, k, lane);
    for (int j = lane; j < k; j += 64) {
        const uint64_t e = buf[j];
        top_scores[b * k + j] = e ? tk_entry_score(e) : -__builtin_huge_valf();
        top_ids[b * k + j] = e ? tk_entry_id(e) : -1;
    }
}

static TkGeom topk_geom(int32_t B, int64_t N) { return tk_geom(B, N, true); }

static bool topk_args_ok(int32_t B, int64_t N, int32_t d, int32_t k) {
    return B >= 0 && N >= 0 && N <= TK_MAX_N && d >= 1 && k >= 1 && k <= TK_MAX_K;
}

// Both kernels of one call.  GROUPED: `user` is the query [B, G, d], the slices run over the tile rows of `tiles`.  NOISE: the
// perturbation of nrms_softmax_sample_dot.  Neither (the plain top-k): a non-null bias ([N] fp32) selects the BIAS
// instantiations, a non-null window the WINDOW ones, a cursor with non-null after_ids the CURSOR ones.  out_stride: the row
// pitch of top_scores / top_ids in elements (0: k).
template <bool GROUPED, bool NOISE>
static int topk_launch(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G, int64_t n_tiles, const float* user,
                       const float* items, const int32_t* item_ids, const TkTile* tiles, const int64_t* exclude, int32_t n_exclude,
                       float* top_scores, int64_t* top_ids, uint64_t* ws, hipStream_t s, const char* who,
                       TkNoise noise = TkNoise{nullptr, 0.0f, 0}, const float* bias = nullptr,
                       TkWindow win = TkWindow{nullptr, nullptr}, TkCursor cur = TkCursor{nullptr, nullptr, 0},
                       int32_t out_stride = 0) {
    const TkGeom g = topk_geom(B, GROUPED ? 32 * n_tiles : N);
    int rc = NRMS_OK;
    char what[64];
    tk_with_pw(k, [&](auto P, auto W) {
        constexpr int p = decltype(P)::value, w = decltype(W)::value;
        if (g.S > 0) {
            const dim3 grid(g.tiles, g.S), block(64 * w);
            const int n = (int)N, nt = (int)n_tiles;
            tk_with_flags([&](auto V, auto BI, auto WI, auto CU) {
                constexpr bool v = decltype(V)::value, bi = decltype(BI)::value, wi = decltype(WI)::value, cu = decltype(CU)::value;
                if constexpr (cu) {
                    if constexpr (wi && !GROUPED && !NOISE)
                        hipLaunchKernelGGL((topk_slice_kernel<p, w, v, false, false, bi, true, TkWindow, TkCursor>), grid, block, 0, s, B,
                                           n, d, k, g.slice_len, g.S, user, items, exclude, n_exclude, ws, G, nt, tiles, item_ids, noise,
                                           bias, win, cur);
                    else if constexpr (!GROUPED && !NOISE)
                        hipLaunchKernelGGL((topk_slice_kernel<p, w, v, false, false, bi, false, TkCursor>), grid, block, 0, s, B, n, d, k,
                                           g.slice_len, g.S, user, items, exclude, n_exclude, ws, G, nt, tiles, item_ids, noise, bias, cur);
                } else if constexpr (wi && !GROUPED && !NOISE)
                    hipLaunchKernelGGL((topk_slice_kernel<p, w, v, false, false, bi, true, TkWindow>), grid, block, 0, s, B, n, d, k,
                                       g.slice_len, g.S, user, items, exclude, n_exclude, ws, G, nt, tiles, item_ids, noise, bias, win);
                else if constexpr (!wi && (!bi || (!GROUPED && !NOISE)))
                    hipLaunchKernelGGL((topk_slice_kernel<p, w, v, GROUPED, NOISE, bi, false>), grid, block, 0, s, B, n, d, k,
                                       g.slice_len, g.S, user, items, exclude, n_exclude, ws, G, nt, tiles, item_ids, noise, bias);
            }, tk_vec_ok(d, user, items), bias != nullptr, win.window != nullptr, cur.after_ids != nullptr);
            snprintf(what, sizeof what, "%s(slices)", who);
            rc = check_launch(what);
            if (rc != NRMS_OK) return;
        }
        hipLaunchKernelGGL(topk_merge_kernel<p>, dim3(B), dim3(64), 0, s, B, k, g.S, ws, top_scores, top_ids,
                           out_stride ? out_stride : k);
        snprintf(what, sizeof what, "%s(merge)", who);
        rc = check_launch(what);
    });
    return rc;
}

}  // namespace nrms
