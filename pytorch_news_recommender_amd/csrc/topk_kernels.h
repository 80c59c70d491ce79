// The kernels of the catalogue selections and their launcher (topk.hip, whose head comment describes them: nrms_topk_dot and
// nrms_topk_grouped_dot; softmaxsample.hip: nrms_softmax_sample_dot, the same slices and merge with a keyed Gumbel perturbation
// added to every score before it meets the threshold).
#pragma once
#include "topk_entry.h"      // the entry, the tile constants and the helpers rankdot.hip shares

namespace nrms {

constexpr int TK_EX_LDS = 64;                  // exclude lists up to this long are staged in LDS, longer ones read globally
constexpr int TK_MAX_K = 256;
constexpr int TK_MIN_SLICE = 4 * TK_IT;        // no slice shorter than this: each slice list costs k workspace entries

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

// Per block: users [u0, u0 + 32) x items [n_begin, n_end) of slice blockIdx.y, 64 W items per step (two 32-item column
// tiles per wave).  Scores go through the filter and the LDS buffers of the block's users; the exclude lists are applied
// when a buffer is sorted, so the filter is one compare per score.  A candidate that finds its user's buffer full stays
// pending in its lane (its score is still in the accumulator); the block then sorts the full buffers down to k, raises their
// thresholds and offers the pending candidates again, until none is left.
//
// Operands: each wave stages its 64 item rows, 32 floats of k at a time, in a private LDS block through coalesced loads
// (lane l of load j reads row 8j + l / 8, floats 4 (l % 8) .. + 3: eight full 128-byte row segments per instruction), and
// reads them back in the MFMA layout; the block's 32 user rows come straight from global memory (shared by the W waves in
// L1).  The next block of k is loaded into registers while the MFMAs of this one run.  Lane (r, h) feeds A[user r][k'=h]
// and B[k'=h][item r]; MFMA t of block m sums k = 32m + t (h = 0) and 32m + 16 + t (h = 1).  The rest of d goes in groups of
// 8 (8g + t and 8g + 4 + t, zero past d).  The same fixed chain for every (user, item) pair.
//
// GROUPED (nrms_topk_grouped_dot): the slices run over the tiles of `tiles` (32 rows each, slice_len and IT are whole tiles),
// user = the query [B, G, d], and each of a wave's two column tiles takes its A operand from query[user, the tile's group];
// rows past a tile's len are masked, and the id of row n is item_ids[n].
//
// NOISE (nrms_softmax_sample_dot): before the filter every accumulator element becomes its perturbed key
// fmaf(score, inv_temperature, g(row key, item)); the block's 32 row seeds are formed once, in LDS.
//
// BIAS (nrms_topk_dot_biased): lane (r, h) loads bias[n] of its item in each of its two column tiles (one coalesced 128-byte
// read per tile, issued before the MFMA loop so that the loop hides its latency) and, before the filter, adds it to the tile's 16
// finished accumulator registers: one fp32 add per score, after the chain, never folded into it.  A NaN sum fails the filter's
// NaN test like a NaN score; entries simply carry s'.
//
// WINDOW (nrms_topk_dot_windowed; with or without BIAS): the block stages its 32 users' (lo, hi) in LDS once and forms their
// hull [blo, bhi).  Lane (r, h) loads item_time[n] of its item in each of its two column tiles where bv[] is loaded, and the
// filter takes (user, item) only if lo <= time < hi (hi <= INT32_MAX, so a time of INT32_MAX is open to nobody).  Dead-tile
// skip: one __ballot over "my item's time lies in [blo, bhi)" decides, wave-uniformly, whether the wave has anything to offer
// in this step; if not it issues no item loads, no LDS staging and no MFMA and goes to the block's __syncthreads_or with
// pend == 0.  The skipped region holds the chain alone, which touches only the wave's private stage[wave] and wave-level
// syncs: every wave still meets every block barrier, the same number of times.
//
// The window's two pointers are a kernel argument of the WINDOW instantiations alone (WIN is TkWindow there and empty
// elsewhere), so every other instantiation keeps the signature, the kernarg layout and the code it had without the flag.
template <int P, int W, bool VEC, bool GROUPED, bool NOISE, bool BIAS, bool WINDOW, class... WIN>
__global__ __launch_bounds__(64 * W) void topk_slice_kernel(int B, int N, int d, int k, int slice_len, int S,
                                                            const float* __restrict__ user, const float* __restrict__ items,
                                                            const int64_t* __restrict__ exclude, int n_exclude,
                                                            uint64_t* __restrict__ ws, int G, int n_tiles,
                                                            const TkTile* __restrict__ tiles,
                                                            const int32_t* __restrict__ item_ids, TkNoise noise,
                                                            const float* __restrict__ bias, WIN... win_arg) {
    static_assert(sizeof...(WIN) == (WINDOW ? 1 : 0), "WINDOW kernels take one TkWindow, the others none");
    const TkWindow win = tk_window_arg(win_arg...);
    static_assert(!(NOISE && GROUPED), "the perturbation is keyed by the item's row");
    static_assert(!(WINDOW && (GROUPED || NOISE)), "the window is for the plain and the biased top-k only");
    static_assert(!(BIAS && (GROUPED || NOISE)), "the prior is for the plain top-k only");
    __shared__ uint64_t buf[TK_UT][P];
    __shared__ uint64_t rseed[NOISE ? TK_UT : 1];
    __shared__ uint64_t thr[TK_UT];
    __shared__ int cnt[TK_UT];
    __shared__ int32_t ex[TK_UT][TK_EX_LDS];
    __shared__ __attribute__((aligned(16))) float stage[W][64 * TK_BP];
    constexpr int IT = 64 * W;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u0 = blockIdx.x * TK_UT;
    const int slice = blockIdx.y;
    const int n_begin = slice * slice_len;
    const int n_end = min(GROUPED ? 32 * n_tiles : N, n_begin + slice_len);      // (grouped: tile rows, not catalogue rows)
    const bool ex_lds = n_exclude <= TK_EX_LDS;
    int2* wwin = nullptr;          // WINDOW: the block's 32 (lo, hi)
    if constexpr (WINDOW) {
        __shared__ int2 wwin_lds[TK_UT];
        wwin = wwin_lds;
        tk_window_stage(wwin, win.window, u0, B);
    }

    if (threadIdx.x < TK_UT) {
        thr[threadIdx.x] = 0;
        cnt[threadIdx.x] = 0;
        if constexpr (NOISE) rseed[threadIdx.x] = tk_noise_row_seed(noise.seed, (uint64_t)noise.row_key[min(u0 + (int)threadIdx.x, B - 1)]);
    }
    if (ex_lds)      // only this slice's ids matter; everything else (ids outside [0, N) included) becomes -1
        for (int i = threadIdx.x; i < TK_UT * n_exclude; i += 64 * W) {
            const int u = i / n_exclude, e = i - u * n_exclude;
            const int64_t v = u0 + u < B ? exclude[(long)(u0 + u) * n_exclude + e] : -1;
            if constexpr (GROUPED) ex[u][e] = (v >= 0 && v <= 0x7FFFFFFF) ? (int32_t)v : -1;    // ids, in any slice
            else ex[u][e] = (v >= n_begin && v < n_end) ? (int32_t)v : -1;
        }
    __syncthreads();
    int blo = 0, bhi = 0;
    if constexpr (WINDOW) tk_window_hull(wwin, blo, bhi);

    // cut user i's buffer (c entries) down to its best k, excluded ids dropped; returns the new threshold, sets c
    auto flush = [&](int i, int& c) {
        tk_drop_excluded(buf[i], c, ex_lds ? ex[i] : nullptr, exclude + (long)(u0 + i) * n_exclude, n_exclude, lane);
        return tk_select<P>(buf[i], c, k, lane);
    };

    const int r = lane & 31, h = lane >> 5;
    constexpr int NA = GROUPED ? TK_TN : 1;           // A operands per k-block: one per column tile when grouped
    const float* arow[NA];
    if constexpr (!GROUPED) arow[0] = user + (long)min(u0 + r, B - 1) * d;
    float* st = stage[wave];
    const int m_full = d / 32;
    for (int n0 = n_begin; n0 < n_end; n0 += IT) {
        const int nw = n0 + 64 * wave;
        tk_f32x16 acc[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
        // grouped: the wave's two tiles (row of their first item, valid rows, group); wave-uniform
        int trow[TK_TN] = {}, tlen[TK_TN] = {};
        if constexpr (GROUPED) {
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) {
                const int t = nw / 32 + c;
                TkTile tl{0, 0, 0, 0};
                if (t < n_tiles) tl = tiles[t];
                trow[c] = __builtin_amdgcn_readfirstlane(tl.row);
                tlen[c] = __builtin_amdgcn_readfirstlane(tl.len);
                arow[c] = user + ((long)min(u0 + r, B - 1) * G + __builtin_amdgcn_readfirstlane(tl.grp)) * d;
            }
        }
        float bv[BIAS ? TK_TN : 1] = {};          // BIAS: loaded here so that the MFMA loop hides the latency, added after it
        if constexpr (BIAS) {
            if (nw < n_end) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) bv[c] = bias[min(nw + 32 * c + r, N - 1)];
            }
        }
        int tv[WINDOW ? TK_TN : 1] = {};         // WINDOW: the time of this lane's item in column tile c
        bool dead = false;                       // WINDOW: no item of this wave's step is open to any user of the block (wave-uniform)
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
        if (nw < n_end && (!GROUPED || tlen[0] + tlen[1] > 0) && !(WINDOW && dead)) {
            const float* srow[8];           // rows this lane stages: 8j + lane / 8
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (GROUPED) srow[j] = items + (long)min(trow[j >> 2] + 8 * (j & 3) + (lane >> 3), N - 1) * d + 4 * (lane & 7);
                else srow[j] = items + (long)min(nw + 8 * j + (lane >> 3), N - 1) * d + 4 * (lane & 7);
            }
#define TK_GLOAD(m)                                                                                                        \
    do {                                                                                                               \
        const int k0_ = 32 * (m);                                                                                      \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                                \
            if (VEC) {                                                                                                 \
                const float4 v_ = *reinterpret_cast<const float4*>(srow[j] + k0_);                                     \
                g[j][0] = v_.x; g[j][1] = v_.y; g[j][2] = v_.z; g[j][3] = v_.w;                                        \
            } else {                                                                                                   \
                _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) g[j][e_] = srow[j][k0_ + e_];                         \
            }                                                                                                          \
        }                                                                                                              \
        _Pragma("unroll") for (int c_ = 0; c_ < NA; ++c_)                                                              \
            _Pragma("unroll") for (int t = 0; t < 16; ++t) a[c_][t] = arow[c_][k0_ + 16 * h + t];                      \
    } while (0)
            if (m_full > 0) {
                float g[8][4];
                float a[NA][16];
                TK_GLOAD(0);
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
                    if (m + 1 < m_full) TK_GLOAD(m + 1);
#pragma unroll
                    for (int t = 0; t < 16; ++t)
#pragma unroll
                        for (int c = 0; c < TK_TN; ++c)
                            acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(acur[GROUPED ? c : 0][t], b[c][t], acc[c], 0, 0, 0);
                    tk_wave_sync();        // this block's LDS reads stay ahead of the next block's writes
                }
            }
#undef TK_GLOAD
            for (int g8 = 4 * m_full; 8 * g8 < d; ++g8) {       // zero-padded groups of 8 past the last whole block
                const int k0 = 8 * g8 + 4 * h;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float at = tk_ld(arow[0], k0 + t, d);
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) {
                        const float* brow = items + (long)min(GROUPED ? trow[c] + r : nw + 32 * c + r, N - 1) * d;
                        const float ac = GROUPED ? tk_ld(arow[GROUPED ? c : 0], k0 + t, d) : at;
                        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, tk_ld(brow, k0 + t, d), acc[c], 0, 0, 0);
                    }
                }
            }
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
        // filter.  C/D layout: item = lane & 31 of the column tile, user row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5).
        // Bit 16 c + q of `pend`: that score still has to be offered.
        uint32_t pend = 0;
        uint32_t gid[TK_TN] = {};           // grouped: the id of this lane's item in column tile c
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            const int n = nw + 32 * c + r;
            bool live = n < n_end;
            if constexpr (GROUPED) {
                live = live && r < tlen[c];
                if (live) gid[c] = (uint32_t)item_ids[trow[c] + r];
            }
            if constexpr (WINDOW) live = live && !dead;       // a skipped wave offers nothing: its accumulators hold no score
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int b = u0 + (q & 3) + 8 * (q >> 2) + 4 * h;
                if constexpr (WINDOW) {
                    const int2 w = wwin[b - u0];
                    if (live && b < B && tv[c] >= w.x && tv[c] < w.y && !__builtin_isnan(acc[c][q])) pend |= 1u << (16 * c + q);
                } else {
                    if (live && b < B && !__builtin_isnan(acc[c][q])) pend |= 1u << (16 * c + q);
                }
            }
        }
        bool first = true;
        while (__syncthreads_or(pend != 0)) {
            if (!first) {
                // sort every full buffer down to its best k (cnt may have run past P: those candidates are pending)
                for (int i = wave; i < TK_UT; i += W) {
                    if (cnt[i] >= P) {
                        int c = P;
                        const uint64_t t = flush(i, c);
                        if (lane == 0) {
                            thr[i] = t;
                            cnt[i] = c;
                        }
                    }
                }
                __syncthreads();
            }
            first = false;
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) {
                const int n = nw + 32 * c + r;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint32_t bit = 1u << (16 * c + q);
                    if (!(pend & bit)) continue;
                    const int i = (q & 3) + 8 * (q >> 2) + 4 * h;
                    const uint64_t e = tk_entry(acc[c][q], GROUPED ? gid[c] : (uint32_t)n);
                    bool keep = false;
                    if (e > thr[i]) {
                        const int slot = atomicAdd(&cnt[i], 1);
                        if (slot < P) buf[i][slot] = e;
                        else keep = true;
                    }
                    if (!keep) pend &= ~bit;
                }
            }
        }
    }
    for (int i = wave; i < TK_UT; i += W) {
        const int b = u0 + i;
        if (b >= B) break;
        int c = min(cnt[i], P);
        flush(i, c);
        uint64_t* dst = ws + ((long)b * S + slice) * k;          // the slice's best k, unsorted, 0-padded
        for (int j = lane; j < k; j += 64) dst[j] = j < c ? buf[i][j] : 0;
    }
}

// One wave per user: the best k of the user's S slice lists, sorted at the end.  Needs P >= k + 64.  top_scores may be null.
template <int P>
__global__ __launch_bounds__(64) void topk_merge_kernel(int B, int k, int S, const uint64_t* __restrict__ ws,
                                                        float* __restrict__ top_scores, int64_t* __restrict__ top_ids) {
    __shared__ uint64_t buf[P];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint64_t* src = ws + (long)b * S * k;
    const long total = (long)S * k;
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
        if (top_scores) top_scores[(long)b * k + j] = e ? tk_entry_score(e) : -__builtin_huge_valf();
        top_ids[(long)b * k + j] = e ? tk_entry_id(e) : -1;
    }
}

struct TopkGeom {
    int tiles, S, slice_len;
};

static TopkGeom topk_geom(int32_t B, int64_t N) {
    TopkGeom g{cdiv(B, TK_UT), 0, 0};
    if (N == 0 || B == 0) return g;
    int s = std::max(1, cdiv(TK_TARGET_BLOCKS, g.tiles));
    s = std::min(s, std::max(1, cdiv(N, TK_MIN_SLICE)));
    g.slice_len = cdiv(cdiv(N, s), TK_IT) * TK_IT;
    g.S = cdiv(N, g.slice_len);
    return g;
}

static bool topk_args_ok(int32_t B, int64_t N, int32_t d, int32_t k) {
    return B >= 0 && N >= 0 && N <= TK_MAX_N && d >= 1 && k >= 1 && k <= TK_MAX_K;
}

// Both kernels of one call.  grouped: `user` is the query [B, G, d], the slices run over the tile rows of `tiles`.
// bias (plain top-k only, [N] fp32): non-null selects the BIAS instantiations.  win (plain top-k only, with or without bias):
// a non-null window selects the WINDOW instantiations.
static int topk_launch(bool grouped, int32_t B, int64_t N, int32_t d, int32_t k, int32_t G, int64_t n_tiles, const float* user,
                       const float* items, const int32_t* item_ids, const TkTile* tiles, const int64_t* exclude, int32_t n_exclude,
                       float* top_scores, int64_t* top_ids, uint64_t* ws, hipStream_t s, const char* who,
                       TkNoise noise = TkNoise{nullptr, 0.0f, 0}, const float* bias = nullptr,
                       TkWindow win = TkWindow{nullptr, nullptr}) {
    const TopkGeom g = topk_geom(B, grouped ? 32 * n_tiles : N);
    char what[64];
    if (g.S > 0) {
        const bool vec = (d & 3) == 0 && ((uintptr_t)user & 15) == 0 && ((uintptr_t)items & 15) == 0;
        const dim3 grid(g.tiles, g.S);
        const int n = (int)N, nt = (int)n_tiles;
#define TK_LAUNCH_G(P, W, V, GR, NS, BI)                                                                                   \
    hipLaunchKernelGGL((topk_slice_kernel<P, W, V, GR, NS, BI, false>), grid, dim3(64 * W), 0, s, B, n, d, k, g.slice_len, g.S, user, \
                       items, exclude, n_exclude, ws, G, nt, tiles, item_ids, noise, bias)
#define TK_LAUNCH_W(P, W, V, BI)                                                                                           \
    hipLaunchKernelGGL((topk_slice_kernel<P, W, V, false, false, BI, true, TkWindow>), grid, dim3(64 * W), 0, s, B, n, d, k,     \
                       g.slice_len, g.S, user, items, exclude, n_exclude, ws, G, nt, tiles, item_ids, noise, bias, win)
#define TK_LAUNCH(P, W)                                                                                                    \
    do {                                                                                                                   \
        if (grouped) {                                                                                                     \
            if (vec) TK_LAUNCH_G(P, W, true, true, false, false);                                                          \
            else TK_LAUNCH_G(P, W, false, true, false, false);                                                             \
        } else if (noise.row_key) {                                                                                        \
            if (vec) TK_LAUNCH_G(P, W, true, false, true, false);                                                          \
            else TK_LAUNCH_G(P, W, false, false, true, false);                                                             \
        } else if (win.window && bias) {                                                                                   \
            if (vec) TK_LAUNCH_W(P, W, true, true);                                                    \
            else TK_LAUNCH_W(P, W, false, true);                                                       \
        } else if (win.window) {                                                                                           \
            if (vec) TK_LAUNCH_W(P, W, true, false);                                                   \
            else TK_LAUNCH_W(P, W, false, false);                                                      \
        } else if (bias) {                                                                                                 \
            if (vec) TK_LAUNCH_G(P, W, true, false, false, true);                                                          \
            else TK_LAUNCH_G(P, W, false, false, false, true);                                                             \
        } else {                                                                                                           \
            if (vec) TK_LAUNCH_G(P, W, true, false, false, false);                                                         \
            else TK_LAUNCH_G(P, W, false, false, false, false);                                                            \
        }                                                                                                                  \
    } while (0)
        if (k + 64 <= 128) TK_LAUNCH(128, TK_WAVES);
        else if (k + 64 <= 256) TK_LAUNCH(256, TK_WAVES);
        else TK_LAUNCH(512, 2);
#undef TK_LAUNCH
#undef TK_LAUNCH_G
#undef TK_LAUNCH_W
        snprintf(what, sizeof what, "%s(slices)", who);
        const int rc = check_launch(what);
        if (rc != NRMS_OK) return rc;
    }
    if (k + 64 <= 128) hipLaunchKernelGGL(topk_merge_kernel<128>, dim3(B), dim3(64), 0, s, B, k, g.S, ws, top_scores, top_ids);
    else if (k + 64 <= 256) hipLaunchKernelGGL(topk_merge_kernel<256>, dim3(B), dim3(64), 0, s, B, k, g.S, ws, top_scores, top_ids);
    else hipLaunchKernelGGL(topk_merge_kernel<512>, dim3(B), dim3(64), 0, s, B, k, g.S, ws, top_scores, top_ids);
    snprintf(what, sizeof what, "%s(merge)", who);
    return check_launch(what);
}

}  // namespace nrms
