// Exact rank of given items in nrms_topk_dot's order over a whole catalogue, without a [B, N] score matrix
// (include/nrms_hip.h: nrms_rank_dot, whose header comment states the contract).
//
// rank(b, t) = 1 + #{eligible n : entry(s(b, n), n) > entry(s(b, t), t)}, with the uint64 entry of topk_entry.h, so "precedes"
// is one integer compare and the counts are integers.  Three kernels:
// A (rank_entries_kernel): per 32-user tile the score chain over the GATHERED rows its users name, T targets and n_exclude
//   excluded ids each, 64 rows per wave; the entry of list position m of user b goes to ent[b][m] (0: id outside [0, N) or
//   NaN score).  The 32 x 32 MFMA tile scores every gathered row against all 32 users; only the owner's score is kept.
// B (rank_count_kernel): the grid and MFMA loop of topk_slice_kernel (32-user tiles x catalogue slices, two 32 x 32 tiles
//   per wave).  Every live, non-NaN score's entry is compared with its user's T target entries in LDS; a __ballot per
//   (accumulator register, target) gives, in its two halves, the number of the 32 items above the target for the two users
//   the register holds, and lane (j, h) keeps the running count of target j for the user of half h: 16 counters per lane.
//   Counts go to LDS, then to counts[b][j] with one integer atomic per (block, user, target).
// C (rank_finish_kernel): per user, the excluded ids pass B counted are taken back out: every distinct, in-range, non-NaN
//   excluded id whose entry precedes the target's (first occurrence of an id only); targets that are excluded, out of range
//   or NaN get rank 0 / score -inf.
//
// nrms_rank_dot_biased ranks by s'(b, n) = s(b, n) + bias[n] (one fp32 add on the finished accumulator): the BIAS instantiations
// of A and B add bias[id] / bias[n] to the score just before tk_entry; C works on entries and is the same kernel.
//
// nrms_rank_dot_windowed ranks inside a per-user interval on a per-item timestamp: the WINDOW instantiations of A and B test
// lo <= item_time[n] < hi in front of tk_entry, and B skips the waves whose 64 items are closed to its whole block; C is the same.
//
// nrms_rank_dot_tagged ranks inside a per-user set of item tags: rank_entries_tagged_kernel and rank_count_tagged_kernel, the TAGS
// forms of A and B (one body each, shared with the kernels above), test the owner's allow bit / the block's transposed bitmap in
// front of tk_entry, and B skips the waves whose 64 items are closed to its whole block; C is the same.
//
// nrms_rank_dot_adjusted ranks by s''(b, n) = s'(b, n) + the delta of user b's lowest slot that names n (topk_entry.h: TkAdjust):
// rank_entries_adjusted_kernel and rank_count_adjusted_kernel, the ADJ forms of A and B, add it to the finished s' in front of
// tk_entry (A from the owner's list in global memory, B through the block's staged slots and per-wave marks); C is the same: the
// entry it takes back out for an excluded id is the s'' entry B counted.
//
// The scores are tk_chain's (topk_entry.h), the one chain topk_slice_kernel runs too, with one A operand: nrms_topk_dot's bits
// (tests/test_hip_rank.py checks it end to end).
#include "topk_entry.h"

namespace nrms {

constexpr int RK_MAX_T = 32;
constexpr int RK_A_CHUNKS = 4096;              // grid.y bound of kernel A (longer gathered lists are walked in a loop)

// Kernel A.  One wave per block; block (x, y): user tile x, gathered positions 64 (y + i gridDim.y) .. + 63 of the tile's list
// of 32 M ids, M = T + n_exclude: position g is list slot m = g % M of user u0 + g / M (slots [0, T): targets, then the
// exclude ids).  ent [B, M].  Blocks y = 0 also zero the tile's counts [B, T] for kernel B.  Needs N >= 1.
// WINDOW: an id whose time is outside its owner's [lo, hi) gets entry 0, like a NaN score: such a target is invalid, such an
// excluded id was never counted by kernel B and is taken out of nothing.
// TAGS: the same for an id whose tag is closed to its owner (tk_tags_open: one word of the owner's allow row, from global
// memory; the ids are gathered one by one, so there is no bitmap to share).
// The body is written once; the kernels below are its instantiations (the TAGS forms are kernels of their own, so that the others
// keep their names, signatures and kernarg layouts).
// ADJ: the owner's delta for the id (tk_adjust_find: the lowest slot of the owner's list, from global memory) is added to s', one
// fp32 add after the prior's, so the entry is the s'' entry kernel B counts; a NaN sum gets entry 0 like a NaN score.
// REQ (nrms_rank_dot_request): the window, the tag set and the adjustments together, each where its pointer is not null (WINDOW,
// TAGS and ADJ are false: the three tests below are the same ones, behind a uniform branch).
template <bool VEC, bool BIAS, bool WINDOW, bool TAGS, bool ADJ = false, bool REQ = false>
__device__ __forceinline__ void rank_entries_body(int B, int N, int d, int T, int n_exclude, const float* __restrict__ user,
                                                  const float* __restrict__ items, const int64_t* __restrict__ targets,
                                                  const int64_t* __restrict__ exclude, uint64_t* __restrict__ ent,
                                                  uint32_t* __restrict__ counts, const float* __restrict__ bias, TkWindow win,
                                                  TkTags tags, TkAdjust adj = TkAdjust{nullptr, nullptr, 0}) {
    static_assert(!(TAGS && WINDOW), "the tag set is for the plain and the biased rank only");
    static_assert(!(ADJ && (TAGS || WINDOW)), "the adjustments are for the plain and the biased rank only");
    static_assert(!(REQ && (ADJ || TAGS || WINDOW)), "a request holds its window, tag set and adjustments itself");
    __shared__ int rows[64];
    __shared__ __attribute__((aligned(16))) float stage[64 * TK_BP];
    const int lane = threadIdx.x;
    const int r = lane & 31, h = lane >> 5;
    const int u0 = blockIdx.x * TK_UT;
    const int M = T + n_exclude;
    const long total = (long)TK_UT * M;
    if (blockIdx.y == 0)
        for (int i = lane; i < TK_UT * T; i += 64) {
            const int b = u0 + i / T;
            if (b < B) counts[(long)b * T + (i % T)] = 0;
        }
    const float* arow[1] = {user + (long)min(u0 + r, B - 1) * d};
    for (long g0 = 64L * blockIdx.y; g0 < total; g0 += 64L * gridDim.y) {
        // this lane's own list position: the id it names, and the row the wave reads for it (row 0 for an id that names none)
        const long g = g0 + lane;
        const int u = (int)(g / M), m = (int)(g - (long)u * M);
        const int b = u0 + u;
        int64_t id = -1;
        if (g < total && b < B) id = m < T ? targets[(long)b * T + m] : exclude[(long)b * n_exclude + (m - T)];
        const bool in_range = id >= 0 && id < N;
        tk_wave_sync();            // the previous round's reads of rows
        rows[lane] = in_range ? (int)id : 0;
        tk_wave_sync();
        tk_f32x16 acc[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
        tk_chain<VEC>(acc, arow, items, d, stage, lane, [&](int i) { return rows[i]; });
        // C/D layout: item = lane & 31 of the column tile, user row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5): the score of
        // position g0 + 32 c + r against its owner u sits in half (u >> 2) & 1, register (u & 3) + 4 (u >> 3)
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            const long gc = g0 + 32 * c + r;
            const int uc = (int)(gc / M), mc = (int)(gc - (long)uc * M);
            const int64_t idc = __shfl(id, 32 * c + r, 64);
            if (gc >= total || u0 + uc >= B || ((uc >> 2) & 1) != h) continue;
            const int qw = (uc & 3) + 4 * (uc >> 3);
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < 16; ++q) s = q == qw ? acc[c][q] : s;
            if constexpr (BIAS) {
                if (idc >= 0 && idc < N) s = s + bias[idc];
            }
            if constexpr (ADJ || REQ) {
                float dl;
                if ((!REQ || adj.adj_ids) && idc >= 0 && idc < N && tk_adjust_find(adj, u0 + uc, idc, dl)) s = s + dl;
            }
            bool ok = idc >= 0 && idc < N && !__builtin_isnan(s);
            if constexpr (WINDOW || REQ) {
                if (ok && (!REQ || win.window)) {
                    const int tv = win.item_time[idc];
                    ok = tv >= win.window[2 * (long)(u0 + uc)] && tv < win.window[2 * (long)(u0 + uc) + 1];
                }
            }
            if constexpr (TAGS || REQ) {
                if (ok && (!REQ || tags.allow)) ok = tk_tags_open(tags, u0 + uc, tags.item_tag[idc]);
            }
            ent[(long)(u0 + uc) * M + mc] = ok ? tk_entry(s, (uint32_t)idc) : 0;
        }
    }
}

template <bool VEC, bool BIAS, bool WINDOW>
__global__ __launch_bounds__(64) void rank_entries_kernel(int B, int N, int d, int T, int n_exclude,
                                                          const float* __restrict__ user, const float* __restrict__ items,
                                                          const int64_t* __restrict__ targets,
                                                          const int64_t* __restrict__ exclude, uint64_t* __restrict__ ent,
                                                          uint32_t* __restrict__ counts, const float* __restrict__ bias,
                                                          TkWindow win) {
    rank_entries_body<VEC, BIAS, WINDOW, false>(B, N, d, T, n_exclude, user, items, targets, exclude, ent, counts, bias, win,
                                                TkTags{nullptr, nullptr, 0});
}

template <bool VEC, bool BIAS>
__global__ __launch_bounds__(64) void rank_entries_tagged_kernel(int B, int N, int d, int T, int n_exclude,
                                                                 const float* __restrict__ user, const float* __restrict__ items,
                                                                 const int64_t* __restrict__ targets,
                                                                 const int64_t* __restrict__ exclude, uint64_t* __restrict__ ent,
                                                                 uint32_t* __restrict__ counts, const float* __restrict__ bias,
                                                                 TkTags tags) {
    rank_entries_body<VEC, BIAS, false, true>(B, N, d, T, n_exclude, user, items, targets, exclude, ent, counts, bias,
                                              TkWindow{nullptr, nullptr}, tags);
}

template <bool VEC, bool BIAS>
__global__ __launch_bounds__(64) void rank_entries_adjusted_kernel(int B, int N, int d, int T, int n_exclude,
                                                                   const float* __restrict__ user, const float* __restrict__ items,
                                                                   const int64_t* __restrict__ targets,
                                                                   const int64_t* __restrict__ exclude, uint64_t* __restrict__ ent,
                                                                   uint32_t* __restrict__ counts, const float* __restrict__ bias,
                                                                   TkAdjust adj) {
    rank_entries_body<VEC, BIAS, false, false, true>(B, N, d, T, n_exclude, user, items, targets, exclude, ent, counts, bias,
                                                     TkWindow{nullptr, nullptr}, TkTags{nullptr, nullptr, 0}, adj);
}

template <bool VEC, bool BIAS>
__global__ __launch_bounds__(64) void rank_entries_request_kernel(int B, int N, int d, int T, int n_exclude,
                                                                  const float* __restrict__ user, const float* __restrict__ items,
                                                                  const int64_t* __restrict__ targets,
                                                                  const int64_t* __restrict__ exclude, uint64_t* __restrict__ ent,
                                                                  uint32_t* __restrict__ counts, const float* __restrict__ bias,
                                                                  TkRequest req) {
    rank_entries_body<VEC, BIAS, false, false, false, true>(B, N, d, T, n_exclude, user, items, targets, exclude, ent, counts, bias,
                                                            req.win, req.tags, req.adj);
}

// Kernel B.  Per block: users [u0, u0 + 32) x items [n_begin, n_end) of slice blockIdx.y, 64 W items per step.  ent [B, M]:
// the first T entries of a row are the user's targets.  counts [B, T] += #{live non-NaN n in the slice : entry(n) > target}.
// WINDOW: topk_slice_kernel's window filter and dead-tile skip.  The block stages its users' (lo, hi) in LDS and forms their
// hull [blo, bhi); a score becomes an entry only if lo <= item_time[n] < hi for its user; a wave none of whose 64 item times
// lies in the hull (one __ballot, wave-uniform) goes to its next step with zero entries: no item loads, no staging, no MFMA.
// The step loop holds no block barrier, so a skipping wave meets the two barriers around it like every other wave.
// TAGS: topk_slice_kernel's tag filter and dead-wave skip.  The block builds the transposed bitmap of its users' tag sets in LDS
// (tk_tags_stage); a lane reads one LDS word per item, tm[c], and a score becomes an entry only if its user's bit of tm[c] is set;
// a wave with tm[0] | tm[1] == 0 in every lane goes to its next step like a WINDOW wave outside the hull.
// ADJ: topk_slice_kernel's adjustments.  The block stages the slots of its users that name a row of its slice (tk_adjust_stage;
// RK_ADJ_CAP words: every slot its 32 users can have), a wave marks its 64 items' hits per step (tk_adjust_mark) and the lane that
// holds a marked pair adds the delta of the pair's lowest slot to the finished s' (tk_adjust_apply) before the entries are formed.
// REQ (nrms_rank_dot_request): the three parts together, each where its pointer is not null (a block-uniform branch).  A wave is
// skipped when the window hull OR the tag bitmap closes all its 64 items to the whole block.
template <int W, bool VEC, bool BIAS, bool WINDOW, bool TAGS, bool ADJ = false, bool REQ = false>
__device__ __forceinline__ void rank_count_body(int B, int N, int d, int T, int M, int slice_len, const float* __restrict__ user,
                                                const float* __restrict__ items, const uint64_t* __restrict__ ent,
                                                uint32_t* __restrict__ counts, const float* __restrict__ bias, TkWindow win,
                                                TkTags tags, TkAdjust adj = TkAdjust{nullptr, nullptr, 0}) {
    static_assert(!(TAGS && WINDOW), "the tag set is for the plain and the biased rank only");
    static_assert(!(ADJ && (TAGS || WINDOW)), "the adjustments are for the plain and the biased rank only");
    static_assert(!(REQ && (ADJ || TAGS || WINDOW)), "a request holds its window, tag set and adjustments itself");
    __shared__ uint64_t tgt[TK_UT][RK_MAX_T];
    __shared__ uint32_t cnts[TK_UT][RK_MAX_T];
    __shared__ __attribute__((aligned(16))) float stage[W][64 * TK_BP];
    constexpr int IT = 64 * W;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u0 = blockIdx.x * TK_UT;
    const int n_begin = blockIdx.y * slice_len;
    const int n_end = min(N, n_begin + slice_len);

    for (int i = threadIdx.x; i < TK_UT * RK_MAX_T; i += 64 * W) {
        const int u = i / RK_MAX_T, j = i % RK_MAX_T;
        tgt[u][j] = (u0 + u < B && j < T) ? ent[(long)(u0 + u) * M + j] : ~0ull;
        cnts[u][j] = 0;
    }
    int2* wwin = nullptr;          // WINDOW: the block's 32 (lo, hi)
    if constexpr (WINDOW) {
        __shared__ int2 wwin_lds[TK_UT];
        wwin = wwin_lds;
        tk_window_stage(wwin, win.window, u0, B);
    }
    uint32_t* ubt = nullptr;       // TAGS: the block's transposed tag bitmap
    if constexpr (TAGS) {
        __shared__ uint32_t ubt_lds[TK_MAX_TAGS];
        ubt = ubt_lds;
        tk_tags_stage(ubt, tags, u0, B, 64 * W);
    }
    [[maybe_unused]] uint32_t* axl = nullptr;       // ADJ: the block's staged slots, their count and one row of marks per wave
    [[maybe_unused]] int* axl_n = nullptr;
    [[maybe_unused]] uint32_t* axm = nullptr;
    if constexpr (ADJ) {
        __shared__ uint32_t axl_lds[RK_ADJ_CAP];
        __shared__ int axl_n_lds;
        __shared__ uint32_t axm_lds[W][64];
        axl = axl_lds;
        axl_n = &axl_n_lds;
        axm = axm_lds[wave];
        if (threadIdx.x == 0) axl_n_lds = 0;
        for (int i = threadIdx.x; i < 64 * W; i += 64 * W) axm_lds[i / 64][i % 64] = 0;
        __syncthreads();
        tk_adjust_stage<RK_ADJ_CAP>(axl, axl_n, adj, u0, B, n_begin, n_end, 64 * W);
    }
    if constexpr (REQ) {
        __shared__ int2 wwin_lds[TK_UT];
        __shared__ uint32_t ubt_lds[TK_MAX_TAGS];
        __shared__ uint32_t axl_lds[RK_ADJ_CAP];
        __shared__ int axl_n_lds;
        __shared__ uint32_t axm_lds[W][64];
        if (win.window) {
            wwin = wwin_lds;
            tk_window_stage(wwin, win.window, u0, B);
        }
        if (tags.allow) {
            ubt = ubt_lds;
            tk_tags_stage(ubt, tags, u0, B, 64 * W);
        }
        if (adj.adj_ids) {
            axl = axl_lds;
            axl_n = &axl_n_lds;
            axm = axm_lds[wave];
            if (threadIdx.x == 0) axl_n_lds = 0;
            for (int i = threadIdx.x; i < 64 * W; i += 64 * W) axm_lds[i / 64][i % 64] = 0;
            __syncthreads();
            tk_adjust_stage<RK_ADJ_CAP>(axl, axl_n, adj, u0, B, n_begin, n_end, 64 * W);
        }
    }
    __syncthreads();
    [[maybe_unused]] int n_axl = 0;
    if constexpr (ADJ) n_axl = *axl_n;
    int blo = 0, bhi = 0;
    if constexpr (WINDOW) tk_window_hull(wwin, blo, bhi);
    if constexpr (REQ) {
        if (adj.adj_ids) n_axl = *axl_n;
        if (wwin) tk_window_hull(wwin, blo, bhi);
    }

    const int r = lane & 31, h = lane >> 5;
    const float* arow[1] = {user + (long)min(u0 + r, B - 1) * d};
    float* st = stage[wave];
    uint32_t cnt[16] = {};          // lane (j, h): items above target j of user (q & 3) + 8 (q >> 2) + 4 h
    for (int n0 = n_begin; n0 < n_end; n0 += IT) {
        const int nw = n0 + 64 * wave;
        if (nw >= n_end) continue;
        int tv[WINDOW || REQ ? TK_TN : 1] = {};         // WINDOW: the time of this lane's item in column tile c
        if constexpr (REQ) {
            if (wwin) {
                bool any = false;
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) {
                    const int n = nw + 32 * c + r;
                    tv[c] = win.item_time[min(n, N - 1)];
                    any |= n < n_end && tv[c] >= blo && tv[c] < bhi;
                }
                if (TK_WINDOW_SKIP && __ballot(any) == 0) continue;       // wave-uniform
            }
        }
        if constexpr (WINDOW) {
            bool any = false;
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) {
                const int n = nw + 32 * c + r;
                tv[c] = win.item_time[min(n, N - 1)];
                any |= n < n_end && tv[c] >= blo && tv[c] < bhi;
            }
            if (TK_WINDOW_SKIP && __ballot(any) == 0) continue;       // wave-uniform: nothing here is open to any user of the block
        }
        uint32_t tm[TAGS || REQ ? TK_TN : 1] = {};      // TAGS: the block's users that this lane's item of column tile c is open to
        if constexpr (REQ) {
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) tm[c] = nw + 32 * c + r < n_end ? ~0u : 0u;          // (no tag set: open to all)
            if (ubt) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) tm[c] &= tk_tags_mask(ubt, tags.item_tag[min(nw + 32 * c + r, N - 1)], tags.n_tags);
                if (TK_TAGS_SKIP && __ballot((tm[0] | tm[1]) != 0) == 0) continue;       // wave-uniform
            }
        }
        if constexpr (TAGS) {
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) {
                const int n = nw + 32 * c + r;
                const uint32_t m = tk_tags_mask(ubt, tags.item_tag[min(n, N - 1)], tags.n_tags);
                tm[c] = n < n_end ? m : 0u;
            }
            if (TK_TAGS_SKIP && __ballot((tm[0] | tm[1]) != 0) == 0) continue;       // wave-uniform, as above
        }
        tk_f32x16 acc[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
        float bv[BIAS ? TK_TN : 1] = {};          // BIAS: loaded ahead of the chain, which hides the latency; added after it
        if constexpr (BIAS) {
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) bv[c] = bias[min(nw + 32 * c + r, N - 1)];
        }
        tk_chain<VEC>(acc, arow, items, d, st, lane, [&](int i) { return min(nw + i, N - 1); });
        if constexpr (ADJ || REQ) {          // s' in place (the same fp32 add as below), then the marked pairs' deltas
            if constexpr (BIAS) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[c][q] = acc[c][q] + bv[c];
            }
            if (!REQ || adj.adj_ids) {
                uint32_t am[TK_TN];
                tk_adjust_mark<RK_ADJ_CAP>(am, axm, axl, n_axl, adj, u0, B, n_begin, nw, n_end, lane);
                tk_adjust_apply(acc, am, adj, u0, nw, lane);
            }
        }
        // C/D layout: item = lane & 31 of the column tile, user row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
        uint64_t e[TK_TN][16];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            const int n = nw + 32 * c + r;
            const bool live = n < n_end;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                float s = acc[c][q];
                if constexpr (BIAS && !ADJ && !REQ) s = s + bv[c];
                bool open = live && !__builtin_isnan(s);
                if constexpr (REQ) {
                    if (wwin) {
                        const int2 w = wwin[(q & 3) + 8 * (q >> 2) + 4 * h];
                        open = open && tv[c] >= w.x && tv[c] < w.y;
                    }
                    open = open && ((tm[c] >> ((q & 3) + 8 * (q >> 2) + 4 * h)) & 1u);
                }
                if constexpr (WINDOW) {
                    const int2 w = wwin[(q & 3) + 8 * (q >> 2) + 4 * h];
                    open = open && tv[c] >= w.x && tv[c] < w.y;
                }
                if constexpr (TAGS) open = open && ((tm[c] >> ((q & 3) + 8 * (q >> 2) + 4 * h)) & 1u);
                e[c][q] = open ? tk_entry(s, (uint32_t)n) : 0;       // 0 precedes nothing
            }
        }
        for (int j = 0; j < T; ++j) {
            uint64_t t[16];          // target j of this half's 16 users: 16 independent LDS reads, two addresses each
#pragma unroll
            for (int q = 0; q < 16; ++q) t[q] = tgt[(q & 3) + 8 * (q >> 2) + 4 * h][j];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                uint32_t above = 0;
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) {
                    const unsigned long long m = __ballot(e[c][q] > t[q]);
                    above += __popc(h ? (uint32_t)(m >> 32) : (uint32_t)m);
                }
                if (r == j) cnt[q] += above;
            }
        }
    }
    if (r < T) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (cnt[q]) atomicAdd(&cnts[(q & 3) + 8 * (q >> 2) + 4 * h][r], cnt[q]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TK_UT * RK_MAX_T; i += 64 * W) {
        const int u = i / RK_MAX_T, j = i % RK_MAX_T;
        if (u0 + u < B && j < T && cnts[u][j]) atomicAdd(&counts[(long)(u0 + u) * T + j], cnts[u][j]);
    }
}

template <int W, bool VEC, bool BIAS, bool WINDOW>
__global__ __launch_bounds__(64 * W) void rank_count_kernel(int B, int N, int d, int T, int M, int slice_len,
                                                            const float* __restrict__ user, const float* __restrict__ items,
                                                            const uint64_t* __restrict__ ent, uint32_t* __restrict__ counts,
                                                            const float* __restrict__ bias, TkWindow win) {
    rank_count_body<W, VEC, BIAS, WINDOW, false>(B, N, d, T, M, slice_len, user, items, ent, counts, bias, win,
                                                 TkTags{nullptr, nullptr, 0});
}

template <int W, bool VEC, bool BIAS>
__global__ __launch_bounds__(64 * W) void rank_count_tagged_kernel(int B, int N, int d, int T, int M, int slice_len,
                                                                   const float* __restrict__ user, const float* __restrict__ items,
                                                                   const uint64_t* __restrict__ ent, uint32_t* __restrict__ counts,
                                                                   const float* __restrict__ bias, TkTags tags) {
    rank_count_body<W, VEC, BIAS, false, true>(B, N, d, T, M, slice_len, user, items, ent, counts, bias, TkWindow{nullptr, nullptr},
                                               tags);
}

template <int W, bool VEC, bool BIAS>
__global__ __launch_bounds__(64 * W) void rank_count_adjusted_kernel(int B, int N, int d, int T, int M, int slice_len,
                                                                     const float* __restrict__ user, const float* __restrict__ items,
                                                                     const uint64_t* __restrict__ ent, uint32_t* __restrict__ counts,
                                                                     const float* __restrict__ bias, TkAdjust adj) {
    rank_count_body<W, VEC, BIAS, false, false, true>(B, N, d, T, M, slice_len, user, items, ent, counts, bias,
                                                      TkWindow{nullptr, nullptr}, TkTags{nullptr, nullptr, 0}, adj);
}

template <int W, bool VEC, bool BIAS>
__global__ __launch_bounds__(64 * W) void rank_count_request_kernel(int B, int N, int d, int T, int M, int slice_len,
                                                                    const float* __restrict__ user, const float* __restrict__ items,
                                                                    const uint64_t* __restrict__ ent, uint32_t* __restrict__ counts,
                                                                    const float* __restrict__ bias, TkRequest req) {
    rank_count_body<W, VEC, BIAS, false, false, false, true>(B, N, d, T, M, slice_len, user, items, ent, counts, bias, req.win,
                                                             req.tags, req.adj);
}

// Kernel C.  One wave per user.  N = 0: every target is invalid (ent and counts are not read).
__global__ __launch_bounds__(64) void rank_finish_kernel(int B, int N, int T, int n_exclude, const int64_t* __restrict__ targets,
                                                         const int64_t* __restrict__ exclude, uint64_t* ent,
                                                         const uint32_t* __restrict__ counts, int32_t* __restrict__ ranks,
                                                         float* __restrict__ target_scores) {
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    if (N == 0) {
        if (lane < T) {
            ranks[b * T + lane] = 0;
            if (target_scores) target_scores[b * T + lane] = -__builtin_huge_valf();
        }
        return;
    }
    const int M = T + n_exclude;
    uint64_t* eb = ent + b * M;
    const int64_t* xb = exclude + b * n_exclude;           // (never read when n_exclude = 0)
    // an id listed twice is taken back out once: only its first occurrence keeps its entry
    for (int x = lane; x < n_exclude; x += 64) {
        if (!eb[T + x]) continue;
        const int64_t id = xb[x];
        bool dup = false;
        for (int y = 0; y < x; ++y) dup |= xb[y] == id;
        if (dup) eb[T + x] = 0;
    }
    __syncthreads();
    if (lane < T) {
        const uint64_t et = eb[lane];
        const int64_t id = targets[b * T + lane];
        bool out = false;
        uint32_t sub = 0;
        for (int x = 0; x < n_exclude; ++x) {
            out |= xb[x] == id;
            sub += eb[T + x] > et;
        }
        const bool valid = et != 0 && !out;
        ranks[b * T + lane] = valid ? (int32_t)(1u + counts[b * T + lane] - sub) : 0;
        if (target_scores) target_scores[b * T + lane] = valid ? tk_entry_score(et) : -__builtin_huge_valf();
    }
}

static bool rank_args_ok(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude) {
    return B >= 0 && N >= 0 && N <= TK_MAX_N && d >= 1 && T >= 1 && T <= RK_MAX_T && n_exclude >= 0;
}

static size_t rank_entry_bytes(int32_t B, int32_t T, int32_t n_exclude) {
    return ((size_t)B * ((size_t)T + (size_t)n_exclude) * sizeof(uint64_t) + 255) / 256 * 256;
}

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_rank_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude) {
    if (!rank_args_ok(B, N, d, T, n_exclude)) return 0;
    // the entries [B, T + n_exclude] and the counts [B, T]; never 0 for accepted arguments
    return 256 + rank_entry_bytes(B, T, n_exclude) + (size_t)B * (size_t)T * sizeof(uint32_t);
}

// nrms_rank_dot (bias null, who "rank_dot"), nrms_rank_dot_biased, nrms_rank_dot_windowed (windowed: item_time and window are
// required) and nrms_rank_dot_tagged (tagged: item_tag and allow are required, 1 <= n_tags <= TK_MAX_TAGS): one body.
static int rank_dot_call(const char* who, int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                         const float* bias, bool windowed, const int32_t* item_time, const int32_t* window, const int64_t* targets,
                         const int64_t* exclude, int32_t n_exclude, int32_t* ranks, float* target_scores, void* workspace,
                         size_t workspace_bytes, void* stream, bool tagged = false, TkTags tags = TkTags{nullptr, nullptr, 0},
                         TkAdjust adj = TkAdjust{nullptr, nullptr, 0}, bool request = false) {
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "T", T, RK_MAX_T, n_exclude);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE(!tagged || (tags.n_tags >= 1 && tags.n_tags <= TK_MAX_TAGS), "%s: n_tags must be in [1, %d] (n_tags=%d)", who,
                 TK_MAX_TAGS, tags.n_tags);
    if (B == 0) return rc;
    if (!exclude) n_exclude = 0;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {"item_time", item_time, windowed && N != 0, 4}, {"window", window, windowed, 4},
                             {"item_tag", tags.item_tag, tagged && N != 0, 4}, {"allow", tags.allow, tagged, 4},
                             {"targets", targets, true, 1}, {"ranks", ranks, true, 1}},
                       workspace, workspace_bytes, nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude), 8);
    if (rc != NRMS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    uint64_t* ent = (uint64_t*)workspace;
    uint32_t* counts = (uint32_t*)((char*)workspace + rank_entry_bytes(B, T, n_exclude));
    const TkGeom g = tk_geom(B, N, false);          // no minimum slice: the workspace does not grow with the slice count
    const int n = (int)N, M = T + n_exclude;
    const TkWindow win = windowed ? TkWindow{item_time, window} : TkWindow{nullptr, nullptr};
    char what[64];
    if (g.S > 0) {
        const dim3 grid_a(g.tiles, std::min((long)RK_A_CHUNKS, ((long)TK_UT * M + 63) / 64)), grid_b(g.tiles, g.S);
        if (request) tk_with_flags([&](auto V, auto BI) {
            constexpr bool v = decltype(V)::value, bi = decltype(BI)::value;
            const TkRequest req{win, tagged ? tags : TkTags{nullptr, nullptr, 0}, adj, TkCursor{nullptr, nullptr, 0}};
            hipLaunchKernelGGL((rank_entries_request_kernel<v, bi>), grid_a, dim3(64), 0, s, B, n, d, T, n_exclude, user, items,
                               targets, exclude, ent, counts, bias, req);
            snprintf(what, sizeof what, "%s(entries)", who);
            rc = check_launch(what);
            if (rc != NRMS_OK) return;
            hipLaunchKernelGGL((rank_count_request_kernel<TK_WAVES, v, bi>), grid_b, dim3(64 * TK_WAVES), 0, s, B, n, d, T, M,
                               g.slice_len, user, items, ent, counts, bias, req);
            snprintf(what, sizeof what, "%s(count)", who);
            rc = check_launch(what);
        }, tk_vec_ok(d, user, items), bias != nullptr);
        else if (adj.adj_ids) tk_with_flags([&](auto V, auto BI) {
            constexpr bool v = decltype(V)::value, bi = decltype(BI)::value;
            hipLaunchKernelGGL((rank_entries_adjusted_kernel<v, bi>), grid_a, dim3(64), 0, s, B, n, d, T, n_exclude, user, items,
                               targets, exclude, ent, counts, bias, adj);
            snprintf(what, sizeof what, "%s(entries)", who);
            rc = check_launch(what);
            if (rc != NRMS_OK) return;
            hipLaunchKernelGGL((rank_count_adjusted_kernel<TK_WAVES, v, bi>), grid_b, dim3(64 * TK_WAVES), 0, s, B, n, d, T, M,
                               g.slice_len, user, items, ent, counts, bias, adj);
            snprintf(what, sizeof what, "%s(count)", who);
            rc = check_launch(what);
        }, tk_vec_ok(d, user, items), bias != nullptr);
        else if (tagged) tk_with_flags([&](auto V, auto BI) {
            constexpr bool v = decltype(V)::value, bi = decltype(BI)::value;
            hipLaunchKernelGGL((rank_entries_tagged_kernel<v, bi>), grid_a, dim3(64), 0, s, B, n, d, T, n_exclude, user, items, targets,
                               exclude, ent, counts, bias, tags);
            snprintf(what, sizeof what, "%s(entries)", who);
            rc = check_launch(what);
            if (rc != NRMS_OK) return;
            hipLaunchKernelGGL((rank_count_tagged_kernel<TK_WAVES, v, bi>), grid_b, dim3(64 * TK_WAVES), 0, s, B, n, d, T, M,
                               g.slice_len, user, items, ent, counts, bias, tags);
            snprintf(what, sizeof what, "%s(count)", who);
            rc = check_launch(what);
        }, tk_vec_ok(d, user, items), bias != nullptr);
        else tk_with_flags([&](auto V, auto BI, auto WI) {
            constexpr bool v = decltype(V)::value, bi = decltype(BI)::value, wi = decltype(WI)::value;
            hipLaunchKernelGGL((rank_entries_kernel<v, bi, wi>), grid_a, dim3(64), 0, s, B, n, d, T, n_exclude, user, items, targets,
                               exclude, ent, counts, bias, win);
            snprintf(what, sizeof what, "%s(entries)", who);
            rc = check_launch(what);
            if (rc != NRMS_OK) return;
            hipLaunchKernelGGL((rank_count_kernel<TK_WAVES, v, bi, wi>), grid_b, dim3(64 * TK_WAVES), 0, s, B, n, d, T, M, g.slice_len,
                               user, items, ent, counts, bias, win);
            snprintf(what, sizeof what, "%s(count)", who);
            rc = check_launch(what);
        }, tk_vec_ok(d, user, items), bias != nullptr, windowed);
        if (rc != NRMS_OK) return rc;
    }
    hipLaunchKernelGGL(rank_finish_kernel, dim3(B), dim3(64), 0, s, B, n, T, n_exclude, targets, exclude, ent, counts, ranks,
                       target_scores);
    snprintf(what, sizeof what, "%s(finish)", who);
    return check_launch(what);
}

extern "C" int nrms_rank_dot(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                             const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                             float* target_scores, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_dot_call("rank_dot", B, N, d, T, user, items, nullptr, false, nullptr, nullptr, targets, exclude, n_exclude, ranks, target_scores, workspace,
                         workspace_bytes, stream);
}

// The biased call's workspace is the unbiased call's: the same entries and counts.
extern "C" size_t nrms_rank_dot_biased_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude) {
    return nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude);
}

extern "C" int nrms_rank_dot_biased(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                                    const float* bias, const int64_t* targets, const int64_t* exclude, int32_t n_exclude,
                                    int32_t* ranks, float* target_scores, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_dot_call("rank_dot_biased", B, N, d, T, user, items, bias, false, nullptr, nullptr, targets, exclude, n_exclude,
                         ranks, target_scores, workspace, workspace_bytes, stream);
}

// The windowed call's workspace is the unwindowed call's: the same entries and counts.
extern "C" size_t nrms_rank_dot_windowed_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude) {
    return nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude);
}

extern "C" int nrms_rank_dot_windowed(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                                      const float* bias, const int32_t* item_time, const int32_t* window, const int64_t* targets,
                                      const int64_t* exclude, int32_t n_exclude, int32_t* ranks, float* target_scores,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    return rank_dot_call("rank_dot_windowed", B, N, d, T, user, items, bias, true, item_time, window, targets, exclude, n_exclude,
                         ranks, target_scores, workspace, workspace_bytes, stream);
}

// nrms_rank_dot_tagged's body (its C entry point is in topktags.hip, with the tagged top-k's).
int nrms::rank_dot_tagged_call(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items, const float* bias,
                               TkTags tags, const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                               float* target_scores, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_dot_call("rank_dot_tagged", B, N, d, T, user, items, bias, false, nullptr, nullptr, targets, exclude, n_exclude, ranks,
                         target_scores, workspace, workspace_bytes, stream, true, tags);
}

// nrms_rank_dot_adjusted's body (its C entry point is in topkadjust.hip, with the adjusted top-k's, which has checked E and the two
// pointers): adj.adj_ids null = the plain / biased call.
int nrms::rank_dot_adjusted_call(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items, const float* bias,
                                 TkAdjust adj, const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                                 float* target_scores, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_dot_call("rank_dot_adjusted", B, N, d, T, user, items, bias, false, nullptr, nullptr, targets, exclude, n_exclude,
                         ranks, target_scores, workspace, workspace_bytes, stream, false, TkTags{nullptr, nullptr, 0}, adj);
}

// nrms_rank_dot_request's body for two or more parts (its C entry point is in topkrequest.hip, which has checked the pairs, n_tags
// and E): the REQ forms of kernels A and B, each part present where its pointer is not null.
int nrms::rank_dot_request_call(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items, const float* bias,
                                TkRequest req, const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                                float* target_scores, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_dot_call("rank_dot_request", B, N, d, T, user, items, bias, req.win.window != nullptr, req.win.item_time,
                         req.win.window, targets, exclude, n_exclude, ranks, target_scores, workspace, workspace_bytes, stream,
                         req.tags.allow != nullptr, req.tags, req.adj, true);
}
