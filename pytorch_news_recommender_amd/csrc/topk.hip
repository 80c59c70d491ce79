// Top-k retrieval over a whole catalogue: the k items of largest user . item score per user, without a [B, N] score
// matrix (include/nrms_hip.h: nrms_topk_dot, whose header comment states the order and the padding rule).
//
// Kernel 1 (topk_slice_kernel): grid = 32-user tiles x catalogue slices.  Each wave forms two 32 x 32 score tiles on
// v_mfma_f32_32x32x2_f32 (tk_chain, topk_entry.h: one accumulator over all of d, no split-K; the one score chain of every
// catalogue kernel, rankdot.hip's included), and every score that beats its user's running threshold is appended to the
// user's LDS buffer (TkFilter, topk_kernels.h).  When a buffer is full, excluded ids are dropped, the best k are selected
// (bitwise search for the k-th entry over registers, no sort) and the user's threshold is raised to the k-th entry; the scores
// that found it full are still in the accumulators and are offered again.  The block writes one k-list per (user, slice) into
// the workspace.
// Kernel 2 (topk_merge_kernel): one wave per user runs the same filter / buffer / select over the user's slice lists and
// sorts the final k once (tk_merge: wave bitonic sort in LDS).
//
// An entry is one uint64: the score as an order-preserving 32-bit key (-0.0 canonicalised to +0.0) above the complement of
// the 32-bit item id, so larger entry = higher score, then smaller id.  Entry 0 lies below every real entry and is padding.
// The order is total, so the result does not depend on the slice count, the launch geometry or the order of insertion.
//
// nrms_topk_grouped_dot runs the same two kernels with a query per (user, item group): the catalogue, stored group after
// group, is laid out in 32-row tiles that never straddle a group (each group padded to a whole number of tiles; the table is
// written by topk_tiles_kernel into the workspace), so every MFMA column tile has one A operand, the tile's group's query
// rows.  Scores keep the chain of nrms_topk_dot, and entries carry item_ids[row] instead of the row.
//
// nrms_topk_dot_biased runs the two kernels of nrms_topk_dot with a per-item prior added to every finished score (the BIAS
// instantiations of topk_slice_kernel): entries carry s' = s + bias[n], everything after the add is the same code.
//
// nrms_topk_dot_windowed adds a per-user eligibility interval on a per-item timestamp (the WINDOW instantiations, with or
// without BIAS): two integer compares in the filter, and a wave whose 64 items are closed to all 32 users of its block skips
// its loads and its MFMA chain (topk_kernels.h describes the skip and why no block barrier can notice it).
//
// nrms_topk_dot_after is a page of that ranking: a per-user cursor, the last (score, id) the caller saw, as one 64-bit key, and
// one more integer compare in the filter (the CURSOR instantiations, with or without BIAS and WINDOW): only entries strictly
// below the key are offered.  nrms_topk_dot_deep chains such pages on the stream, each reading its cursor from the last column the
// page before wrote and merging into its own columns of the [B, K] result (the merge kernel's output row stride).
#include "topk_kernels.h"    // the kernels and their launcher, shared with softmaxsample.hip

namespace nrms {

// One block: the tile table of a grouped catalogue.  Group g (rows [group_ptr[g], group_ptr[g + 1]), clamped to [0, N])
// gets ceil(len / 32) consecutive tiles, the groups in order; tiles [total, n_tiles) are unused (len 0).  A group_ptr that is
// not nondecreasing from 0 to N cannot send a row outside [0, N) or a tile past n_tiles.
__global__ __launch_bounds__(1024) void topk_tiles_kernel(int N, int G, int n_tiles, const int64_t* __restrict__ group_ptr,
                                                          TkTile* __restrict__ tiles) {
    __shared__ long part[1024];
    const int per = (G + 1023) / 1024;
    const int lo = min(G, (int)threadIdx.x * per), hi = min(G, lo + per);
    long s = 0;
    for (int g = lo; g < hi; ++g) {
        int row, len;
        tk_group_span(group_ptr, g, N, row, len);
        s += (len + 31) / 32;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long run = 0;
        for (int i = 0; i < 1024; ++i) { const long t = part[i]; part[i] = run; run += t; }
        part[0] = run;              // (thread 0's own offset is 0: kept in `first` below)
    }
    __syncthreads();
    const long total = part[0];
    long t = threadIdx.x == 0 ? 0 : part[threadIdx.x];
    for (int g = lo; g < hi; ++g) {
        int row, len;
        tk_group_span(group_ptr, g, N, row, len);
        for (int j = 0; j < len && t < n_tiles; j += 32, ++t) tiles[t] = TkTile{row + j, min(32, len - j), g, 0};
    }
    for (long u = total + threadIdx.x; u < n_tiles; u += 1024) tiles[u] = TkTile{0, 0, 0, 0};
}

// Tiles of a grouped catalogue: at most floor(N / 32) + G of them (each group wastes less than one tile); 0 when N = 0.
static int64_t topk_grouped_tiles(int64_t N, int32_t G) { return N == 0 ? 0 : (N + 31 * (int64_t)G) / 32; }

static bool topk_grouped_args_ok(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G) {
    return topk_args_ok(B, N, d, k) && G >= 1 && N + 32 * (int64_t)G <= TK_MAX_N;
}

static size_t topk_tile_bytes(int64_t n_tiles) { return ((size_t)n_tiles * sizeof(TkTile) + 255) / 256 * 256; }

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_topk_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    if (!topk_args_ok(B, N, d, k)) return 0;
    const TkGeom g = topk_geom(B, N);
    return 256 + (size_t)B * (size_t)g.S * (size_t)k * sizeof(uint64_t);     // never 0 for accepted arguments
}

// nrms_topk_dot (bias null, who "topk_dot"), nrms_topk_dot_biased, nrms_topk_dot_windowed (windowed: item_time and window are
// required) and nrms_topk_dot_after (cursored: after_scores and after_ids are required): one body, so the checks and the launch
// cannot drift apart.
static int topk_dot_call(const char* who, int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                         const float* bias, bool windowed, const int32_t* item_time, const int32_t* window, const int64_t* exclude,
                         int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace, size_t workspace_bytes,
                         void* stream, bool cursored = false, const float* after_scores = nullptr,
                         const int64_t* after_ids = nullptr) {
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK || B == 0) return rc;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {"item_time", item_time, windowed && N != 0, 4}, {"window", window, windowed, 4},
                             {"after_scores", after_scores, cursored, 4}, {"after_ids", after_ids, cursored, 8},
                             {"top_scores", top_scores, true, 1}, {"top_ids", top_ids, true, 1}},
                       workspace, workspace_bytes, nrms_topk_dot_workspace_bytes(B, N, d, k), 8);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    return topk_launch<false, false>(B, N, d, k, 1, 0, user, items, nullptr, nullptr, exclude, n_exclude, top_scores, top_ids,
                                     (uint64_t*)workspace, s, who, TkNoise{nullptr, 0.0f, 0}, bias,
                                     windowed ? TkWindow{item_time, window} : TkWindow{nullptr, nullptr},
                                     cursored ? TkCursor{after_scores, after_ids, 1} : TkCursor{nullptr, nullptr, 0});
}

extern "C" int nrms_topk_dot(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                             const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return topk_dot_call("topk_dot", B, N, d, k, user, items, nullptr, false, nullptr, nullptr, exclude, n_exclude, top_scores, top_ids, workspace,
                         workspace_bytes, stream);
}

// One page after a cursor.  The workspace is the uncursored call's: the same slice lists, of the entries below the cursor only.
extern "C" size_t nrms_topk_dot_after_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    return nrms_topk_dot_workspace_bytes(B, N, d, k);
}

extern "C" int nrms_topk_dot_after(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                   const float* bias, const int32_t* item_time, const int32_t* window, const float* after_scores,
                                   const int64_t* after_ids, const int64_t* exclude, int32_t n_exclude, float* top_scores,
                                   int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream) {
    // item_time and window go together: either one makes both required (item_time only where there is an item to read it for)
    return topk_dot_call("topk_dot_after", B, N, d, k, user, items, bias, item_time != nullptr || window != nullptr, item_time,
                         window, exclude, n_exclude, top_scores, top_ids, workspace, workspace_bytes, stream, true, after_scores,
                         after_ids);
}

// The deep list: pages of at most TK_MAX_K columns, one after the other in the one workspace of the longest page.
constexpr int TK_DEEP_MAX_K = 4096;

extern "C" size_t nrms_topk_dot_deep_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t K) {
    if (K < 1 || K > TK_DEEP_MAX_K) return 0;
    return nrms_topk_dot_workspace_bytes(B, N, d, std::min(K, TK_MAX_K));
}

extern "C" int nrms_topk_dot_deep(int32_t B, int64_t N, int32_t d, int32_t K, const float* user, const float* items,
                                  const float* bias, const int32_t* item_time, const int32_t* window, const int64_t* exclude,
                                  int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    const char* who = "topk_dot_deep";
    const bool windowed = item_time != nullptr || window != nullptr;
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "K", K, TK_DEEP_MAX_K, n_exclude);
    if (rc != NRMS_OK || B == 0) return rc;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {"item_time", item_time, windowed && N != 0, 4}, {"window", window, windowed, 4},
                             {"top_scores", top_scores, true, 4}, {"top_ids", top_ids, true, 8}},
                       workspace, workspace_bytes, nrms_topk_dot_deep_workspace_bytes(B, N, d, K), 8);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    const TkWindow win = windowed ? TkWindow{item_time, window} : TkWindow{nullptr, nullptr};
    for (int32_t c0 = 0; c0 < K; c0 += TK_MAX_K) {
        // page c0 / 256 fills columns [c0, c0 + k); its cursor is column c0 - 1, which the page before wrote on this stream
        const int32_t k = std::min(TK_MAX_K, K - c0);
        const TkCursor cur = c0 ? TkCursor{top_scores + c0 - 1, top_ids + c0 - 1, K} : TkCursor{nullptr, nullptr, 0};
        rc = topk_launch<false, false>(B, N, d, k, 1, 0, user, items, nullptr, nullptr, exclude, n_exclude, top_scores + c0,
                                       top_ids + c0, (uint64_t*)workspace, s, who, TkNoise{nullptr, 0.0f, 0}, bias, win, cur, K);
        if (rc != NRMS_OK) return rc;
    }
    return NRMS_OK;
}

// The biased call's workspace is the unbiased call's: entries carry s' in the same slice lists.
extern "C" size_t nrms_topk_dot_biased_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    return nrms_topk_dot_workspace_bytes(B, N, d, k);
}

extern "C" int nrms_topk_dot_biased(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                    const float* bias, const int64_t* exclude, int32_t n_exclude, float* top_scores,
                                    int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream) {
    return topk_dot_call("topk_dot_biased", B, N, d, k, user, items, bias, false, nullptr, nullptr, exclude, n_exclude, top_scores,
                         top_ids, workspace, workspace_bytes, stream);
}

// The windowed call's workspace is the unwindowed call's: the same slice lists, of the eligible entries only.
extern "C" size_t nrms_topk_dot_windowed_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    return nrms_topk_dot_workspace_bytes(B, N, d, k);
}

extern "C" int nrms_topk_dot_windowed(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                      const float* bias, const int32_t* item_time, const int32_t* window, const int64_t* exclude,
                                      int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return topk_dot_call("topk_dot_windowed", B, N, d, k, user, items, bias, true, item_time, window, exclude, n_exclude,
                         top_scores, top_ids, workspace, workspace_bytes, stream);
}

extern "C" size_t nrms_topk_grouped_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G) {
    if (!topk_grouped_args_ok(B, N, d, k, G)) return 0;
    const int64_t nt = topk_grouped_tiles(N, G);
    const TkGeom g = topk_geom(B, 32 * nt);
    return 256 + topk_tile_bytes(nt) + (size_t)B * (size_t)g.S * (size_t)k * sizeof(uint64_t);
}

extern "C" int nrms_topk_grouped_dot(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G, const float* query, const float* items,
                                     const int32_t* item_ids, const int64_t* group_ptr, const int64_t* exclude, int32_t n_exclude,
                                     float* top_scores, int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "topk_grouped_dot";
    NRMS_REQUIRE(G >= 1, "%s: G must be >= 1 (G=%d)", who, G);
    int rc = tk_check_dims(who, B, N, TK_MAX_N - 32 * (int64_t)G, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK || B == 0) return rc;
    rc = tk_check_ptrs(who, {{"query", query, true, 1}, {"items", items, N != 0, 1}, {"item_ids", item_ids, N != 0, 1},
                             {"group_ptr", group_ptr, N != 0, 1}, {"top_scores", top_scores, true, 1}, {"top_ids", top_ids, true, 1}},
                       workspace, workspace_bytes, nrms_topk_grouped_dot_workspace_bytes(B, N, d, k, G), 16);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    const int64_t nt = topk_grouped_tiles(N, G);
    TkTile* tiles = (TkTile*)workspace;
    uint64_t* ws = (uint64_t*)((char*)workspace + topk_tile_bytes(nt));
    if (nt > 0) {
        hipLaunchKernelGGL(topk_tiles_kernel, dim3(1), dim3(1024), 0, s, (int)N, G, (int)nt, group_ptr, tiles);
        rc = check_launch("topk_grouped_dot(tiles)");
        if (rc != NRMS_OK) return rc;
    }
    return topk_launch<true, false>(B, N, d, k, G, nt, query, items, item_ids, tiles, exclude, n_exclude, top_scores, top_ids, ws, s,
                                    who);
}
