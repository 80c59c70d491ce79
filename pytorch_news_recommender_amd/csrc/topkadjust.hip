// Retrieval and ranking with per-user score adjustments (include/nrms_hip.h: nrms_topk_dot_adjusted and nrms_rank_dot_adjusted,
// whose header comment states the contract): impression discounting ("shown three times, not clicked: down by 3 beta"), per-user
// boosts, a per-user block (a NaN delta) that is not the click history.
//
// nrms_topk_dot_adjusted runs the two kernels of nrms_topk_dot: the ADJ instantiations of topk_slice_kernel (topk_kernels.h
// describes them: the block's slots inside its slice compacted once into an LDS list, per step one LDS row of user masks per wave,
// and the lane that holds a marked pair adds the delta of the pair's lowest slot to its accumulator before the filter sees the
// score), with or without BIAS, then topk_merge_kernel unchanged: the slice lists already carry s''.  nrms_rank_dot_adjusted runs
// the three kernels of nrms_rank_dot, the first two in their ADJ forms (rankdot.hip, which keeps the rank kernels and the call's
// body; only the C entry point lives here).
//
// Only this file instantiates the ADJ slice kernels, so topk.hip, topktags.hip, topkcaps.hip and softmaxsample.hip compile what
// they compiled before.
#include "topk_kernels.h"

namespace nrms {

// Both kernels of one adjusted call: topk_launch's plain path with the ADJ slice kernels.
static int topk_adjust_launch(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items, const float* bias,
                              TkAdjust adj, const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids,
                              uint64_t* ws, hipStream_t s, const char* who) {
    const TkGeom g = topk_geom(B, N);
    int rc = NRMS_OK;
    char what[64];
    tk_with_pw(k, [&](auto P, auto W) {
        constexpr int p = decltype(P)::value, w = decltype(W)::value;
        if (g.S > 0) {
            const dim3 grid(g.tiles, g.S), block(64 * w);
            tk_with_flags([&](auto V, auto BI) {
                constexpr bool v = decltype(V)::value, bi = decltype(BI)::value;
                hipLaunchKernelGGL((topk_slice_kernel<p, w, v, false, false, bi, false, TkAdjust>), grid, block, 0, s, B, (int)N, d, k,
                                   g.slice_len, g.S, user, items, exclude, n_exclude, ws, 1, 0, (const TkTile*)nullptr,
                                   (const int32_t*)nullptr, TkNoise{nullptr, 0.0f, 0}, bias, adj);
            }, tk_vec_ok(d, user, items), bias != nullptr);
            snprintf(what, sizeof what, "%s(slices)", who);
            rc = check_launch(what);
            if (rc != NRMS_OK) return;
        }
        hipLaunchKernelGGL(topk_merge_kernel<p>, dim3(B), dim3(64), 0, s, B, k, g.S, ws, top_scores, top_ids, k);
        snprintf(what, sizeof what, "%s(merge)", who);
        rc = check_launch(what);
    });
    return rc;
}

}  // namespace nrms

using namespace nrms;

// The adjusted call's workspace is the unadjusted call's: the same slice lists, of s'' entries.
extern "C" size_t nrms_topk_dot_adjusted_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    return nrms_topk_dot_workspace_bytes(B, N, d, k);
}

extern "C" int nrms_topk_dot_adjusted(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                      const float* bias, const int64_t* adj_ids, const float* adj_delta, int32_t n_adjust,
                                      const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "topk_dot_adjusted";
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK) return rc;
    rc = adjust_check(who, n_adjust, adj_ids, adj_delta);
    if (rc != NRMS_OK || B == 0) return rc;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {"top_scores", top_scores, true, 1}, {"top_ids", top_ids, true, 1}},
                       workspace, workspace_bytes, nrms_topk_dot_adjusted_workspace_bytes(B, N, d, k), 8);
    if (rc != NRMS_OK) return rc;
    if (n_adjust == 0 || !adj_ids)          // no adjustment: the biased / plain call itself
        return nrms_topk_dot_biased(B, N, d, k, user, items, bias, exclude, n_exclude, top_scores, top_ids, workspace, workspace_bytes,
                                    stream);
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    return topk_adjust_launch(B, N, d, k, user, items, bias, TkAdjust{adj_ids, adj_delta, n_adjust}, exclude, n_exclude, top_scores,
                              top_ids, (uint64_t*)workspace, s, who);
}

// The adjusted call's workspace is the unadjusted call's: the same entries and counts.
extern "C" size_t nrms_rank_dot_adjusted_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude) {
    return nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude);
}

extern "C" int nrms_rank_dot_adjusted(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                                      const float* bias, const int64_t* adj_ids, const float* adj_delta, int32_t n_adjust,
                                      const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                                      float* target_scores, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = adjust_check("rank_dot_adjusted", n_adjust, adj_ids, adj_delta);
    if (rc != NRMS_OK) return rc;
    const TkAdjust adj = (n_adjust == 0 || !adj_ids) ? TkAdjust{nullptr, nullptr, 0} : TkAdjust{adj_ids, adj_delta, n_adjust};
    return rank_dot_adjusted_call(B, N, d, T, user, items, bias, adj, targets, exclude, n_exclude, ranks, target_scores, workspace,
                                  workspace_bytes, stream);
}
