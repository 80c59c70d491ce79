// Retrieval with per-category caps (include/nrms_hip.h: nrms_topk_dot_capped, whose header comment states the contract): "at most
// two stories per category in my ten", "one politics story at most for this user".  The capped list is a pure function of
// nrms_topk_dot_biased's total order: walk it, take an item iff its tag has room left, stop after k.
//
// nrms_topk_dot_capped runs two kernels: the CAPS instantiations of topk_slice_kernel (topk_kernels.h describes them: the TAGS
// form with the bitmap built from cap > 0 and tk_select_capped as the filter's selection), with or without BIAS, then
// topk_merge_capped_kernel, tk_merge with the same selection.  One scan is enough because the capped list C(S) of a set S obeys
// C(S1 u S2) = C(C(S1) u C(S2)) (the number of taken items of a tag that precede x is min(cap, #same-tag predecessors), monotone
// in S), and because a threshold is sound once a capped list holds k_b = min(k, sum_t min(max(cap, 0), k)) entries (tk_caps_reach).
//
// Only this file instantiates the CAPS kernels, so every other file compiles what it compiled before.
#include "topk_kernels.h"

namespace nrms {

// Both kernels of one capped call: topk_launch's plain path with the CAPS slice kernels and the capped merge.
static int topk_caps_launch(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items, const float* bias,
                            TkCaps caps, const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids, uint64_t* ws,
                            hipStream_t s, const char* who) {
    const TkGeom g = topk_geom(B, N);
    int rc = NRMS_OK;
    char what[64];
    tk_with_pw(k, [&](auto P, auto W) {
        constexpr int p = decltype(P)::value, w = decltype(W)::value;
        if (g.S > 0) {
            const dim3 grid(g.tiles, g.S), block(64 * w);
            tk_with_flags([&](auto V, auto BI) {
                constexpr bool v = decltype(V)::value, bi = decltype(BI)::value;
                hipLaunchKernelGGL((topk_slice_kernel<p, w, v, false, false, bi, false, TkCaps>), grid, block, 0, s, B, (int)N, d, k,
                                   g.slice_len, g.S, user, items, exclude, n_exclude, ws, 1, 0, (const TkTile*)nullptr,
                                   (const int32_t*)nullptr, TkNoise{nullptr, 0.0f, 0}, bias, caps);
            }, tk_vec_ok(d, user, items), bias != nullptr);
            snprintf(what, sizeof what, "%s(slices)", who);
            rc = check_launch(what);
            if (rc != NRMS_OK) return;
        }
        hipLaunchKernelGGL(topk_merge_capped_kernel<p>, dim3(B), dim3(64), 0, s, B, k, g.S, ws, caps, top_scores, top_ids);
        snprintf(what, sizeof what, "%s(merge)", who);
        rc = check_launch(what);
    });
    return rc;
}

}  // namespace nrms

using namespace nrms;

// The capped call's workspace is the uncapped call's: the same slice lists, of the taken entries only.
extern "C" size_t nrms_topk_dot_capped_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    return nrms_topk_dot_workspace_bytes(B, N, d, k);
}

extern "C" int nrms_topk_dot_capped(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                    const float* bias, const int32_t* item_tag, int32_t n_tags, const int32_t* cap,
                                    const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* who = "topk_dot_capped";
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE(n_tags >= 1 && n_tags <= TK_MAX_TAGS, "%s: n_tags must be in [1, %d] (n_tags=%d)", who, TK_MAX_TAGS, n_tags);
    if (B == 0) return NRMS_OK;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {"item_tag", item_tag, N != 0, 4}, {"cap", cap, true, 4},
                             {"top_scores", top_scores, true, 1}, {"top_ids", top_ids, true, 1}},
                       workspace, workspace_bytes, nrms_topk_dot_capped_workspace_bytes(B, N, d, k), 8);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    return topk_caps_launch(B, N, d, k, user, items, bias, TkCaps{item_tag, cap, n_tags}, exclude, n_exclude, top_scores, top_ids,
                            (uint64_t*)workspace, s, who);
}
