// Per-category caps through the request (include/nrms_hip.h: nrms_topk_dot_request_capped, whose header comment states the
// contract): the capped list of nrms_topk_dot_capped, walked over the items that nrms_topk_dot_request leaves eligible: inside the
// user's time window, outside the topics they muted, with what they were shown pushed down, after the page they have just seen.
//
// Both statements that make one scan of nrms_topk_dot_capped exact are statements about a set of eligible items under a total
// order: C(S1 u S2) = C(C(S1) u C(S2)), and the k_b threshold (tk_caps_reach).  Neither asks which filters produced the set or
// which score the order was formed from, so the REQ form's s'' and its open predicate go in front of the CAPS form's selection
// unchanged, and a cursor only makes the set smaller.
//
// Routing.  No window, no tag set, no adjustments and no cursor: nrms_topk_dot_capped, its own device code.  Everything else runs
// the REQ + CAPS instantiations of topk_slice_kernel (topk_kernels.h: the pack holds a TkRequest and a TkCaps), with or without
// BIAS, then topk_merge_capped_kernel unchanged: the slice lists are capped lists of s'' entries of eligible pairs.
//
// Only this file instantiates the REQ + CAPS slice kernels, so every other translation unit compiles what it compiled before.
#include "topk_kernels.h"

namespace nrms {

// Both kernels of one capped request: topk_launch's plain path with the REQ + CAPS slice kernels and the capped merge.
static int topk_request_caps_launch(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                    const float* bias, TkRequest req, TkCaps caps, const int64_t* exclude, int32_t n_exclude,
                                    float* top_scores, int64_t* top_ids, uint64_t* ws, hipStream_t s, const char* who) {
    const TkGeom g = topk_geom(B, N);
    int rc = NRMS_OK;
    char what[64];
    tk_with_pw(k, [&](auto P, auto W) {
        constexpr int p = decltype(P)::value, w = decltype(W)::value;
        if (g.S > 0) {
            const dim3 grid(g.tiles, g.S), block(64 * w);
            tk_with_flags([&](auto V, auto BI) {
                constexpr bool v = decltype(V)::value, bi = decltype(BI)::value;
                hipLaunchKernelGGL((topk_slice_kernel<p, w, v, false, false, bi, false, TkRequest, TkCaps>), grid, block, 0, s, B,
                                   (int)N, d, k, g.slice_len, g.S, user, items, exclude, n_exclude, ws, 1, 0, (const TkTile*)nullptr,
                                   (const int32_t*)nullptr, TkNoise{nullptr, 0.0f, 0}, bias, req, caps);
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

// The capped request's workspace is the plain call's: the same slice lists, of the taken s'' entries only.
extern "C" size_t nrms_topk_dot_request_capped_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    return nrms_topk_dot_workspace_bytes(B, N, d, k);
}

extern "C" int nrms_topk_dot_request_capped(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                            const float* bias, const int32_t* item_time, const int32_t* window,
                                            const int32_t* item_tag, int32_t n_tags, const uint32_t* allow, const int32_t* cap,
                                            const int64_t* adj_ids, const float* adj_delta, int32_t n_adjust,
                                            const float* after_scores, const int64_t* after_ids, const int64_t* exclude,
                                            int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    const char* who = "topk_dot_request_capped";
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE(n_tags >= 1 && n_tags <= TK_MAX_TAGS, "%s: n_tags must be in [1, %d] (n_tags=%d)", who, TK_MAX_TAGS, n_tags);
    // the tags and the caps are required; every other part is a pair given as both pointers or neither
    const bool has_window = item_time != nullptr || window != nullptr;
    const bool has_cursor = after_scores != nullptr || after_ids != nullptr;
    NRMS_REQUIRE(!has_window || window, "%s: window is null (item_time is given)", who);
    NRMS_REQUIRE(!has_window || item_time || N == 0, "%s: item_time is null (window is given)", who);
    rc = adjust_check(who, n_adjust, adj_ids, adj_delta);
    if (rc != NRMS_OK) return rc;
    const bool has_adjust = n_adjust > 0 && adj_ids != nullptr;
    NRMS_REQUIRE(!has_cursor || after_scores, "%s: after_scores is null (after_ids is given)", who);
    NRMS_REQUIRE(!has_cursor || after_ids, "%s: after_ids is null (after_scores is given)", who);
    if (B == 0) return NRMS_OK;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {"item_time", item_time, false, 4}, {"window", window, false, 4},
                             {"item_tag", item_tag, N != 0, 4}, {"allow", allow, false, 4}, {"cap", cap, true, 4},
                             {"after_scores", after_scores, false, 4}, {"after_ids", after_ids, false, 8},
                             {"top_scores", top_scores, true, 1}, {"top_ids", top_ids, true, 1}},
                       workspace, workspace_bytes, nrms_topk_dot_request_capped_workspace_bytes(B, N, d, k), 8);
    if (rc != NRMS_OK) return rc;
    // the caps alone: the capped call, its own device code
    if (!has_window && !allow && !has_adjust && !has_cursor)
        return nrms_topk_dot_capped(B, N, d, k, user, items, bias, item_tag, n_tags, cap, exclude, n_exclude, top_scores, top_ids,
                                    workspace, workspace_bytes, stream);
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    const TkRequest req{has_window ? TkWindow{item_time, window} : TkWindow{nullptr, nullptr},
                        allow ? TkTags{item_tag, allow, n_tags} : TkTags{nullptr, nullptr, 0},
                        has_adjust ? TkAdjust{adj_ids, adj_delta, n_adjust} : TkAdjust{nullptr, nullptr, 0},
                        has_cursor ? TkCursor{after_scores, after_ids, 1} : TkCursor{nullptr, nullptr, 0}};
    return topk_request_caps_launch(B, N, d, k, user, items, bias, req, TkCaps{item_tag, cap, n_tags}, exclude, n_exclude,
                                    top_scores, top_ids, (uint64_t*)workspace, s, who);
}
