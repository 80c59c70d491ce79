// One request through several catalogue filters at once (include/nrms_hip.h: nrms_topk_dot_request and nrms_rank_dot_request,
// whose header comment states the composition): news that is still live (a time window), outside the topics this user muted (a tag
// set), with what they were already shown pushed down (adjustments), after the page they have just seen (a cursor).
//
// Routing.  No part or one part: the existing entry point (nrms_topk_dot_biased, _windowed, _tagged, _adjusted, _after), and window
// + cursor: nrms_topk_dot_after, which has held that pair since the cursor was added; those paths run the device code they ran
// before.  Every other combination runs the REQ instantiations of topk_slice_kernel (topk_kernels.h describes them: the four
// parts' stages side by side, each behind a block-uniform branch on its pointer), with or without BIAS, then topk_merge_kernel
// unchanged: the slice lists carry s'' entries of eligible pairs only.  nrms_rank_dot_request runs the three kernels of
// nrms_rank_dot, the first two in their REQ forms (rankdot.hip keeps the rank kernels and the call's body).
//
// Only this file instantiates the REQ slice kernels, so every other translation unit compiles what it compiled before.
#include "topk_kernels.h"

namespace nrms {

// Both kernels of one request: topk_launch's plain path with the REQ slice kernels.
static int topk_request_launch(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items, const float* bias,
                               TkRequest req, const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids,
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
                hipLaunchKernelGGL((topk_slice_kernel<p, w, v, false, false, bi, false, TkRequest>), grid, block, 0, s, B, (int)N, d, k,
                                   g.slice_len, g.S, user, items, exclude, n_exclude, ws, 1, 0, (const TkTile*)nullptr,
                                   (const int32_t*)nullptr, TkNoise{nullptr, 0.0f, 0}, bias, req);
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

// The parts of a request as the caller gave them: a pair is present when either of its pointers is (the adjustments: with
// n_adjust > 0), and then both are required.
struct RequestParts {
    bool window, tags, adjust, cursor;
    int count() const { return (int)window + (int)tags + (int)adjust + (int)cursor; }
};

// The checks both request calls make before they route: the pairs (a half-given pair names its missing pointer), n_tags and E.
static int request_check(const char* who, int64_t N, const int32_t* item_time, const int32_t* window, const int32_t* item_tag,
                         int32_t n_tags, const uint32_t* allow, const int64_t* adj_ids, const float* adj_delta, int32_t n_adjust,
                         const float* after_scores, const int64_t* after_ids, RequestParts& parts) {
    parts.window = item_time != nullptr || window != nullptr;
    parts.tags = item_tag != nullptr || allow != nullptr;
    parts.cursor = after_scores != nullptr || after_ids != nullptr;
    NRMS_REQUIRE(!parts.window || window, "%s: window is null (item_time is given)", who);
    NRMS_REQUIRE(!parts.window || item_time || N == 0, "%s: item_time is null (window is given)", who);
    NRMS_REQUIRE(!parts.tags || allow, "%s: allow is null (item_tag is given)", who);
    NRMS_REQUIRE(!parts.tags || item_tag || N == 0, "%s: item_tag is null (allow is given)", who);
    NRMS_REQUIRE(!parts.tags || (n_tags >= 1 && n_tags <= TK_MAX_TAGS), "%s: n_tags must be in [1, %d] (n_tags=%d)", who,
                 TK_MAX_TAGS, n_tags);
    const int rc = adjust_check(who, n_adjust, adj_ids, adj_delta);
    if (rc != NRMS_OK) return rc;
    parts.adjust = n_adjust > 0 && adj_ids != nullptr;
    NRMS_REQUIRE(!parts.cursor || after_scores, "%s: after_scores is null (after_ids is given)", who);
    NRMS_REQUIRE(!parts.cursor || after_ids, "%s: after_ids is null (after_scores is given)", who);
    return NRMS_OK;
}

}  // namespace nrms

using namespace nrms;

// The request's workspace is the plain call's: the same slice lists, of the s'' entries of the eligible pairs.
extern "C" size_t nrms_topk_dot_request_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    return nrms_topk_dot_workspace_bytes(B, N, d, k);
}

extern "C" int nrms_topk_dot_request(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                     const float* bias, const int32_t* item_time, const int32_t* window, const int32_t* item_tag,
                                     int32_t n_tags, const uint32_t* allow, const int64_t* adj_ids, const float* adj_delta,
                                     int32_t n_adjust, const float* after_scores, const int64_t* after_ids, const int64_t* exclude,
                                     int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    const char* who = "topk_dot_request";
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK) return rc;
    RequestParts parts;
    rc = request_check(who, N, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta, n_adjust, after_scores, after_ids, parts);
    if (rc != NRMS_OK || B == 0) return rc;
    // no part, one part, window + cursor: the existing call, its own checks and its own device code
    if (parts.count() == 0)
        return nrms_topk_dot_biased(B, N, d, k, user, items, bias, exclude, n_exclude, top_scores, top_ids, workspace, workspace_bytes,
                                    stream);
    if (parts.cursor && !parts.tags && !parts.adjust)
        return nrms_topk_dot_after(B, N, d, k, user, items, bias, item_time, window, after_scores, after_ids, exclude, n_exclude,
                                   top_scores, top_ids, workspace, workspace_bytes, stream);
    if (parts.count() == 1) {
        if (parts.window)
            return nrms_topk_dot_windowed(B, N, d, k, user, items, bias, item_time, window, exclude, n_exclude, top_scores, top_ids,
                                          workspace, workspace_bytes, stream);
        if (parts.tags)
            return nrms_topk_dot_tagged(B, N, d, k, user, items, bias, item_tag, n_tags, allow, exclude, n_exclude, top_scores, top_ids,
                                        workspace, workspace_bytes, stream);
        return nrms_topk_dot_adjusted(B, N, d, k, user, items, bias, adj_ids, adj_delta, n_adjust, exclude, n_exclude, top_scores,
                                      top_ids, workspace, workspace_bytes, stream);
    }
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {"item_time", item_time, false, 4}, {"window", window, false, 4},
                             {"item_tag", item_tag, false, 4}, {"allow", allow, false, 4},
                             {"after_scores", after_scores, false, 4}, {"after_ids", after_ids, false, 8},
                             {"top_scores", top_scores, true, 1}, {"top_ids", top_ids, true, 1}},
                       workspace, workspace_bytes, nrms_topk_dot_request_workspace_bytes(B, N, d, k), 8);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    const TkRequest req{parts.window ? TkWindow{item_time, window} : TkWindow{nullptr, nullptr},
                        parts.tags ? TkTags{item_tag, allow, n_tags} : TkTags{nullptr, nullptr, 0},
                        parts.adjust ? TkAdjust{adj_ids, adj_delta, n_adjust} : TkAdjust{nullptr, nullptr, 0},
                        parts.cursor ? TkCursor{after_scores, after_ids, 1} : TkCursor{nullptr, nullptr, 0}};
    return topk_request_launch(B, N, d, k, user, items, bias, req, exclude, n_exclude, top_scores, top_ids, (uint64_t*)workspace, s,
                               who);
}

// The request's workspace is the plain call's: the same entries and counts.
extern "C" size_t nrms_rank_dot_request_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude) {
    return nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude);
}

extern "C" int nrms_rank_dot_request(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                                     const float* bias, const int32_t* item_time, const int32_t* window, const int32_t* item_tag,
                                     int32_t n_tags, const uint32_t* allow, const int64_t* adj_ids, const float* adj_delta,
                                     int32_t n_adjust, const int64_t* targets, const int64_t* exclude, int32_t n_exclude,
                                     int32_t* ranks, float* target_scores, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "rank_dot_request";
    RequestParts parts;
    const int rc = request_check(who, N, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta, n_adjust, nullptr, nullptr,
                                 parts);
    if (rc != NRMS_OK) return rc;
    if (parts.count() == 0)
        return nrms_rank_dot_biased(B, N, d, T, user, items, bias, targets, exclude, n_exclude, ranks, target_scores, workspace,
                                    workspace_bytes, stream);
    if (parts.count() == 1) {
        if (parts.window)
            return nrms_rank_dot_windowed(B, N, d, T, user, items, bias, item_time, window, targets, exclude, n_exclude, ranks,
                                          target_scores, workspace, workspace_bytes, stream);
        if (parts.tags)
            return nrms_rank_dot_tagged(B, N, d, T, user, items, bias, item_tag, n_tags, allow, targets, exclude, n_exclude, ranks,
                                        target_scores, workspace, workspace_bytes, stream);
        return nrms_rank_dot_adjusted(B, N, d, T, user, items, bias, adj_ids, adj_delta, n_adjust, targets, exclude, n_exclude, ranks,
                                      target_scores, workspace, workspace_bytes, stream);
    }
    const TkRequest req{parts.window ? TkWindow{item_time, window} : TkWindow{nullptr, nullptr},
                        parts.tags ? TkTags{item_tag, allow, n_tags} : TkTags{nullptr, nullptr, 0},
                        parts.adjust ? TkAdjust{adj_ids, adj_delta, n_adjust} : TkAdjust{nullptr, nullptr, 0},
                        TkCursor{nullptr, nullptr, 0}};
    return rank_dot_request_call(B, N, d, T, user, items, bias, req, targets, exclude, n_exclude, ranks, target_scores, workspace,
                                 workspace_bytes, stream);
}
