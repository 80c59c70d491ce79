// Retrieval and ranking inside a per-user set of item tags (include/nrms_hip.h: nrms_topk_dot_tagged and nrms_rank_dot_tagged,
// whose header comment states the contract): "never show me sports", "only the topics I follow", an edition, a publisher block.
//
// nrms_topk_dot_tagged runs the two kernels of nrms_topk_dot: the TAGS instantiations of topk_slice_kernel (topk_kernels.h
// describes them: the block's 32 tag sets transposed once into an LDS bitmap, one LDS word per item, one register bit test per
// score, and a wave none of whose 64 items is open to any user of its block skips its loads and its MFMA chain), with or without
// BIAS, then topk_merge_kernel unchanged.  nrms_rank_dot_tagged runs the three kernels of nrms_rank_dot, the first two in their
// TAGS forms (rankdot.hip, which keeps the rank kernels and the call's body; only the C entry point lives here).
//
// Only this file instantiates the TAGS slice kernels, so topk.hip and softmaxsample.hip compile what they compiled before.
#include "topk_kernels.h"

namespace nrms {

static bool tags_ok(int32_t n_tags) { return n_tags >= 1 && n_tags <= TK_MAX_TAGS; }

// Both kernels of one tagged call: topk_launch's plain path with the TAGS slice kernels.
static int topk_tags_launch(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items, const float* bias,
                            TkTags tags, const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids, uint64_t* ws,
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
                hipLaunchKernelGGL((topk_slice_kernel<p, w, v, false, false, bi, false, TkTags>), grid, block, 0, s, B, (int)N, d, k,
                                   g.slice_len, g.S, user, items, exclude, n_exclude, ws, 1, 0, (const TkTile*)nullptr,
                                   (const int32_t*)nullptr, TkNoise{nullptr, 0.0f, 0}, bias, tags);
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

// The tagged call's workspace is the untagged call's: the same slice lists, of the eligible entries only.
extern "C" size_t nrms_topk_dot_tagged_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k) {
    return nrms_topk_dot_workspace_bytes(B, N, d, k);
}

extern "C" int nrms_topk_dot_tagged(int32_t B, int64_t N, int32_t d, int32_t k, const float* user, const float* items,
                                    const float* bias, const int32_t* item_tag, int32_t n_tags, const uint32_t* allow,
                                    const int64_t* exclude, int32_t n_exclude, float* top_scores, int64_t* top_ids, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* who = "topk_dot_tagged";
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE(tags_ok(n_tags), "%s: n_tags must be in [1, %d] (n_tags=%d)", who, TK_MAX_TAGS, n_tags);
    if (B == 0) return NRMS_OK;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {"item_tag", item_tag, N != 0, 4}, {"allow", allow, true, 4},
                             {"top_scores", top_scores, true, 1}, {"top_ids", top_ids, true, 1}},
                       workspace, workspace_bytes, nrms_topk_dot_tagged_workspace_bytes(B, N, d, k), 8);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    return topk_tags_launch(B, N, d, k, user, items, bias, TkTags{item_tag, allow, n_tags}, exclude, n_exclude, top_scores, top_ids,
                            (uint64_t*)workspace, s, who);
}

// The tagged call's workspace is the untagged call's: the same entries and counts.
extern "C" size_t nrms_rank_dot_tagged_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t T, int32_t n_exclude) {
    return nrms_rank_dot_workspace_bytes(B, N, d, T, n_exclude);
}

extern "C" int nrms_rank_dot_tagged(int32_t B, int64_t N, int32_t d, int32_t T, const float* user, const float* items,
                                    const float* bias, const int32_t* item_tag, int32_t n_tags, const uint32_t* allow,
                                    const int64_t* targets, const int64_t* exclude, int32_t n_exclude, int32_t* ranks,
                                    float* target_scores, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_dot_tagged_call(B, N, d, T, user, items, bias, TkTags{item_tag, allow, n_tags}, targets, exclude, n_exclude, ranks,
                                target_scores, workspace, workspace_bytes, stream);
}
