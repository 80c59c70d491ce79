// Negatives from the model's own softmax over a whole catalogue: S items per user, without replacement, from
// softmax(user . item / temperature), without a [B, N] score matrix (include/nrms_hip.h: nrms_softmax_sample_dot, whose header
// comment states the draw).
//
// Gumbel-top-S: the S largest of s(b, n) / temperature + g(b, n), g i.i.d. standard Gumbel, are a Plackett-Luce draw without
// replacement from softmax(s / temperature).  So this is nrms_topk_dot (csrc/topk.hip) with a perturbation in its epilogue: the
// same slice and merge kernels (topk_kernels.h, NOISE), the same score chain, and each accumulator element turned into its key
// fmaf(score, inv_temperature, g) before it meets its user's threshold.  g is a pure integer function of (seed, row key, item)
// followed by two logf, so a row's draw does not depend on the batch, the slices or the launch geometry.
#include <math.h>

#include "topk_kernels.h"

namespace nrms {

// The test hook: the word and the perturbation of every (row, item) pair, element i = b * N + n.
__global__ __launch_bounds__(256) void softmax_noise_kernel(long total, long N, const int64_t* __restrict__ row_key, uint64_t seed,
                                                            uint32_t* __restrict__ words, float* __restrict__ gumbel) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / N;
        const uint32_t w = tk_noise_word(tk_noise_row_seed(seed, (uint64_t)row_key[b]), (uint32_t)(i - b * N));
        if (words) words[i] = w;
        if (gumbel) gumbel[i] = tk_gumbel(w);
    }
}

static bool softmax_sample_args_ok(int32_t B, int64_t N, int32_t d, int32_t S, int32_t n_exclude) {
    return topk_args_ok(B, N, d, S) && n_exclude >= 0;
}

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_softmax_sample_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t S, int32_t n_exclude) {
    if (!softmax_sample_args_ok(B, N, d, S, n_exclude)) return 0;
    const TkGeom g = topk_geom(B, N);
    return 256 + (size_t)B * (size_t)g.S * (size_t)S * sizeof(uint64_t);     // never 0 for accepted arguments
}

extern "C" int nrms_softmax_sample_dot(int32_t B, int64_t N, int32_t d, int32_t S, const float* user, const float* items,
                                       const int64_t* row_key, float inv_temperature, uint64_t seed, const int64_t* exclude,
                                       int32_t n_exclude, int64_t* ids, float* keys, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    const char* who = "softmax_sample_dot";
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "S", S, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE(inv_temperature >= 0.0f && isfinite(inv_temperature), "%s: inv_temperature must be finite and >= 0 (inv_temperature=%g)",
                 who, (double)inv_temperature);
    if (B == 0) return NRMS_OK;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"row_key", row_key, true, 1}, {"ids", ids, true, 1}},
                       workspace, workspace_bytes, nrms_softmax_sample_dot_workspace_bytes(B, N, d, S, n_exclude), 8);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    return topk_launch<false, true>(B, N, d, S, 1, 0, user, items, nullptr, nullptr, exclude, n_exclude, keys, ids, (uint64_t*)workspace,
                                    s, who, TkNoise{row_key, inv_temperature, seed});
}

extern "C" int nrms_softmax_sample_noise(int32_t B, int64_t N, const int64_t* row_key, uint64_t seed, uint32_t* words, float* gumbel,
                                         void* stream) {
    NRMS_REQUIRE(B >= 0, "softmax_sample_noise: B must be >= 0 (B=%d)", B);
    NRMS_REQUIRE(N >= 0 && N <= TK_MAX_N, "softmax_sample_noise: N must be in [0, %d] (N=%lld)", TK_MAX_N, (long long)N);
    NRMS_REQUIRE(words || gumbel, "softmax_sample_noise: words and gumbel are both null");
    const long total = (long)B * N;
    if (total == 0) return NRMS_OK;
    NRMS_REQUIRE(row_key, "softmax_sample_noise: row_key is null");
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(softmax_noise_kernel, dim3(blocks), dim3(256), 0, s, total, (long)N, row_key, seed, words, gumbel);
    return check_launch("softmax_sample_noise");
}
