// Greedy maximal-marginal-relevance re-ranking of a per-user shortlist (include/nrms_hip.h: nrms_mmr_rerank, whose header
// comment states the contract: which entries are valid, the relevance, the cosine, the value v, the order and the padding).
//
// Two kernels:
// A (mmr_gram_kernel): per user the M x M matrix of raw dot products of the item rows the shortlist names, into the workspace
//   (pitch Mp = M rounded up to 64, entries that name no row read row 0 and are never used).  One wave per 64 x 64 block of
//   the upper block triangle: 2 x 2 tiles of v_mfma_f32_32x32x2_f32, every operand row read straight from global memory (16
//   contiguous floats per lane and block of 32 floats of k, the next block in flight while the MFMAs of this one run), one
//   accumulator per (i, j) over all of d.  The k order is the same for every pair and a product commutes, so dot(i, j) and
//   dot(j, i) have the same bits whichever tile formed them; blocks above the diagonal are stored a second time, transposed
//   (four consecutive rows of a lane's accumulator are one float4 of the mirrored row).
// B (mmr_greedy_kernel): one wave per user.  Lane l holds entries l, l + 64, l + 128, l + 192: validity, relevance, 1 / norm
//   (from the Gram diagonal) and the running maximum similarity to the picks.  Each step is a wave argmax over a uint64 key
//   (the value as an order-preserving 32-bit key above the complement of the position: larger key = larger v, then the
//   smaller position; NaN below every number), one coalesced read of the pick's Gram row and four multiplies per lane.  The
//   ILD sum runs over the picked pairs in pick order through a 256-float LDS copy of the step's cosine row.
//
// The Gram matrix costs 2 M^2 d flops per user once (upper triangle: a little over half of that) and each greedy step then
// reads 4 Mp bytes; recomputing cos(pick, .) per step from the gathered rows instead re-reads M d floats per step
// (docs/EXPERIMENTS.md).
#include "topk_entry.h"

namespace nrms {

constexpr int MMR_MAX_M = 256;
constexpr int MMR_ST = 64;                     // Gram block per wave (2 x 2 MFMA tiles), and the pitch granule
constexpr int MMR_GRID_B = 32768;              // users per launch (grid.y)

__host__ __device__ inline int mmr_pitch(int M) { return (M + MMR_ST - 1) / MMR_ST * MMR_ST; }

// Kernel A.  Block (x, y): block pair x of the upper block triangle (ti <= tj) of user b0 + y.  Needs N >= 1.
template <bool VEC>
__global__ __launch_bounds__(64) void mmr_gram_kernel(int M, int Mp, int d, long N, const float* __restrict__ items,
                                                      const int64_t* __restrict__ short_ids, float* __restrict__ gram) {
    const int lane = threadIdx.x;
    const int r = lane & 31, h = lane >> 5;
    const int T = Mp / MMR_ST;
    int p = blockIdx.x, ti = 0;
    while (p >= T - ti) {
        p -= T - ti;
        ++ti;
    }
    const int tj = ti + p;
    const long b = blockIdx.y;
    const int64_t* ids = short_ids + b * M;
    float* G = gram + b * Mp * Mp;
    // rows 0, 1: the two 32-row tiles of block row ti (A operands); rows 2, 3: of block column tj (B operands).  A position
    // past M or an id outside [0, N) reads row 0: its products are never used.
    const float* row[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int pos = MMR_ST * (c < 2 ? ti : tj) + 32 * (c & 1) + r;
        const int64_t id = pos < M ? ids[pos] : -1;
        row[c] = items + (id >= 0 && id < N ? id : 0) * d;
    }
    tk_f32x16 acc[2][2];
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) acc[ia][jb] = tk_f32x16{};
    const int m_full = d / 32;
    // block m of 32 floats of k: lane (r, h) holds floats 32m + 16h .. + 15 of its four rows; MFMA t sums k = 32m + t (h = 0)
    // and 32m + 16 + t (h = 1)
#define MMR_GLOAD(dst, m)                                                                                                  \
    do {                                                                                                                   \
        const int k0_ = 32 * (m) + 16 * h;                                                                                 \
        _Pragma("unroll") for (int c_ = 0; c_ < 4; ++c_) {                                                                 \
            if (VEC) {                                                                                                     \
                _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) {                                                         \
                    const float4 v_ = *reinterpret_cast<const float4*>(row[c_] + k0_ + 4 * q_);                            \
                    dst[c_][4 * q_] = v_.x; dst[c_][4 * q_ + 1] = v_.y; dst[c_][4 * q_ + 2] = v_.z; dst[c_][4 * q_ + 3] = v_.w; \
                }                                                                                                          \
            } else {                                                                                                       \
                _Pragma("unroll") for (int t_ = 0; t_ < 16; ++t_) dst[c_][t_] = row[c_][k0_ + t_];                         \
            }                                                                                                              \
        }                                                                                                                  \
    } while (0)
    if (m_full > 0) {
        float nx[4][16];
        MMR_GLOAD(nx, 0);
        for (int m = 0; m < m_full; ++m) {
            float cur[4][16];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int t = 0; t < 16; ++t) cur[c][t] = nx[c][t];
            if (m + 1 < m_full) MMR_GLOAD(nx, m + 1);
#pragma unroll
            for (int t = 0; t < 16; ++t)
#pragma unroll
                for (int ia = 0; ia < 2; ++ia)
#pragma unroll
                    for (int jb = 0; jb < 2; ++jb)
                        acc[ia][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[ia][t], cur[2 + jb][t], acc[ia][jb], 0, 0, 0);
        }
    }
#undef MMR_GLOAD
    for (int k0 = 32 * m_full; k0 < d; k0 += 8) {       // zero-padded groups of 8 past the last whole block
        const int kk = k0 + 4 * h;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float x[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = tk_ld(row[c], kk + t, d);
#pragma unroll
            for (int ia = 0; ia < 2; ++ia)
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
                    acc[ia][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[ia], x[2 + jb], acc[ia][jb], 0, 0, 0);
        }
    }
    // C/D layout: column = lane & 31 of the tile, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5).  Every index is below Mp.
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            const int i0 = MMR_ST * ti + 32 * ia, j0 = MMR_ST * tj + 32 * jb;
#pragma unroll
            for (int q = 0; q < 16; ++q) G[(long)(i0 + (q & 3) + 8 * (q >> 2) + 4 * h) * Mp + j0 + r] = acc[ia][jb][q];
            if (ti != tj) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<float4*>(G + (long)(j0 + r) * Mp + i0 + 8 * g + 4 * h) =
                        make_float4(acc[ia][jb][4 * g], acc[ia][jb][4 * g + 1], acc[ia][jb][4 * g + 2], acc[ia][jb][4 * g + 3]);
            }
        }
}

// The order of the greedy argmax as one integer: larger = larger v (-0.0 as +0.0), then the smaller position; a NaN v below
// every number.  Never 0, which stands for "not a candidate".
__device__ __forceinline__ uint64_t mmr_key(float v, int pos) {
    uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (__builtin_isnan(v)) u = 0;
    return ((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)pos);
}

// Kernel B.  One wave per user.  gram is not read when the row has no valid entry (N = 0: it is null).
__global__ __launch_bounds__(64) void mmr_greedy_kernel(int M, int Mp, int k, long N, float lambda,
                                                        const int64_t* __restrict__ short_ids,
                                                        const float* __restrict__ short_scores, const float* __restrict__ gram,
                                                        int64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                        float* __restrict__ out_value, float* __restrict__ ild) {
    __shared__ float rinv[MMR_MAX_M];
    __shared__ float simrow[MMR_MAX_M];
    __shared__ int picks[MMR_MAX_M];
    constexpr int E = MMR_MAX_M / 64;
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const float* G = gram + b * Mp * Mp;
    const float inf = __builtin_huge_valf();

    int64_t id[E];
    float s[E], rel[E], rn[E], ms[E];
    bool live[E];                                // valid and not yet picked
    float lo = inf, hi = -inf;
    int n_valid = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        id[e] = i < M ? short_ids[b * M + i] : -1;
        s[e] = i < M ? short_scores[b * M + i] : 0.0f;
        live[e] = i < M && id[e] >= 0 && id[e] < N && __builtin_fabsf(s[e]) < inf;
        if (live[e]) {
            lo = fminf(lo, s[e]);
            hi = fmaxf(hi, s[e]);
        }
        n_valid += __popcll(__ballot(live[e]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    const float range = __fsub_rn(hi, lo);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        rel[e] = (live[e] && hi != lo) ? __fdiv_rn(__fsub_rn(s[e], lo), range) : 0.0f;
        const float dd = live[e] ? G[(long)i * Mp + i] : 0.0f;
        rn[e] = (dd > 0.0f && dd < inf) ? __fdiv_rn(1.0f, __fsqrt_rn(dd)) : 0.0f;
        rinv[i] = rn[e];
        ms[e] = 0.0f;
    }
    tk_wave_sync();

    const float c1 = __fsub_rn(1.0f, lambda);
    const int n = min(k, n_valid);
    float pair_sum = 0.0f;
    for (int t = 0; t < n; ++t) {
        float v[E];
        uint64_t best = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            v[e] = __fsub_rn(__fmul_rn(lambda, rel[e]), __fmul_rn(c1, ms[e]));
            const uint64_t key = live[e] ? mmr_key(v[e], lane + 64 * e) : 0;
            best = key > best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)best, o, 64);
            best = other > best ? other : best;
        }
        const int p = (int)(0xFFFFFFFFu - (uint32_t)best);           // n <= #valid: a candidate is left, best != 0
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (lane + 64 * e == p) {
                out_ids[b * k + t] = id[e];
                out_scores[b * k + t] = s[e];
                if (out_value) out_value[b * k + t] = v[e];
                live[e] = false;
            }
        }
        const float rp = rinv[p];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + 64 * e;
            const float g = i < Mp ? G[(long)p * Mp + i] : 0.0f;
            const float cs = __fmul_rn(g, __fmul_rn(rn[e], rp));
            ms[e] = t == 0 ? cs : fmaxf(ms[e], cs);
            if (ild) simrow[i] = cs;
        }
        if (ild) {
            tk_wave_sync();
            for (int u = 0; u < t; ++u) pair_sum = __fadd_rn(pair_sum, simrow[picks[u]]);
            if (lane == 0) picks[t] = p;
            tk_wave_sync();
        }
    }
    for (int j = n + lane; j < k; j += 64) {
        out_ids[b * k + j] = -1;
        out_scores[b * k + j] = -inf;
        if (out_value) out_value[b * k + j] = -inf;
    }
    if (ild && lane == 0)
        ild[b] = n < 2 ? __builtin_nanf("") : __fsub_rn(1.0f, __fdiv_rn(pair_sum, (float)(n * (n - 1) / 2)));
}

static bool mmr_args_ok(int32_t B, int32_t M, int32_t d, int32_t k, int64_t N, float lambda) {
    return B >= 0 && M >= 1 && M <= MMR_MAX_M && k >= 1 && k <= M && d >= 1 && N >= 0 && lambda >= 0.0f && lambda <= 1.0f;
}

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_mmr_rerank_workspace_bytes(int32_t B, int32_t M, int32_t d, int32_t k) {
    if (!mmr_args_ok(B, M, d, k, 0, 0.0f)) return 0;
    const size_t mp = (size_t)mmr_pitch(M);
    return 256 + (size_t)B * mp * mp * sizeof(float);        // the Gram matrices [B, Mp, Mp]; never 0 for accepted arguments
}

extern "C" int nrms_mmr_rerank(int32_t B, int32_t M, int32_t d, int32_t k, int64_t N, float lambda, const float* items,
                               const int64_t* short_ids, const float* short_scores, int64_t* out_ids, float* out_scores,
                               float* out_value, float* ild, void* workspace, size_t workspace_bytes, void* stream) {
    NRMS_REQUIRE(B >= 0, "mmr_rerank: B must be >= 0 (B=%d)", B);
    NRMS_REQUIRE(M >= 1 && M <= MMR_MAX_M, "mmr_rerank: M must be in [1, %d] (M=%d)", MMR_MAX_M, M);
    NRMS_REQUIRE(d >= 1, "mmr_rerank: d must be >= 1 (d=%d)", d);
    NRMS_REQUIRE(k >= 1 && k <= M, "mmr_rerank: k must be in [1, M] (k=%d, M=%d)", k, M);
    NRMS_REQUIRE(N >= 0, "mmr_rerank: N must be >= 0 (N=%lld)", (long long)N);
    NRMS_REQUIRE(lambda >= 0.0f && lambda <= 1.0f, "mmr_rerank: lambda must be in [0, 1] (lambda=%g)", (double)lambda);
    if (B == 0) return NRMS_OK;
    NRMS_REQUIRE(items || N == 0, "mmr_rerank: items is null");
    NRMS_REQUIRE(short_ids, "mmr_rerank: short_ids is null");
    NRMS_REQUIRE(short_scores, "mmr_rerank: short_scores is null");
    NRMS_REQUIRE(out_ids, "mmr_rerank: out_ids is null");
    NRMS_REQUIRE(out_scores, "mmr_rerank: out_scores is null");
    NRMS_REQUIRE(workspace, "mmr_rerank: workspace is null");
    const size_t need = nrms_mmr_rerank_workspace_bytes(B, M, d, k);
    if (workspace_bytes < need) {
        set_error("mmr_rerank: workspace %zu < required %zu bytes", workspace_bytes, need);
        return NRMS_EWORKSPACE;
    }
    NRMS_REQUIRE(((uintptr_t)workspace & 15) == 0, "mmr_rerank: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts("mmr_rerank", s);
    const int Mp = mmr_pitch(M);
    const int T = Mp / MMR_ST;
    float* gram = (float*)workspace;
    const bool vec = (d & 3) == 0 && ((uintptr_t)items & 15) == 0;
    for (int64_t b0 = 0; b0 < B; b0 += MMR_GRID_B) {
        const int nb = (int)std::min<int64_t>(MMR_GRID_B, B - b0);
        if (N > 0) {
            const dim3 grid(T * (T + 1) / 2, nb);
            float* g = gram + (size_t)b0 * Mp * Mp;
            if (vec) hipLaunchKernelGGL(mmr_gram_kernel<true>, grid, dim3(64), 0, s, M, Mp, d, (long)N, items, short_ids + b0 * M, g);
            else hipLaunchKernelGGL(mmr_gram_kernel<false>, grid, dim3(64), 0, s, M, Mp, d, (long)N, items, short_ids + b0 * M, g);
            const int rc = check_launch("mmr_rerank(gram)");
            if (rc != NRMS_OK) return rc;
        }
    }
    hipLaunchKernelGGL(mmr_greedy_kernel, dim3(B), dim3(64), 0, s, M, Mp, k, (long)N, lambda, short_ids, short_scores,
                       N > 0 ? gram : nullptr, out_ids, out_scores, out_value, ild);
    return check_launch("mmr_rerank(greedy)");
}
