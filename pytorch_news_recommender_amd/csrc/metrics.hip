// Per-impression ranking metrics of the MIND scorer (AUC, MRR, nDCG@k_a, nDCG@k_b) and the submission
// ranks of test(), in one pass over the candidate pairs of each impression (include/nrms_hip.h:
// nrms_impression_metrics).  Tie rule (one place: the header comment of nrms_impression_metrics):
//   metric rank     rank_m(i) = 1 + #{j : s_j > s_i} + #{j > i : s_j == s_i}   (later slot first)
//   submission rank rank_s(i) = 1 + #{j : s_j > s_i} + #{j < i : s_j == s_i}   (earlier slot first, NaN last)
#include "common.h"

namespace nrms {

constexpr int MET_STAGE = 512;        // candidates of one row staged in LDS per wave (a multiple of 64)
constexpr int MET_WAVES = 4;

__device__ __forceinline__ void met_wave_sync() {
    // LDS operations of one wave execute in issue order; this only stops the compiler from moving
    // LDS accesses across the restaging boundary.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double met_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);       // fixed butterfly: run-to-run bit-identical
    return v;
}

// Stages candidates [c0, c0 + MET_STAGE) of the row; slots at or past n get a NaN score, which every
// comparison of the sweep rejects, so the sweep may run over whole groups of 4.
__device__ __forceinline__ void met_stage(const float* s, const uint8_t* y, int n, int c0, float* ls, uint8_t* ly, int lane) {
    for (int c = lane; c < MET_STAGE; c += 64) {
        const int g = c0 + c;
        const bool in = g < n;
        ls[c] = in ? s[g] : __int_as_float(0x7FC00000);
        ly[c] = in ? y[g] : (uint8_t)0;
    }
}

// One wave per impression.  Lane l owns candidates i = l, l + 64, ...; one sweep over j per owned i
// counts, from the same two comparisons, the scores above s_i (gt), equal to it (eq, i itself included),
// equal to it at an earlier slot (eqb), and the same for negatives only (gtn, eqn).  Counts are integers;
// f64 appears only in the final sums and divisions.
__global__ __launch_bounds__(64 * MET_WAVES) void impression_metrics_kernel(
    int n_imp, int max_c, const float* __restrict__ scores, const uint8_t* __restrict__ labels,
    const int32_t* __restrict__ lens, int k_a, int k_b, double* auc, double* mrr, double* ndcg_a, double* ndcg_b,
    int32_t* ranks) {
    __shared__ __attribute__((aligned(16))) float lds_s[MET_WAVES][MET_STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t lds_y[MET_WAVES][MET_STAGE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int imp = blockIdx.x * MET_WAVES + wave;
    if (imp >= n_imp) return;
    const int n = max(0, min(lens[imp], max_c));
    const float* s = scores + (long)imp * max_c;
    const uint8_t* y = labels + (long)imp * max_c;
    float* ls = lds_s[wave];
    uint8_t* ly = lds_y[wave];
    const unsigned long long below = (1ull << lane) - 1ull;

    // prologue: stage the first chunk (NaN-padded up to a multiple of 64); count positives, NaN scores and
    // NaN-scored negatives of the prefix
    int npos = 0, n_nan = 0, nan_neg = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < n;
        const float v = in ? s[c] : __int_as_float(0x7FC00000);
        const uint8_t yc = in ? y[c] : (uint8_t)0;
        if (c < MET_STAGE) {
            ls[c] = v;
            ly[c] = yc;
        }
        const bool isn = in && __builtin_isnan(v);
        npos += __popcll(__ballot(in && yc != 0));
        n_nan += __popcll(__ballot(isn));
        nan_neg += __popcll(__ballot(isn && yc == 0));
    }
    met_wave_sync();
    const int nneg = n - npos;
    const int n_chunks = (n + MET_STAGE - 1) / MET_STAGE;
    int staged = 0;

    unsigned long long twice = 0;        // 2 #{pos > neg} + #{pos == neg}: nrms_impression_auc's statistic
    double rr = 0.0, dcg_a = 0.0, dcg_b = 0.0;
    int nan_seen = 0;
    for (int ib = 0; ib < n; ib += 64) {
        const int i = ib + lane;
        const bool own = i < n;
        const float si = own ? s[i] : __int_as_float(0x7FC00000);
        const bool pos_i = own && y[i] != 0;
        const bool nan_i = own && __builtin_isnan(si);
        const unsigned long long nanmask = __ballot(nan_i);
        const int nan_before = nan_seen + __popcll(nanmask & below);
        nan_seen += __popcll(nanmask);

        int gt = 0, eq = 0, eqb = 0, gtn = 0, eqn = 0;
        for (int ch = 0; ch < n_chunks; ++ch) {
            if (ch != staged) {          // wave-uniform: only rows wider than one stage get here
                met_wave_sync();
                met_stage(s, y, n, ch * MET_STAGE, ls, ly, lane);
                met_wave_sync();
                staged = ch;
            }
            const int base = ch * MET_STAGE;
            const int len4 = (min(MET_STAGE, n - base) + 3) & ~3;
            for (int j4 = 0; j4 < len4; j4 += 4) {
                const float4 sv = *reinterpret_cast<const float4*>(ls + j4);
                const uint32_t yv = *reinterpret_cast<const uint32_t*>(ly + j4);
                const float sq[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool g = sq[q] > si, e = sq[q] == si;
                    const bool neg = ((yv >> (8 * q)) & 0xFFu) == 0u;
                    gt += g;
                    eq += e;
                    eqb += e && (base + j4 + q < i);
                    gtn += g && neg;
                    eqn += e && neg;
                }
            }
        }
        if (own) {
            if (ranks) ranks[(long)imp * max_c + i] = nan_i ? 1 + (n - n_nan) + nan_before : 1 + gt + eqb;
            if (pos_i && !nan_i) {
                twice += 2ull * (unsigned)(nneg - nan_neg - gtn - eqn) + (unsigned)eqn;
                const int rank_m = 1 + gt + (eq - 1 - eqb);
                rr += 1.0 / (double)rank_m;
                const double disc = 1.0 / log2((double)rank_m + 1.0);
                if (rank_m <= k_a) dcg_a += disc;
                if (rank_m <= k_b) dcg_b += disc;
            }
        }
    }
    if (ranks)
        for (int c = n + lane; c < max_c; c += 64) ranks[(long)imp * max_c + c] = 0;

    // ideal DCG: positives in ranks 1 .. min(n_pos, k)
    double ideal_a = 0.0, ideal_b = 0.0;
    for (int r = 1 + lane; r <= min(npos, max(k_a, k_b)); r += 64) {
        const double disc = 1.0 / log2((double)r + 1.0);
        if (r <= k_a) ideal_a += disc;
        if (r <= k_b) ideal_b += disc;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) twice += __shfl_xor(twice, o, 64);
    rr = met_wave_sum(rr);
    dcg_a = met_wave_sum(dcg_a);
    dcg_b = met_wave_sum(dcg_b);
    ideal_a = met_wave_sum(ideal_a);
    ideal_b = met_wave_sum(ideal_b);
    if (lane == 0) {
        const double qnan = __longlong_as_double(0x7FF8000000000000LL);
        if (auc) auc[imp] = (npos == 0 || nneg == 0) ? qnan : 0.5 * (double)twice / ((double)npos * (double)nneg);
        const bool undef = npos == 0 || n_nan != 0;       // the reference's 0/0, or an unorderable score
        if (mrr) mrr[imp] = undef ? qnan : rr / (double)npos;
        if (ndcg_a) ndcg_a[imp] = undef ? qnan : dcg_a / ideal_a;
        if (ndcg_b) ndcg_b[imp] = undef ? qnan : dcg_b / ideal_b;
    }
}

}  // namespace nrms

using namespace nrms;

extern "C" int nrms_impression_metrics(int32_t n_imp, int32_t max_c, const float* scores, const uint8_t* labels,
                                       const int32_t* lens, int32_t k_a, int32_t k_b, double* auc, double* mrr,
                                       double* ndcg_a, double* ndcg_b, int32_t* ranks, void* stream) {
    NRMS_REQUIRE(n_imp >= 0 && max_c > 0, "impression_metrics: bad arguments (n_imp=%d, max_c=%d)", n_imp, max_c);
    NRMS_REQUIRE(k_a >= 1 && k_b >= 1, "impression_metrics: nDCG cutoffs must be >= 1 (k_a=%d, k_b=%d)", k_a, k_b);
    if (n_imp == 0) return NRMS_OK;          // empty tensors may carry null data pointers
    NRMS_REQUIRE(scores && labels && lens, "impression_metrics: bad arguments (null input)");
    NRMS_REQUIRE(auc || mrr || ndcg_a || ndcg_b || ranks, "impression_metrics: every output is null");
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts("impression_metrics", s);
    hipLaunchKernelGGL(impression_metrics_kernel, dim3(cdiv(n_imp, MET_WAVES)), dim3(64 * MET_WAVES), 0, s, n_imp, max_c,
                       scores, labels, lens, k_a, k_b, auc, mrr, ndcg_a, ndcg_b, ranks);
    return check_launch("impression_metrics");
}
