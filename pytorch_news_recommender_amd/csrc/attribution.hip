// Why a news item was recommended: its score split exactly over the clicks of the history (include/nrms_hip.h:
// nrms_attribution_dot, whose header comment states the contract: the term, the total, the reasons, the unnamed share, invalid
// entries).
//
// The user vector of an NRMS-style user encoder is the additive-attention sum u[b] = sum_h w[b, h] ctx[b, h, :], so
// u[b] . x = sum_h w[b, h] (ctx[b, h, :] . x): term h is what click h contributes to the score of item x.
//
// One kernel (attribution_kernel), one wave per (user, 64 positions of the user's list):
// 1. The score chain over the GATHERED catalogue rows the 64 positions name (rank_entries_kernel's form of tk_chain), with the
//    32 ctx rows of one half of the history as the A operand; histories longer than 32 slots take a second pass.  The 32 x 32
//    MFMA tile scores every gathered row against every slot of the half, and here all of them are wanted.
// 2. Each finished accumulator is multiplied by its slot's w (one fp32 multiply) and goes to a 64 x 64 block of terms in LDS,
//    item-major with a pitch of 65 floats: the accumulator's lanes are items, so a store's 32 items land on 32 different banks
//    (the two half-waves, 4 slots apart, overlap two-way), and in step 3 lane i walks row i, bank (i + h) mod 64: conflict-free.
// 3. Lane i owns list position j0 + i: one sequential pass over the H terms forms the ordered sum, the sum over the unnamed
//    slots and, by insertion into 8 registers of tk_entry(c, slot), the m largest terms.
// 4. The chunk's contrib rows are one contiguous stretch of [K, H]: the wave writes it with coalesced stores from LDS.
// No workspace is used: the terms of a chunk never leave LDS.
#include "topk_entry.h"

namespace nrms {

constexpr int AT_MAX_H = 64;
constexpr int AT_MAX_K = 256;
constexpr int AT_MAX_M = 8;
constexpr int AT_IT = 64;                      // list positions per wave (TK_TN column tiles of 32)
constexpr int AT_TP = 65;                      // LDS pitch (floats) of an item's row of terms

// Block (x, y): user x, list positions 64 y .. + 63.  items is not read when N == 0.
template <bool VEC>
__global__ __launch_bounds__(64) void attribution_kernel(int H, long N, int d, int K, int m, const float* __restrict__ ctx,
                                                         const float* __restrict__ w, const float* __restrict__ items,
                                                         const int64_t* __restrict__ ids,
                                                         const uint8_t* __restrict__ slot_named, float* __restrict__ contrib,
                                                         float* __restrict__ total, int32_t* __restrict__ top_slots,
                                                         float* __restrict__ top_contrib, float* __restrict__ unnamed_share) {
    __shared__ int rows[AT_IT];
    __shared__ uint8_t named[AT_MAX_H];
    __shared__ __attribute__((aligned(16))) float stage[64 * TK_BP];
    __shared__ float terms[AT_IT * AT_TP];
    const int lane = threadIdx.x;
    const int r = lane & 31, h = lane >> 5;
    const long b = blockIdx.x;
    const int j0 = AT_IT * blockIdx.y;
    const int n_pos = min(AT_IT, K - j0);          // >= 1: the grid has ceil(K / 64) chunks
    const float inf = __builtin_huge_valf();

    // this lane's own list position: the id it names, and the row the wave reads for it (row 0 for an id that names none)
    const int64_t id = lane < n_pos ? ids[b * K + j0 + lane] : -1;
    const bool valid = id >= 0 && id < N;
    rows[lane] = valid ? (int)id : 0;
    if (lane < H) named[lane] = slot_named ? slot_named[b * H + lane] : 1;
    tk_wave_sync();

    if (__ballot(valid) != 0) {                    // wave-uniform; some position names a row, so N >= 1
        for (int half = 0; 32 * half < H; ++half) {
            const float* arow[1] = {ctx + (b * H + min(32 * half + r, H - 1)) * d};
            float wq[16];                          // w of the 16 slots this lane's accumulator registers hold
#pragma unroll
            for (int q = 0; q < 16; ++q) wq[q] = w[b * H + min(32 * half + (q & 3) + 8 * (q >> 2) + 4 * h, H - 1)];
            tk_f32x16 acc[TK_TN];
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
            tk_chain<VEC>(acc, arow, items, d, stage, lane, [&](int i) { return rows[i]; });
            // C/D layout: item = lane & 31 of the column tile, slot = (q & 3) + 8 (q >> 2) + 4 (lane >> 5) of the half
#pragma unroll
            for (int c = 0; c < TK_TN; ++c)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int slot = 32 * half + (q & 3) + 8 * (q >> 2) + 4 * h;
                    if (slot < H) terms[(32 * c + r) * AT_TP + slot] = __fmul_rn(wq[q], acc[c][q]);
                }
        }
    }
    tk_wave_sync();
    if (!valid)                                    // (also every row when the chain did not run): a row of zeros
        for (int s = 0; s < H; ++s) terms[lane * AT_TP + s] = 0.0f;

    if (lane < n_pos) {
        float sum = 0.0f, un = 0.0f;
        uint64_t best[AT_MAX_M] = {};              // descending; 0 = nothing
        if (valid) {
            for (int s = 0; s < H; ++s) {
                const float c = terms[lane * AT_TP + s];
                const bool nm = named[s] != 0;
                sum = __fadd_rn(sum, c);
                if (!nm) un = __fadd_rn(un, c);
                uint64_t e = (nm && !__builtin_isnan(c)) ? tk_entry(c, (uint32_t)s) : 0;
#pragma unroll
                for (int p = 0; p < AT_MAX_M; ++p) {
                    const uint64_t hi = e > best[p] ? e : best[p];
                    e = e > best[p] ? best[p] : e;
                    best[p] = hi;
                }
            }
        }
        const long o = b * K + j0 + lane;
        total[o] = valid ? sum : -inf;
        if (unnamed_share) unnamed_share[o] = un;
#pragma unroll
        for (int p = 0; p < AT_MAX_M; ++p) {
            if (p < m) {
                top_slots[o * m + p] = best[p] ? (int32_t)tk_entry_id(best[p]) : -1;
                top_contrib[o * m + p] = best[p] ? tk_entry_score(best[p]) : -inf;
            }
        }
    }
    if (contrib) {
        tk_wave_sync();
        float* out = contrib + (b * K + j0) * H;   // rows j0 .. j0 + n_pos - 1 of [K, H]: contiguous
        for (int e = lane; e < n_pos * H; e += 64) out[e] = terms[(e / H) * AT_TP + (e % H)];
    }
}

static bool attribution_args_ok(int32_t B, int32_t H, int32_t d, int32_t K, int32_t m) {
    return B >= 0 && H >= 1 && H <= AT_MAX_H && d >= 1 && K >= 1 && K <= AT_MAX_K && m >= 1 && m <= AT_MAX_M;
}

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_attribution_dot_workspace_bytes(int32_t B, int32_t H, int32_t d, int32_t K, int32_t m) {
    if (!attribution_args_ok(B, H, d, K, m)) return 0;
    return 256;        // reserved: a chunk's terms stay in LDS and the call touches no workspace today; never 0 for accepted arguments
}

extern "C" int nrms_attribution_dot(int32_t B, int32_t H, int64_t N, int32_t d, int32_t K, int32_t m, const float* ctx,
                                    const float* w, const float* items, const int64_t* ids, const uint8_t* slot_named,
                                    float* contrib, float* total, int32_t* top_slots, float* top_contrib, float* unnamed_share,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "attribution_dot";
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "K", K, AT_MAX_K, 0);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE(H >= 1 && H <= AT_MAX_H, "%s: H must be in [1, %d] (H=%d)", who, AT_MAX_H, H);
    NRMS_REQUIRE(m >= 1 && m <= AT_MAX_M, "%s: m must be in [1, %d] (m=%d)", who, AT_MAX_M, m);
    if (B == 0) return NRMS_OK;
    rc = tk_check_ptrs(who, {{"ctx", ctx, true, 4}, {"w", w, true, 4}, {"items", items, N != 0, 4}, {"ids", ids, true, 8},
                             {"slot_named", slot_named, false, 1}, {"contrib", contrib, false, 4}, {"total", total, true, 4},
                             {"top_slots", top_slots, true, 4}, {"top_contrib", top_contrib, true, 4},
                             {"unnamed_share", unnamed_share, false, 4}},
                       workspace, workspace_bytes, nrms_attribution_dot_workspace_bytes(B, H, d, K, m), 8);
    if (rc != NRMS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    const dim3 grid(B, cdiv(K, AT_IT));
    tk_with_flags([&](auto V) {
        hipLaunchKernelGGL((attribution_kernel<decltype(V)::value>), grid, dim3(64), 0, s, H, (long)N, d, K, m, ctx, w, items, ids,
                           slot_named, contrib, total, top_slots, top_contrib, unnamed_share);
    }, tk_vec_ok(d, ctx, items));
    return check_launch(who);
}
