// Per-epoch negative sampling from an impression log resident in HBM (include/nrms_hip.h, "Impression log"; data_handler.py
// ImpressionFeed).  The reference shuffles an impression's non-clicked news ONCE, offline, and gives the p-th clicked item the
// slice [p S, (p + 1) S) of that shuffle (MIND_2020/data_processor.py:519-528); here the shuffle is a ranking by Philox keys, a
// pure function of (log, S, seed), so a feed redraws it at the start of every epoch without leaving the device.
//
//   neg_sample_wave_kernel: one wave per impression of at most 64 shown items (MIND: tens, mean 37), four impressions per
//       workgroup.  Lane j holds entry j: its Philox word (issued as soon as the impression's first position is known, in
//       front of the loads of the id and the label, which it does not depend on), its label's bit in a __ballot mask -- the
//       popcount below a lane is a positive's number p, the popcount of the whole mask the number of rows -- and its rank,
//       counted against the other negatives' words read lane by lane (v_readlane: the loop walks the set bits of the wave-uniform
//       negatives mask, so it costs one compare per NEGATIVE, not per lane).  No LDS, no barrier.
//   neg_sample_block_kernel: one workgroup per longer impression (65 .. max_shown <= 2048), the negatives' keys
//       (word << 32 | position) and ids compacted into LDS by per-wave __ballot prefixes, ranks by counting against the LDS copy
//       (every lane reads the same address: a broadcast).  At n <= 2048 that is n / 256 keys per lane times n compares; a
//       workgroup-wide bitonic sort of 2048 keys is 66 barrier-separated stages and would order ranks nobody reads: only the
//       ranks below n_pos * S are stored.  It also writes the rows of an impression above max_shown (positives only, counted
//       into *n_bad), whatever its length.
//
// The wave kernel appends the impressions it leaves to the block kernel to a list in the caller's workspace (one integer
// atomicAdd on the list's length per such impression: the list's ORDER varies from run to run, the bytes of cand and clen do
// not -- every row has one writer and every value is a plain vector store).  The block kernel is a fixed grid that strides over
// the list, so the host never learns the list's length.
#include "common.h"

namespace nrms {

constexpr int NS_BLOCK = 256;
constexpr int NS_WAVES = NS_BLOCK / WAVE;
constexpr int NS_MAX_SHOWN = 2048;
constexpr int NS_LONG_GRID = 1024;
constexpr size_t NS_LIST_OFFSET = 256;            // workspace: int32 list length at 0, the list from here

struct NegArgs {
    long n_imp;
    const int64_t* imp_ptr; const int32_t* shown; const uint8_t* label; const int64_t* sample_ptr;
    int S, max_shown;
    uint64_t seed;
    int64_t* cand; int64_t* clen;
    int* n_bad;
};

// word e & 3 of the call of group e >> 2 (selects, not an indexed array: no scratch)
__device__ __forceinline__ uint32_t neg_word(uint64_t seed, uint64_t e) {
    uint32_t r[4];
    philox4x32_7(seed, e >> 2, PHILOX_SITE_NEG_SAMPLE, r);
    const uint32_t lo = (e & 1) ? r[1] : r[0], hi = (e & 1) ? r[3] : r[2];
    return (e & 2) ? hi : lo;
}

// what an impression may index: its entries inside the log, its rows inside cand
__device__ __forceinline__ bool neg_extent_ok(const NegArgs& a, long i, int64_t& p0, int64_t& n, int64_t& row0, int64_t& n_rows) {
    p0 = a.imp_ptr[i];
    const int64_t p1 = a.imp_ptr[i + 1], nnz = a.imp_ptr[a.n_imp];
    row0 = a.sample_ptr[i];
    const int64_t row1 = a.sample_ptr[i + 1], n_samples = a.sample_ptr[a.n_imp];
    n = p1 - p0;
    n_rows = row1 - row0;
    return p0 >= 0 && p1 >= p0 && p1 <= nnz && row0 >= 0 && row1 >= row0 && row1 <= n_samples;
}

// row of positive p: its id, its length, zeros behind the negatives it will be given
__device__ __forceinline__ void neg_store_positive(const NegArgs& a, int64_t row, int32_t id, int64_t p, int64_t n_neg) {
    int64_t cnt = n_neg - p * a.S;
    cnt = cnt < 0 ? 0 : (cnt > a.S ? a.S : cnt);
    int64_t* out = a.cand + row * (a.S + 1);
    out[0] = id;
    for (int k = (int)cnt; k < a.S; ++k) out[1 + k] = 0;
    a.clen[row] = 1 + cnt;
}

__global__ __launch_bounds__(NS_BLOCK) void neg_sample_wave_kernel(NegArgs a, int* __restrict__ n_long, int32_t* __restrict__ long_list) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * NS_WAVES + (threadIdx.x >> 6);
    if (i >= a.n_imp) return;                                      // (wave-uniform)
    int64_t p0, n, row0, n_rows;
    if (!neg_extent_ok(a, i, p0, n, row0, n_rows)) {
        if (lane == 0) atomicAdd(a.n_bad, 1);
        return;
    }
    if (n > WAVE || n > a.max_shown) {
        if (lane == 0) long_list[atomicAdd(n_long, 1)] = (int32_t)i;
        return;
    }
    const bool in = lane < n;
    const uint64_t e = (uint64_t)(p0 + (in ? lane : 0));
    const uint32_t w = neg_word(a.seed, e);
    const int32_t id = in ? a.shown[e] : 0;
    const bool pos = in && a.label[e] != 0;
    const unsigned long long pos_mask = __ballot(pos), neg_mask = __ballot(in && !pos);
    const int n_pos = __popcll(pos_mask), n_neg = __popcll(neg_mask);
    if (n_pos != n_rows) {                                         // sample_ptr is not the scan of this log's positives
        if (lane == 0) atomicAdd(a.n_bad, 1);
        return;
    }
    if (n_pos == 0) return;
    if (pos) neg_store_positive(a, row0 + __popcll(pos_mask & ((1ull << lane) - 1ull)), id, __popcll(pos_mask & ((1ull << lane) - 1ull)), n_neg);
    int r = 0;
    for (unsigned long long m = neg_mask; m != 0ull; m &= m - 1ull) {
        const int k = __ffsll((long long)m) - 1;                   // wave-uniform: v_readlane
        const uint32_t wk = (uint32_t)__builtin_amdgcn_readlane((int)w, k);
        r += (wk < w || (wk == w && k < lane)) ? 1 : 0;
    }
    if (in && !pos) {
        const int p = r / a.S;
        if (p < n_pos) a.cand[(row0 + p) * (a.S + 1) + 1 + (r - p * a.S)] = id;
    }
}

__global__ __launch_bounds__(NS_BLOCK) void neg_sample_block_kernel(NegArgs a, const int* __restrict__ n_long, const int32_t* __restrict__ long_list) {
    __shared__ uint64_t key[NS_MAX_SHOWN];
    __shared__ int32_t nid[NS_MAX_SHOWN];
    __shared__ int wave_pos[NS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = *n_long;
    for (int item = blockIdx.x; item < count; item += gridDim.x) {
        const long i = long_list[item];
        int64_t p0, n, row0, n_rows;
        if (i < 0 || i >= a.n_imp || !neg_extent_ok(a, i, p0, n, row0, n_rows)) continue;     // (the wave kernel listed valid ones only)
        const bool too_long = n > a.max_shown;
        // how many positives: the rows this impression owns
        int mine = 0;
        for (int64_t j = tid; j < n; j += NS_BLOCK) mine += a.label[p0 + j] != 0 ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
        __syncthreads();                                           // the previous item's readers of key / nid / wave_pos are done
        if (lane == 0) wave_pos[wave] = mine;
        __syncthreads();
        int64_t n_pos = 0;
#pragma unroll
        for (int v = 0; v < NS_WAVES; ++v) n_pos += wave_pos[v];
        if (n_pos != n_rows || too_long) {
            if (tid == 0) atomicAdd(a.n_bad, 1);
            if (n_pos != n_rows) continue;
        }
        const int64_t n_neg = too_long ? 0 : n - n_pos;            // above max_shown: positives only, every clen 1
        // positives -> slot 0 of their rows; negatives -> key and id at their ordinal in LDS.  A chunk of 256 entries at a time,
        // the positives in front of it carried in `before`.
        int64_t before = 0;
        for (int64_t c0 = 0; c0 < n; c0 += NS_BLOCK) {
            const int64_t j = c0 + tid;
            const bool in = j < n;
            const uint64_t e = (uint64_t)(p0 + (in ? j : 0));
            const uint32_t w = too_long ? 0u : neg_word(a.seed, e);
            const bool pos = in && a.label[e] != 0;
            const int32_t id = in ? a.shown[e] : 0;
            const unsigned long long pm = __ballot(pos);
            __syncthreads();                                       // wave_pos: the previous chunk's readers are done
            if (lane == 0) wave_pos[wave] = __popcll(pm);
            __syncthreads();
            int64_t p = before + __popcll(pm & ((1ull << lane) - 1ull));
            int chunk = 0;
#pragma unroll
            for (int v = 0; v < NS_WAVES; ++v) {
                p += v < wave ? wave_pos[v] : 0;
                chunk += wave_pos[v];
            }
            before += chunk;
            if (pos) neg_store_positive(a, row0 + p, id, p, n_neg);
            else if (in && !too_long) {
                key[j - p] = ((uint64_t)w << 32) | (uint64_t)j;    // j < 2048: (word, position) in one compare
                nid[j - p] = id;
            }
        }
        if (too_long) continue;
        __syncthreads();
        for (int q = tid; q < n_neg; q += NS_BLOCK) {
            const uint64_t my = key[q];
            int r = 0;
            for (int t = 0; t < (int)n_neg; ++t) r += key[t] < my ? 1 : 0;
            const int p = r / a.S;
            if (p < n_pos) a.cand[(row0 + p) * (a.S + 1) + 1 + (r - p * a.S)] = nid[q];
        }
    }
}

}  // namespace nrms

using namespace nrms;

static bool neg_shape_ok(int64_t n_imp, int32_t S) { return n_imp >= 0 && n_imp < (1L << 31) && S >= 1 && S <= 64; }
static size_t neg_workspace(int64_t n_imp) { return NS_LIST_OFFSET + (((size_t)n_imp * sizeof(int32_t) + 255) & ~(size_t)255); }

extern "C" size_t nrms_negative_sample_workspace_bytes(int64_t n_imp, int64_t nnz, int32_t S) {
    if (!neg_shape_ok(n_imp, S) || nnz < 0) {
        set_error("negative_sample_workspace_bytes: n_imp=%ld nnz=%ld S=%d (n_imp in [0, 2^31), nnz >= 0, S in [1, 64])", (long)n_imp, (long)nnz, S);
        return 0;
    }
    return neg_workspace(n_imp);                 // the list of impressions the one-wave path leaves to the workgroup path
}

extern "C" int nrms_negative_sample(int64_t n_imp, const int64_t* imp_ptr, const int32_t* shown, const uint8_t* label, const int64_t* sample_ptr,
                                    int32_t S, int32_t max_shown, uint64_t seed, int64_t* cand, int64_t* clen, int32_t* n_bad, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    NRMS_REQUIRE(neg_shape_ok(n_imp, S), "negative_sample: n_imp=%ld S=%d (n_imp in [0, 2^31), S in [1, 64])", (long)n_imp, S);
    NRMS_REQUIRE(max_shown >= 1 && max_shown <= NS_MAX_SHOWN, "negative_sample: max_shown=%d (must be in [1, %d])", max_shown, NS_MAX_SHOWN);
    NRMS_REQUIRE(imp_ptr && shown && label && sample_ptr && cand && clen && n_bad, "negative_sample: null argument");
    NRMS_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 3) == 0, "negative_sample: workspace must be 4-byte aligned and not null");
    const size_t need = neg_workspace(n_imp);
    if (workspace_bytes < need) {
        set_error("negative_sample: workspace %zu < required %zu bytes", workspace_bytes, need);
        return NRMS_EWORKSPACE;
    }
    if (n_imp == 0) return NRMS_OK;
    int* n_long = (int*)workspace;
    int32_t* long_list = (int32_t*)((char*)workspace + NS_LIST_OFFSET);
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts("negative_sample", s);
    if (hipMemsetAsync(n_long, 0, sizeof(int), s) != hipSuccess) {
        set_error("negative_sample: hipMemsetAsync failed");
        return NRMS_ELAUNCH;
    }
    NegArgs a{(long)n_imp, imp_ptr, shown, label, sample_ptr, (int)S, (int)max_shown, seed, cand, clen, n_bad};
    hipLaunchKernelGGL(neg_sample_wave_kernel, dim3(cdiv(n_imp, NS_WAVES)), dim3(NS_BLOCK), 0, s, a, n_long, long_list);
    hipLaunchKernelGGL(neg_sample_block_kernel, dim3(n_imp < NS_LONG_GRID ? (int)n_imp : NS_LONG_GRID), dim3(NS_BLOCK), 0, s, a, (const int*)n_long,
                       (const int32_t*)long_list);
    return check_launch("negative_sample");
}
