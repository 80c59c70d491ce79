// Per-epoch negatives for a click log that records no impressions (include/nrms_hip.h, "Click log"; data_handler.py ClickFeed).
// Every training row -- one click -- takes S negatives from the whole catalogue, drawn by integer weights (a smoothed popularity)
// through their running sum `cum`, never a news of the user's own set, never the same news twice in a row: a pure integer
// function of (row_key, row_user, row_pos, sets, cum, S, seed), so a feed redraws it at the start of every epoch without leaving
// the device and the result depends on neither the batch, the rank nor the launch.
//
//   cat_neg_kernel: a row occupies a SEGMENT of P = next power of two >= S lanes, 64 / P rows per wavefront, four wavefronts per
//       workgroup.  Lane s of a segment owns slot s: it computes the slot's attempts -- one Philox call per two attempts, an
//       upper-bound search of the draw in cum (17 steps at 130 000 news, the 1 MB of cum L2-resident), a binary search of the drawn
//       id in the user's sorted set -- into eight registers c0 .. c7 indexed by unrolled loops only (an array indexed by a lane's
//       own attempt number would live in scratch: DESIGN.md section 3c), with a bit per attempt in `dead` for "is 0 / is the
//       user's own / not computed yet".  The slots are then resolved in S steps: at step t every lane forms its first live
//       attempt, lane t's is broadcast over the segment (__shfl of width P) and becomes slot t's value, and the lanes above t kill
//       their attempts equal to it.  Attempts 2 .. 7 are LAZY: the wave starts with two, and while any of its lanes reaches its
//       step with every computed attempt dead (__any: wave-uniform) all lanes compute the next two and the resolution is redone
//       from the per-attempt bits -- at most three times, and at S = 4 under a smoothed popularity once per some thirty waves.  A
//       slot whose first live attempt lies among the computed ones has the value it would have with all eight, so the laziness
//       shows in no byte.  The pack is a __ballot of the valued lanes shifted to the segment and two popcounts.  No LDS, no
//       barrier; every byte of cand and clen has one writer and is a plain vector store; one atomicAdd per wave and counter.
#include "common.h"

namespace nrms {

constexpr int CN_BLOCK = 256;
constexpr int CN_WAVES = CN_BLOCK / WAVE;
constexpr int CN_ATTEMPTS = 8;
constexpr size_t CN_WORKSPACE = 256;              // reserved: the call reads and writes none of it today

struct CatNegArgs {
    long n_rows;
    const int64_t* row_key; const int32_t* row_user; const int32_t* row_pos;
    long n_users;
    const int64_t* set_ptr; const int32_t* set_news;
    long n_news;
    const int64_t* cum;
    int S, P;
    uint64_t seed;
    int64_t* cand; int64_t* clen;
    int* n_short; int* n_bad;
};

// ---- the per-row logic, the same source on the host (a stand-alone program may include this file's functions) and the device ----
__host__ __device__ __forceinline__ uint64_t catneg_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the id n with cum[n] <= x < cum[n + 1], for x < cum[n_news]: an id of weight 0 is never returned, whatever ties cum holds
__host__ __device__ __forceinline__ int32_t catneg_search(const int64_t* __restrict__ cum, long n_news, uint64_t x) {
    long lo = 0, hi = n_news;                                      // cum[lo] <= x < cum[hi]
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if ((uint64_t)cum[mid] <= x) lo = mid; else hi = mid;
    }
    return (int32_t)lo;
}

// is id among set[b .. e) (ascending, distinct)
__host__ __device__ __forceinline__ bool catneg_member(const int32_t* __restrict__ set, int64_t b, int64_t e, int32_t id) {
    while (b < e) {
        const int64_t mid = (b + e) >> 1;
        const int32_t v = set[mid];
        if (v == id) return true;
        if (v < id) b = mid + 1; else e = mid;
    }
    return false;
}

// attempts 2 h and 2 h + 1 of slot s of the row with key k: the two drawn ids, and bit j set where attempt 2 h + j may not be used
// (id 0, or one of the user's own)
__host__ __device__ __forceinline__ uint32_t catneg_attempt_pair(const int64_t* __restrict__ cum, long n_news, uint64_t W, uint64_t seed, uint64_t k,
                                                                 int s, int h, const int32_t* __restrict__ set, int64_t b, int64_t e, int32_t& n0,
                                                                 int32_t& n1) {
    uint32_t r[4];
    philox4x32_7(seed, (((k * 64u + (uint64_t)s) << 2) | (uint64_t)h), PHILOX_SITE_CATALOGUE_NEG, r);
    n0 = catneg_search(cum, n_news, catneg_mulhi(((uint64_t)r[0] << 32) | r[1], W));
    n1 = catneg_search(cum, n_news, catneg_mulhi(((uint64_t)r[2] << 32) | r[3], W));
    return ((n0 == 0 || catneg_member(set, b, e, n0)) ? 1u : 0u) | ((n1 == 0 || catneg_member(set, b, e, n1)) ? 2u : 0u);
}

__host__ __device__ __forceinline__ bool catneg_row_ok(long n_users, long n_news, int32_t user, int32_t pos) {
    return user >= 0 && user < n_users && pos > 0 && pos < n_news;
}

__global__ __launch_bounds__(CN_BLOCK) void cat_neg_kernel(CatNegArgs a) {
    const int lane = threadIdx.x & 63;
    const int P = a.P, S = a.S;
    const int s = lane & (P - 1), seg0 = lane & ~(P - 1);
    const long wave = (long)blockIdx.x * CN_WAVES + (threadIdx.x >> 6);
    const long row = wave * (WAVE / P) + lane / P;
    if (wave * (WAVE / P) >= a.n_rows) return;                     // (wave-uniform)
    const bool in = row < a.n_rows && s < S;                       // this lane owns a slot of a row
    const uint64_t W = (uint64_t)a.cum[a.n_news];
    uint64_t key = 0;
    int32_t user = 0, pos = 0;
    if (in) {
        key = (uint64_t)a.row_key[row];
        user = a.row_user[row];
        pos = a.row_pos[row];
    }
    const bool ok = in && catneg_row_ok(a.n_users, a.n_news, user, pos);
    int64_t b = 0, e = 0;
    if (ok) {
        b = a.set_ptr[user];
        e = a.set_ptr[user + 1];
        if (b < 0 || e < b || e > a.set_ptr[a.n_users]) b = e = 0; // (a damaged set_ptr: nothing is read outside set_news)
    }
    int32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0;
    uint32_t base_dead = 0xFFu;                                    // bit j: attempt j is 0, the user's own, or not computed yet
    if (ok) base_dead = 0xFCu | catneg_attempt_pair(a.cum, a.n_news, W, a.seed, key, s, 0, a.set_news, b, e, c0, c1);
    int32_t val = -1;
    for (int computed = 2;; computed += 2) {
        // ---- resolve the slots in order
        uint32_t dead = base_dead;
        bool starved = false;
        val = -1;
        for (int t = 0; t < S; ++t) {
            const uint32_t live = ~dead & 0xFFu;
            int32_t mine = -1;
            if (live) {
                const int f = __ffs((int)live) - 1;
                mine = f == 0 ? c0 : f == 1 ? c1 : f == 2 ? c2 : f == 3 ? c3 : f == 4 ? c4 : f == 5 ? c5 : f == 6 ? c6 : c7;
            }
            const int32_t v = __shfl(mine, t, P);                  // lane t of every segment
            if (s == t) {
                val = v;
                starved = ok && v < 0;
            } else if (s > t && v >= 0) {
                dead |= (c0 == v ? 1u : 0u) | (c1 == v ? 2u : 0u) | (c2 == v ? 4u : 0u) | (c3 == v ? 8u : 0u) | (c4 == v ? 16u : 0u) |
                        (c5 == v ? 32u : 0u) | (c6 == v ? 64u : 0u) | (c7 == v ? 128u : 0u);
            }
        }
        if (computed >= CN_ATTEMPTS || !__any(starved)) break;     // (wave-uniform)
        // ---- some slot ran out of attempts: two more for every slot of the wave
        if (ok) {
            int32_t n0, n1;
            const uint32_t d = catneg_attempt_pair(a.cum, a.n_news, W, a.seed, key, s, computed >> 1, a.set_news, b, e, n0, n1);
            if (computed == 2) { c2 = n0; c3 = n1; }
            else if (computed == 4) { c4 = n0; c5 = n1; }
            else { c6 = n0; c7 = n1; }
            base_dead = (base_dead & ~(3u << computed)) | (d << computed);
        }
    }
    // ---- pack: the valued slots in slot order, zeros behind them
    const bool valued = ok && val >= 0;
    const unsigned long long vm = __ballot(valued);
    const unsigned long long seg = P == 64 ? vm : (vm >> seg0) & ((1ull << P) - 1ull);
    const int count = __popcll(seg), before = __popcll(seg & ((1ull << s) - 1ull));
    if (in) {
        int64_t* out = a.cand + row * (S + 1);
        if (valued) out[1 + before] = val;
        if (s >= count) out[1 + s] = 0;                            // slots count .. S - 1: the lanes count .. S - 1, one each
        if (s == 0) {
            out[0] = ok ? pos : 0;
            a.clen[row] = 1 + count;
        }
    }
    const int n_short = __popcll(__ballot(ok && val < 0)), n_bad = __popcll(__ballot(in && !ok && s == 0));
    if (lane == 0 && n_short) atomicAdd(a.n_short, n_short);
    if (lane == 0 && n_bad) atomicAdd(a.n_bad, n_bad);
}

}  // namespace nrms

using namespace nrms;

static bool catneg_shape_ok(int64_t n_rows, int64_t n_news, int32_t S) {
    return n_rows >= 0 && n_rows < (1L << 31) && n_news >= 2 && n_news < (1L << 31) && S >= 1 && S <= 64;
}

extern "C" size_t nrms_catalogue_negative_sample_workspace_bytes(int64_t n_rows, int64_t n_news, int32_t S) {
    if (!catneg_shape_ok(n_rows, n_news, S)) {
        set_error("catalogue_negative_sample_workspace_bytes: n_rows=%ld n_news=%ld S=%d (n_rows in [0, 2^31), n_news in [2, 2^31), S in [1, 64])",
                  (long)n_rows, (long)n_news, S);
        return 0;
    }
    return CN_WORKSPACE;
}

extern "C" int nrms_catalogue_negative_sample(int64_t n_rows, const int64_t* row_key, const int32_t* row_user, const int32_t* row_pos, int64_t n_users,
                                              const int64_t* set_ptr, const int32_t* set_news, int64_t n_news, const int64_t* cum, int32_t S,
                                              uint64_t seed, int64_t* cand, int64_t* clen, int32_t* n_short, int32_t* n_bad, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    NRMS_REQUIRE(catneg_shape_ok(n_rows, n_news, S),
                 "catalogue_negative_sample: n_rows=%ld n_news=%ld S=%d (n_rows in [0, 2^31), n_news in [2, 2^31), S in [1, 64])", (long)n_rows,
                 (long)n_news, S);
    NRMS_REQUIRE(n_users >= 0 && n_users < (1L << 31), "catalogue_negative_sample: n_users=%ld (must be in [0, 2^31))", (long)n_users);
    NRMS_REQUIRE(row_key && row_user && row_pos && set_ptr && set_news && cum && cand && clen && n_short && n_bad,
                 "catalogue_negative_sample: null argument");
    NRMS_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 3) == 0, "catalogue_negative_sample: workspace must be 4-byte aligned and not null");
    if (workspace_bytes < CN_WORKSPACE) {
        set_error("catalogue_negative_sample: workspace %zu < required %zu bytes", workspace_bytes, CN_WORKSPACE);
        return NRMS_EWORKSPACE;
    }
    if (n_rows == 0) return NRMS_OK;
    int P = 1;
    while (P < S) P <<= 1;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts("catalogue_negative_sample", s);
    CatNegArgs a{(long)n_rows, row_key, row_user, row_pos, (long)n_users, set_ptr, set_news, (long)n_news, cum, (int)S, P, seed, cand, clen, n_short, n_bad};
    const long rows_per_block = (long)CN_WAVES * (WAVE / P);
    hipLaunchKernelGGL(cat_neg_kernel, dim3(cdiv(n_rows, rows_per_block)), dim3(CN_BLOCK), 0, s, a);
    return check_launch("catalogue_negative_sample");
}
