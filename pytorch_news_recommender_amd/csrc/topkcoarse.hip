// The exact top-k through an fp16 shortlist with a certificate (include/nrms_hip.h: nrms_catalogue_pack_f16 and
// nrms_topk_dot_coarse, whose header comment states the contract and the bound).
//
// nrms_catalogue_pack_f16 (coarse_pack_kernel): one wave per catalogue row writes the row's fp16 copy (h(x), zero-padded to the
// pitch) and forms ||row||^2 and ||row - h(row)||^2 in fp64; the maxima over the rows go to stats with an integer atomic max
// on the bits of the rounded-up fp32 norms (non-negative floats order as their bits), so the result has no order.
//
// nrms_topk_dot_coarse, four stages on one stream:
// (a) coarse_user_kernel: one wave per user, u16 = h(user[b]) into the workspace and the three norms in fp64.
// (b) coarse_slice_kernel: the grid, the 32-user tiles, the slices and the TkFilter of topk_slice_kernel with list length M.  The
//     score is one fp32 accumulator per (user, item) on v_mfma_f32_32x32x16_f16 over the whole pitch, no split-K: superblock sb of
//     64 halves is four MFMAs, lane (r, h) feeding halves 64 sb + 32 h + 8 s + j (s = 0..3; j = 0..7) of user r as A and of item r
//     as B.  The k order inside an instruction is the hardware's; it is the same for every pair, so the coarse bits of a (user row,
//     item row) do not depend on B, N, M, the row's position, the exclude list or the run.  Operands come straight from global
//     memory as four 16-byte loads per row and superblock (64 contiguous bytes per lane; the rows of the pitch are 64-byte aligned),
//     the next superblock loaded while this one's MFMAs run.  8 waves per block at every M.
// (c) topk_merge_kernel at k = M: the shortlist, sorted by (coarse score desc, id asc).
// (d) coarse_rescore_kernel: the rank_entries_kernel pattern, tk_chain over the gathered fp32 rows the shortlist names, with the
//     user's own row among the tile's 32 A rows: nrms_topk_dot's bits for that (user row, item row).  coarse_finish_kernel: one
//     wave per user sorts the exact entries, writes the first min(k, L) and evaluates the certificate in fp64, every product and
//     sum rounded up.
#include "topk_kernels.h"

namespace nrms {

constexpr int TC_MAX_M = 256;

typedef _Float16 tc_f16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ __forceinline__ int tc_pitch(int d) { return 32 * ((d + 31) / 32); }

// h(x): |x| > 65504 becomes +-65504, |x| < 2^-14 becomes 0 (sign kept), then round to nearest even.  No subnormal and no
// infinity is ever formed, so the conversion's denormal mode cannot matter.  x finite.
__device__ __forceinline__ _Float16 tc_h(float x) {
    const float a = __builtin_fabsf(x);
    float y = x;
    if (a > 65504.0f) y = __builtin_copysignf(65504.0f, x);
    if (a < 0x1p-14f) y = __builtin_copysignf(0.0f, x);
    return (_Float16)y;
}

__device__ __forceinline__ bool tc_finite(float x) { return __builtin_fabsf(x) <= 3.4028234663852886e38f; }

// the next double towards +inf (x not NaN; +inf stays)
__device__ __forceinline__ double tc_up(double x) {
    if (x == 0.0) return __longlong_as_double(1LL);
    long long b = __double_as_longlong(x);
    if (b == 0x7FF0000000000000LL) return x;
    return __longlong_as_double(x > 0.0 ? b + 1 : b - 1);
}
__device__ __forceinline__ double tc_mul_up(double a, double b) { return tc_up(a * b); }
__device__ __forceinline__ double tc_add_up(double a, double b) { return tc_up(a + b); }

// >= sqrt(the exact sum) of n non-negative terms that were each rounded once and added to nearest in any order
// (a sum of 0 is exact: the squares of fp32 values do not underflow in fp64)
__device__ __forceinline__ double tc_norm_up(double sum, int n) {
    if (sum == 0.0) return 0.0;
    const double s = tc_up(sum * (1.0 + (double)(n + 64) * 0x1p-51));
    return tc_up(tc_up(__builtin_sqrt(s)));
}

// the smallest fp32 >= x (x >= 0)
__device__ __forceinline__ float tc_f32_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

__device__ __forceinline__ double tc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave: the fp16 copy of row src[0, d) at dst[0, pitch) and the row's sums; returns false (dst all zero) for a row that
// holds a NaN or an infinity.  nn = sum x^2, n16 = sum h(x)^2, ee = sum (x - h(x))^2, each the same in every lane.
__device__ __forceinline__ bool tc_pack_row(const float* __restrict__ src, uint16_t* __restrict__ dst, int d, int pitch, int lane,
                                            double& nn, double& n16, double& ee) {
    bool bad = false;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int k = lane; k < d; k += 64) {
        const float x = src[k];
        if (!tc_finite(x)) {
            bad = true;
            continue;
        }
        const double xd = (double)x, hd = (double)(float)tc_h(x);
        a += xd * xd;
        b += hd * hd;
        c += (xd - hd) * (xd - hd);
    }
    bad = __ballot(bad) != 0;
    nn = tc_wave_sum(a);
    n16 = tc_wave_sum(b);
    ee = tc_wave_sum(c);
    for (int k = lane; k < pitch; k += 64) {
        uint16_t v = 0;
        if (!bad && k < d) v = __builtin_bit_cast(uint16_t, tc_h(src[k]));
        dst[k] = v;
    }
    return !bad;
}

// 4 rows per block, one wave each.  stats: two floats, zeroed by the caller on the same stream.
__global__ __launch_bounds__(256) void coarse_pack_kernel(long N, int d, int pitch, const float* __restrict__ items,
                                                          uint16_t* __restrict__ items16, uint32_t* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    double nn, n16, ee;
    const bool ok = tc_pack_row(items + n * d, items16 + n * pitch, d, pitch, lane, nn, n16, ee);
    if (lane == 0) {
        if (ok) {
            atomicMax(&stats[0], __float_as_uint(tc_f32_up(tc_norm_up(nn, d))));
            atomicMax(&stats[1], __float_as_uint(tc_f32_up(tc_norm_up(ee, d))));
        } else {
            atomicMax(&stats[0], 0x7F800000u);
        }
    }
}

// (a) One wave per user.  unorm[b] = {un, un16, ue, 0}; a non-finite user row is stored as zeros with infinite norms.
__global__ __launch_bounds__(64) void coarse_user_kernel(int d, int pitch, const float* __restrict__ user, uint16_t* __restrict__ u16,
                                                         double* __restrict__ unorm) {
    const long b = blockIdx.x;
    const int lane = threadIdx.x;
    double nn, n16, ee;
    const bool ok = tc_pack_row(user + b * d, u16 + b * pitch, d, pitch, lane, nn, n16, ee);
    if (lane < 4) {
        const double inf = __builtin_huge_val();
        double v = 0.0;
        if (lane == 0) v = ok ? tc_norm_up(nn, d) : inf;
        if (lane == 1) v = ok ? tc_norm_up(n16, d) : inf;
        if (lane == 2) v = ok ? tc_norm_up(ee, d) : inf;
        unorm[4 * b + lane] = v;
    }
}

// (b) Per block: users [u0, u0 + 32) x items [n_begin, n_end) of slice blockIdx.y, 64 W items per step; one M-list per (user, slice).
// k order: each whole superblock of 64 halves (128 bytes of a row) is four MFMAs, lane (r, h) feeding halves 64 sb + 32 h + 8 s + j
// (s = 0..3, j = 0..7) of user r as A and of item r as B: four 16-byte loads of 64 contiguous bytes per lane, so the two halves of a
// wave consume a row's 128-byte line in the same instructions and no line is needed twice.  A last block of 32 halves (pitch an
// odd multiple of 32) is two MFMAs over halves 16 h + 8 s + j of it.
// Before the filter every lane tests its 32 scores against its 16 users' thresholds held in registers (the score part of
// TkFilter's thr, read from LDS after the chain, ahead of offer's first barrier: TkFilter writes thr only between the barriers of offer, which every wave
// meets every step, so the read cannot race; a stale or absent threshold only lets more through).  A score below its user's
// threshold score could not pass the filter's own entry compare either, so the lists are the same; what is saved is the filter's
// per-score LDS compare and its second barrier on the steps where no score of the block can enter any list, nearly all of them.
template <int P, int W>
__global__ __launch_bounds__(64 * W) void coarse_slice_kernel(int B, int N, int pitch, int M, int slice_len, int S,
                                                              const uint16_t* __restrict__ u16, const uint16_t* __restrict__ items16,
                                                              const int64_t* __restrict__ exclude, int n_exclude,
                                                              uint64_t* __restrict__ ws) {
    TK_FILTER_LDS(lds, P);
    constexpr int IT = 64 * W;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = blockIdx.y;
    const int u0 = blockIdx.x * TK_UT;
    const int n_begin = slice * slice_len;
    const int n_end = min(N, n_begin + slice_len);
    // The exclude lists are staged by TkFilter::start as ever, but applied here, to the few scores that pass the threshold test
    // below, not by the filter at every cut of a buffer (which costs a buffer's length x n_exclude compares per cut, most of the
    // filter's time at M = 64 and 50 excluded ids): the filter proper runs with no exclude list.  The lists are the same: an
    // excluded id never enters a buffer instead of being dropped from it.
    TkFilter<P, W>{lds, exclude, n_exclude, M, u0, B, lane, wave}.start(n_begin, n_end);
    TkFilter<P, W> flt{lds, exclude, 0, M, u0, B, lane, wave};
    __syncthreads();
    // start() left -1 for every excluded id outside this slice, most of them: the ids inside it move to the front of the user's
    // staged list, and only those exn[u] are compared
    __shared__ int exn[TK_UT];
    if (n_exclude <= TK_EX_LDS && threadIdx.x < TK_UT) {
        int c = 0;
        for (int x = 0; x < n_exclude; ++x) {
            const int32_t v = lds.ex[threadIdx.x][x];
            if (v >= 0) lds.ex[threadIdx.x][c++] = v;
        }
        exn[threadIdx.x] = c;
    }
    __syncthreads();

    const int r = lane & 31, h = lane >> 5;
    const int sb_n = pitch / 64;              // whole superblocks; a row of the pitch is 8 sb_n (+ 4) uint4
    const bool tail = (pitch & 32) != 0;
    const uint4* arow = reinterpret_cast<const uint4*>(u16 + (long)min(u0 + r, B - 1) * pitch);
    auto mfma = [](uint4 a, uint4 b, tk_f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(tc_f16x8, a), __builtin_bit_cast(tc_f16x8, b), c, 0, 0, 0);
    };
    for (int n0 = n_begin; n0 < n_end; n0 += IT) {
        const int nw = n0 + 64 * wave;
        tk_f32x16 acc[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
        if (nw < n_end) {
            const uint4* brow[TK_TN];
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) brow[c] = reinterpret_cast<const uint4*>(items16 + (long)min(nw + 32 * c + r, N - 1) * pitch);
            uint4 a[4], bq[TK_TN][4];
            auto load_sb = [&](int sb) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    a[s] = arow[8 * sb + 4 * h + s];
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) bq[c][s] = brow[c][8 * sb + 4 * h + s];
                }
            };
            if (sb_n > 0) load_sb(0);
#pragma unroll 1
            for (int sb = 0; sb < sb_n; ++sb) {
                uint4 ac[4], bc[TK_TN][4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    ac[s] = a[s];
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) bc[c][s] = bq[c][s];
                }
                if (sb + 1 < sb_n) load_sb(sb + 1);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) acc[c] = mfma(ac[s], bc[c][s], acc[c]);
            }
            if (tail) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const uint4 at = arow[8 * sb_n + 2 * h + s];
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) acc[c] = mfma(at, brow[c][8 * sb_n + 2 * h + s], acc[c]);
                }
            }
        }
        bool live[TK_TN];
        uint32_t id[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            id[c] = (uint32_t)(nw + 32 * c + r);
            live[c] = nw + 32 * c + r < n_end;
        }
        uint32_t pend = flt.pending(acc, live, TkOpenAll{});
        float tf[16];                         // the threshold score of user row (q & 3) + 8 (q >> 2) + 4 h (NaN: none yet)
#pragma unroll
        for (int q = 0; q < 16; ++q) tf[q] = tk_entry_score(lds.thr[(q & 3) + 8 * (q >> 2) + 4 * h]);
#pragma unroll
        for (int c = 0; c < TK_TN; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (acc[c][q] < tf[q]) pend &= ~(1u << (16 * c + q));
        if (n_exclude > 0) {
            for (uint32_t rem = pend; rem != 0; rem &= rem - 1) {      // this lane's surviving scores, one by one (no unrolling:
                const int t = __builtin_ctz(rem);                       //  there are few of them after the first steps)
                const int q = t & 15;
                const int i = (q & 3) + 8 * (q >> 2) + 4 * h;          // (u0 + i < B: pending() tested it)
                const uint32_t idc = t < 16 ? id[0] : id[1];
                bool out = false;
                if (n_exclude <= TK_EX_LDS) {
                    const int nx = exn[i];
#pragma unroll 1
                    for (int x = 0; x < nx; ++x) out |= lds.ex[i][x] == (int32_t)idc;
                } else {
                    const int64_t* xl = exclude + (long)(u0 + i) * n_exclude;
#pragma unroll 1
                    for (int x = 0; x < n_exclude; ++x) out |= xl[x] == (int64_t)idc;
                }
                if (out) pend &= ~(1u << t);
            }
        }
        // unconditional: the offer holds the block's barriers, and a wave with pend == 0 has to meet them too
        flt.offer(acc, pend, [&](int c) { return id[c]; });
    }
    flt.write(ws, S, slice);
}

// (d) One wave per block; block (x, y): user tile x, gathered positions 64 y .. + 63 of the tile's 32 M shortlist slots: position g
// is slot g % M of user u0 + g / M.  ent[b][m] = the exact entry of short_ids[b][m] (0: an empty slot or a NaN score).  Needs N >= 1.
template <bool VEC>
__global__ __launch_bounds__(64) void coarse_rescore_kernel(int B, int N, int d, int M, const float* __restrict__ user,
                                                            const float* __restrict__ items, const int64_t* __restrict__ short_ids,
                                                            uint64_t* __restrict__ ent) {
    __shared__ int rows[64];
    __shared__ __attribute__((aligned(16))) float stage[64 * TK_BP];
    const int lane = threadIdx.x;
    const int r = lane & 31, h = lane >> 5;
    const int u0 = blockIdx.x * TK_UT;
    const int total = TK_UT * M;
    const int g0 = 64 * blockIdx.y;
    const float* arow[1] = {user + (long)min(u0 + r, B - 1) * d};
    const int g = g0 + lane;
    const int u = g / M, m = g - u * M;
    int64_t id = -1;
    if (g < total && u0 + u < B) id = short_ids[(long)(u0 + u) * M + m];
    const bool in_range = id >= 0 && id < N;
    rows[lane] = in_range ? (int)id : 0;
    tk_wave_sync();
    tk_f32x16 acc[TK_TN];
#pragma unroll
    for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
    tk_chain<VEC>(acc, arow, items, d, stage, lane, [&](int i) { return rows[i]; });
    // C/D layout: item = lane & 31 of the column tile, user row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5): the score of position
    // g0 + 32 c + r against its owner u sits in half (u >> 2) & 1, register (u & 3) + 4 (u >> 3)
#pragma unroll
    for (int c = 0; c < TK_TN; ++c) {
        const int gc = g0 + 32 * c + r;
        const int uc = gc / M, mc = gc - uc * M;
        const int64_t idc = __shfl(id, 32 * c + r, 64);
        if (gc >= total || u0 + uc >= B || ((uc >> 2) & 1) != h) continue;
        const int qw = (uc & 3) + 4 * (uc >> 3);
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s = q == qw ? acc[c][q] : s;
        const bool ok = idc >= 0 && idc < N && !__builtin_isnan(s);
        ent[(long)(u0 + uc) * M + mc] = ok ? tk_entry(s, (uint32_t)idc) : 0;
    }
}

// (d) One wave per user: the exact entries sorted, the first min(k, L) written, and the certificate.  N = 0: ent is not read.
__global__ __launch_bounds__(64) void coarse_finish_kernel(int N, int d, int k, int M, const uint64_t* __restrict__ ent,
                                                           const float* __restrict__ short_scores, const int64_t* __restrict__ short_ids,
                                                           const double* __restrict__ unorm, const float* __restrict__ stats,
                                                           float* __restrict__ top_scores, int64_t* __restrict__ top_ids,
                                                           uint8_t* __restrict__ certified) {
    __shared__ uint64_t buf[TC_MAX_M];
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    int L = 0;
    for (int j0 = 0; j0 < TC_MAX_M; j0 += 64) {
        const int j = j0 + lane;
        const bool real = N > 0 && j < M && short_ids[b * M + j] >= 0;
        buf[j] = real ? ent[b * M + j] : 0;
        L += __popcll(__ballot(real));
    }
    tk_wave_sync();
    tk_sort_desc<TC_MAX_M>(buf, lane);
    for (int j = lane; j < k; j += 64) {
        const uint64_t e = buf[j];
        top_scores[b * k + j] = e ? tk_entry_score(e) : -__builtin_huge_valf();
        top_ids[b * k + j] = e ? tk_entry_id(e) : -1;
    }
    if (lane != 0) return;
    const double inf = __builtin_huge_val();
    const double NRM = (double)stats[0], ERR = (double)stats[1];
    const double un = unorm[4 * b], un16 = unorm[4 * b + 1], ue = unorm[4 * b + 2];
    // (comparisons with a NaN are false: a NaN anywhere leaves the row uncertified)
    bool ok = NRM < inf && ERR < inf && un < inf && un16 < inf && ue < inf && NRM >= 0.0 && ERR >= 0.0 && d < (1 << 23);
    ok = ok && tc_mul_up(un, NRM) <= 0x1p100;
    if (ok && L >= M) {
        const uint64_t ek = buf[k - 1];
        const double dd = (double)d;
        const double gamma = tc_up(tc_up(dd * 0x1p-24) / (1.0 - dd * 0x1p-24));       // (the denominator is exact)
        const double alpha = dd * 0x1p-21;
        double E = tc_mul_up(ue, NRM);
        E = tc_add_up(E, tc_mul_up(un16, ERR));
        E = tc_add_up(E, tc_mul_up(gamma, tc_mul_up(un, NRM)));
        E = tc_add_up(E, tc_mul_up(alpha, tc_mul_up(un16, tc_add_up(NRM, ERR))));
        E = tc_add_up(E, tc_up(dd * 0x1p-140));
        const double cM = (double)short_scores[b * M + M - 1];
        ok = ek != 0 && (double)tk_entry_score(ek) > tc_add_up(cM, E);
    }
    certified[b] = ok ? 1 : 0;
}

static bool coarse_args_ok(int32_t B, int64_t N, int32_t d, int32_t k, int32_t M) {
    return topk_args_ok(B, N, d, k) && M >= k && M <= TC_MAX_M && d <= 0x7FFFFFFF - 31;
}

static size_t tc_align(size_t x) { return (x + 255) / 256 * 256; }

// The workspace after its base is aligned to 16 bytes: u16 [B, pitch], unorm [B, 4] f64, the slice lists [B, S, M], the
// shortlist (ids, scores) and the exact entries [B, M].
struct TcLayout {
    size_t u16, unorm, lists, short_ids, short_scores, ent, total;
};
static TcLayout tc_layout(int32_t B, int64_t N, int32_t d, int32_t M) {
    const TkGeom g = topk_geom(B, N);
    TcLayout L;
    size_t o = 0;
    L.u16 = o;          o += tc_align((size_t)B * (size_t)tc_pitch(d) * sizeof(uint16_t));
    L.unorm = o;        o += tc_align((size_t)B * 4 * sizeof(double));
    L.lists = o;        o += tc_align((size_t)B * (size_t)g.S * (size_t)M * sizeof(uint64_t));
    L.short_ids = o;    o += tc_align((size_t)B * (size_t)M * sizeof(int64_t));
    L.short_scores = o; o += tc_align((size_t)B * (size_t)M * sizeof(float));
    L.ent = o;          o += tc_align((size_t)B * (size_t)M * sizeof(uint64_t));
    L.total = o;
    return L;
}

}  // namespace nrms

using namespace nrms;

extern "C" int32_t nrms_catalogue_f16_pitch(int32_t d) { return d >= 1 && d <= 0x7FFFFFFF - 31 ? tc_pitch(d) : 0; }

extern "C" int nrms_catalogue_pack_f16(int64_t N, int32_t d, const float* items, uint16_t* items16, float* stats, void* stream) {
    const char* who = "catalogue_pack_f16";
    NRMS_REQUIRE(N >= 0 && N <= TK_MAX_N, "%s: N must be in [0, %lld] (N=%lld)", who, (long long)TK_MAX_N, (long long)N);
    NRMS_REQUIRE(d >= 1 && d <= 0x7FFFFFFF - 31, "%s: d must be >= 1 (d=%d)", who, d);
    NRMS_REQUIRE(stats, "%s: stats is null", who);
    NRMS_REQUIRE(((uintptr_t)stats & 3) == 0, "%s: stats must be 4-byte aligned", who);
    NRMS_REQUIRE(N == 0 || items, "%s: items is null", who);
    NRMS_REQUIRE(N == 0 || items16, "%s: items16 is null", who);
    NRMS_REQUIRE(((uintptr_t)items & 3) == 0, "%s: items must be 4-byte aligned", who);
    NRMS_REQUIRE(((uintptr_t)items16 & 15) == 0, "%s: items16 must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    if (hipMemsetAsync(stats, 0, 2 * sizeof(float), s) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", who);
        return NRMS_ELAUNCH;
    }
    if (N == 0) return NRMS_OK;
    hipLaunchKernelGGL(coarse_pack_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, (long)N, d, tc_pitch(d), items, items16,
                       (uint32_t*)stats);
    return check_launch(who);
}

extern "C" size_t nrms_topk_dot_coarse_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k, int32_t M) {
    if (!coarse_args_ok(B, N, d, k, M)) return 0;
    return 256 + tc_layout(B, N, d, M).total;          // never 0 for accepted arguments; 16 of the 256 align the base
}

extern "C" int nrms_topk_dot_coarse(int32_t B, int64_t N, int32_t d, int32_t k, int32_t M, const float* user, const float* items,
                                    const uint16_t* items16, const float* stats, const int64_t* exclude, int32_t n_exclude,
                                    float* top_scores, int64_t* top_ids, uint8_t* certified, float* short_scores, int64_t* short_ids,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "topk_dot_coarse";
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE(M >= k && M <= TC_MAX_M, "%s: M must be in [k, %d] (k=%d, M=%d)", who, TC_MAX_M, k, M);
    NRMS_REQUIRE(d <= 0x7FFFFFFF - 31, "%s: d too large (d=%d)", who, d);
    if (B == 0) return NRMS_OK;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"items16", items16, N != 0, 16},
                             {"stats", stats, true, 4}, {"top_scores", top_scores, true, 1}, {"top_ids", top_ids, true, 1},
                             {"certified", certified, true, 1}, {"short_scores", short_scores, false, 1},
                             {"short_ids", short_ids, false, 1}},
                       workspace, workspace_bytes, nrms_topk_dot_coarse_workspace_bytes(B, N, d, k, M), 8);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    const TcLayout L = tc_layout(B, N, d, M);
    char* base = (char*)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    uint16_t* u16 = (uint16_t*)(base + L.u16);
    double* unorm = (double*)(base + L.unorm);
    uint64_t* lists = (uint64_t*)(base + L.lists);
    int64_t* sids = short_ids ? short_ids : (int64_t*)(base + L.short_ids);
    float* sscores = short_scores ? short_scores : (float*)(base + L.short_scores);
    uint64_t* ent = (uint64_t*)(base + L.ent);
    const TkGeom g = topk_geom(B, N);
    const int n = (int)N, pitch = tc_pitch(d);
    // (the stages' timing names do not start with the call's, so that reading "topk_dot_coarse" counts the call once)
    {
        TimingScope t1("coarse_stage(user)", s);
        hipLaunchKernelGGL(coarse_user_kernel, dim3(B), dim3(64), 0, s, d, pitch, user, u16, unorm);
        rc = check_launch("topk_dot_coarse(user)");
        if (rc != NRMS_OK) return rc;
    }
    tk_with_pw(M, [&](auto P, auto W) {
        // P from tk_with_pw; its W (2 waves at P = 512, whose buffers fill the LDS beside tk_chain's staging blocks) is not taken: this
        // kernel stages nothing in LDS, so 8 waves fit at every P (TkFilter's lists do not depend on W)
        constexpr int p = decltype(P)::value, w = TK_WAVES;
        if (g.S > 0) {
            TimingScope t2("coarse_stage(slices)", s);
            hipLaunchKernelGGL((coarse_slice_kernel<p, w>), dim3(g.tiles, g.S), dim3(64 * w), 0, s, B, n, pitch, M, g.slice_len, g.S,
                               u16, items16, exclude, n_exclude, lists);
            rc = check_launch("topk_dot_coarse(slices)");
            if (rc != NRMS_OK) return;
        }
        TimingScope t3("coarse_stage(merge)", s);
        hipLaunchKernelGGL(topk_merge_kernel<p>, dim3(B), dim3(64), 0, s, B, M, g.S, lists, sscores, sids, M);
        rc = check_launch("topk_dot_coarse(merge)");
    });
    if (rc != NRMS_OK) return rc;
    TimingScope t4("coarse_stage(rescore)", s);
    if (N > 0) {
        const dim3 grid(g.tiles, (TK_UT * M + 63) / 64);
        if (tk_vec_ok(d, user, items))
            hipLaunchKernelGGL(coarse_rescore_kernel<true>, grid, dim3(64), 0, s, B, n, d, M, user, items, sids, ent);
        else
            hipLaunchKernelGGL(coarse_rescore_kernel<false>, grid, dim3(64), 0, s, B, n, d, M, user, items, sids, ent);
        rc = check_launch("topk_dot_coarse(rescore)");
        if (rc != NRMS_OK) return rc;
    }
    hipLaunchKernelGGL(coarse_finish_kernel, dim3(B), dim3(64), 0, s, n, d, k, M, ent, sscores, sids, unorm, stats, top_scores, top_ids,
                       certified);
    return check_launch("topk_dot_coarse(finish)");
}
