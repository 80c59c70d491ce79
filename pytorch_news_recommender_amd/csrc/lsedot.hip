// The exact log-partition of a softmax over a whole catalogue, without a [B, N] score matrix (include/nrms_hip.h:
// nrms_logsumexp_dot, whose header comment states the contract): for up to 8 (inv_temperature, bias_scale) variants at once,
// lse(b, j) = log sum over the eligible n of exp(z_j(b, n)), z_j = fmaf(s(b, n), inv_temperature[j], bias_scale[j] * bias[n]).
//
// The scores are tk_chain's (topk_entry.h), the one chain topk_slice_kernel and rank_count_kernel run, over rank_count_kernel's
// grid (32-user tiles x catalogue slices, two 32 x 32 tiles per wave).  What is new is the epilogue and its reduction:
// init   (lse_init_kernel): zeroes the call's keys, counts and masses, whatever the workspace held.
// pass 1 (lse_scan_kernel<SUM = false>): the exact maximum and the count of the eligible z_j of every (user, variant): a float
//   maximum is order-free, and it reaches the workspace as an integer atomicMax on its order-preserving 32-bit key.
// pass 2 (lse_scan_kernel<SUM = true>): t = expf(z_j - zmax) in [0, 1], converted to fixed point (unit 2^-63, two 64-bit limbs:
//   floor(t 2^31) and the next 32 bits) and added up in integers.  Integer addition is associative, so neither the lanes' fold,
//   the waves' partial sums in LDS nor the blocks' atomics can change a bit of the mass: the result is a function of the multiset
//   of the eligible z_j, not of the launch geometry.
// finish (lse_finish_kernel): one lane per (user, variant): zmax + log(mass) in fp64, rounded once to fp32.
//
// Exclusion comes BEFORE the maximum and the sum.  A block compacts the exclude ids of its 32 users that fall into its slice
// into LDS once (lists longer than TK_EX_LDS stay in global memory and are walked there); in every step a wave marks, in a
// 64-entry LDS row of 32-bit user masks, the pairs of its 64 items that are excluded, and the lane that holds a pair clears it.
//
// The fold: a lane holds one value per accumulator register q (16 users) for its item; lse_fold reduces over the 32 items of a
// half wave in a transposing butterfly (16 + 8 + 4 + 2 + 1 exchanges in place of 16 x 5) and leaves user q = (lane >> 1) & 15 of
// the half in lanes 2 q and 2 q + 1, whose even lane adds it to the wave's running value in LDS.
#include <math.h>

#include "topk_kernels.h"

namespace nrms {

constexpr int LSE_MAX_J = 8;
constexpr int LSE_MASS_WORDS = 2;               // hi: units of 2^-31; lo: units of 2^-63

struct LseParams {
    float inv_t[LSE_MAX_J];
    float bscale[LSE_MAX_J];
};

// The order-preserving key of a float, -0.0 as +0.0 (the upper half of tk_entry); 0 lies below every real key.
__device__ __forceinline__ uint32_t lse_key(float z) {
    const uint32_t u = __float_as_uint(z == 0.0f ? 0.0f : z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lse_key_value(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// t in [0, 1] as fixed point: hi = floor(t 2^31) <= 2^31, lo = floor(frac(t 2^31) 2^32) < 2^32.  The two scalings are by powers
// of two and the subtraction is of a number's own integer part: all exact, so hi 2^-31 + lo 2^-63 = t for every fp32
// t >= 2^-40 (24 significant bits above 2^-63) and t truncated to a multiple of 2^-63 below that.
__device__ __forceinline__ void lse_fixed(float t, uint32_t& hi, uint32_t& lo) {
    const float x = t * 0x1p31f;
    const float xi = truncf(x);
    hi = (uint32_t)xi;
    lo = (uint32_t)((x - xi) * 0x1p32f);
}

// v[q], q in [0, 16), of the 32 lanes of each half wave -> op over those 32 lanes of v[(lane >> 1) & 15].
template <class T, class Op>
__device__ __forceinline__ T lse_fold(const T (&v)[16], int lane, Op op) {
    T a[8], b[4], c[2];
    const bool u16 = lane & 16, u8 = lane & 8, u4 = lane & 4, u2 = lane & 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = op(u16 ? v[i + 8] : v[i], __shfl_xor(u16 ? v[i] : v[i + 8], 16));
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = op(u8 ? a[i + 4] : a[i], __shfl_xor(u8 ? a[i] : a[i + 4], 8));
#pragma unroll
    for (int i = 0; i < 2; ++i) c[i] = op(u4 ? b[i + 2] : b[i], __shfl_xor(u4 ? b[i] : b[i + 2], 4));
    const T e = op(u2 ? c[1] : c[0], __shfl_xor(u2 ? c[0] : c[1], 2));
    return op(e, __shfl_xor(e, 1));
}

__global__ __launch_bounds__(256) void lse_init_kernel(long BJ, unsigned long long* __restrict__ mass, uint32_t* __restrict__ zkey,
                                                       uint32_t* __restrict__ cnt) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < BJ; i += (long)gridDim.x * 256) {
        mass[LSE_MASS_WORDS * i] = 0;
        mass[LSE_MASS_WORDS * i + 1] = 0;
        zkey[i] = 0;
        cnt[i] = 0;
    }
}

// Per block: users [u0, u0 + 32) x items [n_begin, n_end) of slice blockIdx.y, 64 W items per step.  zkey, cnt [B, J]; mass
// [B, J, 2].  SUM = false writes zkey and cnt, SUM = true reads them and writes mass.  The step loop holds no block barrier.
template <int W, bool VEC, bool SUM>
__global__ __launch_bounds__(64 * W) void lse_scan_kernel(int B, int N, int d, int J, int slice_len, const float* __restrict__ user,
                                                          const float* __restrict__ items, const float* __restrict__ bias,
                                                          LseParams par, const int64_t* __restrict__ exclude, int n_exclude,
                                                          uint32_t* __restrict__ zkey, uint32_t* __restrict__ cnt,
                                                          unsigned long long* __restrict__ mass) {
    __shared__ __attribute__((aligned(16))) float stage[W][64 * TK_BP];
    __shared__ int2 xl[TK_UT * TK_EX_LDS];          // (id, user row) of the block's exclude ids inside its slice
    __shared__ int xl_n;
    __shared__ uint32_t xm[W][64];                      // per wave: bit u of entry i = user row u excludes item nw + i
    __shared__ float p_it[LSE_MAX_J], p_bs[LSE_MAX_J];
    __shared__ float zm[SUM ? LSE_MAX_J : 1][TK_UT];    // SUM: the block's maxima (NaN: nothing to add for this pair of (user, j))
    __shared__ unsigned long long a_sum[SUM ? W : 1][LSE_MAX_J][TK_UT][LSE_MASS_WORDS];
    __shared__ float a_max[SUM ? 1 : W][LSE_MAX_J][TK_UT];
    __shared__ uint32_t a_cnt[SUM ? 1 : W][LSE_MAX_J][TK_UT];
    constexpr int IT = 64 * W;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u0 = blockIdx.x * TK_UT;
    const int n_begin = blockIdx.y * slice_len;
    const int n_end = min(N, n_begin + slice_len);
    const bool ex_lds = n_exclude <= TK_EX_LDS;
    const float ninf = -__builtin_huge_valf();

    if (threadIdx.x == 0) xl_n = 0;
    if (threadIdx.x < LSE_MAX_J) {
        p_it[threadIdx.x] = par.inv_t[threadIdx.x];
        p_bs[threadIdx.x] = par.bscale[threadIdx.x];
    }
    for (int i = threadIdx.x; i < W * 64; i += 64 * W) xm[i / 64][i % 64] = 0;
    for (int i = threadIdx.x; i < LSE_MAX_J * TK_UT; i += 64 * W) {
        const int j = i / TK_UT, u = i % TK_UT;
        if constexpr (SUM) {
            // a pair of (user, j) with no eligible item or an infinite maximum adds nothing: the finish kernel sets its lse
            float z = __builtin_nanf("");
            if (u0 + u < B && j < J && cnt[(long)(u0 + u) * J + j]) {
                const float v = lse_key_value(zkey[(long)(u0 + u) * J + j]);
                if (!__builtin_isinf(v)) z = v;
            }
            zm[j][u] = z;
#pragma unroll
            for (int w = 0; w < W; ++w) a_sum[w][j][u][0] = a_sum[w][j][u][1] = 0;
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                a_max[w][j][u] = ninf;
                a_cnt[w][j][u] = 0;
            }
        }
    }
    __syncthreads();
    if (ex_lds)
        for (int i = threadIdx.x; i < TK_UT * n_exclude; i += 64 * W) {
            const int u = i / n_exclude, e = i - u * n_exclude;
            const int64_t v = u0 + u < B ? exclude[(long)(u0 + u) * n_exclude + e] : -1;
            if (v >= n_begin && v < n_end) xl[atomicAdd(&xl_n, 1)] = make_int2((int)v, u);
        }
    __syncthreads();
    const int n_xl = xl_n;

    const int r = lane & 31, h = lane >> 5;
    const int uq = ((lane >> 1) & 3) + 8 * ((lane >> 3) & 3) + 4 * h;          // the user row lse_fold leaves in this lane
    const float* arow[1] = {user + (long)min(u0 + r, B - 1) * d};
    float* st = stage[wave];
    for (int n0 = n_begin; n0 < n_end; n0 += IT) {
        const int nw = n0 + 64 * wave;
        if (nw >= n_end) continue;
        float bv[TK_TN] = {};          // loaded ahead of the chain, which hides the latency
        if (bias) {
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) bv[c] = bias[min(nw + 32 * c + r, N - 1)];
        }
        // the excluded pairs of this step: entry i of xm[wave], bit u
        if (ex_lds) {
            for (int i = lane; i < n_xl; i += 64) {
                const int2 e = xl[i];
                const unsigned off = (unsigned)(e.x - nw);
                if (off < 64u) atomicOr(&xm[wave][off], 1u << e.y);
            }
        } else {
            for (int i = lane; i < TK_UT * n_exclude; i += 64) {
                const int u = i / n_exclude, e = i - u * n_exclude;
                if (u0 + u >= B) break;
                const int64_t v = exclude[(long)(u0 + u) * n_exclude + e];
                if (v >= nw && v < (int64_t)nw + 64) atomicOr(&xm[wave][(int)(v - nw)], 1u << u);
            }
        }
        tk_wave_sync();
        uint32_t xmask[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) xmask[c] = xm[wave][32 * c + r];
        tk_wave_sync();
#pragma unroll
        for (int c = 0; c < TK_TN; ++c)
            if (xmask[c]) xm[wave][32 * c + r] = 0;
        tk_wave_sync();

        tk_f32x16 acc[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
        tk_chain<VEC>(acc, arow, items, d, st, lane, [&](int i) { return min(nw + i, N - 1); });
        // C/D layout: item = lane & 31 of the column tile, user row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5).  open[c] bit q: the
        // pair is a real item of the slice that its user does not exclude.
        uint32_t open[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            open[c] = 0;
            if (nw + 32 * c + r < n_end) {
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (!((xmask[c] >> ((q & 3) + 8 * (q >> 2) + 4 * h)) & 1u)) open[c] |= 1u << q;
            }
        }
#pragma unroll 1
        for (int j = 0; j < J; ++j) {
            const float it = p_it[j], bs = p_bs[j];
            float cj[TK_TN];
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) cj[c] = bias ? bs * bv[c] : 0.0f;
            if constexpr (SUM) {
                unsigned long long vh[16], vl[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float zmq = zm[j][(q & 3) + 8 * (q >> 2) + 4 * h];
                    vh[q] = 0;
                    vl[q] = 0;
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) {
                        const float z = __builtin_fmaf(acc[c][q], it, cj[c]);
                        const float a = z - zmq;             // NaN for a NaN z and for a pair (user, j) that adds nothing
                        float t = 0.0f;
                        if (((open[c] >> q) & 1u) && !__builtin_isnan(a)) t = fminf(expf(a), 1.0f);
                        uint32_t hi, lo;
                        lse_fixed(t, hi, lo);
                        vh[q] += hi;
                        vl[q] += lo;
                    }
                }
                auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
                const unsigned long long fh = lse_fold(vh, lane, add), fl = lse_fold(vl, lane, add);
                if (!(lane & 1)) {
                    a_sum[wave][j][uq][0] += fh;
                    a_sum[wave][j][uq][1] += fl;
                }
            } else {
                float vm[16];
                uint32_t vc[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    vm[q] = ninf;
                    vc[q] = 0;
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) {
                        const float z = __builtin_fmaf(acc[c][q], it, cj[c]);
                        if (((open[c] >> q) & 1u) && !__builtin_isnan(z)) {
                            vm[q] = fmaxf(vm[q], z);
                            vc[q] += 1;
                        }
                    }
                }
                const float fm = lse_fold(vm, lane, [](float x, float y) { return fmaxf(x, y); });
                const uint32_t fc = lse_fold(vc, lane, [](uint32_t x, uint32_t y) { return x + y; });
                if (!(lane & 1)) {
                    a_max[wave][j][uq] = fmaxf(a_max[wave][j][uq], fm);
                    a_cnt[wave][j][uq] += fc;
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < J * TK_UT; i += 64 * W) {
        const int j = i / TK_UT, u = i % TK_UT;
        if (u0 + u >= B) continue;
        const long o = (long)(u0 + u) * J + j;
        if constexpr (SUM) {
            unsigned long long sh = 0, sl = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                sh += a_sum[w][j][u][0];
                sl += a_sum[w][j][u][1];
            }
            if (sh) atomicAdd(&mass[LSE_MASS_WORDS * o], sh);
            if (sl) atomicAdd(&mass[LSE_MASS_WORDS * o + 1], sl);
        } else {
            float m = ninf;
            uint32_t n = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                m = fmaxf(m, a_max[w][j][u]);
                n += a_cnt[w][j][u];
            }
            if (n) {
                atomicMax(&zkey[o], lse_key(m));
                atomicAdd(&cnt[o], n);
            }
        }
    }
}

// One lane per (user, variant).  mass_out: the test hook's copy of the two limbs.
__global__ __launch_bounds__(256) void lse_finish_kernel(long BJ, const unsigned long long* __restrict__ mass,
                                                         const uint32_t* __restrict__ zkey, const uint32_t* __restrict__ cnt,
                                                         float* __restrict__ lse, float* __restrict__ zmax,
                                                         int32_t* __restrict__ n_eligible, uint64_t* __restrict__ mass_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BJ) return;
    const uint32_t n = cnt[i];
    const float inf = __builtin_huge_valf();
    const float zx = n ? lse_key_value(zkey[i]) : -inf;
    const unsigned long long hi = mass[LSE_MASS_WORDS * i], lo = mass[LSE_MASS_WORDS * i + 1];
    float out = zx;                                   // -inf: nothing eligible, or only -inf logits; +inf: a +inf logit
    if (n && !__builtin_isinf(zx)) out = (float)((double)zx + log((double)hi * 0x1p-31 + (double)lo * 0x1p-63));
    if (lse) lse[i] = out;
    if (zmax) zmax[i] = zx;
    if (n_eligible) n_eligible[i] = (int32_t)n;
    if (mass_out) {
        mass_out[LSE_MASS_WORDS * i] = hi;
        mass_out[LSE_MASS_WORDS * i + 1] = lo;
    }
}

static bool lse_args_ok(int32_t B, int64_t N, int32_t d, int32_t J, int32_t n_exclude) {
    return B >= 0 && N >= 0 && N <= TK_MAX_N && d >= 1 && J >= 1 && J <= LSE_MAX_J && n_exclude >= 0;
}

static size_t lse_mass_bytes(int32_t B, int32_t J) { return (size_t)B * (size_t)J * LSE_MASS_WORDS * sizeof(uint64_t); }

// nrms_logsumexp_dot and nrms_logsumexp_dot_mass (hook: mass_out is the required output, lse is null): one body.
static int lse_call(const char* who, bool hook, int32_t B, int64_t N, int32_t d, int32_t J, const float* user, const float* items,
                    const float* bias, const float* inv_temperature, const float* bias_scale, const int64_t* exclude,
                    int32_t n_exclude, float* lse, float* zmax, int32_t* n_eligible, uint64_t* mass_out, void* workspace,
                    size_t workspace_bytes, void* stream) {
    int rc = tk_check_dims(who, B, N, TK_MAX_N, d, "J", J, LSE_MAX_J, n_exclude);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE(inv_temperature, "%s: inv_temperature is null", who);
    LseParams par{};
    for (int j = 0; j < J; ++j) {
        NRMS_REQUIRE(inv_temperature[j] >= 0.0f && isfinite(inv_temperature[j]),
                     "%s: inv_temperature must be finite and >= 0 (inv_temperature[%d]=%g)", who, j, (double)inv_temperature[j]);
        NRMS_REQUIRE(!bias_scale || isfinite(bias_scale[j]), "%s: bias_scale must be finite (bias_scale[%d]=%g)", who, j,
                     (double)(bias_scale ? bias_scale[j] : 0.0f));
        par.inv_t[j] = inv_temperature[j];
        par.bscale[j] = bias_scale ? bias_scale[j] : 1.0f;
    }
    if (B == 0) return NRMS_OK;
    if (!exclude) n_exclude = 0;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"bias", bias, false, 4},
                             {hook ? "mass" : "lse", hook ? (const void*)mass_out : (const void*)lse, true, 1}},
                       workspace, workspace_bytes, nrms_logsumexp_dot_workspace_bytes(B, N, d, J, n_exclude), 8);
    if (rc != NRMS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    unsigned long long* mass = (unsigned long long*)workspace;
    uint32_t* zkey = (uint32_t*)((char*)workspace + lse_mass_bytes(B, J));
    uint32_t* cnt = zkey + (size_t)B * J;
    const long BJ = (long)B * J;
    const int fin_blocks = (int)((BJ + 255) / 256);
    char what[64];
    hipLaunchKernelGGL(lse_init_kernel, dim3(std::min(fin_blocks, 4096)), dim3(256), 0, s, BJ, mass, zkey, cnt);
    snprintf(what, sizeof what, "%s(init)", who);
    rc = check_launch(what);
    if (rc != NRMS_OK) return rc;
    const TkGeom g = tk_geom(B, N, false);          // no minimum slice: the workspace does not grow with the slice count
    if (g.S > 0) {
        const dim3 grid(g.tiles, g.S), block(64 * TK_WAVES);
        const int n = (int)N;
        tk_with_flags([&](auto V) {
            constexpr bool v = decltype(V)::value;
            hipLaunchKernelGGL((lse_scan_kernel<TK_WAVES, v, false>), grid, block, 0, s, B, n, d, J, g.slice_len, user, items, bias, par,
                               exclude, n_exclude, zkey, cnt, mass);
            snprintf(what, sizeof what, "%s(max)", who);
            rc = check_launch(what);
            if (rc != NRMS_OK) return;
            hipLaunchKernelGGL((lse_scan_kernel<TK_WAVES, v, true>), grid, block, 0, s, B, n, d, J, g.slice_len, user, items, bias, par,
                               exclude, n_exclude, zkey, cnt, mass);
            snprintf(what, sizeof what, "%s(sum)", who);
            rc = check_launch(what);
        }, tk_vec_ok(d, user, items));
        if (rc != NRMS_OK) return rc;
    }
    hipLaunchKernelGGL(lse_finish_kernel, dim3(fin_blocks), dim3(256), 0, s, BJ, mass, zkey, cnt, lse, zmax, n_eligible, mass_out);
    snprintf(what, sizeof what, "%s(finish)", who);
    return check_launch(what);
}

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_logsumexp_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t J, int32_t n_exclude) {
    if (!lse_args_ok(B, N, d, J, n_exclude)) return 0;
    // the masses [B, J, 2], the maxima's keys [B, J] and the counts [B, J]; never 0 for accepted arguments
    return 256 + lse_mass_bytes(B, J) + 2 * (size_t)B * (size_t)J * sizeof(uint32_t);
}

extern "C" int nrms_logsumexp_dot(int32_t B, int64_t N, int32_t d, int32_t J, const float* user, const float* items,
                                  const float* bias, const float* inv_temperature, const float* bias_scale, const int64_t* exclude,
                                  int32_t n_exclude, float* lse, float* zmax, int32_t* n_eligible, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return lse_call("logsumexp_dot", false, B, N, d, J, user, items, bias, inv_temperature, bias_scale, exclude, n_exclude, lse, zmax,
                    n_eligible, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int nrms_logsumexp_dot_mass(int32_t B, int64_t N, int32_t d, int32_t J, const float* user, const float* items,
                                       const float* bias, const float* inv_temperature, const float* bias_scale,
                                       const int64_t* exclude, int32_t n_exclude, uint64_t* mass, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return lse_call("logsumexp_dot_mass", true, B, N, d, J, user, items, bias, inv_temperature, bias_scale, exclude, n_exclude, nullptr,
                    nullptr, nullptr, mass, workspace, workspace_bytes, stream);
}
