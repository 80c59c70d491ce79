// A sectioned front page: per user the k best items of EVERY section of a catalogue in one call, without a [B, N] score
// matrix (include/nrms_hip.h: nrms_topk_sections_dot, whose header comment states the contract).
//
// The catalogue is stored section after section and laid out in the 32-row tiles of nrms_topk_grouped_dot (csrc/topk.hip), which
// never straddle a section.  The host does not know the section lengths (section_ptr lives on the device), so everything is
// sized from bounds: at most nt_max = (N + 31 G) / 32 tiles, slices of L tiles that never straddle a section either, and at most
// S_max = ceil(nt_max / L) + G of them (each section wastes less than one slice).
//
// Kernel 1 (topksec_tables_kernel, one block): the tile table, the slice table {first tile, end tile, section} with empty
//   entries past the real total, and slice_of_section[G + 1], the prefix sum of ceil(tiles_g / L).
// Kernel 2 (topksec_slice_kernel): grid = 32-user tiles x S_max.  topk_slice_kernel's GROUPED path with the block's range taken
//   from its slice-table entry (an empty entry exits without writing) and ONE A operand, the user's own row, for both column
//   tiles: the score chain of nrms_topk_dot, the same bits.  BIAS adds bias[row] to the finished accumulator, as
//   nrms_topk_dot_biased does.
// Kernel 3 (topksec_merge_kernel): one wave per (user, section) over the k-lists of the section's slices, topk_merge_kernel
//   with a per-block source range.
//
// These are sibling kernels, not new modes of topk_slice_kernel: the existing instantiations' score bits are pinned by their
// tests, and their source stays untouched.
#include "topk_kernels.h"

namespace nrms {

constexpr int TKS_MAX_G = 4096;              // sections per call: four per thread of the one-block table kernel
constexpr int TKS_MAX_SLICE_TILES = 1 << 20;
constexpr int TKS_MAX_SLICES = 65535;        // the slice kernel's grid.y

// One slice: tiles [t0, t1) of section grp (t0 == t1: an unused entry past the last real slice).
struct TkSlice {
    int t0, t1, grp, pad;
};

// One block: the three tables.  Section g (rows [section_ptr[g], section_ptr[g + 1]), clamped to [0, N]) gets ceil(len / 32)
// consecutive tiles and ceil(tiles / L) consecutive slices, the sections in order.  A section_ptr that is not nondecreasing
// from 0 to N cannot send a row outside [0, N), a tile past n_tiles or a slice past S_max.
__global__ __launch_bounds__(1024) void topksec_tables_kernel(int N, int G, int n_tiles, int L, int S_max,
                                                              const int64_t* __restrict__ section_ptr, TkTile* __restrict__ tiles,
                                                              TkSlice* __restrict__ slices, int* __restrict__ slice_of_section) {
    __shared__ long tpart[1024], spart[1024];
    __shared__ long total[2];
    const int per = (G + 1023) / 1024;
    const int lo = min(G, (int)threadIdx.x * per), hi = min(G, lo + per);
    auto span = [&](int g, int& row, int& len) {
        row = 0;
        len = 0;
        if (N == 0) return;          // section_ptr may be null
        const long a = min((long)N, max(0L, (long)section_ptr[g]));
        const long e = min((long)N, max(0L, (long)section_ptr[g + 1]));
        row = (int)a;
        len = (int)max(0L, e - a);
    };
    long st = 0, ss = 0;
    for (int g = lo; g < hi; ++g) {
        int row, len;
        span(g, row, len);
        const long nt = (len + 31) / 32;
        st += nt;
        ss += (nt + L - 1) / L;
    }
    tpart[threadIdx.x] = st;
    spart[threadIdx.x] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
        long trun = 0, srun = 0;
        for (int i = 0; i < 1024; ++i) {
            const long a = tpart[i], b = spart[i];
            tpart[i] = trun;
            spart[i] = srun;
            trun += a;
            srun += b;
        }
        total[0] = trun;
        total[1] = srun;
    }
    __syncthreads();
    long t = tpart[threadIdx.x], s = spart[threadIdx.x];
    for (int g = lo; g < hi; ++g) {
        int row, len;
        span(g, row, len);
        const long nt = (len + 31) / 32, ns = (nt + L - 1) / L;
        slice_of_section[g] = (int)min(s, (long)S_max);
        for (long j = 0; j < nt && t + j < n_tiles; ++j) tiles[t + j] = TkTile{row + 32 * (int)j, min(32, len - 32 * (int)j), g, 0};
        for (long j = 0; j < ns && s + j < S_max; ++j)
            slices[s + j] = TkSlice{(int)min(t + j * L, (long)n_tiles), (int)min(t + min((j + 1) * L, nt), (long)n_tiles), g, 0};
        s += ns;
        t += nt;
    }
    if (threadIdx.x == 0) slice_of_section[G] = (int)min(total[1], (long)S_max);
    for (long u = total[0] + threadIdx.x; u < n_tiles; u += 1024) tiles[u] = TkTile{0, 0, 0, 0};
    for (long u = total[1] + threadIdx.x; u < S_max; u += 1024) slices[u] = TkSlice{0, 0, 0, 0};
}

// topk_slice_kernel (topk_kernels.h, whose comment describes the operands, the filter and the buffers) for one slice-table
// entry per block: users [u0, u0 + 32) x the tiles [t0, t1) of one section, 2 W tiles per step.  Rows past a tile's len are
// masked, the id of row n is item_ids[n], and both column tiles take the user's own row as A operand.
template <int P, int W, bool VEC, bool BIAS>
__global__ __launch_bounds__(64 * W) void topksec_slice_kernel(int B, int N, int d, int k, int S,
                                                               const float* __restrict__ user, const float* __restrict__ items,
                                                               const int64_t* __restrict__ exclude, int n_exclude,
                                                               uint64_t* __restrict__ ws, const TkSlice* __restrict__ slices,
                                                               const TkTile* __restrict__ tiles,
                                                               const int32_t* __restrict__ item_ids,
                                                               const float* __restrict__ bias) {
    __shared__ uint64_t buf[TK_UT][P];
    __shared__ uint64_t thr[TK_UT];
    __shared__ int cnt[TK_UT];
    __shared__ int32_t ex[TK_UT][TK_EX_LDS];
    __shared__ __attribute__((aligned(16))) float stage[W][64 * TK_BP];
    constexpr int IT = 64 * W;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u0 = blockIdx.x * TK_UT;
    const int slice = blockIdx.y;
    const TkSlice sl = slices[slice];
    const int t_end = __builtin_amdgcn_readfirstlane(sl.t1);
    const int n_begin = 32 * __builtin_amdgcn_readfirstlane(sl.t0), n_end = 32 * t_end;      // tile rows, not catalogue rows
    if (n_begin >= n_end) return;          // an unused entry: the whole block leaves before any barrier, nothing is written
    const bool ex_lds = n_exclude <= TK_EX_LDS;

    if (threadIdx.x < TK_UT) {
        thr[threadIdx.x] = 0;
        cnt[threadIdx.x] = 0;
    }
    if (ex_lds)      // ids, in any slice; everything that is no 31-bit id becomes -1
        for (int i = threadIdx.x; i < TK_UT * n_exclude; i += 64 * W) {
            const int u = i / n_exclude, e = i - u * n_exclude;
            const int64_t v = u0 + u < B ? exclude[(long)(u0 + u) * n_exclude + e] : -1;
            ex[u][e] = (v >= 0 && v <= 0x7FFFFFFF) ? (int32_t)v : -1;
        }
    __syncthreads();

    // cut user i's buffer (c entries) down to its best k, excluded ids dropped; returns the new threshold, sets c
    auto flush = [&](int i, int& c) {
        tk_drop_excluded(buf[i], c, ex_lds ? ex[i] : nullptr, exclude + (long)(u0 + i) * n_exclude, n_exclude, lane);
        return tk_select<P>(buf[i], c, k, lane);
    };

    const int r = lane & 31, h = lane >> 5;
    const float* arow = user + (long)min(u0 + r, B - 1) * d;
    float* st = stage[wave];
    const int m_full = d / 32;
    for (int n0 = n_begin; n0 < n_end; n0 += IT) {
        const int nw = n0 + 64 * wave;
        tk_f32x16 acc[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
        // the wave's two tiles (row of their first item, valid rows); wave-uniform
        int trow[TK_TN] = {}, tlen[TK_TN] = {};
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            const int t = nw / 32 + c;
            TkTile tl{0, 0, 0, 0};
            if (t < t_end) tl = tiles[t];
            trow[c] = __builtin_amdgcn_readfirstlane(tl.row);
            tlen[c] = __builtin_amdgcn_readfirstlane(tl.len);
        }
        float bv[BIAS ? TK_TN : 1] = {};          // BIAS: loaded here so that the MFMA loop hides the latency, added after it
        if constexpr (BIAS) {
            if (nw < n_end) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) bv[c] = bias[min(trow[c] + r, N - 1)];
            }
        }
        if (nw < n_end && tlen[0] + tlen[1] > 0) {
            const float* srow[8];           // rows this lane stages: 8j + lane / 8
#pragma unroll
            for (int j = 0; j < 8; ++j) srow[j] = items + (long)min(trow[j >> 2] + 8 * (j & 3) + (lane >> 3), N - 1) * d + 4 * (lane & 7);
#define TKS_GLOAD(m)                                                                                                       \
    do {                                                                                                               \
        const int k0_ = 32 * (m);                                                                                      \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                                \
            if (VEC) {                                                                                                 \
                const float4 v_ = *reinterpret_cast<const float4*>(srow[j] + k0_);                                     \
                g[j][0] = v_.x; g[j][1] = v_.y; g[j][2] = v_.z; g[j][3] = v_.w;                                        \
            } else {                                                                                                   \
                _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) g[j][e_] = srow[j][k0_ + e_];                         \
            }                                                                                                          \
        }                                                                                                              \
        _Pragma("unroll") for (int t = 0; t < 16; ++t) a[t] = arow[k0_ + 16 * h + t];                                  \
    } while (0)
            if (m_full > 0) {
                float g[8][4];
                float a[16];
                TKS_GLOAD(0);
                for (int m = 0; m < m_full; ++m) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        *reinterpret_cast<float4*>(st + (8 * j + (lane >> 3)) * TK_BP + 4 * (lane & 7)) =
                            make_float4(g[j][0], g[j][1], g[j][2], g[j][3]);
                    tk_wave_sync();
                    float b[TK_TN][16];
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c)
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const float4 v = *reinterpret_cast<const float4*>(st + (32 * c + r) * TK_BP + 16 * h + 4 * t);
                            b[c][4 * t] = v.x; b[c][4 * t + 1] = v.y; b[c][4 * t + 2] = v.z; b[c][4 * t + 3] = v.w;
                        }
                    float acur[16];
#pragma unroll
                    for (int t = 0; t < 16; ++t) acur[t] = a[t];
                    if (m + 1 < m_full) TKS_GLOAD(m + 1);
#pragma unroll
                    for (int t = 0; t < 16; ++t)
#pragma unroll
                        for (int c = 0; c < TK_TN; ++c)
                            acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(acur[t], b[c][t], acc[c], 0, 0, 0);
                    tk_wave_sync();        // this block's LDS reads stay ahead of the next block's writes
                }
            }
#undef TKS_GLOAD
            for (int g8 = 4 * m_full; 8 * g8 < d; ++g8) {       // zero-padded groups of 8 past the last whole block
                const int k0 = 8 * g8 + 4 * h;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float at = tk_ld(arow, k0 + t, d);
#pragma unroll
                    for (int c = 0; c < TK_TN; ++c) {
                        const float* brow = items + (long)min(trow[c] + r, N - 1) * d;
                        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(at, tk_ld(brow, k0 + t, d), acc[c], 0, 0, 0);
                    }
                }
            }
        }
        if constexpr (BIAS) {
            if (nw < n_end) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[c][q] = acc[c][q] + bv[c];
            }
        }
        // filter.  C/D layout: item = lane & 31 of the column tile, user row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5).
        // Bit 16 c + q of `pend`: that score still has to be offered.
        uint32_t pend = 0;
        uint32_t gid[TK_TN] = {};           // the id of this lane's item in column tile c
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) {
            const bool live = nw + 32 * c + r < n_end && r < tlen[c];
            if (live) gid[c] = (uint32_t)item_ids[trow[c] + r];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int b = u0 + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (live && b < B && !__builtin_isnan(acc[c][q])) pend |= 1u << (16 * c + q);
            }
        }
        bool first = true;
        while (__syncthreads_or(pend != 0)) {
            if (!first) {
                // sort every full buffer down to its best k (cnt may have run past P: those candidates are pending)
                for (int i = wave; i < TK_UT; i += W) {
                    if (cnt[i] >= P) {
                        int c = P;
                        const uint64_t t = flush(i, c);
                        if (lane == 0) {
                            thr[i] = t;
                            cnt[i] = c;
                        }
                    }
                }
                __syncthreads();
            }
            first = false;
#pragma unroll
            for (int c = 0; c < TK_TN; ++c) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint32_t bit = 1u << (16 * c + q);
                    if (!(pend & bit)) continue;
                    const int i = (q & 3) + 8 * (q >> 2) + 4 * h;
                    const uint64_t e = tk_entry(acc[c][q], gid[c]);
                    bool keep = false;
                    if (e > thr[i]) {
                        const int slot = atomicAdd(&cnt[i], 1);
                        if (slot < P) buf[i][slot] = e;
                        else keep = true;
                    }
                    if (!keep) pend &= ~bit;
                }
            }
        }
    }
    for (int i = wave; i < TK_UT; i += W) {
        const int b = u0 + i;
        if (b >= B) break;
        int c = min(cnt[i], P);
        flush(i, c);
        uint64_t* dst = ws + ((long)b * S + slice) * k;          // the slice's best k, unsorted, 0-padded
        for (int j = lane; j < k; j += 64) dst[j] = j < c ? buf[i][j] : 0;
    }
}

// One wave per (user, section): the best k of the k-lists of the section's slices, sorted at the end (topk_merge_kernel with
// the source range of block b * G + g taken from slice_of_section).  Needs P >= k + 64.
template <int P>
__global__ __launch_bounds__(64) void topksec_merge_kernel(int G, int k, int S, const int* __restrict__ slice_of_section,
                                                           const uint64_t* __restrict__ ws, float* __restrict__ top_scores,
                                                           int64_t* __restrict__ top_ids) {
    __shared__ uint64_t buf[P];
    const int lane = threadIdx.x;
    const int b = blockIdx.x / G, g = blockIdx.x - b * G;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int s0 = slice_of_section[g], s1 = slice_of_section[g + 1];
    const uint64_t* src = ws + ((long)b * S + s0) * k;
    const long total = (long)max(0, s1 - s0) * k;
    int cnt = 0;
    uint64_t thr = 0;
    for (long c0 = 0; c0 < total; c0 += 64) {
        const long c = c0 + lane;
        const uint64_t e = c < total ? src[c] : 0;
        const bool take = e > thr;
        const unsigned long long m = __ballot(take);
        if (take) buf[cnt + __popcll(m & below)] = e;
        cnt += __popcll(m);
        if (cnt + 64 > P) {
            tk_wave_sync();
            thr = tk_select<P>(buf, cnt, k, lane);
        }
    }
    tk_wave_sync();
    tk_flush<P>(buf, cnt, k, lane);
    for (int j = lane; j < k; j += 64) {
        const uint64_t e = buf[j];
        top_scores[(long)blockIdx.x * k + j] = e ? tk_entry_score(e) : -__builtin_huge_valf();
        top_ids[(long)blockIdx.x * k + j] = e ? tk_entry_id(e) : -1;
    }
}

// The sizes of one call, all from bounds the host knows.
struct TopksecGeom {
    int64_t nt;         // tile bound
    int L, S_max;       // tiles per slice, slice bound
    bool ok;
    size_t tile_bytes, slice_bytes, ptr_bytes, entry_bytes;
};

static size_t topksec_round(size_t n) { return (n + 255) / 256 * 256; }

static TopksecGeom topksec_geom(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G, int32_t slice_tiles) {
    TopksecGeom g{};
    if (!topk_args_ok(B, N, d, k) || G < 1 || G > TKS_MAX_G || N + 32 * (int64_t)G > TK_MAX_N ||
        (int64_t)B * G * k > 0x7FFFFFFF || slice_tiles < 0 || slice_tiles > TKS_MAX_SLICE_TILES)
        return g;
    g.nt = N == 0 ? 0 : (N + 31 * (int64_t)G) / 32;
    g.L = slice_tiles ? slice_tiles : std::max(1, topk_geom(std::max(B, 1), 32 * g.nt).slice_len / 32);
    const int64_t s = (g.nt + g.L - 1) / g.L + G;
    if (s > TKS_MAX_SLICES) return g;
    g.S_max = (int)s;
    g.ok = true;
    g.tile_bytes = topksec_round((size_t)g.nt * sizeof(TkTile));
    g.slice_bytes = topksec_round((size_t)g.S_max * sizeof(TkSlice));
    g.ptr_bytes = topksec_round((size_t)(G + 1) * sizeof(int));
    g.entry_bytes = (size_t)B * (size_t)g.S_max * (size_t)k * sizeof(uint64_t);
    return g;
}

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_topk_sections_dot_workspace_bytes(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G,
                                                         int32_t slice_tiles) {
    const TopksecGeom g = topksec_geom(B, N, d, k, G, slice_tiles);
    if (!g.ok) return 0;
    return 256 + g.tile_bytes + g.slice_bytes + g.ptr_bytes + g.entry_bytes;     // never 0 for accepted arguments
}

extern "C" int nrms_topk_sections_dot(int32_t B, int64_t N, int32_t d, int32_t k, int32_t G, int32_t slice_tiles,
                                      const float* user, const float* items, const int32_t* item_ids, const int64_t* section_ptr,
                                      const float* bias, const int64_t* exclude, int32_t n_exclude, float* top_scores,
                                      int64_t* top_ids, void* workspace, size_t workspace_bytes, void* stream) {
    NRMS_REQUIRE(B >= 0, "topk_sections_dot: B must be >= 0 (B=%d)", B);
    NRMS_REQUIRE(G >= 1 && G <= TKS_MAX_G, "topk_sections_dot: G must be in [1, %d] (G=%d)", TKS_MAX_G, G);
    NRMS_REQUIRE(N >= 0 && N + 32 * (int64_t)G <= TK_MAX_N, "topk_sections_dot: N must be in [0, %d - 32 G] (N=%lld, G=%d)",
                 TK_MAX_N, (long long)N, G);
    NRMS_REQUIRE(d >= 1, "topk_sections_dot: d must be >= 1 (d=%d)", d);
    NRMS_REQUIRE(k >= 1 && k <= TK_MAX_K, "topk_sections_dot: k must be in [1, %d] (k=%d)", TK_MAX_K, k);
    NRMS_REQUIRE((int64_t)B * G * k <= 0x7FFFFFFF, "topk_sections_dot: B * G * k must be <= 2^31 - 1 (B=%d, G=%d, k=%d)", B, G, k);
    NRMS_REQUIRE(slice_tiles >= 0 && slice_tiles <= TKS_MAX_SLICE_TILES,
                 "topk_sections_dot: slice_tiles must be 0 or in [1, %d] (slice_tiles=%d)", TKS_MAX_SLICE_TILES, slice_tiles);
    NRMS_REQUIRE(n_exclude >= 0, "topk_sections_dot: n_exclude must be >= 0 (n_exclude=%d)", n_exclude);
    const TopksecGeom g = topksec_geom(B, N, d, k, G, slice_tiles);
    NRMS_REQUIRE(g.ok, "topk_sections_dot: slice_tiles too small for N: more than %d slices (N=%lld, G=%d, slice_tiles=%d)",
                 TKS_MAX_SLICES, (long long)N, G, slice_tiles);
    if (B == 0) return NRMS_OK;
    NRMS_REQUIRE(user, "topk_sections_dot: user is null");
    NRMS_REQUIRE(items || N == 0, "topk_sections_dot: items is null");
    NRMS_REQUIRE(item_ids || N == 0, "topk_sections_dot: item_ids is null");
    NRMS_REQUIRE(section_ptr || N == 0, "topk_sections_dot: section_ptr is null");
    NRMS_REQUIRE(((uintptr_t)bias & 3) == 0, "topk_sections_dot: bias must be 4-byte aligned");
    NRMS_REQUIRE(top_scores, "topk_sections_dot: top_scores is null");
    NRMS_REQUIRE(top_ids, "topk_sections_dot: top_ids is null");
    NRMS_REQUIRE(workspace, "topk_sections_dot: workspace is null");
    const size_t need = nrms_topk_sections_dot_workspace_bytes(B, N, d, k, G, slice_tiles);
    if (workspace_bytes < need) {
        set_error("topk_sections_dot: workspace %zu < required %zu bytes", workspace_bytes, need);
        return NRMS_EWORKSPACE;
    }
    NRMS_REQUIRE(((uintptr_t)workspace & 15) == 0, "topk_sections_dot: workspace must be 16-byte aligned");
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts("topk_sections_dot", s);
    char* p = (char*)workspace;
    TkTile* tiles = (TkTile*)p;
    TkSlice* slices = (TkSlice*)(p + g.tile_bytes);
    int* slice_of_section = (int*)(p + g.tile_bytes + g.slice_bytes);
    uint64_t* ws = (uint64_t*)(p + g.tile_bytes + g.slice_bytes + g.ptr_bytes);
    const int n = (int)N;
    hipLaunchKernelGGL(topksec_tables_kernel, dim3(1), dim3(1024), 0, s, n, G, (int)g.nt, g.L, g.S_max, section_ptr, tiles, slices,
                       slice_of_section);
    int rc = check_launch("topk_sections_dot(tables)");
    if (rc != NRMS_OK) return rc;
    if (g.nt > 0) {
        const bool vec = (d & 3) == 0 && ((uintptr_t)user & 15) == 0 && ((uintptr_t)items & 15) == 0;
        const dim3 grid(cdiv(B, TK_UT), g.S_max);
#define TKS_LAUNCH_G(P, W, V, BI)                                                                                          \
    hipLaunchKernelGGL((topksec_slice_kernel<P, W, V, BI>), grid, dim3(64 * W), 0, s, B, n, d, k, g.S_max, user, items, exclude, \
                       n_exclude, ws, slices, tiles, item_ids, bias)
#define TKS_LAUNCH(P, W)                                                                                                   \
    do {                                                                                                                   \
        if (bias) {                                                                                                        \
            if (vec) TKS_LAUNCH_G(P, W, true, true);                                                                       \
            else TKS_LAUNCH_G(P, W, false, true);                                                                          \
        } else {                                                                                                           \
            if (vec) TKS_LAUNCH_G(P, W, true, false);                                                                      \
            else TKS_LAUNCH_G(P, W, false, false);                                                                         \
        }                                                                                                                  \
    } while (0)
        if (k + 64 <= 128) TKS_LAUNCH(128, TK_WAVES);
        else if (k + 64 <= 256) TKS_LAUNCH(256, TK_WAVES);
        else TKS_LAUNCH(512, 2);
#undef TKS_LAUNCH
#undef TKS_LAUNCH_G
        rc = check_launch("topk_sections_dot(slices)");
        if (rc != NRMS_OK) return rc;
    }
    const dim3 mgrid((unsigned)((int64_t)B * G));
    if (k + 64 <= 128) hipLaunchKernelGGL(topksec_merge_kernel<128>, mgrid, dim3(64), 0, s, G, k, g.S_max, slice_of_section, ws, top_scores, top_ids);
    else if (k + 64 <= 256) hipLaunchKernelGGL(topksec_merge_kernel<256>, mgrid, dim3(64), 0, s, G, k, g.S_max, slice_of_section, ws, top_scores, top_ids);
    else hipLaunchKernelGGL(topksec_merge_kernel<512>, mgrid, dim3(64), 0, s, G, k, g.S_max, slice_of_section, ws, top_scores, top_ids);
    return check_launch("topk_sections_dot(merge)");
}
