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
// Kernel 2 (topksec_slice_kernel): grid = 32-user tiles x S_max.  The pieces of topk_slice_kernel (topk_kernels.h: tk_chain,
//   TkWaveTiles, TkFilter) with the block's range taken from its slice-table entry (an empty entry exits without writing) and
//   ONE A operand, the user's own row, for both column tiles: nrms_topk_dot's scores, bit for bit, and 32 VGPRs fewer than
//   the grouped kernel's two operands (profiles/topk_sections_resource_usage.txt).  BIAS adds bias[row] to the finished accumulator, as nrms_topk_dot_biased does.
// Kernel 3 (topksec_merge_kernel): one wave per (user, section): tk_merge over the k-lists of the section's slices.
//
// The slice kernel is a __global__ of its own, not a mode of topk_slice_kernel: what differs (where the block's range comes
// from, the early exit, the bias by row) is its frame, and everything inside the frame is the shared code.
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
    long st = 0, ss = 0;
    for (int g = lo; g < hi; ++g) {
        int row, len;
        tk_group_span(section_ptr, g, N, row, len);
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
        tk_group_span(section_ptr, g, N, row, len);
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

// topk_slice_kernel (topk_kernels.h) for one slice-table entry per block: users [u0, u0 + 32) x the tiles [t0, t1) of one
// section, 2 W tiles per step.  Rows past a tile's len are masked, the id of row n is item_ids[n], and both column tiles take
// the user's own row as A operand.
template <int P, int W, bool VEC, bool BIAS>
__global__ __launch_bounds__(64 * W) void topksec_slice_kernel(int B, int N, int d, int k, int S,
                                                               const float* __restrict__ user, const float* __restrict__ items,
                                                               const int64_t* __restrict__ exclude, int n_exclude,
                                                               uint64_t* __restrict__ ws, const TkSlice* __restrict__ slices,
                                                               const TkTile* __restrict__ tiles,
                                                               const int32_t* __restrict__ item_ids,
                                                               const float* __restrict__ bias) {
    TK_FILTER_LDS(lds, P);
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
    TkFilter<P, W> flt{lds, exclude, n_exclude, k, u0, B, lane, wave};
    flt.start(0, 0x80000000L);
    __syncthreads();

    const int r = lane & 31;
    const float* arow[1] = {user + (long)min(u0 + r, B - 1) * d};
    float* st = stage[wave];
    for (int n0 = n_begin; n0 < n_end; n0 += IT) {
        const int nw = n0 + 64 * wave;
        tk_f32x16 acc[TK_TN];
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) acc[c] = tk_f32x16{};
        const TkWaveTiles tl(tiles, t_end, nw);
        float bv[BIAS ? TK_TN : 1] = {};          // BIAS: loaded here so that the chain hides the latency, added after it
        if constexpr (BIAS) {
            if (nw < n_end) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c) bv[c] = bias[min(tl.row[c] + r, N - 1)];
            }
        }
        if (nw < n_end && tl.len[0] + tl.len[1] > 0) tk_chain<VEC>(acc, arow, items, d, st, lane, [&](int i) { return tl.row_of(i, N); });
        if constexpr (BIAS) {
            if (nw < n_end) {
#pragma unroll
                for (int c = 0; c < TK_TN; ++c)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[c][q] = acc[c][q] + bv[c];
            }
        }
        bool live[TK_TN];
        uint32_t id[TK_TN] = {};            // the id of this lane's item in column tile c
#pragma unroll
        for (int c = 0; c < TK_TN; ++c) live[c] = tl.live(c, nw, n_end, r, item_ids, id[c]);
        // unconditional: the offer holds the block's barriers, and a wave with nothing to offer has to meet them too
        flt.offer(acc, flt.pending(acc, live, TkOpenAll{}), [&](int c) { return id[c]; });
    }
    flt.write(ws, S, slice);
}

// One wave per (user, section), block b * G + g: the best k of the k-lists of the section's slices
// [slice_of_section[g], slice_of_section[g + 1]).
template <int P>
__global__ __launch_bounds__(64) void topksec_merge_kernel(int G, int k, int S, const int* __restrict__ slice_of_section,
                                                           const uint64_t* __restrict__ ws, float* __restrict__ top_scores,
                                                           int64_t* __restrict__ top_ids) {
    __shared__ uint64_t buf[P];
    const int b = blockIdx.x / G, g = blockIdx.x - b * G;
    const int s0 = slice_of_section[g], s1 = slice_of_section[g + 1];
    tk_merge<P>(buf, ws + ((long)b * S + s0) * k, (long)max(0, s1 - s0) * k, k, threadIdx.x, top_scores + (long)blockIdx.x * k,
                top_ids + (long)blockIdx.x * k);
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
    const char* who = "topk_sections_dot";
    NRMS_REQUIRE(G >= 1 && G <= TKS_MAX_G, "%s: G must be in [1, %d] (G=%d)", who, TKS_MAX_G, G);
    int rc = tk_check_dims(who, B, N, TK_MAX_N - 32 * (int64_t)G, d, "k", k, TK_MAX_K, n_exclude);
    if (rc != NRMS_OK) return rc;
    NRMS_REQUIRE((int64_t)B * G * k <= 0x7FFFFFFF, "%s: B * G * k must be <= 2^31 - 1 (B=%d, G=%d, k=%d)", who, B, G, k);
    NRMS_REQUIRE(slice_tiles >= 0 && slice_tiles <= TKS_MAX_SLICE_TILES, "%s: slice_tiles must be 0 or in [1, %d] (slice_tiles=%d)", who,
                 TKS_MAX_SLICE_TILES, slice_tiles);
    const TopksecGeom g = topksec_geom(B, N, d, k, G, slice_tiles);
    NRMS_REQUIRE(g.ok, "%s: slice_tiles too small for N: more than %d slices (N=%lld, G=%d, slice_tiles=%d)", who, TKS_MAX_SLICES,
                 (long long)N, G, slice_tiles);
    if (B == 0) return NRMS_OK;
    rc = tk_check_ptrs(who, {{"user", user, true, 1}, {"items", items, N != 0, 1}, {"item_ids", item_ids, N != 0, 1},
                             {"section_ptr", section_ptr, N != 0, 1}, {"bias", bias, false, 4}, {"top_scores", top_scores, true, 1},
                             {"top_ids", top_ids, true, 1}},
                       workspace, workspace_bytes, nrms_topk_sections_dot_workspace_bytes(B, N, d, k, G, slice_tiles), 16);
    if (rc != NRMS_OK) return rc;
    if (!exclude) n_exclude = 0;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts(who, s);
    char* p = (char*)workspace;
    TkTile* tiles = (TkTile*)p;
    TkSlice* slices = (TkSlice*)(p + g.tile_bytes);
    int* slice_of_section = (int*)(p + g.tile_bytes + g.slice_bytes);
    uint64_t* ws = (uint64_t*)(p + g.tile_bytes + g.slice_bytes + g.ptr_bytes);
    const int n = (int)N;
    hipLaunchKernelGGL(topksec_tables_kernel, dim3(1), dim3(1024), 0, s, n, G, (int)g.nt, g.L, g.S_max, section_ptr, tiles, slices,
                       slice_of_section);
    rc = check_launch("topk_sections_dot(tables)");
    if (rc != NRMS_OK) return rc;
    tk_with_pw(k, [&](auto P, auto W) {
        constexpr int pp = decltype(P)::value, w = decltype(W)::value;
        if (g.nt > 0) {
            tk_with_flags([&](auto V, auto BI) {
                hipLaunchKernelGGL((topksec_slice_kernel<pp, w, decltype(V)::value, decltype(BI)::value>), dim3(cdiv(B, TK_UT), g.S_max),
                                   dim3(64 * w), 0, s, B, n, d, k, g.S_max, user, items, exclude, n_exclude, ws, slices, tiles, item_ids,
                                   bias);
            }, tk_vec_ok(d, user, items), bias != nullptr);
            rc = check_launch("topk_sections_dot(slices)");
            if (rc != NRMS_OK) return;
        }
        hipLaunchKernelGGL(topksec_merge_kernel<pp>, dim3((unsigned)((int64_t)B * G)), dim3(64), 0, s, G, k, g.S_max, slice_of_section,
                           ws, top_scores, top_ids);
        rc = check_launch("topk_sections_dot(merge)");
    });
    return rc;
}
