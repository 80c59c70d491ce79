// Neighbour sampling from a device-resident click graph (include/nrms_hip.h, "Click graph"; model/graph_hip.py; SURVEY section 8
// row f-4, PARITY UNPINNED: the reference has no graph model).
//
//   nrms_graph_sample_neighbors: one lane per draw (slot r, draw t), the K draws of a slot on consecutive lanes, so the int32
//       results of a wavefront are one contiguous 256-byte store.  A draw is a chain of dependent gathers (slot id -> news_ptr
//       pair -> news_users -> user_ptr pair -> user_news: three gathers into the graph behind the slot's own id) with no arithmetic
//       to speak of between them: the Philox call does not depend on any load and is issued in front of the chain, the kernel
//       keeps no state between draws and needs under 20 VGPRs (hipcc's resource report: 18; the dispatch record: 12), so
//       a SIMD holds its eight waves and the chain's latency (L2 / Infinity Cache hits: MIND's graph is a few MB) is hidden by
//       other waves, not by unrolling.  No grid-stride loop: a draw's wave retires as soon as its chain ends.
//   nrms_graph_resolve_rows: neighbour news ids -> rows of the batch's numbering, through two tables over the news ids in the
//       caller's workspace: first[j] = the smallest slot that shows news j (integer atomicMin: order-independent) and a bitmap of
//       the out-of-batch neighbour ids (atomicOr), whose prefix popcount is an id's rank in ascending order.  Every output is a
//       pure function of the inputs: two calls give the same bytes.
#include "common.h"

namespace nrms {

constexpr int GS_BLOCK = 256;
constexpr int GS_NONE = 0x7f7f7f7f;          // first[]: "no slot shows this news" (what hipMemsetAsync(0x7f) leaves)

struct GraphArgs {
    long n_users, n_news, n_edges;
    const int64_t* user_ptr; const int32_t* user_news; const int64_t* news_ptr; const int32_t* news_users;
};

__global__ __launch_bounds__(GS_BLOCK) void graph_sample_kernel(GraphArgs g, long n_draws, int K, const int64_t* __restrict__ slot_ids,
                                                                uint64_t seed, int32_t* __restrict__ out, int* n_bad) {
    const long i = (long)blockIdx.x * GS_BLOCK + threadIdx.x;
    int bad = 0;
    if (i < n_draws) {
        const long r = i / K;
        const int t = (int)(i - r * K);
        const int64_t j = slot_ids[r];
        int32_t res = -1;
        if (j < 0 || j >= g.n_news) bad = t == 0 ? 1 : 0;          // counted once per slot
        else if (j > 0) {
            uint32_t rnd[4];
            philox4x32_7(seed, (uint64_t)j * (uint64_t)K + (uint64_t)t, PHILOX_SITE_GRAPH_SAMPLE, rnd);
            const int64_t p0 = g.news_ptr[j], p1 = g.news_ptr[j + 1];
            const uint64_t deg = (uint64_t)(p1 - p0);
            // (a well-formed graph passes every range test below; they keep a damaged one from indexing out of bounds)
            if (p0 >= 0 && p1 > p0 && p1 <= g.n_edges && deg <= 0x7fffffffull) {
                const int32_t u = g.news_users[p0 + (int64_t)(((uint64_t)rnd[0] * deg) >> 32)];
                if (u >= 0 && u < g.n_users) {
                    const int64_t q0 = g.user_ptr[u], q1 = g.user_ptr[u + 1];
                    const uint64_t du = (uint64_t)(q1 - q0);
                    if (q0 >= 0 && q1 > q0 && q1 <= g.n_edges && du <= 0x7fffffffull) {
                        const int32_t m = g.user_news[q0 + (int64_t)(((uint64_t)rnd[1] * du) >> 32)];
                        res = (m == (int32_t)j || m <= 0 || m >= g.n_news) ? -1 : m;
                    }
                }
            }
        }
        out[i] = res;
    }
    if (__ballot(bad != 0) != 0ull) {                      // rare path, as sanitize_ids_kernel
        bad = (int)wave_sum((float)bad);
        if ((threadIdx.x & 63) == 0) atomicAdd(n_bad, bad);
    }
}

__global__ __launch_bounds__(GS_BLOCK) void graph_first_row_kernel(long n_slots, long n_news, const int64_t* __restrict__ slot_ids, int* first) {
    const long r = (long)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (r >= n_slots) return;
    const int64_t j = slot_ids[r];
    // a popular news fills hundreds of slots: only a slot below the value it can see goes to the atomic (the value only ever
    // falls, so a stale read costs an atomic that changes nothing, never a wrong minimum)
    if (j > 0 && j < n_news && first[j] > (int)r) atomicMin(&first[j], (int)r);
}

__global__ __launch_bounds__(GS_BLOCK) void graph_mark_kernel(long n_draws, long n_news, const int32_t* __restrict__ nbr, const int* __restrict__ first,
                                                              unsigned* bits) {
    const long i = (long)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (i >= n_draws) return;
    const int32_t m = nbr[i];
    if (m > 0 && m < n_news && first[m] == GS_NONE && (bits[m >> 5] & (1u << (m & 31))) == 0u)      // (bits are only ever set: as above)
        atomicOr(&bits[m >> 5], 1u << (m & 31));
}

// prefix[w] = number of marked ids below word w; one workgroup, every lane a contiguous run of words (4 words per lane at MIND's
// 130 000 news; sized for catalogues up to ~10^7 news, include/nrms_hip.h -- beyond that this pass wants a multi-block scan)
__global__ __launch_bounds__(1024) void graph_rank_kernel(long n_words, const unsigned* __restrict__ bits, int* __restrict__ prefix, int cap,
                                                          int* n_extra, int* n_dropped) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const long per = (n_words + 1023) / 1024;
    const long w0 = tid * per, w1 = w0 + per < n_words ? w0 + per : n_words;
    int sum = 0;
    for (long w = w0; w < w1; ++w) sum += __popc(bits[w]);
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                   // inclusive scan of the 1024 run sums
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (long w = w0; w < w1; ++w) {
        prefix[w] = run;
        run += __popc(bits[w]);
    }
    if (tid == 1023) {
        const int total = part[1023];
        *n_extra = total < cap ? total : cap;
        if (total > cap) *n_dropped += total - cap;        // one writer per call; calls on one stream are ordered
    }
}

__global__ __launch_bounds__(GS_BLOCK) void graph_emit_kernel(long n_words, const unsigned* __restrict__ bits, const int* __restrict__ prefix, int cap,
                                                              int32_t* extra_ids) {
    const long w = (long)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (w >= n_words) return;
    unsigned b = bits[w];
    int e = prefix[w];
    while (b != 0u && e < cap) {
        const int bit = __ffs(b) - 1;
        extra_ids[e++] = (int32_t)(w * 32 + bit);
        b &= b - 1u;
    }
}

__global__ __launch_bounds__(GS_BLOCK) void graph_rows_kernel(long n_slots, long n_draws, long n_news, const int32_t* __restrict__ nbr,
                                                              const int* __restrict__ first, const unsigned* __restrict__ bits,
                                                              const int* __restrict__ prefix, int cap, int64_t* __restrict__ rows) {
    const long i = (long)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (i >= n_draws) return;
    const int32_t m = nbr[i];
    int64_t row = -1;
    if (m > 0 && m < n_news) {
        const int f = first[m];
        if (f != GS_NONE) row = f;
        else {
            const int e = prefix[m >> 5] + __popc(bits[m >> 5] & ((1u << (m & 31)) - 1u));
            row = e < cap ? n_slots + e : -1;
        }
    }
    rows[i] = row;
}

struct ResolveLayout { size_t first, bits, prefix, total; long n_words; };
static ResolveLayout resolve_layout(long n_news) {
    ResolveLayout L{};
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.n_words = (n_news + 31) / 32;
    L.first = 0;
    L.bits = up((size_t)n_news * sizeof(int));
    L.prefix = L.bits + up((size_t)L.n_words * sizeof(unsigned));
    L.total = L.prefix + up((size_t)L.n_words * sizeof(int));
    return L;
}

}  // namespace nrms

using namespace nrms;

// n_slots is bounded before the product is formed, and stays below GS_NONE so that no slot index reads as "no slot"
static bool sample_shape_ok(int64_t n_slots, int32_t K) {
    return n_slots >= 0 && n_slots < (int64_t)GS_NONE && K >= 1 && K <= 64 && n_slots * (long)K < (1L << 31);
}

extern "C" size_t nrms_graph_sample_workspace_bytes(int64_t n_slots, int32_t K) {
    if (!sample_shape_ok(n_slots, K)) set_error("graph_sample_workspace_bytes: n_slots=%ld K=%d", (long)n_slots, K);
    return 0;                                    // the draws keep no state outside their lanes
}

extern "C" int nrms_graph_sample_neighbors(const nrms_click_graph* graph, int64_t n_slots, int32_t K, const int64_t* slot_ids, uint64_t seed,
                                           int32_t* neighbor_ids, int32_t* n_bad, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    NRMS_REQUIRE(graph != nullptr, "graph_sample_neighbors: null graph");
    NRMS_REQUIRE(sample_shape_ok(n_slots, K), "graph_sample_neighbors: n_slots=%ld K=%d (K in [1, 64], n_slots < 0x7f7f7f7f, n_slots * K < 2^31)", (long)n_slots, K);
    NRMS_REQUIRE(graph->n_news >= 1 && graph->n_news < (1L << 31) && graph->n_users >= 0 && graph->n_users < (1L << 31) && graph->n_edges >= 0,
                 "graph_sample_neighbors: n_news=%ld n_users=%ld n_edges=%ld", (long)graph->n_news, (long)graph->n_users, (long)graph->n_edges);
    NRMS_REQUIRE(graph->user_ptr && graph->news_ptr && (graph->n_edges == 0 || (graph->user_news && graph->news_users)),
                 "graph_sample_neighbors: null graph array");
    if (n_slots == 0) return NRMS_OK;
    NRMS_REQUIRE(slot_ids && neighbor_ids && n_bad, "graph_sample_neighbors: null argument");
    GraphArgs g{(long)graph->n_users, (long)graph->n_news, (long)graph->n_edges, graph->user_ptr, graph->user_news, graph->news_ptr, graph->news_users};
    const long n_draws = (long)n_slots * K;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts("graph_sample", s);
    hipLaunchKernelGGL(graph_sample_kernel, dim3(cdiv(n_draws, GS_BLOCK)), dim3(GS_BLOCK), 0, s, g, n_draws, (int)K, slot_ids, seed, neighbor_ids, n_bad);
    return check_launch("graph_sample");
}

extern "C" size_t nrms_graph_resolve_workspace_bytes(int64_t n_news) {
    if (n_news < 1 || n_news >= (1L << 31)) {
        set_error("graph_resolve_workspace_bytes: n_news=%ld", (long)n_news);
        return 0;
    }
    return resolve_layout((long)n_news).total;
}

extern "C" int nrms_graph_resolve_rows(int64_t n_slots, int32_t K, int64_t n_news, const int64_t* slot_ids, const int32_t* neighbor_ids, int32_t cap,
                                       int64_t* neighbor_rows, int32_t* extra_ids, int32_t* n_extra, int32_t* n_dropped, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    NRMS_REQUIRE(sample_shape_ok(n_slots, K), "graph_resolve_rows: n_slots=%ld K=%d (K in [1, 64], n_slots < 0x7f7f7f7f, n_slots * K < 2^31)", (long)n_slots, K);
    NRMS_REQUIRE(n_news >= 1 && n_news < (1L << 31), "graph_resolve_rows: n_news=%ld", (long)n_news);
    NRMS_REQUIRE(cap >= 0 && n_slots + (long)cap < (1L << 31), "graph_resolve_rows: cap=%d", cap);
    NRMS_REQUIRE(n_extra && n_dropped && (cap == 0 || extra_ids), "graph_resolve_rows: null argument");
    NRMS_REQUIRE(n_slots == 0 || (slot_ids && neighbor_ids && neighbor_rows), "graph_resolve_rows: null argument");
    const ResolveLayout L = resolve_layout((long)n_news);
    NRMS_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 3) == 0, "graph_resolve_rows: workspace must be 4-byte aligned");
    if (workspace_bytes < L.total) {
        set_error("graph_resolve_rows: workspace %zu < required %zu bytes", workspace_bytes, L.total);
        return NRMS_EWORKSPACE;
    }
    char* base = (char*)workspace;
    int* first = (int*)(base + L.first);
    unsigned* bits = (unsigned*)(base + L.bits);
    int* prefix = (int*)(base + L.prefix);
    const long n_draws = (long)n_slots * K;
    hipStream_t s = (hipStream_t)stream;
    TimingScope ts("graph_resolve", s);
    if (hipMemsetAsync(first, 0x7f, (size_t)n_news * sizeof(int), s) != hipSuccess || hipMemsetAsync(bits, 0, (size_t)L.n_words * sizeof(unsigned), s) != hipSuccess
        || (cap > 0 && hipMemsetAsync(extra_ids, 0, (size_t)cap * sizeof(int32_t), s) != hipSuccess)) {
        set_error("graph_resolve_rows: hipMemsetAsync failed");
        return NRMS_ELAUNCH;
    }
    if (n_slots > 0) {
        hipLaunchKernelGGL(graph_first_row_kernel, dim3(cdiv(n_slots, GS_BLOCK)), dim3(GS_BLOCK), 0, s, (long)n_slots, (long)n_news, slot_ids, first);
        hipLaunchKernelGGL(graph_mark_kernel, dim3(cdiv(n_draws, GS_BLOCK)), dim3(GS_BLOCK), 0, s, n_draws, (long)n_news, neighbor_ids, (const int*)first, bits);
    }
    hipLaunchKernelGGL(graph_rank_kernel, dim3(1), dim3(1024), 0, s, L.n_words, (const unsigned*)bits, prefix, (int)cap, n_extra, n_dropped);
    if (n_slots > 0) {
        if (cap > 0)
            hipLaunchKernelGGL(graph_emit_kernel, dim3(cdiv(L.n_words, GS_BLOCK)), dim3(GS_BLOCK), 0, s, L.n_words, (const unsigned*)bits, (const int*)prefix,
                               (int)cap, extra_ids);
        hipLaunchKernelGGL(graph_rows_kernel, dim3(cdiv(n_draws, GS_BLOCK)), dim3(GS_BLOCK), 0, s, (long)n_slots, n_draws, (long)n_news, neighbor_ids,
                           (const int*)first, (const unsigned*)bits, (const int*)prefix, (int)cap, neighbor_rows);
    }
    return check_launch("graph_resolve");
}
