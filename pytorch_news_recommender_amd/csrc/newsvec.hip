// nrms_bert's news-vector layer (model/nrms.py:216-256 of the reference: BertNewsEncoder): each news slot of a batch looks
// up its pretrained row and goes through one Linear, then dropout.  The batch's DISTINCT ids go through the Linear once:
//
//   forward   ids -> validated keys -> stable radix sort of (id, slot) -> groups in ascending id order (uid, seg_start,
//             slot_u) -> Y[U, E] = table[uid] W^T + b (NT GEMM, a_rows = uid, device row count) -> out[slot] =
//             dropout(Y[slot_u[slot]]) (site NRMS_DROPOUT_SITE_NEWSVEC)
//   backward  dY[u] = sum over the group's slots, in a fixed order (spans of slots, then the spans), of dropout'(dout[slot])
//             (no atomics); X[u] = table[uid[u]];
//             d(W), d(b) += dY^T [X | 1] (TN GEMM, device row count); d(table)[uid[u]] = dY[u] W (NT GEMM, c_rows = uid)
//
// Popular news repeat across histories, and the dropout comes after the dense layer, so grouping is exact.
#include "gemm.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace nrms {

constexpr int NV_SCAN_THREADS = 1024;

// keys[i] = the slot's id as int32 (ids outside [0, n_rows) read as 0 and counted), vals[i] = i
__global__ __launch_bounds__(256) void nv_keys_kernel(long n, const int64_t* ids, int n_rows, int* keys, int* vals, int* n_bad) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (i < n) {
        const int64_t v = ids[i];
        const bool ok = v >= 0 && v < n_rows;
        keys[i] = ok ? (int)v : 0;
        vals[i] = (int)i;
        bad = ok ? 0 : 1;
    }
    // one integer atomic per wave that met a bad id
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && (threadIdx.x & 63) == __ffsll((long long)m) - 1 && n_bad != nullptr) atomicAdd(n_bad, (int)__popcll(m));
}

// One workgroup: group the sorted keys.  Thread t owns the contiguous chunk [t c, (t + 1) c); heads are counted per chunk,
// scanned in LDS, then every sorted position writes its group.  n_slots of a batch is a few ten thousand.
__global__ __launch_bounds__(NV_SCAN_THREADS) void nv_group_kernel(long n, const int* ks, const int* vs, int* n_unique, int* uid,
                                                                     int* seg_start, int* slot_u) {
    __shared__ int part[NV_SCAN_THREADS];
    const int t = threadIdx.x;
    const long c = (n + NV_SCAN_THREADS - 1) / NV_SCAN_THREADS;
    const long i0 = min(n, t * c), i1 = min(n, i0 + c);
    int cnt = 0;
    for (long i = i0; i < i1; ++i) cnt += (i == 0 || ks[i] != ks[i - 1]) ? 1 : 0;
    part[t] = cnt;
    __syncthreads();
    for (int o = 1; o < NV_SCAN_THREADS; o <<= 1) {          // Hillis-Steele inclusive scan
        const int v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int g = part[t] - cnt - 1;                               // group of the position before the chunk
    for (long i = i0; i < i1; ++i) {
        if (i == 0 || ks[i] != ks[i - 1]) {
            ++g;
            uid[g] = ks[i];
            seg_start[g] = (int)i;
        }
        slot_u[vs[i]] = g;
    }
    if (t == NV_SCAN_THREADS - 1) {
        *n_unique = part[t];
        seg_start[part[t]] = (int)n;
    }
}

// out[slot, :] = Y[slot_u[slot], :] x keep(slot, :) / (1 - p); one thread per 4 columns
__global__ __launch_bounds__(256) void nv_expand_kernel(long n, int d, const int* slot_u, const float* y, Dropout drop, float* out) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;     // group of 4 elements of out
    const int d4 = d >> 2;
    if (g >= n * d4) return;
    const long slot = g / d4;
    const int c = (int)(g - slot * d4) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(y + (long)slot_u[slot] * d + c);
    if (drop.thresh != 0u) v *= dropout_scale4(drop.seed, NRMS_DROPOUT_SITE_NEWSVEC, (uint64_t)g, drop.thresh, drop.inv_keep);
    *reinterpret_cast<f32x4*>(out + slot * d + c) = v;
}

// dY[u, :] = sum over the group's slots in slot order of dout[slot, :] x keep / (1 - p), and X[u, :] = table[uid[u], :].
// A group is a run of the sorted positions (padding id 0 alone can hold half of the history slots), so the sum is split
// into spans of NV_SPAN positions: one workgroup per span walks its positions in order (one thread per 4 columns, d <= 1024)
// and stores each run -- a group that lies inside the span straight into dY, the run of a group that crosses the span's
// edge into the span's partial slot 0 (the run starts at the span's first position) or 1 (it starts later).  nv_combine
// then adds a crossing group's partials span after span.  Fixed association, no atomics: bit-reproducible.
constexpr int NV_SPAN = 32;
__global__ __launch_bounds__(256) void nv_span_kernel(long n, int d, const int* seg_start, const int* slot_u, const int* uid,
                                                      const int* sorted_slot, const float* dout, const float* table, Dropout drop,
                                                      float* dy, float* x, float* part) {
    const long s = blockIdx.x;
    const long p0 = s * NV_SPAN, p1 = min(n, p0 + NV_SPAN);
    const int c = threadIdx.x * 4;
    if (c >= d) return;
    const int d4 = d >> 2;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    long r0 = p0;
    for (long i = p0; i < p1; ++i) {
        const long slot = sorted_slot[i];                    // ascending within a group: the radix sort is stable
        const int g = slot_u[slot];
        f32x4 v = *reinterpret_cast<const f32x4*>(dout + slot * d + c);
        if (drop.thresh != 0u)
            v *= dropout_scale4(drop.seed, NRMS_DROPOUT_SITE_NEWSVEC, (uint64_t)(slot * d4 + threadIdx.x), drop.thresh, drop.inv_keep);
        acc += v;
        const long a = seg_start[g], b = seg_start[g + 1];
        if (i == a)                                          // the group's first position: gather its table row once
            *reinterpret_cast<f32x4*>(x + (long)g * d + c) = *reinterpret_cast<const f32x4*>(table + (long)uid[g] * d + c);
        if (i + 1 == b || i + 1 == p1) {                     // the run ends: the group ends or the span does
            float* dst = (a >= p0 && b <= p1) ? dy + (long)g * d : part + (s * 2 + (r0 == p0 ? 0 : 1)) * d;
            *reinterpret_cast<f32x4*>(dst + c) = acc;
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
            r0 = i + 1;
        }
    }
}

// dY of the groups that cross a span edge: their partials in span order
__global__ __launch_bounds__(256) void nv_combine_kernel(int d, const int* n_unique, const int* seg_start, const float* part, float* dy) {
    const int u = blockIdx.x;
    if (u >= *n_unique) return;
    const long a = seg_start[u], b = seg_start[u + 1];
    const long s0 = a / NV_SPAN, s1 = (b - 1) / NV_SPAN;
    if (s0 == s1) return;
    const int c = threadIdx.x * 4;
    if (c >= d) return;
    f32x4 acc = *reinterpret_cast<const f32x4*>(part + (s0 * 2 + (a == s0 * NV_SPAN ? 0 : 1)) * d + c);
    for (long s = s0 + 1; s <= s1; ++s) acc += *reinterpret_cast<const f32x4*>(part + s * 2 * d + c);
    *reinterpret_cast<f32x4*>(dy + (long)u * d + c) = acc;
}

static size_t up256(size_t x) { return (x + 255) / 256 * 256; }
static int nv_key_bits(int n_rows) { int b = 1; while ((1L << b) < (long)n_rows) ++b; return b; }

// the saved area (written by the forward, read by the backward) and the workspace of both directions
struct NvSaved { size_t n_unique, uid, seg_start, slot_u, sorted_slot, total; };
struct NvWs { size_t keys, vals, keys2, sort_tmp, sort_tmp_bytes, y, x, part, wt, tn_partial, wplanes, total; };

static NvSaved nv_saved(const nrms_newsvec_desc* d) {
    NvSaved s;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = up256(off + bytes); return o; };
    const size_t n = (size_t)d->n_slots;
    s.n_unique = take(4);
    s.uid = take(n * 4);
    s.seg_start = take((n + 1) * 4);
    s.slot_u = take(n * 4);
    s.sorted_slot = take(n * 4);
    s.total = off;
    return s;
}

static NvWs nv_ws(const nrms_newsvec_desc* d) {
    NvWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = up256(off + bytes); return o; };
    const size_t n = (size_t)d->n_slots, e = (size_t)d->d;
    w.keys = take(n * 4);
    w.vals = take(n * 4);
    w.keys2 = take(n * 4);
    size_t tb = 0;
    (void)rocprim::radix_sort_pairs(nullptr, tb, (const int*)nullptr, (int*)nullptr, (const int*)nullptr, (int*)nullptr, n, 0,
                                    nv_key_bits(d->n_rows), (hipStream_t)0);
    w.sort_tmp_bytes = tb;
    w.sort_tmp = take(tb);
    w.y = take(n * e * 4);                                   // forward: Y; backward: dY
    w.x = take(n * e * 4);                                   // backward: the distinct rows of the table
    w.part = take(((n + NV_SPAN - 1) / NV_SPAN) * 2 * e * 4);   // backward: two span partials per span
    w.wt = take(e * e * 4);                                  // backward: W^T
    w.tn_partial = take(gemm_tn_workspace_floats((int)n, (int)e, (int)e, nullptr) * 4);
    w.wplanes = take(d->precision == NRMS_PRECISION_FP32 ? 0 : gemm_nt_bf16_wplane_bytes((int)e, (int)e));
    w.total = off;
    return w;
}

static int nv_validate(const nrms_newsvec_desc* d, const char* who) {
    NRMS_REQUIRE(d != nullptr, "%s: null desc", who);
    NRMS_REQUIRE(d->n_slots >= 0 && d->n_slots < (1L << 31) / 1024, "%s: n_slots=%ld", who, (long)d->n_slots);
    NRMS_REQUIRE(d->n_rows > 0, "%s: n_rows=%d", who, d->n_rows);
    NRMS_REQUIRE(d->d > 0 && (d->d & 3) == 0 && d->d <= 1024, "%s: d=%d must be a positive multiple of 4, <= 1024", who, d->d);
    NRMS_REQUIRE((long)d->n_rows * d->d < (1L << 31) * 4L, "%s: n_rows * d too large", who);
    NRMS_REQUIRE(d->precision == NRMS_PRECISION_FP32 || d->precision == NRMS_PRECISION_BF16X3 || d->precision == NRMS_PRECISION_BF16,
                 "%s: precision %d (fp32, bf16x3 or bf16)", who, d->precision);
    NRMS_REQUIRE(d->p_drop >= 0.f && d->p_drop < 1.f, "%s: p_drop must be in [0,1)", who);
    return NRMS_OK;
}

static int nv_nt(const nrms_newsvec_desc* d, const NTArgs& g, void* wplanes, hipStream_t s, const char* name) {
    if (d->precision == NRMS_PRECISION_FP32) return launch_gemm_nt(A_PLAIN, E_STORE, g, s, name);
    return launch_gemm_nt_bf16(A_PLAIN, E_STORE, d->precision == NRMS_PRECISION_BF16X3 ? 3 : 1, g, wplanes, s, name);
}

static int nv_check_ws(const char* who, size_t have, size_t need, const void* p) {
    if (have < need || (need && p == nullptr)) { set_error("%s: buffer %zu < required %zu bytes", who, have, need); return NRMS_EWORKSPACE; }
    NRMS_REQUIRE(((uintptr_t)p & 255) == 0, "%s: buffers must be 256-byte aligned", who);
    return NRMS_OK;
}

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_newsvec_saved_bytes(const nrms_newsvec_desc* desc) {
    if (nv_validate(desc, "newsvec_saved_bytes")) return 0;
    return nv_saved(desc).total;
}

extern "C" size_t nrms_newsvec_workspace_bytes(const nrms_newsvec_desc* desc) {
    if (nv_validate(desc, "newsvec_workspace_bytes")) return 0;
    return nv_ws(desc).total;
}

extern "C" int nrms_newsvec_fwd(const nrms_newsvec_desc* desc, const int64_t* ids, const float* table, const float* w,
                                const float* b, float* out, void* saved, size_t saved_bytes, int32_t* n_bad, void* workspace,
                                size_t workspace_bytes, void* stream) {
    int rc = nv_validate(desc, "newsvec_fwd");
    if (rc) return rc;
    NRMS_REQUIRE(table && w && b, "newsvec_fwd: null weight");
    const long n = desc->n_slots;
    if (n == 0) return NRMS_OK;
    NRMS_REQUIRE(ids && out, "newsvec_fwd: null ids / out");
    const NvSaved S = nv_saved(desc);
    const NvWs W = nv_ws(desc);
    if ((rc = nv_check_ws("newsvec_fwd: saved", saved_bytes, S.total, saved))) return rc;
    if ((rc = nv_check_ws("newsvec_fwd: workspace", workspace_bytes, W.total, workspace))) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* sv = (char*)saved;
    char* ws = (char*)workspace;
    int* n_unique = (int*)(sv + S.n_unique);
    int* uid = (int*)(sv + S.uid);
    int* sorted_slot = (int*)(sv + S.sorted_slot);
    int* keys = (int*)(ws + W.keys);
    int* keys2 = (int*)(ws + W.keys2);
    {
        TimingScope ts("newsvec_group", s);
        hipLaunchKernelGGL(nv_keys_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, n, ids, desc->n_rows, keys, (int*)(ws + W.vals), n_bad);
        size_t tb = W.sort_tmp_bytes;
        if (rocprim::radix_sort_pairs(ws + W.sort_tmp, tb, (const int*)keys, keys2, (const int*)(ws + W.vals), sorted_slot, (size_t)n, 0,
                                      nv_key_bits(desc->n_rows), s) != hipSuccess) {
            set_error("newsvec_fwd: radix_sort_pairs failed");
            return NRMS_ELAUNCH;
        }
        hipLaunchKernelGGL(nv_group_kernel, dim3(1), dim3(NV_SCAN_THREADS), 0, s, n, (const int*)keys2, (const int*)sorted_slot, n_unique,
                           uid, (int*)(sv + S.seg_start), (int*)(sv + S.slot_u));
        rc = check_launch("newsvec_group");
        if (rc) return rc;
    }
    const int d = desc->d;
    float* y = (float*)(ws + W.y);
    NTArgs g{};
    g.M = (int)n; g.N = d; g.K = d; g.rows_per_tile = NT_BM;
    g.A = table; g.lda = d; g.a_rows = uid; g.m_dev = n_unique;
    g.W = w; g.bias = b; g.C = y; g.ldc = d;
    rc = nv_nt(desc, g, ws + W.wplanes, s, "newsvec_dense_fwd");
    if (rc) return rc;
    TimingScope ts("newsvec_expand", s);
    hipLaunchKernelGGL(nv_expand_kernel, dim3(cdiv(n * (d / 4), 256)), dim3(256), 0, s, n, d, (const int*)(sv + S.slot_u), (const float*)y,
                       make_dropout(desc->seed, desc->p_drop), out);
    return check_launch("newsvec_expand");
}

extern "C" int nrms_newsvec_bwd(const nrms_newsvec_desc* desc, const float* table, const float* w, const float* dout,
                                const void* saved, size_t saved_bytes, float* d_table, float* d_w, float* d_b, void* workspace,
                                size_t workspace_bytes, void* stream) {
    int rc = nv_validate(desc, "newsvec_bwd");
    if (rc) return rc;
    NRMS_REQUIRE(table && w && d_table && d_w && d_b, "newsvec_bwd: null weight / gradient");
    const long n = desc->n_slots;
    if (n == 0) return NRMS_OK;
    NRMS_REQUIRE(dout != nullptr, "newsvec_bwd: null dout");
    const NvSaved S = nv_saved(desc);
    const NvWs W = nv_ws(desc);
    if ((rc = nv_check_ws("newsvec_bwd: saved", saved_bytes, S.total, saved))) return rc;
    if ((rc = nv_check_ws("newsvec_bwd: workspace", workspace_bytes, W.total, workspace))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const char* sv = (const char*)saved;
    char* ws = (char*)workspace;
    const int* n_unique = (const int*)(sv + S.n_unique);
    const int* uid = (const int*)(sv + S.uid);
    const int d = desc->d;
    float* dy = (float*)(ws + W.y);
    float* x = (float*)(ws + W.x);
    {
        TimingScope ts("newsvec_reduce", s);
        float* part = (float*)(ws + W.part);
        hipLaunchKernelGGL(nv_span_kernel, dim3(cdiv(n, NV_SPAN)), dim3(256), 0, s, n, d, (const int*)(sv + S.seg_start),
                           (const int*)(sv + S.slot_u), uid, (const int*)(sv + S.sorted_slot), dout, table,
                           make_dropout(desc->seed, desc->p_drop), dy, x, part);
        hipLaunchKernelGGL(nv_combine_kernel, dim3((unsigned)n), dim3(256), 0, s, d, n_unique, (const int*)(sv + S.seg_start),
                           (const float*)part, dy);
        rc = check_launch("newsvec_reduce");
        if (rc) return rc;
    }
    // d(W), d(b) += dY^T [X | 1] over the U distinct rows
    TNArgs t{};
    t.M = (int)n; t.N = d; t.K = d; t.amode = A_PLAIN;
    t.A = dy; t.lda = d; t.B = x; t.ldb = d;
    t.dW = d_w; t.dbias = d_b; t.partial = (float*)(ws + W.tn_partial);
    t.m_dev = n_unique;
    rc = desc->precision == NRMS_PRECISION_FP32 ? launch_gemm_tn(t, s, "newsvec_dw_bwd")
                                                : launch_gemm_tn_bf16(desc->precision == NRMS_PRECISION_BF16X3 ? 3 : 1, t, s, "newsvec_dw_bwd");
    if (rc) return rc;
    // d(table)[uid[u]] = dY[u] W: distinct rows, plain stores
    float* wt = (float*)(ws + W.wt);
    rc = launch_transpose(w, wt, d, d, s);
    if (rc) return rc;
    NTArgs g{};
    g.M = (int)n; g.N = d; g.K = d; g.rows_per_tile = NT_BM;
    g.A = dy; g.lda = d; g.m_dev = n_unique; g.c_rows = uid;
    g.W = wt; g.C = d_table; g.ldc = d;
    return nv_nt(desc, g, ws + W.wplanes, s, "newsvec_dx_bwd");
}

extern "C" int nrms_newsvec_distinct(const nrms_newsvec_desc* desc, const void* saved, int32_t* n_unique, int32_t* ids, void* stream) {
    int rc = nv_validate(desc, "newsvec_distinct");
    if (rc) return rc;
    NRMS_REQUIRE(saved && n_unique, "newsvec_distinct: null argument");
    const NvSaved S = nv_saved(desc);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(n_unique, (const char*)saved + S.n_unique, 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        (ids != nullptr && desc->n_slots > 0 &&
         hipMemcpyAsync(ids, (const char*)saved + S.uid, (size_t)desc->n_slots * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)) {
        set_error("newsvec_distinct: hipMemcpyAsync failed");
        return NRMS_ELAUNCH;
    }
    return NRMS_OK;
}

extern "C" size_t nrms_newsvec_rows_workspace_bytes(int64_t n_rows, int32_t d, int32_t precision) {
    if (n_rows < 0 || d <= 0 || (d & 3) != 0 || d > 1024) return 0;
    return precision == NRMS_PRECISION_FP32 ? 256 : up256(gemm_nt_bf16_wplane_bytes(d, d));
}

extern "C" int nrms_newsvec_rows_fwd(int64_t n_rows, int32_t d, int32_t precision, const float* table, const float* w, const float* b,
                                     float* out, void* workspace, size_t workspace_bytes, void* stream) {
    NRMS_REQUIRE(n_rows >= 0 && n_rows < (1L << 31) && d > 0 && (d & 3) == 0 && d <= 1024, "newsvec_rows_fwd: n_rows=%ld d=%d",
                 (long)n_rows, d);
    NRMS_REQUIRE(precision == NRMS_PRECISION_FP32 || precision == NRMS_PRECISION_BF16X3 || precision == NRMS_PRECISION_BF16,
                 "newsvec_rows_fwd: precision %d", precision);
    NRMS_REQUIRE(table && w && b && out, "newsvec_rows_fwd: null argument");
    const size_t need = nrms_newsvec_rows_workspace_bytes(n_rows, d, precision);
    NRMS_REQUIRE(workspace != nullptr, "newsvec_rows_fwd: null workspace");
    if (workspace_bytes < need) {
        set_error("newsvec_rows_fwd: workspace %zu < required %zu bytes", workspace_bytes, need);
        return NRMS_EWORKSPACE;
    }
    if (n_rows == 0) return NRMS_OK;
    nrms_newsvec_desc dd{};
    dd.precision = precision;
    NTArgs g{};
    g.M = (int)n_rows; g.N = d; g.K = d; g.rows_per_tile = NT_BM;
    g.A = table; g.lda = d; g.W = w; g.bias = b; g.C = out; g.ldc = d;
    return nv_nt(&dd, g, workspace, (hipStream_t)stream, "newsvec_rows_fwd");
}
