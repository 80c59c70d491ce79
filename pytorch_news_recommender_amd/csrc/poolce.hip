// In-batch sampled softmax over the batch's shared candidate pool (nrms_pooled_ce_fwd_bwd, include/nrms_hip.h).
//
//   scores   Z[b, j] = <user[b], cand[j]> + col_bias[j], or -inf where column j is not in the softmax of row b   [B, M] in the workspace
//   softmax  per row: loss_b, and Z overwritten with g = (softmax - onehot(own)) * grad_scale                     one workgroup per row
//   loss     loss_sum[0] += the row losses, one 256-leaf tree
//   duser    = G . V   (K = M, split over K into slabs that are added in ascending order)
//   dcand    = G^T . U (K = B)
//
// The three products are ONE kernel, pc_gemm_kernel: C[m, n] = sum_k A(m, k) B(k, n) with element strides for both operands, on the
// exact f32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain).  A workgroup of four waves owns a 32 x 128 tile, one 32 x 32
// accumulator per wave; a K stage of 32 is staged through LDS with bounds-checked scalar loads (zero past M, N or K), so no extent
// has to be a multiple of anything: d = 1 and B*C = 3 run the same code as d = 300.  The gemm.hip launchers were not reused: their
// contracts (K % 4 == 0, 16-byte rows, W as [N, K], accumulate-into-dW with a ones column) fit none of the three products without
// two transposes of the [B, M] matrix.
//
// Every sum has a fixed order: k ascending inside a product, K slabs ascending, the softmax denominator per thread in fp32 runs of
// 16 added up in double and then a 256-leaf tree in double, the row losses a 256-leaf tree.  The only atomic is the integer count
// n_pairs.  Every workspace byte that is read has been written by an earlier kernel of the same call.
#include "common.h"

namespace nrms {

constexpr int PC_BM = 32;              // tile rows (one MFMA)
constexpr int PC_BN = 128;             // tile columns (4 waves x 32)
constexpr int PC_BK = 32;              // K per LDS stage
constexpr int PC_PITCH = PC_BK + 1;    // LDS row pitch in floats: rows 1 bank apart, the fragment reads of 32 rows hit 32 banks
constexpr int PC_RCHUNK = 64;          // reject entries per row held in LDS at a time
constexpr int PC_SPLIT_K = 512;        // duser: one K slab per 512 pool columns, at most PC_MAX_SPLITS slabs of whole stages
constexpr int PC_MAX_SPLITS = 8;

enum { PC_STORE = 0, PC_SCORES = 1 };

struct PcGemm {
    int M, N, K;
    const float* A; long a_m, a_k;     // A(m, k) = A[m * a_m + k * a_k]
    const float* B; long b_k, b_n;     // B(k, n) = B[k * b_k + n * b_n]
    float* C; long ldc;                // C[m * ldc + n]
    long c_slab;                       // blockIdx.z writes C + blockIdx.z * c_slab ...
    int k_per_slab;                    // ... the sum over k in [z * k_per_slab, min(K, (z + 1) * k_per_slab))
    // PC_SCORES epilogue (m = batch row b, n = pool column j)
    int Cn, R;
    const int64_t* cand_id;
    const uint8_t* mask;
    const int64_t* reject;
    const float* col_bias;
    unsigned long long* n_pairs;
};

// A_KFAST / B_KFAST: the operand is contiguous along k (else along m / n); it only picks the staging order that coalesces
template <int EPI, bool A_KFAST, bool B_KFAST>
__global__ __launch_bounds__(256) void pc_gemm_kernel(PcGemm g) {
    __shared__ float As[PC_BM * PC_PITCH];
    __shared__ float Bs[PC_BN * PC_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int m0 = blockIdx.y * PC_BM, n0 = blockIdx.x * PC_BN;
    const int kbeg = blockIdx.z * g.k_per_slab;
    const int kend = min(g.K, kbeg + g.k_per_slab);

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int k0 = kbeg; k0 < kend; k0 += PC_BK) {
#pragma unroll
        for (int it = 0; it < PC_BM * PC_BK / 256; ++it) {
            const int e = tid + 256 * it;
            const int k = A_KFAST ? (e & 31) : (e >> 5);
            const int m = A_KFAST ? (e >> 5) : (e & 31);
            const bool ok = m0 + m < g.M && k0 + k < kend;
            As[m * PC_PITCH + k] = ok ? g.A[(long)(m0 + m) * g.a_m + (long)(k0 + k) * g.a_k] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < PC_BN * PC_BK / 256; ++it) {
            const int e = tid + 256 * it;
            const int k = B_KFAST ? (e & 31) : (e >> 7);
            const int n = B_KFAST ? (e >> 5) : (e & 127);
            const bool ok = n0 + n < g.N && k0 + k < kend;
            Bs[n * PC_PITCH + k] = ok ? g.B[(long)(k0 + k) * g.b_k + (long)(n0 + n) * g.b_n] : 0.f;
        }
        __syncthreads();
        const float* ap = As + i * PC_PITCH + hh;
        const float* bp = Bs + (32 * wave + i) * PC_PITCH + hh;
#pragma unroll
        for (int kk = 0; kk < PC_BK; kk += 2) acc = mfma32(ap[kk], bp[kk], acc);      // lane half hh holds k = kk + hh
        __syncthreads();
    }

    const int n = n0 + 32 * wave + i;
    const bool nok = n < g.N;
    if constexpr (EPI == PC_STORE) {
        float* c = g.C + (long)blockIdx.z * g.c_slab;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + crow32(r, hh);
            if (m < g.M && nok) c[(long)m * g.ldc + n] = acc[r];
        }
    } else {
    // ---- scores epilogue: bias, the exclusion rule, -inf --------------------------------------------------------------------------
    __shared__ long long rej_s[PC_BM][PC_RCHUNK];
    __shared__ long long own_s[PC_BM];
    __shared__ int live_s[PC_BM];
    if (tid < PC_BM) {
        const int b = m0 + tid;
        long long oid = 0;
        int lv = 0;
        if (b < g.M) {
            const long oc = (long)b * g.Cn;
            oid = g.cand_id[oc];
            lv = g.mask == nullptr || g.mask[oc] != 0;
        }
        own_s[tid] = oid;
        live_s[tid] = lv;
    }
    const long long colid = nok ? (long long)g.cand_id[n] : 0;
    const bool col_live = nok && (g.mask == nullptr || g.mask[n] != 0);
    const float bias = (nok && g.col_bias != nullptr) ? g.col_bias[n] : 0.f;
    unsigned hit = 0;                          // bit r: this column's id is in the reject list of accumulator row r
    for (int e0 = 0; e0 < g.R; e0 += PC_RCHUNK) {
        const int ne = min(PC_RCHUNK, g.R - e0);
        __syncthreads();                       // the previous chunk has been read
        for (int idx = tid; idx < PC_BM * PC_RCHUNK; idx += 256) {
            const int row = idx / PC_RCHUNK, e = idx - row * PC_RCHUNK;
            const int b = m0 + row;
            rej_s[row][e] = (b < g.M && e < ne) ? (long long)g.reject[(long)b * g.R + e0 + e] : 0;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long* rr = rej_s[crow32(r, hh)];
            bool h = false;
            for (int e = 0; e < ne; ++e) h |= rr[e] == colid;
            hit |= (unsigned)h << r;
        }
    }
    __syncthreads();                           // own_s / live_s (the only barrier when R == 0)
    if (colid <= 0) hit = 0;                   // reject entries <= 0 match nothing (the zero fill of rej_s included)
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = crow32(r, hh);
        const int b = m0 + row;
        if (b < g.M && nok) {
            const bool own = (long)n == (long)b * g.Cn;
            const bool incl = live_s[row] != 0 && (own || (col_live && colid != own_s[row] && ((hit >> r) & 1u) == 0u));
            g.C[(long)b * g.ldc + n] = incl ? acc[r] + bias : -INFINITY;
            cnt += (incl && !own) ? 1 : 0;
        }
    }
    if (g.n_pairs != nullptr) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0 && cnt != 0) atomicAdd(g.n_pairs, (unsigned long long)cnt);      // integer: exact in any order
    }
    }
}

// One workgroup per row of Z.  The denominator as in ce_loss_kernel (pool.hip): fp32 runs of 16 slots added up in double, here per
// thread over its strided slots, then a fixed tree in double; log and reciprocal in double, rounded once.
__global__ __launch_bounds__(256) void pc_softmax_kernel(int Cn, int M, float* Z, const uint8_t* mask, float gscale, float* row_loss,
                                                         int want_grad) {
    __shared__ double red[256];
    __shared__ float redf[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float* z = Z + (long)b * M;
    const int own = b * Cn;
    if (mask != nullptr && mask[own] == 0) {           // dead row: no loss, no gradient
        if (want_grad)
            for (int j = tid; j < M; j += 256) z[j] = 0.f;
        if (tid == 0) row_loss[b] = 0.f;
        return;
    }
    float mx = -INFINITY;
    for (int j = tid; j < M; j += 256) mx = fmaxf(mx, z[j]);
    redf[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) redf[tid] = fmaxf(redf[tid], redf[tid + o]);
        __syncthreads();
    }
    mx = redf[0];
    double sum = 0.0;
    float run = 0.f;
    int in_run = 0;
    for (int j = tid; j < M; j += 256) {
        run += expf(z[j] - mx);                        // exp(-inf) = 0 for the excluded slots
        if (++in_run == 16) { sum += (double)run; run = 0.f; in_run = 0; }
    }
    sum += (double)run;
    red[tid] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    sum = red[0];
    if (tid == 0) row_loss[b] = (float)(((double)mx - (double)z[own]) + log(sum));
    if (!want_grad) return;
    __syncthreads();                                   // z[own] has been read
    const float inv = (float)(1.0 / sum);
    for (int j = tid; j < M; j += 256) {
        const float v = z[j];
        const float e = expf(v - mx);
        const float p = (j == own) ? __builtin_fmaf(e, inv, -1.0f) : e * inv;
        z[j] = (v == -INFINITY) ? 0.f : p * gscale;    // excluded: exactly +0
    }
}

__global__ __launch_bounds__(256) void pc_loss_sum_kernel(int B, const float* row_loss, float* loss_sum) {
    __shared__ float red[256];
    float local = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) local += row_loss[b];
    red[threadIdx.x] = local;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_sum[0] += red[0];
}

// out[i] = slab 0 [i] + slab 1 [i] + ... in ascending order
__global__ void pc_slab_sum_kernel(long n, int slabs, const float* partial, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = partial[i];
    for (int z = 1; z < slabs; ++z) s += partial[(long)z * n + i];
    out[i] = s;
}

struct PcLayout { size_t z, row_loss, partial, total; int slabs, k_per_slab; };

static size_t pc_align(size_t x) { return (x + 255) / 256 * 256; }

static bool pc_shape_ok(int B, int C, int d, int R) {
    return B >= 1 && B <= 4096 && C >= 1 && C <= 64 && (long)B * C <= 32768 && d >= 1 && d <= 1024 && R >= 0 && R <= 256;
}

static PcLayout pc_layout(int B, int C, int d) {
    const long M = (long)B * C;
    PcLayout L;
    const long want = (M + PC_SPLIT_K - 1) / PC_SPLIT_K;
    L.slabs = want < PC_MAX_SPLITS ? (int)want : PC_MAX_SPLITS;
    L.k_per_slab = cdiv(cdiv(M, L.slabs), PC_BK) * PC_BK;
    L.z = 0;
    L.row_loss = pc_align(L.z + (size_t)B * M * 4);
    L.partial = pc_align(L.row_loss + (size_t)B * 4);
    L.total = pc_align(L.partial + (L.slabs > 1 ? (size_t)L.slabs * B * d * 4 : 0));
    return L;
}

}  // namespace nrms

using namespace nrms;

extern "C" size_t nrms_pooled_ce_workspace_bytes(int32_t B, int32_t C, int32_t d, int32_t R) {
    if (!pc_shape_ok(B, C, d, R)) {
        set_error("pooled_ce_workspace_bytes: B=%d C=%d d=%d R=%d (B in [1, 4096], C in [1, 64], B*C <= 32768, d in [1, 1024], R in [0, 256])",
                  B, C, d, R);
        return 0;
    }
    return pc_layout(B, C, d).total;
}

extern "C" int nrms_pooled_ce_fwd_bwd(int32_t B, int32_t C, int32_t d, int32_t R, const float* cand, const float* user,
                                      const int64_t* cand_id, const uint8_t* cand_mask, const int64_t* reject, const float* col_bias,
                                      float grad_scale, float* loss_sum, float* dcand, float* duser, int64_t* n_pairs, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    NRMS_REQUIRE(pc_shape_ok(B, C, d, R),
                 "pooled_ce: B=%d C=%d d=%d R=%d (B in [1, 4096], C in [1, 64], B*C <= 32768, d in [1, 1024], R in [0, 256])", B, C, d, R);
    NRMS_REQUIRE(cand && user && cand_id && loss_sum, "pooled_ce: null argument");
    NRMS_REQUIRE((reject != nullptr) == (R > 0), "pooled_ce: reject must be NULL exactly when R == 0 (R=%d)", R);
    NRMS_REQUIRE((dcand != nullptr) == (duser != nullptr), "pooled_ce: dcand and duser must both be given or both be NULL");
    const PcLayout L = pc_layout(B, C, d);
    NRMS_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 15) == 0, "pooled_ce: workspace must be 16-byte aligned and not null");
    NRMS_REQUIRE(workspace_bytes >= L.total, "pooled_ce: workspace %zu < required %zu bytes", workspace_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    const int M = B * C;
    const bool want_grad = dcand != nullptr;
    char* ws = (char*)workspace;
    float* Z = (float*)(ws + L.z);
    float* row_loss = (float*)(ws + L.row_loss);
    float* partial = (float*)(ws + L.partial);
    int rc;
    {
        TimingScope ts("pooled_ce_scores", s);
        PcGemm g{};
        g.M = B; g.N = M; g.K = d;
        g.A = user; g.a_m = d; g.a_k = 1;
        g.B = cand; g.b_k = 1; g.b_n = d;
        g.C = Z; g.ldc = M; g.c_slab = 0; g.k_per_slab = d;
        g.Cn = C; g.R = R; g.cand_id = cand_id; g.mask = cand_mask; g.reject = reject; g.col_bias = col_bias;
        g.n_pairs = (unsigned long long*)n_pairs;
        hipLaunchKernelGGL((pc_gemm_kernel<PC_SCORES, true, true>), dim3(cdiv(M, PC_BN), cdiv(B, PC_BM), 1), dim3(256), 0, s, g);
        if ((rc = check_launch("pooled_ce_scores")) != NRMS_OK) return rc;
    }
    {
        TimingScope ts("pooled_ce_softmax", s);
        hipLaunchKernelGGL(pc_softmax_kernel, dim3(B), dim3(256), 0, s, C, M, Z, cand_mask, grad_scale, row_loss, want_grad ? 1 : 0);
        if ((rc = check_launch("pooled_ce_softmax")) != NRMS_OK) return rc;
    }
    {
        TimingScope ts("pooled_ce_loss_sum", s);
        hipLaunchKernelGGL(pc_loss_sum_kernel, dim3(1), dim3(256), 0, s, B, row_loss, loss_sum);
        if ((rc = check_launch("pooled_ce_loss_sum")) != NRMS_OK) return rc;
    }
    if (!want_grad) return NRMS_OK;
    {
        TimingScope ts("pooled_ce_duser", s);
        PcGemm g{};
        g.M = B; g.N = d; g.K = M;
        g.A = Z; g.a_m = M; g.a_k = 1;
        g.B = cand; g.b_k = d; g.b_n = 1;
        g.C = L.slabs > 1 ? partial : duser; g.ldc = d; g.c_slab = (long)B * d;
        g.k_per_slab = L.k_per_slab;
        hipLaunchKernelGGL((pc_gemm_kernel<PC_STORE, true, false>), dim3(cdiv(d, PC_BN), cdiv(B, PC_BM), L.slabs), dim3(256), 0, s, g);
        if ((rc = check_launch("pooled_ce_duser")) != NRMS_OK) return rc;
    }
    if (L.slabs > 1) {
        TimingScope ts("pooled_ce_duser_sum", s);
        const long n = (long)B * d;
        hipLaunchKernelGGL(pc_slab_sum_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, n, L.slabs, partial, duser);
        if ((rc = check_launch("pooled_ce_duser_sum")) != NRMS_OK) return rc;
    }
    {
        TimingScope ts("pooled_ce_dcand", s);
        PcGemm g{};
        g.M = M; g.N = d; g.K = B;
        g.A = Z; g.a_m = 1; g.a_k = M;
        g.B = user; g.b_k = d; g.b_n = 1;
        g.C = dcand; g.ldc = d; g.c_slab = 0; g.k_per_slab = B;
        hipLaunchKernelGGL((pc_gemm_kernel<PC_STORE, false, false>), dim3(cdiv(d, PC_BN), cdiv(M, PC_BM), 1), dim3(256), 0, s, g);
        if ((rc = check_launch("pooled_ce_dcand")) != NRMS_OK) return rc;
    }
    return NRMS_OK;
}
