// Experiment (docs/EXPERIMENTS.md, "Diversified re-ranking"): greedy MMR WITHOUT a Gram matrix.  One block of four waves per user;
// every step recomputes cos(pick, .) against the M gathered item rows (plain fp32 FMAs: four lanes share a row, 16 rows per wave
// pass, the pick's row staged in LDS), so a step re-reads M d floats per user instead of one Gram row.  No MFMA chain, no ILD, no
// padding rule: it is an upper bound on what this shape can do, timed beside csrc/mmr.hip's two kernels by tools/bench_mmr.py's
// sizes (B = 512, N = 130 000, d = 300, M = 256, k = 1, 10, 100; random shortlists).
//   hipcc --offload-arch=gfx950 -O3 -o mmr_nogram mmr_nogram.hip && ./mmr_nogram
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

constexpr int M = 256, D = 300;

__global__ __launch_bounds__(256) void nogram_kernel(int k, float lambda, const float* __restrict__ items,
                                                     const int64_t* __restrict__ ids, const float* __restrict__ scores,
                                                     int64_t* __restrict__ out_ids) {
    __shared__ __attribute__((aligned(16))) float prow[D];
    __shared__ float rinv[M], rel[M], maxsim[M];
    __shared__ __attribute__((aligned(16))) float val[M];
    __shared__ int live[M];
    __shared__ int pick;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    const int q = lane & 3, rr = lane >> 2;                    // four lanes per row, 16 rows per wave pass
    // norms, relevance
    for (int pass = 0; pass < 4; ++pass) {
        const int i = 64 * wave + 16 * pass + rr;
        const float* x = items + ids[b * M + i] * D;
        float acc = 0.0f;
        for (int c = q; c < D / 4; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(x + 4 * c);
            acc = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, acc))));
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        if (q == 0) rinv[i] = acc > 0.0f ? 1.0f / sqrtf(acc) : 0.0f;
    }
    float s = scores[b * M + tid], lo = s, hi = s;
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    val[wave] = lo;
    val[4 + wave] = hi;
    __syncthreads();
    lo = fminf(fminf(val[0], val[1]), fminf(val[2], val[3]));
    hi = fmaxf(fmaxf(val[4], val[5]), fmaxf(val[6], val[7]));
    __syncthreads();
    rel[tid] = hi != lo ? (s - lo) / (hi - lo) : 0.0f;
    maxsim[tid] = 0.0f;
    live[tid] = 1;
    __syncthreads();
    for (int t = 0; t < k; ++t) {
        // argmax of v over the live entries: per wave by shuffles, then wave 0 over the four
        const float v = lambda * rel[tid] - (1.0f - lambda) * maxsim[tid];
        uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        unsigned long long key = live[tid] ? ((unsigned long long)u << 32) | (0xFFFFFFFFu - (uint32_t)tid) : 0ull;
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o, 64);
            key = other > key ? other : key;
        }
        if (lane == 0) reinterpret_cast<unsigned long long*>(val)[wave] = key;
        __syncthreads();
        if (tid == 0) {
            unsigned long long best = 0;
            for (int w = 0; w < 4; ++w) {
                const unsigned long long o = reinterpret_cast<unsigned long long*>(val)[w];
                best = o > best ? o : best;
            }
            const int p = (int)(0xFFFFFFFFu - (uint32_t)best);
            pick = p;
            live[p] = 0;
            out_ids[b * k + t] = ids[b * M + p];
        }
        __syncthreads();
        const int p = pick;
        const float* xp = items + ids[b * M + p] * D;
        for (int c = tid; c < D; c += 256) prow[c] = xp[c];
        __syncthreads();
        const float rp = rinv[p];
        for (int pass = 0; pass < 4; ++pass) {
            const int i = 64 * wave + 16 * pass + rr;
            const float* x = items + ids[b * M + i] * D;
            float acc = 0.0f;
            for (int c = q; c < D / 4; c += 4) {
                const float4 a = *reinterpret_cast<const float4*>(x + 4 * c);
                const float4 w = *reinterpret_cast<const float4*>(prow + 4 * c);
                acc = fmaf(a.x, w.x, fmaf(a.y, w.y, fmaf(a.z, w.z, fmaf(a.w, w.w, acc))));
            }
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            if (q == 0) {
                const float cs = acc * (rinv[i] * rp);
                maxsim[i] = t == 0 ? cs : fmaxf(maxsim[i], cs);
            }
        }
        __syncthreads();
    }
}

int main() {
    const int B = 512, N = 130000;
    std::vector<float> h_items((size_t)N * D), h_scores((size_t)B * M);
    std::vector<int64_t> h_ids((size_t)B * M);
    srand(1);
    for (auto& v : h_items) v = rand() / (float)RAND_MAX - 0.5f;
    for (auto& v : h_scores) v = rand() / (float)RAND_MAX;
    for (auto& v : h_ids) v = (int64_t)(((uint64_t)rand() * 32768u + (uint64_t)rand()) % N);
    float *items, *scores;
    int64_t *ids, *out;
    if (hipMalloc(&items, h_items.size() * 4) != hipSuccess || hipMalloc(&scores, h_scores.size() * 4) != hipSuccess ||
        hipMalloc(&ids, h_ids.size() * 8) != hipSuccess || hipMalloc(&out, (size_t)B * M * 8) != hipSuccess) {
        printf("hipMalloc failed\n");
        return 1;
    }
    hipMemcpy(items, h_items.data(), h_items.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(scores, h_scores.data(), h_scores.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(ids, h_ids.data(), h_ids.size() * 8, hipMemcpyHostToDevice);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const int ks[3] = {1, 10, 100};
    for (int ki = 0; ki < 3; ++ki) {
        const int k = ks[ki];
        float best = 1e30f;
        for (int run = 0; run < 4; ++run) {                    // run 0 warms up
            const int reps = 10;
            hipEventRecord(e0, 0);
            for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(nogram_kernel, dim3(B), dim3(256), 0, 0, k, 0.5f, items, ids, scores, out);
            hipEventRecord(e1, 0);
            if (hipEventSynchronize(e1) != hipSuccess) {
                printf("kernel failed: %s\n", hipGetErrorString(hipGetLastError()));
                return 1;
            }
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            if (run > 0 && ms / reps < best) best = ms / reps;
        }
        std::vector<int64_t> h_out((size_t)B * k);
        hipMemcpy(h_out.data(), out, h_out.size() * 8, hipMemcpyDeviceToHost);
        long sum = 0;
        for (auto v : h_out) sum += v;
        printf("no-Gram greedy k=%-3d %8.3f ms (min of 3 x 10 launches)  id checksum %ld\n", k, best, sum);
    }
    return 0;
}
