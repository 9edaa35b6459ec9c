// Temperature sampling of materialised logits (nanovllm/layers/sampler.py): token = argmax_j (l_j + T g_j) with the counter-based
// Gumbel noise of sample_noise.h, so a row's token is a pure function of (logits, T, seed, row key, step) and a captured decode
// step draws fresh noise on every replay from the device-resident row_steps counter alone.  The eager path, the prefill's first
// token and the non-fused decode step; the fused step perturbs inside the LM head instead (linear_stream.hip).
//   * one 1024-thread workgroup per row, 16-byte non-temporal loads: 8 bf16 logits = two Philox calls (one per four columns)
//   * a row with T <= 0 (or NaN) never touches the generator: it is argmax_rows_kernel's loop, the same token bit for bit
//   * the advance bookkeeping rides in the same launch as in nvh_greedy_advance; the noise step is read from row_steps when the
//     row starts, the increment happens behind the workgroup's barrier
#include "common.h"
#include "kernels.h"

namespace nvh {

namespace {

__global__ __launch_bounds__(1024) void sample_rows_kernel(int64_t* __restrict__ out, const uint16_t* __restrict__ x, int n, int64_t stride,
                                                            const SampleArgs s, const AdvanceArgs adv) {
    __shared__ float lds_v[16];
    __shared__ int lds_i[16];
    const int r = blockIdx.x;
    const uint16_t* row = x + r * stride;
    const float temp = s.temperatures[r];
    const uint32_t key = s.row_keys[r];
    const uint64_t step = (uint64_t)(s.steps ? s.steps[r] : adv.row_steps[r]);
    const bool noisy = temp > 0.f;                                          // workgroup-uniform
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    const int chunks = n / 8;
    for (int c = threadIdx.x; c < chunks; c += 1024) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row + c * 8));
        float sc[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) { sc[2 * k] = bf16_lo(v[k]); sc[2 * k + 1] = bf16_hi(v[k]); }
        if (noisy) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint32_t w[4];
                sample_bits4(s.seed, key, step, (uint32_t)(c * 8 + 4 * h), w);
#pragma unroll
                for (int k = 0; k < 4; ++k) sc[4 * h + k] = sample_score(sc[4 * h + k], temp, gumbel_from_bits(w[k]));
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (argmax_better(sc[k], c * 8 + k, best, bidx)) { best = sc[k]; bidx = c * 8 + k; }
    }
    for (int i = chunks * 8 + threadIdx.x; i < n; i += 1024) {              // tail when n % 8 != 0: a column per thread
        float f = bf16_lo((uint32_t)row[i]);
        if (noisy) f = sample_score(f, temp, sample_gumbel(s.seed, key, step, (uint32_t)i));
        if (argmax_better(f, i, best, bidx)) { best = f; bidx = i; }
    }
    // wave fold (NaN first, value desc, column asc), then across the 16 waves
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bidx, off, 64);
        if (argmax_better(ov, oi, best, bidx)) { best = ov; bidx = oi; }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { lds_v[wave] = best; lds_i[wave] = bidx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w)
            if (argmax_better(lds_v[w], lds_i[w], best, bidx)) { best = lds_v[w]; bidx = lds_i[w]; }
        bidx = bidx < 0 ? 0 : (bidx >= n ? n - 1 : bidx);                   // n >= 1 (host): always a valid column
        if (out) out[r] = bidx;
        if (adv.input_ids) advance_row(adv, r, bidx);
    }
}

// g of columns 0..n-1 for one (seed, row key, step): the generator on its own, for bit-level tests
__global__ __launch_bounds__(256) void gumbel_noise_kernel(float* __restrict__ out, uint64_t seed, uint32_t row_key, uint64_t step, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sample_gumbel(seed, row_key, step, (uint32_t)i);
}

}  // namespace

int launch_sample_rows(int64_t* out, const void* x, int n_rows, int n, int64_t stride, const SampleArgs& s, const AdvanceArgs& adv, hipStream_t stream) {
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(sample_rows_kernel, dim3(n_rows), dim3(1024), 0, stream, out, (const uint16_t*)x, n, stride, s, adv);
    return check_launch("sample_rows");
}

int launch_gumbel_noise(float* out, uint64_t seed, uint32_t row_key, uint64_t step, int n, hipStream_t stream) {
    hipLaunchKernelGGL(gumbel_noise_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, out, seed, row_key, step, n);
    return check_launch("gumbel_noise");
}

}  // namespace nvh
