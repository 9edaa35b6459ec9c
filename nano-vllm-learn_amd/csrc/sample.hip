// The next token of each row of materialised logits, greedy or by temperature sampling (nanovllm/layers/sampler.py):
// token = argmax_j (l_j + T g_j) with the counter-based Gumbel noise of sample_noise.h, so a row's token is a pure function of
// (logits, T, seed, row key, step) and a captured decode step draws fresh noise on every replay from the device-resident row_steps
// counter alone.  The eager path, the prefill's first token and the non-fused decode step; the fused step perturbs inside the LM
// head instead (linear_stream.hip).  ONE kernel body (choose_row), built from token_choice.h, in two instantiations:
//   greedy_rows_kernel   torch.argmax per row (ties -> lowest index); no SampleArgs, none of the generator's registers
//   sample_rows_kernel   the same body with the noise; a row with T <= 0 (or NaN) never touches the generator and takes the
//                        greedy instantiation's statements, so it is the same token bit for bit
//   * one 1024-thread workgroup per row, 16-byte non-temporal loads: 8 bf16 logits = two Philox calls (one per four columns)
//   * the advance bookkeeping rides in the same launch; the noise step is read from row_steps when the row starts, the increment
//     happens behind the workgroup's barrier
#include "common.h"
#include "kernels.h"
#include "token_choice.h"

namespace nvh {

namespace {

template <bool kMayPerturb>
__device__ __forceinline__ void choose_row(int64_t* __restrict__ out, const uint16_t* __restrict__ x, int n, int64_t stride,
                                           const SampleArgs& s, const AdvanceArgs& adv) {
    __shared__ ArgmaxFold<16> fold;
    const int r = blockIdx.x;
    RowNoise z{};
    if constexpr (kMayPerturb) z = row_noise(s, adv, r);
    const bool noisy = kMayPerturb && z.temp > 0.f;                         // workgroup-uniform
    const auto all = [](uint32_t) { return true; };
    float best = -INFINITY;
    int bidx = kNoColumn;
    walk_row<1, true>(x + r * stride, n,
        [&](int col0, const u32x4& v) {
            if (noisy) perturbed_argmax_chunk(z, col0, v, all, best, bidx);
            else argmax_chunk(col0, v, best, bidx);
        },
        [&](int col, uint32_t bits) {
            if (noisy) perturbed_argmax_column(z, col, bits, all, best, bidx);
            else argmax_column(col, bits, best, bidx);
        });
    block_argmax(best, bidx, fold);
    if (threadIdx.x == 0) finish_row(out, adv, r, n, bidx);
}

__global__ __launch_bounds__(1024) void greedy_rows_kernel(int64_t* __restrict__ out, const uint16_t* __restrict__ x, int n, int64_t stride,
                                                            const AdvanceArgs adv) {
    choose_row<false>(out, x, n, stride, SampleArgs{}, adv);
}

__global__ __launch_bounds__(1024) void sample_rows_kernel(int64_t* __restrict__ out, const uint16_t* __restrict__ x, int n, int64_t stride,
                                                            const SampleArgs s, const AdvanceArgs adv) {
    choose_row<true>(out, x, n, stride, s, adv);
}

// g of columns 0..n-1 for one (seed, row key, step): the generator on its own, for bit-level tests
__global__ __launch_bounds__(256) void gumbel_noise_kernel(float* __restrict__ out, uint64_t seed, uint32_t row_key, uint64_t step, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sample_gumbel(seed, row_key, step, (uint32_t)i);
}

}  // namespace

int launch_argmax_rows(int64_t* out, const void* x, int n_rows, int n, int64_t stride, const AdvanceArgs& adv, hipStream_t stream) {
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(greedy_rows_kernel, dim3(n_rows), dim3(kRowThreads), 0, stream, out, (const uint16_t*)x, n, stride, adv);
    return check_launch("argmax_rows");
}

int launch_sample_rows(int64_t* out, const void* x, int n_rows, int n, int64_t stride, const SampleArgs& s, const AdvanceArgs& adv, hipStream_t stream) {
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(sample_rows_kernel, dim3(n_rows), dim3(kRowThreads), 0, stream, out, (const uint16_t*)x, n, stride, s, adv);
    return check_launch("sample_rows");
}

int launch_gumbel_noise(float* out, uint64_t seed, uint32_t row_key, uint64_t step, int n, hipStream_t stream) {
    hipLaunchKernelGGL(gumbel_noise_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, out, seed, row_key, step, n);
    return check_launch("gumbel_noise");
}

}  // namespace nvh
