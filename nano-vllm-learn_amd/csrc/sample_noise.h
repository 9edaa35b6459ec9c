// The sampling noise: ONE definition for every kernel that samples (sample.hip, the candidate epilogue of linear_stream.hip) and for
// the tests' fp64 restatement.  Temperature sampling as nanovllm/layers/sampler.py draws it, argmax_j softmax(l / T)_j / E_j with
// E_j ~ Exp(1), equals argmax_j (l_j + T g_j) with g_j = -ln E_j standard Gumbel: no softmax, no division, and T = 0 is the greedy
// arg-max bit for bit.  The noise is a pure function of (seed, row_key, step, column): it does not know tiles, batches or ranks.
//   generator  Philox4x32-10 (Random123): key (seed_lo, seed_hi), counter (column >> 2, row_key, step_lo, step_hi); column c takes
//              output word c & 3, so four consecutive columns share one call
//   uniform    u = ((bits >> 9) + 0.5) * 2^-23: an odd multiple of 2^-24, exact in fp32, strictly inside (0, 1)
//   Gumbel     g = -ln(-ln u), in [-2.82, 16.64] (the tails cut off beyond carry about 6e-8 of the mass per draw)
//   score      T > 0 ? fma(T, g, l) : l   (a NaN temperature compares false: greedy), ordered by argmax_better
// Every floating-point step is spelled out (explicit fma, no expression a compiler may contract), so that files built with
// different -ffp-contract settings produce the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvh {

struct SampleArgs {                  // all null / 0: no sampling
    const float* temperatures;      // [rows]
    const uint32_t* row_keys;       // [rows] what tells two rows of one step apart (the engine: sequence ids)
    const int64_t* steps;           // [rows] the noise counter, read as uint64 (the engine: row_steps, tokens generated so far)
    uint64_t seed;
};

__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of columns 4 * (column >> 2) .. + 3
__host__ __device__ inline void sample_bits4(uint64_t seed, uint32_t row_key, uint64_t step, uint32_t column, uint32_t out[4]) {
    philox4x32_10(column >> 2, row_key, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

#ifdef __HIPCC__
// g = -ln(-ln u).  The large g that win come from u next to 1, where ln u is tiny: there (u > 3/4) -ln u is taken from w = 1 - u,
// which is exact in fp32 (2^24 - (2k + 1) is an integer below 2^24), as 2 atanh(w / (2 - w)) = 2 (z + z^3/3 + z^5/5 + z^7/7 ...),
// z <= 1/7: the first omitted term is below 2e-9 relative.  Elsewhere |log2 u| >= 0.41 and the hardware logarithm's error is
// relative to that.  The outer logarithm's error enters g absolutely.
__device__ __forceinline__ float gumbel_from_bits(uint32_t bits) {
    constexpr float kLn2 = 0.6931471805599453f;
    const uint32_t k = bits >> 9;
    const float u = (float)(2u * k + 1u) * 0x1p-24f;
    const float w = (float)(0xFFFFFFu - 2u * k) * 0x1p-24f;
    const float z = w * __builtin_amdgcn_rcpf(2.f - w);
    const float z2 = z * z;
    const float poly = __builtin_fmaf(z2, __builtin_fmaf(z2, __builtin_fmaf(z2, 1.f / 7.f, 0.2f), 1.f / 3.f), 1.f);
    const float e_near1 = (z + z) * poly;
    const float e_far = -kLn2 * __builtin_amdgcn_logf(u);
    const float e = k >= 0x600000u ? e_near1 : e_far;
    return -kLn2 * __builtin_amdgcn_logf(e);
}

__device__ __forceinline__ float sample_score(float logit, float temperature, float g) {
    return temperature > 0.f ? __builtin_fmaf(temperature, g, logit) : logit;
}

// one column's Gumbel draw
__device__ __forceinline__ float sample_gumbel(uint64_t seed, uint32_t row_key, uint64_t step, uint32_t column) {
    uint32_t w[4];
    sample_bits4(seed, row_key, step, column, w);
    const uint32_t lo = (column & 1) ? w[1] : w[0], hi = (column & 1) ? w[3] : w[2];
    return gumbel_from_bits((column & 2) ? hi : lo);
}
#endif

}  // namespace nvh
