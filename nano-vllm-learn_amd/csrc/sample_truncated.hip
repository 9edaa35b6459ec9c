// Top-k / top-p sampling of materialised logits: the Gumbel-max of sample.hip over a TRUNCATED column set (semantics: nvh_attn.h,
// DESIGN.md section 14).  Truncation is defined on value classes: a bf16 row has at most 65536 distinct values, so "the k-th largest
// value" and "the classes whose weight above stays below top_p * Z" are found by radix selection over an order-preserving 16-bit key
// (12 bits in a 4096-bin LDS histogram, the low 4 bits in 16 sub-bins of the one bin that holds the cut), never by sorting columns.
// The kept set is {key >= threshold key}; only those columns ever see the generator.
//   * one 1024-thread workgroup per row; the row (<= 300 KB) is re-read from the cache once per pass with ordinary 16-byte loads
//   * pass 1  arg-max in torch.argmax's order: the greedy token of a T <= 0 row, the lowest NaN column of a NaN row, the row maximum
//     pass 2  top-k on: column counts per bin; suffix scan -> the bin of v_k          pass 3  its 16 sub-bins -> key(v_k)
//     pass 4  top-p on: weights of the top-k survivors per bin; scan vs top_p * Z     pass 5  its 16 sub-bins -> key(v_p)
//     final   Philox / Gumbel / fma for columns with key >= max(key(v_k), key(v_p)) only, arg-max fold, finish_row
//   * determinism: a weight is the INTEGER round(w * 2^40), w = exp((l - max) / T) in [0, 1], added with integer LDS atomics
//     (associative: the sums do not depend on the order of arrival; n <= 2^18 columns keep every sum below 2^58), scanned in a
//     fixed order and compared with top_p * Z in fp64.  No floating-point atomic, no order-dependent float sum.
//   * LDS: 4096 x uint32 counts (16 KB) + 4096 x uint64 weights (32 KB) + 16 + 16 sub-bins and the folds' scratch: 48.5 KB
#include "common.h"
#include "kernels.h"
#include "token_choice.h"

namespace nvh {

namespace {

constexpr int kThreads = kRowThreads;
constexpr int kBins = 4096;                     // key >> 4
constexpr int kPerThread = kBins / kThreads;    // consecutive bins a thread scans
constexpr float kWeightOne = 0x1p40f;           // fixed point of a weight

// bf16 bits -> 16-bit key with key(a) < key(b) <=> a < b (-0 is +0: one value class); NaN rows never get here
__device__ __forceinline__ uint32_t order_key(uint32_t b) {
    b = b == 0x8000u ? 0u : b;
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}

// round(exp((l - max) / T) * 2^40); scale = log2(e) / T.  The top class is exactly 2^40 (also when max is infinite or scale
// overflowed); whatever else an infinite operand produces is clamped into [0, 1] before the conversion.
__device__ __forceinline__ uint64_t fixed_weight(uint32_t bits, float row_max, float scale) {
    const float l = bf16_lo(bits);
    const float w = l == row_max ? 1.f : __builtin_fminf(__builtin_fmaxf(fast_exp2((l - row_max) * scale), 0.f), 1.f);
    return (uint64_t)__builtin_rintf(w * kWeightOne);
}

struct Fold {                       // LDS scratch of the workgroup-wide folds
    ArgmaxFold<16> arg;
    uint64_t wave_sum[16];
    uint64_t total, above;
    int bin;
};

struct Cut { int bin; uint64_t above; double target; };   // bin -1: no bin qualifies

// The cut of a 4096-bin histogram: the LOWEST bin b whose mass above it, above(b) = sum of hist[b' > b], is below the target
// (above() grows as b falls, so the qualifying bins are a suffix).  target = of_total ? x * sum(hist) : x.  Thread t owns bins
// 4t .. 4t + 3; the suffix sums run lane by lane, wave by wave, in one fixed order.  Every thread returns the same Cut.
template <typename T>
__device__ __forceinline__ Cut find_cut(const T* hist, double x, bool of_total, Fold& f) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint64_t h[kPerThread], own = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) { h[j] = hist[t * kPerThread + j]; own += h[j]; }
    uint64_t incl = own;                                                    // own + the higher lanes of this wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = __shfl_down((unsigned long long)incl, off, 64);
        if (lane + off < 64) incl += o;
    }
    __syncthreads();                                                        // the previous cut's readers are done
    if (lane == 0) f.wave_sum[wave] = incl;
    if (t == 0) f.bin = -1;
    __syncthreads();
    uint64_t above = incl - own, total = 0;                                 // above: the mass of the bins > 4t + 3
    for (int w = 0; w < 16; ++w) { total += f.wave_sum[w]; if (w > wave) above += f.wave_sum[w]; }
    const double target = of_total ? x * (double)total : x;
    uint64_t a[kPerThread + 1];                                             // a[j + 1] = above(4t + j); a[0] = above(4t - 1)
    a[kPerThread] = above;
#pragma unroll
    for (int j = kPerThread - 1; j >= 0; --j) a[j] = a[j + 1] + h[j];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const bool lower_qualifies = (t > 0 || j > 0) && (double)a[j] < target;
        if ((double)a[j + 1] < target && !lower_qualifies) { f.bin = t * kPerThread + j; f.above = a[j + 1]; }   // one writer at most
    }
    __syncthreads();
    return Cut{f.bin, f.above, target};
}

// the same cut inside bin c.bin: the lowest of its 16 sub-bins whose mass above stays below the target -> the 16-bit key
template <typename T>
__device__ __forceinline__ uint32_t refine_cut(const Cut& c, const T* sub) {
    uint64_t a = c.above;
    int s = 15;                                                             // sub-bin 15 qualifies: the bin did
    for (; s > 0; --s) {
        a += sub[s];
        if (!((double)a < c.target)) break;
    }
    return (uint32_t)(c.bin << 4 | s);
}

__global__ __launch_bounds__(1024) void sample_truncated_kernel(int64_t* __restrict__ out, const uint16_t* __restrict__ x, int n, int64_t stride,
                                                                 const SampleArgs s, const int32_t* __restrict__ top_ks,
                                                                 const float* __restrict__ top_ps, const AdvanceArgs adv) {
    __shared__ uint32_t cnt[kBins];
    __shared__ unsigned long long wgt[kBins];
    __shared__ uint32_t sub_cnt[16];
    __shared__ unsigned long long sub_wgt[16];
    __shared__ Fold fold;
    const int r = blockIdx.x;
    const uint16_t* row = x + r * stride;
    const RowNoise z = row_noise(s, adv, r);
    const float temp = z.temp;
    // a pass over the row's columns: the row (<= 300 KB) comes from the cache, four ordinary 16-byte loads in flight per thread
    const auto each_column = [&](auto&& f) { for_columns<4, false>(row, n, f); };

    // pass 1: the greedy arg-max
    float best = -INFINITY;
    int bidx = kNoColumn;
    each_column([&](int col, uint32_t bits) { argmax_column(col, bits, best, bidx); });
    block_argmax(best, bidx, fold.arg);

    if (temp > 0.f && best == best) {                                       // workgroup-uniform; a NaN row keeps its lowest NaN column
        const float row_max = best;
        const uint32_t key_max = order_key(__float_as_uint(row_max) >> 16);
        const int top_k = top_ks[r];
        const float top_p = top_ps[r];
        const bool k_on = top_k > 0 && top_k < n, p_on = top_p < 1.f;        // a NaN top_p compares false: off
        uint32_t key_k = 0, key_p = 0;
        if (k_on) {
            // pass 2: columns per bin; the bin of the k-th largest value is the lowest with fewer than k columns above it
#pragma unroll
            for (int j = 0; j < kPerThread; ++j) cnt[threadIdx.x * kPerThread + j] = 0;
            if (threadIdx.x < 16) sub_cnt[threadIdx.x] = 0;
            __syncthreads();
            each_column([&](int, uint32_t bits) { atomicAdd(&cnt[order_key(bits) >> 4], 1u); });
            __syncthreads();
            const Cut c = find_cut(cnt, (double)top_k, false, fold);         // 1 <= k < n: a bin always qualifies
            // pass 3: that bin's 16 values
            each_column([&](int, uint32_t bits) {
                const uint32_t key = order_key(bits);
                if ((int)(key >> 4) == c.bin) atomicAdd(&sub_cnt[key & 15], 1u);
            });
            __syncthreads();
            key_k = refine_cut(c, sub_cnt);
        }
        if (p_on && top_p > 0.f) {
            // pass 4: fixed-point weights of the top-k survivors per bin; the lowest bin with less than top_p * Z above it
            const float scale = kLog2e / temp;
#pragma unroll
            for (int j = 0; j < kPerThread; ++j) wgt[threadIdx.x * kPerThread + j] = 0;
            if (threadIdx.x < 16) sub_wgt[threadIdx.x] = 0;
            __syncthreads();
            each_column([&](int, uint32_t bits) {
                const uint32_t key = order_key(bits);
                if (key < key_k) return;
                const uint64_t w = fixed_weight(bits, row_max, scale);
                if (w) atomicAdd(&wgt[key >> 4], (unsigned long long)w);     // below 2^-41 a weight rounds to nothing
            });
            __syncthreads();
            const Cut c = find_cut(wgt, (double)top_p, true, fold);
            // pass 5: that bin's 16 values
            each_column([&](int, uint32_t bits) {
                const uint32_t key = order_key(bits);
                if ((int)(key >> 4) != c.bin || key < key_k) return;
                const uint64_t w = fixed_weight(bits, row_max, scale);
                if (w) atomicAdd(&sub_wgt[key & 15], (unsigned long long)w);
            });
            __syncthreads();
            key_p = c.bin < 0 ? 0xFFFFu : refine_cut(c, sub_wgt);
        } else if (p_on) {
            key_p = key_max;                                                // top_p <= 0: the largest class only
        }
        uint32_t thr = key_k > key_p ? key_k : key_p;
        thr = thr < key_max ? thr : key_max;                                // the largest class is always kept

        // final pass: the perturbed arg-max of sample_rows_kernel over the kept columns
        const auto kept = [thr](uint32_t bits) { return order_key(bits) >= thr; };
        best = -INFINITY;
        bidx = kNoColumn;
        walk_row<1, false>(row, n,
            [&](int col0, const u32x4& v) { perturbed_argmax_chunk(z, col0, v, kept, best, bidx); },
            [&](int col, uint32_t bits) { perturbed_argmax_column(z, col, bits, kept, best, bidx); });
        __syncthreads();                                                    // pass 1's fold has been read by every thread
        block_argmax(best, bidx, fold.arg);
    }
    if (threadIdx.x == 0) finish_row(out, adv, r, n, bidx);
}

}  // namespace

int launch_sample_truncated(int64_t* out, const void* x, int n_rows, int n, int64_t stride, const SampleArgs& s, const int32_t* top_ks,
                            const float* top_ps, const AdvanceArgs& adv, hipStream_t stream) {
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(sample_truncated_kernel, dim3(n_rows), dim3(kThreads), 0, stream, out, (const uint16_t*)x, n, stride, s, top_ks, top_ps, adv);
    return check_launch("sample_truncated");
}

}  // namespace nvh
