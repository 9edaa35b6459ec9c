// Token choice, device side: the pieces every kernel that picks a row's next token is made of, each stated once.
//   block_argmax      the workgroup arg-max fold in argmax_better's order (NaN first, value desc, column asc)
//   walk_row          a bf16 logits row as 16-byte chunks of 8 columns plus the n % 8 tail; for_columns is its per-column form
//   argmax_chunk / perturbed_argmax_chunk / perturbed_argmax_column
//                     what a thread does with a chunk: the greedy fold, or the Gumbel-max of sample_noise.h over the kept columns
//   load_row_meta / store_row_advance / advance_row
//                     the between-steps bookkeeping of a decode session, as loads and as stores
//   finish_row        the end of a row: clamp, write, advance
// Users: sample.hip (greedy and sampled rows), sample_truncated.hip, argmax_candidates_kernel (layer_ops.hip).  The candidate fold
// inside linear_stream.hip's GEMM epilogue shares argmax_better and sample_score only.
#pragma once
#include "common.h"
#include "kernels.h"

namespace nvh {

constexpr int kRowThreads = 1024;                   // threads of a workgroup that walks a logits row

// A thread's running choice starts at (-INFINITY, kNoColumn): it loses to every real (value, column).
constexpr int kNoColumn = 0x7fffffff;

// (v, col) replaces the running choice if argmax_better says so.  Written as two selects: as a branch around two moves the
// compiler keeps the branch, which costs the greedy kernel 7 % at 151936 columns.
__device__ __forceinline__ void argmax_take(float v, int col, float& best, int& bidx) {
    const bool better = argmax_better(v, col, best, bidx);
    best = better ? v : best;
    bidx = better ? col : bidx;
}

template <int WAVES>
struct ArgmaxFold { float v[WAVES]; int i[WAVES]; };         // LDS scratch: one slot per wave

// arg-max over a workgroup of WAVES waves, the result in every thread (a caller that uses it in thread 0 alone leaves the scan
// of the slots to that thread: the reads sink into its branch).  One barrier.  A second fold over the same scratch needs a
// barrier of the caller's between the first fold's reads and this one's writes.
template <int WAVES>
__device__ __forceinline__ void block_argmax(float& best, int& bidx, ArgmaxFold<WAVES>& f) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bidx, off, 64);
        argmax_take(ov, oi, best, bidx);
    }
    if ((threadIdx.x & 63) == 0) { f.v[threadIdx.x >> 6] = best; f.i[threadIdx.x >> 6] = bidx; }
    __syncthreads();
    best = f.v[0]; bidx = f.i[0];
    for (int w = 1; w < WAVES; ++w) argmax_take(f.v[w], f.i[w], best, bidx);
}

// chunk(first column, the 8 packed bf16 of a 16-byte load) for every full chunk of the row, column(column, bf16 bits) for the
// n % 8 tail (a column per thread).  kAhead loads are in flight per thread: a pass that re-reads a cached row waits for its loads'
// latency (19 round trips at 151936 columns), not for their bytes.  kNonTemporal: the row is read once and not again.
template <int kAhead, bool kNonTemporal, typename Chunk, typename Column>
__device__ __forceinline__ void walk_row(const uint16_t* __restrict__ row, int n, Chunk&& chunk, Column&& column) {
    const int chunks = n / 8;
    for (int c0 = threadIdx.x; c0 < chunks; c0 += kAhead * kRowThreads) {
        u32x4 v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            if (c0 + u * kRowThreads >= chunks) continue;
            const u32x4* p = reinterpret_cast<const u32x4*>(row + (c0 + u * kRowThreads) * 8);
            v[u] = kNonTemporal ? __builtin_nontemporal_load(p) : *p;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int c = c0 + u * kRowThreads;
            if (c >= chunks) break;
            chunk(c * 8, v[u]);
        }
    }
    for (int i = chunks * 8 + threadIdx.x; i < n; i += kRowThreads) column(i, (uint32_t)row[i]);
}

// f(column, bf16 bits) for every column of the row, in ascending order within a thread
template <int kAhead, bool kNonTemporal, typename F>
__device__ __forceinline__ void for_columns(const uint16_t* __restrict__ row, int n, F&& f) {
    walk_row<kAhead, kNonTemporal>(row, n, [&](int col0, const u32x4& v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { f(col0 + 2 * k, v[k] & 0xFFFFu); f(col0 + 2 * k + 1, v[k] >> 16); }
    }, f);
}

__device__ __forceinline__ void argmax_column(int col, uint32_t bits, float& best, int& bidx) {
    argmax_take(bf16_lo(bits), col, best, bidx);
}

__device__ __forceinline__ void argmax_chunk(int col0, const u32x4& v, float& best, int& bidx) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        argmax_take(bf16_lo(v[k]), col0 + 2 * k, best, bidx);
        argmax_take(bf16_hi(v[k]), col0 + 2 * k + 1, best, bidx);
    }
}

struct RowNoise { uint64_t seed; uint32_t key; uint64_t step; float temp; };   // what the noise of one row is a function of

// s.steps null: the counter is the session's row_steps, read when the row starts (the advance increments it behind the fold's barrier)
__device__ __forceinline__ RowNoise row_noise(const SampleArgs& s, const AdvanceArgs& adv, int row) {
    return RowNoise{s.seed, s.row_keys[row], (uint64_t)(s.steps ? s.steps[row] : adv.row_steps[row]), s.temperatures[row]};
}

// The perturbed arg-max over a chunk's columns with keep(bf16 bits): four columns share one sample_bits4 call, and a half of the
// chunk with no kept column makes none.
template <typename Keep>
__device__ __forceinline__ void perturbed_argmax_chunk(const RowNoise& z, int col0, const u32x4& v, Keep&& keep, float& best, int& bidx) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t bits[4] = {v[2 * h] & 0xFFFFu, v[2 * h] >> 16, v[2 * h + 1] & 0xFFFFu, v[2 * h + 1] >> 16};
        bool kept[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) { kept[k] = keep(bits[k]); any |= kept[k]; }
        if (!any) continue;
        uint32_t w[4];
        sample_bits4(z.seed, z.key, z.step, (uint32_t)(col0 + 4 * h), w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float sc = sample_score(bf16_lo(bits[k]), z.temp, gumbel_from_bits(w[k]));
            if (kept[k]) argmax_take(sc, col0 + 4 * h + k, best, bidx);
        }
    }
}

template <typename Keep>
__device__ __forceinline__ void perturbed_argmax_column(const RowNoise& z, int col, uint32_t bits, Keep&& keep, float& best, int& bidx) {
    if (!keep(bits)) return;
    const float sc = sample_score(bf16_lo(bits), z.temp, sample_gumbel(z.seed, z.key, z.step, (uint32_t)col));
    argmax_take(sc, col, best, bidx);
}

// ---- scheduler.postprocess (append the token) + prepare_decode for the NEXT step (engine/model_runner.py:244-269), on the device:
// the row's workgroup owns the row's metadata, so there is nothing to synchronise.  Two halves, so that a kernel with other loads
// to wait for can issue the metadata loads early and keep the bookkeeping behind the choice to stores only.
struct RowMeta {
    int ctx;            // context_lens[row]; 0: a padding row (slot -1), which stays as it is
    int blk;            // the block that holds the token the next step stores (index ctx = new_ctx - 1)
    int64_t steps, pos;
    int64_t tok;        // the row's current input token (what a padding row keeps)
};

__device__ __forceinline__ RowMeta load_row_meta(const AdvanceArgs& adv, int row) {
    RowMeta m{adv.context_lens[row], 0, adv.row_steps[row], adv.positions[row], adv.input_ids[row]};
    if (m.ctx > 0) m.blk = adv.block_tables[row * adv.bt_stride + m.ctx / adv.block_size];
    return m;
}

__device__ __forceinline__ void store_row_advance(const AdvanceArgs& adv, int row, const RowMeta& m, int token) {
    if (m.ctx > 0) {
        adv.tokens_log[m.steps * adv.log_stride + row] = token;
        adv.row_steps[row] = m.steps + 1;
        adv.input_ids[row] = token;
        adv.positions[row] = m.pos + 1;
        adv.context_lens[row] = m.ctx + 1;
        adv.slot_mapping[row] = m.blk * adv.block_size + m.ctx % adv.block_size;
    }
}

__device__ __forceinline__ void advance_row(const AdvanceArgs& adv, int row, int token) {
    store_row_advance(adv, row, load_row_meta(adv, row), token);
}

// the end of a row, in the one thread that holds the fold's result
__device__ __forceinline__ void finish_row(int64_t* __restrict__ out, const AdvanceArgs& adv, int row, int n, int bidx) {
    bidx = bidx < 0 ? 0 : (bidx >= n ? n - 1 : bidx);                       // n >= 1 (host): always a valid column
    if (out) out[row] = bidx;
    if (adv.input_ids) advance_row(adv, row, bidx);
}

}  // namespace nvh
