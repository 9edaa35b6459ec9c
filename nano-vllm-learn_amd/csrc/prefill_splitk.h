// Split-key prefill: the cross-workgroup hand-off of a q-tile whose key tiles are shared out over several workgroups (included by prefill_mfma.hip).
// The tiled body runs unchanged on each split's contiguous tile range; what differs is the end: with more than one live split a workgroup does not
// normalise and write `out` but publishes its partial — un-normalised O^T (fp32), running max (log2 domain) and row sum per query row — as a record,
// takes the q-tile's ticket, and the LAST ARRIVER merges all live records in split order, so the result does not depend on who arrives last.
// The protocol is the decode kernel's (decode_chunked.h): 16-byte write-through (sc1) stores through a raw buffer descriptor of the
// q-tile's record group, s_waitcnt vmcnt(0) in every wave, workgroup barrier, ONE relaxed agent-scope add on the q-tile's own ticket line, LDS broadcast +
// barrier, then 16-byte L1-bypassing (sc1) loads.  No fence, no spin-wait; the last arriver stores the ticket back to zero behind the barrier.
// Record: 64 rows of [D floats of O | max | sum | 0 | 0] = 64 * (D + 4) * 4 bytes, a multiple of 256 (no line shared between two workgroups' records).
// A thread writes exactly the elements its MFMA accumulators hold (row = its query column, 4 contiguous dims per 16-dim tile) and the merging
// workgroup's thread reads the same elements back: no transpose, no LDS.
#pragma once
#include "common.h"
#include "kernels.h"

namespace nvh {

namespace {

constexpr int kSkRecAux = 16;                // gfx940+ cache-policy bits of the buffer intrinsics: 16 = sc1
typedef __amdgpu_buffer_rsrc_t SkRecBuf;

// which key tiles split `split` of `key_splits` walks when the q-tile sees `n_tiles`: live = min(key_splits, n_tiles) splits share them in contiguous,
// balanced ranges (sizes differ by at most one).  Every workgroup of the q-tile computes the same partition; splits at or past `live` have nothing to do.
__device__ __forceinline__ void splitk_range(int n_tiles, int key_splits, int split, int& live, int& t_beg, int& t_end) {
    live = n_tiles < key_splits ? n_tiles : key_splits;
    if (live < 1) live = 1;                  // (a q-tile that sees no key: split 0 writes its zero rows directly)
    t_beg = (int)((int64_t)split * n_tiles / live);
    t_end = (int)((int64_t)(split + 1) * n_tiles / live);
}

// Publishes this workgroup's partial of q-tile `unit` and returns false, or — in the last arriver — returns true with (o, l) replaced by the merge of all
// `live` records in split order (m is consumed).  row: the thread's query row in the tile (16 * wave + lane % 16), lg: its lane group (lane / 16);
// l: the row sum already folded over the four lane groups.  Called by all 256 threads after the tile loop's last barrier: the LDS images are dead,
// their first word carries the ticket.
template <int D>
__device__ __forceinline__ bool splitk_handoff(const PrefillArgs& a, unsigned char* const lds, const int unit, const int split, const int live,
                                               const int row, const int lg, f32x4 (&o)[D / 16], const float m, float& l) {
    constexpr int DT = D / 16;
    constexpr uint32_t ROWB = (D + 4) * 4, REC = 64 * ROWB;
    constexpr int CB = D == 64 ? 4 : 2;      // records requested together: CB * (DT + 1) 16-byte loads in flight per thread
    static_assert(REC == splitk_record_bytes(D), "the plan's record size");
    float* const recs = a.sk_records + (int64_t)unit * a.key_splits * (REC / 4);
    const SkRecBuf rb = __builtin_amdgcn_make_buffer_rsrc(recs, 0, (int)(live * REC), 0x00020000);   // spans exactly the live records of this q-tile
    const uint32_t mine = (uint32_t)split * REC + (uint32_t)row * ROWB, dcol = 16 * lg;
#pragma unroll
    for (int t = 0; t < DT; ++t) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[t]), rb, (int)(mine + 64 * t + dcol), 0, kSkRecAux);
    if (lg == 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{m, l, 0.f, 0.f}), rb, (int)(mine + 4 * D), 0, kSkRecAux);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's share of the record has reached the memory side
    __syncthreads();                                             // ... and every wave's
    unsigned* const lds_ticket = reinterpret_cast<unsigned*>(lds);
    unsigned* const ctr = a.sk_tickets + (int64_t)unit * kTicketStride;
    if (threadIdx.x == 0) {
        *lds_ticket = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (*lds_ticket != (unsigned)live - 1) return false;         // workgroup-uniform
    if (threadIdx.x == 0) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch; completes under the record loads
    const uint32_t rowoff = (uint32_t)row * ROWB;
    float M = -INFINITY, L = 0.f;
    f32x4 acc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < live; c0 += CB) {
        f32x4 ml[CB], av[CB][DT];
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            const uint32_t r = (uint32_t)(c0 + i < live ? c0 + i : live - 1) * REC + rowoff;      // (a batch's surplus slots repeat the last record and are skipped below)
            ml[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (int)(r + 4 * D), 0, kSkRecAux));
#pragma unroll
            for (int t = 0; t < DT; ++t) av[i][t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (int)(r + 64 * t + dcol), 0, kSkRecAux));
        }
        // every load of the batch is issued before any is consumed (see the same statement in decode_chunked.h)
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            asm volatile("" : "+v"(ml[i]));
#pragma unroll
            for (int t = 0; t < DT; ++t) asm volatile("" : "+v"(av[i][t]));
        }
        float Mc = M;
#pragma unroll
        for (int i = 0; i < CB; ++i)
            if (c0 + i < live) Mc = fmaxf(Mc, ml[i][0]);
        const float Mu = Mc == -INFINITY ? 0.f : Mc;             // a row no split has seen a key for: keep exp2 finite (its sum stays 0)
        const float fo = fast_exp2(M - Mu);                      // M = -inf on the first batch -> 0
        L *= fo;
#pragma unroll
        for (int t = 0; t < DT; ++t) acc[t] *= fo;
#pragma unroll
        for (int i = 0; i < CB; ++i)
            if (c0 + i < live) {
                const float f = fast_exp2(ml[i][0] - Mu);
                L = fmaf(ml[i][1], f, L);
#pragma unroll
                for (int t = 0; t < DT; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[t][j] = fmaf(av[i][t][j], f, acc[t][j]);
            }
        M = Mc;
    }
    l = L;
#pragma unroll
    for (int t = 0; t < DT; ++t) o[t] = acc[t];
    return true;
}

}  // namespace

}  // namespace nvh
