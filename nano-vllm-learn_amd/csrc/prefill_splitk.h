// Split-key prefill: the cross-workgroup hand-off of a q-tile whose key tiles are shared out over several workgroups (included by prefill_mfma.hip).
// The tiled body runs unchanged on each split's contiguous tile range; what differs is the end: with more than one live split a workgroup does not
// normalise and write `out` but publishes its partial — un-normalised O^T (fp32), running max (log2 domain) and row sum per query row — as a record,
// takes the q-tile's ticket, and the LAST ARRIVER merges all live records in split order, so the result does not depend on who arrives last.
// The protocol and the merge are handoff.h's; this file lays out the record.
// Record: 64 rows of [D floats of O | max | sum | 0 | 0] = 64 * (D + 4) * 4 bytes, a multiple of 256 (no line shared between two workgroups' records).
// A thread writes exactly the elements its MFMA accumulators hold (row = its query column, 4 contiguous dims per 16-dim tile) and the merging
// workgroup's thread reads the same elements back: no transpose, no LDS.
#pragma once
#include "common.h"
#include "handoff.h"
#include "kernels.h"

namespace nvh {

namespace {

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
    const RecBuf rb = rec_buffer(a.sk_records + (int64_t)unit * a.key_splits * (REC / 4), (uint32_t)(live * REC));   // spans exactly the live records of this q-tile
    const uint32_t rowoff = (uint32_t)row * ROWB, mine = (uint32_t)split * REC + rowoff, dcol = 16 * lg;
#pragma unroll
    for (int t = 0; t < DT; ++t) st16(rb, mine + 64 * t + dcol, o[t]);
    if (lg == 0) st16(rb, mine + 4 * D, f32x4{m, l, 0.f, 0.f});
    if (!handoff_arrive(reinterpret_cast<unsigned*>(lds), a.sk_tickets + (int64_t)unit * kTicketStride, live)) return false;   // workgroup-uniform
    // a row that no split has seen a key for can occur here (EMPTY_ROWS): its sum stays 0
    handoff_merge<CB, DT, true>(rb, live, [&](int c) { return (uint32_t)c * REC + rowoff + 4 * D; },
                                [&](int c, int t) { return (uint32_t)c * REC + rowoff + 64 * t + dcol; }, o, l);
    return true;
}

}  // namespace

}  // namespace nvh
