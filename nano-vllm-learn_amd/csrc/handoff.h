// The cross-workgroup hand-off "last arriver merges", stated once.  Its users: the chunked decode kernel
// (decode_chunked.h), the split-key prefill (prefill_splitk.h) and the split-K reducer of the streaming GEMM (linear_stream.hip).
// Work that is split over `live` workgroups ends like this in every one of them:
//   1. every thread stores its share of the workgroup's partial result (a "record") with WRITE-THROUGH stores (sc1: st16 / st_sc1);
//   2. handoff_arrive(): every wave drains its stores (s_waitcnt vmcnt(0)), workgroup barrier, ONE thread takes the unit's ticket
//      (relaxed agent-scope add, executed at the memory side), LDS broadcast, barrier;
//   3. the workgroup whose add returned live - 1 — the last arriver — stores the ticket back to zero behind that barrier, reads all
//      records with L1-BYPASSING loads (sc1: ld16 / ld_sc1) and merges them in split order: the result does not depend on who
//      arrives last.  Everybody else is done.
// Why no release / acquire fence is needed on gfx950, and what the protocol therefore rests on:
//   * an sc1 store is written through the XCD's L2 to the memory side, the one point all XCDs share, and its vmcnt acknowledgement
//     comes back when it is there: after vmcnt(0) in EVERY storing wave plus the barrier, the whole record is globally visible before
//     the ticket add is even issued.  The drain is inline asm: the compiler can drop a builtin wait it believes redundant;
//   * the ticket is a read-modify-write on one unsharded address, executed at the memory side: the adds of a unit's workgroups are
//     totally ordered there, each issued after its workgroup's record is visible, so the add that returns live - 1 is ordered after
//     every other workgroup's record;
//   * the last arriver's loads are issued after its add has RETURNED (data dependence through the LDS broadcast and the barrier that the
//     ticket holder joins), bypass the CU's L1 (which no other CU's store ever refreshes) and so read the written-through bytes;
//   * records and tickets live in hipMalloc memory and are accessed as 4- or 16-byte items; no workgroup ever waits for another
//     (no spin), so the protocol sets no condition on where or when a unit's workgroups run;
//   * compiler side: stores, add and loads are atomics or buffer intrinsics, kept in program order by the "memory"-clobbering asm
//     drain and the barriers between them.
// -DNVH_HANDOFF_FENCES (cross-check build, never shipped; tools/probes/run_fence_crosscheck.sh) turns ALL users into the HIP memory
// model's textbook form: plain stores, an agent-scope release fence before the ticket, an agent-scope acquire fence behind it, plain
// loads.  The parity tests run against that build and its results are compared bit for bit with the shipped form's.  The fences are a
// whole-L2 write-back + invalidate under a full launch: +3-4 us per decode attention call, 4-5 us per split-K GEMM.
#pragma once
#include <type_traits>

#include "common.h"

namespace nvh {

// ---- the flavour switch: this is the only place that tests NVH_HANDOFF_FENCES
#ifdef NVH_HANDOFF_FENCES
#define NVH_HANDOFF_RELEASE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent")
#define NVH_HANDOFF_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
constexpr bool kHandoffFences = true;
constexpr int kRecAux = 0;
#else
#define NVH_HANDOFF_RELEASE() do {} while (0)
#define NVH_HANDOFF_ACQUIRE() do {} while (0)
constexpr bool kHandoffFences = false;
constexpr int kRecAux = 16;                               // gfx940+ cache-policy bits of the buffer intrinsics: 1 = sc0, 2 = nt, 16 = sc1
#endif

// ---- record access, 16-byte items: buffer_store_dwordx4 / buffer_load_dwordx4 through a raw buffer descriptor of the unit's record
// group (the compiler sees them as memory operations and counts their vmcnt, which inline-asm global_* accesses would leave to
// hand-placed waits).  A write-through store is one fabric write per LANE whatever its width: 16-byte items are a quarter of the writes
// of dwords.  Byte offsets; the caller's descriptor spans exactly the group, so out-of-range accesses cannot happen.
// (rec_buffer itself is protocol-neutral: a raw descriptor of any wave-uniform byte range.  The fused decode launch also reads q and the
// newest K / V row through one, with its own always-sc1 load: that is the producer -> consumer spin protocol, not this hand-off.)
typedef __amdgpu_buffer_rsrc_t RecBuf;
__device__ __forceinline__ RecBuf rec_buffer(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);   // raw buffer, 32-bit data format word of gfx9
}
__device__ __forceinline__ void st16(RecBuf rb, uint32_t byte_off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rb, (int)byte_off, 0, kRecAux);
}
__device__ __forceinline__ f32x4 ld16(RecBuf rb, uint32_t byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (int)byte_off, 0, kRecAux));
}
// ---- record access, 4-byte items (the GEMM's partials): relaxed agent-scope atomics compile to global_store_dword / global_load_dword sc1
__device__ __forceinline__ void st_sc1(float* p, float v) {
    if constexpr (kHandoffFences) *p = v;
    else __hip_atomic_store(reinterpret_cast<unsigned*>(p), __builtin_bit_cast(unsigned, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p) {
    if constexpr (kHandoffFences) return *p;
    else return __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// Step 2 and the first half of step 3.  Called by every thread of the workgroup behind its record stores; true in the last of the
// `live` arrivers only (workgroup-uniform).  lds_ticket: one LDS word nobody else uses across the call; ticket: the unit's counter,
// zero before the launch and left zero by it — a pointer, or a callable that forms the pointer: it is then evaluated inside thread 0's
// two blocks only, so that its address arithmetic and registers stay off every other wave's way to the barrier.
// ONE TICKET PER 128-BYTE LINE (kTicketStride words apart): the memory side executes the adds on one line one after the other (~12 ns
// each); with dense tickets the 16-32 units that share a line made every unit's last arriver queue behind all their adds.
template <typename Ticket>
__device__ __forceinline__ bool handoff_arrive(unsigned* lds_ticket, Ticket ticket, int live) {
    auto counter = [&]() -> unsigned* {
        if constexpr (std::is_pointer_v<Ticket>) return ticket;
        else return ticket();
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's share of the record has reached the memory side
    __syncthreads();                                             // ... and every wave's
    if (threadIdx.x == 0) {
        NVH_HANDOFF_RELEASE();
        const unsigned drawn = __hip_atomic_fetch_add(counter(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        NVH_HANDOFF_ACQUIRE();
        *lds_ticket = drawn;
    }
    __syncthreads();
    if (*lds_ticket != (unsigned)live - 1) return false;
    // (the empty statement keeps the early return a branch of its own.  Without it hipcc folds the return into the reset's condition
    // and every kernel of linear_stream.hip compiles differently from the hand-written form this replaced (compared per kernel in the assembly: all 208
    // differ, some by hundreds of lines); with it half are identical and half differ by one scalar instruction)
    asm volatile("" ::: "memory");
    // The last arriver zeroes the ticket for the next launch.  RESET BEHIND THE BARRIER, not next to the add: the barrier's wait
    // would hold the whole workgroup until this store is acknowledged (~0.2 us on the launch's critical path); here it completes
    // under the record loads (the kernel's end waits for it like for the output stores).
    if (threadIdx.x == 0) __hip_atomic_store(counter(), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// The second half of step 3 for (max, sum, O) records of an online softmax (max in the log2 domain, O un-normalised): merges records
// 0 .. live - 1 in that order into (acc, L).  A thread owns NV 16-byte items of O per record plus the record's {max, sum, -, -} item;
// ml_off(c) and o_off(c, t) give their byte offsets in `rb` for record c.  Records are requested CB at a time.
// EMPTY_ROWS: a row that no record has seen a key for (every max = -inf) can occur; its exp2 arguments are kept finite and its sum stays 0.
template <int CB, int NV, bool EMPTY_ROWS, typename MlOff, typename OOff>
__device__ __forceinline__ void handoff_merge(RecBuf rb, int live, MlOff ml_off, OOff o_off, f32x4 (&acc)[NV], float& L) {
    float M = -INFINITY;
    L = 0.f;
#pragma unroll
    for (int t = 0; t < NV; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < live; c0 += CB) {
        f32x4 ml[CB], av[CB][NV];
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            const int c = c0 + i < live ? c0 + i : live - 1;     // (a batch's surplus slots repeat the last record and are skipped below)
            ml[i] = ld16(rb, ml_off(c));
#pragma unroll
            for (int t = 0; t < NV; ++t) av[i][t] = ld16(rb, o_off(c, t));
        }
        // EVERY LOAD OF THE BATCH IS ISSUED HERE, before any is consumed: left alone, hipcc sank the last load of an 8-wide batch into
        // the `c0 + i < live` block that uses it — behind the wait for the other fifteen, a second memory-side round trip (0.6 us) in
        // the last arriver of every unit split over 5-8 workgroups (stamped: 1.24 us for this step of the decode kernel at 7/1/128)
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            asm volatile("" : "+v"(ml[i]));
#pragma unroll
            for (int t = 0; t < NV; ++t) asm volatile("" : "+v"(av[i][t]));
        }
        float Mc = M;
#pragma unroll
        for (int i = 0; i < CB; ++i)
            if (c0 + i < live) Mc = fmaxf(Mc, ml[i][0]);
        const float Mu = EMPTY_ROWS && Mc == -INFINITY ? 0.f : Mc;
        const float fo = fast_exp2(M - Mu);                      // M = -inf on the first batch -> 0
        L *= fo;
#pragma unroll
        for (int t = 0; t < NV; ++t) acc[t] *= fo;
#pragma unroll
        for (int i = 0; i < CB; ++i)
            if (c0 + i < live) {
                const float f = fast_exp2(ml[i][0] - Mu);
                L = fmaf(ml[i][1], f, L);
#pragma unroll
                for (int t = 0; t < NV; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[t][j] = fmaf(av[i][t][j], f, acc[t][j]);
            }
        M = Mc;
    }
}

}  // namespace nvh
