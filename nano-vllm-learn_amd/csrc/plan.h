// The routing plan: which kernel instantiation an attention call launches is decided HERE, once, and nowhere else.
// api.hip asks for a plan, the launchers (prefill_mfma.hip, paged_decode.hip, qkv_attend.hip) execute it without looking at a shape,
// nvh_plan_prefill / nvh_plan_decode report it to the host (ops.py allocates scratch from it, tests/test_plan_cpu.py pins it).
// Plain host C++ without HIP: pure functions of their arguments (the CU count is one of them), buildable with any host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nvh_attn.h"

// ---- rule thresholds (A/B builds change them with -D)
#ifndef NVH_PREFILL_QT2_FROM
#define NVH_PREFILL_QT2_FROM 2048            // D = 64: two 16-row sub-tiles per wave from this many query rows on
#endif
#ifndef NVH_PREFILL_QT2_FROM_PV16
#define NVH_PREFILL_QT2_FROM_PV16 512        // ... in the fp16 P V form: its two-sub-tile body fits 128 registers = 4 waves per SIMD (same-box A/B against 2048:
                                             // S = 512 42.5 -> 40.5 us, S = 1024 62.8 -> 58.8, S = 1536 77.8 -> 74.0; profiles/r03_prefill_qt2_pv16_ab.txt)
#endif
#ifndef NVH_D128_HALF_RULE
#define NVH_D128_HALF_RULE(chunks) ((chunks) <= 8)   // the chunk counts at which head_dim 128 takes 64-token passes by default.  Measured (same box,
                             // B = 32, 64- against 128-token passes, ctx 1034 / 1536 / 2048 / 3072): 7/1/128 (8 chunks) 8.02 / 8.81 / 9.95 / 12.76 against
                             // 8.25 / 9.27 / 10.23 / 12.74 us; 28/4/128 (2 chunks) -3 % everywhere; 16/8/128 (1 chunk) -0.2 .. -1 %; 7/1/128 at B = 64 (4 chunks)
                             // -1.3 %, B = 16 (16 chunks) +1.3 %, B = 8 (32 chunks) +9 %: with 128-token passes twelve passes over eight chunks leave half the
                             // workgroups with twice the tokens of the others; with many chunks the finer passes only add per-pass work
#endif
#ifndef NVH_D128_WAVES
#define NVH_D128_WAVES 4     // waves per workgroup of the chunked kernel at head_dim 128 when the caller does not choose (4 or 8).
                             // With 4-byte records 8 waves won (7/1/128 ctx 1536: 11.1 vs 12.1 us); since the records move as 16-byte items
                             // 4 waves (32-token tiles, the k = 32 MFMA) win everywhere: 7/1/128 9.2 vs 9.6, 28/4/128 19.8 vs 20.6, 16/8/128 33.3 vs 34.0
#endif

namespace nvh {

// ============================================================================================ prefill
constexpr int kPv16MinKeys = 512;            // fp16 P V by default from this many keys per sequence on (40.5 vs 42.0 us at 32 x 512; below, the conversion
                                             // launch costs what it saves); == ops.PV16_MIN_KEYS
constexpr int kShortMaxKeys = 128;           // the short-sequence kernel keeps two 64-key tiles resident (256 keys with four measured slower than the tiled kernel)
constexpr int kShortMinPairs = 128;          // fewer (sequence, kv head) pairs: the tiled kernel spreads heads and q-tiles over the CUs
constexpr int kPv16GroupRows = 64;           // rows per range flag of the bf16 -> fp16 conversion (one conversion workgroup per group)

struct PrefillRequest { int kernel, short_waves, pv, out_f32, paged; };   // NVH_PREFILL_*; 0 / 8 / 16; NVH_PV_NEVER / ALWAYS / AUTO; paged: a block table
struct PrefillShape { int batch, max_seqlen_q, max_seqlen_k, total_k, kvh, hd; };
struct PrefillPlan {
    int error = 0;               // 0 or NVH_E_SHAPE, with `message`
    const char* message = "";
    int kernel = NVH_PLAN_TILED; // NVH_PLAN_SHORT / NVH_PLAN_TILED
    int paged = 0;
    int q_subtiles = 1;          // tiled kernel: 16-row query sub-tiles per wave (1 or 2)
    int short_waves = 0;         // short kernel: waves per workgroup actually launched (8 or 16); 0 for the tiled kernel
    int pv = NVH_PV_EXACT;       // NVH_PV_EXACT / F16_SCRATCH / F16_IN_KERNEL / F16_HANDED_IN
    size_t scratch_bytes = 0;    // F16_SCRATCH: what the call needs
    int key_splits = 1;          // > 1: the split-key form of the tiled kernel (plan_prefill_splitk), workgroups per q-tile
};

// nvh_prefill_varlen_pv16 scratch: one int32 range flag per kPv16GroupRows rows (padded to 256 bytes), then the fp16 rows
inline size_t pv16_header_bytes(int total_k) { return ((size_t)((total_k + kPv16GroupRows - 1) / kPv16GroupRows) * 4 + 255) / 256 * 256; }
inline size_t pv16_scratch_bytes(int total_k, int kvh, int hd) {
    if (total_k <= 0 || kvh <= 0 || hd <= 0) return 0;
    return pv16_header_bytes(total_k) + (size_t)total_k * kvh * hd * 2;
}

inline PrefillPlan plan_prefill(const PrefillRequest& r, const PrefillShape& s, int cus) {
    (void)cus;                                                   // (no prefill rule reads it today: the pair threshold is a constant)
    PrefillPlan p;
    p.paged = r.paged;
    const int64_t pairs = (int64_t)s.batch * s.kvh;
    const bool variant = r.kernel != NVH_PREFILL_AUTO || r.short_waves != 0;
    if (r.kernel == NVH_PREFILL_TILED_F16V && r.paged) { p.error = NVH_E_SHAPE; p.message = "the fp16-V measurement variant never reads a paged cache"; return p; }
    if (r.pv == NVH_PV_ALWAYS && r.paged) { p.error = NVH_E_SHAPE; p.message = "fp16 P V not with a block table (V is read from the cache)"; return p; }
    if (r.pv == NVH_PV_ALWAYS && variant && r.kernel != NVH_PREFILL_TILED_F16V) {
        p.error = NVH_E_SHAPE; p.message = "fp16 P V goes with the default kernel choice"; return p;
    }
    // ---- which kernel.  The short-sequence kernel: every key of a sequence resident in LDS, one workgroup per (sequence, kv head).
    // NVH_PREFILL_TILED / _F16V: never; _SHORT: whenever the shape allows (tests); AUTO: when it also fills the chip
    const bool short_fits = !r.paged && s.max_seqlen_k <= kShortMaxKeys && s.max_seqlen_q <= s.max_seqlen_k;
    bool take_short = false;
    if (r.kernel == NVH_PREFILL_SHORT) {
        if (!short_fits) { p.error = NVH_E_SHAPE; p.message = "the short-sequence kernel needs max_seqlen_q <= max_seqlen_k <= 128 and no block table"; return p; }
        take_short = true;
    } else if (r.kernel == NVH_PREFILL_AUTO) {
        take_short = short_fits && pairs >= kShortMinPairs;
    }
    // ---- which P V form.  The short kernel converts its resident V images itself at head_dim 64 and more than one key tile (below, the
    // conversion costs what it saves); the tiled kernel reads an fp16 copy of V made by a launch of its own.
    const bool in_kernel = take_short && s.hd == 64 && s.max_seqlen_k > 64;
    bool fp16 = r.pv == NVH_PV_ALWAYS;
    // AUTO: where it pays and is invisible: bf16 output (whose own rounding is 8x coarser than P's), packed rows, the default kernel choice
    if (r.pv == NVH_PV_AUTO) fp16 = !r.out_f32 && !r.paged && !variant && (s.max_seqlen_k >= kPv16MinKeys || in_kernel);
    if (r.kernel == NVH_PREFILL_TILED_F16V) p.pv = NVH_PV_F16_HANDED_IN;
    else if (!fp16) p.pv = NVH_PV_EXACT;
    else if (take_short) p.pv = in_kernel ? NVH_PV_F16_IN_KERNEL : NVH_PV_EXACT;
    else p.pv = NVH_PV_F16_SCRATCH;
    if (p.pv == NVH_PV_F16_SCRATCH) p.scratch_bytes = pv16_scratch_bytes(s.total_k, s.kvh, s.hd);
    if (take_short) {
        p.kernel = NVH_PLAN_SHORT;
        // a wave's tile is a long dependent chain (QK -> max -> exp2 -> hi/lo -> PV): four waves per SIMD to fill it where the registers allow
        // (measured, Qwen2-0.5B heads, S = 128: 256 workgroups 22.7 us with 16 waves against 25.2 with 8; 512 workgroups, two per CU,
        // 37.4 us with 8 against 41.9 with 16; the tiled kernel 28.3 / 56)
#ifdef NVH_SHORT_FORCE_WAVES                  // A/B builds
        const int waves = r.short_waves ? r.short_waves : NVH_SHORT_FORCE_WAVES;
#else
        const int waves = r.short_waves ? r.short_waves : (pairs >= 384 ? 8 : 16);
#endif
        p.short_waves = s.hd == 64 && waves == 16 ? 16 : 8;      // head_dim 128 has the 8-wave instantiation only, whatever was asked
        return p;
    }
    p.kernel = NVH_PLAN_TILED;
    if (s.hd == 128) p.q_subtiles = s.max_seqlen_q > 128 ? 2 : 1;
    else p.q_subtiles = s.max_seqlen_q >= (p.pv == NVH_PV_F16_SCRATCH ? NVH_PREFILL_QT2_FROM_PV16 : NVH_PREFILL_QT2_FROM) ? 2 : 1;
    return p;
}

// ---- split-key prefill (nvh_prefill_varlen_splitk): workgroups per (sequence, head, 64-row q-tile), each walking a contiguous share of the key tiles
// the q-tile can see.  The tiled kernel gives a q-tile ONE workgroup: few query rows against a long cached prefix leave most CUs idle.
constexpr int kSplitkTileKeys = 64;          // keys per tile and query rows per q-tile of the split form (prefill_mfma.hip asserts it)
constexpr int kSplitkMaxSplits = 16;         // absolute cap: records the last arriver of a q-tile merges
constexpr int kSplitkTargetPerCu = 2;        // workgroups per CU the split grid is brought towards (floor, never beyond).  Measured, graph-replayed calls, us, same box,
                                             // key_splits 1 / 2 / 3 / 4 / 6 / 8 / 12 / 16 (profiles/prefill_splitk_ab.txt):
                                             //   14/2/64 8 x 128 vs 2048 (224 q-tiles): 33.4 / 28.5 / 28.9 / 31.2 / 38.0 / 46.3 / 62.2 / 93.7 -> 2 (448 workgroups)
                                             //   14/2/64 4 x 512 vs 4096 (448 q-tiles): 72.9 / 72.6 / 75.3 / 76.4 / 89.0 / 104 / 148 / 231   -> 1 (nothing to gain at 1.75 per CU)
constexpr int kSplitkMinTiles = 8;           // key tiles a split keeps at least: below, the record round trip outweighs the shorter walk
                                             //   14/2/64 1 x 64 vs 4096 (14 q-tiles, 64 tiles): 62.2 / 35.9 / 26.9 / 21.9 / 18.8 / 16.8 / 16.6 / 17.8 -> 8 (flat from 8 to 12)
                                             //   14/2/64 1 x 16 vs 4096:                        61.5 / 35.3 / 26.4 / 21.6 / 18.4 / 16.5 / 16.3 / 17.6 -> 8

inline int prefill_splitk_units(int batch, int max_seqlen_q, int h) {
    if (batch <= 0 || max_seqlen_q <= 0 || h <= 0) return 0;
    const int64_t u = (int64_t)batch * h * ((max_seqlen_q + kSplitkTileKeys - 1) / kSplitkTileKeys);
    return u > INT32_MAX ? INT32_MAX : (int)u;
}

// key splits of a prefill call; `forced` > 0 (tests and A/B runs) overrides the rule, clamped to the key tiles of max_seqlen_k and the cap.
// ticket_units: q-tiles the workspace header has tickets for (kSplitkTicketUnits)
inline int prefill_key_splits(int forced, int batch, int max_seqlen_q, int max_seqlen_k, int h, int hd, int ticket_units, int cus) {
    (void)hd;
    const int units = prefill_splitk_units(batch, max_seqlen_q, h);
    const int tiles = (max_seqlen_k + kSplitkTileKeys - 1) / kSplitkTileKeys;
    if (units < 1 || tiles < 2 || units > ticket_units) return 1;
    int s;
    if (forced > 0) {
        s = forced;
    } else {
        if (units >= 2 * (int64_t)cus) return 1;                 // the unsplit grid already gives every CU two workgroups
        s = (int)((int64_t)kSplitkTargetPerCu * cus / units);
        if (s > tiles / kSplitkMinTiles) s = tiles / kSplitkMinTiles;
    }
    if (s > tiles) s = tiles;
    if (s > kSplitkMaxSplits) s = kSplitkMaxSplits;
    return s < 1 ? 1 : s;
}

// nvh_prefill_varlen_splitk: one split = exactly the plan of nvh_prefill_varlen; more = the tiled kernel's split-key form (64-row q-tiles, exact P V)
inline PrefillPlan plan_prefill_splitk(int forced, int paged, int out_f32, const PrefillShape& s, int h, int ticket_units, int cus) {
    PrefillPlan p = plan_prefill(PrefillRequest{NVH_PREFILL_AUTO, 0, NVH_PV_NEVER, out_f32, paged}, s, cus);
    const int splits = prefill_key_splits(forced, s.batch, s.max_seqlen_q, s.max_seqlen_k, h, s.hd, ticket_units, cus);
    if (p.error || splits <= 1) return p;
    p.kernel = NVH_PLAN_TILED;
    p.q_subtiles = 1;
    p.short_waves = 0;
    p.pv = NVH_PV_EXACT;
    p.key_splits = splits;
    return p;
}

// record of one split of one q-tile: 64 rows of [hd floats of un-normalised O | max (log2 domain) | sum | 0 | 0]; a multiple of 256 bytes at both head_dims
constexpr size_t splitk_record_bytes(int hd) { return (size_t)kSplitkTileKeys * (hd + 4) * 4; }
static_assert(splitk_record_bytes(64) % 256 == 0 && splitk_record_bytes(128) % 256 == 0, "records start on 256-byte boundaries");

// ============================================================================================ decode
struct DecodeShape { int batch, h, kvh, hd, block_size, max_blocks, ticket_pairs; };   // ticket_pairs: pairs the workspace header has tickets for (kMaxSplitPairs)
struct DecodePlan {
    int error = 0;
    const char* message = "";
    int impl = NVH_DECODE_CHUNKED;   // NVH_DECODE_CHUNKED / SPLIT_MFMA / SPLIT_VALU
    int waves = 0;               // waves per workgroup actually launched
    int pass_tokens = 0;         // tokens per pass actually launched (split kernels: tokens per workgroup)
    int chunks = 1;              // chunked kernel: workgroups per (sequence, kv head); passes are dealt to them round-robin
    int num_splits = 1;          // passes of decode_split_tokens() the longest possible context has (sizes the workspace records)
};

// tokens one workgroup of the split kernels covers = the chunked kernel's full pass (four waves x 4096 / hd tokens; paged_decode.hip asserts it)
constexpr int decode_split_tokens(int hd) { return hd == 64 ? 256 : 128; }

inline int decode_num_splits(int hd, int max_blocks, int block_size) {
    const int split = decode_split_tokens(hd);
    const int64_t cap = (int64_t)max_blocks * block_size;
    const int n = (int)((cap + split - 1) / split);
    return n < 1 ? 1 : n;
}

// workgroups per (sequence, kv head): one wave of workgroups over the chip, at most one per pass; `forced` > 0 (the
// variant entry point, tests and A/B runs) overrides the choice
inline int decode_chunks(const DecodeShape& s, int num_splits, int forced, int cus) {
    const int64_t pairs = (int64_t)s.batch * s.kvh;
    if (pairs < 1 || pairs > s.ticket_pairs) return 1;         // (more pairs than tickets: far more than CUs anyway)
    // floor, never nearest: every workgroup needs a CU to itself (134 KB of LDS), so a launch of more workgroups than CUs runs its
    // surplus as a second round (measured, B = 48 / 28 / 36 at ctx 1536: 3 / 5 / 4 chunks 13.8 / 11.0 / 10.8 us against
    // 10.1 / 8.0 / 8.5 with 2 / 4 / 3)
    int c = forced > 0 ? forced : (int)(cus / pairs);
    if (c < 1) c = 1;
    return c > num_splits ? num_splits : c;
}

// variant: NVH_DECODE_*; waves: 0 / 4 / 8; chunks: 0 or forced (nvh_paged_decode_variant; nvh_paged_decode passes CHUNKED, 0, 0)
inline DecodePlan plan_decode(int variant, int waves, int chunks, const DecodeShape& s, int cus) {
    DecodePlan p;
    if (variant == NVH_DECODE_SPLIT_VALU && s.h / (s.kvh > 0 ? s.kvh : 1) > 8) {
        p.error = NVH_E_SHAPE; p.message = "the VALU variant serves groups of at most 8 query heads"; return p;
    }
    p.num_splits = decode_num_splits(s.hd, s.max_blocks, s.block_size);
    // (tickets are only drawn when a (sequence, kv head) pair is split over several workgroups, i.e. when batch * kvh is small)
    p.chunks = decode_chunks(s, p.num_splits, chunks, cus);
    const int full = decode_split_tokens(s.hd);
    p.pass_tokens = full;
    if (variant == NVH_DECODE_SPLIT_MFMA) { p.impl = variant; p.waves = 4; return p; }
    if (variant == NVH_DECODE_SPLIT_VALU) { p.impl = variant; p.waves = 8; return p; }
    p.impl = NVH_DECODE_CHUNKED;
    const int forced_pass = variant == NVH_DECODE_CHUNKED_P128 ? 128 : variant == NVH_DECODE_CHUNKED_P256 ? 256 : variant == NVH_DECODE_CHUNKED_P64 ? 64 : 0;
    // D = 64: 8 waves (two per SIMD; 32-token tiles) by default: 6.97 vs 7.44 us at ctx 1034, 8.36 vs 8.47 at 1536; D = 128: NVH_D128_WAVES
    p.waves = waves == 4 ? 4 : (waves == 8 ? 8 : (s.hd == 64 ? 8 : NVH_D128_WAVES));
    if (s.hd == 64) {
        // Pass size at D = 64.  A pair split over 3-5 workgroups leaves each with one or two 256-token passes: whenever the pass count is not a
        // multiple of the chunk count some workgroups carry twice the tokens of the others and the call takes as long as they do.  128-token
        // passes (16-token wave tiles, the k = 16 MFMA) balance them: B = 32 (4 chunks) -0.5 / -1.9 / -6.6 / -4.0 / +1.9 / -3.7 / -1.9 % at ctx
        // 600 / 1034 / 1300 / 1536 / 1800 / 2500 / 3300, B = 40 (3 chunks) -2.9 % on average, B = 24 (5) -1.2 %.  With 8 and more chunks (small
        // batches) the passes outnumber nothing and the doubled per-pass work costs +1..12 %; with 2 chunks (B = 64) it is a wash.
        // The 128-token form exists with 8 waves only: forcing it overrides `waves`.  A forced 64 (which head_dim 64 does not have) forces 256.
        if (forced_pass == 128 || (forced_pass == 0 && p.waves == 8 && p.chunks >= 3 && p.chunks <= 5)) { p.waves = 8; p.pass_tokens = 128; }
    } else {
        // Pass size at D = 128: 64-token passes (four waves x 16-token tiles, the k = 16 MFMA) where 128-token passes leave some workgroups of a
        // pair with twice the tokens of the others, unless the caller chose the waves.  A forced 128 or 256 forces the full (128-token) pass.
        if (forced_pass == 64 || (forced_pass == 0 && waves == 0 && NVH_D128_HALF_RULE(p.chunks))) { p.waves = 4; p.pass_tokens = 64; }
    }
    return p;
}

// The one-launch qkv + attention form needs every workgroup of its grid resident at once (consumers wait for producers): two per CU by
// LDS (72 KB each) and threads (512 each), and a ticket line per (sequence, kv head) pair
inline bool one_launch_fits(int producer_tiles, int64_t pairs, int chunks, int ticket_pairs, int cus) {
    return producer_tiles + pairs * chunks <= 2 * (int64_t)cus && pairs <= ticket_pairs;
}

}  // namespace nvh
