// Streaming linear layer for 65 <= M <= 256 rows (decode batches above linear_stream.hip's 64), same contract: LinearArgs with the
// prologues none / folded RMSNorm (norm_mode 0 / 2) and the four epilogues; x row-major or in fragment order, out_packed for the
// next GEMM.  linear_stream.hip cannot grow into this range: its waves split K and each holds the x fragments of EVERY row tile
// (512 VGPRs of x at 16 row tiles), and its cross-wave reduction tile would no longer fit beside the staging area.  Here
//   * WAVES SPLIT THE ROWS: a workgroup (8 waves) owns one weight tile (NB blocks of 16 weight rows) over its K range and all M
//     rows; wave w owns row tiles w and w + 8 (RT = 1 up to 128 rows, 2 above).  No cross-wave reduction: the epilogue runs from
//     each wave's v_mfma_f32_16x16x32_bf16 accumulators.
//   * W GOES THROUGH LDS ONCE: the 8 waves together DMA the tile's weight rows of the workgroup's whole K range (at most 16 pieces
//     of 64 K-elements) with global_load_lds, 8 rows x 128 B per instruction, chunk order XOR-swizzled on the source (the image
//     of linear_stream.hip); one drain + barrier, then every wave reads its B operands from there.
//   * X IS STREAMED: one 1 KiB fragment load per (row tile, k-step) in fragment order, through two register groups of RG = 4
//     k-steps each: group g + 1 is requested before the MFMAs of group g.  The folded-norm row sums ride on the same fragments
//     (v_dot2_f32_bf16).
//   * SPLIT-K by handoff.h alone: 16-byte record items (st16 / ld16), one ticket per tile, the last arriver sums the partials in
//     split order in the accumulator layout and runs the epilogue.  No float atomics, no fences, no second launch.
// Tile width and split-K: rows_shape() below, the one statement of the rule.
#include "common.h"
#include "handoff.h"
#include "kernels.h"

namespace nvh {

namespace {

constexpr int RW = 8;             // waves per workgroup
constexpr int RPCAP = 16;         // K pieces (64 elements = one 128-byte line per weight row) a workgroup stages at most
constexpr int RG = 4;             // k-steps (32 elements) per x register group
constexpr int kEShape = -2;         // == NVH_E_SHAPE (nvh_attn.h)
constexpr size_t kRowsTicketBytes = 1u << 20;   // the workspace's ticket header: THE SAME BYTES WHATEVER THE SHAPE (one ticket per 128-byte line), so that
constexpr int kRowsMaxSplitTiles = (int)(kRowsTicketBytes / (4 * kTicketStride));   // one buffer serves launches of different shapes: no record ever lands on another shape's ticket
constexpr int kRowsCus = 256;     // CUs the rule below shapes launches for (MI355X); a constant, so that the workspace size is a pure function

struct RowsShape { int nb, tiles, ksplit, mt; };

// THE RULE.  A unit is 16 output columns (SiLU / RoPE: 16 weight rows and their 16 partner rows).
//   Tile width.  Every workgroup reads all of x: M * K * 2 bytes from L2, against 32 * K * 2 bytes of weights per 32 weight rows from
//   HBM, i.e. x traffic is M / 32 (2-8) times the weight traffic at NB = 2 and half of that at NB = 4.  NB = 4 costs 128 KiB of LDS
//   (one workgroup per CU instead of two), so it is taken only where N is so large that two waves of workgroups per CU remain
//   (tiles >= 2 * CUs at the wide width: the LM head, 151936 / 64 = 2374 tiles; Qwen2-7B's gate_up).  gate_up of Qwen2-0.5B stays
//   at 16 + 16 columns: 304 workgroups of 56 KiB, all resident two per CU.
//   Split-K.  Needed above 16 pieces (the LDS image); where N is small (fewer tiles than half the CUs: o_proj, down_proj) K is
//   also split to fill the CUs, as long as every split keeps at least 4 pieces (a partial record is M x 16 NB floats written and
//   read back, M * NB * 64 bytes against NB * 2 KiB of weights per piece: below 4 pieces the records outweigh the stream).
RowsShape rows_shape(int m, int n, int k, int epi) {
    const bool paired = epi == EPI_SILU || epi == EPI_ROPE;
    const int units = paired ? n / 32 : n / 16, pieces = k / 64;
    const int per_wide = paired ? 2 : 4, wide_tiles = (units + per_wide - 1) / per_wide;
    RowsShape s;
    s.nb = wide_tiles >= 2 * kRowsCus ? 4 : 2;
    const int per = paired ? s.nb / 2 : s.nb;
    s.tiles = (units + per - 1) / per;
    const int need = (pieces + RPCAP - 1) / RPCAP;
    int fill = s.tiles < kRowsCus / 2 ? kRowsCus / s.tiles : 1;
    if (fill > pieces / 4) fill = pieces / 4;
    s.ksplit = need > fill ? need : fill;
    if (s.ksplit < 1) s.ksplit = 1;
    s.mt = (m + 15) / 16;
    return s;
}

inline size_t rows_record_bytes(const RowsShape& s) { return (size_t)s.mt * (s.nb * 1024 + 64); }   // [mt][NB][64 lanes][4] accumulators, [mt][4][4] row sums

template <int RT, int NB, int EPI, int NORM>
__global__ __launch_bounds__(RW * 64) void linear_rows_kernel(const LinearArgs a, const int p_pq, const int p_pr) {
    constexpr bool PAIRED = EPI == EPI_SILU || EPI == EPI_ROPE;
    constexpr int CG = PAIRED ? NB / 2 : NB;                       // column units per tile
    __shared__ __attribute__((aligned(16))) unsigned char lds_w[RPCAP * NB * 2048];
    __shared__ unsigned lds_ticket;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 15, lg = lane >> 4;
    const int tile = blockIdx.x, split = blockIdx.y;
    const int mt = (a.M + 15) >> 4;
    // this workgroup's K pieces (the first p_pr splits carry one more)
    const int p0 = p_pq * split + min(split, p_pr), np = p_pq + (split < p_pr ? 1 : 0);      // 1..RPCAP (host)
    const int KS = a.K >> 5;

    // ---- column units of this tile: first weight row of each LDS block, first output column, validity (a ragged last tile)
    const int units = PAIRED ? a.N >> 5 : a.N >> 4;
    auto unit_of = [&](int c, int& col0, int& w_first, int& w_second, int& head, int& hi0) -> bool {
        const int unit = tile * CG + c;
        const int u = unit < units ? unit : units - 1;             // past the matrix: fetched clamped, never stored
        head = 0; hi0 = 0; w_second = 0;
        if constexpr (EPI == EPI_ROPE) {
            const int sh = a.hd == 128 ? 2 : 1;                    // units per head: hd / 32
            head = u >> sh;
            hi0 = 16 * (u & ((1 << sh) - 1));
            col0 = head * a.hd + hi0;
            w_first = col0;
            w_second = col0 + a.hd / 2;
        } else {
            col0 = u * 16;
            w_first = col0;
            if constexpr (EPI == EPI_SILU) w_second = a.inter + col0;
        }
        return unit < units;
    };

    // ---- W DMA: instruction i = (piece, block, half) of this workgroup's image, dealt round-robin to the 8 waves
    {
        const int dr = lane >> 3, dp = lane & 7;
        const int total = np * NB * 2;
        for (int i = wave; i < total; i += RW) {
            const int hh = i & 1, nb = (i >> 1) % NB, pi = i / (2 * NB);
            int col0, w_first, w_second, head, hi0;
            unit_of(PAIRED ? nb >> 1 : nb, col0, w_first, w_second, head, hi0);
            const int row = 8 * hh + dr;
            int wrow = ((PAIRED && (nb & 1)) ? w_second : w_first) + row;
            wrow = wrow < a.N ? wrow : a.N - 1;
            const uint16_t* src = a.w + (int64_t)wrow * a.K + (p0 + pi) * 64 + (dp ^ ((row >> 1) & 7)) * 8;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(lds_w + ((pi * NB + nb) * 2 + hh) * 1024), 16, 0, NVH_DMA_AUX);
        }
    }

    // ---- this wave's row tiles and the x stream
    int tm[RT];
    bool tv[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) { tm[t] = wave + RW * t; tv[t] = tm[t] < mt; }
    const int nks = 2 * np, ks0 = 2 * p0;
    auto load_group = [&](u32x4 (&buf)[RG][RT], int g) {
#pragma unroll
        for (int i = 0; i < RG; ++i) {
            const int s = g * RG + i;
            if (s < nks) {
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    if (tv[t]) {
                        if (a.x_packed) {
                            buf[i][t] = *reinterpret_cast<const u32x4*>(a.x + (((int64_t)tm[t] * KS + ks0 + s) * 64 + lane) * 8);
                        } else {
                            const int r = 16 * tm[t] + lq;                       // rows past M repeat the last row; discarded
                            buf[i][t] = *reinterpret_cast<const u32x4*>(a.x + (int64_t)(r < a.M ? r : a.M - 1) * a.x_stride + (ks0 + s) * 32 + lg * 8);
                        }
                    }
                }
            }
        }
    };
    f32x4 acc[RT][NB];
    float ss2[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        ss2[t] = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[t][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int rswz = (lq >> 1) & 7;
    auto compute_group = [&](u32x4 (&buf)[RG][RT], int g) {
#pragma unroll
        for (int i = 0; i < RG; ++i) {
            const int s = g * RG + i;
            if (s < nks) {
                const int pi = s >> 1, j = s & 1;
                u32x4 braw[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    braw[nb] = *reinterpret_cast<const u32x4*>(lds_w + (pi * NB + nb) * 2048 + lq * 128 + (((4 * j + lg) ^ rswz) * 16));
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    if (tv[t]) {
                        const u32x4 av = buf[i][t];
                        if constexpr (NORM == 2) {
#pragma unroll
                            for (int w = 0; w < 4; ++w) ss2[t] = dot2_bf16(av[w], av[w], ss2[t]);
                        }
                        const bf16x8 af = *reinterpret_cast<const bf16x8*>(&av);
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[t][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, *reinterpret_cast<const bf16x8*>(&braw[nb]), acc[t][nb], 0, 0, 0);
                    }
                }
            }
        }
    };

    u32x4 xa[RG][RT], xb[RG][RT];
    load_group(xa, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's share of the image has landed (and its first x group)
    __syncthreads();                                             // ... and every wave's
    const int groups = (nks + RG - 1) / RG;
    for (int g = 0; g < groups; g += 2) {
        load_group(xb, g + 1);
        compute_group(xa, g);
        load_group(xa, g + 2);
        compute_group(xb, g + 1);
    }

    // ---- row sums of squares in the accumulator layout: rowss[t][r] belongs to row 4 * lg + r of the tile
    f32x4 rowss[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        rowss[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (NORM == 2) {
            const float tot = sum_xor32(sum_xor16(ss2[t]));      // every lane: the sum of row lq over the four k groups
#pragma unroll
            for (int r = 0; r < 4; ++r) rowss[t][r] = __shfl(tot, 4 * lg + r, 64);
        }
    }

    if (a.ksplit > 1) {
        // ---- split-K (handoff.h): publish the partial in the accumulator layout, take the tile's ticket; the last arriver sums
        // the records in split order
        const uint32_t rec = (uint32_t)mt * (NB * 1024 + 64);
        const RecBuf rb = rec_buffer(reinterpret_cast<const unsigned char*>(a.ws) + (size_t)tile * a.ksplit * rec, (uint32_t)a.ksplit * rec);
        const uint32_t ss_base = (uint32_t)mt * NB * 1024;
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            if (tv[t]) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) st16(rb, split * rec + ((tm[t] * NB + nb) * 64 + lane) * 16, acc[t][nb]);
                if (NORM == 2 && lq == 0) st16(rb, split * rec + ss_base + (tm[t] * 4 + lg) * 16, rowss[t]);
            }
        }
        if (!handoff_arrive(&lds_ticket, [&] { return &a.counters[tile * kTicketStride]; }, a.ksplit)) return;   // workgroup-uniform
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            rowss[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[t][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int sp = 0; sp < a.ksplit; ++sp) {
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                if (tv[t]) {
                    f32x4 part[NB], ps = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) part[nb] = ld16(rb, sp * rec + ((tm[t] * NB + nb) * 64 + lane) * 16);
                    if constexpr (NORM == 2) ps = ld16(rb, sp * rec + ss_base + (tm[t] * 4 + lg) * 16);
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) acc[t][nb] += part[nb];
                    rowss[t] += ps;
                }
            }
        }
    }

    // ---- epilogue, straight from the accumulators: acc[t][nb][r] = product[16 * tm + 4 * lg + r][column lq of block nb]
    __bf16* const out = reinterpret_cast<__bf16*>(a.out);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        if (!tv[t]) continue;
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            int col0, w_first, w_second, head, hi0;
            if (!unit_of(c, col0, w_first, w_second, head, hi0)) continue;
            const int col = col0 + lq;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * tm[t] + 4 * lg + r;
                if (row >= a.M) continue;
                float y0 = acc[t][PAIRED ? 2 * c : c][r], y1 = PAIRED ? acc[t][PAIRED ? 2 * c + 1 : c][r] : 0.f;
                if constexpr (NORM == 2) {                       // x.(g*W)^T * rsqrt(mean(x^2)+eps) == RMSNorm(x).W^T without the two bf16 roundings
                    const float inv_row = rsqrtf(rowss[t][r] / a.K + a.norm_eps);
                    y0 *= inv_row;
                    y1 *= inv_row;
                }
                if constexpr (EPI == EPI_SILU) {
                    const float gt = (float)(__bf16)y0, up = (float)(__bf16)y1;             // the projection output is bf16 in the reference
                    const __bf16 o = (__bf16)((float)(__bf16)(gt / (1.f + __expf(-gt))) * up);
                    if (out) out[(int64_t)row * a.out_stride + col] = o;
                    if (a.out_packed) a.out_packed[pack_index(row, col, a.inter)] = __builtin_bit_cast(uint16_t, o);
                } else if constexpr (EPI == EPI_RESADD) {
                    __bf16* const p = out + (int64_t)row * a.out_stride + col;
                    const __bf16 o = (__bf16)(y0 + (float)*p);
                    *p = o;
                    if (a.out_packed) a.out_packed[pack_index(row, col, a.N)] = __builtin_bit_cast(uint16_t, o);
                } else if constexpr (EPI == EPI_ROPE) {
                    float x1 = y0, x2 = y1;
                    if (a.bias) {
                        x1 += (float)__builtin_bit_cast(__bf16, a.bias[w_first + lq]);
                        x2 += (float)__builtin_bit_cast(__bf16, a.bias[w_second + lq]);
                    }
                    x1 = (float)(__bf16)x1;                      // the projection output is bf16 in the reference
                    x2 = (float)(__bf16)x2;
                    const int i = hi0 + lq;                      // index inside the half head
                    float r1 = x1, r2 = x2;
                    if (head < a.h + a.kvh) {                    // q or k head: rotate (products and sums rounded separately)
                        const float* const cs = a.cos_sin + a.positions[row] * a.hd;
                        const float co = cs[i], si = cs[a.hd / 2 + i];
                        const float p1 = x1 * co, p2 = x2 * si, p3 = x2 * co, p4 = x1 * si;
                        r1 = p1 - p2;
                        r2 = p3 + p4;
                    }
                    if (head < a.h) {
                        __bf16* const q = out + (int64_t)row * a.out_stride + head * a.hd + i;
                        q[0] = (__bf16)r1;
                        q[a.hd / 2] = (__bf16)r2;
                    } else {
                        const int slot = a.slots[row];
                        if (slot >= 0) {
                            const bool is_v = head >= a.h + a.kvh;
                            __bf16* const dst = reinterpret_cast<__bf16*>(is_v ? a.v_cache : a.k_cache) +
                                                ((int64_t)slot * a.kvh + (head - a.h - (is_v ? a.kvh : 0))) * a.hd + i;
                            dst[0] = (__bf16)r1;
                            dst[a.hd / 2] = (__bf16)r2;
                        }
                    }
                } else {
                    const __bf16 o = (__bf16)(y0 + (a.bias ? (float)__builtin_bit_cast(__bf16, a.bias[col]) : 0.f));
                    if (out) out[(int64_t)row * a.out_stride + col] = o;
                    if (a.out_packed) a.out_packed[pack_index(row, col, a.N)] = __builtin_bit_cast(uint16_t, o);
                }
            }
        }
    }
}

template <int RT, int NB, int EPI>
int launch_rows_n(const LinearArgs& a, hipStream_t stream) {
    const int pieces = a.K / 64, pq = pieces / a.ksplit, pr = pieces % a.ksplit;
    const dim3 grid(a.tiles, a.ksplit), block(RW * 64);
    if (a.norm_mode == 2) hipLaunchKernelGGL((linear_rows_kernel<RT, NB, EPI, 2>), grid, block, 0, stream, a, pq, pr);
    else hipLaunchKernelGGL((linear_rows_kernel<RT, NB, EPI, 0>), grid, block, 0, stream, a, pq, pr);
    return check_launch("linear_rows");
}

template <int RT, int NB>
int launch_rows_e(const LinearArgs& a, hipStream_t stream) {
    switch (a.epi) {
        case EPI_NONE: return launch_rows_n<RT, NB, EPI_NONE>(a, stream);
        case EPI_SILU: return launch_rows_n<RT, NB, EPI_SILU>(a, stream);
        case EPI_RESADD: return launch_rows_n<RT, NB, EPI_RESADD>(a, stream);
        case EPI_ROPE: return launch_rows_n<RT, NB, EPI_ROPE>(a, stream);
    }
    return kEShape;
}

}  // namespace

// [ticket header, kRowsTicketBytes][partial records [tiles][ksplit][rows_record_bytes]]; 0 when K is not split
size_t linear_rows_workspace_bytes(int m, int n, int k, int epi) {
    if (m <= 64 || m > 256 || k <= 0 || k % 64 || n <= 0 || n % 16) return 0;
    const RowsShape s = rows_shape(m, n, k, epi);
    if (s.ksplit <= 1) return 0;
    return kRowsTicketBytes + (size_t)s.tiles * s.ksplit * rows_record_bytes(s);
}

int launch_linear_rows(const LinearArgs& a_in, hipStream_t stream) {
    LinearArgs a = a_in;
    if (a.M <= 64 || a.M > 256 || a.K % 64 != 0 || a.N % 16 != 0) { set_error("linear_rows: m=%d (65..256) n=%d (%%16) k=%d (%%64)", a.M, a.N, a.K); return kEShape; }
    if (a.cand_val || a.smp.temperatures) { set_error("linear_small_m_ex: candidates / sampling inside the GEMM serve at most 64 rows (m=%d): write the logits and use the advance calls", a.M); return kEShape; }
    if (a.norm_mode == 1) { set_error("linear_small_m_ex: the exact-norm prologue (norm_weight) serves at most 64 rows (m=%d): fold the norm weight (norm_folded)", a.M); return kEShape; }
    if ((a.epi == EPI_SILU || a.epi == EPI_ROPE) && a.N % 32 != 0) { set_error("linear_rows: paired epilogue needs n %% 32 == 0 (n=%d)", a.N); return kEShape; }
    const RowsShape s = rows_shape(a.M, a.N, a.K, a.epi);
    a.tiles = s.tiles;
    a.ksplit = s.ksplit;
    a.ws = nullptr;
    a.counters = nullptr;
    if (s.ksplit > 1) {
        const size_t counters_bytes = kRowsTicketBytes;
        if (s.tiles > kRowsMaxSplitTiles) { set_error("linear_small_m_ex: m=%d n=%d k=%d splits K over %d tiles, more than the %d tickets of the workspace header", a.M, a.N, a.K, s.tiles, kRowsMaxSplitTiles); return kEShape; }
        if (!a.ws_raw || a.ws_bytes < counters_bytes + (size_t)s.tiles * s.ksplit * rows_record_bytes(s)) {
            set_error("linear_small_m_ex: m=%d n=%d k=%d splits K over %d workgroups and needs a workspace of nvh_linear_small_m_workspace() bytes", a.M, a.N, a.K, s.ksplit);
            return kEShape;
        }
        a.counters = reinterpret_cast<unsigned*>(a.ws_raw);
        a.ws = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(a.ws_raw) + counters_bytes);
    }
    if (s.mt <= RW) return s.nb == 4 ? launch_rows_e<1, 4>(a, stream) : launch_rows_e<1, 2>(a, stream);
    return s.nb == 4 ? launch_rows_e<2, 4>(a, stream) : launch_rows_e<2, 2>(a, stream);
}

}  // namespace nvh
