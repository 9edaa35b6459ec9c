"""GPU: every dispatch form of the small-M GEMMs (csrc/linear_stream.hip, csrc/skinny_gemm.hip) against an EXACT reference.

Operands are chosen so that the true result is itself a bf16 number: x holds integers in [-2, 2], every weight row at most
128 non-zeros of +-1.  Every output is then an integer of magnitude <= 256 (exact in bf16), every fp32 partial sum is exact in
any order and any split, and one dropped, doubled or misrouted K term moves the result by at least 1.  The reference is
x.double() @ w.double().T and the comparison is torch.equal: no tolerance, no outlier share.  Each case re-asserts on the CPU,
before the launch, that its reference survives the round trip through bf16 and that at most 10 % of it is zero.

Dispatch rules the shape tables are derived from (launch_linear_stream / launch_x), with pieces = K / 64:
    MT     = ceil(M / 16)                                  1..4, a template argument of every kernel
    tiles  = N / 16  (silu: inter / 16; rope: (H + 2 KVH) * D / 32)
    ksplit = ceil(pieces / 16);  ksplit > 1 needs a workspace (linear_workspace_bytes > 0), without one the call falls to
             the loop kernel of skinny_gemm.hip
    none:          ksplit == 1 and tiles > 1024 -> MULTI (512 workgroups walk the tiles, 4 waves)
                   ksplit  > 1 and tiles > 1024 -> 4 waves, PM = 4, split-K
                   otherwise                    -> 8 waves, PM = 2 (split-K when ksplit > 1)
    silu_mul:      ksplit == 1, tiles > 256, ceil(inter / 24) <= 256, inter % 8 == 0 -> WIDE tiles of 24 + 24 columns
    residual_add:  ks5 = ceil(pieces / 20); ksplit > 1, tiles * ksplit > 256, tiles * ks5 <= 256 -> 8 waves, PM = 3, ks5 splits
                   (ks5 == 1: no hand-off at all although a workspace is bound)
"""
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu            # (the SiLU margin check below needs no GPU)

NAN_BITS = 0x7FC1                     # a quiet-NaN bf16 pattern no kernel produces: "this element was never written"
SENTINEL = 77.0                       # the same for the residual stream (which is read, so it has to be a number)
PAD_ROWS = 16                         # rows behind M in the strided output buffers
PAD_COLS = 3                          # columns behind `cols`: an odd row stride


# ------------------------------------------------------------------------------------------------ operands and references
def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _sparse_pm1(gen, n, k, nnz, distinct=False):
    """[n, k] with at most `nnz` non-zeros per row, each +-1, at random columns (drawn with replacement: a repeated column is
    one non-zero; distinct=True: exactly min(nnz, k) columns, for the few rows where the count matters)."""
    if distinct:
        idx = torch.rand(n, k, generator=gen).argsort(1)[:, :nnz]
    else:
        idx = torch.randint(0, k, (n, nnz), generator=gen)
    nnz = idx.shape[1]
    sgn = (torch.randint(0, 2, (n, nnz), generator=gen) * 2 - 1).float()
    return torch.zeros(n, k).scatter_(1, idx, sgn)


def _round_trips(t64):
    return torch.equal(t64.float().bfloat16().double(), t64)


def _exact(t64):
    """float64 -> bf16, asserting that nothing is lost."""
    assert _round_trips(t64), "the reference is not exactly representable in bf16"
    return t64.float().bfloat16()


def _self_check(ref_bf16):
    zero_share = float((ref_bf16 == 0).float().mean())
    assert zero_share <= 0.10, f"{zero_share:.3f} of the reference is zero: 'all zeros' must not come close to passing"


def silu_tie_margin():
    """Smallest relative distance of float64 silu(g), g an integer in [-8, 8] \\ {0}, from a bf16 rounding tie (the midpoint of
    two neighbouring bf16 numbers).  The kernel evaluates g / (1 + __expf(-g)) in fp32 (relative error ~2^-21); as long as the
    margin is far above that, rounding the float64 value gives the kernel's bf16 bit for bit."""
    worst = 1.0
    for g in range(-8, 9):
        if g == 0:
            continue
        v = abs(g / (1.0 + math.exp(-g)))
        ulp = 2.0 ** (math.frexp(v)[1] - 8)          # bf16: 8 significant bits
        frac = v / ulp - math.floor(v / ulp)
        worst = min(worst, abs(frac - 0.5) * ulp / v)
    return worst


@functools.lru_cache(maxsize=None)
def _case(epi, m, n, k, bias=False, pm1=False, seed=0, dup=False):
    """CPU operands (bf16) and the exact expected output of one case.  n is the weight's row count except for silu_mul, where
    it is `inter` (the weight then has 2 * inter rows: gate rows first).  pm1: x in {-1, +1} (norm_folded cases: mean(x^2) == 1).
    dup: two weight rows are copies of two others (exact ties between columns for the candidates test)."""
    assert not (pm1 and bias)
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * m + 31 * n + k)
    if pm1:
        x = _ints(gen, (m, k), 0, 1) * 2 - 1
    elif epi == "silu_mul":
        # gate sums have at most 3 terms here, so a uniform draw from [-2, 2] would leave ~15 % of the gates (hence of the
        # outputs) at zero; +-1 with probability 0.48 each and +-2 with 0.02 each keeps every gate value in [-6, 6] present
        # (the tie-margin worst cases g = 2 and g = 6 among them) and the zero share under the 10 % bar
        mag = 1 + (torch.rand(m, k, generator=gen) < 0.04).float()
        x = mag * (_ints(gen, (m, k), 0, 1) * 2 - 1)
    else:
        x = _ints(gen, (m, k), -2, 2)
    b = _ints(gen, (n,), -8, 8) if bias else None
    res = _ints(gen, (m, n), -64, 64) if epi == "residual_add" else None
    for nnz in (128, 96):                                  # 96: the redraw for a sum that leaves the exact range
        if epi == "silu_mul":
            # gate rows: exactly 3 non-zeros (<= 4, |gate| <= 8; an odd count of mostly odd terms is rarely zero); up rows as everywhere
            w = torch.cat([_sparse_pm1(gen, n, k, 3, distinct=True), _sparse_pm1(gen, n, k, nnz)])
        else:
            w = _sparse_pm1(gen, n, k, nnz)
        if dup:
            w[n - 7] = w[11]
            w[n // 2] = w[3]
        y = x.double() @ w.double().T
        if pm1 and res is not None:
            # norm_folded: the kernel adds the residual to y * (1 - 5e-7).  Where y + res cancels to zero the true result is the
            # 5e-7 * y that is left, not 0 (and its bits hang on the last bit of the fp32 rsqrt): keep the operands off that
            # one ill-conditioned point (for the same reason the norm_folded cases carry no bias)
            res = torch.where((y + res.double() == 0) & (y != 0), res + 1, res)
        full = y + (b.double() if bias else 0) + (res.double() if res is not None else 0)
        if _round_trips(y) and _round_trips(full):
            break
    ref = _exact(full)                                     # the projection (+ bias / residual) is a bf16 number everywhere
    _exact(y)
    if epi == "silu_mul":
        g, u = y[:, :n], y[:, n:]
        assert float(g.abs().max()) <= 8 and silu_tie_margin() >= 2.0 ** -16
        # the kernel's rounding points (linear_stream.hip, SiLU epilogue): bf16(bf16(g * sigmoid(g)) * u), in float64; the
        # product of an 8-bit and a 9-bit significand is exact in fp32 as in float64, so it is rounded once, identically
        act = (g / (1.0 + torch.exp(-g))).float().bfloat16().double()
        ref = (act * u).float().bfloat16()
    _self_check(ref)
    to = lambda t: None if t is None else t.bfloat16()
    return dict(epi=epi, m=m, n=n, k=k, x=to(x), w=to(w), bias=to(b), res=to(res), ref=ref, pm1=pm1)


def _cols(c):
    return c["n"]


def _tiles(c):
    return c["ref"].shape[1] // 32 if c["epi"] == "rope_store" else c["n"] // 16      # rope: `ref` is the whole qkv row


def _weight_rows(c):
    return 2 * c["n"] if c["epi"] == "silu_mul" else c["n"]


def _dev(t):
    return None if t is None else t.cuda()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _nan_buffer(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _pack(x, pad_bits=0):
    """ops.pack_rows with a chosen bit pattern in the padding rows (M .. 16 * ceil(M / 16))."""
    m, c = x.shape
    mt = (m + 15) // 16
    xp = torch.full((mt * 16, c), pad_bits, dtype=torch.int16, device=x.device).view(torch.bfloat16)
    xp[:m] = x
    return xp.view(mt, 16, c // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def _launch(c, d, *, workspace=None, x=None, x_packed_rows=None, out=None, out_packed=None, folded=False, candidates=None):
    """One ops.fused_linear call of case `c` on the device operands `d`; returns the output tensor (residual_add: the updated
    residual stream)."""
    from nanovllm_hip import ops
    kw = dict(epilogue=c["epi"], workspace=workspace, x_packed_rows=x_packed_rows, out_packed=out_packed,
              norm_folded=folded, norm_eps=1e-6, candidates=candidates)
    if c["epi"] == "residual_add" and out is None:
        out = d["res"].clone()
    return ops.fused_linear(d["x"] if x is None else x, d["w"], bias=d["bias"], out=out, **kw)


def _check_exact_everywhere(c, folded=False):
    """The streaming kernel (three times on one zero-filled workspace when K is split: identical bits, tickets back at zero)
    and the loop kernel (no workspace) against the exact reference."""
    from nanovllm_hip import ops
    m, k, epi = c["m"], c["k"], c["epi"]
    d = {key: _dev(c[key]) for key in ("x", "w", "bias", "res")}
    ref = c["ref"].cuda()
    need = ops.linear_workspace_bytes(m, _weight_rows(c), k, epi)
    assert (need > 0) == (k // 64 > 16), "workspace bytes > 0 <=> K is split over workgroups"
    outs = []
    if need:
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        outs = [_launch(c, d, workspace=ws, folded=folded) for _ in range(3)]
    outs.append(_launch(c, d, workspace=None, folded=folded))      # K <= 1024: the streaming kernel; else the loop kernel
    if epi == "none" and not need and not folded:                  # the plain entry point forwards to the same launch
        outs.append(ops.linear_small_m(d["x"], d["w"], d["bias"]))
    if epi == "silu_mul" and not need and not folded:
        outs.append(ops.linear_small_m(d["x"], d["w"], silu_mul=True))
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert o.shape == ref.shape
        bad = (o != ref).nonzero()
        assert torch.equal(o, ref), f"launch {i} of {len(outs)}: {bad.shape[0]} wrong elements, first (row, col) {bad[:4].tolist()}"
    if need:
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        assert int(ws[: _tiles(c) * 128].view(torch.int32).abs().sum()) == 0       # one ticket per 128-byte line, all zero again


# ------------------------------------------------------------------------------------------------ none (+ bias)
# (N, K, M, bias): pieces = K / 64, tiles = N / 16
NONE_ROWS = [
    (16, 64, 33, False),       # 1 tile, 1 piece (seven of the eight waves own no piece): 8 waves PM 2, MT 3
    (16384, 64, 17, False),    # tiles 1024: the last single-tile grid, 8 waves PM 2, MT 2
    (16400, 64, 1, True),      # tiles 1025 > 1024, ksplit 1: MULTI, 1025 tiles over 512 workgroups (one gets 3, the rest 2), MT 1
    (16912, 128, 64, False),   # tiles 1057, 2 pieces: MULTI, uneven deal (33 workgroups walk 3 tiles), MT 4
    (64, 1088, 15, True),      # 17 pieces -> ksplit 2 (9 + 8), 4 tiles: 8 waves PM 2 split-K with bias, MT 1
    (1040, 2048, 49, False),   # 32 pieces -> ksplit 2, tiles 65: 8 waves PM 2 split-K without bias, MT 4
    (16400, 1088, 49, False),  # tiles 1025 > 1024 and ksplit 2: the 4-wave PM 4 split-K launch (deep LM head), MT 4
    (64, 18944, 16, False),    # 296 pieces -> ksplit 19 (pieces % ksplit = 11: splits of 16 and 15), summed 8 at a time, MT 1
]


@gpu
@pytest.mark.parametrize("n,k,m,bias", NONE_ROWS)
def test_exact_none(n, k, m, bias):
    _check_exact_everywhere(_case("none", m, n, k, bias=bias))


# ------------------------------------------------------------------------------------------------ silu_mul
# (inter, K, M): tiles = inter / 16, wide_tiles = ceil(inter / 24)
SILU_ROWS = [
    (16, 64, 33),      # 1 tile: 8 waves PM 2, MT 3
    (4096, 64, 1),     # tiles 256: not above 256, so narrow tiles (16 + 16 columns), MT 1
    (4112, 64, 17),    # tiles 257, wide_tiles 172: WIDE, last tile holds 8 columns (24 * 171 = 4104), MT 2
    (4864, 128, 64),   # tiles 304, wide_tiles 203: WIDE, last tile holds 16 columns (24 * 202 = 4848), MT 4
    (6128, 64, 15),    # wide_tiles 256: the last WIDE size, 8-column tail, MT 1
    (6144, 64, 48),    # wide_tiles 256 exactly, no tail, MT 3
    (6160, 64, 49),    # wide_tiles 257 > 256: narrow tiles again, 385 workgroups, MT 4
    (48, 3584, 16),    # 56 pieces -> ksplit 4 (14 each), 3 tiles: 8 waves PM 2 split-K, epilogue in the last arriver, MT 1
]


@gpu
@pytest.mark.parametrize("inter,k,m", SILU_ROWS)
def test_exact_silu_mul(inter, k, m):
    _check_exact_everywhere(_case("silu_mul", m, inter, k))


def test_silu_tie_margin():
    """The float64 reference of the SiLU epilogue stands on its own margin: for integer gates in [-8, 8] silu(g) stays at
    least 2^-16 (relative) away from every bf16 rounding tie; the worst cases are g = 2 and g = 6 at about 2^-14."""
    assert 2.0 ** -16 <= silu_tie_margin() <= 2.0 ** -13


# ------------------------------------------------------------------------------------------------ residual_add
# (N, K, M): ks5 = ceil(pieces / 20)
RESADD_ROWS = [
    (16, 64, 48),       # 1 tile, 1 piece: 8 waves PM 2, MT 3
    (896, 896, 64),     # 14 pieces, ksplit 1: 8 waves PM 2, MT 4
    (2064, 1088, 17),   # tiles 129, ksplit 2 (258 > 256), ks5 1 (129 <= 256): PM 3, ksplit forced to 1 with a workspace bound, MT 2
    (4096, 1280, 33),   # tiles 256, 20 pieces: ksplit 2, ks5 1, the upper edge of that rule in tiles and in K, MT 3
    (896, 4864, 49),    # tiles 56, 76 pieces: ksplit 5 (280 > 256), ks5 4 (224): PM 3, four splits of 19 pieces, MT 4
    (4112, 1088, 1),    # tiles 257: ks5 1 would still be 257 > 256, so the plain 8 waves PM 2 split of 2, MT 1
    (64, 18944, 15),    # 4 tiles x ksplit 19 = 76 <= 256: no ks5 rule, 8 waves PM 2, 19 splits, MT 1
]


@gpu
@pytest.mark.parametrize("n,k,m", RESADD_ROWS)
def test_exact_residual_add(n, k, m):
    _check_exact_everywhere(_case("residual_add", m, n, k))


# ------------------------------------------------------------------------------------------------ rope_store
# (H, KVH, D, K, M): tiles = (H + 2 KVH) * D / 32; a tile is 16 columns of a head and their partners D / 2 further on
ROPE_ROWS = [
    (2, 1, 64, 64, 15),      # 8 tiles, 1 piece, MT 1
    (14, 2, 64, 896, 33),    # Qwen2-0.5B: 36 tiles, ksplit 1, MT 3
    (7, 1, 128, 3584, 64),   # 36 tiles, 56 pieces -> ksplit 4: split-K at D = 128 (four tiles per head), MT 4
    (4, 2, 64, 2048, 17),    # 16 tiles, ksplit 2: split-K at D = 64 (two tiles per head), MT 2
]


def _rope_setup(c, h, kvh, hd):
    """Device operands of a rope_store case and the expected (q, k_cache, v_cache): nvh_rope_store (pinned bit-exact to the
    reference goldens by test_hip_rope_store.py) applied to the exact bf16 qkv."""
    from nanovllm_hip import ops
    from nanovllm_hip.models.qwen import cos_sin_table
    m, bs, nb = c["m"], 64, 2
    gen = torch.Generator().manual_seed(h * 131 + hd + m)
    pos = torch.randint(0, 4096, (m,), generator=gen).cuda()
    slots = torch.randperm(nb * bs, generator=gen)[:m].int()
    slots[2::9] = -1
    slots[0] = -1
    slots = slots.cuda()
    table = cos_sin_table(hd, 4096, 1e6, "cuda")
    kc0 = torch.randn(nb, bs, kvh, hd, generator=gen).bfloat16().cuda()
    vc0 = torch.randn(nb, bs, kvh, hd, generator=gen).bfloat16().cuda()
    qkv = c["ref"].cuda()
    kc_ref, vc_ref = kc0.clone(), vc0.clone()
    ops.rope_store(qkv, pos, table, h, kvh, hd, kc_ref, vc_ref, slots)
    mk = lambda: dict(positions=pos, cos_sin=table, k_cache=kc0.clone(), v_cache=vc0.clone(), slot_mapping=slots,
                      num_heads=h, num_kv_heads=kvh, head_dim=hd)
    return mk, qkv[:, :h * hd].contiguous(), kc_ref, vc_ref


def _rope_case(h, kvh, hd, k, m, pm1=False):
    return _case("rope_store", m, (h + 2 * kvh) * hd, k, bias=not pm1, pm1=pm1)      # (norm_folded cases: no bias, see FOLDED_ROWS)


def _check_rope(c, h, kvh, hd, folded=False):
    from nanovllm_hip import ops
    m, n, k = c["m"], c["n"], c["k"]
    d = {key: _dev(c[key]) for key in ("x", "w", "bias")}
    mk, q_ref, kc_ref, vc_ref = _rope_setup(c, h, kvh, hd)
    need = ops.linear_workspace_bytes(m, n, k, "rope_store")
    assert (need > 0) == (k // 64 > 16)
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")
    runs = []
    for wsp in ([ws, ws, ws, None] if need else [None]):           # None with K > 1024: the loop kernel
        rope = mk()
        q = ops.fused_linear(d["x"], d["w"], bias=d["bias"], epilogue="rope_store", rope=rope, workspace=wsp,
                             norm_folded=folded, norm_eps=1e-6)
        runs.append((q, rope["k_cache"], rope["v_cache"]))
    torch.cuda.synchronize()
    for q, kc, vc in runs:
        assert torch.equal(q, q_ref)
        assert torch.equal(kc, kc_ref) and torch.equal(vc, vc_ref)
    if need:
        assert int(ws[: _tiles(c) * 128].view(torch.int32).abs().sum()) == 0


@gpu
@pytest.mark.parametrize("h,kvh,hd,k,m", ROPE_ROWS)
def test_exact_rope_store(h, kvh, hd, k, m):
    """The projection (+ integer bias) is exact, so the fused epilogue must give, bit for bit, nvh_rope_store of the exact
    bf16 qkv: on q and on both caches, rows with slot -1 skipped."""
    _check_rope(_rope_case(h, kvh, hd, k, m), h, kvh, hd)


# ------------------------------------------------------------------------------------------------ norm_folded
# x in {-1, +1}: mean(x^2) is exactly 1 and the row scale rsqrt(1 + 1e-6) = 1 - 5e-7.  An integer sum of magnitude <= 128 (or
# <= 2^9 with bias / residual) times that scale lies 5e-7 (relative) from a bf16 number whose nearest rounding boundary is 2^-9
# away, so it rounds back to itself: bit-equality with the UNSCALED integer reference.  That argument is about the scaled sum
# alone: a bias (or residual) of -y added BEHIND the scale leaves 5e-7 * y where the unscaled sum has 0, which is the right
# answer of the folded norm and not an integer.  So these cases carry no bias, and the residual is kept off exact cancellation
# (see _case).  The row sums of squares travel through the same paths as the products (wave reduction, split-K partial
# records), so each grid form gets one row.
FOLDED_ROWS = [
    ("none", 16400, 64, 33),            # MULTI: the row sums are taken in the first tile only
    ("none", 1040, 2048, 17),           # split-K: the row sums ride behind the partial records
    ("silu_mul", 4112, 64, 49),         # WIDE tiles
    ("silu_mul", 48, 3584, 15),         # split-K with two row blocks per record
    ("residual_add", 896, 4864, 15),    # PM 3, ks5 = 4
    ("residual_add", 2064, 1088, 64),   # PM 3, ks5 = 1
]


@gpu
@pytest.mark.parametrize("epi,n,k,m", FOLDED_ROWS)
def test_exact_norm_folded(epi, n, k, m):
    _check_exact_everywhere(_case(epi, m, n, k, pm1=True), folded=True)


@gpu
@pytest.mark.parametrize("h,kvh,hd,k,m", [(14, 2, 64, 896, 17), (4, 2, 64, 2048, 64)])
def test_exact_norm_folded_rope_store(h, kvh, hd, k, m):
    _check_rope(_rope_case(h, kvh, hd, k, m, pm1=True), h, kvh, hd, folded=True)


# ------------------------------------------------------------------------------------------------ forms of the same launch
# One row per grid form and epilogue; cols % 32 == 0 throughout (out_packed needs whole fragments), which the boundary rows of
# the tables above are not, hence rows of their own here.  (epilogue, N or inter, K, M, bias)
FORM_ROWS = [
    ("none", 16384, 64, 17, True),            # single tile per workgroup, 8 waves
    ("none", 16416, 64, 33, False),           # tiles 1026: MULTI
    ("none", 1056, 2048, 49, True),           # 8-wave split-K
    ("none", 16416, 1088, 15, False),         # 4-wave split-K
    ("silu_mul", 4096, 64, 33, False),        # narrow tiles
    ("silu_mul", 4864, 128, 17, False),       # WIDE, 16-column tail
    ("silu_mul", 6112, 64, 49, False),        # WIDE (255 tiles), 16-column tail, MT 4
    ("silu_mul", 96, 2048, 15, False),        # split-K
    ("residual_add", 896, 896, 64, False),    # no split
    ("residual_add", 2080, 1088, 17, False),  # tiles 130: PM 3, ks5 == 1
    ("residual_add", 896, 4864, 33, False),   # PM 3, ks5 == 4
    ("residual_add", 4128, 1088, 49, False),  # tiles 258: plain split of 2
]


@gpu
@pytest.mark.parametrize("epi,n,k,m,bias", FORM_ROWS)
def test_forms_change_no_bit(epi, n, k, m, bias):
    """Fragment-packed x, out_packed, a strided x and a strided out are the same arithmetic behind a different fetch or store:
    each must give the exact reference, and must write nothing but rows < M and columns < cols.

    Padding rows of the packed layouts (M .. 16 * ceil(M / 16)): nothing is promised about their CONTENT.  The consumer of an
    out_packed buffer is the next launch's x_packed fetch (models/qwen.py, _forward_decode_fused), which feeds them to MFMA rows
    whose products the epilogue discards (row >= M); the model allocates the buffers zero-filled once and never clears them
    again.  So two things are asserted: the producer writes rows < M only (a NaN-prefilled out_packed keeps its pattern in the
    padding rows, as the row-major output does), and the consumer does not depend on them (x_packed with NaN padding rows gives
    the exact result)."""
    from nanovllm_hip import ops
    c = _case(epi, m, n, k, bias=bias)
    d = {key: _dev(c[key]) for key in ("x", "w", "bias", "res")}
    ref = c["ref"].cuda()
    cols, rows16 = _cols(c), (m + 15) // 16 * 16
    assert cols % 32 == 0
    need = ops.linear_workspace_bytes(m, _weight_rows(c), k, epi)
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda") if need else None

    # fragment-packed x: zero padding (ops.pack_rows) and NaN padding
    for xp in (ops.pack_rows(d["x"]), _pack(d["x"], NAN_BITS)):
        assert torch.equal(_launch(c, d, workspace=ws, x=xp, x_packed_rows=m), ref)

    # out_packed next to the row-major output, and alone where the row-major output is optional
    packed = _nan_buffer(rows16 * cols)
    assert torch.equal(_launch(c, d, workspace=ws, out_packed=packed), ref)
    un = ops.unpack_rows(packed, rows16, cols)
    assert torch.equal(un[:m], ref)
    assert bool((_bits(un[m:]) == NAN_BITS).all()), "out_packed: a padding row was written"
    if epi != "residual_add":
        packed2 = _nan_buffer(rows16 * cols)
        assert ops.fused_linear(d["x"], d["w"], bias=d["bias"], epilogue=epi, workspace=ws, out_packed=packed2, want_out=False) is None
        assert torch.equal(_bits(packed2), _bits(packed))

    # strided x: the slack columns hold 7 and must not enter the sums
    xs = torch.full((m, k + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    xs[:, :k] = d["x"]
    assert torch.equal(_launch(c, d, workspace=ws, x=xs[:, :k]), ref)

    # strided out with an odd row stride: rows >= M and columns >= cols keep their pattern, bit for bit
    if epi == "residual_add":
        buf = torch.full((64 + PAD_ROWS, cols + PAD_COLS), SENTINEL, dtype=torch.bfloat16, device="cuda")
        buf[:m, :cols] = d["res"]
    else:
        buf = _nan_buffer(64 + PAD_ROWS, cols + PAD_COLS)
    expect = _bits(buf.clone())
    expect[:m, :cols] = _bits(ref)
    out = _launch(c, d, workspace=ws, out=buf[:m, :cols])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and out.stride(0) == cols + PAD_COLS
    assert torch.equal(_bits(buf), expect)
    if need:
        assert int(ws[: _tiles(c) * 128].view(torch.int32).abs().sum()) == 0


@gpu
@pytest.mark.parametrize("h,kvh,hd,k,m", [(2, 1, 64, 64, 15), (14, 2, 64, 896, 33), (4, 2, 64, 2048, 17)])
def test_forms_change_no_bit_rope_store(h, kvh, hd, k, m):
    """The same for the RoPE + store epilogue (it has no out_packed form: q goes to the attention launch row-major)."""
    from nanovllm_hip import ops
    c = _rope_case(h, kvh, hd, k, m)
    d = {key: _dev(c[key]) for key in ("x", "w", "bias")}
    mk, q_ref, kc_ref, vc_ref = _rope_setup(c, h, kvh, hd)
    cols = h * hd
    need = ops.linear_workspace_bytes(m, c["n"], k, "rope_store")
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda") if need else None
    xs = torch.full((m, k + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    xs[:, :k] = d["x"]
    for x, rows in ((ops.pack_rows(d["x"]), m), (_pack(d["x"], NAN_BITS), m), (xs[:, :k], None)):
        rope = mk()
        q = ops.fused_linear(x, d["w"], bias=d["bias"], epilogue="rope_store", rope=rope, workspace=ws, x_packed_rows=rows)
        assert torch.equal(q, q_ref) and torch.equal(rope["k_cache"], kc_ref) and torch.equal(rope["v_cache"], vc_ref)
    buf = _nan_buffer(64 + PAD_ROWS, cols + PAD_COLS)
    expect = _bits(buf.clone())
    expect[:m, :cols] = _bits(q_ref)
    rope = mk()
    ops.fused_linear(d["x"], d["w"], bias=d["bias"], epilogue="rope_store", rope=rope, workspace=ws, out=buf[:m, :cols])
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), expect)
    assert torch.equal(rope["k_cache"], kc_ref) and torch.equal(rope["v_cache"], vc_ref)


# ------------------------------------------------------------------------------------------------ arg-max candidates
@gpu
@pytest.mark.parametrize("n,k,m,groups", [(16384, 64, 17, 1024), (16400, 64, 49, 512), (2048, 896, 5, 128)])
def test_candidates_reduce_to_exact_argmax(n, k, m, groups):
    """Integer outputs tie all the time (and two weight rows are duplicated on top): the candidate records of each grid form,
    reduced over the groups, must be exactly (max, LOWEST arg-max) of the integer reference, whether or not the logits are
    written as well."""
    from nanovllm_hip import ops
    c = _case("none", m, n, k, dup=True)
    d = {key: _dev(c[key]) for key in ("x", "w", "bias", "res")}
    ref = c["ref"].float()
    best_ref = ref.max(dim=1).values
    idx_ref = torch.where(ref == best_ref[:, None], torch.arange(n)[None, :], n).min(dim=1).values
    assert ops.linear_candidate_groups(n, k) == groups             # 1024: one tile per workgroup; 512: MULTI
    for want_out in (True, False):
        cv = torch.full((groups, 64), float("nan"), dtype=torch.float32, device="cuda")
        ci = torch.full((groups, 64), -1, dtype=torch.int32, device="cuda")
        out = ops.fused_linear(d["x"], d["w"], candidates=(cv, ci), want_out=want_out)
        torch.cuda.synchronize()
        assert (out is None) == (not want_out)
        if want_out:
            assert torch.equal(out.cpu(), c["ref"])
        vals, idxs = cv[:, :m].cpu(), ci[:, :m].cpu().long()
        best = vals.max(dim=0).values                              # (a group that wrote nothing leaves NaN: max is NaN)
        idx = torch.where(vals == best[None, :], idxs, n).min(dim=0).values
        assert torch.equal(best, best_ref) and torch.equal(idx, idx_ref)
        assert bool(torch.isnan(cv[:, m:]).all()) and bool((ci[:, m:] == -1).all())     # rows >= M: never written
