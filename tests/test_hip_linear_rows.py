"""GPU: the row-split streaming GEMM for 65..256 rows (csrc/linear_rows.hip) against an EXACT reference, as test_hip_linear_exact.py:
x holds integers in [-2, 2] (norm_folded: +-1, so the row scale 1 - 5e-7 rounds away), weight rows at most 128 entries of +-1, so
every result is a bf16 integer and the float64 reference is compared with torch.equal.
Launch forms (rows_shape in linear_rows.hip), with units = N / 16 (silu / rope: weight rows / 32) and pieces = K / 64:
    RT     = 1 up to 128 rows (8 waves, one row tile each), 2 above
    NB     = 4 weight-row blocks per workgroup when ceil(units / (4, paired: 2)) >= 512, else 2
    ksplit = max(ceil(pieces / 16), tiles < 128 ? min(256 // tiles, pieces // 4) : 1)
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC1                     # a quiet-NaN bf16 pattern no kernel produces


def _pm1_rows(gen, n, k, nnz, distinct=False):
    idx = torch.rand(n, k, generator=gen).argsort(1)[:, :nnz] if distinct else torch.randint(0, k, (n, nnz), generator=gen)
    sgn = (torch.randint(0, 2, idx.shape, generator=gen) * 2 - 1).float()
    return torch.zeros(n, k).scatter_(1, idx, sgn)


_round_trips = lambda t64: torch.equal(t64.float().bfloat16().double(), t64)


def _silu_tie_margin():
    """Smallest relative distance of float64 silu(g), g an integer in [-8, 8] \\ {0}, from a bf16 rounding tie."""
    worst = 1.0
    for g in [g for g in range(-8, 9) if g]:
        v = abs(g / (1.0 + math.exp(-g)))
        ulp = 2.0 ** (math.frexp(v)[1] - 8)
        worst = min(worst, abs(v / ulp - math.floor(v / ulp) - 0.5) * ulp / v)
    return worst


@functools.lru_cache(maxsize=None)
def _case(epi, m, n, k, bias=False, pm1=False):
    """CPU operands (bf16) and the exact expected output; n = weight rows, except silu_mul: n = inter (gate rows first)."""
    gen = torch.Generator().manual_seed(7919 * m + 31 * n + k)
    sign = torch.randint(0, 2, (m, k), generator=gen).float() * 2 - 1
    if pm1:
        x = sign
    elif epi == "silu_mul":                                     # mostly +-1, a few +-2: every gate in [-6, 6] occurs, few are zero
        x = sign * (1 + (torch.rand(m, k, generator=gen) < 0.04).float())
    else:
        x = torch.randint(-2, 3, (m, k), generator=gen).float()
    b = torch.randint(-8, 9, (n,), generator=gen).float() if bias else None
    res = torch.randint(-64, 65, (m, n), generator=gen).float() if epi == "residual_add" else None
    for nnz in (128, 96):                                       # 96: the redraw for a sum that leaves the exact range
        w = _pm1_rows(gen, n, k, nnz)
        if epi == "silu_mul":
            w = torch.cat([_pm1_rows(gen, n, k, 3, distinct=True), w])
        y = x.double() @ w.double().T
        if pm1 and res is not None:                             # keep the folded norm off exact cancellation (5e-7 * y would be left)
            res = torch.where((y + res.double() == 0) & (y != 0), res + 1, res)
        full = y + (b.double() if bias else 0) + (res.double() if res is not None else 0)
        if _round_trips(y) and _round_trips(full):
            break
    assert _round_trips(y) and _round_trips(full), "the reference is not exactly representable in bf16"
    ref = full.float().bfloat16()
    if epi == "silu_mul":
        g, u = y[:, :n], y[:, n:]
        assert float(g.abs().max()) <= 8 and _silu_tie_margin() >= 2.0 ** -16
        ref = ((g / (1.0 + torch.exp(-g))).float().bfloat16().double() * u).float().bfloat16()      # rounded once, as the kernel does
    assert float((ref == 0).float().mean()) <= 0.10, "too much of the reference is zero"
    to = lambda t: None if t is None else t.bfloat16().cuda()
    return dict(epi=epi, m=m, k=k, wrows=w.shape[0], x=to(x), w=to(w), bias=to(b), res=to(res), ref=ref.cuda(), pm1=pm1)


def _run(c, ws, **kw):
    from nanovllm_hip import ops
    out = c["res"].clone() if c["epi"] == "residual_add" else None
    kw.setdefault("x", c["x"])
    return ops.fused_linear(kw.pop("x"), c["w"], bias=c["bias"], epilogue=c["epi"], out=out, workspace=ws, norm_folded=c["pm1"], norm_eps=1e-6, **kw)


def _workspace(c, split, tiles):                                # zero-filled; split-K <=> workspace bytes > 0, as the tables state
    from nanovllm_hip import ops
    need = ops.linear_workspace_bytes(c["m"], c["wrows"], c["k"], c["epi"])
    assert (need > 0) == split and need >= (tiles * 128 if split else 0)
    return torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda") if need else None


_tickets_zero = lambda ws, tiles: ws is None or int(ws[: tiles * 128].view(torch.int32).abs().sum()) == 0   # one ticket per 128-byte line


# (epilogue, N or inter, K, M, bias, folded, split, tiles): the launch form each row takes
ROWS = [
    ("none", 32, 64, 65, True, False, False, 1),             # one tile, one piece, one live row in the fifth row tile, RT 1
    ("none", 48, 448, 80, False, True, False, 2),            # ragged second tile (one block); 7 pieces: just under the narrow-N split
    ("none", 48, 512, 129, True, False, True, 2),            # 8 pieces -> ksplit 2, RT 2 (wave 0 owns row tiles 0 and 8)
    ("none", 4096, 1024, 65, False, False, False, 128),      # 128 tiles: no fill split; 16 pieces, the whole LDS image
    ("none", 4096, 1088, 256, False, True, True, 128),       # 17 pieces -> ksplit 2 (9 + 8), all 16 row tiles
    ("none", 32784, 64, 256, False, False, False, 513),      # 2049 units -> NB 4 (64 columns), last tile holds one block
    ("silu_mul", 16, 64, 65, False, False, False, 1),
    ("silu_mul", 32, 448, 256, False, True, False, 2),
    ("silu_mul", 48, 512, 80, False, False, True, 3),        # ksplit 2: both row blocks of a record
    ("silu_mul", 16400, 64, 129, False, False, False, 513),  # 1025 units -> NB 4 (32 + 32 columns), last tile holds one unit
    ("residual_add", 32, 64, 80, False, False, False, 1),
    ("residual_add", 48, 448, 65, False, False, False, 2),
    ("residual_add", 48, 512, 256, False, True, True, 2),
    ("residual_add", 896, 4864, 129, False, False, True, 28),  # Qwen2-0.5B down_proj: 76 pieces -> ksplit 9 (8 or 9 pieces each)
]


@pytest.mark.parametrize("epi,n,k,m,bias,folded,split,tiles", ROWS)
def test_exact(epi, n, k, m, bias, folded, split, tiles):
    c = _case(epi, m, n, k, bias=bias, pm1=folded)
    ws = _workspace(c, split, tiles)
    outs = [_run(c, ws) for _ in range(3 if split else 1)]      # split-K: three launches on one workspace
    torch.cuda.synchronize()
    for o in outs:
        bad = (o != c["ref"]).nonzero()
        assert torch.equal(o, c["ref"]), f"{bad.shape[0]} wrong elements, first (row, col) {bad[:4].tolist()}"
    assert _tickets_zero(ws, tiles)


# (H, KVH, D, K, M, folded, split): tiles = (H + 2 KVH) * D / 32
ROPE_ROWS = [
    (2, 1, 64, 64, 65, False, False),       # 8 tiles, one piece
    (14, 2, 64, 896, 80, True, True),       # Qwen2-0.5B qkv: 36 tiles, 14 pieces -> ksplit 3
    (2, 1, 128, 448, 129, False, False),    # D = 128 (four units per head), 7 pieces: unsplit
    (7, 1, 128, 3584, 256, False, True),    # 36 tiles, 56 pieces -> ksplit 7
]


@pytest.mark.parametrize("h,kvh,hd,k,m,folded,split", ROPE_ROWS)
def test_exact_rope_store(h, kvh, hd, k, m, folded, split):
    """The projection (+ integer bias) is exact, so the epilogue must give, bit for bit, nvh_rope_store of the exact bf16 qkv:
    q and both caches, rows with slot -1 untouched."""
    from nanovllm_hip import ops
    from nanovllm_hip.models.qwen import cos_sin_table
    c = _case("rope_store", m, (h + 2 * kvh) * hd, k, bias=not folded, pm1=folded)
    tiles = (h + 2 * kvh) * hd // 32
    ws = _workspace(c, split, tiles)
    gen = torch.Generator().manual_seed(h * 131 + hd + m)
    pos = torch.randint(0, 4096, (m,), generator=gen).cuda()
    slots = torch.randperm(4 * 64, generator=gen)[:m].int()
    slots[0::9] = -1
    slots = slots.cuda()
    table = cos_sin_table(hd, 4096, 1e6, "cuda")
    kc0, vc0 = (torch.randn(4, 64, kvh, hd, generator=gen).bfloat16().cuda() for _ in range(2))
    q_ref, kc_ref, vc_ref = c["ref"].clone(), kc0.clone(), vc0.clone()
    ops.rope_store(q_ref, pos, table, h, kvh, hd, kc_ref, vc_ref, slots)      # rotates q and k in place, stores k and v
    for _ in range(3 if split else 1):
        rope = dict(positions=pos, cos_sin=table, k_cache=kc0.clone(), v_cache=vc0.clone(), slot_mapping=slots, num_heads=h, num_kv_heads=kvh, head_dim=hd)
        q = _run(c, ws, rope=rope)
        assert torch.equal(q, q_ref[:, :h * hd]) and torch.equal(rope["k_cache"], kc_ref) and torch.equal(rope["v_cache"], vc_ref)
    assert _tickets_zero(ws, tiles)


@pytest.mark.parametrize("epi,n,k,m,split,tiles", [("none", 64, 512, 80, True, 2), ("silu_mul", 32, 64, 129, False, 2), ("residual_add", 64, 448, 65, False, 2)])
def test_packed_forms_change_no_bit(epi, n, k, m, split, tiles):
    """Fragment-order x (zero or NaN padding rows) gives the bits of row-major x; out_packed unpacks to `out` and its padding
    rows are never written."""
    from nanovllm_hip import ops
    c = _case(epi, m, n, k)
    ws = _workspace(c, split, tiles)
    rows16 = (m + 15) // 16 * 16
    nan_pad = torch.full((rows16, k), NAN_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    nan_pad[:m] = c["x"]
    for xp in (ops.pack_rows(c["x"]), ops.pack_rows(nan_pad)):
        assert torch.equal(_run(c, ws, x=xp, x_packed_rows=m), c["ref"])
    packed = torch.full((rows16 * n,), NAN_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    assert torch.equal(_run(c, ws, out_packed=packed), c["ref"])
    un = ops.unpack_rows(packed, rows16, n)
    assert torch.equal(un[:m], c["ref"]) and bool((un[m:].contiguous().view(torch.int16) == NAN_BITS).all())
    assert _tickets_zero(ws, tiles)


def test_fused_decode_layer_80_rows():
    """One decode step over 80 rows of the two-layer toy model of test_hip_model_vs_oracle.py through _forward_decode_fused
    against the plain layer body; that file's bars for a fused decode step (0.03 of the largest logit, 2^-6 of the mean)."""
    from nanovllm_hip.engine import llm_engine, model_runner, sequence
    from nanovllm_hip.models import qwen
    from nanovllm_hip.utils.context import reset_context, set_context
    cfg = qwen.model_config("Qwen2-0.5B", num_hidden_layers=2, vocab_size=2048)
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, 2048, (1 + (7 * i) % 40,), generator=g).tolist() for i in range(80)]
    eng = llm_engine.LLMEngine(cfg, num_kvcache_blocks=96, enforce_eager=True, seed=3)
    seqs = [sequence.Sequence(p, max_tokens=4) for p in prompts]
    eng.prefill(seqs, reserve_tokens=4)
    r = eng.runner
    m = model_runner.build_decode_meta(seqs, r.block_size)
    logits = {}
    for fused in (True, False):                                 # the same step twice: it stores the same K/V rows again
        qwen.FUSED_DECODE = fused
        try:
            with torch.inference_mode():
                set_context(False, slot_mapping=r._dev(m["slot_mapping"]), context_lens=r._dev(m["context_lens"]), block_tables=r._dev(m["block_tables"]))
                hidden = r.model(r._dev(m["input_ids"]), r._dev(m["positions"]))
                assert isinstance(hidden, qwen.PackedResidual) == fused
                logits[fused] = r.model.compute_logits(hidden).float().cpu()
                reset_context()
        finally:
            qwen.FUSED_DECODE = True
    diff = (logits[True] - logits[False]).abs()
    assert diff.max() <= 0.03 * logits[False].abs().max() and diff.mean() <= 2.0 ** -6 * logits[False].abs().mean()
