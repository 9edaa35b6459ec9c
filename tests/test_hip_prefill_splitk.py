"""Split-key prefill against plain float64 softmax attention on the CPU (bf16 inputs taken exactly, bottom-right causal mask, keys gathered through
the block table).  Bar: tests/test_hip_parity.py's, 1e-3 for fp32 output, 1e-3 + one bf16 ulp for bf16 output.  The ragged batch: more splits than key
tiles, the ragged last tile and the diagonal in the last split, a q-tile with one key tile, an empty sequence."""
import ctypes
import functools

import numpy as np
import pytest
import torch

ATOL, BF16_ULP = 1e-3, 2.0 ** -8
BS = 256
SEQS = [(1, 200), (16, 333), (70, 70 + 256), (64, 64), (0, 0)]           # (sq, sk)
HEADS = [(14, 2, 64), (16, 8, 64), (14, 2, 128), (16, 8, 128)]


def reference(q, k, v, seqs, scale):
    """float64 softmax attention per sequence; q [Tq, H, D], k / v [Tk, KVH, D] (CPU), query r sees keys <= r + (sk - sq)"""
    out = torch.zeros(q.shape, dtype=torch.float64)
    g = q.shape[1] // k.shape[1]
    q0 = k0 = 0
    for sq, sk in seqs:
        if sq and sk:
            kk = k[k0:k0 + sk].double().repeat_interleave(g, dim=1)
            vv = v[k0:k0 + sk].double().repeat_interleave(g, dim=1)
            s = torch.einsum("qhd,khd->hqk", q[q0:q0 + sq].double(), kk) * scale
            seen = torch.arange(sk)[None, :] <= torch.arange(sq)[:, None] + (sk - sq)
            p = torch.softmax(s.masked_fill(~seen, float("-inf")), dim=-1)
            out[q0:q0 + sq] = torch.einsum("hqk,khd->qhd", p, vv)
        q0, k0 = q0 + sq, k0 + sk
    return out.numpy()


@functools.lru_cache(maxsize=None)
def case(h, kvh, d):
    """One ragged batch per head shape, inputs on the GPU in both K / V layouts, and its reference (computed once)."""
    gen = torch.Generator().manual_seed(h * 1000 + d)
    tq, tk = sum(s[0] for s in SEQS), sum(s[1] for s in SEQS)
    q, k, v = (torch.randn(n, hh, d, generator=gen).bfloat16() for n, hh in ((tq, h), (tk, kvh), (tk, kvh)))
    cu = lambda i: torch.tensor(np.concatenate([[0], np.cumsum([s[i] for s in SEQS])]), dtype=torch.int32).cuda()
    blocks = [(sk + BS - 1) // BS for _, sk in SEQS]
    ids = iter(torch.randperm(sum(blocks), generator=gen).tolist())
    table = torch.full((len(SEQS), max(blocks) + 1), -1, dtype=torch.int32)
    kc, vc = (torch.zeros(sum(blocks), BS, kvh, d, dtype=torch.bfloat16) for _ in range(2))
    k0 = 0
    for i, (_, sk) in enumerate(SEQS):
        for j in range(blocks[i]):
            table[i, j] = next(ids)
            n = min(BS, sk - j * BS)
            kc[table[i, j], :n], vc[table[i, j], :n] = k[k0 + j * BS:k0 + j * BS + n], v[k0 + j * BS:k0 + j * BS + n]
        k0 += sk
    return dict(q=q.cuda(), cu_q=cu(0), cu_k=cu(1), max_q=max(s[0] for s in SEQS), max_k=max(s[1] for s in SEQS), scale=d ** -0.5,
                packed=(k.cuda(), v.cuda(), None), paged=(kc.cuda(), vc.cuda(), table.cuda()), expected=reference(q, k, v, SEQS, d ** -0.5))


def check_close(got, expected, what):
    """got: a bf16 or fp32 GPU tensor"""
    err = np.abs(got.double().cpu().numpy() - expected)
    print(f"{what} {got.dtype}: max err {err.max():.3e}")
    assert (err <= ATOL + (BF16_ULP * np.abs(expected) if got.dtype == torch.bfloat16 else 0)).all(), f"{what} {got.dtype}: off by {err.max():.3e}"


def splitk_raw(c, layout, out, key_splits, ws):
    """nvh_prefill_varlen_splitk itself, on torch's current stream; ws: a uint8 GPU tensor or None"""
    from nanovllm_hip import _lib
    q, (k, v, bt) = c["q"], c[layout]
    _, h, d = q.shape
    paged = bt is not None
    rc = _lib.load().nvh_prefill_varlen_splitk(
        out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), c["cu_q"].data_ptr(), c["cu_k"].data_ptr(), bt.data_ptr() if paged else None,
        len(SEQS), c["max_q"], c["max_k"], h, k.shape[-2], d, BS if paged else 0, bt.shape[1] if paged else 0, q.stride(0),
        0 if paged else k.stride(0), 0 if paged else v.stride(0), bt.stride(0) if paged else 0, c["scale"], 0, 0 if out.dtype == torch.bfloat16 else 1,
        torch.cuda.current_stream().cuda_stream, key_splits, ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0)
    _lib.check(rc, "nvh_prefill_varlen_splitk")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("key_splits", [2, 3, 5])
@pytest.mark.parametrize("layout", ["paged", "packed"])
@pytest.mark.parametrize("h,kvh,d", HEADS)
def test_parity(h, kvh, d, layout, key_splits):
    from nanovllm_hip import ops
    c = case(h, kvh, d)
    k, v, bt = c[layout]
    for dt in (torch.float32, torch.bfloat16):
        got = ops.flash_attn_varlen_func(c["q"], k, v, c["max_q"], c["cu_q"], c["max_k"], c["cu_k"], softmax_scale=c["scale"], block_table=bt,
                                         out_dtype=dt, key_splits=key_splits)
        check_close(got, c["expected"], f"{h}/{kvh}/{d} {layout} key_splits={key_splits}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["paged", "packed"])
@pytest.mark.parametrize("h,kvh,d", [(14, 2, 64), (16, 8, 128)])
def test_one_split_is_todays_launch(h, kvh, d, layout):
    from nanovllm_hip import ops
    c = case(h, kvh, d)
    k, v, bt = c[layout]
    for dt in (torch.float32, torch.bfloat16):
        today = ops.flash_attn_varlen_func(c["q"], k, v, c["max_q"], c["cu_q"], c["max_k"], c["cu_k"], softmax_scale=c["scale"], block_table=bt, out_dtype=dt)
        assert torch.equal(splitk_raw(c, layout, torch.zeros_like(today), 1, None), today)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["paged", "packed"])
@pytest.mark.parametrize("h,kvh,d", [(14, 2, 64), (16, 8, 128)])
def test_deterministic_and_reusable(h, kvh, d, layout):
    from nanovllm_hip import _lib
    c = case(h, kvh, d)
    need = _lib.load().nvh_prefill_splitk_workspace(len(SEQS), c["max_q"], c["max_k"], h, d, 3, 0)
    assert need > 65536
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    outs = [splitk_raw(c, layout, torch.zeros_like(c["q"]), 3, ws) for _ in range(2)]
    replayed = torch.zeros_like(c["q"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        splitk_raw(c, layout, replayed, 3, ws)
    for _ in range(3):                                                   # several replays, each against the eager result
        replayed.zero_()
        graph.replay()
        outs.append(replayed.clone())
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    check_close(outs[0], c["expected"], "reused workspace")
    assert not ws[:65536].any(), "every launch leaves its tickets at zero"


@pytest.mark.gpu
@pytest.mark.parametrize("h,kvh,d", [(14, 2, 64), (16, 8, 128)])
def test_module_reads_the_prefix_cache_in_splits(h, kvh, d):
    """Attention.forward in prefill with Context.block_tables: the new rows are stored, then all keys are read through the cache, two splits per q-tile."""
    from nanovllm_hip import reset_context, set_context
    from nanovllm_hip.layers.attention_hip import Attention
    seqs, tables = [(40, 340), (17, 17 + 256)], [[3, 1, -1], [0, 2, -1]]     # (new tokens, all tokens), blocks of 256
    gen = torch.Generator().manual_seed(d)
    tq, tk = sum(s[0] for s in seqs), sum(s[1] for s in seqs)
    k_all, v_all = (torch.randn(tk, kvh, d, generator=gen).bfloat16() for _ in range(2))
    q = torch.randn(tq, h, d, generator=gen).bfloat16()
    kc, vc = (torch.zeros(4, BS, kvh, d, dtype=torch.bfloat16) for _ in range(2))
    new_rows, slots, k0 = [], [], 0
    for (sq, sk), tab in zip(seqs, tables):
        for t in range(sk):
            slot = tab[t // BS] * BS + t % BS
            if t < sk - sq:                                              # the cached prefix is in the cache already
                kc.view(-1, kvh, d)[slot], vc.view(-1, kvh, d)[slot] = k_all[k0 + t], v_all[k0 + t]
            else:
                new_rows.append(k0 + t)
                slots.append(slot)
        k0 += sk
    attn = Attention(h, d, d ** -0.5, kvh, prefill_key_splits=2)
    attn.k_cache, attn.v_cache = kc.cuda(), vc.cuda()
    cu = lambda i: torch.tensor(np.concatenate([[0], np.cumsum([s[i] for s in seqs])]), dtype=torch.int32).cuda()
    set_context(True, cu(0), cu(1), 40, 340, torch.tensor(slots, dtype=torch.int32).cuda(), None, torch.tensor(tables, dtype=torch.int32).cuda())
    try:
        o = attn(q.cuda().view(tq, h * d), k_all[new_rows].cuda().view(tq, kvh * d), v_all[new_rows].cuda().view(tq, kvh * d))
    finally:
        reset_context()
    check_close(o.view(tq, h, d), reference(q, k_all, v_all, seqs, d ** -0.5), f"module {h}/{kvh}/{d}")


# ---------------------------------------------------------------------------------------------- CPU
def test_argument_errors():
    from nanovllm_hip import _lib, ops
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    call = lambda splits, ws, nbytes, hd=64: lib.nvh_prefill_varlen_splitk(p, p, p, p, p, p, p, 1, 64, 4096, 14, 2, hd, 256, 16, 896, 128, 128, 16, 0.125, 0, 0,
                                                                          None, splits, ws, nbytes)
    assert lib.nvh_prefill_splitk_workspace(1, 64, 4096, 14, 64, 4, 256) == 65536 + 14 * 4 * 64 * 68 * 4
    assert lib.nvh_prefill_splitk_workspace(1, 64, 4096, 14, 64, 1, 256) == 0
    assert call(4, p, 65536) == -4 and b"workspace" in lib.nvh_last_error()
    assert call(4, None, 0) == -5
    assert call(-1, p, 1 << 30) == -2 and call(4, p, 1 << 30, hd=96) == -2
    q = torch.zeros(1, 14, 64, dtype=torch.bfloat16)
    for bad in (dict(kernel="tiled"), dict(short_waves=8), dict(pv_fp16=True)):
        with pytest.raises(ValueError, match="key_splits"):
            ops.flash_attn_varlen_func(q, q, q, 1, None, 1, None, key_splits=2, **bad)


def test_plan_rule():
    from nanovllm_hip import _lib
    lib = _lib.load()

    def plan(batch, max_q, max_k, forced=0):
        s = ctypes.c_int(-1)
        assert lib.nvh_plan_prefill_splitk(ctypes.byref(s), forced, batch, max_q, max_k, 14, 2, 64, 1, 256) == 0
        return s.value

    assert plan(16, 512, 1024) == 1                  # 1792 workgroups unsplit: at least 2 x CUs
    assert plan(5, 512, 4096) == 1                   # 560: still at least 512
    assert plan(1, 64, 4096) == 8                    # a follow-up chat turn on a long history: 14 workgroups unsplit, 8 key tiles per split
    assert plan(1, 64, 4096, forced=100) == 16       # forced: the absolute cap ...
    assert plan(1, 64, 200, forced=100) == 4         # ... and the key tiles of max_seqlen_k
    assert plan(1, 64, 64, forced=3) == 1
    assert plan(64, 64, 4096, forced=2) == 1         # 896 q-tiles: more than the 512 tickets
    assert plan(64, 64, 4096) == 1
