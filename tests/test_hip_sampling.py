"""GPU: temperature sampling on the device (csrc/sample_noise.h, sample.hip, the sampled candidates of linear_stream.hip) against
a float64 numpy restatement of the noise definition: token = argmax_j (l_j + T g_j), g = -ln(-ln u), u = ((bits >> 9) + 0.5) 2^-23,
bits = word (j & 3) of Philox4x32-10 with key (seed_lo, seed_hi) and counter (j >> 2, row_key, step_lo, step_hi).
Tokens are compared EXACTLY: every case first asserts that the float64 top-two gap of every row exceeds 2 T 2^-10, twice the
error budget of the fp32 noise (the seeds below were chosen on the CPU so that it holds)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = np.uint64
MASK = U(0xFFFFFFFF)


def philox(ctr, key):
    c = [np.asarray(x, U) for x in np.broadcast_arrays(*ctr)]
    k0, k1 = U(key[0]), U(key[1])
    for _ in range(10):
        p0, p1 = c[0] * U(0xD2511F53), c[2] * U(0xCD9E8D57)
        c = [(p1 >> U(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> U(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + U(0x9E3779B9)) & MASK, (k1 + U(0xBB67AE85)) & MASK
    return c


def gumbel64(seed, key, step, n):
    """g of columns 0..n-1, [..., n] for keys / steps [...]: one Philox call per four columns, column j = word j & 3."""
    key, step = np.asarray(key, U)[..., None], np.asarray(step, U)[..., None]
    w = philox([np.arange((n + 3) // 4, dtype=U), key, step & MASK, step >> U(32)], [seed & 0xFFFFFFFF, seed >> 32])
    bits = np.stack(w, axis=-1).reshape(*w[0].shape[:-1], -1)[..., :n]
    return -np.log(-np.log(((bits >> U(9)).astype(np.float64) + 0.5) * 2.0 ** -23))


for _c, _k, _out in (([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"), ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                     ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1")):
    assert " ".join(f"{int(x):08x}" for x in philox(_c, _k)) == _out


def ref_tokens(logits, temps, keys, steps, seed):
    """float64 arg-max of l + T g per row and the precondition: every row's top-two gap > 2 T 2^-10."""
    l = logits.float().cpu().numpy().astype(np.float64)
    t = np.asarray(temps, np.float64)[:, None]
    s = l + t * gumbel64(seed, keys, steps, l.shape[1])
    top = np.sort(np.partition(s, -2, axis=1)[:, -2:], axis=1)
    gap = top[:, 1] - top[:, 0]
    assert (gap > 2 * t[:, 0] * 2.0 ** -10).all(), f"top-two gap inside the noise budget in rows {np.nonzero(gap <= 2 * t[:, 0] * 2.0 ** -10)[0]}"
    return s.argmax(axis=1)


def rows_inputs(m, dev, first_key=7, first_step=3):
    temps = [(0.0, 0.5, 1.0, 1.5)[i % 4] for i in range(m)]
    keys, steps = [first_key + 3 * i for i in range(m)], [first_step + i for i in range(m)]
    return (temps, keys, steps), (torch.tensor(temps, device=dev), torch.tensor(keys, dtype=torch.uint32).to(dev), torch.tensor(steps, device=dev))


@pytest.mark.parametrize("seed,key,step", [(0, 0, 0), (0x1234ABCD5678, 0xFFFFFFFF, 5), (3, 17, (1 << 40) + 9), ((1 << 63) + 12345, 2, (1 << 64) - 1)])
def test_noise_matches_float64(seed, key, step):
    from nanovllm_hip import ops
    n = 1 << 16
    g = ops.gumbel_noise(seed, key, step, n).cpu().numpy().astype(np.float64)
    g64 = gumbel64(seed, key, step, n)
    err = np.abs(g - g64).max()
    print(f"gumbel_noise seed {seed:#x} key {key:#x} step {step:#x}: max |g - g64| = {err:.3e}, g in [{g.min():.3f}, {g.max():.3f}]")
    assert err <= 2.0 ** -10
    if (seed, key, step) == (0, 0, 0):                           # columns 0..3 are the four words of the first known-answer vector
        bits = np.array([0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], U)
        assert np.abs(g[:4] + np.log(-np.log(((bits >> U(9)).astype(np.float64) + 0.5) * 2.0 ** -23))).max() <= 2.0 ** -10


# n = 5: the n % 8 tail alone, no 16-byte chunk; n = 8200: one full sweep of the 1024 threads plus one chunk
@pytest.mark.parametrize("m,n,lseed,seed", [(3, 1003, 1, 11), (64, 151936, 2, (1 << 33) + 5), (3, 5, 1, 5), (2, 8200, 1, 3)])
def test_sample_rows_equals_float64_argmax(m, n, lseed, seed):
    from nanovllm_hip import ops
    dev = torch.device("cuda")
    stride = (n + 7) // 8 * 8
    logits = torch.zeros(m, stride, dtype=torch.bfloat16)
    logits[:, :n] = (3 * torch.randn(m, n, generator=torch.Generator().manual_seed(lseed))).bfloat16()
    logits = logits.to(dev)[:, :n]
    (temps, keys, steps), tensors = rows_inputs(m, dev)
    ref = ref_tokens(logits, temps, keys, steps, seed)
    got = ops.sample_rows(logits, *tensors, seed).cpu().numpy()
    assert np.array_equal(got, ref)
    greedy = torch.argmax(logits.float(), dim=-1).cpu().numpy()
    assert np.array_equal(got[0::4], greedy[0::4]) and (got != greedy).any()


def advance_state(m, dev, steps=4):
    return dict(input_ids=torch.zeros(m, dtype=torch.int64, device=dev), positions=torch.full((m,), 10, dtype=torch.int64, device=dev),
                context_lens=torch.full((m,), 10, dtype=torch.int32, device=dev), slot_mapping=torch.full((m,), 9, dtype=torch.int32, device=dev),
                block_tables=torch.zeros(m, 1, dtype=torch.int32, device=dev), block_size=256,
                tokens_log=torch.zeros(steps, m, dtype=torch.int64, device=dev), row_steps=torch.zeros(m, dtype=torch.int64, device=dev))


@pytest.mark.parametrize("m", [1, 17, 64])
def test_fused_lm_head_samples_its_own_logits(m):
    from nanovllm_hip import ops
    dev = torch.device("cuda")
    k, n, seed = 128, 16 * 1025, 21                              # 1025 tiles: the multi-tile form (> 1024), every workgroup owns 2 tiles or more
    groups = ops.linear_candidate_groups(n, k)
    assert 1 < groups and n // 16 >= 2 * groups
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(m, k, generator=gen).bfloat16().to(dev)
    w = (torch.randn(n, k, generator=gen) * 3 / k ** 0.5).bfloat16().to(dev)
    (temps, keys, _), (t_t, t_k, _) = rows_inputs(m, dev)
    st = advance_state(m, dev)
    st["row_steps"] += 2                                         # the noise step is the advance counter
    cand = lambda: (torch.zeros(groups, 64, dtype=torch.float32, device=dev), torch.zeros(groups, 64, dtype=torch.int32, device=dev))
    cv, ci = cand()
    out = ops.fused_linear(x, w, candidates=(cv, ci), sampling=(t_t, t_k, st["row_steps"], seed), want_out=True)
    by_rows = ops.sample_rows(out, t_t, t_k, st["row_steps"].clone(), seed)
    ops.greedy_advance_candidates(cv, ci, groups, m, *(st[f] for f in ("input_ids", "positions", "context_lens", "slot_mapping", "block_tables", "block_size", "tokens_log", "row_steps")))
    ref = ref_tokens(out, temps, keys, [2] * m, seed)
    assert np.array_equal(st["input_ids"].cpu().numpy(), ref) and np.array_equal(by_rows.cpu().numpy(), ref)
    # temperature 0 everywhere is the greedy launch, bit for bit
    (cv0, ci0), (cvz, ciz) = cand(), cand()
    out0 = ops.fused_linear(x, w, candidates=(cv0, ci0), want_out=True)
    ops.fused_linear(x, w, candidates=(cvz, ciz), sampling=(torch.zeros_like(t_t), t_k, st["row_steps"], seed), want_out=False)
    assert torch.equal(out0, out) and torch.equal(cv0[:, :m], cvz[:, :m]) and torch.equal(ci0[:, :m], ciz[:, :m])
    assert torch.equal(cv0[:groups, :m].max(dim=0).values, out.float().max(dim=1).values)


def test_graph_replay_draws_fresh_noise():
    from nanovllm_hip import ops
    dev = torch.device("cuda")
    m, n, seed = 4, 1003, 9
    logits = (3 * torch.randn(m, 1008, generator=torch.Generator().manual_seed(3))).bfloat16().to(dev)[:, :n]
    (temps, keys, _), (t_t, t_k, _) = rows_inputs(m, dev)
    st = advance_state(m, dev)
    call = lambda: ops.sample_advance(logits, *(st[f] for f in ("input_ids", "positions", "context_lens", "slot_mapping", "block_tables", "block_size", "tokens_log", "row_steps")), t_t, t_k, seed)
    call()                                                       # loads the kernel outside the capture
    eager0 = st["tokens_log"][0].clone()
    for f, v in (("row_steps", 0), ("positions", 10), ("context_lens", 10), ("tokens_log", 0)):
        st[f].fill_(v)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    ref = np.stack([ref_tokens(logits, temps, keys, [s] * m, seed) for s in range(3)])
    assert np.array_equal(st["tokens_log"][:3].cpu().numpy(), ref) and torch.equal(eager0, st["tokens_log"][0])
    assert (st["row_steps"] == 3).all() and (ref[0] != ref[1]).any()


def test_engine_generates_sampled_tokens():
    from nanovllm_hip.engine.llm_engine import LLMEngine
    from nanovllm_hip.engine.sequence import Sequence
    from nanovllm_hip.models import qwen
    cfg = qwen.model_config("Qwen2-0.5B", num_hidden_layers=2, vocab_size=2048)
    eng = LLMEngine(cfg, num_kvcache_blocks=12, seed=4)
    gen = torch.Generator().manual_seed(11)
    prompts = [torch.randint(0, 2048, (n,), generator=gen).tolist() for n in (300, 17, 256, 1)]
    temps, new = [0.0, 0.8, 0.0, 1.2], 17

    def run(temperature, seed, graph=True):
        Sequence.counter = itertools.count()                     # the noise key of a request is its sequence id
        cfg.seed = seed
        if graph:
            return eng.generate(prompts, new, temperature=temperature)
        seqs = [Sequence(p, max_tokens=new, temperature=t) for p, t in zip(prompts, temperature)]
        eng.prefill(seqs, reserve_tokens=new)
        sess = eng.runner.decode_session(seqs, new - 1, use_graph=False)
        sess.step(new - 1)
        sess.finish()
        for s in seqs:
            eng.block_manager.deallocate(s)
        return [s.completion_token_ids for s in seqs]

    greedy, a, a2, b, eager = run(0.0, 1), run(temps, 1), run(temps, 1), run(temps, 2), run(temps, 1, graph=False)
    assert all(len(r) == new for r in a)
    assert a[0] == greedy[0] and a[2] == greedy[2] and b[0] == greedy[0] and b[2] == greedy[2]
    assert a == a2 and a == eager
    assert a[1] != b[1] or a[3] != b[3]
    assert a[1] != greedy[1] or a[3] != greedy[3]
