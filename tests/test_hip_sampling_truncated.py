"""GPU: top-k / top-p sampling (csrc/sample_truncated.hip) against a float64 numpy restatement of include/nvh_attn.h: value classes via
np.unique, w = exp((l - max) / T), top-k keeps the classes with fewer than k columns above them, top-p (over those) the classes whose
weight above is < top_p * Z plus the largest, token = argmax over the kept columns of l + T g with the noise of test_hip_sampling.py.
Tokens are compared EXACTLY; every case first asserts on the CPU (the seeds below were chosen there so that every row passes)
  (a) the float64 top-two gap among the kept columns exceeds 2 T 2^-10, as in test_hip_sampling.py;
  (b) where top-p is on, no class boundary's weight_above / Z lies within 2^-12 of top_p.  The kernel's weights are fp32
      exp2((l - max) * (log2 e / T)): two roundings of an argument below 41 in magnitude (smaller weights round to nothing) give
      41 ln2 2^-23 = 3.4e-6 relative, v_exp_f32 about 1e-7, the 2^-40 fixed point at most 2^-23 of Z in all: the ratio is off by
      under 1e-5, and 2^-12 leaves a margin above 20.  The largest class is exempt: nothing lies above it, 0 < top_p * Z is exact."""
import functools
import itertools

import numpy as np
import pytest
import torch
from test_hip_sampling import advance_state, gumbel64, rows_inputs

pytestmark = pytest.mark.gpu
ADVANCE_FIELDS = ("input_ids", "positions", "context_lens", "slot_mapping", "block_tables", "block_size", "tokens_log", "row_steps")


def ref_tokens(logits, temps, g, top_ks, top_ps):
    """(tokens, kept columns per row) of the float64 definition; asserts the preconditions (a) and (b)."""
    toks, kept = [], []
    for i, row in enumerate(logits.float().cpu().numpy().astype(np.float64)):
        t, k, p, n = temps[i], top_ks[i], float(np.float32(top_ps[i])), row.size
        if not t > 0:
            toks.append(row.argmax()), kept.append(n)
            continue
        vals, inv, cnt = np.unique(row, return_inverse=True, return_counts=True)        # classes, ascending
        keep = np.ones(vals.size, bool)
        if 0 < k < n:
            keep &= cnt[::-1].cumsum()[::-1] - cnt < k                                 # fewer than k columns above the class
        if p < 1:
            w = np.where(keep, cnt * np.exp((vals - vals[-1]) / t), 0.0)
            above = (w[::-1].cumsum()[::-1] - w) / w.sum()
            assert (np.abs(above[keep][:-1] - p) > 2.0 ** -12).all(), f"row {i}: a class boundary within 2^-12 of top_p"
            keep &= above < p
            keep[-1] = True
        mask = keep[inv.reshape(-1)]
        s = np.where(mask, row + t * g[i], -np.inf)
        top = np.sort(s[mask])[-2:]
        assert top.size < 2 or top[1] - top[0] > 2 * t * 2.0 ** -10, f"row {i}: top-two gap inside the noise budget"
        toks.append(s.argmax()), kept.append(mask.sum())
    return np.array(toks), np.array(kept)


@functools.lru_cache(maxsize=None)
def rows_case(m, n, lseed, seed, half_steps=False):
    """Logits (3 randn, or rounded to multiples of 0.5 with a last row of zeros), the per-row inputs and the float64 noise: built once."""
    dev = torch.device("cuda")
    logits = torch.zeros(m, (n + 7) // 8 * 8, dtype=torch.bfloat16)
    x = 3 * torch.randn(m, n, generator=torch.Generator().manual_seed(lseed))
    if half_steps:
        x = (2 * x).round() / 2
        x[-1] = 0
    logits[:, :n] = x.bfloat16()
    (temps, keys, steps), tensors = rows_inputs(m, dev)
    return logits.to(dev)[:, :n], temps, tensors, gumbel64(seed, keys, steps, n)


def run(case, seed, top_ks, top_ps):
    from nanovllm_hip import ops
    logits, temps, tensors, g = case
    ref, kept = ref_tokens(logits, temps, g, top_ks, top_ps)
    got = ops.sample_rows(logits, *tensors, seed, top_k=torch.tensor(top_ks, dtype=torch.int32).to(logits.device),
                          top_p=torch.tensor(top_ps, dtype=torch.float32).to(logits.device)).cpu().numpy()
    assert np.array_equal(got, ref), f"rows {np.nonzero(got != ref)[0]}: got {got}, float64 {ref}, kept {kept}"
    return got, kept


@pytest.mark.parametrize("top_p", [1.0, 0.8, 1e-6])
@pytest.mark.parametrize("top_k", [0, 1, 20, -1])                                       # -1: n itself
@pytest.mark.parametrize("m,n,lseed,seed", [(5, 1003, 2, 11), (8, 151936, 7, (1 << 33) + 5), (3, 5, 1, 7), (2, 8200, 1, 3)])   # 5: the tail alone; 8200: a sweep + one chunk
def test_grid_equals_float64(m, n, lseed, seed, top_k, top_p):
    from nanovllm_hip import ops
    case = rows_case(m, n, lseed, seed)
    logits, temps, tensors, _ = case
    got, kept = run(case, seed, [n if top_k < 0 else top_k] * m, [top_p] * m)
    plain = ops.sample_rows(logits, *tensors, seed).cpu().numpy()
    greedy = torch.argmax(logits.float(), dim=-1).cpu().numpy()
    assert np.array_equal(got[0::4], greedy[0::4])                                       # T = 0 rows
    if top_k in (0, -1) and top_p == 1.0:
        assert np.array_equal(got, plain) and (kept == n).all()
    if top_k == 1 or top_p == 1e-6:
        assert (kept[np.array(temps) > 0] == 1).all() and np.array_equal(got, greedy)    # a unique maximum in every row
    if top_k == 20 and top_p == 0.8:
        assert (got != plain).any() and (kept[np.array(temps) > 0] > 1).any()            # a cut that is neither everything nor the maximum alone


def test_ties_keep_the_whole_class():
    from nanovllm_hip import ops
    m, n, seed = 6, 40003, 13
    case = rows_case(m, n, 1, seed, half_steps=True)
    top_ks = [0, n // 2, n // 3, 20, 0, 5]
    got, kept = run(case, seed, top_ks, [1.0, 1.0, 0.8, 1.0, 1.0, 0.5])
    assert kept[1] > top_ks[1] + 1000 and kept[3] > 20 and kept[5] == n                     # thousands of columns tie at the k-th value
    assert got[5] == ops.sample_rows(case[0], *case[2], seed).cpu().numpy()[5]           # the all-zero row: nothing to truncate


def test_mixed_rows_in_one_launch():
    m, n, seed = 8, 1003, 17
    got, kept = run(rows_case(m, n, 1, seed), seed, [0, 20, 0, 5, n, 1, 50, -3], [0.5, 1.0, 0.8, 0.5, 1.0, 0.3, 0.9, 2.0])
    assert kept[7] == n and kept[1] >= 20 and 1 < kept[2] < n and kept[5] == 1


def test_graph_replay_truncated():
    from nanovllm_hip import ops
    dev = torch.device("cuda")
    m, n, seed = 4, 1003, 9
    logits = (3 * torch.randn(m, 1008, generator=torch.Generator().manual_seed(3))).bfloat16().to(dev)[:, :n]
    (temps, keys, _), (t_t, t_k, _) = rows_inputs(m, dev)
    top_ks, top_ps = [20] * m, [0.8] * m
    t_ks, t_ps = torch.tensor(top_ks, dtype=torch.int32).to(dev), torch.tensor(top_ps).to(dev)
    st = advance_state(m, dev)
    call = lambda: ops.sample_advance(logits, *(st[f] for f in ADVANCE_FIELDS), t_t, t_k, seed, top_k=t_ks, top_p=t_ps)
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
    ref = np.stack([ref_tokens(logits, temps, gumbel64(seed, keys, [s] * m, n), top_ks, top_ps)[0] for s in range(3)])
    assert np.array_equal(st["tokens_log"][:3].cpu().numpy(), ref) and torch.equal(eager0, st["tokens_log"][0])
    assert (st["row_steps"] == 3).all() and (ref[0] != ref[1]).any()


def test_engine_generates_truncated_tokens():
    from nanovllm_hip.engine.llm_engine import LLMEngine
    from nanovllm_hip.engine.sequence import Sequence
    from nanovllm_hip.models import qwen
    cfg = qwen.model_config("Qwen2-0.5B", num_hidden_layers=2, vocab_size=2048)
    eng = LLMEngine(cfg, num_kvcache_blocks=12, seed=4)
    gen = torch.Generator().manual_seed(11)
    prompts = [torch.randint(0, 2048, (n,), generator=gen).tolist() for n in (300, 17, 256, 1)]
    temps, new = [0.0, 0.8, 0.0, 1.2], 17

    def run(temperature, graph=True, **trunc):
        Sequence.counter = itertools.count()                     # the noise key of a request is its sequence id
        if graph:
            return eng.generate(prompts, new, temperature=temperature, **trunc)
        seqs = [Sequence(p, max_tokens=new, temperature=t, **trunc) for p, t in zip(prompts, temperature)]
        eng.prefill(seqs, reserve_tokens=new)
        sess = eng.runner.decode_session(seqs, new - 1, use_graph=False)
        sess.step(new - 1)
        sess.finish()
        for s in seqs:
            eng.block_manager.deallocate(s)
        return [s.completion_token_ids for s in seqs]

    greedy = run(0.0)
    a, a2, eager = run(temps, top_k=20, top_p=0.8), run(temps, top_k=20, top_p=0.8), run(temps, graph=False, top_k=20, top_p=0.8)
    assert all(len(r) == new for r in a) and a == a2 and a == eager
    assert a[0] == greedy[0] and a[2] == greedy[2]
    assert run(temps, top_k=1) == greedy
