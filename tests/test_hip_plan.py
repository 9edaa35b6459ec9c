"""The plan is what runs: the default calls give bit-identical results to the variant entry points driven by the selectors the plan query
reports (nvh_plan_decode / nvh_plan_prefill with cus = 0, the current device's).  Routing itself is pinned on the CPU: test_plan_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from nanovllm_hip import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.mark.parametrize("B,H,KVH,D", [(32, 14, 2, 64), (64, 14, 2, 64), (8, 28, 4, 128)])     # test_plan_cpu.py decode rows (a), (b), (j)
def test_default_decode_is_the_planned_variant(ops, B, H, KVH, D):
    from nanovllm_hip import _lib
    bs, width = 256, 4
    rng = np.random.default_rng(B + D)
    ctxs = rng.integers(400, 801, size=B).astype(np.int32)                  # ragged around 600 tokens
    ctxs[B // 2] = 0                                                        # a padding row
    need = (ctxs + bs - 1) // bs
    nb = int(need.sum()) + 2
    bt = np.full((B, width), -1, np.int32)
    ids = iter(rng.permutation(nb).tolist())
    for b in range(B):
        for j in range(need[b]):
            bt[b, j] = next(ids)
    gen = torch.Generator().manual_seed(B + D)
    kc = torch.randn(nb, bs, KVH, D, generator=gen).bfloat16().cuda()
    vc = torch.randn(nb, bs, KVH, D, generator=gen).bfloat16().cuda()
    q = torch.randn(B, H, D, generator=gen).bfloat16().cuda()
    cl, btd = torch.from_numpy(ctxs).cuda(), torch.from_numpy(bt).cuda()

    plan = _lib.DecodePlan()
    assert _lib.load().nvh_plan_decode(ctypes.byref(plan), 0, 0, 0, B, H, KVH, D, bs, width, 0) == 0
    assert plan.impl == 0 and plan.pass_tokens in (64, 128, 256)
    kw = dict(variant=f"chunked_p{plan.pass_tokens}", waves=plan.waves, chunks=plan.chunks)
    for dt in (torch.bfloat16, torch.float32):
        got = ops.flash_attn_with_kvcache(q, kc, vc, cl, btd, out_dtype=dt)
        ref = ops.flash_attn_with_kvcache(q, kc, vc, cl, btd, out_dtype=dt, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), f"default decode != {kw} ({dt})"
        assert not got[B // 2].any()
    # the selectors do reach the kernel: the other pass size sums in another order, so its fp32 result differs somewhere (not vacuous above)
    other = {64: {128: 256, 256: 128}, 128: {64: 128, 128: 64}}[D][plan.pass_tokens]
    alt = ops.flash_attn_with_kvcache(q, kc, vc, cl, btd, out_dtype=torch.float32, variant=f"chunked_p{other}", chunks=plan.chunks)
    torch.cuda.synchronize()
    assert not torch.equal(got, alt)


def _prefill_case(n_seq, seq, H=14, KVH=2, D=64, seed=0):
    gen = torch.Generator().manual_seed(seed + n_seq)
    T = n_seq * seq
    q = torch.randn(T, H, D, generator=gen).bfloat16().cuda()
    k = torch.randn(T, KVH, D, generator=gen).bfloat16().cuda()
    v = torch.randn(T, KVH, D, generator=gen).bfloat16().cuda()
    cu = torch.arange(0, T + 1, seq, dtype=torch.int32).cuda()
    return q, k, v, cu


def _prefill_plan(n_seq, seq, pv, out_code, KVH=2, D=64):
    from nanovllm_hip import _lib
    plan = _lib.PrefillPlan()
    assert _lib.load().nvh_plan_prefill(ctypes.byref(plan), 0, 0, pv, out_code, 0, n_seq, seq, seq, n_seq * seq, KVH, D, 0) == 0
    return plan


def test_default_prefill_is_the_planned_kernel(ops):
    from nanovllm_hip import _lib
    # f32 output: the P V form is exact on both sides.  64 sequences of 128 tokens: the short-sequence kernel, with the planned waves
    q, k, v, cu = _prefill_case(64, 128)
    plan = _prefill_plan(64, 128, _lib.PV_AUTO, _lib.NVH_F32)
    assert plan.kernel == _lib.PLAN_SHORT and plan.pv_form == _lib.PV_EXACT and plan.short_waves in (8, 16)
    got = ops.flash_attn_varlen_func(q, k, v, 128, cu, 128, cu, out_dtype=torch.float32)
    ref = ops.flash_attn_varlen_func(q, k, v, 128, cu, 128, cu, out_dtype=torch.float32, kernel="short", short_waves=plan.short_waves)
    assert torch.equal(got, ref)
    # 63 sequences: the tiled kernel
    q, k, v, cu = _prefill_case(63, 128)
    plan = _prefill_plan(63, 128, _lib.PV_AUTO, _lib.NVH_F32)
    assert plan.kernel == _lib.PLAN_TILED and plan.pv_form == _lib.PV_EXACT
    got = ops.flash_attn_varlen_func(q, k, v, 128, cu, 128, cu, out_dtype=torch.float32)
    ref = ops.flash_attn_varlen_func(q, k, v, 128, cu, 128, cu, out_dtype=torch.float32, kernel="tiled")
    assert torch.equal(got, ref)
    # bf16 output, 4 sequences of 512 tokens: the default is the fp16 P V form through scratch
    q, k, v, cu = _prefill_case(4, 512)
    plan = _prefill_plan(4, 512, _lib.PV_AUTO, _lib.NVH_BF16)
    assert plan.pv_form == _lib.PV_F16_SCRATCH and plan.scratch_bytes > 0 and plan.q_subtiles == 2
    got = ops.flash_attn_varlen_func(q, k, v, 512, cu, 512, cu)
    ref = ops.flash_attn_varlen_func(q, k, v, 512, cu, 512, cu, pv_fp16=True)
    exact = ops.flash_attn_varlen_func(q, k, v, 512, cu, 512, cu, pv_fp16=False)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert not torch.equal(got, exact)                                      # (the two forms do differ: the comparison above is not vacuous)
