"""The routing plan (csrc/plan.h) pinned on the CPU through the host-only query entry points nvh_plan_prefill / nvh_plan_decode.
Every expected value is a literal read off the rules as they stood before the plan existed (launch_short / launch_d / launch_chunked,
decode_chunks, ops.flash_attn_varlen_func); nothing is computed by asking the library twice.  cus = 256 (MI355X) is passed explicitly."""
import ctypes

import pytest

CUS = 256
BF16, F32 = 0, 1
AUTO, TILED, SHORT, F16V = 0, 1, 2, 3                    # NVH_PREFILL_*
NEVER, ALWAYS, PV_AUTO = 0, 1, 2                         # NVH_PV_* requests
EXACT, SCRATCH, IN_KERNEL, HANDED_IN = 0, 1, 2, 3        # NVH_PV_* forms
K_SHORT, K_TILED = 0, 1                                  # NVH_PLAN_*
E_SHAPE = -2


@pytest.fixture(scope="module")
def lib():
    from nanovllm_hip import _lib
    return _lib.load()


def prefill(lib, batch, max_q, max_k, kvh=2, hd=64, kernel=AUTO, short_waves=0, pv=PV_AUTO, out=BF16, paged=False, total_k=None):
    """-> (rc, (kernel, paged, q_subtiles, short_waves, pv_form, scratch_bytes))"""
    from nanovllm_hip import _lib
    p = _lib.PrefillPlan()
    rc = lib.nvh_plan_prefill(ctypes.byref(p), kernel, short_waves, pv, out, int(paged), batch, max_q, max_k,
                              batch * max_k if total_k is None else total_k, kvh, hd, CUS)
    return rc, (p.kernel, p.paged, p.q_subtiles, p.short_waves, p.pv_form, p.scratch_bytes)


def scratch(lib, batch, max_k, kvh=2, hd=64):
    return lib.nvh_prefill_pv16_scratch_bytes(batch * max_k, kvh, hd)


# rows (a) .. (i): (batch, max_q, max_k, hd, request kwargs, expected plan, expected nvh_prefill_pv16_uses_scratch)
ROWS_A_TO_I = {
    "a": ((64, 128, 128, 64), {}, (K_SHORT, 0, 1, 16, IN_KERNEL, 0), 0),
    "b": ((192, 128, 128, 64), {}, (K_SHORT, 0, 1, 8, IN_KERNEL, 0), 0),
    "c": ((63, 128, 128, 64), {}, (K_TILED, 0, 1, 0, EXACT, 0), 1),
    "d": ((64, 64, 64, 64), {}, (K_SHORT, 0, 1, 16, EXACT, 0), 0),
    "e": ((64, 64, 64, 64), {"pv": ALWAYS}, (K_SHORT, 0, 1, 16, EXACT, 0), 0),
    "f": ((64, 128, 128, 128), {"short_waves": 16}, (K_SHORT, 0, 1, 8, EXACT, 0), 0),
    "g": ((64, 128, 128, 128), {"pv": ALWAYS}, (K_SHORT, 0, 1, 8, EXACT, 0), 0),
    "h": ((4, 511, 511, 64), {}, (K_TILED, 0, 1, 0, EXACT, 0), 1),
    "i": ((4, 512, 512, 64), {}, (K_TILED, 0, 2, 0, SCRATCH, "scratch"), 1),
}


@pytest.mark.parametrize("row", sorted(ROWS_A_TO_I))
def test_prefill_rows_a_to_i(lib, row):
    (batch, mq, mk, hd), req, exp, uses = ROWS_A_TO_I[row]
    if exp[5] == "scratch":
        exp = exp[:5] + (scratch(lib, batch, mk, 2, hd),)
        assert exp[5] == 256 + batch * mk * 2 * hd * 2           # (flags of 32 groups fit the first 256 bytes)
    assert prefill(lib, batch, mq, mk, hd=hd, **req) == (0, exp)
    # the older query keeps its answer (it never looked at head_dim) and agrees with the plan of the ALWAYS request
    assert lib.nvh_prefill_pv16_uses_scratch(batch, mq, mk, 2, hd) == uses
    rc, always = prefill(lib, batch, mq, mk, hd=hd, pv=ALWAYS)
    assert rc == 0 and (always[4] == SCRATCH) == bool(uses) and (always[5] > 0) == bool(uses)


def test_prefill_rows_j_to_t(lib):
    # j: as (i) with f32 output: exact, one sub-tile
    assert prefill(lib, 4, 512, 512, out=F32) == (0, (K_TILED, 0, 1, 0, EXACT, 0))
    # k: hd 64, exact form: two sub-tiles from 2048 query rows on
    assert prefill(lib, 2, 2047, 2047, pv=NEVER) == (0, (K_TILED, 0, 1, 0, EXACT, 0))
    assert prefill(lib, 2, 2048, 2048, pv=NEVER) == (0, (K_TILED, 0, 2, 0, EXACT, 0))
    # l: fp16 via scratch, the sub-tile rule reads max_q (511 < 512), not max_k
    assert prefill(lib, 2, 511, 600, pv=ALWAYS) == (0, (K_TILED, 0, 1, 0, SCRATCH, scratch(lib, 2, 600)))
    # m: hd 128: two sub-tiles above 128 query rows, either form
    for pv, form in ((NEVER, EXACT), (ALWAYS, SCRATCH)):
        for mq, sub in ((128, 1), (129, 2)):
            rc, p = prefill(lib, 2, mq, mq, hd=128, pv=pv)
            assert rc == 0 and p[:5] == (K_TILED, 0, sub, 0, form)
    # n, o: paged
    assert prefill(lib, 2, 300, 600, paged=True) == (0, (K_TILED, 1, 1, 0, EXACT, 0))
    assert prefill(lib, 2, 300, 600, paged=True, pv=ALWAYS)[0] == E_SHAPE
    assert b"block table" in lib.nvh_last_error()
    # p, q: the SHORT selector takes the kernel whatever the batch, and refuses more than 128 keys
    assert prefill(lib, 1, 128, 128, kernel=SHORT) == (0, (K_SHORT, 0, 1, 16, EXACT, 0))
    assert prefill(lib, 1, 129, 129, kernel=SHORT)[0] == E_SHAPE
    # r, s: the fp16-V measurement selector: never the short kernel, the exact form's sub-tile threshold
    assert prefill(lib, 64, 128, 128, kernel=F16V) == (0, (K_TILED, 0, 1, 0, HANDED_IN, 0))
    assert prefill(lib, 2, 2047, 2047, kernel=F16V) == (0, (K_TILED, 0, 1, 0, HANDED_IN, 0))
    assert prefill(lib, 2, 2048, 2048, kernel=F16V) == (0, (K_TILED, 0, 2, 0, HANDED_IN, 0))
    # t: more query rows than keys: never the short kernel
    assert prefill(lib, 64, 128, 100) == (0, (K_TILED, 0, 1, 0, EXACT, 0))
    # the TILED selector refuses the short kernel on its best shape; short_waves = 8 on the 16-wave shape
    assert prefill(lib, 64, 128, 128, kernel=TILED) == (0, (K_TILED, 0, 1, 0, EXACT, 0))
    assert prefill(lib, 64, 128, 128, short_waves=8) == (0, (K_SHORT, 0, 1, 8, EXACT, 0))


def test_pv16_min_keys_is_the_plans_boundary(lib):
    from nanovllm_hip import ops
    assert ops.PV16_MIN_KEYS == 512
    forms = [prefill(lib, 4, n, n)[1][4] for n in (129, 300, 511, 512, 513, 4096)]
    assert forms == [EXACT, EXACT, EXACT, SCRATCH, SCRATCH, SCRATCH]


# ---------------------------------------------------------------------------------------------------------------- decode
CHUNKED, SPLIT_MFMA, SPLIT_VALU, P128, P256, P64 = 0, 1, 2, 3, 4, 5
SPLIT = {64: 256, 128: 128}                              # tokens per full pass: MGeo<D>::SPLIT of the kernels (4 waves x 4096 / D)


def decode(lib, hd, batch, max_blocks=4, variant=CHUNKED, waves=0, chunks=0, h=None, kvh=None):
    """-> (rc, (impl, waves, pass_tokens, chunks, num_splits)); block 256; 14 / 2 heads at hd 64, 28 / 4 at hd 128"""
    from nanovllm_hip import _lib
    h = h or (14 if hd == 64 else 28)
    kvh = kvh or (2 if hd == 64 else 4)
    p = _lib.DecodePlan()
    rc = lib.nvh_plan_decode(ctypes.byref(p), variant, waves, chunks, batch, h, kvh, hd, 256, max_blocks, CUS)
    return rc, (p.impl, p.waves, p.pass_tokens, p.chunks, p.num_splits)


def test_decode_rows(lib):
    ns = lambda hd, max_blocks: max_blocks * 256 // SPLIT[hd]
    assert decode(lib, 64, 32) == (0, (CHUNKED, 8, 128, 4, ns(64, 4)))                       # a
    assert decode(lib, 64, 64) == (0, (CHUNKED, 8, 256, 2, 4))                               # b
    assert decode(lib, 64, 24, 8) == (0, (CHUNKED, 8, 128, 5, 8))                            # c
    assert decode(lib, 64, 20, 8) == (0, (CHUNKED, 8, 256, 6, 8))                            # d
    assert decode(lib, 64, 32, waves=4) == (0, (CHUNKED, 4, 256, 4, 4))                      # e
    assert decode(lib, 64, 32, variant=P128, waves=4) == (0, (CHUNKED, 8, 128, 4, 4))        # f: the 128-token form has 8 waves only
    assert decode(lib, 64, 32, variant=P64) == (0, (CHUNKED, 8, 256, 4, 4))                  # g: a pass size hd 64 does not have forces 256
    assert decode(lib, 64, 513, h=7, kvh=1) == (0, (CHUNKED, 8, 256, 1, 4))                  # h: 513 pairs > 512 tickets (one kv head: 513 is odd)
    assert decode(lib, 64, 513, h=7, kvh=1, chunks=4)[1][3] == 1
    assert decode(lib, 64, 256, h=14, kvh=2)[1][3] == 1                                      # 512 pairs: tickets suffice, but 256 CUs / 512 pairs
    assert decode(lib, 64, 32, chunks=16) == (0, (CHUNKED, 8, 128, 4, 4))                    # i: clamped to num_splits
    assert decode(lib, 64, 32, 16, chunks=16) == (0, (CHUNKED, 8, 256, 16, 16))
    assert decode(lib, 128, 8) == (0, (CHUNKED, 4, 64, 8, ns(128, 4)))                       # j
    assert decode(lib, 128, 8, waves=8) == (0, (CHUNKED, 8, 128, 8, 8))                      # k
    assert decode(lib, 128, 8, waves=4) == (0, (CHUNKED, 4, 128, 8, 8))
    assert decode(lib, 128, 8, variant=P128) == (0, (CHUNKED, 4, 128, 8, 8))                 # l
    assert decode(lib, 128, 8, variant=P256) == (0, (CHUNKED, 4, 128, 8, 8))
    assert decode(lib, 128, 8, variant=P64, waves=8) == (0, (CHUNKED, 4, 64, 8, 8))
    assert decode(lib, 128, 4) == (0, (CHUNKED, 4, 64, 8, 8))                                # m: min(16, num_splits = 8)
    assert decode(lib, 128, 4, 8) == (0, (CHUNKED, 4, 128, 16, 16))                          # m, n: 16 chunks: past the half-pass rule (<= 8)
    assert decode(lib, 128, 4, 5) == (0, (CHUNKED, 4, 128, 10, 10))                          # n: 10 chunks
    assert decode(lib, 64, 32, variant=SPLIT_VALU, h=18, kvh=2)[0] == E_SHAPE                # o: group size 9
    assert decode(lib, 64, 32, variant=SPLIT_VALU) == (0, (SPLIT_VALU, 8, 256, 4, 4))
    assert decode(lib, 128, 8, variant=SPLIT_MFMA) == (0, (SPLIT_MFMA, 4, 128, 8, 8))
    # the CU count is an argument: half the chip, half the chunks
    from nanovllm_hip import _lib
    p = _lib.DecodePlan()
    assert lib.nvh_plan_decode(ctypes.byref(p), CHUNKED, 0, 0, 32, 14, 2, 64, 256, 4, 128) == 0 and (p.chunks, p.pass_tokens) == (2, 256)


def test_plan_queries_validate(lib):
    from nanovllm_hip import _lib
    p, d = _lib.PrefillPlan(), _lib.DecodePlan()
    assert lib.nvh_plan_prefill(None, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 64, CUS) == -5
    assert lib.nvh_plan_prefill(ctypes.byref(p), 4, 0, 0, 0, 0, 1, 1, 1, 1, 2, 64, CUS) == E_SHAPE
    assert lib.nvh_plan_prefill(ctypes.byref(p), 0, 0, 3, 0, 0, 1, 1, 1, 1, 2, 64, CUS) == E_SHAPE
    assert lib.nvh_plan_prefill(ctypes.byref(p), 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 96, CUS) == E_SHAPE
    assert lib.nvh_plan_prefill(ctypes.byref(p), 0, 0, 0, 7, 0, 1, 1, 1, 1, 2, 64, CUS) == -1
    assert lib.nvh_plan_decode(None, 0, 0, 0, 1, 14, 2, 64, 256, 4, CUS) == -5
    assert lib.nvh_plan_decode(ctypes.byref(d), 6, 0, 0, 1, 14, 2, 64, 256, 4, CUS) == E_SHAPE
    assert lib.nvh_plan_decode(ctypes.byref(d), 0, 5, 0, 1, 14, 2, 64, 256, 4, CUS) == E_SHAPE
    assert lib.nvh_plan_decode(ctypes.byref(d), 0, 0, 0, 1, 14, 2, 96, 256, 4, CUS) == E_SHAPE
