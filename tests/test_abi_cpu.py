"""CPU checks of the drop-in boundary: the C-ABI library loads, exports every symbol include/nvh_attn.h
declares, validates arguments without touching a GPU, and the host-side mirror keeps the reference's
interface (names, constructor, attributes, Context fields).  No compute calls here."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from nanovllm_hip import _lib
    return _lib.load()


def test_header_symbols_all_exported(lib):
    from nanovllm_hip import _lib
    header = open(os.path.join(ROOT, "include", "nvh_attn.h")).read()
    declared = set(re.findall(r"\b(nvh_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.EXPORTS), f"binding/header mismatch: {declared ^ set(_lib.EXPORTS)}"
    for name in declared:
        assert hasattr(lib, name), f"libnvh_attn.so does not export {name}"


def test_version_matches_header(lib):
    header = open(os.path.join(ROOT, "include", "nvh_attn.h")).read()
    assert lib.nvh_version() == int(re.search(r"#define NVH_VERSION (\d+)", header).group(1))


def test_workspace_is_pure_function_of_static_shapes(lib):
    a = lib.nvh_paged_decode_workspace(32, 14, 64, 16, 256)
    assert a == lib.nvh_paged_decode_workspace(32, 14, 64, 16, 256) and a > 0
    hdr = 65536 + 8192                                                       # fixed header (tickets + the fused launch's counters), then the partial records
    assert lib.nvh_paged_decode_workspace(64, 14, 64, 16, 256) - hdr == 2 * (a - hdr)
    assert lib.nvh_paged_decode_workspace(32, 14, 96, 16, 256) == 0          # unsupported head_dim
    # partial = (D + 2) floats per (row, head, split)
    assert (a - hdr) % ((64 + 2) * 4 * 32 * 14) == 0 and (a - hdr) // ((64 + 2) * 4 * 32 * 14) == 2 * 16


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p = (p + 15) & ~15
    # null pointers
    assert lib.nvh_store_kvcache(None, None, None, None, None, 4, 2, 64, 128, 128, 0, None) == -5
    assert b"null" in lib.nvh_last_error()
    # zero work is a no-op that needs no pointers
    assert lib.nvh_store_kvcache(None, None, None, None, None, 0, 2, 64, 128, 128, 0, None) == 0
    assert lib.nvh_paged_decode(None, None, None, None, None, None, 0, 14, 2, 64, 256, 4, 896, 4, 0.125, 0, 0, None, 0, None) == 0
    # dtype / shape / stride / alignment / workspace checks fire before any launch
    assert lib.nvh_store_kvcache(p, p, p, p, p, 4, 2, 64, 128, 128, 7, None) == -1
    assert lib.nvh_store_kvcache(p, p, p, p, p, 4, 2, 64, 100, 128, 0, None) == -3
    assert lib.nvh_store_kvcache(p + 2, p, p, p, p, 4, 2, 64, 128, 128, 0, None) == -6
    assert lib.nvh_paged_decode(p, p, p, p, p, p, 1, 14, 2, 96, 256, 4, 1344, 4, 0.1, 0, 0, p, 1 << 20, None) == -2
    assert lib.nvh_paged_decode(p, p, p, p, p, p, 1, 14, 3, 64, 256, 4, 896, 4, 0.1, 0, 0, p, 1 << 20, None) == -2
    assert lib.nvh_paged_decode(p, p, p, p, p, p, 1, 14, 2, 64, 100, 4, 896, 4, 0.1, 0, 0, p, 1 << 20, None) == -2
    assert lib.nvh_paged_decode(p, p, p, p, p, p, 1, 14, 2, 64, 256, 4, 896, 4, 0.1, 0, 0, p, 16, None) == -4
    assert b"workspace" in lib.nvh_last_error()
    assert lib.nvh_prefill_varlen(p, p, p, p, p, p, None, 2, 16, 16, 14, 2, 64, 0, 0, 890, 128, 128, 0, 0.1, 0, 0, None) == -3
    # arg-max + advance + next step's embedding lookup: argument errors before any launch
    adv = (p, p, 8, 64, 4, p, p, p, p, p, 4, 256, p, 4, p)
    assert lib.nvh_greedy_advance_candidates_embed(*adv, None, 1000, 896, p, 896, p, 0, None) == -5          # no embedding table
    assert lib.nvh_greedy_advance_candidates_embed(*adv, p, 1000, 896, None, 896, p, 0, None) == -5          # no output rows
    assert lib.nvh_greedy_advance_candidates_embed(*adv, p, 1000, 900, p, 900, None, 0, None) == -2          # hidden % 32
    assert lib.nvh_greedy_advance_candidates_embed(*adv, p, 1000, 896, p, 800, None, 0, None) == -2          # row stride < hidden
    assert lib.nvh_greedy_advance_candidates_embed(*adv, p, 0, 896, p, 896, None, 0, None) == -2             # vocab
    assert lib.nvh_greedy_advance_candidates_embed(*adv, p + 2, 1000, 896, p, 896, None, 0, None) == -6
    assert lib.nvh_greedy_advance_candidates_embed(*adv, p, 1000, 896, p, 896, None, 3, None) == -1
    assert lib.nvh_greedy_advance_candidates_embed(p, p, 8, 64, 0, p, p, p, p, p, 4, 256, p, 4, p, None, 0, 0, None, 0, None, 0, None) == 0   # zero rows
    # the variant entry points validate their selectors
    dec = (p, p, p, p, p, p, 1, 14, 2, 64, 256, 4, 896, 4, 0.1, 0, 0, p, 1 << 20, None)
    assert lib.nvh_paged_decode_variant(6, 0, 0, *dec) == -2 and lib.nvh_paged_decode_variant(0, 5, 0, *dec) == -2
    assert lib.nvh_paged_decode_variant(2, 0, 0, p, p, p, p, p, p, 1, 16, 1, 64, 256, 4, 1024, 4, 0.1, 0, 0, p, 1 << 20, None) == -2   # VALU form: G <= 8
    pre = (p, p, p, p, p, p, None, 2, 16, 16, 14, 2, 64, 0, 0, 896, 128, 128, 0, 0.1, 0, 0, None)
    assert lib.nvh_prefill_varlen_variant(4, 0, *pre) == -2 and lib.nvh_prefill_varlen_variant(2, 4, *pre) == -2
    paged = (p, p, p, p, p, p, p, 2, 16, 16, 14, 2, 64, 256, 4, 896, 128, 128, 4, 0.1, 0, 0, None)
    assert lib.nvh_prefill_varlen_variant(3, 0, *paged) == -2                       # the fp16-V measurement variant never reads a paged cache
    # the fused front of a decode layer and the fp16 row conversion: argument errors before any launch
    assert lib.nvh_qkv_rope_attend(None, p, None, p, p, 256, 4, 4, 0.1, 0, p, 1 << 20, None) == -5
    assert lib.nvh_qkv_rope_attend_status(None, None) == -5
    assert lib.nvh_bf16_rows_to_f16(p, p, 4, 100, 128, 128, None) == -2 and lib.nvh_bf16_rows_to_f16(p, p, 4, 128, 100, 128, None) == -3
    assert lib.nvh_bf16_rows_to_f16(None, None, 0, 128, 128, 128, None) == 0
    # the streaming linear layer takes K in whole 128-byte weight lines (k % 64), and says so under its own name
    assert lib.nvh_linear_small_m(p, p, p, None, 4, 16, 96, 0, 96, 16, 0, None) == _E_SHAPE
    assert b"linear_small_m:" in lib.nvh_last_error() and b"%64" in lib.nvh_last_error()
    assert lib.nvh_linear_small_m(p, p, p, None, 4, 16, 32, 0, 32, 16, 0, None) == _E_SHAPE
    # prefill with P V on the fp16 pipe: scratch size is a pure function of the shapes; argument errors before any stream operation
    assert lib.nvh_prefill_pv16_scratch_bytes(100, 2, 64) == 256 + 100 * 2 * 64 * 2 and lib.nvh_prefill_pv16_scratch_bytes(0, 2, 64) == 0
    pv = (p, p, p, p, p, p, 2, 1024, 1024, 2048, 14, 2, 64, 896, 128, 128, 0.125, 0, 0)
    assert lib.nvh_prefill_varlen_pv16(*pv, None, 0, None) == -5                      # no scratch
    assert lib.nvh_prefill_pv16_uses_scratch(2, 1024, 1024, 2, 64) == 1 and lib.nvh_prefill_pv16_uses_scratch(128, 128, 128, 2, 64) == 0
    assert lib.nvh_prefill_pv16_uses_scratch(16, 128, 128, 2, 64) == 1               # few sequences: the tiled kernel
    assert lib.nvh_prefill_varlen_pv16(*pv, p, 4096, None) == -4                      # scratch too small
    assert b"scratch" in lib.nvh_last_error()
    assert lib.nvh_prefill_varlen_pv16(*pv[:9], 0, *pv[10:], p, 1 << 20, None) == -4  # total_k missing
    assert lib.nvh_prefill_varlen_pv16(p, p, p, p, p, p, 0, 0, 0, 0, 14, 2, 64, 896, 128, 128, 0.125, 0, 0, None, 0, None) == 0   # empty batch


# ---- the eight token-choice entry points: one argument table, defects by argument name
_E_DTYPE, _E_SHAPE, _E_STRIDE, _E_NULL, _E_ALIGN = -1, -2, -3, -5, -6
_ADVANCE = ["input_ids", "positions", "context_lens", "slot_mapping", "block_tables", "bt_stride", "block_size", "tokens_log", "log_stride", "row_steps"]
_LOGITS = ["logits", "n_rows", "n", "stride"]
_CANDS = ["cand_val", "cand_idx", "groups", "cand_stride", "n_rows"]
_EMBED = ["embed_weight", "vocab", "hidden", "hidden_out", "hidden_stride", "hidden_packed"]
TOKEN_CHOICE_ARGS = {
    "argmax_rows": ["out", *_LOGITS, "dtype", "stream"],
    "greedy_advance": [*_LOGITS, *_ADVANCE, "dtype", "stream"],
    "sample_rows": ["out", *_LOGITS, "temperatures", "row_keys", "steps", "seed", "dtype", "stream"],
    "sample_advance": [*_LOGITS, *_ADVANCE, "temperatures", "row_keys", "seed", "dtype", "stream"],
    "sample_rows_truncated": ["out", *_LOGITS, "temperatures", "row_keys", "steps", "top_ks", "top_ps", "seed", "dtype", "stream"],
    "sample_advance_truncated": [*_LOGITS, *_ADVANCE, "temperatures", "row_keys", "top_ks", "top_ps", "seed", "dtype", "stream"],
    "greedy_advance_candidates": [*_CANDS, *_ADVANCE, "stream"],
    "greedy_advance_candidates_embed": [*_CANDS, *_ADVANCE, *_EMBED, "dtype", "stream"],
}
_SCALARS = dict(n_rows=4, n=64, stride=64, bt_stride=4, block_size=256, log_stride=4, seed=11, dtype=0, stream=None, groups=8, cand_stride=64,
                vocab=1000, hidden=896, hidden_stride=896)
_POINTERS = ("out", "logits", "temperatures", "row_keys", "steps", "top_ks", "top_ps", "cand_val", "cand_idx", "embed_weight", "hidden_out", "hidden_packed",
             "input_ids", "positions", "context_lens", "slot_mapping", "block_tables", "tokens_log", "row_steps")
# one defect per call: (argument, bad value or "null" / "misaligned", code); a row applies to every entry point that has the argument
ONE_DEFECT = [("dtype", 7, _E_DTYPE)] + \
             [(p, "null", _E_NULL) for p in _POINTERS if p != "hidden_packed"] + \
             [("n", 0, _E_SHAPE), ("n", -3, _E_SHAPE), ("block_size", 0, _E_SHAPE), ("block_size", -1, _E_SHAPE), ("log_stride", 3, _E_SHAPE),
              ("stride", 68, _E_STRIDE), ("stride", 56, _E_STRIDE), ("logits", "misaligned", _E_ALIGN)]
# two defects per call: dtype, null pointers, shape, stride, alignment, in that order, at every entry point
# (the last column: the code before the entry points shared one path, where it was another)
TWO_DEFECTS = [
    ("greedy_advance", {"positions": "null", "n": 0}, _E_NULL, None),
    ("sample_rows", {"n": 0, "stride": 68}, _E_SHAPE, None),
    ("argmax_rows", {"stride": 68, "logits": "misaligned"}, _E_STRIDE, None),
    ("sample_rows_truncated", {"top_ps": "null", "logits": "misaligned"}, _E_NULL, None),
    ("sample_advance", {"dtype": 7, "input_ids": "null"}, _E_DTYPE, _E_NULL),
    ("sample_advance", {"block_size": 0, "logits": "null"}, _E_NULL, _E_SHAPE),
    ("sample_advance_truncated", {"dtype": 7, "log_stride": 3}, _E_DTYPE, _E_SHAPE),
    ("greedy_advance_candidates_embed", {"groups": 0, "hidden_out": "null"}, _E_NULL, _E_SHAPE),
]


def _token_choice_call(lib, entry, defects):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    vals = {**_SCALARS, **{name: p for name in _POINTERS}}
    for name, bad in defects.items():
        vals[name] = {"null": None, "misaligned": p + 2}.get(bad, bad) if isinstance(bad, str) else bad
    rc = getattr(lib, "nvh_" + entry)(*[vals[a] for a in TOKEN_CHOICE_ARGS[entry]])
    return rc, lib.nvh_last_error().decode()


def _error_label(entry):
    return "greedy_advance_candidates" if entry == "greedy_advance_candidates_embed" else entry   # the two share their checks' messages


@pytest.mark.parametrize("entry", list(TOKEN_CHOICE_ARGS))
def test_token_choice_entry_points_report_one_defect(lib, entry):
    args = TOKEN_CHOICE_ARGS[entry]
    assert set(args) <= set(_SCALARS) | set(_POINTERS)
    rows = [(a, bad, code) for a, bad, code in ONE_DEFECT if a in args]
    assert {code for _, _, code in rows} >= ({_E_NULL, _E_SHAPE} if "logits" not in args else {_E_DTYPE, _E_NULL, _E_SHAPE, _E_STRIDE, _E_ALIGN})
    for arg, bad, code in rows:
        rc, msg = _token_choice_call(lib, entry, {arg: bad})
        assert rc == code, f"nvh_{entry}({arg}={bad}): {rc}, expected {code} ({msg})"
        assert _error_label(entry) in msg, f"nvh_{entry}({arg}={bad}): the message does not name the entry point: {msg}"
    assert _token_choice_call(lib, entry, {"n_rows": 0, "dtype": 7, "logits": "null", "input_ids": "null", "cand_val": "null"})[0] == 0   # zero rows: before any check


@pytest.mark.parametrize("entry,defects,code,code_before", TWO_DEFECTS)
def test_token_choice_entry_points_share_one_precedence(lib, entry, defects, code, code_before):
    rc, msg = _token_choice_call(lib, entry, defects)
    assert rc == code and _error_label(entry) in msg, f"nvh_{entry}({defects}): {rc}, expected {code} ({msg})"


def test_ops_refuse_cpu_tensors():
    """No CPU fallback: the product path must fail loudly off-GPU."""
    from nanovllm_hip import ops
    q = torch.zeros(1, 14, 64, dtype=torch.bfloat16)
    kc = torch.zeros(1, 256, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.flash_attn_with_kvcache(q, kc, kc, torch.ones(1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.store_kvcache(q[:, :2], q[:, :2], kc, kc, torch.zeros(1, dtype=torch.int32))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from nanovllm_hip import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libnvh_attn.so"))
    with pytest.raises(_lib.NvhLibraryError, match="no fallback"):
        _lib.load()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "nano-vllm-learn_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{f} imports the oracle"


def test_attention_module_mirrors_reference_interface():
    from nanovllm_hip import VALID_ATTN_BACKENDS, resolve_attention
    from nanovllm_hip.layers.attention_hip import Attention
    assert "hip" in VALID_ATTN_BACKENDS and not "hip".startswith("sdpa")
    for ref_name in ("flash", "sdpa", "sdpa.math", "triton"):             # config.py:6
        assert ref_name in VALID_ATTN_BACKENDS
    cls, kw = resolve_attention("hip", block_size=256)
    assert cls is Attention and kw == {"block_size": 256}
    with pytest.raises(ValueError):
        resolve_attention("nope")
    params = list(inspect.signature(Attention.__init__).parameters)
    assert params[1:5] == ["num_heads", "head_dim", "scale", "num_kv_heads"]     # attention.py:60-66, positional use qwen3.py:89-95
    m = Attention(14, 64, 0.125, 2, **kw)
    assert m.k_cache.numel() == 0 and m.v_cache.numel() == 0              # attention.py:72, duck-typed by model_runner.py:151
    assert list(inspect.signature(m.forward).parameters) == ["q", "k", "v"]


def test_context_fields_match_reference():
    from nanovllm_hip import Context, get_context, reset_context, set_context
    assert [f for f in Context.__dataclass_fields__] == ["is_prefill", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q",
                                                         "max_seqlen_k", "slot_mapping", "context_lens", "block_tables"]
    set_context(False, slot_mapping=1, context_lens=2, block_tables=3)
    c = get_context()
    assert (c.is_prefill, c.slot_mapping, c.context_lens, c.block_tables) == (False, 1, 2, 3)
    reset_context()
    assert get_context() == Context()


def test_pack_index_matches_the_torch_packer():
    """nvh_pack_index (host-callable) is the layout ops.pack_rows / unpack_rows produce."""
    import torch
    from nanovllm_hip import _lib, ops
    lib = _lib.load()
    m, c = 37, 96
    x = torch.arange(m * c, dtype=torch.float32).view(m, c).bfloat16()
    xp = ops.pack_rows(x)
    assert xp.numel() == 48 * c
    for row, col in [(0, 0), (1, 0), (0, 8), (15, 31), (16, 0), (36, 95), (17, 40)]:
        assert xp[lib.nvh_pack_index(row, col, c)] == x[row, col]
    assert torch.equal(ops.unpack_rows(xp, m, c), x)
    assert lib.nvh_linear_small_m_workspace(32, 896, 896, 2) == 0           # K <= 1024: one workgroup per tile, no hand-off
    assert lib.nvh_linear_small_m_workspace(32, 896, 4864, 2) >= 56 * 4 + 56 * 5 * (2 * 256 + 32) * 4
