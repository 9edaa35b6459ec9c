#!/usr/bin/env python3
"""One attention call per launchable row of the routing table (tests/test_plan_cpu.py), at small sizes, to be run under a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/dispatch_trace.py
    python3 tools/dispatch_trace.py --summarize OUT/*/*kernel_trace.csv > listing.txt

The listing has one line per dispatch of a library kernel: row label, kernel name with its template arguments, grid, workgroup.  Two
builds route alike when their listings are identical.  Only the public Python signatures are used, so the same file runs on either build.
A tool, not a test: nothing is checked here.  Rows (o), (q) and decode (o) are refusals, and row (t) (more query rows than keys) is a
shape no GPU test of the suite runs: their routing is pinned on the CPU only."""
import csv
import sys


def rows():
    """-> [(label, callable)]"""
    import numpy as np
    import torch
    from nanovllm_hip import ops

    gen = torch.Generator().manual_seed(0)

    def prefill(n_seq, mq, mk, H=14, KVH=2, D=64, v_f16=False, **kw):
        q = torch.randn(n_seq * mq, H, D, generator=gen).bfloat16().cuda()
        k = torch.randn(n_seq * mk, KVH, D, generator=gen).bfloat16().cuda()
        v = torch.randn(n_seq * mk, KVH, D, generator=gen).bfloat16().cuda()
        if v_f16:
            v = v.half()
        cq = torch.arange(0, n_seq * mq + 1, mq, dtype=torch.int32).cuda()
        ck = torch.arange(0, n_seq * mk + 1, mk, dtype=torch.int32).cuda()
        return lambda: ops.flash_attn_varlen_func(q, k, v, mq, cq, mk, ck, **kw)

    def paged_prefill(n_seq, mq, mk, H=14, KVH=2, D=64, bs=256, **kw):
        per = (mk + bs - 1) // bs
        kc = torch.randn(n_seq * per, bs, KVH, D, generator=gen).bfloat16().cuda()
        vc = torch.randn(n_seq * per, bs, KVH, D, generator=gen).bfloat16().cuda()
        q = torch.randn(n_seq * mq, H, D, generator=gen).bfloat16().cuda()
        bt = torch.arange(n_seq * per, dtype=torch.int32).view(n_seq, per).cuda()
        cq = torch.arange(0, n_seq * mq + 1, mq, dtype=torch.int32).cuda()
        ck = torch.arange(0, n_seq * mk + 1, mk, dtype=torch.int32).cuda()
        return lambda: ops.flash_attn_varlen_func(q, kc, vc, mq, cq, mk, ck, block_table=bt, **kw)

    def decode(B, D, max_blocks=4, H=None, KVH=None, bs=256, **kw):
        H, KVH = H or (14 if D == 64 else 28), KVH or (2 if D == 64 else 4)
        nb = 8                                                   # every sequence reads the same few blocks: the trace is about the grid only
        kc = torch.randn(nb, bs, KVH, D, generator=gen).bfloat16().cuda()
        vc = torch.randn(nb, bs, KVH, D, generator=gen).bfloat16().cuda()
        q = torch.randn(B, H, D, generator=gen).bfloat16().cuda()
        bt = torch.from_numpy((np.arange(B * max_blocks, dtype=np.int32) % nb).reshape(B, max_blocks)).cuda()
        cl = torch.full((B,), 300, dtype=torch.int32).cuda()
        return lambda: ops.flash_attn_with_kvcache(q, kc, vc, cl, bt, **kw)

    f32 = torch.float32
    return [
        ("prefill a", prefill(64, 128, 128)),
        ("prefill b", prefill(192, 128, 128)),
        ("prefill c", prefill(63, 128, 128)),
        ("prefill d", prefill(64, 64, 64)),
        ("prefill e", prefill(64, 64, 64, pv_fp16=True)),
        ("prefill f", prefill(64, 128, 128, H=4, D=128, short_waves=16)),
        ("prefill g", prefill(64, 128, 128, H=4, D=128, pv_fp16=True)),
        ("prefill h", prefill(4, 511, 511)),
        ("prefill i", prefill(4, 512, 512)),
        ("prefill j", prefill(4, 512, 512, out_dtype=f32)),
        ("prefill k 2047", prefill(1, 2047, 2047, H=2, KVH=1, pv_fp16=False)),
        ("prefill k 2048", prefill(1, 2048, 2048, H=2, KVH=1, pv_fp16=False)),
        ("prefill l", prefill(2, 511, 600, pv_fp16=True)),
        ("prefill m 128 exact", prefill(2, 128, 128, H=4, D=128, pv_fp16=False)),
        ("prefill m 129 exact", prefill(2, 129, 129, H=4, D=128, pv_fp16=False)),
        ("prefill m 128 fp16", prefill(2, 128, 128, H=4, D=128, pv_fp16=True)),
        ("prefill m 129 fp16", prefill(2, 129, 129, H=4, D=128, pv_fp16=True)),
        ("prefill n", paged_prefill(2, 300, 600)),
        ("prefill u auto", paged_prefill(1, 64, 4096, key_splits="auto")),        # split-key form: 8 workgroups per q-tile by the rule
        ("prefill u forced", paged_prefill(2, 300, 600, key_splits=3)),
        ("prefill u one", paged_prefill(16, 512, 1024, key_splits="auto")),       # the unsplit grid fills the chip: row n's kernel
        ("prefill p", prefill(1, 128, 128, kernel="short")),
        ("prefill r", prefill(64, 128, 128, kernel="tiled_f16v", v_f16=True)),
        ("prefill s 2047", prefill(1, 2047, 2047, H=2, KVH=1, kernel="tiled_f16v", v_f16=True)),
        ("prefill s 2048", prefill(1, 2048, 2048, H=2, KVH=1, kernel="tiled_f16v", v_f16=True)),
        ("decode a", decode(32, 64)),
        ("decode b", decode(64, 64)),
        ("decode c", decode(24, 64, 8)),
        ("decode d", decode(20, 64, 8)),
        ("decode e", decode(32, 64, waves=4)),
        ("decode f", decode(32, 64, variant="chunked_p128", waves=4)),
        ("decode g", decode(32, 64, variant="chunked_p64")),
        ("decode h", decode(513, 64, H=7, KVH=1)),
        ("decode i", decode(32, 64, chunks=16)),
        ("decode j", decode(8, 128)),
        ("decode k", decode(8, 128, waves=8)),
        ("decode l p128", decode(8, 128, variant="chunked_p128")),
        ("decode l p256", decode(8, 128, variant="chunked_p256")),
        ("decode m", decode(4, 128)),
        ("decode n", decode(4, 128, 8)),
        ("decode split_mfma", decode(32, 64, variant="split_mfma")),
        ("decode split_valu", decode(32, 64, variant="split_valu")),
    ]


def run():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    table = rows()
    torch.cuda.synchronize()
    sep = torch.zeros(64, device="cuda")
    for i, (label, call) in enumerate(table):
        sep.sigmoid_()                                           # a dispatch no row makes, in front of every row: the row boundary in the trace
        call()
        torch.cuda.synchronize()
    sep.sigmoid_()
    torch.cuda.synchronize()
    print(f"[dispatch_trace] {len(table)} rows launched")


def summarize(path):
    labels = [label for label, _ in _labels()]
    recs = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))

    def dims(r, what):
        if f"{what}_X" in r:
            return "x".join(r[f"{what}_{a}"] for a in "XYZ")
        return r[what]
    bounds = [i for i, r in enumerate(recs) if "sigmoid" in r["Kernel_Name"].lower()]
    assert len(bounds) == len(labels) + 1, f"{len(bounds)} separator dispatches for {len(labels)} rows"
    for n, label in enumerate(labels):
        for r in recs[bounds[n] + 1:bounds[n + 1]]:
            if "nvh::" in r["Kernel_Name"]:
                print(f"{label:22s} {r['Kernel_Name']}  grid {dims(r, 'Grid_Size')}  workgroup {dims(r, 'Workgroup_Size')}")


def _labels():
    """Row labels without touching a GPU (the summary runs anywhere): the literals of rows()."""
    import ast
    import inspect
    src = inspect.getsource(rows)
    tree = ast.parse(src)
    ret = [n for n in ast.walk(tree) if isinstance(n, ast.Return) and isinstance(n.value, ast.List)][-1]
    return [(e.elts[0].value, None) for e in ret.value.elts]


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        import os
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path[:0] = [root, os.path.join(root, "nano-vllm-learn_amd")]
        run()
