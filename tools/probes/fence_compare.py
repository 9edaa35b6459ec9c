#!/usr/bin/env python3
"""Results of a second build of the library (argv[1]: the fenced cross-check build, or any other) against the shipped library, bit for bit, on
small cases that exercise each user of the cross-workgroup hand-off (csrc/handoff.h): the chunked decode kernel, the split-key prefill and the
split-K streaming GEMM (each library in its own process: a process binds one library)."""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD = r'''
import os, sys
import numpy as np, torch
ROOT = sys.argv[1]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nano-vllm-learn_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
from nanovllm_hip import ops
from test_hip_parity import _decode_case, dev_i32
outs = {}
for i, (B, H, KVH, D, lo, hi) in enumerate([(32, 14, 2, 64, 1025, 2048), (1, 7, 1, 64, 4096, 4096), (3, 14, 2, 128, 650, 1300), (5, 7, 1, 128, 1, 900), (8, 16, 8, 128, 200, 700), (64, 14, 2, 64, 2049, 4096)]):
    q, kc, vc, ctxs, bt = _decode_case(900 + i, B, H, KVH, D, lo, hi, 16, 0)
    for rep in range(3):
        o = ops.flash_attn_with_kvcache(q.cuda(), kc.cuda(), vc.cuda(), dev_i32(ctxs), dev_i32(bt), out_dtype=torch.float32)
    torch.cuda.synchronize()
    outs[f"decode{i}"] = o.cpu().numpy()
# split-key prefill, paged: one sequence, 16 query rows over a 1088-key cached prefix (17 key tiles of 64); the splits give one and two merge
# batches at head_dim 64 (4 records per batch), two and three at head_dim 128 (2 per batch)
SQ, SK, BS = 16, 1088, 256
for H, KVH, D, splits in [(4, 2, 64, (2, 5)), (2, 1, 128, (3, 5))]:
    gen = torch.Generator().manual_seed(H * 1000 + D)
    q = torch.randn(SQ, H, D, generator=gen).bfloat16().cuda()
    nb = (SK + BS - 1) // BS
    kc, vc = (torch.randn(nb, BS, KVH, D, generator=gen).bfloat16().cuda() for _ in range(2))
    bt = torch.randperm(nb, generator=gen).to(torch.int32).reshape(1, nb).cuda()
    cu_q, cu_k = dev_i32([0, SQ]), dev_i32([0, SK])
    for ks in splits:
        for rep in range(3):
            o = ops.flash_attn_varlen_func(q, kc, vc, SQ, cu_q, SK, cu_k, softmax_scale=D ** -0.5, block_table=bt, out_dtype=torch.float32, key_splits=ks)
        torch.cuda.synchronize()
        outs[f"prefill_splitk_{H}_{KVH}_{D}_splits{ks}"] = o.cpu().numpy()
# split-K streaming GEMM, residual_add epilogue: the smallest split-K shapes of tests/test_hip_layer_ops.py
for m, n, k in [(17, 64, 1088), (64, 512, 2048)]:
    gen = torch.Generator().manual_seed(n + k)
    x = torch.randn(m, k, generator=gen).bfloat16().cuda()
    w = (torch.randn(n, k, generator=gen) * 0.02).bfloat16().cuda()
    res0 = torch.randn(m, n, generator=gen).bfloat16().cuda()
    ws = torch.zeros(ops.linear_workspace_bytes(m, n, k, "residual_add"), dtype=torch.uint8, device="cuda")
    for rep in range(3):
        res = res0.clone()
        ops.fused_linear(x, w, epilogue="residual_add", out=res, workspace=ws)
    torch.cuda.synchronize()
    outs[f"gemm_splitk_{m}_{n}_{k}"] = res.view(torch.int16).cpu().numpy()
np.savez(sys.argv[2], **outs)
'''
res = []
for lib in (None, sys.argv[1]):
    env = dict(os.environ)
    if lib:
        env["NVH_LIB_PATH"] = lib
    else:
        env.pop("NVH_LIB_PATH", None)
    f = tempfile.mktemp(suffix=".npz")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, f], check=True, env=env)
    res.append(dict(np.load(f)))
for k in sorted(res[0]):
    same = np.array_equal(res[0][k], res[1][k])
    print(f"{k}: shape {res[0][k].shape} second library == shipped bit for bit: {same}")
    assert same
print(f"{os.path.basename(sys.argv[1])} and the shipped library agree bit for bit on all {len(res[0])} cases")
