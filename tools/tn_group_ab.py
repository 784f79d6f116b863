"""A/B of da_set_option('gemm_tn_ungroup', 1 | 0) on the eight linear weight gradients of a transformer block at the three
levels of the batch-B step (one process, interleaved rounds; each op includes its slab reduces), with the plan
da_gemm_tn_group_plan gives the block.  usage: tn_group_ab.py [B=256] [workspace MiB=128]"""
import sys, os, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffusion_amd import ops
dev = torch.device('cuda'); BF = torch.bfloat16
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ops.SPLITK_WS = torch.empty((int(sys.argv[2]) if len(sys.argv) > 2 else 128) * 256 * 1024, device=dev, dtype=torch.float32)


def once(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


for h, C in ((32, 320), (16, 640), (8, 1280)):
    M = B * h * h
    # proj_out, ff.net.2, ff.net.0.proj, attn2.to_out, attn2.to_q, attn1.to_out, attn1.qkv, proj_in: (N, Cin, bias) in backward order
    shapes = [(C, C, 1), (C, 4 * C, 1), (8 * C, C, 1), (C, C, 1), (C, C, 0), (C, C, 1), (3 * C, C, 0), (C, C, 1)]
    acts = {c: torch.randn(M, c, device=dev).to(BF) for c in {s[0] for s in shapes} | {s[1] for s in shapes}}
    items = [(acts[N], acts[Cin], torch.zeros(N, Cin, device=dev), torch.zeros(N, device=dev) if b else None) for N, Cin, b in shapes]
    fl = sum(2.0 * M * N * Cin for N, Cin, _ in shapes)
    plan = ops.gemm_tn_group_plan(shapes, M, ops.SPLITK_WS.numel())
    fn = lambda: ops.gemm_tn_wgrad_group(items, M)
    ts = {1: [], 0: []}
    for rnd in range(5):
        for v in ts:
            ops.set_option('gemm_tn_ungroup', v)
            fn(); ts[v].append(once(fn, 5))
    m = {v: statistics.median(t) for v, t in ts.items()}
    print(f'M={M:6d} C={C:4d}: per-layer {m[1]*1e3:7.1f} us {fl/m[1]/1e9:6.1f} TF/s | grouped {m[0]*1e3:7.1f} us {fl/m[0]/1e9:6.1f} TF/s '
          f'x{m[1]/m[0]:.3f} | splits {plan["splits"]} group_of {plan["group_of"]}', flush=True)
    del items, acts
ops.set_option('gemm_tn_ungroup', 0)
