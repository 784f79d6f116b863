"""Decode rate of the frozen SD-2 VAE decoder: ``VAEDecoderHIP`` (models/vae_hip.py, bf16 on the HIP kernels) against the
PyTorch-ROCm fp16 ``AutoencoderKL.decode`` it replaces in ``generate()``, same random-init full-size weights, same latents.
Prints one JSON line.

  python tools/decode_bench.py [--repeats 5] [--iters 5] [--warmup 2] [--limit 300]

Shapes: 256 px at batch 16 (32x32 latents) and 512 px at batch 4 (64x64 latents).  Each shape is measured by a child process of
its own under a time limit (--limit seconds; nothing more is started after a child that failed or ran out of time).  Inside a
child both decoders are warmed up, then timed in alternation - HIP, torch, HIP, torch ... - ``repeats`` times with
``iters`` decodes per timed window (device events), so that both see the same state of a shared box; the median window and
the spread (min ... max) of each are reported, and rel-L2 of the two outputs against each other.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 16), (512, 4)]   # (pixels, batch)


def worker(px, batch, repeats, iters, warmup):
    import torch
    from diffusion_amd.models.vae import AutoencoderKL
    from diffusion_amd.models.vae_hip import VAEDecoderHIP
    if not torch.cuda.is_available():
        raise SystemExit('decode_bench: no GPU')
    dev = torch.device('cuda:0')
    torch.manual_seed(7)
    vae = AutoencoderKL().to(dev).eval()
    hip = VAEDecoderHIP(vae)
    vae = vae.half()
    z = torch.randn(batch, 4, px // 8, px // 8, device=dev)
    zh = z.half()
    forms = {'hip': lambda: hip.decode(z).sample, 'torch_fp16': lambda: vae.decode(zh).sample}
    with torch.no_grad():
        outs = {}
        for name, fn in forms.items():
            for _ in range(warmup):
                outs[name] = fn()
        torch.cuda.synchronize()
        a, b = outs['hip'].float(), outs['torch_fp16'].float()
        rel = ((a - b).norm() / b.norm()).item()
        del outs, a, b
        ms = {name: [] for name in forms}
        for _ in range(repeats):
            for name, fn in forms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(iters):
                    fn()
                t1.record()
                t1.synchronize()
                ms[name].append(t0.elapsed_time(t1) / iters)
    res = {'px': px, 'batch': batch, 'rel_l2_hip_vs_torch_fp16': round(rel, 5)}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {'decode_ms': round(med, 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
                     'images_per_s': round(batch / med * 1e3, 1)}
    print('DECODE_BENCH ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=300, help='seconds one shape may take')
    ap.add_argument('--worker', type=int, nargs=2, metavar=('PX', 'BATCH'), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], a.worker[1], a.repeats, a.iters, a.warmup)
    shapes = []
    for px, batch in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--worker', str(px), str(batch), '--repeats', str(a.repeats),
               '--iters', str(a.iters), '--warmup', str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f'decode_bench: {px} px batch {batch} did not finish in {a.limit} s; nothing more started')
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('DECODE_BENCH ')]
        if r.returncode != 0 or not line:
            raise SystemExit(f'decode_bench: {px} px batch {batch} failed ({r.returncode}); nothing more started\n'
                             + r.stderr[-2000:])
        shapes.append(json.loads(line[-1][len('DECODE_BENCH '):]))
    print(json.dumps({'bench': 'vae_decode', 'repeats': a.repeats, 'iters': a.iters, 'warmup': a.warmup, 'shapes': shapes}),
          flush=True)


if __name__ == '__main__':
    main()
