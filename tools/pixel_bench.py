"""Training rate of the pixel-space model: ``continuous_pixel_diffusion()`` (full-width ``UNetConfig.pixel()``, the CLIP
ViT-L/14 text encoder on the HIP kernels, captions encoded every step), through the in-tree ``Trainer`` with the fused
AdamW step, at 64x64 pixels.  Prints one JSON line.

  python tools/pixel_bench.py [--batch 64] [--side 64] [--steps 10] [--warmup 3] [--discrete]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--side', type=int, default=64)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--discrete', action='store_true', help='discrete_pixel_diffusion instead of the continuous model')
    a = ap.parse_args()
    from diffusion_amd.models.models import continuous_pixel_diffusion, discrete_pixel_diffusion
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    torch.manual_seed(17)
    model = (discrete_pixel_diffusion if a.discrete else continuous_pixel_diffusion)()
    opt = FusedAdamW(lr=1e-4, weight_decay=0.01, unet=model.unet)
    tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration=f'{a.steps + a.warmup}ba',
                 device_train_microbatch_size='auto', log_every=10**9)
    dev = model.unet.device_
    batch = {'image': torch.rand(a.batch, 3, a.side, a.side, device=dev) * 2 - 1,
             'captions': torch.randint(0, 49408, (a.batch, 77), device=dev)}
    for _ in range(a.warmup):
        tr.train_batch(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = tr.train_batch(batch)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    print(json.dumps({'model': 'discrete_pixel_diffusion' if a.discrete else 'continuous_pixel_diffusion',
                      'side': a.side, 'batch': a.batch, 'microbatch': list(tr._auto_mb.values()),
                      'steps': a.steps, 'warmup': a.warmup, 'step_ms': round(dt * 1e3, 2),
                      'images_per_s': round(a.batch / dt, 1), 'loss': float(loss.item()),
                      'params': model.unet.num_params, 'device': torch.cuda.get_device_name(0)}), flush=True)


if __name__ == '__main__':
    main()
