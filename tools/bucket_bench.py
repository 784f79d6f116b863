"""What aspect-ratio bucketing costs a training step.  Prints one JSON line; nothing here is a threshold.

  python tools/bucket_bench.py [--batch 16] [--rounds 3] [--steady 3] [--images 64] [--repeats 20] [--tiny] [--out FILE]

Step.  The SD-2-base U-Net on precomputed latents (seeded random weights and inputs), one optimizer step per call of
``Trainer.train_batch``, host clock around a device synchronise.  After every shape has run once (code objects, workspaces):
  steady_ms      per shape of ``bucket_table(512)`` (17) and for the square 512: ``--steady`` consecutive steps of the SAME
                 shape, the first one dropped - the time of a run that only ever sees that shape
  alternating_ms per shape, the step when the shape changes EVERY step: ``--rounds`` rounds, each cycling the 17 shapes, a
                 square 512 step after each bucket step (``square_interleaved_ms``), so both are taken in the same rounds
  the summary    mean of the 17 steady times, mean of the alternating times, their ratio, and both against the square step
Every bucket has at most 512 * 512 pixels, so its step should cost about the square one; what alternating adds on top of the
steady mean is what rebuilding the per-shape scratch (``UNetHIP._ensure_scratch``) and the allocator cost.

Ingest.  ``--images`` seeded 640 x 480 sources to (448, 576), the bucket a 4:3 landscape image falls into: the rectangular
entry (centre crop) and the augmenting entry with random origins and flips (``ops.image_ingest_aug``), device events, median
of ``--repeats`` launches, kind 0."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def ingest_part(a, dev):
    import torch
    from diffusion_amd import ops
    from diffusion_amd.datasets.buckets import assign_bucket, bucket_table, draw_aug
    from diffusion_amd.datasets.image_ingest import pack_images
    B, w, h = a.images, 640, 480
    table = bucket_table(512)
    Rh, Rw = table[assign_bucket(w, h, table)]
    rng = np.random.default_rng(17)
    base = rng.integers(0, 256, (B, h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8).repeat(8, 1).repeat(8, 2)[:, :h, :w]
    imgs = (base.astype(np.int16) + rng.integers(-20, 21, (B, h, w, 3), dtype=np.int16)).clip(0, 255).astype(np.uint8)
    raw, off, hw = pack_images([torch.from_numpy(im) for im in imgs])
    aug = torch.tensor([draw_aug(17, 0, i, w, h, (Rh, Rw), True, 0.5) for i in range(B)], dtype=torch.int32)
    d_raw, d_off, d_hw, d_aug = raw.to(dev), off.to(dev), hw.to(dev), aug.to(dev)
    x = torch.empty(B * Rh * Rw, 8, device=dev, dtype=torch.bfloat16)

    def timed(fn, reps, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}

    rect = timed(lambda: ops.image_ingest_rect(d_raw, d_off, d_hw, Rh, Rw, x, 0, host=(off, hw)), a.repeats)
    augd = timed(lambda: ops.image_ingest_aug(d_raw, d_off, d_hw, d_aug, Rh, Rw, x, 0, host=(off, hw, aug)), a.repeats)
    rect2 = timed(lambda: ops.image_ingest_rect(d_raw, d_off, d_hw, Rh, Rw, x, 0, host=(off, hw)), a.repeats)
    return {'images': B, 'source': [w, h], 'bucket': [Rh, Rw], 'flipped': int(aug[:, 2].sum()), 'repeats': a.repeats,
            'rect': rect, 'aug': augd, 'rect_again': rect2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steady', type=int, default=3)
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--tiny', action='store_true', help='the tiny U-Net on bucket_table(128, 64, 64, 256): a rehearsal, not a measurement')
    ap.add_argument('--out', default=None, help='also write the JSON here')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bucket_bench: no GPU')
    from diffusion_amd.datasets.buckets import bucket_table
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    dev = torch.device('cuda:0')
    R, table, text_dim = (128, bucket_table(128, 64, 64, 256), 128) if a.tiny else (512, bucket_table(512), 1024)
    name = 'tiny' if a.tiny else 'stabilityai/stable-diffusion-2-base'
    torch.manual_seed(17)
    model = stable_diffusion_2(model_name=name, pretrained=False, precomputed_latents=True, fsdp=False, seed=17)
    trainer = Trainer(model, train_dataloader=None, optimizers=FusedAdamW(lr=1e-4, weight_decay=0.01, unet=model.unet),
                      max_duration='1ba', device_train_microbatch_size=a.batch)
    g = torch.Generator().manual_seed(1000)
    cond = torch.randn(a.batch, 77, text_dim, generator=g).half().to(dev)

    def batch(shape):
        return {'image_latents': torch.randn(a.batch, 4, shape[0] // 8, shape[1] // 8, generator=g).half().to(dev),
                'caption_latents': cond}

    batches = {s: batch(s) for s in table}
    square = batch((R, R))   # its own tensors; the same shape as the table's square entry

    def step(bt):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = trainer.train_batch(bt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss.item())

    for s in table:   # every shape once: code objects, workspaces, the allocator's blocks
        step(batches[s])
    steady = {}
    for s in table + ['square']:
        bt = square if s == 'square' else batches[s]
        ts = [step(bt)[0] for _ in range(a.steady)]
        steady[s] = statistics.mean(ts[1:])
    alt = {s: [] for s in table}
    sq = []
    for _ in range(a.rounds):
        for s in table:
            alt[s].append(step(batches[s])[0])
            sq.append(step(square)[0])
    steady_mean = statistics.mean(steady[s] for s in table)
    alt_mean = statistics.mean(statistics.mean(v) for v in alt.values())
    res = {'bench': 'bucket_bench', 'model': name, 'R': R, 'batch': a.batch, 'rounds': a.rounds, 'steady_steps': a.steady - 1,
           'shapes': [{'shape': list(s), 'steady_ms': round(steady[s], 2), 'alternating_ms': round(statistics.mean(alt[s]), 2),
                       'alternating_min_ms': round(min(alt[s]), 2), 'alternating_max_ms': round(max(alt[s]), 2)} for s in table],
           'square_steady_ms': round(steady['square'], 2), 'square_interleaved_ms': round(statistics.mean(sq), 2),
           'square_interleaved_min_ms': round(min(sq), 2), 'square_interleaved_max_ms': round(max(sq), 2),
           'steady_mean_ms': round(steady_mean, 2), 'alternating_mean_ms': round(alt_mean, 2),
           'alternating_over_steady_mean': round(alt_mean / steady_mean, 4),
           'alternating_over_square_interleaved': round(alt_mean / statistics.mean(sq), 4),
           'images_per_s_alternating': round(a.batch / alt_mean * 1e3, 1),
           'images_per_s_square_interleaved': round(a.batch / statistics.mean(sq) * 1e3, 1)}
    del trainer, model, batches, square
    torch.cuda.empty_cache()
    res['ingest'] = ingest_part(a, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
