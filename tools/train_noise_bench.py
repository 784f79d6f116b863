"""What the training step's noising costs with the draws in the launch.  Prints one JSON line (and writes it to --out).

  * at the two bench shapes (256x4x32x32 and 64x4x64x64): torch.randint + torch.randn + da_add_noise, the three launches of the
    default path, against the one da_add_noise_rng launch - plain, and with offset noise, input perturbation and stratified
    timesteps all on;
  * the graphed training step at microbatch 16 (SD-2-base U-Net, latents 4x32x32, batch 64): noise_source 'torch' against
    'philox' on one model and one trainer, each with its own captured graph.

The candidates alternate inside every round; a window is a loop of launches between two device events.

  python tools/train_noise_bench.py [--rounds 5] [--launches 200] [--steps 3] [--no-step] [--out profiles/train_noise_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def window_us(fn, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    e.synchronize()
    return 1e3 * s.elapsed_time(e) / launches


def summary(v):
    return {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}


def noising(a, dev):
    from diffusion_amd import ops
    from diffusion_amd.models.schedulers import DDPMScheduler
    from diffusion_amd.train_noise import batch_entries
    sa, sb = DDPMScheduler().device_tables(dev)
    out = {}
    for B, C, H, W in ((256, 4, 32, 32), (64, 4, 64, 64)):
        x0 = torch.randn(B, C, H, W, device=dev)
        xt = torch.empty(B * H * W, 8, device=dev, dtype=torch.bfloat16)
        tg = torch.empty(B * H * W, 8, device=dev, dtype=torch.float32)
        t = torch.empty(B, device=dev, dtype=torch.int64)
        ent = batch_entries(17, 0, 0, 1, B, dev)
        seeds, slots = ent['_sample_seeds'], ent['_sample_slots']

        def three_launches():
            tt = torch.randint(0, 1000, (B,), device=dev)
            ops.add_noise(x0, torch.randn_like(x0), tt, sa, sb, xt, tg, False)

        def fused():
            ops.add_noise_rng(x0, seeds, t, xt, tg, 'epsilon', sa, sb)

        def fused_all_options():
            ops.add_noise_rng(x0, seeds, t, xt, tg, 'epsilon', sa, sb, slots=slots, n_slots=B, noise_offset=0.1,
                              perturbation=0.1)

        cands = {'randint_randn_add_noise': three_launches, 'add_noise_rng': fused, 'add_noise_rng_all_options': fused_all_options}
        for fn in cands.values():
            window_us(fn, 20)
        ts = {k: [] for k in cands}
        for _ in range(a.rounds):
            for k, fn in cands.items():
                ts[k].append(window_us(fn, a.launches))
        out[f'{B}x{C}x{H}x{W}'] = {k: summary(v) for k, v in ts.items()}
    return out


def graphed_step(a, dev):
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.train_noise import TrainNoise
    from diffusion_amd.trainer import Trainer
    B, mb = 64, 16
    model = stable_diffusion_2(model_name='stabilityai/stable-diffusion-2-base', pretrained=False, precomputed_latents=True,
                               fsdp=False, seed=17)
    opt = FusedAdamW(lr=1e-4, weight_decay=0.01, unet=model.unet)
    tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration='1ba', device_train_microbatch_size=mb,
                 use_graphs=True, seed=17)
    g = torch.Generator().manual_seed(1000)
    batch = {'image_latents': torch.randn(B, 4, 32, 32, generator=g).half().to(dev),
             'caption_latents': torch.randn(B, 77, 1024, generator=g).half().to(dev)}
    modes = {'torch': TrainNoise(), 'philox': TrainNoise(noise_source='philox')}

    def run(mode, steps):
        model.train_noise = modes[mode]
        tr.train_batch(batch)   # untimed: the capture, or the first replay after the switch
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            tr.train_batch(batch)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / steps

    for m in modes:
        run(m, 1)
    ts = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            ts[m].append(run(m, a.steps))
    return {'batch': B, 'microbatch': mb, 'graphs_captured': tr._graph_cache.captures,
            'step_ms': {m: summary(v) for m, v in ts.items()}, 'all_ms': {m: [round(x, 3) for x in v] for m, v in ts.items()}}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('train_noise_bench: needs an MI355X (a CPU run measures nothing)')
    dev = torch.device('cuda')
    res = {'rounds': a.rounds, 'launches_per_window': a.launches, 'noising_us_per_call': noising(a, dev)}
    if not a.no_step:
        res['graphed_step_mb16'] = graphed_step(a, dev)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)
