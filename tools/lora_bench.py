"""What a LoRA step costs at the bench shape (SD-2-base U-Net, latents 4x32x32, batch 256): ms/step of full fine-tuning
against the LoRA step as an interleaved A/B of Trainer.train_batch on one model, and the per-step passes LoRA adds - the
projection (da_lora_project), AdamW over the adapter buffers, the merge (da_lora_merge) and the transposed-shadow refresh
- timed on their own.  Prints one JSON line.

  python tools/lora_bench.py [--rank 16] [--targets to_q to_k ...] [--rounds 4] [--steps 3] [--batch 256]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def times_ms(fn, launches):
    out = []
    for _ in range(launches):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return {'median_ms': round(statistics.median(out), 4), 'min_ms': round(min(out), 4), 'max_ms': round(max(out), 4)}


def main(a):
    from diffusion_amd import ops
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    dev = torch.device('cuda')
    B, S = a.batch, 32
    torch.manual_seed(17)
    model = stable_diffusion_2(model_name='stabilityai/stable-diffusion-2-base', pretrained=False, precomputed_latents=True,
                               fsdp=False, seed=17)
    unet = model.unet
    opt = FusedAdamW(lr=1e-4, weight_decay=0.01, unet=unet)
    tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration='1ba', device_train_microbatch_size=B)
    g = torch.Generator().manual_seed(1000)
    batch = {'image_latents': torch.randn(B, 4, S, S, generator=g).half().to(dev),
             'caption_latents': torch.randn(B, 77, 1024, generator=g).half().to(dev)}

    def run(lora, steps):
        if lora and unet.lora is None:
            unet.add_lora(a.rank, target_modules=a.targets)
            opt.attach_lora()
        elif not lora and unet.lora is not None:
            opt.detach_lora()
            unet.remove_lora()
        tr.train_batch(batch)     # untimed: the first step after a switch
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            tr.train_batch(batch)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / steps

    run(False, 1), run(True, 1)
    ts = {False: [], True: []}
    for _ in range(a.rounds):
        for lora in (False, True):
            ts[lora].append(run(lora, a.steps))
    full, lo = statistics.median(ts[False]), statistics.median(ts[True])
    ad = unet.lora
    mt, da, db = ad.tiles()
    res = {'batch': B, 'latent': S, 'rank': ad.rank, 'targets': list(ad.target_modules), 'adapted_matrices': len(ad.items),
           'adapter_params': sum(it.r * (it.K + it.N) for it in ad.items),
           'adapted_weight_elements': sum(it.N * it.K for it in ad.items), 'tiles': {'merge': mt, 'dA': da, 'dB': db},
           'rounds': a.rounds, 'steps_per_round': a.steps, 'step_ms_full': round(full, 3), 'step_ms_lora': round(lo, 3),
           'lora_over_full': round(lo / full, 4), 'full_all': [round(t, 3) for t in ts[False]],
           'lora_all': [round(t, 3) for t in ts[True]]}
    # the passes the LoRA step adds, on their own (the step above has just left a real dW in unet.grad)
    step = [unet.opt_step]

    def adamw():
        step[0] += 1
        ops.adamw(ad.params, ad.grad, ad.exp_avg, ad.exp_avg_sq, ad.shadow_scratch, 1e-4, 0.9, 0.999, 1e-8, 0.01, step[0], 1.0)

    passes = {'project': lambda: ops.lora_project(unet.grad, ad), 'adapter_adamw': adamw,
              'merge': lambda: ops.lora_merge(unet.master, ad, unet.shadow), 'refresh_transposed': unet.refresh_transposed}
    res['passes'] = {}
    for name, fn in passes.items():
        for _ in range(3):
            fn()
        res['passes'][name] = times_ms(fn, a.launches)
    res['passes_total_median_ms'] = round(sum(v['median_ms'] for v in res['passes'].values()), 4)
    return res


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rank', type=int, default=16)
    ap.add_argument('--targets', nargs='*', default=None)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    print(json.dumps(main(ap.parse_args())))
