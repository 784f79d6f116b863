"""The denoising loop of ``generate()`` three ways: ``'torch'`` (the reference's loop around ``unet(...)`` with the scheduler
step in torch ops), ``'hip'`` (``sampling.LatentSampler``) and ``'graph'`` (the same, one hipGraph replay per step).  Prints
one JSON line.

  python tools/sample_bench.py [--batches 1,4,16] [--steps 20] [--px 256] [--guidance 3.0] [--seconds 6] [--model NAME]
                                [--scheduler ddim|dpm++2m] [--inpaint] [--guidance-rescale PHI]

SD-2-base U-Net, random init, precomputed text embeddings (no VAE, no text encoder: the loop alone), latents of
``px / 8``.  Per batch size B (2 B U-Net rows with guidance):
  * every mode runs once untimed first (warm-up of every shape; the graph is captured here), with the allocator's peak read
    around it: ``peak_mib`` is ``torch.cuda.max_memory_allocated`` of that run, ``above_resident_mib`` the same minus what
    was allocated when it started (weights, scratch; for 'graph' the run includes the capture and its private pool);
  * then whole ``sample()`` calls are timed in rounds, the three modes interleaved and the starting mode rotated per round, a
    host clock around each call closed by a device synchronise, until ``--seconds`` have been spent on the batch size;
  * ``ms_per_step`` and ``images_per_s`` are from the median call; ``spread`` is (max - min) / median over the calls;
  * ``rel_l2_vs_torch`` compares the final latents of the same seeded inputs.
``--scheduler dpm++2m`` runs the three modes with ``DPMSolverMultistepScheduler`` and adds a fourth to the same rounds,
``ddim_hip`` (the ``'hip'`` mode with the DDIM scheduler), so that the per-step times of the two solvers come from
interleaved calls of one session.
``--inpaint`` adds ``inpaint`` to the same rounds: the ``'hip'`` mode as a masked sample (``sample(known=, mask_px=)``, a
half-plane mask, ``start_index=0`` so that it runs the same ``--steps`` steps), i.e. one ``sampler_init`` launch and the
blended step launch in place of the plain one.  ``ms_per_step_vs_hip`` is its median call over the unmasked ``'hip'`` one.
``--guidance-rescale PHI`` (PHI in (0, 1], needs ``--guidance`` > 1) adds ``rescale`` to the same rounds: the ``'hip'`` mode
with ``sample(guidance_rescale=PHI)``, i.e. one statistics launch per step and the rescaled step launch in place of the plain
one.  ``ms_per_step_vs_hip`` is its median call over the plain ``'hip'`` one and ``ms_per_step_over_hip`` the difference.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ('torch', 'hip', 'graph')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,4,16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--px', type=int, default=256)
    ap.add_argument('--guidance', type=float, default=3.0)
    ap.add_argument('--seconds', type=float, default=6.0)
    ap.add_argument('--model', default='stabilityai/stable-diffusion-2-base')
    ap.add_argument('--scheduler', default='ddim', choices=('ddim', 'dpm++2m'))
    ap.add_argument('--inpaint', action='store_true')
    ap.add_argument('--guidance-rescale', type=float, default=0.0)
    a = ap.parse_args()
    if a.guidance_rescale and not (0.0 < a.guidance_rescale <= 1.0 and a.guidance > 1.0):
        raise SystemExit('sample_bench: --guidance-rescale takes PHI in (0, 1] and needs --guidance > 1')

    import torch
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.models.schedulers import make_inference_scheduler
    from diffusion_amd.sampling import LatentSampler
    if not torch.cuda.is_available():
        raise SystemExit('sample_bench: no GPU')
    dev = torch.device('cuda:0')
    model = stable_diffusion_2(model_name=a.model, pretrained=False, precomputed_latents=True, fsdp=False,
                               inference_scheduler=a.scheduler)
    unet, sch = model.unet, model.inference_scheduler
    sampler = LatentSampler(unet, sch)
    modes = MODES + (('ddim_hip',) if a.scheduler != 'ddim' else ()) + (('inpaint',) if a.inpaint else ()) \
        + (('rescale',) if a.guidance_rescale else ())
    ddim_sampler = LatentSampler(unet, make_inference_scheduler('ddim', like=sch))
    S, D = a.px // 8, unet.cfg.cross_attention_dim
    cfg = a.guidance > 1.0

    @torch.no_grad()
    def torch_loop(lat, txt, unc):   # generate()'s 'torch' loop
        emb = torch.cat([unc, txt]) if cfg else txt
        sch.set_timesteps(a.steps)
        for t in sch.timesteps:
            lin = torch.cat([lat] * 2) if cfg else lat
            pred = unet(lin, t, encoder_hidden_states=emb).sample
            if cfg:
                pu, pt = pred.chunk(2)
                pred = pu + a.guidance * (pt - pu)
            lat = sch.step(pred, t, lat)['prev_sample']
        return lat

    def run(mode, lat, txt, unc):
        if mode == 'inpaint':
            return sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance, known=known,
                                  start_index=0, mask_px=mask_px)
        if mode == 'rescale':
            return sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance,
                                  guidance_rescale=a.guidance_rescale)
        if mode == 'torch':
            return torch_loop(lat, txt, unc)
        if mode == 'ddim_hip':
            return ddim_sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance)
        return sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance, graph=mode == 'graph')

    res = {'bench': 'sample', 'model': a.model, 'scheduler': a.scheduler, 'px': a.px, 'steps': a.steps, 'guidance': a.guidance,
           'guidance_rescale': a.guidance_rescale, 'seconds_per_batch': a.seconds, 'batches': []}
    for B in (int(b) for b in a.batches.split(',')):
        g = torch.Generator().manual_seed(100 + B)
        lat = torch.randn(B, unet.cfg.in_channels, S, S, generator=g).to(dev)
        txt, unc = torch.randn(B, 77, D, generator=g).to(dev), torch.randn(B, 77, D, generator=g).to(dev)
        known = torch.randn(lat.shape, generator=g).to(dev)
        mask_px = torch.zeros(B, a.px, a.px, device=dev)
        mask_px[:, :, a.px // 2:] = 1.0   # repaint the right half
        row, outs, times = {'B': B}, {}, {m: [] for m in modes}
        sampler.graphs.clear()
        run('hip', lat, txt, unc)   # scratch and workspaces of this shape exist before any peak is read
        for m in modes:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            outs[m] = run(m, lat, txt, unc)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            row[m] = {'peak_mib': round(peak / 2**20, 1), 'above_resident_mib': round((peak - base) / 2**20, 1)}
        t_end, rnd = time.perf_counter() + a.seconds, 0
        while time.perf_counter() < t_end or rnd < 3:
            for k in range(len(modes)):
                m = modes[(k + rnd) % len(modes)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(m, lat, txt, unc)
                torch.cuda.synchronize()
                times[m].append(time.perf_counter() - t0)
            rnd += 1
        ref = outs['torch'].float()
        for m in modes:
            med = statistics.median(times[m])
            row[m].update(ms_per_step=round(med * 1e3 / a.steps, 3), images_per_s=round(B / med, 2), calls=len(times[m]),
                          spread=round((max(times[m]) - min(times[m])) / med, 3))
            if m in MODES:   # ddim_hip is another solver, inpaint another sample: their latents are not comparable
                row[m]['rel_l2_vs_torch'] = float(f'{((outs[m].float() - ref).norm() / ref.norm()).item():.3e}')
        if 'ddim_hip' in modes:
            row['hip']['ms_per_step_vs_ddim_hip'] = round(statistics.median(times['hip']) /
                                                          statistics.median(times['ddim_hip']), 4)
        if 'inpaint' in modes:
            row['inpaint']['ms_per_step_vs_hip'] = round(statistics.median(times['inpaint']) /
                                                         statistics.median(times['hip']), 4)
        if 'rescale' in modes:
            row['rescale']['ms_per_step_vs_hip'] = round(statistics.median(times['rescale']) /
                                                         statistics.median(times['hip']), 4)
            row['rescale']['ms_per_step_over_hip'] = round((statistics.median(times['rescale']) -
                                                            statistics.median(times['hip'])) * 1e3 / a.steps, 4)
        for m in ('hip', 'graph'):
            row[m]['speedup_vs_torch'] = round(statistics.median(times['torch']) / statistics.median(times[m]), 3)
        res['batches'].append(row)
        del outs
    sampler.graphs.clear()
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
