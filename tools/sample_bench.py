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
``--eta ETA`` (DDIM, ETA in (0, 1]) or ``--scheduler dpm++2m-sde`` makes the schedule stochastic: ``'hip'`` and ``'graph'`` then
draw their step noise inside the step launch (``ops.sampler_step_rng``), ``'torch'`` takes the same Philox noise as
``variance_noise``, and two modes join the same rounds: ``det_hip``, the ``'hip'`` mode of the deterministic twin (eta = 0,
``dpm++2m``), and ``unfused``, the stochastic eager loop with the draw as a launch of its own (``ops.randn_philox``) feeding
the deterministic step (its noise operand; the two-step form, which has none, adds ``kn z`` and recasts in torch ops).
``ms_per_step_over_det_hip`` is a mode's median call minus ``det_hip``'s, per step; ``unfused_equals_hip`` says whether the
two stochastic eager loops ended on the same bits: they do for DDIM (the noise operand is the same FMA), not for the two-step
form, whose ``add_(z, alpha=kn)`` here rounds differently from the kernel's product-then-sum.
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
    ap.add_argument('--scheduler', default='ddim', choices=('ddim', 'dpm++2m', 'dpm++2m-sde'))
    ap.add_argument('--inpaint', action='store_true')
    ap.add_argument('--guidance-rescale', type=float, default=0.0)
    ap.add_argument('--eta', type=float, default=0.0)
    a = ap.parse_args()
    if a.guidance_rescale and not (0.0 < a.guidance_rescale <= 1.0 and a.guidance > 1.0):
        raise SystemExit('sample_bench: --guidance-rescale takes PHI in (0, 1] and needs --guidance > 1')
    if a.eta and not (0.0 < a.eta <= 1.0 and a.scheduler == 'ddim'):
        raise SystemExit('sample_bench: --eta takes ETA in (0, 1] and goes with --scheduler ddim')

    import torch
    from diffusion_amd import ops
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.models.schedulers import is_stochastic, make_inference_scheduler
    from diffusion_amd.sampling import LatentSampler
    if not torch.cuda.is_available():
        raise SystemExit('sample_bench: no GPU')
    dev = torch.device('cuda:0')
    model = stable_diffusion_2(model_name=a.model, pretrained=False, precomputed_latents=True, fsdp=False,
                               inference_scheduler=a.scheduler, inference_eta=a.eta)
    unet, sch = model.unet, model.inference_scheduler
    stochastic = is_stochastic(sch)
    sampler = LatentSampler(unet, sch)
    modes = MODES + (('ddim_hip',) if a.scheduler != 'ddim' else ()) + (('inpaint',) if a.inpaint else ()) \
        + (('rescale',) if a.guidance_rescale else ()) + (('det_hip', 'unfused') if stochastic else ())
    ddim_sampler = LatentSampler(unet, make_inference_scheduler('ddim', like=sch))
    det_sampler = LatentSampler(unet, make_inference_scheduler('ddim' if a.scheduler == 'ddim' else 'dpm++2m', like=sch))
    S, D = a.px // 8, unet.cfg.cross_attention_dim
    cfg = a.guidance > 1.0

    @torch.no_grad()
    def torch_loop(lat, txt, unc):   # generate()'s 'torch' loop
        emb = torch.cat([unc, txt]) if cfg else txt
        sch.set_timesteps(a.steps)
        for i, t in enumerate(sch.timesteps):
            lin = torch.cat([lat] * 2) if cfg else lat
            pred = unet(lin, t, encoder_hidden_states=emb).sample
            if cfg:
                pu, pt = pred.chunk(2)
                pred = pu + a.guidance * (pt - pu)
            kw = dict(variance_noise=ops.randn_philox(seeds, i, 0, tuple(lat.shape))) if stochastic else {}
            lat = sch.step(pred, t, lat, **kw)['prev_sample']
        return lat

    @torch.no_grad()
    def unfused_loop(lat, txt, unc):
        """LatentSampler's eager loop with the draw as its own launch: randn_philox, then the deterministic step entry."""
        B, C, H, W = lat.shape
        rows, npix, copies = (2 * B if cfg else B), B * H * W, (2 if cfg else 1)
        sch.set_timesteps(a.steps)
        ts = sch.timesteps.tolist()
        ms = bool(getattr(sch, 'multistep', False))
        if ms:
            tab = [sch.step_coefficients_sde(i) for i in range(len(ts))]
            coef = torch.tensor([list(r[:5]) + [a.guidance, 0.0, 0.0] for r in tab], dtype=torch.float64).float().to(dev)
            kn = [r[5] for r in tab]
        else:
            coef = torch.tensor([[*sch.step_coefficients(t), a.guidance] for t in ts], dtype=torch.float64).float().to(dev)
        t_tab = torch.tensor(ts, dtype=torch.int64)[:, None].expand(len(ts), rows).contiguous().to(dev)
        ctx = unet.prepare_ctx(torch.cat([unc, txt]) if cfg else txt)
        kv = unet.project_context(ctx)
        x = torch.zeros(npix, 8, device=dev)
        xt = torch.empty(rows * H * W, 8, device=dev, dtype=torch.bfloat16)
        hist = torch.empty(npix, 8, device=dev) if ms else None
        z = torch.empty(B, C, H, W, device=dev)
        ops.sampler_step(x, x, torch.tensor([0.0, 0.0, 1.0, 0.0], device=dev), x, xt, lat.contiguous(), C=C, cfg=False,
                         copies=copies)
        for i in range(len(ts)):
            pred = unet.forward_features(xt, t_tab[i], ctx, rows, (H, W), kv=kv, record=False)
            ops.randn_philox(seeds, i, 0, out=z)
            if ms:
                ops.sampler_step_ms(pred, x, hist, coef[i], x, None, C=C, cfg=cfg, copies=copies)
                x.view(B, H, W, 8)[..., :C].add_(z.permute(0, 2, 3, 1), alpha=kn[i])
                ops.cast_f32_bf16(x, xt[:npix])
                if copies == 2:
                    xt[npix:].copy_(xt[:npix])
            else:
                ops.sampler_step(pred, x, coef[i], x, xt, z, C=C, cfg=cfg, copies=copies)
        return x.view(B, H, W, 8)[..., :C].permute(0, 3, 1, 2).contiguous()

    def run(mode, lat, txt, unc):
        skw = dict(seeds=seeds) if stochastic else {}
        if mode == 'inpaint':
            return sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance, known=known,
                                  start_index=0, mask_px=mask_px, **skw)
        if mode == 'rescale':
            return sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance,
                                  guidance_rescale=a.guidance_rescale, **skw)
        if mode == 'torch':
            return torch_loop(lat, txt, unc)
        if mode == 'unfused':
            return unfused_loop(lat, txt, unc)
        if mode == 'det_hip':
            return det_sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance)
        if mode == 'ddim_hip':
            return ddim_sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance)
        return sampler.sample(lat, txt, unc, num_inference_steps=a.steps, guidance_scale=a.guidance, graph=mode == 'graph',
                              **skw)

    res = {'bench': 'sample', 'model': a.model, 'scheduler': a.scheduler, 'px': a.px, 'steps': a.steps, 'guidance': a.guidance,
           'guidance_rescale': a.guidance_rescale, 'eta': a.eta, 'seconds_per_batch': a.seconds, 'batches': []}
    for B in (int(b) for b in a.batches.split(',')):
        g = torch.Generator().manual_seed(100 + B)
        lat = torch.randn(B, unet.cfg.in_channels, S, S, generator=g).to(dev)
        txt, unc = torch.randn(B, 77, D, generator=g).to(dev), torch.randn(B, 77, D, generator=g).to(dev)
        known = torch.randn(lat.shape, generator=g).to(dev)
        mask_px = torch.zeros(B, a.px, a.px, device=dev)
        mask_px[:, :, a.px // 2:] = 1.0   # repaint the right half
        seeds = ops.philox_seeds([1138 + b for b in range(B)], B, dev)   # read by the stochastic modes only
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
            if m in MODES or m == 'unfused':   # ddim_hip / det_hip are other solvers, inpaint another sample: not comparable
                row[m]['rel_l2_vs_torch'] = float(f'{((outs[m].float() - ref).norm() / ref.norm()).item():.3e}')
        if stochastic:
            det = statistics.median(times['det_hip'])
            for m in ('hip', 'unfused', 'graph'):
                row[m]['ms_per_step_over_det_hip'] = round((statistics.median(times[m]) - det) * 1e3 / a.steps, 4)
            row['unfused_equals_hip'] = bool(torch.equal(outs['unfused'], outs['hip']))
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
