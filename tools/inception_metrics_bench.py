"""``InceptionScore`` and ``KernelInceptionDistance`` on the HIP path against ``generate()`` for the same batch.  Prints one
JSON line.

  python tools/inception_metrics_bench.py [--batch 4] [--px 512] [--steps 50] [--guidance 3.0] [--seconds 8] [--model NAME]
                                          [--rows 2000] [--score-rows 5000] [--no-generate]

Random-init weights throughout (the Inception tower and its logits head from the metrics' fixed seed, SD-2-base's
configuration for the model).
  * 'updates': ``InceptionScore.update`` + ``KernelInceptionDistance.update(real=True)`` + ``update(real=False)`` of ``--batch``
    fp32 images of ``--px`` x ``--px`` resident on the device (``normalize=True``): three walks of the shared tower, one
    ``da_fc_logits_f32``, three appends;
  * 'kid_compute': ``KernelInceptionDistance.compute()`` at the defaults (100 subsets of 1000) over ``--rows`` stored rows per
    side - the host's subset draw and range check, the upload, ``da_poly_mmd``, the read-back;
  * 'score_compute': ``InceptionScore.compute()`` (10 splits) over ``--score-rows`` stored rows;
  * 'generate': ``StableDiffusion.generate()`` of that batch (text encoder, ``--steps`` sampler steps with guidance, VAE decode).
The stores of the two compute routes hold random rows: their cost does not depend on the values.  Each route runs once
untimed, then whole calls are timed in rounds, the routes interleaved and the starting route rotated, a host clock around
each call closed by a device synchronise, until ``--seconds`` are spent (at least three rounds).  ``ms`` is the median call,
``spread`` is (max - min) / median.  The two requirements of DESIGN.md section 4.8: the three updates cost at most 1.5 % of
generating the batch, and ``kid_compute`` at most 1 % of generating ``subset_size`` = 1000 images (the batch's time scaled
linearly).
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--px', type=int, default=512)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--guidance', type=float, default=3.0)
    ap.add_argument('--seconds', type=float, default=8.0)
    ap.add_argument('--model', default='stabilityai/stable-diffusion-2-base')
    ap.add_argument('--rows', type=int, default=2000, help='stored rows per side for kid_compute')
    ap.add_argument('--score-rows', type=int, default=5000, help='stored rows for score_compute')
    ap.add_argument('--no-generate', action='store_true', help='time the metric routes only')
    a = ap.parse_args()

    import torch
    from diffusion_amd.metrics.inception_score import InceptionScore
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    if not torch.cuda.is_available():
        raise SystemExit('inception_metrics_bench: no GPU')
    dev = torch.device('cuda:0')
    B = a.batch
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        kw = dict(normalize=True, device=dev, max_batch=max(B, 1))
        score_u, kid_u = InceptionScore(**kw), KernelInceptionDistance(**kw)   # fed by 'updates'
        score_c, kid_c = InceptionScore(**kw), KernelInceptionDistance(**kw)   # hold the rows of the compute routes
    g = torch.Generator().manual_seed(1)
    images = torch.rand(B, 3, a.px, a.px, generator=g).to(dev)
    for side in ('real', 'fake'):
        kid_c.stores[side].append(torch.randn(a.rows, 2048, generator=g).to(dev))
    score_c.store.append((3.0 * torch.randn(a.score_rows, 1008, generator=g)).to(dev))

    def updates():
        score_u.reset()   # host-side row counts only: the stores keep their allocation
        kid_u.reset()
        score_u.update(images)
        kid_u.update(images, real=True)
        kid_u.update(images, real=False)

    routes = {'updates': updates, 'kid_compute': kid_c.compute, 'score_compute': score_c.compute}
    if not a.no_generate:
        from diffusion_amd.models.models import stable_diffusion_2
        model = stable_diffusion_2(model_name=a.model, pretrained=False, fsdp=False, encode_latents_in_fp16=False)
        ids = torch.randint(1000, 40000, (B, 77), generator=torch.Generator().manual_seed(2))
        routes['generate'] = lambda: model.generate(tokenized_prompts=ids, height=a.px, width=a.px, guidance_scale=a.guidance,
                                                     num_inference_steps=a.steps, seed=3, progress_bar=False)
    names = list(routes)
    for n in names:
        routes[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    t_end, rnd = time.perf_counter() + a.seconds, 0
    while time.perf_counter() < t_end or rnd < 3:
        for k in range(len(names)):
            n = names[(k + rnd) % len(names)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[n]()
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
        rnd += 1
    kid_mean, kid_std = kid_c.compute()
    is_mean, is_std = score_c.compute()
    res = {'bench': 'inception_metrics', 'batch': B, 'px': a.px, 'steps': a.steps, 'guidance': a.guidance, 'seconds': a.seconds,
           'rounds': rnd, 'kid': dict(subsets=kid_c.subsets, subset_size=kid_c.subset_size, rows_per_side=a.rows,
                                      mmd_engine='v_mfma_f64_16x16x4_f64', value=[float(kid_mean), float(kid_std)]),
           'score': dict(splits=score_c.splits, rows=a.score_rows, value=[float(is_mean), float(is_std)])}
    for n in names:
        med = statistics.median(times[n])
        res[n] = dict(ms=round(med * 1e3, 3), calls=len(times[n]), spread=round((max(times[n]) - min(times[n])) / med, 3))
    pairs = 2.0 * kid_c.subsets * kid_c.subset_size ** 2 * 2048 * 2   # XX and YY halved by symmetry, XY whole
    res['kid_compute']['whole_call_fp64_tflops'] = round(pairs / (res['kid_compute']['ms'] * 1e-3) / 1e12, 2)
    if 'generate' in res:
        gen = res['generate']['ms']
        res['updates_over_generate'] = float(f'{res["updates"]["ms"] / gen:.3e}')
        res['requirement_updates_at_most_1p5_percent_of_generate'] = bool(res['updates_over_generate'] <= 0.015)
        gen_m = gen * kid_c.subset_size / B
        res['generate_of_subset_size_images_ms'] = round(gen_m, 1)
        res['kid_compute_over_generate_of_subset_size_images'] = float(f'{res["kid_compute"]["ms"] / gen_m:.3e}')
        res['requirement_kid_compute_at_most_1_percent'] = bool(res['kid_compute_over_generate_of_subset_size_images'] <= 0.01)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
