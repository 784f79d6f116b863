"""``FrechetInceptionDistance.update`` on the HIP path against torch's own bf16 tower and against ``generate()`` for the same
batch.  Prints one JSON line.

  python tools/fid_bench.py [--batch 4] [--px 512] [--steps 50] [--guidance 3.0] [--seconds 8] [--model NAME] [--no-generate]

Random-init weights throughout (the Inception tower from the metric's fixed seed, SD-2-base's configuration for the model).
  * 'hip': one ``update(real=True)`` plus one ``update(real=False)`` of ``--batch`` fp32 images of ``--px`` x ``--px`` resident
    on the device (``normalize=True``): ``da_inception_preprocess``, the 94 + 13 launches of ``InceptionV3HIP``, the global
    average and ``da_feature_moments``, twice;
  * 'torch_bf16': the same network, the same folded weights, walked with torch's own ops (``F.conv2d`` + ReLU, ``F.max_pool2d``,
    ``F.avg_pool2d``) in bf16 channels-last on the same GPU, from the same preprocessed input, twice - the tower only, without
    the preprocessing and the moments;
  * 'generate': ``StableDiffusion.generate()`` of that batch (text encoder, ``--steps`` sampler steps with guidance, VAE decode).
Each route runs once untimed, then whole calls are timed in rounds, the routes interleaved and the starting route rotated, a
host clock around each call closed by a device synchronise, until ``--seconds`` are spent (at least three rounds).  ``ms`` is
the median call, ``spread`` is (max - min) / median.  ``fid_over_generate`` is the requirement of DESIGN.md section 4.8: the
real + fake updates must cost at most 1 % of generating the batch.
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
    ap.add_argument('--no-generate', action='store_true', help='time the two towers only')
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from diffusion_amd import ops
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    if not torch.cuda.is_available():
        raise SystemExit('fid_bench: no GPU')
    dev = torch.device('cuda:0')
    B = a.batch
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        metric = FrechetInceptionDistance(normalize=True, device=dev, max_batch=max(B, 1))
    images = torch.rand(B, 3, a.px, a.px, generator=torch.Generator().manual_seed(1)).to(dev)
    tower = metric._tower()
    P = tower.plan

    # torch's tower: the plan walked with torch ops on bf16 channels-last tensors, the tower's own folded weights
    tw = {}
    for name, (cin, cout, kh, kw, *_r) in P.units.items():
        W, bias = tower.units[name]
        tw[name] = (W.view(cout, kh, kw, cin).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last),
                    bias.to(torch.bfloat16))
    tbuf = {name: torch.empty(B, C, side, side, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
            for name, (side, C) in P.bufs.items()}
    pre = torch.empty(B * 299 * 299, 8, device=dev, dtype=torch.bfloat16)
    ops.inception_preprocess(images, pre)
    tbuf['x'].copy_(pre.view(B, 299, 299, 8).permute(0, 3, 1, 2))

    @torch.no_grad()
    def torch_tower():
        for op in P.ops:
            if op[0] == 'conv':
                _, unit, src, dst, col = op
                cin, cout, kh, kw, s, ph, pw = P.units[unit]
                W, bias = tw[unit]
                tbuf[dst][:, col:col + cout] = F.relu(F.conv2d(tbuf[src], W, bias, stride=s, padding=(ph, pw)))
            else:
                _, kind, s, p, src, dst, col = op
                x = tbuf[src]
                y = F.max_pool2d(x, 3, stride=s, padding=p) if kind == 0 else \
                    F.avg_pool2d(x, 3, stride=s, padding=p, count_include_pad=False)
                tbuf[dst][:, col:col + x.shape[1]] = y
        return tbuf[P.blocks[-1]].float().mean(dim=(2, 3))

    def hip():
        metric.update(images, real=True)
        metric.update(images, real=False)

    def torch_bf16():
        torch_tower()
        return torch_tower()

    routes = {'hip': hip, 'torch_bf16': torch_bf16}
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
    f_hip, f_torch = metric.features(images), torch_tower()
    rel = ((f_hip - f_torch).norm() / f_torch.norm()).item()
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
    res = {'bench': 'fid', 'batch': B, 'px': a.px, 'steps': a.steps, 'guidance': a.guidance, 'seconds': a.seconds, 'rounds': rnd}
    for n in names:
        med = statistics.median(times[n])
        res[n] = dict(ms=round(med * 1e3, 3), calls=len(times[n]), spread=round((max(times[n]) - min(times[n])) / med, 3))
        if n != 'generate':
            res[n]['images_per_s'] = round(2 * B / med, 1)
    res['hip_over_torch_bf16'] = round(res['hip']['ms'] / res['torch_bf16']['ms'], 3)
    res['features_rel_l2_vs_torch_bf16'] = float(f'{rel:.3e}')
    if 'generate' in res:
        res['fid_over_generate'] = float(f'{res["hip"]["ms"] / res["generate"]["ms"]:.3e}')
        res['requirement_fid_at_most_1_percent_of_generate'] = bool(res['fid_over_generate'] <= 0.01)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
