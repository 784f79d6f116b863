"""``CLIPScore.update`` on the HIP path against the reference route, and the preprocessing kernel alone against PIL.  Prints one
JSON line.

  python tools/clip_score_bench.py [--batch 16] [--px 512] [--seconds 6] [--layers N]

Full ViT-L/14 widths (openai/clip-vit-large-patch14's configuration, random init; ``--layers`` narrows both towers for a
rehearsal), ``--batch`` uint8 images of ``--px`` x ``--px`` on the host and as many captions.
  * 'hip': ``CLIPScore.update`` (upload of the bytes, ``da_clip_preprocess``, the two towers, ``da_clip_score``);
  * 'reference': what torchmetrics' CLIPScore does - ``CLIPImageProcessor`` (PIL, on the host), the tokenizer, the torch
    ``CLIPModel`` in fp16 on the GPU, normalise, 100 x cosine, running sum.
Each route runs once untimed, then whole calls are timed in rounds, the two routes interleaved and the starting route
rotated, a host clock around each call closed by a device synchronise, until ``--seconds`` are spent.  ``ms`` and
``images_per_s`` are from the median call, ``spread`` is (max - min) / median.  ``preprocess`` times the kernel alone
(device events around 20 launches on resident images) and PIL's resize + crop + normalise of the same images on the host.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--px', type=int, default=512)
    ap.add_argument('--seconds', type=float, default=6.0)
    ap.add_argument('--layers', type=int, default=0, help='layers per tower (0: the full 24 / 12)')
    a = ap.parse_args()

    import copy
    import torch
    from transformers import CLIPConfig, CLIPImageProcessor, CLIPModel
    from diffusion_amd import ops
    from diffusion_amd.metrics.clip_score import CLIPScore
    from diffusion_amd.models.text import CLIP_L14_TEXT, CLIP_L14_VISION, ByteTokenizer
    if not torch.cuda.is_available():
        raise SystemExit('clip_score_bench: no GPU')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    tc, vc = dict(CLIP_L14_TEXT), dict(CLIP_L14_VISION)
    if a.layers:
        tc['num_hidden_layers'] = vc['num_hidden_layers'] = a.layers
    model = CLIPModel(CLIPConfig(text_config=tc, vision_config=vc, projection_dim=vc['projection_dim'])).float().eval()
    tok, proc = ByteTokenizer(), CLIPImageProcessor()
    metric = CLIPScore(model=model, tokenizer=tok, device=dev)
    half = copy.deepcopy(model).to(dev, torch.float16)
    B = a.batch
    images = torch.randint(0, 256, (B, 3, a.px, a.px), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    captions = [f'caption number {i} of a generated picture' for i in range(B)]
    ref_state = torch.zeros(2, device=dev)

    @torch.no_grad()
    def reference():
        pv = proc(images=[i for i in images], return_tensors='pt')['pixel_values']
        ids = tok(captions, padding='max_length', max_length=77, truncation=True, return_tensors='pt')['input_ids']
        out = half(input_ids=ids.to(dev), pixel_values=pv.to(dev, torch.float16))
        score = 100.0 * (out.image_embeds * out.text_embeds).sum(-1)
        ref_state[0] += score.sum()
        ref_state[1] += B
        return score.float()

    routes = {'hip': lambda: metric.update(images, captions), 'reference': reference}
    names = list(routes)
    outs = {n: routes[n]() for n in names}
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
    res = {'bench': 'clip_score', 'batch': B, 'px': a.px, 'vision_layers': vc['num_hidden_layers'],
           'text_layers': tc['num_hidden_layers'], 'seconds': a.seconds}
    for n in names:
        med = statistics.median(times[n])
        res[n] = dict(ms=round(med * 1e3, 3), images_per_s=round(B / med, 1), calls=len(times[n]),
                      spread=round((max(times[n]) - min(times[n])) / med, 3))
    res['speedup_vs_reference'] = round(statistics.median(times['reference']) / statistics.median(times['hip']), 3)
    res['max_abs_score_diff_vs_fp16_reference'] = float(f'{(outs["hip"] - outs["reference"]).abs().max().item():.3e}')

    # the preprocessing alone: the kernel on resident images (device events) against PIL on the host
    vision = metric._towers()[0]
    d_img = images.to(dev)
    vision.patch_matrix(d_img, metric.mean, metric.std)
    n_launch = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n_launch):
        vision.patch_matrix(d_img, metric.mean, metric.std)
    e1.record()
    torch.cuda.synchronize()
    kernel_ms = e0.elapsed_time(e1) / n_launch
    pil = []
    for _ in range(3):
        t0 = time.perf_counter()
        proc(images=[i for i in images], return_tensors='pt')
        pil.append(time.perf_counter() - t0)
    pil_ms = statistics.median(pil) * 1e3
    res['preprocess'] = dict(kernel_ms=round(kernel_ms, 4), kernel_images_per_s=round(B / kernel_ms * 1e3, 1),
                             pil_host_ms=round(pil_ms, 2), pil_images_per_s=round(B / pil_ms * 1e3, 1),
                             source_mb_per_image=round(3 * a.px * a.px / 1e6, 3))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
