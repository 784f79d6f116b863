"""The gradient-norm pass on the full SD-2 layout (865.9 M words, 596 storages), da_adamw beside it on the same box, and
(--step) the whole-step cost of GradientClipping as an interleaved A/B of Trainer.train_batch.  Prints one JSON line.

  python tools/grad_norm_bench.py              norm pass (3 launches) and da_adamw: median / min / max of --launches each
  python tools/grad_norm_bench.py --step       batch 256 at 32^2: steps without and with clipping, interleaved in rounds"""
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
    return out


def summary(ts, nbytes):
    med = statistics.median(ts)
    return {'median_ms': round(med, 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4), 'launches': len(ts),
            'TB_per_s': round(nbytes / med / 1e9, 3)}


def kernel_bench(a):
    from diffusion_amd import ops
    from diffusion_amd.models.unet import SumsqTables, UNetConfig, build_layout, grad_segment_list
    dev = torch.device('cuda')
    fp = build_layout(UNetConfig())[0]
    names, offs, numels = grad_segment_list(fp)
    tables = SumsqTables(list(zip(offs, numels))).to(dev)
    n = fp.total
    g = torch.randn(n, device=dev) * 1e-3
    partials = torch.zeros(len(tables.chunks), device=dev)
    seg = torch.zeros(len(names), device=dev)
    stats = torch.zeros(ops.GRAD_STATS_WORDS, device=dev)
    norm = lambda: ops.segment_sumsq(g, tables, partials, seg, stats, 1.0, 1.0)
    for _ in range(3):
        norm()
    res = {'words': sum(numels), 'buffer_words': n, 'segments': len(names), 'chunks': len(tables.chunks),
           'norm_pass': summary(times_ms(norm, a.launches), 4 * sum(numels))}
    # the gaps of this buffer hold random words too: a pass that read them would be off by gap_share
    inside = sum(float(g[o:o + k].double().square().sum()) for o, k in zip(offs, numels))
    res['total_rel_err'] = abs(float(stats[0]) - inside) / inside
    res['gap_share'] = abs(float(g.double().square().sum()) - inside) / inside
    p, m, v = (torch.zeros(n, device=dev) for _ in range(3))
    sh = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    step = [0]

    def adamw():
        step[0] += 1
        ops.adamw(p, g, m, v, sh, 1e-4, 0.9, 0.999, 1e-8, 0.01, step[0], 1.0)

    def adamw_dev():
        step[0] += 1
        ops.adamw_dev(p, g, m, v, sh, 1e-4, 0.9, 0.999, 1e-8, 0.01, step[0], stats)

    for name, fn in (('adamw', adamw), ('adamw_dev', adamw_dev)):
        for _ in range(3):
            fn()
        res[name] = summary(times_ms(fn, a.launches), 30 * n)     # 4 x fp32 read, 3 x fp32 + 1 x bf16 written
    return res


def step_bench(a):
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    dev = torch.device('cuda')
    B, S = a.batch, 32
    torch.manual_seed(17)
    model = stable_diffusion_2(model_name='stabilityai/stable-diffusion-2-base', pretrained=False, precomputed_latents=True,
                               fsdp=False, seed=17)
    opt = FusedAdamW(lr=1e-4, weight_decay=0.01, unet=model.unet)
    tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration='1ba', device_train_microbatch_size=B)
    g = torch.Generator().manual_seed(1000)
    batch = {'image_latents': torch.randn(B, 4, S, S, generator=g).half().to(dev),
             'caption_latents': torch.randn(B, 77, 1024, generator=g).half().to(dev)}

    def run(clip, steps):
        opt.clip_max_norm, opt.guard_nonfinite = (1.0, True) if clip else (None, False)
        tr.train_batch(batch)
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
        for clip in (False, True):
            ts[clip].append(run(clip, a.steps))
    base, clipped = statistics.median(ts[False]), statistics.median(ts[True])
    return {'batch': B, 'latent': S, 'rounds': a.rounds, 'steps_per_round': a.steps,
            'step_ms_without': round(base, 3), 'step_ms_with_clipping': round(clipped, 3),
            'difference_ms': round(clipped - base, 3), 'without_all': [round(t, 3) for t in ts[False]],
            'with_all': [round(t, 3) for t in ts[True]], 'skipped_steps': opt.last_grad_stats()['skipped_steps']}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--steps', type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(step_bench(a) if a.step else kernel_bench(a)))
