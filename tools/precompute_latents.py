"""Precompute VAE latents and text-encoder states for an MDS directory of raw images: the counterpart of the reference's
scripts/precompute_latents.py:220-340 on the HIP kernels, without ``streaming``, ``wandb`` or any fetch.

  python tools/precompute_latents.py --in DIR --out DIR [--resolutions 256 512] [--batch-size 64] [--model DIR|tiny]
                                     [--seed 17] [--caption-drop-prob 0.1] [--num-workers 8]
                                     [--aspect-buckets R [--bucket-step 64] [--bucket-min R/2] [--bucket-max 2R]]

Reads the ``jpg`` and ``caption`` columns of ``--in`` (datasets/mds.py) and writes to ``--out`` every input column
unchanged plus ``caption_latents`` and ``latents_{R}`` for each resolution (fp16 bytes, the columns of
precompute_latents.py:269-271 that ``MDSLatentDataset`` trains from).  Per batch: the workers decode, the packed uint8
pixels are uploaded ONCE, one ``ops.image_ingest`` per resolution reads that same upload (LargestCenterSquare + ToTensor +
Normalize on the device), ``VAEEncoderHIP`` -> ``latent_dist.sample() * 0.18215``, ``TextEncoderHIP`` on the tokenised
caption (dropped to '' with ``--caption-drop-prob``, reference :234).  A sample whose decoded image is smaller than R on its
shorter side gets ``b''`` for ``latents_{R}`` (reference :303-306).

``--aspect-buckets R`` adds two columns for aspect-ratio bucketed training (datasets/buckets.py) and changes
none of the others: ``latents_ar{R}``, the fp16 bytes ``[4, Rh/8, Rw/8]`` of the image encoded at its bucket ``(Rh, Rw)``
of ``bucket_table(R, step, min, max)`` (assigned from the decoded size; resized to cover the bucket and centre-cropped by
``ops.image_ingest_rect``, smaller images are upscaled), and ``latents_ar{R}_hw``, two int32 ``Rh, Rw``.  Per batch the
images of one bucket are ingested and encoded together, the buckets in table order; their latent samples come from a
generator of their own, so the square columns are the same bytes with and without the flag.

``--model tiny`` is a seeded random-init VAE and a 128-wide text encoder (throughput runs and tests); a directory is a local
Stable Diffusion checkpoint (``vae/``, ``text_encoder/``, ``tokenizer/``).  Randomness: one device generator seeded with
``--seed`` draws the latent samples batch by batch, resolution by resolution in the order given; one host generator with
the same seed decides the caption drops.  Prints one JSON line: images, seconds, images/s and the decode / ingest / encode /
write split (host clock, each phase closed by a device synchronise)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LATENT_SCALE = 0.18215


class _DecodeDataset:
    """index -> decoded pixels (the DataLoader workers' share of the work)"""

    def __init__(self, directory):
        self.directory, self.mds = directory, None

    def __len__(self):
        from diffusion_amd.datasets.mds import MDSDirectory
        return len(MDSDirectory(self.directory))

    def __getitem__(self, i):
        import torch
        from diffusion_amd.datasets.image_ingest import decode_rgb
        from diffusion_amd.datasets.mds import MDSDirectory
        if self.mds is None:
            self.mds = MDSDirectory(self.directory)
        return {'index': i, 'image_u8': torch.from_numpy(decode_rgb(self.mds.get(i, columns=('jpg',))['jpg']))}


def build_encoders(model: str = 'tiny', seed: int = 17):
    """``(VAEEncoderHIP, TextEncoderHIP, tokenizer)`` for ``--model``."""
    import torch
    from diffusion_amd.models.text import build_text_encoder, build_tokenizer
    from diffusion_amd.models.text_hip import TextEncoderHIP
    from diffusion_amd.models.vae import AutoencoderKL
    from diffusion_amd.models.vae_hip import VAEEncoderHIP
    torch.manual_seed(seed)
    vae = AutoencoderKL()
    if model == 'tiny':
        text = build_text_encoder(None, torch.float32, hidden_size=128)
        tok = build_tokenizer(None)
    elif os.path.isdir(model):
        from diffusion_amd.models.models import load_local_vae_weights
        load_local_vae_weights(vae, model)
        text = build_text_encoder(os.path.join(model, 'text_encoder'), torch.float32)
        tok = build_tokenizer(os.path.join(model, 'tokenizer'))
    else:
        raise ValueError(f'--model {model!r}: "tiny" or a local checkpoint directory')
    return VAEEncoderHIP(vae.to('cuda').eval()), TextEncoderHIP(text.to('cuda').eval()), tok


def precompute(in_dir, out_dir, resolutions=(256, 512), batch_size=64, model='tiny', seed=17, caption_drop_prob=0.1,
               num_workers=0, encoders=None, samples_per_shard=1 << 30, size_limit=256 << 20, aspect_buckets=None,
               bucket_step=64, bucket_min=None, bucket_max=None):
    """Convert ``in_dir`` to ``out_dir``; returns the dict the CLI prints.  ``encoders = (vae_hip, text_hip, tokenizer)``
    replaces the ones ``model`` would build.  ``aspect_buckets``: the resolution R of the bucketed columns, or None;
    ``resolutions`` may then be empty."""
    import numpy as np
    import torch
    from torch.utils.data import DataLoader
    from diffusion_amd import ops
    from diffusion_amd.datasets.image_ingest import collate_raw_images
    from diffusion_amd.datasets.mds import MDSDirectory, MDSWriter
    from diffusion_amd.models.vae import DiagonalGaussian
    if not torch.cuda.is_available():
        raise RuntimeError('precompute_latents: an MI355X is required (the encoders have no CPU path)')
    resolutions = [int(r) for r in resolutions]
    table = None
    if aspect_buckets is not None:
        from diffusion_amd.datasets.buckets import assign_bucket, bucket_table
        aspect_buckets = int(aspect_buckets)
        table = bucket_table(aspect_buckets, int(bucket_step), bucket_min, bucket_max)
    if (not resolutions and table is None) or any(r < 8 or r % 8 or r > 4096 for r in resolutions):
        raise ValueError(f'resolutions must be multiples of 8 in 8..4096, got {resolutions}')
    with open(os.path.join(in_dir, 'index.json')) as f:
        shards = json.load(f)['shards']
    if not shards:
        raise ValueError(f'{in_dir}: no shards')
    columns = dict(zip(shards[0]['column_names'], shards[0]['column_encodings']))
    if any(dict(zip(s['column_names'], s['column_encodings'])) != columns for s in shards):
        raise ValueError(f'{in_dir}: the shards do not share one column table')
    if 'jpg' not in columns or 'caption' not in columns:
        raise ValueError(f'{in_dir}: needs the columns jpg and caption, has {sorted(columns)}')
    new_cols = ['caption_latents'] + [f'latents_{r}' for r in resolutions]
    ar_col = f'latents_ar{aspect_buckets}'
    if table is not None:
        new_cols += [ar_col, ar_col + '_hw']
    clash = [c for c in new_cols if c in columns]
    if clash:
        raise ValueError(f'{in_dir} already has {clash}')
    vae_hip, text_hip, tok = encoders if encoders is not None else build_encoders(model, seed)
    dev = torch.device('cuda')
    gen = torch.Generator(device=dev).manual_seed(seed)
    drop_gen = torch.Generator().manual_seed(seed)
    ar_gen = torch.Generator(device=dev).manual_seed(seed + 1)   # the bucketed latents' own stream: see the module docstring
    mds = MDSDirectory(in_dir)
    writer = MDSWriter(out_dir, dict(columns, **{c: 'bytes' for c in new_cols}), samples_per_shard, size_limit)
    loader = DataLoader(_DecodeDataset(in_dir), batch_size=batch_size, shuffle=False, drop_last=False,
                        num_workers=num_workers, collate_fn=collate_raw_images(pin_memory=num_workers == 0))
    t = {'decode': 0.0, 'ingest': 0.0, 'encode': 0.0, 'write': 0.0}
    n_images = 0
    t_start = t0 = time.perf_counter()

    def lap(key):
        nonlocal t0
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        t[key] += t1 - t0
        t0 = t1

    for batch in loader:
        lap('decode')
        off, hw = batch['image_off'], batch['image_hw']
        B = off.numel()
        d_raw, d_off, d_hw = (batch[k].to(dev, non_blocking=True) for k in ('image_raw', 'image_off', 'image_hw'))
        xs = []
        for R in resolutions:   # every resolution off the same upload
            x = torch.empty(B * R * R, 8, device=dev, dtype=torch.bfloat16)
            ops.image_ingest(d_raw, d_off, d_hw, R, x, 0, host=(off, hw))
            xs.append(x)
        groups = []   # (bucket, indices into the batch, ingested pixels), buckets in table order
        if table is not None:
            which = [assign_bucket(int(w), int(h), table) for h, w in hw.tolist()]
            for bi in sorted(set(which)):
                idx = torch.tensor([i for i, b in enumerate(which) if b == bi], dtype=torch.int64)
                Rh, Rw = table[bi]
                g_off, g_hw = off[idx].contiguous(), hw[idx].contiguous()
                x = torch.empty(len(idx) * Rh * Rw, 8, device=dev, dtype=torch.bfloat16)
                ops.image_ingest_rect(d_raw, g_off.to(dev), g_hw.to(dev), Rh, Rw, x, 0, host=(g_off, g_hw))
                groups.append((bi, idx.tolist(), x))
        lap('ingest')
        samples = [mds.get(int(i)) for i in batch['index']]
        latents = []
        with torch.no_grad():
            for R, x in zip(resolutions, xs):
                z = DiagonalGaussian(vae_hip.moments_nhwc8(x, B, R, R)).sample(generator=gen) * LATENT_SCALE
                latents.append(z.half().cpu().numpy())
            ar = [None] * B
            for bi, idx, x in groups:
                Rh, Rw = table[bi]
                z = DiagonalGaussian(vae_hip.moments_nhwc8(x, len(idx), Rh, Rw)).sample(generator=ar_gen) * LATENT_SCALE
                z = z.half().cpu().numpy()
                for j, i in enumerate(idx):
                    ar[i] = (np.ascontiguousarray(z[j]).tobytes(), np.array([Rh, Rw], np.int32).tobytes())
            del xs, groups
            caps = ['' if torch.rand(1, generator=drop_gen) < caption_drop_prob else s['caption'] for s in samples]
            ids = torch.tensor([tok(c, padding='max_length', max_length=tok.model_max_length, truncation=True)['input_ids']
                                for c in caps])
            cond = text_hip(ids)[0].half().cpu().numpy()
        lap('encode')
        for i, smp in enumerate(samples):
            short = int(hw[i].min())
            smp['caption_latents'] = np.ascontiguousarray(cond[i]).tobytes()
            for R, z in zip(resolutions, latents):
                smp[f'latents_{R}'] = np.ascontiguousarray(z[i]).tobytes() if short >= R else b''
            if table is not None:
                smp[ar_col], smp[ar_col + '_hw'] = ar[i]
            writer.write(smp)
        n_images += B
        lap('write')
    writer.finish()
    lap('write')
    sec = time.perf_counter() - t_start
    return {'tool': 'precompute_latents', 'images': n_images, 'seconds': round(sec, 3),
            'images_per_s': round(n_images / sec, 1) if sec > 0 else None, 'resolutions': resolutions,
            'batch_size': batch_size, 'num_workers': num_workers, **{f'{k}_s': round(v, 3) for k, v in t.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--in', dest='in_dir', required=True)
    ap.add_argument('--out', dest='out_dir', required=True)
    ap.add_argument('--resolutions', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--batch-size', type=int, default=64)
    ap.add_argument('--model', default='tiny', help='"tiny" (seeded random weights) or a local checkpoint directory')
    ap.add_argument('--seed', type=int, default=17)
    ap.add_argument('--caption-drop-prob', type=float, default=0.1)
    ap.add_argument('--num-workers', type=int, default=8)
    ap.add_argument('--aspect-buckets', type=int, default=None, metavar='R',
                    help='also write latents_ar{R} / latents_ar{R}_hw: every image encoded at its bucket of bucket_table(R)')
    ap.add_argument('--bucket-step', type=int, default=64)
    ap.add_argument('--bucket-min', type=int, default=None, help='smallest bucket side (default R // 2)')
    ap.add_argument('--bucket-max', type=int, default=None, help='largest bucket side (default 2 * R)')
    a = ap.parse_args()
    print(json.dumps(precompute(a.in_dir, a.out_dir, a.resolutions, a.batch_size, a.model, a.seed, a.caption_drop_prob,
                                a.num_workers, aspect_buckets=a.aspect_buckets, bucket_step=a.bucket_step,
                               bucket_min=a.bucket_min, bucket_max=a.bucket_max)), flush=True)


if __name__ == '__main__':
    main()
