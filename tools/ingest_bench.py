"""The HIP resize-crop ingest (``ops.image_ingest``, csrc/image.hip) against the host path it replaces, and against the VAE
encode that follows it.  Prints one JSON line.

  python tools/ingest_bench.py [--images 64] [--width 640] [--height 480] [--repeats 20] [--workers 16] [--no-vae]

For ``--images`` seeded ``width x height`` RGB sources and R = 256 and 512:
  kernel_ms       median of ``--repeats`` launches after warm-up, device events around each launch (kind 0: bf16 NHWC-8)
  gbytes_per_s    (source bytes inside the crop window's tap range + output bytes) / kernel time - the bytes the transform
                  needs, computed from the shapes, not what the kernel happened to fetch
  host_ms         the reference's transform on the host for the same batch: PIL ``resize`` (antialiased bilinear) + crop +
                  float conversion in ``--workers`` processes (the results come back to the parent, as DataLoader workers'
                  do), median of 5
  upload_fp32_ms  the fp32 [B,3,R,R] batch to the device (pinned source), median of 5; ``upload_u8_ms`` the packed bytes
  vae_encode_ms   ``VAEEncoderHIP.moments_nhwc8`` on the ingested batch (random-init full-size VAE), median of 3

  python tools/ingest_bench.py --geometry {0,1} --filter {0,1} [--images 64] [--width 640] [--height 480] [--repeats 20]

With ``--geometry`` / ``--filter`` (one given: the other is 0) the other forms of the kernel are timed instead
(``ops.image_resize``, range 1, kind 1: the COCO evaluation loader's transforms) against the same transform in torch ops on
the device - ``uint8 -> fp32 / 255 -> F.interpolate(mode='bilinear', align_corners=False, antialias=filter == 0)`` to the
resized extent, then the crop - both by device events, plus the largest difference between the two results.
"""
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


def _host_transform(args):
    arr, R = args
    from PIL import Image
    from diffusion_amd.datasets.image_ingest import ingest_geometry
    h, w = arr.shape[:2]
    nw, nh, top, left = ingest_geometry(w, h, R)
    img = Image.fromarray(arr).resize((nw, nh), Image.BILINEAR).crop((left, top, left + R, top + R))
    return np.ascontiguousarray((np.asarray(img, dtype=np.float32) / 127.5 - 1.0).transpose(2, 0, 1))


def _window(n_in, n_out, first, last):
    """source samples [lo, hi) the output indices first..last of one axis read (the rule of csrc/image.hip)"""
    m2 = 2 * max(n_in, n_out)
    lo = max(((2 * first + 1) * n_in - m2 + n_out) // (2 * n_out), 0)
    hi = min(((2 * last + 1) * n_in + m2 + n_out) // (2 * n_out), n_in)
    return lo, hi


def resize_forms(a):
    """--geometry / --filter: ops.image_resize against F.interpolate on the device"""
    import torch
    import torch.nn.functional as F
    from diffusion_amd import ops
    from diffusion_amd.datasets.image_ingest import ingest_geometry, pack_images
    if not torch.cuda.is_available():
        raise SystemExit('ingest_bench: no GPU')
    dev = torch.device('cuda:0')
    B, w, h, g, f = a.images, a.width, a.height, a.geometry or 0, a.filter or 0
    rng = np.random.default_rng(17)
    base = rng.integers(0, 256, (B, h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8).repeat(8, 1).repeat(8, 2)[:, :h, :w]
    imgs = (base.astype(np.int16) + rng.integers(-20, 21, (B, h, w, 3), dtype=np.int16)).clip(0, 255).astype(np.uint8)
    raw, off, hw = pack_images([torch.from_numpy(im) for im in imgs])
    d_raw, d_off, d_hw = raw.to(dev), off.to(dev), hw.to(dev)
    d_u8 = torch.from_numpy(imgs).to(dev)

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
        return statistics.median(ms), min(ms), max(ms)

    res = {'bench': 'image_resize', 'images': B, 'source': [w, h], 'repeats': a.repeats, 'geometry': g, 'filter': f,
           'range': 1, 'shapes': []}
    for R in (256, 512):
        nw, nh, top, left = (R, R, 0, 0) if g else ingest_geometry(w, h, R)
        out = torch.empty(B, 3, R, R, device=dev)

        def torch_path():
            x = d_u8.permute(0, 3, 1, 2).float() / 255
            x = F.interpolate(x, size=(nh, nw), mode='bilinear', align_corners=False, antialias=f == 0)
            return x[:, :, top:top + R, left:left + R].contiguous()

        med, lo, hi = timed(lambda: ops.image_resize(d_raw, d_off, d_hw, R, R, out, 1, g, f, 1, host=(off, hw)), a.repeats)
        t_med, t_lo, t_hi = timed(torch_path, a.repeats)
        diff = float((out - torch_path()).abs().max())
        res['shapes'].append({'R': R, 'kernel_ms': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                              'torch_ms': round(t_med, 4), 'torch_min_ms': round(t_lo, 4), 'torch_max_ms': round(t_hi, 4),
                              'max_abs_diff_vs_torch': diff})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--no-vae', action='store_true')
    ap.add_argument('--geometry', type=int, choices=(0, 1), default=None, help='0 cover + centre crop, 1 stretch')
    ap.add_argument('--filter', type=int, choices=(0, 1), default=None, help='0 antialiased triangle, 1 two-tap bilinear')
    a = ap.parse_args()
    if a.geometry is not None or a.filter is not None:
        return resize_forms(a)
    B, w, h = a.images, a.width, a.height
    rng = np.random.default_rng(17)
    # smooth seeded content plus noise, so that neither the filter nor a cache sees a constant
    base = rng.integers(0, 256, (B, h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8).repeat(8, 1).repeat(8, 2)[:, :h, :w]
    imgs = (base.astype(np.int16) + rng.integers(-20, 21, (B, h, w, 3), dtype=np.int16)).clip(0, 255).astype(np.uint8)

    # the host path first: its worker pool is forked before this process opens the device
    import multiprocessing as mp
    host = {}
    with mp.get_context('fork').Pool(a.workers) as pool:
        for R in (256, 512):
            pool.map(_host_transform, [(im, R) for im in imgs[:a.workers]])   # warm the workers
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                out = pool.map(_host_transform, [(im, R) for im in imgs])
                ts.append((time.perf_counter() - t0) * 1e3)
            host[R] = (statistics.median(ts), np.stack(out))

    import torch
    from diffusion_amd import ops
    from diffusion_amd.datasets.image_ingest import ingest_geometry, pack_images
    if not torch.cuda.is_available():
        raise SystemExit('ingest_bench: no GPU')
    dev = torch.device('cuda:0')
    raw, off, hw = pack_images([torch.from_numpy(im) for im in imgs], pin_memory=True)

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
        return statistics.median(ms), min(ms), max(ms)

    d_raw = torch.empty_like(raw, device=dev)
    up_u8 = timed(lambda: d_raw.copy_(raw, non_blocking=True), 5)[0]
    d_off, d_hw = off.to(dev), hw.to(dev)
    vae_hip = None
    if not a.no_vae:
        from diffusion_amd.models.vae import AutoencoderKL
        from diffusion_amd.models.vae_hip import VAEEncoderHIP
        torch.manual_seed(7)
        vae_hip = VAEEncoderHIP(AutoencoderKL().to(dev).eval())
    res = {'bench': 'image_ingest', 'images': B, 'source': [w, h], 'repeats': a.repeats, 'workers': a.workers,
           'upload_u8_ms': round(up_u8, 3), 'shapes': []}
    for R in (256, 512):
        nw, nh, top, left = ingest_geometry(w, h, R)
        (y0, y1), (x0, x1) = _window(h, nh, top, top + R - 1), _window(w, nw, left, left + R - 1)
        nbytes = B * (3 * (y1 - y0) * (x1 - x0) + R * R * 16)
        x = torch.empty(B * R * R, 8, device=dev, dtype=torch.bfloat16)
        med, lo, hi = timed(lambda: ops.image_ingest(d_raw, d_off, d_hw, R, x, 0, host=(off, hw)), a.repeats)
        f32 = torch.empty(B, 3, R, R, device=dev)
        ops.image_ingest(d_raw, d_off, d_hw, R, f32, 1, host=(off, hw))
        host_ms, host_out = host[R]
        pinned = torch.from_numpy(host_out).pin_memory()
        up_f32 = timed(lambda: f32.copy_(pinned, non_blocking=True), 5)[0]
        ops.image_ingest(d_raw, d_off, d_hw, R, f32, 1, host=(off, hw))
        diff = float((f32.cpu() - torch.from_numpy(host_out)).abs().max())
        row = {'R': R, 'kernel_ms': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4), 'bytes': nbytes,
               'gbytes_per_s': round(nbytes / med / 1e6, 1), 'host_ms': round(host_ms, 2), 'upload_fp32_ms': round(up_f32, 3),
               'max_abs_diff_vs_pil_in_u8_steps': round(diff * 127.5, 3)}
        if vae_hip is not None:
            row['vae_encode_ms'] = round(timed(lambda: vae_hip.moments_nhwc8(x, B, R, R), 3, warm=1)[0], 2)
        res['shapes'].append(row)
        del x, f32
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
