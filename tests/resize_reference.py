"""float64 restatement of ``da_image_resize`` (geometry x filter x range), shared by tests/test_coco_host.py,
tests/test_image_resize_gpu.py and tests/test_coco_eval_gpu.py.

Per axis n_in -> n_out a [n_out, n_in] weight matrix, the image by ``einsum``:
  filter 0  the antialiased triangle filter (Pillow's; ``F.interpolate(mode='bilinear', antialias=True)``): scale = n_in / n_out,
            fs = max(scale, 1), centre c = (i + 0.5) scale, taps x in [max(int(c - fs + 0.5), 0), min(int(c + fs + 0.5), n_in))
            weighing max(0, 1 - |(x - c + 0.5) / fs|), divided by their sum;
  filter 1  two taps (``F.interpolate(mode='bilinear', align_corners=False, antialias=False)``): num = max((2i + 1) n_in - n_out, 0),
            i0 = num // (2 n_out), r = num - 2 n_out i0, i1 = min(i0 + 1, n_in - 1), weights (2 n_out - r) / (2 n_out) on i0 and
            r / (2 n_out) on i1.
geometry 0 takes the resized extent and the crop from ``ingest_geometry`` (resize to cover, centre crop), geometry 1 stretches
each axis to the target.  range 0 is v / 127.5 - 1, range 1 is v / 255."""
import numpy as np

# (h, w) -> (Rh, Rw): the kernel cases
CASES = [((16, 16), (16, 16)), ((7, 5), (16, 16)), ((40, 23), (16, 16)), ((5, 61), (17, 33)), ((1, 1), (16, 16)),
         ((1, 9), (4, 20)), ((130, 97), (32, 16)), ((16, 16), (37, 5)), ((400, 7), (16, 16)), ((7, 400), (16, 16)),
         ((2, 3), (1, 1)), ((64, 64), (1, 70))]
CONSTANT_LEVELS = (0, 1, 128, 255)


def antialias_matrix(n_in, n_out):
    scale = n_in / n_out
    fs = max(scale, 1.0)
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo, hi = max(int(c - fs + 0.5), 0), min(int(c + fs + 0.5), n_in)
        x = np.arange(lo, hi, dtype=np.float64)
        wgt = np.maximum(0.0, 1.0 - np.abs((x - c + 0.5) / fs))
        m[i, lo:hi] = wgt / wgt.sum()
    return m


def two_tap_matrix(n_in, n_out):
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        num = max((2 * i + 1) * n_in - n_out, 0)
        i0 = num // (2 * n_out)
        r = num - i0 * 2 * n_out
        i1 = min(i0 + 1, n_in - 1)
        m[i, i0] += (2 * n_out - r) / (2.0 * n_out)
        m[i, i1] += r / (2.0 * n_out)
    return m


def axis_matrix(n_in, n_out, filter):
    return (antialias_matrix, two_tap_matrix)[filter](n_in, n_out)


def resize_f64(img, Rh, Rw, geometry, filter, range_):
    """uint8 [h, w, 3] -> float64 [3, Rh, Rw]"""
    from diffusion_amd.datasets.image_ingest import ingest_geometry
    h, w = img.shape[:2]
    if geometry == 0:
        nw, nh, top, left = ingest_geometry(w, h, (Rh, Rw))
    else:
        nw, nh, top, left = Rw, Rh, 0, 0
    my = axis_matrix(h, nh, filter)[top:top + Rh]
    mx = axis_matrix(w, nw, filter)[left:left + Rw]
    out = np.einsum('yv,vuc,xu->cyx', my, img.astype(np.float64), mx)
    return out / 255.0 if range_ else out / 127.5 - 1.0


def seeded_image(h, w, seed):
    """structured content (a coarse random grid, upsampled) plus noise: neither constant nor white noise"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (h // 4 + 1, w // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:h, :w]
    return (coarse + rng.integers(-30, 31, (h, w, 3))).clip(0, 255).astype(np.uint8)


def rne_bf16_bits(x32):
    """fp32 ndarray -> the uint16 bit patterns of its round-to-nearest-even bfloat16 (finite inputs)"""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
