"""float64 restatement of the image ingest (LargestCenterSquare(R) + ToTensor + Normalize(0.5, 0.5)) and the PIL pipeline
it restates, shared by tests/test_image_ingest_host.py and tests/test_image_ingest_gpu.py.

Filter: PIL's antialiased bilinear (triangle) resize, separable.  Per axis n_in -> n_out: scale = n_in / n_out,
fs = max(scale, 1); output i has centre c = (i + 0.5) scale and taps x in [max(int(c - fs + 0.5), 0), min(int(c + fs + 0.5),
n_in)) with weights max(0, 1 - |(x - c + 0.5) / fs|) divided by their sum.  Nothing is rounded to uint8 (PIL does, after each
pass: the two differ by less than one uint8 step)."""
import numpy as np

# the kernel cases of the issue: (h, w) -> R
KERNEL_CASES_R16 = [(16, 16), (9, 23), (37, 53), (53, 37), (17, 16), (16, 19), (64, 64)]
CASE_21_TAPS = ((1000, 333), 32)
CASE_ONE_ROW = ((1, 40), 8)


def geometry(w, h, R):
    """written independently of diffusion_amd.datasets.image_ingest.ingest_geometry: Python's round() is half-to-even"""
    if w <= h:
        nw, nh = R, (R * h) // w
    else:
        nw, nh = (R * w) // h, R
    return nw, nh, int(round((nh - R) / 2.0)), int(round((nw - R) / 2.0))


def axis_matrix(n_in, n_out):
    """[n_out, n_in] float64 resampling matrix of one axis"""
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


def ingest_f64(img, R):
    """uint8 [h, w, 3] -> float64 [3, R, R]"""
    h, w = img.shape[:2]
    nw, nh, top, left = geometry(w, h, R)
    my = axis_matrix(h, nh)[top:top + R]
    mx = axis_matrix(w, nw)[left:left + R]
    out = np.einsum('yv,vuc,xu->cyx', my, img.astype(np.float64), mx)
    return out / 127.5 - 1.0


def ingest_pil(img, R):
    """the reference pipeline on PIL: resize (shorter side -> R, antialiased bilinear), centre crop, /255, (x - 0.5) / 0.5"""
    from PIL import Image
    h, w = img.shape[:2]
    nw, nh, top, left = geometry(w, h, R)
    pil = Image.fromarray(img).resize((nw, nh), Image.BILINEAR)
    assert pil.size == (nw, nh)
    pil = pil.crop((left, top, left + R, top + R))
    arr = np.asarray(pil, dtype=np.float64) / 255.0
    return ((arr - 0.5) / 0.5).transpose(2, 0, 1)


def seeded_image(h, w, seed):
    """structured content (a coarse random grid, upsampled) plus noise: neither constant nor white noise"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (h // 4 + 1, w // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:h, :w]
    return (coarse + rng.integers(-30, 31, (h, w, 3))).clip(0, 255).astype(np.uint8)


def rne_bf16_bits(x32):
    """fp32 ndarray -> the uint16 bit patterns of its round-to-nearest-even bfloat16 (finite inputs)"""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
