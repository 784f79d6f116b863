"""float64 restatement of the rectangular image ingest (resize to cover Rh x Rw, centre crop, ToTensor, Normalize(0.5, 0.5))
and the PIL pipeline it restates, shared by tests/test_rect_host.py and tests/test_image_ingest_rect_gpu.py.  The filter,
the seeded images and the bf16 rounding are those of tests/ingest_reference.py; only the geometry is new."""
from fractions import Fraction

import numpy as np

from ingest_reference import axis_matrix, rne_bf16_bits, seeded_image  # noqa: F401  (re-exported for the tests)

# the kernel cases: source (h, w) -> target (Rh, Rw).  (64, 64) -> (16, 24) has a partial tile in x; (1000, 333) 21 taps per
# axis; the last two a 1-pixel-high and a 1-pixel-wide source
RECT_CASES = [((16, 32), (16, 32)), ((9, 23), (16, 32)), ((37, 53), (16, 32)), ((53, 37), (32, 16)), ((64, 64), (16, 24)),
              ((17, 31), (16, 32)), ((1000, 333), (32, 48)), ((1, 40), (8, 16)), ((40, 1), (8, 16))]


def geometry(w, h, Rh, Rw):
    """written independently of diffusion_amd.datasets.image_ingest.ingest_geometry: the larger of the two exact scale
    factors Rw / w and Rh / h covers the target (a tie goes to the width); Python's round() is half-to-even"""
    sx, sy = Fraction(Rw, w), Fraction(Rh, h)
    if sx >= sy:
        nw, nh = Rw, int(sx * h)      # floor of a positive rational
    else:
        nw, nh = int(sy * w), Rh
    return nw, nh, int(round((nh - Rh) / 2.0)), int(round((nw - Rw) / 2.0))


def ingest_f64(img, Rh, Rw):
    """uint8 [h, w, 3] -> float64 [3, Rh, Rw]"""
    h, w = img.shape[:2]
    nw, nh, top, left = geometry(w, h, Rh, Rw)
    my = axis_matrix(h, nh)[top:top + Rh]
    mx = axis_matrix(w, nw)[left:left + Rw]
    out = np.einsum('yv,vuc,xu->cyx', my, img.astype(np.float64), mx)
    return out / 127.5 - 1.0


def ingest_pil(img, Rh, Rw):
    """the pipeline on PIL: resize to (nw, nh) (antialiased bilinear), centre crop Rh x Rw, / 255, (x - 0.5) / 0.5"""
    from PIL import Image
    h, w = img.shape[:2]
    nw, nh, top, left = geometry(w, h, Rh, Rw)
    pil = Image.fromarray(img).resize((nw, nh), Image.BILINEAR)
    assert pil.size == (nw, nh)
    pil = pil.crop((left, top, left + Rw, top + Rh))
    arr = np.asarray(pil, dtype=np.float64) / 255.0
    return ((arr - 0.5) / 0.5).transpose(2, 0, 1)
