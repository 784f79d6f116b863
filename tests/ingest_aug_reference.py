"""float64 restatement of the augmenting image ingest (``da_image_ingest_aug``): the cover-resize of
tests/ingest_rect_reference.py with the crop origin given per image and an optional horizontal mirror, for
tests/test_image_ingest_aug_gpu.py.  Filter, geometry, seeded images and bf16 rounding
are the ones of the two files it sits next to."""
import numpy as np

from ingest_reference import axis_matrix, rne_bf16_bits, seeded_image  # noqa: F401  (re-exported for the tests)
from ingest_rect_reference import geometry  # noqa: F401

# sources (h, w), none above 70 px, packed in this order.  Against the two targets below: (21, 24) has one row of slack at
# (20, 24); (20, 25) resizes to an odd width with one column of slack; (37, 70) to an odd width (37) with more; (40, 1) is
# one pixel wide; (17, 31) and (9, 23) hold an odd number of bytes, so the images after them begin at odd offsets
SOURCES = [(21, 24), (17, 31), (20, 25), (37, 70), (9, 23), (70, 37), (64, 64), (40, 1), (53, 37), (33, 66)]
# neither side a multiple of the 16-pixel tile; 2 x 2 and 2 x 3 blocks per image
TARGETS = [(20, 24), (17, 33)]


def aug_f64(img, Rh, Rw, top, left, flip):
    """uint8 [h, w, 3] -> float64 [3, Rh, Rw]: resize to cover, mirror the resized image's columns when ``flip``, take the
    window at (top, left), v / 127.5 - 1"""
    h, w = img.shape[:2]
    nw, nh, _, _ = geometry(w, h, Rh, Rw)
    assert 0 <= top <= nh - Rh and 0 <= left <= nw - Rw and flip in (0, 1)
    my = axis_matrix(h, nh)[top:top + Rh]
    mx = axis_matrix(w, nw)
    if flip:
        mx = mx[::-1]   # resized column nw - 1 - c in place of c
    mx = mx[left:left + Rw]
    return np.einsum('yv,vuc,xu->cyx', my, img.astype(np.float64), mx) / 127.5 - 1.0
