"""Host side of ``da_clip_preprocess``: the resize geometry of transformers' ``CLIPImageProcessor`` and Pillow's 8-bit
bicubic tap weights as integer tables.

Pillow resamples ``uint8`` images with 22-bit fixed-point weights (``PRECISION_BITS = 32 - 8 - 2``), one axis at a time.
The tables below are built with the same float64 operations in the same order as its ``precompute_coeffs`` /
``normalize_coeffs_8bpc``, so the kernel, which only multiplies, adds, shifts and clamps integers, reproduces Pillow's levels.
"""
from __future__ import annotations

import functools
from typing import Tuple

import numpy as np

PRECISION_BITS = 22


def resize_geometry(H: int, W: int, R: int) -> Tuple[int, int, int, int]:
    """(new_h, new_w, top, left): the shorter side becomes R, the longer one ``int(R * long / short)``, then the centre
    crop to R x R starts at ``(n - R) // 2`` (transformers' ``get_resize_output_image_size`` / ``center_crop``)."""
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(R * long / short)
    new_h, new_w = (new_long, R) if W <= H else (R, new_long)
    return new_h, new_w, (new_h - R) // 2, (new_w - R) // 2


def _cubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=64)
def bicubic_table(n_in: int, n_out: int, R: int) -> np.ndarray:
    """int32 [R, 2 + taps]: row j = (lo, count, k[0..count)) for index ``(n_out - R) // 2 + j`` of the axis resized from
    ``n_in`` to ``n_out`` samples; unused tail entries are 0.  ``n_in == n_out`` gives the identity rows (j, 1, 2**22).
    Read-only (the array is cached)."""
    if n_in < 1 or n_out < R or R < 1:
        raise ValueError(f'bicubic_table: n_in {n_in}, n_out {n_out}, R {R}')
    first = (n_out - R) // 2
    rows = []
    if n_in == n_out:   # Pillow skips the pass; the same levels come out of one tap of weight 1
        rows = [(first + j, [1 << PRECISION_BITS]) for j in range(R)]
    else:
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = 2.0 * fs
        ss = 1.0 / fs
        for i in range(first, first + R):
            c = (i + 0.5) * scale
            lo = max(int(c - support + 0.5), 0)
            hi = min(int(c + support + 0.5), n_in)
            w = [_cubic((x + lo - c + 0.5) * ss) for x in range(hi - lo)]
            ww = 0.0
            for v in w:
                ww += v
            if ww != 0.0:
                w = [v / ww for v in w]
            rows.append((lo, [int((-0.5 if v < 0 else 0.5) + v * (1 << PRECISION_BITS)) for v in w]))
    taps = max(len(k) for _, k in rows)
    tab = np.zeros((R, 2 + taps), dtype=np.int32)
    for j, (lo, k) in enumerate(rows):
        tab[j, 0], tab[j, 1] = lo, len(k)
        tab[j, 2:2 + len(k)] = k
    tab.setflags(write=False)
    return tab


def tables_for(H: int, W: int, R: int) -> Tuple[np.ndarray, np.ndarray]:
    """(xtab, ytab) of one image size: columns W -> new_w, rows H -> new_h, each cropped to R."""
    new_h, new_w, _, _ = resize_geometry(H, W, R)
    return bicubic_table(W, new_w, R), bicubic_table(H, new_h, R)
