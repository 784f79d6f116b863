"""CPU-only tests of the rectangular-image support's host half: ``ingest_geometry`` with an ``(Rh, Rw)`` pair against the
independent restatement of tests/ingest_rect_reference.py, the float64 restatement of the filter against PIL on the kernel
cases, the collate / dataloader with a pair, the U-Net's divisibility rule and the new entry's binding."""
import io

import numpy as np
import pytest
import torch

import ingest_rect_reference as RR
from diffusion_amd.datasets.image_ingest import MDSImageDataset, collate_raw_images, ingest_geometry, target_hw


def _png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format='PNG')
    return buf.getvalue()


def test_geometry_with_a_pair_matches_the_restatement_covers_and_stays_inside():
    sides = [1, 2, 3, 7, 9, 16, 17, 23, 31, 37, 40, 53, 64, 333, 1000]
    targets = [(8, 16), (16, 8), (16, 32), (32, 16), (16, 24), (32, 48), (7, 33), (1, 5), (24, 24), (4096, 1)]
    fit_w = fit_h = 0
    for w in sides:
        for h in sides:
            for Rh, Rw in targets:
                nw, nh, top, left = got = ingest_geometry(w, h, (Rh, Rw))
                assert got == RR.geometry(w, h, Rh, Rw), (w, h, Rh, Rw)
                assert got == ingest_geometry(w, h, [Rh, Rw])
                assert nw >= Rw and nh >= Rh and (nw == Rw or nh == Rh)          # covers, and one axis lands on the target
                assert 0 <= top <= nh - Rh and 0 <= left <= nw - Rw             # the crop window lies inside
                assert abs((nh - Rh - top) - top) <= 1 and abs((nw - Rw - left) - left) <= 1   # ... and is centred
                fit_w += nw == Rw
                fit_h += nh == Rh and nw != Rw
    assert fit_w > 100 and fit_h > 100   # both branches of the rule occur
    # known answers: (w, h, (Rh, Rw)) -> (nw, nh, top, left); the second is a tie of the two scale factors
    assert ingest_geometry(23, 9, (16, 32)) == (40, 16, 0, 4)
    assert ingest_geometry(32, 16, (16, 32)) == (32, 16, 0, 0)
    assert ingest_geometry(37, 53, (32, 16)) == (22, 32, 0, 3)
    assert ingest_geometry(64, 64, (16, 24)) == (24, 24, 4, 0)
    assert ingest_geometry(333, 1000, (32, 48)) == (48, 144, 56, 0)
    for bad in ((0, 8), (8, 0), (8,), (8, 8, 8)):
        with pytest.raises(ValueError):
            ingest_geometry(10, 10, bad)


def test_geometry_pair_equals_the_int_form_on_squares():
    import ingest_reference as IR
    rng = np.random.default_rng(5)
    table = [(int(rng.integers(1, 200)), int(rng.integers(1, 200)), int(rng.choice([1, 7, 8, 16, 24, 33, 256])))
             for _ in range(2000)]
    for w, h, R in table:
        assert ingest_geometry(w, h, (R, R)) == ingest_geometry(w, h, R) == IR.geometry(w, h, R), (w, h, R)
    assert target_hw(16) == (16, 16) and target_hw([8, 24]) == (8, 24) and target_hw((8, 24)) == (8, 24)


def test_f64_restatement_within_one_step_of_pil_on_the_rect_cases():
    """the float64 filter under the rectangular geometry against PIL's own pipeline: below one uint8 step on every kernel
    case, as for the square cases (PIL rounds to uint8 after each pass)"""
    pytest.importorskip('PIL.Image')
    worst = 0.0
    for k, ((h, w), (Rh, Rw)) in enumerate(RR.RECT_CASES):
        img = RR.seeded_image(h, w, 200 + k)
        f64 = RR.ingest_f64(img, Rh, Rw)
        assert f64.shape == (3, Rh, Rw)
        d = np.abs(f64 - RR.ingest_pil(img, Rh, Rw)).max() * 127.5
        print(f'{h}x{w} -> {Rh}x{Rw}: {d:.4f} uint8 steps')
        worst = max(worst, d)
        assert d <= 1.01, ((h, w), (Rh, Rw), d)
    assert worst > 0.1
    img = RR.seeded_image(16, 32, 5)   # identity
    assert np.array_equal(RR.ingest_f64(img, 16, 32), img.astype(np.float64).transpose(2, 0, 1) / 127.5 - 1.0)


def test_dataloader_takes_a_pair_for_raw_directories_only(tmp_path):
    pytest.importorskip('PIL.Image')
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader
    from diffusion_amd.datasets.mds import write_mds
    shapes = [(20, 31), (33, 18), (16, 16), (9, 23)]
    imgs = [RR.seeded_image(h, w, 40 + i) for i, (h, w) in enumerate(shapes)]
    raw_dir, lat_dir, both_dir = str(tmp_path / 'raw'), str(tmp_path / 'lat'), str(tmp_path / 'both')
    write_mds(raw_dir, {'jpg': 'bytes', 'caption': 'str'}, [{'jpg': _png(im), 'caption': f'image {i}'} for i, im in enumerate(imgs)])
    lat = {'caption': 'x', 'caption_latents': np.zeros(77 * 8, np.float16).tobytes(),
           'latents_256': np.zeros(4 * 32 * 32, np.float16).tobytes()}
    write_mds(lat_dir, {'caption': 'str', 'caption_latents': 'bytes', 'latents_256': 'bytes'}, [dict(lat) for _ in imgs])
    write_mds(both_dir, {'jpg': 'bytes', 'caption': 'str', 'caption_latents': 'bytes', 'latents_256': 'bytes'},
              [dict(lat, jpg=_png(im)) for im in imgs])
    dl = build_streaming_laion_dataloader(local=raw_dir, batch_size=2, resize_size=[32, 64], shuffle=False, drop_last=False)
    assert isinstance(dl.dataset.datasets[0], MDSImageDataset)
    b = next(iter(dl))
    assert b['image_size'] == (32, 64) and isinstance(b['image_size'], tuple)
    assert b['image_hw'].tolist() == [[20, 31], [33, 18]] and b['image_raw'].numel() == 3 * (20 * 31 + 33 * 18)
    assert collate_raw_images(image_size=(8, 24)).image_size == (8, 24) and collate_raw_images(image_size=32).image_size == 32
    # no latents column can belong to a rectangular size: a directory with a jpg column is read as raw images
    dl2 = build_streaming_laion_dataloader(local=both_dir, batch_size=2, resize_size=(32, 64), shuffle=False)
    assert isinstance(dl2.dataset.datasets[0], MDSImageDataset) and next(iter(dl2))['image_size'] == (32, 64)
    with pytest.raises(ValueError):   # latents only
        build_streaming_laion_dataloader(local=lat_dir, batch_size=2, resize_size=[32, 64])
    with pytest.raises(ValueError):   # the synthetic dataset
        build_streaming_laion_dataloader(batch_size=2, resize_size=[32, 64])
    with pytest.raises(ValueError):   # a shard directory (no index.json)
        (tmp_path / 'shards').mkdir()
        build_streaming_laion_dataloader(local=str(tmp_path / 'shards'), batch_size=2, resize_size=[32, 64])
    with pytest.raises(ValueError):
        build_streaming_laion_dataloader(local=raw_dir, batch_size=2, resize_size=[32, 64, 3])
    # the int form is what it was
    assert next(iter(build_streaming_laion_dataloader(local=raw_dir, batch_size=2, resize_size=32, shuffle=False)))['image_size'] == 32


def test_new_entry_is_declared_bound_and_exported():
    """the header / SIGNATURES tests of tests/test_abi_and_host.py cover every entry; this names the new one"""
    import os
    import re
    from diffusion_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'diffusion_amd.h')).read()
    m = re.search(r'int da_image_ingest_rect\(([^)]*)\)', src)
    assert m and len(m.group(1).split(',')) == len(_lib.SIGNATURES['da_image_ingest_rect']) == 9
    assert len(_lib.SIGNATURES['da_image_ingest']) == 8   # the square entry keeps its ABI
    assert hasattr(_lib.load(), 'da_image_ingest_rect')


def test_spatial_rule_of_the_unet_walk():
    """H and W are multiples of 2 ** (levels - 1); an int is the square pair (pure host logic, no device)"""
    from diffusion_amd.models.unet import UNetConfig, UNetHIP, spatial_hw
    assert spatial_hw(16) == (16, 16) and spatial_hw((8, 32)) == (8, 32) and spatial_hw(torch.Size([8, 24])) == (8, 24)
    with pytest.raises(ValueError):
        spatial_hw((8, 8, 8))

    class _Cfg:   # check_spatial reads the level count only
        cfg = UNetConfig.tiny()
    for ok in ((8, 8), (8, 32), (32, 8), (8, 24), (64, 96)):
        UNetHIP.check_spatial(_Cfg, *ok)
    for bad in ((8, 12), (12, 8), (4, 8), (8, 0), (20, 20)):
        with pytest.raises(ValueError, match='multiples of 8'):
            UNetHIP.check_spatial(_Cfg, *bad)
