"""CPU-only tests of the raw-image ingest's host half (diffusion_amd/datasets/image_ingest.py): the resize / crop geometry
against known answers and PIL, the float64 restatement of the filter (tests/ingest_reference.py) against the PIL pipeline,
the packing collate, and the dataloader's choice of dataset for a raw-image MDS directory."""
import io
import os

import numpy as np
import pytest
import torch

import ingest_reference as IR
from diffusion_amd.datasets.image_ingest import (MDSImageDataset, collate_raw_images, decode_rgb, ingest_geometry,
                                                 pack_images)

KNOWN = [  # (w, h, R) -> (nw, nh, top, left)
    ((427, 640, 256), (256, 383, 64, 0)),
    ((16, 17, 16), (16, 17, 0, 0)),
    ((19, 16, 16), (19, 16, 0, 2)),
    ((23, 9, 16), (40, 16, 0, 12)),
    ((53, 37, 16), (22, 16, 0, 3)),
]


def _png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format='PNG')
    return buf.getvalue()


@pytest.mark.parametrize('args,want', KNOWN)
def test_geometry_known_answers(args, want):
    assert ingest_geometry(*args) == want
    assert IR.geometry(*args) == want


def test_geometry_matches_pil_on_a_seeded_table():
    """>= 200 seeded (w, h, R): the integer rule equals floor(R*long/short) with Python's half-even round of the crop
    origin, PIL's resize to that target has that size and its crop box is R x R; both half-even cases occur (d odd with
    q = d // 2 even, and with q odd)."""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(17)
    table = [(int(rng.integers(1, 90)), int(rng.integers(1, 90)), int(rng.choice([1, 7, 8, 16, 24, 33]))) for _ in range(240)]
    table += [(16, 17, 16), (16, 19, 16), (19, 16, 16), (16, 23, 16)]   # d = 1 (q = 0), d = 3 (q = 1), d = 7 (q = 3)
    seen = set()
    for w, h, R in table:
        nw, nh, top, left = ingest_geometry(w, h, R)
        assert (nw, nh, top, left) == IR.geometry(w, h, R), (w, h, R)
        assert min(nw, nh) == R and max(nw, nh) == (R * max(w, h)) // min(w, h)
        img = Image.new('RGB', (w, h)).resize((nw, nh), Image.BILINEAR)
        assert img.size == (nw, nh)
        assert img.crop((left, top, left + R, top + R)).size == (R, R)
        assert 0 <= top <= nh - R and 0 <= left <= nw - R
        d = max(nw, nh) - R
        if d % 2:
            seen.add((d // 2) % 2)
            assert max(top, left) == d // 2 + ((d // 2) & 1)
        else:
            assert max(top, left) == d // 2
    assert seen == {0, 1}
    with pytest.raises(ValueError):
        ingest_geometry(0, 5, 16)


def test_f64_restatement_within_one_step_of_pil():
    """The float64 filter against PIL's own pipeline on the kernel test's shapes: PIL rounds to uint8 after each pass
    (0.5 + 0.5 steps) and holds its coefficients in 22 bits, so the bound is 1.01 steps of 2/255."""
    pytest.importorskip('PIL.Image')
    cases = [(hw, 16) for hw in IR.KERNEL_CASES_R16] + [(hw, 24) for hw in IR.KERNEL_CASES_R16] + [IR.CASE_21_TAPS, IR.CASE_ONE_ROW]
    worst = 0.0
    for k, ((h, w), R) in enumerate(cases):
        img = IR.seeded_image(h, w, 100 + k)
        d = np.abs(IR.ingest_f64(img, R) - IR.ingest_pil(img, R)).max() * 127.5
        print(f'{h}x{w} -> {R}: {d:.4f} uint8 steps')
        worst = max(worst, d)
        assert d <= 1.01, ((h, w), R, d)
    assert worst > 0.1   # the comparison is not vacuous: the uint8 roundings are there
    # identity: a 16x16 source at R = 16 is the source itself
    img = IR.seeded_image(16, 16, 5)
    assert np.array_equal(IR.ingest_f64(img, 16), img.astype(np.float64).transpose(2, 0, 1) / 127.5 - 1.0)
    # 21 taps per axis for 1000 -> 32, 2 for an upscale
    assert (IR.axis_matrix(1000, 96)[40] > 0).sum() == 21 and (IR.axis_matrix(9, 16)[5] > 0).sum() == 2


def test_collate_packs_bytes_offsets_and_sizes():
    rng = np.random.default_rng(3)
    shapes = [(5, 3), (4, 7), (1, 1)]   # 45 bytes -> the second image starts at an odd offset, 45 + 84 = 129 -> so does the third
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in shapes]
    samples = [{'image_u8': im, 'captions': torch.full((77,), i, dtype=torch.int64)} for i, im in enumerate(imgs)]
    batch = collate_raw_images(image_size=32)(samples)
    assert set(batch) == {'image_raw', 'image_off', 'image_hw', 'image_size', 'captions'}
    assert batch['image_raw'].dtype == torch.uint8 and batch['image_raw'].shape == (45 + 84 + 3,)
    assert batch['image_off'].dtype == torch.int64 and batch['image_off'].tolist() == [0, 45, 129]
    assert batch['image_hw'].dtype == torch.int32 and batch['image_hw'].tolist() == [[5, 3], [4, 7], [1, 1]]
    assert batch['image_size'] == 32 and batch['captions'].shape == (3, 77) and batch['captions'][2, 0] == 2
    for im, o in zip(imgs, batch['image_off'].tolist()):
        assert torch.equal(batch['image_raw'][o:o + im.numel()], im.reshape(-1))
    assert 'image_size' not in collate_raw_images()(samples)
    with pytest.raises(ValueError):
        pack_images([torch.zeros(4, 4, 4, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        pack_images([torch.zeros(4, 4, 3)])


def test_dataloader_selects_the_image_dataset_for_raw_mds(tmp_path):
    pytest.importorskip('PIL.Image')
    from diffusion_amd.datasets.laion.laion import MDSLatentDataset, build_streaming_laion_dataloader
    from diffusion_amd.datasets.mds import write_mds
    shapes = [(20, 31), (33, 18), (16, 16), (9, 23)]
    imgs = [IR.seeded_image(h, w, 40 + i) for i, (h, w) in enumerate(shapes)]
    raw_dir, lat_dir = str(tmp_path / 'raw'), str(tmp_path / 'lat')
    write_mds(raw_dir, {'jpg': 'bytes', 'caption': 'str', 'width': 'int32'},
              [{'jpg': _png(im), 'caption': f'image {i}', 'width': im.shape[1]} for i, im in enumerate(imgs)])
    s = 256 // 8
    write_mds(lat_dir, {'jpg': 'bytes', 'caption': 'str', 'caption_latents': 'bytes', 'latents_256': 'bytes'},
              [{'jpg': _png(im), 'caption': 'x', 'caption_latents': np.zeros(77 * 8, np.float16).tobytes(),
                'latents_256': np.zeros(4 * s * s, np.float16).tobytes()} for im in imgs])
    assert np.array_equal(decode_rgb(_png(imgs[0])), imgs[0])
    gray = decode_rgb(_png(imgs[0][..., 0]))   # mode 'L' is converted
    assert gray.shape == imgs[0].shape and gray.dtype == np.uint8 and np.array_equal(gray[..., 1], imgs[0][..., 0])

    dl = build_streaming_laion_dataloader(local=raw_dir, batch_size=2, resize_size=256, shuffle=False, drop_last=False)
    parts = dl.dataset.datasets
    assert len(parts) == 1 and isinstance(parts[0], MDSImageDataset)
    smp = parts[0][1]
    assert set(smp) == {'image_u8', 'captions'} and smp['image_u8'].dtype == torch.uint8
    assert np.array_equal(smp['image_u8'].numpy(), imgs[1]) and smp['captions'].dtype == torch.int64 and smp['captions'].shape == (77,)
    batches = list(dl)
    assert len(batches) == 2
    b = batches[0]
    assert set(b) == {'image_raw', 'image_off', 'image_hw', 'image_size', 'captions'}
    assert (b['image_raw'].dtype, b['image_off'].dtype, b['image_hw'].dtype) == (torch.uint8, torch.int64, torch.int32)
    assert b['image_size'] == 256 and b['image_hw'].tolist() == [[20, 31], [33, 18]] and b['captions'].shape == (2, 77)
    assert b['image_off'].tolist() == [0, 20 * 31 * 3] and b['image_raw'].numel() == 3 * (20 * 31 + 33 * 18)
    assert np.array_equal(b['image_raw'][20 * 31 * 3:].numpy().reshape(33, 18, 3), imgs[1])

    # a directory that already works keeps its dataset class and batch dict
    dl2 = build_streaming_laion_dataloader(local=lat_dir, batch_size=2, resize_size=256, shuffle=False)
    assert isinstance(dl2.dataset.datasets[0], MDSLatentDataset)
    assert set(next(iter(dl2))) == {'caption_latents', 'image_latents', 'captions'}
    # jpg present, latents for ANOTHER resolution only: raw images at this one
    dl3 = build_streaming_laion_dataloader(local=lat_dir, batch_size=2, resize_size=512, shuffle=False)
    assert isinstance(dl3.dataset.datasets[0], MDSImageDataset)
    with pytest.raises(ValueError):
        build_streaming_laion_dataloader(local=[raw_dir, lat_dir], batch_size=2, resize_size=256)
