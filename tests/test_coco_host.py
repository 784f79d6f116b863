"""CPU-only tests of the COCO evaluation route's host half: the targets the reference's YAML names resolve, the float64
restatement of ``da_image_resize`` (tests/resize_reference.py) against ``F.interpolate``, the MDS encodings a COCO directory
uses, and ``build_streaming_cocoval_dataloader`` (captions, batching, the unpadded rank partition, the transform it asks for)."""
import inspect
import json
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_reference as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_the_reference_yaml_eval_dataset_target_resolves_with_the_reference_signature():
    from diffusion_amd import hydra_lite
    cfg = hydra_lite.load_config(os.path.join(GOLDEN, 'reference_SD-2-base-256.yaml'))
    fn = hydra_lite.resolve_target(cfg.dataset.eval_dataset['_target_'])
    assert fn.__name__ == 'build_streaming_cocoval_dataloader'
    params = inspect.signature(fn).parameters
    got = [(n, p.default) for n, p in params.items() if p.kind is not inspect.Parameter.VAR_KEYWORD]
    assert got == [('batch_size', inspect.Parameter.empty), ('remote', inspect.Parameter.empty),
                   ('local', '/tmp/mds-cache/mds-coco-val/'), ('shuffle', False), ('resize_size', 512), ('use_crop', False),
                   ('caption_selection', 'first'), ('num_canonical_nodes', None)]
    assert list(params)[-1] == 'dataloader_kwargs' and params['dataloader_kwargs'].kind is inspect.Parameter.VAR_KEYWORD
    from diffusion_amd.datasets import build_streaming_cocoval_dataloader
    assert build_streaming_cocoval_dataloader is fn


def test_log_diffusion_images_resolves_through_the_prefix_alias():
    from diffusion_amd import hydra_lite
    from diffusion_amd.trainer import Callback
    cls = hydra_lite.resolve_target('diffusion.callbacks.LogDiffusionImages')
    assert cls.__name__ == 'LogDiffusionImages' and issubclass(cls, Callback)
    names = list(inspect.signature(cls.__init__).parameters)[1:]
    assert names == ['prompts', 'size', 'num_inference_steps', 'guidance_scale', 'text_key', 'tokenized_prompts', 'seed']
    cb = cls(prompts=['x'])
    assert (cb.size, cb.num_inference_steps, cb.guidance_scale, cb.text_key, cb.seed) == (256, 50, 0.0, 'captions', 1138)


def test_da_image_resize_is_exported():
    from diffusion_amd import _lib
    assert len(_lib.SIGNATURES['da_image_resize']) == 12
    assert hasattr(_lib.load(), 'da_image_resize')


@pytest.mark.parametrize('antialias', [False, True])
def test_restatement_matches_torch_interpolate(antialias):
    """stretch geometry, range 1, against F.interpolate on uint8 / 255 in fp32: the difference is torch's fp32 weights
    (measured worst 2.2e-6 two-tap at 5x61 -> 17x33, 9.7e-7 antialiased); 1e-5 is the project's bound against float64"""
    worst = 0.0
    for k, ((h, w), (Rh, Rw)) in enumerate(RR.CASES):
        img = RR.seeded_image(h, w, 300 + k)
        x = torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255
        want = F.interpolate(x, size=(Rh, Rw), mode='bilinear', align_corners=False, antialias=antialias)[0]
        got = RR.resize_f64(img, Rh, Rw, 1, 0 if antialias else 1, 1)
        assert got.shape == (3, Rh, Rw)
        d = float(np.abs(got - want.double().numpy()).max())
        print(f'{h}x{w} -> {Rh}x{Rw} antialias={antialias}: {d:.3e}')
        worst = max(worst, d)
        assert d <= 1e-5, ((h, w), (Rh, Rw), d)
    print(f'worst {worst:.3e}')


def test_restatement_at_geometry_0_is_the_ingest_restatement():
    import ingest_rect_reference as IRR
    img = RR.seeded_image(37, 53, 5)
    assert np.array_equal(RR.resize_f64(img, 16, 32, 0, 0, 0), IRR.ingest_f64(img, 16, 32))


# ---------------------------------------------------------------------------------------------- MDS
def _jpeg(img, fmt='JPEG'):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format=fmt)
    return buf.getvalue()


def test_mds_round_trip_of_json_jpeg_and_pil_columns(tmp_path):
    pytest.importorskip('PIL.Image')
    from PIL import Image
    from diffusion_amd.datasets.image_ingest import decode_rgb
    from diffusion_amd.datasets.mds import MDSDirectory, write_mds
    rgb, grey = RR.seeded_image(9, 13, 1), RR.seeded_image(6, 4, 2)[..., 0]
    samples = [{'image': _jpeg(rgb), 'raw': Image.fromarray(rgb), 'captions': ['a "quoted" café', 'second'], 'n': 3},
               {'image': _jpeg(grey), 'raw': Image.fromarray(grey), 'captions': [], 'n': 4}]
    write_mds(str(tmp_path), {'image': 'jpeg', 'raw': 'pil', 'captions': 'json', 'n': 'int'}, samples)
    with open(tmp_path / 'index.json') as f:
        shard = json.load(f)['shards'][0]
    assert shard['column_names'] == ['captions', 'image', 'n', 'raw']
    assert shard['column_encodings'] == ['json', 'jpeg', 'int', 'pil'] and shard['column_sizes'] == [None, None, 8, None]
    mds = MDSDirectory(str(tmp_path))
    a, b = mds.get(0), mds.get(1)
    assert a['captions'] == samples[0]['captions'] and b['captions'] == [] and int(a['n']) == 3
    assert a['image'] == samples[0]['image'] and isinstance(a['image'], bytes)   # handed on undecoded
    assert decode_rgb(b['image']).shape == (6, 4, 3)
    assert a['raw'].dtype == np.uint8 and np.array_equal(a['raw'], rgb)
    assert np.array_equal(b['raw'], np.repeat(grey[..., None], 3, 2))   # mode L converted to RGB


def test_pil_sample_assembled_with_struct(tmp_path):
    """a shard written byte by byte from the layouts of the module header: uint32 width, height, len(mode) | mode | tobytes()"""
    pytest.importorskip('PIL.Image')
    from diffusion_amd.datasets.mds import MDSDirectory
    img = RR.seeded_image(3, 5, 9)
    pil = struct.pack('<III', 5, 3, 3) + b'RGB' + img.tobytes()
    caps = json.dumps(['one', 'two']).encode()
    blob = struct.pack('<II', len(caps), len(pil)) + caps + pil     # columns sorted by name: captions, image
    head = 4 + 4 * 2
    with open(tmp_path / 'shard.00000.mds', 'wb') as f:
        f.write(struct.pack('<III', 1, head, head + len(blob)) + blob)
    with open(tmp_path / 'index.json', 'w') as f:
        json.dump({'version': 2, 'shards': [{'column_names': ['captions', 'image'], 'column_encodings': ['json', 'pil'],
                                             'column_sizes': [None, None], 'samples': 1, 'compression': None, 'format': 'mds',
                                             'raw_data': {'basename': 'shard.00000.mds'}}]}, f)
    smp = MDSDirectory(str(tmp_path)).get(0)
    assert smp['captions'] == ['one', 'two'] and np.array_equal(smp['image'], img)


# ---------------------------------------------------------------------------------------------- the loader
N_SAMPLES = 5


@pytest.fixture(scope='module')
def coco_dir(tmp_path_factory):
    pytest.importorskip('PIL.Image')
    from diffusion_amd.datasets.mds import write_mds
    d = tmp_path_factory.mktemp('coco')
    samples = [{'image': _jpeg(RR.seeded_image(10 + 3 * i, 8 + 5 * i, i)), 'captions': [f'first of {i}', f'second of {i}']}
               for i in range(N_SAMPLES)]
    write_mds(str(d), {'image': 'jpeg', 'captions': 'json'}, samples, samples_per_shard=2)
    return str(d)


def _build(coco_dir, **kw):
    from diffusion_amd.datasets import build_streaming_cocoval_dataloader
    kw.setdefault('batch_size', 2)
    kw.setdefault('resize_size', 16)
    return build_streaming_cocoval_dataloader(remote=None, local=coco_dir, num_workers=0, **kw)


def _ids(text):
    from diffusion_amd.models.text import build_tokenizer
    return build_tokenizer(None)(text, padding='max_length', max_length=77, truncation=True)['input_ids']


def test_first_and_random_caption_selection(coco_dir):
    ds = _build(coco_dir).dataset
    assert len(ds) == N_SAMPLES
    for i in range(N_SAMPLES):
        smp = ds[i]
        assert smp['captions'].dtype == torch.int64 and smp['captions'].tolist() == _ids(f'first of {i}')
        assert smp['image_u8'].dtype == torch.uint8 and tuple(smp['image_u8'].shape) == (10 + 3 * i, 8 + 5 * i, 3)
    ds = _build(coco_dir, caption_selection='RANDOM').dataset   # checked once, on the lower-cased value
    both = [_ids('first of 1'), _ids('second of 1')]
    seen = {both.index(ds[1]['captions'].tolist()) for _ in range(40)}   # 2 ** -39 to miss one of the two
    assert seen == {0, 1}
    for bad in ('last', 'First one', ''):
        with pytest.raises(ValueError, match='caption selection'):
            _build(coco_dir, caption_selection=bad)


def test_last_short_batch_is_kept_and_batches_carry_the_transform(coco_dir):
    loader = _build(coco_dir)
    batches = list(loader)
    assert len(loader) == 3 and [b['image_off'].numel() for b in batches] == [2, 2, 1]
    b = batches[0]
    assert set(b) == {'captions', 'image_raw', 'image_off', 'image_hw', 'image_size', 'image_transform'}
    assert b['image_size'] == 16 and b['captions'].shape == (2, 77)
    assert b['image_hw'].tolist() == [[10, 8], [13, 13]]


@pytest.mark.parametrize('kw,want', [(dict(), dict(geometry=1, filter=1, range=1)),
                                     (dict(antialias=True), dict(geometry=1, filter=0, range=1)),
                                     (dict(use_crop=True), dict(geometry=0, filter=0, range=1)),
                                     (dict(use_crop=True, antialias=False), dict(geometry=0, filter=0, range=1))])
def test_use_crop_and_antialias_map_to_the_transform(coco_dir, kw, want):
    assert next(iter(_build(coco_dir, **kw)))['image_transform'] == want


def test_laion_batches_carry_no_transform():
    from diffusion_amd.datasets.image_ingest import collate_raw_images
    batch = collate_raw_images(8)([{'image_u8': torch.zeros(4, 4, 3, dtype=torch.uint8), 'captions': torch.zeros(77)}])
    assert 'image_transform' not in batch


@pytest.mark.parametrize('shuffle', [False, True])
def test_two_ranks_partition_is_disjoint_exhaustive_and_unpadded(coco_dir, shuffle):
    per_rank = []
    for rank in range(2):
        loader = _build(coco_dir, shuffle=shuffle, rank=rank, world=2, seed=3)
        idx = [i for batch in loader.batch_sampler for i in batch]
        assert len(loader) == -(-len(idx) // 2)
        per_rank.append(idx)
    assert sorted(per_rank[0] + per_rank[1]) == list(range(N_SAMPLES))   # odd count: no sample twice, none missing
    assert [len(p) for p in per_rank] == [3, 2]
    if not shuffle:
        assert per_rank == [[0, 2, 4], [1, 3]]


def test_remote_without_local_and_missing_directory_raise(tmp_path):
    from diffusion_amd.datasets import build_streaming_cocoval_dataloader
    for local in (None, ''):
        with pytest.raises(ValueError, match='local'):
            build_streaming_cocoval_dataloader(batch_size=2, remote='s3://bucket/coco', local=local)
    with pytest.raises(FileNotFoundError):
        build_streaming_cocoval_dataloader(batch_size=2, remote='s3://bucket/coco', local=str(tmp_path / 'nowhere'))
    with pytest.raises(FileNotFoundError):
        build_streaming_cocoval_dataloader(batch_size=2, remote=None, local=str(tmp_path / 'nowhere'))
