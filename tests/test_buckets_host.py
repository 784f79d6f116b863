"""Host tests of aspect-ratio bucketing (diffusion_amd/datasets/buckets.py and the three dataloader keys of DESIGN 4.12):
the bucket tables, the assignment, the size scan, the batch sampler for 1, 2 and 3 ranks (constructed with ``(world, rank)``,
no process group), the augmentation draws, and what the dataloader refuses.  No GPU."""
import json
import math

import numpy as np
import pytest
import torch

from bucket_data import BUCKET_KW, ORDER, SHAPES, T5, write_image_mds

T17_HALF = [(256, 832), (256, 896), (256, 960), (256, 1024), (320, 704), (320, 768), (384, 640), (448, 576), (512, 512)]


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    pytest.importorskip('PIL.Image')
    return write_image_mds(str(tmp_path_factory.mktemp('buckets') / 'raw'))


# ---------------------------------------------------------------- tables and assignment
def test_the_three_tables_match_literally():
    from diffusion_amd.datasets.buckets import bucket_table
    assert bucket_table(128, 64, 64, 256) == T5
    t512 = bucket_table(512)
    assert t512 == sorted(set(T17_HALF) | {(w, h) for h, w in T17_HALF}) and len(t512) == 17
    assert len(bucket_table(256)) == 9
    assert bucket_table(128, **BUCKET_KW) == T5


@pytest.mark.parametrize('args', [(256,), (512,), (128, 64, 64, 256), (768, 128), (512, 64, 128, 2048)])
def test_tables_are_closed_under_transposition_bounded_in_area_and_on_the_grid(args):
    from diffusion_amd.datasets.buckets import bucket_table
    R, step = args[0], (args[1] if len(args) > 1 else 64)
    t = bucket_table(*args)
    assert t == sorted(set(t)) and (R, R) in t
    for Rh, Rw in t:
        assert (Rw, Rh) in t and Rh * Rw <= R * R and Rh % step == 0 and Rw % step == 0 and min(Rh, Rw) >= step


def test_table_rejects_steps_the_unet_cannot_take():
    from diffusion_amd.datasets.buckets import bucket_table
    for kw in (dict(step=32), dict(step=96), dict(step=0), dict(step=64, min_side=32), dict(step=64, min_side=512, max_side=256)):
        with pytest.raises(ValueError):
            bucket_table(256, **kw)
    with pytest.raises(ValueError):
        bucket_table(200)


def test_assignment_on_hand_computed_cases():
    from diffusion_amd.datasets.buckets import assign_bucket
    # w / h = 3.5: |log 3.5 - log 4| = 0.134 against |log 3.5 - log 3| = 0.154 -> (64, 256)
    assert T5[assign_bucket(350, 100, T5)] == (64, 256)
    assert T5[assign_bucket(100, 350, T5)] == (256, 64)
    for s in (1, 50, 4000):
        assert T5[assign_bucket(s, s, T5)] == (128, 128)
    assert T5[assign_bucket(300, 100, T5)] == (64, 192) and T5[assign_bucket(100, 300, T5)] == (192, 64)
    # sqrt(3): exactly between square (log ratio 0) and 3:1 (log 3) is not representable; a representable tie: w / h = 1
    # against a table without the square is equally far from (64, 128) and (128, 64) -> equal areas -> the earlier entry;
    # with a larger bucket at the same distance the larger area wins
    assert assign_bucket(77, 77, [(64, 128), (128, 64)]) == 0
    assert assign_bucket(77, 77, [(128, 64), (64, 128)]) == 0
    assert assign_bucket(77, 77, [(64, 128), (256, 128), (128, 64)]) == 1
    assert assign_bucket(77, 77, [(64, 128), (128, 256), (256, 128)]) == 1   # (128, 256) and (256, 128) tie on area too
    # every image goes to the argmin of the stated distance
    rng = np.random.default_rng(0)
    for _ in range(200):
        w, h = (int(v) for v in rng.integers(1, 3000, 2))
        d = [abs(math.log(w / h) - math.log(Rw / Rh)) for Rh, Rw in T5]
        assert d[assign_bucket(w, h, T5)] <= min(d) + 1e-12


# ---------------------------------------------------------------- sampler
def _populations(batch, world):
    """bucket populations that are multiples of batch * world (nothing may be left out) and differ from bucket to bucket"""
    G = batch * world
    return [2 * G, 3 * G, 1 * G, 4 * G]


def _bucket_of_index(pops, seed=1):
    b = np.concatenate([np.full(n, k) for k, n in enumerate(pops)])
    return b[np.random.default_rng(seed).permutation(len(b))]


@pytest.mark.parametrize('world', [1, 2, 3])
def test_sampler_batches_are_single_bucket_aligned_over_ranks_disjoint_and_complete(world):
    from diffusion_amd.datasets.buckets import AspectBucketBatchSampler
    batch = 4
    pops = _populations(batch, world)
    boi = _bucket_of_index(pops)
    per_rank = []
    for r in range(world):
        s = AspectBucketBatchSampler(boi, batch, world, r, seed=3, shuffle=True, drop_last=True)
        s.set_epoch(2)
        per_rank.append(list(s))
        assert len(per_rank[-1]) == len(s) == sum(pops) // (batch * world)
    seen = []
    for step in zip(*per_rank):
        buckets = {int(boi[i]) for b in step for i in b}
        assert len(buckets) == 1                      # one bucket per batch, the same one on every rank
        assert all(len(b) == batch for b in step)
        flat = [i for b in step for i in b]
        assert len(set(flat)) == len(flat)            # the ranks' samples are disjoint
        seen += flat
    assert len(set(seen)) == len(seen)                # no index twice in an epoch
    left_out = len(boi) - len(seen)
    assert left_out <= (batch * world - 1) * len(pops)   # the cap
    assert left_out == 0                              # and with populations that are multiples of batch * world: exactly none


@pytest.mark.parametrize('world', [1, 2, 3])
def test_sampler_remainders_drop_last_and_wrap(world):
    from diffusion_amd.datasets.buckets import AspectBucketBatchSampler
    batch, G = 2, 2 * world
    pops = [G + 1, 2 * G - 1, 1, 3 * G]
    boi = _bucket_of_index(pops, seed=2)
    for drop_last in (True, False):
        ranks = [AspectBucketBatchSampler(boi, batch, world, r, 0, True, drop_last) for r in range(world)]
        out = [list(s) for s in ranks]
        n = sum(p // G if drop_last else -(-p // G) for p in pops)
        assert all(len(o) == n == len(s) for o, s in zip(out, ranks))
        seen = [i for o in out for b in o for i in b]
        for step in zip(*out):
            assert len({int(boi[i]) for b in step for i in b}) == 1 and all(len(b) == batch for b in step)
        if drop_last:
            assert len(set(seen)) == len(seen)
            assert len(boi) - len(seen) == sum(p % G for p in pops) <= (G - 1) * len(pops)
        else:
            assert set(seen) == set(range(len(boi)))   # wrapped inside the bucket: everything is seen, some twice


def test_sampler_is_a_function_of_seed_and_epoch_and_skip_yields_the_tail():
    from diffusion_amd.datasets.buckets import AspectBucketBatchSampler
    boi = _bucket_of_index(_populations(4, 2))

    def run(seed, epoch, skip=0, shuffle=True):
        s = AspectBucketBatchSampler(boi, 4, 2, 1, seed, shuffle, True)
        s.set_epoch(epoch)
        s.skip = skip
        return list(s), s

    a, _ = run(3, 0)
    assert run(3, 0)[0] == a
    assert run(3, 1)[0] != a and run(4, 0)[0] != a
    assert sorted(map(sorted, run(3, 1)[0])) != sorted(map(sorted, a))   # the batches themselves are recomposed, not only reordered
    for k in (0, 1, 5, len(a) - 1, len(a)):
        tail, s = run(3, 0, skip=k)
        assert tail == a[k:]
        assert s.skip == 0 and list(s) == a       # the skip applies to one iterator
    plain, _ = run(3, 0, shuffle=False)
    assert plain == run(9, 5, shuffle=False)[0]
    assert all(b == sorted(b) for b in plain)


# ---------------------------------------------------------------- sizes
def test_scan_image_sizes_from_columns_from_headers_and_from_the_cache(tmp_path, image_dir):
    from diffusion_amd.datasets import buckets as BK
    from diffusion_amd.datasets.mds import write_mds
    want = np.array([(SHAPES[k][1], SHAPES[k][0]) for k in ORDER])
    got = BK.scan_image_sizes(image_dir)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # with width / height columns the recorded values are taken and the bytes are not even parsed
    cols = str(tmp_path / 'cols')
    write_mds(cols, {'jpg': 'bytes', 'caption': 'str', 'width': 'int32', 'height': 'int32'},
              [{'jpg': b'not an image', 'caption': '', 'width': 100 + i, 'height': 7 * i + 1} for i in range(5)])
    assert BK.scan_image_sizes(cols).tolist() == [[100 + i, 7 * i + 1] for i in range(5)]
    # the cache: written by the first scan, read by the second (the header reader is not called again)
    cache = str(tmp_path / 'sizes.json')
    assert np.array_equal(BK.scan_image_sizes(image_dir, cache), want)
    assert json.load(open(cache))['sizes'] == want.tolist()
    real, BK._header_size = BK._header_size, None
    try:
        assert np.array_equal(BK.scan_image_sizes(image_dir, cache), want)
        with pytest.raises(TypeError):
            BK.scan_image_sizes(image_dir)
    finally:
        BK._header_size = real
    assert BK.scan_image_sizes(cols, cache).tolist() == [[100 + i, 7 * i + 1] for i in range(5)]   # another directory's cache is not used


# ---------------------------------------------------------------- dataloader
def _loader(image_dir, **kw):
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader
    args = dict(local=image_dir, batch_size=4, resize_size=128, aspect_buckets=BUCKET_KW, seed=11)
    args.update(kw)
    return build_streaming_laion_dataloader(**args)


def test_bucketed_batches_carry_their_bucket_and_the_fixture_fills_four_buckets(image_dir):
    from diffusion_amd.datasets.buckets import assign_bucket
    dl = _loader(image_dir)
    assert dl.bucket_table == T5
    boi = dl.batch_sampler.bucket_of_index
    assert sorted(np.bincount(boi, minlength=5).tolist()) == [0, 8, 8, 12, 12]
    batches = list(dl)
    assert len(batches) == len(dl) == 10
    for b in batches:
        assert isinstance(b['image_size'], tuple) and b['image_size'] in T5 and 'image_aug' not in b and 'image_target' not in b
        for h, w in b['image_hw'].tolist():
            assert T5[assign_bucket(w, h, T5)] == b['image_size']
    assert len({b['image_size'] for b in batches}) == 4
    # explicit pairs: the same thing with a two-entry table
    dl2 = _loader(image_dir, aspect_buckets=[[128, 128], [64, 256]])
    assert dl2.bucket_table == [(64, 256), (128, 128)] and {b['image_size'] for b in dl2} == {(64, 256), (128, 128)}


def _aug_by_sample(dl, epochs=(0,)):
    """{(epoch, h, w): (top, left, flip)} over whole epochs; the 40 sizes are distinct, so (h, w) names the sample"""
    out = {}
    for e in epochs:
        dl.set_epoch(e)
        for b in dl:
            assert b['image_aug'].dtype == torch.int32 and b['image_aug'].shape == (b['image_hw'].shape[0], 3)
            for (h, w), a in zip(b['image_hw'].tolist(), b['image_aug'].tolist()):
                out[(e, h, w)] = tuple(a)
    return out


def test_augmentation_draws_do_not_depend_on_workers_world_size_or_batch_position(image_dir):
    from torch.utils.data import DataLoader
    from diffusion_amd.datasets.buckets import AspectBucketBatchSampler
    from diffusion_amd.datasets.image_ingest import ingest_geometry
    assert len(set(SHAPES)) == len(SHAPES)
    kw = dict(random_crop=True, flip_prob=0.5, drop_last=False)
    base = _aug_by_sample(_loader(image_dir, **kw), epochs=(0, 1))
    assert len(base) == 80
    assert _aug_by_sample(_loader(image_dir, num_workers=2, **kw), epochs=(0, 1)) == base
    assert _aug_by_sample(_loader(image_dir, batch_size=3, **kw), epochs=(0, 1)) == base
    # other world sizes: the dataset and collate function of the loader under the sampler of rank r of 2 and of 3
    dl = _loader(image_dir, **kw)
    for world in (2, 3):
        got = {}
        for r in range(world):
            s = AspectBucketBatchSampler(dl.batch_sampler.bucket_of_index, 4, world, r, 11, True, False)
            for b in DataLoader(dl.dataset, batch_sampler=s, collate_fn=dl.collate_fn):
                for (h, w), a in zip(b['image_hw'].tolist(), b['image_aug'].tolist()):
                    got[(0, h, w)] = tuple(a)
        assert got == {k: v for k, v in base.items() if k[0] == 0}
    # in range, not constant, different in the next epoch, and flips near one half
    e0 = {k[1:]: v for k, v in base.items() if k[0] == 0}
    e1 = {k[1:]: v for k, v in base.items() if k[0] == 1}
    assert e0 != e1
    boi ={(SHAPES[k][0], SHAPES[k][1]): T5[int(b)] for k, b in zip(ORDER, dl.batch_sampler.bucket_of_index)}
    moved = 0
    for (h, w), (top, left, flip) in e0.items():
        Rh, Rw = boi[(h, w)]
        nw, nh, ctop, cleft = ingest_geometry(w, h, (Rh, Rw))
        assert 0 <= top <= nh - Rh and 0 <= left <= nw - Rw and flip in (0, 1)
        moved += (top, left) != (ctop, cleft)
    assert moved >= 10 and 8 <= sum(v[2] for v in e0.values()) <= 32
    # each switch alone; without buckets the one target is resize_size
    only_flip = _aug_by_sample(_loader(image_dir, flip_prob=1.0, drop_last=False))
    for (_, h, w), (top, left, flip) in only_flip.items():
        assert (top, left, flip) == (*ingest_geometry(w, h, boi[(h, w)])[2:], 1)
    only_crop = _aug_by_sample(_loader(image_dir, random_crop=True, drop_last=False))
    assert {k: v[:2] for k, v in only_crop.items()} == {k: v[:2] for k, v in base.items() if k[0] == 0}
    assert not any(v[2] for v in only_crop.values())
    plain = _loader(image_dir, aspect_buckets=None, random_crop=True, flip_prob=0.5, resize_size=32, drop_last=False)
    for b in plain:
        assert b['image_size'] == 32
        for (h, w), (top, left, flip) in zip(b['image_hw'].tolist(), b['image_aug'].tolist()):
            nw, nh, _, _ = ingest_geometry(w, h, 32)
            assert 0 <= top <= nh - 32 and 0 <= left <= nw - 32 and flip in (0, 1)


def test_a_loader_resumed_mid_epoch_yields_the_rest_of_the_epoch_with_its_captions_and_draws(image_dir):
    """what a checkpoint restores is the global RNG state and the position (epoch, batches done).  A fresh loader given both
    continues the uninterrupted one: same samples, same crop / flip draws, and the same caption drops - those come from the
    global stream, which making the new iterator must therefore leave alone"""
    kw = dict(random_crop=True, flip_prob=0.5, caption_drop_prob=0.5)

    def rows(b):
        return (b['image_size'], b['image_hw'].tolist(), b['image_aug'].tolist(), b['captions'].tolist())

    torch.manual_seed(5)
    it = iter(_loader(image_dir, **kw))
    full, state = [], None
    for k in range(10):
        if k == 3:
            state = torch.get_rng_state()
        full.append(rows(next(it)))
    assert len({tuple(map(tuple, r[3])) for r in full}) > 1   # captions do get dropped
    torch.manual_seed(999)
    dl = _loader(image_dir, **kw)
    torch.set_rng_state(state)
    dl.set_epoch(0, skip_batches=3)
    assert [rows(b) for b in dl] == full[3:]


def test_without_the_new_keys_the_batches_are_what_they_were(image_dir):
    """``aspect_buckets=None`` (the default): the seeded single-shape run as it was before the keys existed - the
    permutation of ``EpochRandomSampler`` (``randperm`` under ``manual_seed(seed + epoch)``) cut into batches in order, the
    int ``image_size``, and no ``image_aug``"""
    from diffusion_amd.datasets.laion.laion import (EpochRandomSampler, ResumableBatchSampler,
                                                   build_streaming_laion_dataloader)
    for kw in (dict(), dict(aspect_buckets=None, random_crop=False, flip_prob=0.0)):
        dl = build_streaming_laion_dataloader(local=image_dir, batch_size=4, resize_size=32, seed=11, **kw)
        assert type(dl.batch_sampler) is ResumableBatchSampler and type(dl.batch_sampler.sampler) is EpochRandomSampler
        assert type(dl.dataset).__name__ == 'ConcatDataset'
        for epoch in (0, 1):
            perm = torch.randperm(40, generator=torch.Generator().manual_seed(11 + epoch)).tolist()
            batches = list(dl)
            assert len(batches) == 10
            for k, b in enumerate(batches):
                assert b['image_size'] == 32 and 'image_aug' not in b
                assert set(b) == {'captions', 'image_raw', 'image_off', 'image_hw', 'image_size'}
                assert b['image_hw'].tolist() == [list(SHAPES[ORDER[i]]) for i in perm[4 * k:4 * k + 4]]


def test_everything_the_dataloader_refuses_is_a_value_error_before_anything_is_read(tmp_path, image_dir):
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader as build
    from diffusion_amd.datasets.mds import write_mds
    lat = {'caption': 'x', 'caption_latents': np.zeros(77 * 8, np.float16).tobytes(),
           'latents_128': np.zeros(4 * 16 * 16, np.float16).tobytes()}
    lat_dir = str(tmp_path / 'lat')
    write_mds(lat_dir, {'caption': 'str', 'caption_latents': 'bytes', 'latents_128': 'bytes'}, [dict(lat) for _ in range(4)])
    npz_dir = tmp_path / 'npz'
    npz_dir.mkdir()
    np.savez(str(npz_dir / 's0.npz'), caption_latents=np.zeros((2, 77 * 8), np.float16), latents_128=np.zeros((2, 1024), np.float16))
    bad = [dict(),                                                        # synthetic data
           dict(local=str(npz_dir)),                                      # .npz shards
           dict(local=image_dir, resize_size=[64, 128]),                  # a rectangular resize_size
           dict(local=image_dir, aspect_buckets=dict(step=32)),           # a step the U-Net cannot take
           dict(local=image_dir, aspect_buckets=dict(step=96)),
           dict(local=image_dir, aspect_buckets=dict(stride=64)),         # an unknown key
           dict(local=image_dir, aspect_buckets=[[64, 100]]),             # an explicit pair off the grid
           dict(local=image_dir, aspect_buckets=[]),
           dict(local=image_dir, aspect_buckets='yes')]
    for kw in bad:
        args = dict(batch_size=2, resize_size=128, aspect_buckets=True)
        args.update(kw)
        with pytest.raises(ValueError):
            build(**args)
    # augmentation needs raw images
    for kw in (dict(local=lat_dir, random_crop=True), dict(local=lat_dir, flip_prob=0.5), dict(flip_prob=0.5), dict(random_crop=True),
               dict(local=str(npz_dir), flip_prob=0.5), dict(local=image_dir, flip_prob=1.5), dict(local=image_dir, flip_prob=-0.1)):
        with pytest.raises(ValueError):
            build(batch_size=2, resize_size=128, **kw)
    # a latent directory without the bucketed columns names the tool flag
    with pytest.raises(ValueError, match='--aspect-buckets 128'):
        build(local=lat_dir, batch_size=2, resize_size=128, aspect_buckets=True)
    # and with them it is read: the shapes of the `_hw` column are the table
    ar_dir = str(tmp_path / 'ar')
    shapes = [(64, 256), (128, 128), (64, 256), (128, 128), (192, 64), (192, 64)]
    write_mds(ar_dir, {'caption': 'str', 'caption_latents': 'bytes', 'latents_128': 'bytes', 'latents_ar128': 'bytes',
                       'latents_ar128_hw': 'bytes'},
              [dict(lat, latents_ar128=np.full(4 * (h // 8) * (w // 8), i, np.float16).tobytes(),
                    latents_ar128_hw=np.array([h, w], np.int32).tobytes()) for i, (h, w) in enumerate(shapes)])
    dl = build(local=ar_dir, batch_size=2, resize_size=128, aspect_buckets=True, seed=1)
    assert dl.bucket_table == [(64, 256), (128, 128), (192, 64)]
    got = sorted((tuple(b['image_latents'].shape), sorted(b['image_latents'][:, 0, 0, 0].tolist())) for b in dl)
    assert got == [((2, 4, 8, 32), [0.0, 2.0]), ((2, 4, 16, 16), [1.0, 3.0]), ((2, 4, 24, 8), [4.0, 5.0])]
    assert len(dl) == 3 and next(iter(build(local=ar_dir, batch_size=2, resize_size=128)))['image_latents'].shape == (2, 4, 16, 16)
