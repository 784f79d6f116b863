"""Aspect-ratio bucketing, the host half: the table of target shapes, the assignment of an image to one of them, a scan of
the image sizes of an MDS directory, the batch sampler that keeps every batch inside one bucket, and the per-sample
random-crop / flip draws that ``ops.image_ingest_aug`` executes.  Nothing here touches the device.

A bucket is an ``(Rh, Rw)`` pair (rows x columns, pixels) of about ``R * R`` pixels whose sides are multiples of ``step``.
Every batch of a bucketed run holds images of ONE bucket, so a training step still sees one rectangular shape (DESIGN
4.12); the shape changes from step to step."""
from __future__ import annotations

import io
import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

UNET_STEP = 64   # SD-2: VAE factor 8 x the U-Net's 2 ** (levels - 1) = 8 (UNetHIP.check_spatial on the latent)


def bucket_table(R: int, step: int = 64, min_side: Optional[int] = None, max_side: Optional[int] = None,
                 unet_step: int = UNET_STEP) -> List[Tuple[int, int]]:
    """The sorted ``(Rh, Rw)`` buckets of resolution ``R``: for every width ``w`` in ``range(min_side, max_side + 1, step)``
    the largest height ``h <= max_side`` that is a multiple of ``step`` with ``h * w <= R * R``, both ways round, plus the
    square.  ``min_side`` defaults to ``R // 2`` and ``max_side`` to ``2 * R``.  ``step`` must be a positive multiple of
    ``unet_step`` (the pixel granularity the U-Net accepts: 64 for SD-2), and so must ``R``, or a bucket could not be
    trained on."""
    R, step = int(R), int(step)
    min_side = R // 2 if min_side is None else int(min_side)
    max_side = 2 * R if max_side is None else int(max_side)
    if step < 1 or step % int(unet_step):
        raise ValueError(f'bucket_table: step {step} must be a positive multiple of {unet_step} px (the U-Net needs latent '
                         f'sides that are multiples of {unet_step // 8})')
    if R < step or R % step:
        raise ValueError(f'bucket_table: R = {R} must be a positive multiple of step = {step}')
    if min_side < step or min_side % step or max_side < min_side:
        raise ValueError(f'bucket_table: min_side {min_side} must be a positive multiple of step {step} and <= max_side '
                         f'{max_side}')
    out = {(R, R)}
    for w in range(min_side, max_side + 1, step):
        h = min(max_side, (R * R // w) // step * step)
        if h >= min_side:
            out.add((h, w))
            out.add((w, h))
    return sorted(out)


def assign_bucket(w: int, h: int, table: Sequence[Tuple[int, int]]) -> int:
    """Index into ``table`` of the bucket for a ``w x h`` image: the one whose aspect ratio is closest in log space,
    ``|log(w / h) - log(Rw / Rh)|`` minimal; ties go to the larger area, then to the earlier entry."""
    if w < 1 or h < 1 or not len(table):
        raise ValueError(f'assign_bucket: a positive size and a non-empty table are needed, got {(w, h)}')
    a = math.log(w) - math.log(h)
    best, best_key = 0, None
    for i, (Rh, Rw) in enumerate(table):
        d = abs(a - (math.log(Rw) - math.log(Rh)))
        # distances of exact ties (w/h = 1 against (64, 128) and (128, 64)) differ by rounding at most: compare with a margin
        key = (d, -Rh * Rw)
        if best_key is None or key[0] < best_key[0] - 1e-12 or (abs(key[0] - best_key[0]) <= 1e-12 and key[1] < best_key[1]):
            best, best_key = i, key
    return best


def resolve_table(aspect_buckets, resize_size) -> List[Tuple[int, int]]:
    """``build_streaming_laion_dataloader``'s ``aspect_buckets`` -> the table.  ``True``: ``bucket_table(resize_size)``; a
    dict: its ``step`` / ``min_side`` / ``max_side``; a list: explicit ``[Rh, Rw]`` pairs, each side a multiple of 64."""
    if hasattr(resize_size, '__len__'):
        raise ValueError(f'aspect_buckets needs an int resize_size (the buckets are derived from it), got {list(resize_size)}')
    R = int(resize_size)
    if aspect_buckets is True:
        return bucket_table(R)
    if isinstance(aspect_buckets, dict) or hasattr(aspect_buckets, 'keys'):
        extra = set(aspect_buckets.keys()) - {'step', 'min_side', 'max_side'}
        if extra:
            raise ValueError(f'aspect_buckets: unknown keys {sorted(extra)} (step, min_side, max_side)')
        return bucket_table(R, **{k: int(v) for k, v in aspect_buckets.items()})
    if isinstance(aspect_buckets, (list, tuple)) or hasattr(aspect_buckets, '__len__'):
        if not len(aspect_buckets) or any(not hasattr(p, '__len__') or len(p) != 2 for p in aspect_buckets):
            raise ValueError(f'aspect_buckets: a non-empty list of [Rh, Rw] pairs is expected, got {aspect_buckets!r}')
        table = sorted({(int(p[0]), int(p[1])) for p in aspect_buckets})
        bad = [p for p in table if min(p) < UNET_STEP or p[0] % UNET_STEP or p[1] % UNET_STEP]
        if bad:
            raise ValueError(f'aspect_buckets: sides must be positive multiples of {UNET_STEP} px, got {bad}')
        return table
    raise ValueError(f'aspect_buckets: None, True, a dict or a list of [Rh, Rw] pairs, got {aspect_buckets!r}')


def _header_size(data: bytes) -> Tuple[int, int]:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:   # lazy: the header is parsed, no pixel is decoded
        return int(img.width), int(img.height)


def scan_image_sizes(directory: str, cache: Optional[str] = None) -> np.ndarray:
    """``int64 [N, 2]`` of ``(w, h)`` per sample of an MDS directory, without decoding pixels: from the ``width`` /
    ``height`` columns when every shard has both, else from the header of the ``jpg`` bytes (Pillow reads it lazily).
    ``cache``: a ``.json`` path; a cache written for the same shard list is returned instead of scanning, otherwise the
    scan is stored there.  A wrong recorded size only costs a worse bucket: the ingest reads the true size."""
    from .mds import MDSDirectory
    with open(os.path.join(directory, 'index.json')) as f:
        shards = json.load(f)['shards']
    stamp = [[s['raw_data']['basename'], int(s['samples'])] for s in shards]
    if cache and os.path.exists(cache):
        with open(cache) as f:
            c = json.load(f)
        if c.get('shards') == stamp:
            return np.asarray(c['sizes'], dtype=np.int64).reshape(-1, 2)
    mds = MDSDirectory(directory)
    cols = all('width' in s['column_names'] and 'height' in s['column_names'] for s in shards) and bool(shards)
    sizes = np.zeros((len(mds), 2), dtype=np.int64)
    for i in range(len(mds)):
        if cols:
            smp = mds.get(i, columns=('width', 'height'))
            sizes[i] = int(smp['width']), int(smp['height'])
        else:
            sizes[i] = _header_size(mds.get(i, columns=('jpg',))['jpg'])
    if cache:
        with open(cache, 'w') as f:
            json.dump({'shards': stamp, 'sizes': sizes.tolist()}, f)
    return sizes


def _seed(*parts: int) -> int:
    """one 63-bit generator seed from a tuple of integers (splitmix64 over the parts): the streams of (seed, epoch, bucket),
    (seed, epoch) and (seed, epoch, index) never coincide by accident the way sums of the parts would"""
    x = 0x9E3779B97F4A7C15
    for p in parts:
        x = (x ^ (int(p) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
        x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 31
    return x >> 1


class AspectBucketBatchSampler(torch.utils.data.Sampler):
    """Batch sampler whose every batch lies inside one bucket, identical in shape over the ranks of a data-parallel job.

    Per epoch each bucket's members are permuted by a generator seeded with ``(seed, epoch, bucket)`` (kept in index order
    without ``shuffle``) and cut into GLOBAL batches of ``batch_size * world``; ``drop_last`` drops a bucket's remainder,
    otherwise it is filled by wrapping round inside the bucket.  The list of global batches is shuffled with
    ``(seed, epoch)``, and rank ``r`` yields slice ``r`` of each: all ranks train the same shape at the same step on
    disjoint samples.  ``skip`` drops the first batches of the next iterator at index level (``ResumableBatchSampler``'s
    contract, used by ``EpochDataLoader.set_epoch(e, skip_batches=k)``)."""

    def __init__(self, bucket_of_index, batch_size: int, world: int = 1, rank: int = 0, seed: int = 0, shuffle: bool = True,
                 drop_last: bool = True):
        self.bucket_of_index = np.asarray(bucket_of_index, dtype=np.int64).reshape(-1)
        self.batch_size, self.world, self.rank = int(batch_size), int(world), int(rank)
        if self.batch_size < 1 or self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f'AspectBucketBatchSampler: batch_size {batch_size}, world {world}, rank {rank}')
        self.seed, self.shuffle, self.drop_last = int(seed), bool(shuffle), bool(drop_last)
        self.epoch = 0
        self.skip = 0
        self.sampler = self   # EpochDataLoader tells `batch_sampler.sampler` the epoch
        self._members: Dict[int, np.ndarray] = {int(b): np.nonzero(self.bucket_of_index == b)[0]
                                                for b in np.unique(self.bucket_of_index)}

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def global_batches(self, epoch: Optional[int] = None) -> List[Tuple[int, List[int]]]:
        """``[(bucket, indices of one global batch)]`` of an epoch, in the order they are trained"""
        epoch = self.epoch if epoch is None else int(epoch)
        G = self.batch_size * self.world
        out = []
        for b in sorted(self._members):
            idx = self._members[b]
            if self.shuffle:
                g = torch.Generator().manual_seed(_seed(self.seed, epoch, b))
                idx = idx[torch.randperm(len(idx), generator=g).numpy()]
            full = len(idx) // G
            for k in range(full):
                out.append((b, idx[k * G:(k + 1) * G].tolist()))
            rest = len(idx) - full * G
            if rest and not self.drop_last:
                tail = np.concatenate([idx[full * G:], np.resize(idx, G - rest)])   # wrap round inside the bucket
                out.append((b, tail.tolist()))
        if self.shuffle:
            g = torch.Generator().manual_seed(_seed(self.seed, epoch))
            out = [out[i] for i in torch.randperm(len(out), generator=g).tolist()]
        return out

    def __iter__(self):
        skip, self.skip = self.skip, 0
        r, n = self.rank, self.batch_size
        for _, idx in self.global_batches()[skip:]:
            yield idx[r * n:(r + 1) * n]

    def __len__(self):
        G = self.batch_size * self.world
        return sum(len(m) // G if self.drop_last else -(-len(m) // G) for m in self._members.values())


def draw_aug(seed: int, epoch: int, index: int, w: int, h: int, target, random_crop: bool, flip_prob: float):
    """The ``(top, left, flip)`` of sample ``index`` in ``epoch``: a function of ``(seed, epoch, index)`` and the decoded
    size alone - not of the worker that decodes it, its place in the batch or the world size.  Origins are uniform over
    ``[0, n - R]`` per axis of the resized image (``ingest_geometry``); without ``random_crop`` they are the centre crop's."""
    from .image_ingest import ingest_geometry
    nw, nh, top, left = ingest_geometry(int(w), int(h), target)
    Rh, Rw = target if hasattr(target, '__len__') else (target, target)
    g = torch.Generator().manual_seed(_seed(seed, epoch, index))
    u = torch.rand(3, generator=g, dtype=torch.float64).tolist()   # always three draws: each switch leaves the others' alone
    if random_crop:
        top = min(int(u[0] * (nh - Rh + 1)), nh - Rh)
        left = min(int(u[1] * (nw - Rw + 1)), nw - Rw)
    return top, left, int(u[2] < float(flip_prob))


class BucketedImages(torch.utils.data.Dataset):
    """Wraps the raw-image dataset of a dataloader: tells the collate function each sample's target shape
    (``image_target``: its bucket, or the one target of an unbucketed run) and, with augmentation on, its ``image_aug``
    draw (``draw_aug`` on the GLOBAL index and the epoch ``EpochDataLoader`` sets before it makes an iterator)."""

    def __init__(self, dataset, targets, table=None, seed: int = 0, random_crop: bool = False, flip_prob: float = 0.0):
        self.dataset, self.table = dataset, table
        self.targets = targets   # int64 [N] bucket indices into `table`, or the single target (int or pair)
        self.seed, self.random_crop, self.flip_prob = int(seed), bool(random_crop), float(flip_prob)
        self.augment = self.random_crop or self.flip_prob > 0.0
        self.epoch = 0

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.dataset)

    def target_of(self, index: int):
        return self.table[int(self.targets[index])] if self.table is not None else self.targets

    def __getitem__(self, index):
        smp = self.dataset[index]
        target = self.target_of(index)
        if self.table is not None:
            smp['image_target'] = torch.tensor(target, dtype=torch.int32)
        if self.augment:
            h, w = smp['image_u8'].shape[:2]
            smp['image_aug'] = torch.tensor(draw_aug(self.seed, self.epoch, index, w, h, target, self.random_crop,
                                                     self.flip_prob), dtype=torch.int32)
        return smp
